"""Learned D-AMP (the L-DAMP baseline of Fig. 5c) on the HIP library: counterpart of the reference's ``aux_models.LDAMP``
(``src/score_based_channels/aux_models.py:62-190``) with ``aux_unet.FlippedNormUnet`` denoisers, inference only.

Supported is the configuration ``train_ldamp.py:41-47`` trains: ``backbone='FlippedUNet'``, ``shared_nets=False``, one U-Net
(``chans=16``, ``num_pools=3``) per unroll, Nt x Nr = 64 x 16.  Other settings raise ``ValueError`` on the host.

torch only owns the device memory and the stream; every number is computed by the HIP kernels (``csrc/ldamp.hip`` behind
``sbc_ldamp_*`` of ``include/sbc_hip.h``).  ``state_dict_spec`` / ``seeded_state_dict`` need neither torch nor the library.
"""
import ctypes as C
import zlib

import numpy as np

from . import _lib

NT, NR = 64, 16
CHANS, NUM_POOLS = 16, 3
BACKBONE = 'FlippedUNet'
# sbc_ldamp_stage ids (include/sbc_hip.h)
STAGES = ('r', 'x', 'd0a', 'd0', 'p0', 'd1a', 'd1', 'p1', 'd2a', 'd2', 'p2', 'ba', 'bb',
          't0', 'u0a', 'u0', 't1', 'u1a', 'u1', 't2', 'u2a', 'u2', 'stat')


def unet_spec(chans=CHANS, num_pools=NUM_POOLS, in_chans=2, out_chans=2):
    """Ordered ``[(name, shape)]`` of one ``FlippedNormUnet``'s ``state_dict`` (module registration order of ``aux_unet.Unet``:
    down path, bottleneck, up convolutions, transposed convolutions; InstanceNorm2d has no tensors)."""
    def block(prefix, cin, cout):
        return [(prefix + '.layers.0.weight', (cout, cin, 3, 3)), (prefix + '.layers.4.weight', (cout, cout, 3, 3))]
    t, ch = block('unet.down_sample_layers.0', in_chans, chans), chans
    for i in range(1, num_pools):
        t += block('unet.down_sample_layers.%d' % i, ch, 2 * ch)
        ch *= 2
    t += block('unet.conv', ch, 2 * ch)
    up, tr = [], []
    for i in range(num_pools):
        tr.append(('unet.up_transpose_conv.%d.layers.0.weight' % i, (2 * ch, ch, 2, 2)))
        up += block('unet.up_conv.%d' % i if i < num_pools - 1 else 'unet.up_conv.%d.0' % i, 2 * ch, ch)
        if i < num_pools - 1:
            ch //= 2
    up += [('unet.up_conv.%d.1.weight' % (num_pools - 1), (out_chans, ch, 1, 1)), ('unet.up_conv.%d.1.bias' % (num_pools - 1), (out_chans,))]
    return t + up + tr


def state_dict_spec(max_unrolls=10):
    """Ordered ``[(name, shape)]`` of the reference ``LDAMP.state_dict()``: ``update_nets.<u>.`` + ``unet_spec()``, 19 tensors per net."""
    return [('update_nets.%d.%s' % (u, n), s) for u in range(int(max_unrolls)) for n, s in unet_spec()]


def seeded_state_dict(seed, max_unrolls=10):
    """Deterministic stand-in for trained weights: every tensor uniform within +-1/sqrt(fan_in) (fan_in = shape[1] x kernel area; the
    bias takes its weight's), drawn from a numpy ``PCG64`` generator keyed by ``(seed, crc32(name))`` -- a tensor's values depend on
    the seed and its own name only."""
    sd = {}
    for name, shape in state_dict_spec(max_unrolls):
        rng = np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(name.encode())]))
        wshape = sd[name[:-4] + 'weight'].shape if name.endswith('.bias') else shape
        b = 1.0 / np.sqrt(float(np.prod(wshape[1:])))
        sd[name] = rng.uniform(-b, b, size=shape).astype(np.float32)
    return sd


def check_hparams(hparams):
    """Host-side refusal of what the kernels do not cover; returns ``max_unrolls``."""
    def get(key, default):
        v = hparams.get(key, default) if isinstance(hparams, dict) else getattr(hparams, key, default)
        return default if (v is None or (isinstance(v, dict) and not v)) else v
    backbone, shared = get('backbone', BACKBONE), get('shared_nets', False)
    if backbone != BACKBONE:
        raise ValueError('backbone=%r is not supported: only %r (DnCNN and UNet are out of scope)' % (backbone, BACKBONE))
    if shared:
        raise ValueError('shared_nets=%r is not supported: one net per unroll (shared_nets=False) only' % (shared,))
    in_channels = int(get('in_channels', 2))
    if in_channels != 2:
        raise ValueError('in_channels=%r is not supported: the denoisers take (re, im) = 2 channels' % (in_channels,))
    max_unrolls = int(get('max_unrolls', 10))
    if not 1 <= max_unrolls <= 64:
        raise ValueError('max_unrolls must be in [1, 64] (got %r)' % (max_unrolls,))
    return max_unrolls


def check_state_dict(sd, max_unrolls):
    """Raise ``KeyError`` / ``ValueError`` like ``load_state_dict(strict=True)`` would."""
    _lib.check_against_spec(sd, state_dict_spec(max_unrolls))


def check_run_args(Y_shape, P_shape, eig_shape, num_unrolls, max_unrolls, directions_shape=None):
    """Host-side checks of a run that need no data."""
    if len(Y_shape) != 3 or len(P_shape) != 3:
        raise ValueError('Y_herm must be [B, Np, Nr] and P_herm [B, Np, Nt] (got %s, %s)' % (tuple(Y_shape), tuple(P_shape)))
    B, Np, Nr = Y_shape
    if (P_shape[2], Nr) != (NT, NR):
        raise ValueError('geometry Nt x Nr = %d x %d is not supported: only %d x %d' % (P_shape[2], Nr, NT, NR))
    if P_shape[0] != B or P_shape[1] != Np or not 1 <= Np <= NT:
        raise ValueError('need P_herm [B, Np, %d] with Y_herm\'s B and Np, 1 <= Np <= %d (got Y %s, P %s)' % (NT, NT, tuple(Y_shape), tuple(P_shape)))
    if tuple(eig_shape) != (B,):
        raise ValueError('eig1 must have shape (%d,) (got %s)' % (B, tuple(eig_shape)))
    if not 1 <= int(num_unrolls) <= max_unrolls:
        raise ValueError('num_unrolls must be in [1, %d] (got %r)' % (max_unrolls, num_unrolls))
    if directions_shape is not None and tuple(directions_shape) != (int(num_unrolls), B, NT, NR, 2):
        raise ValueError('directions must be [%d, %d, %d, %d, 2] (got %s)' % (int(num_unrolls), B, NT, NR, tuple(directions_shape)))


def replay_directions(seed, sample_ids, num_unrolls):
    """The directions a run without ``directions=`` draws on the device, float32 ``[num_unrolls, B, 64, 16, 2]`` on the host
    (``sbc_debug_ldamp_directions``: written by the kernel the run itself launches)."""
    ids = [int(i) for i in sample_ids]
    out = np.empty((int(num_unrolls), len(ids), NT, NR, 2), np.float32)
    buf = np.empty((NT, NR, 2), np.float32)
    for u in range(int(num_unrolls)):
        for j, i in enumerate(ids):
            _lib.check(_lib.lib().sbc_debug_ldamp_directions(C.c_uint64(int(seed)), C.c_int64(i), u, buf.ctypes.data_as(C.c_void_p)))
            out[u, j] = buf
    return out


def stage_layout(stage, n_images):
    """``(offset, (n_images, C, H, W))`` of a stage in a call's workspace (``sbc_ldamp_stage``); ``stage``: a name of ``STAGES`` or an id."""
    sid = STAGES.index(stage) if isinstance(stage, str) else int(stage)
    off, c, h, w = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().sbc_ldamp_stage(sid, int(n_images), C.byref(off), C.byref(c), C.byref(h), C.byref(w)))
    return off.value, (int(n_images), c.value, h.value, w.value)


class LDAMP(_lib.DeviceHandle):
    """``LDAMP(hparams)`` / ``load_state_dict`` / ``eval`` / ``__call__(sample, num_unrolls)`` as the reference module; additions:
    ``directions=`` (float32 ``[num_unrolls, B, 64, 16, 2]``: the random directions instead of device draws), ``seed=`` and
    ``sample_ids=`` (key of the device draws: direction of sample ``b`` at unroll ``u`` = Philox stream ``(seed, sample_ids[b], u)``,
    default ids ``0 .. B-1``), ``return_logs=`` (also return a dict of per-unroll ``h``, ``z``, ``div``, ``eps``) and ``H=`` (the true
    channels: the per-sample NMSE is added to the logs as ``nmse``)."""

    _destroy = 'sbc_ldamp_destroy'

    def __init__(self, hparams, device=None):
        super().__init__(device)
        self.max_unrolls = check_hparams(hparams)

    def load_state_dict(self, model_state):
        sd = _lib.numpy_state_dict(model_state)
        check_state_dict(sd, self.max_unrolls)
        return self._load(sd, [n for n, _ in state_dict_spec(self.max_unrolls)],
                          lambda refs, n, out: _lib.lib().sbc_ldamp_create(refs, n, self.max_unrolls, out))

    def _workspace(self, B, unrolls, dev):
        return self._workspace_of(_lib.lib().sbc_ldamp_workspace_floats(int(B), int(unrolls)), dev)

    def denoise(self, net, r, stream=None):
        """``D_net(r)`` for complex64 ``r`` ``[B, 64, 16]`` -> complex64 ``[B, 64, 16]`` (one evaluation; asynchronous)."""
        import torch
        self._need_weights()
        if not isinstance(r, torch.Tensor) or r.dtype != torch.complex64 or r.dim() != 3 or tuple(r.shape[1:]) != (NT, NR):
            raise ValueError('r must be a complex64 tensor [B, %d, %d] (got %s %s)' % (NT, NR, getattr(r, 'dtype', type(r)), tuple(getattr(r, 'shape', ()))))
        if not 0 <= int(net) < self.max_unrolls:
            raise ValueError('net must be in [0, %d) (got %r)' % (self.max_unrolls, net))
        dev = self._torch_device()
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):           # whatever torch has to copy or convert is ordered on the same stream
            r = r.to(dev).resolve_conj().contiguous()
        B = r.shape[0]
        out = torch.empty_like(r)
        if B == 0:                                       # an empty tensor has no address to hand to the library
            return out
        with torch.cuda.device(dev):
            ws = self._workspace(B, 0, dev)
            _lib.check(_lib.lib().sbc_ldamp_denoise(self._h, int(net), C.c_void_p(r.data_ptr()), C.c_void_p(out.data_ptr()), B,
                                                    C.c_void_p(ws.data_ptr()), C.c_void_p(s.cuda_stream)))
            r.record_stream(s)
            ws.record_stream(s)
        self.last_workspace = (ws, B)
        return out

    def stage(self, name):
        """A stage tensor ``[n_images, C, H, W]`` of the last call, a view of its workspace (``'r'``: interleaved ``[n_images, 64, 16, 2]``;
        ``'stat'``: ``[n_images, 4]``)."""
        ws, n = self.last_workspace
        off, shape = stage_layout(name, n)
        t = ws[off:off + int(np.prod(shape))]
        return t.view(n, NT, NR, 2) if name == 'r' else t.view(n, 4) if name == 'stat' else t.view(*shape)

    def __call__(self, sample, num_unrolls, directions=None, seed=0, sample_ids=None, return_logs=False, H=None, stream=None):
        import torch
        self._need_weights()
        Y, P, eig = sample['Y_herm'], sample['P_herm'], sample['eig1']
        for name, t in (('Y_herm', Y), ('P_herm', P)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.complex64:
                raise ValueError('%s must be a complex64 tensor (got %s)' % (name, getattr(t, 'dtype', type(t))))
        if not isinstance(eig, torch.Tensor):
            raise ValueError('eig1 must be a tensor (got %s)' % type(eig))
        if directions is not None and not isinstance(directions, torch.Tensor):
            directions = torch.from_numpy(np.ascontiguousarray(directions, dtype=np.float32))
        check_run_args(tuple(Y.shape), tuple(P.shape), tuple(eig.shape), num_unrolls, self.max_unrolls,
                       None if directions is None else tuple(directions.shape))
        B, Np, U = Y.shape[0], Y.shape[1], int(num_unrolls)
        sample0 = 0
        if sample_ids is not None:
            ids = np.asarray(sample_ids.cpu().numpy() if isinstance(sample_ids, torch.Tensor) else sample_ids).astype(np.int64)
            if ids.shape != (B,) or (B and not np.array_equal(ids, ids[0] + np.arange(B))):
                raise ValueError('sample_ids must be %d consecutive integers (got %s)' % (B, ids))
            sample0 = int(ids[0]) if B else 0
        if H is not None and (not isinstance(H, torch.Tensor) or H.dtype != torch.complex64 or tuple(H.shape) != (B, NT, NR)):
            raise ValueError('H must be a complex64 tensor [%d, %d, %d]' % (B, NT, NR))
        dev = self._torch_device()
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):           # whatever torch has to copy or convert is ordered on the same stream
            Y, P = Y.to(dev).resolve_conj().contiguous(), P.to(dev).resolve_conj().contiguous()
            eig = eig.to(dev, torch.float32).contiguous()
            if directions is not None:
                directions = directions.to(dev, torch.float32).contiguous()
            if H is not None:
                H = H.to(dev).resolve_conj().contiguous()
        H_hat = torch.empty((B, NT, NR), dtype=torch.complex64, device=dev)
        logs = {}
        if return_logs:
            logs = {'h': torch.empty((U, B, NT, NR), dtype=torch.complex64, device=dev),
                    'z': torch.empty((U, B, Np, NR), dtype=torch.complex64, device=dev),
                    'div': torch.empty((U, B), dtype=torch.float32, device=dev),
                    'eps': torch.empty((U, B), dtype=torch.float32, device=dev)}
        nmse = torch.empty((B,), dtype=torch.float32, device=dev) if H is not None else None
        if nmse is not None:
            logs['nmse'] = nmse
        if B == 0:                                       # an empty tensor has no address to hand to the library
            return (H_hat, logs) if (return_logs or H is not None) else H_hat
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None           # noqa: E731
        with torch.cuda.device(dev):
            ws = self._workspace(B, U, dev)
            d = _lib.sbc_ldamp_run_desc(Y_herm=ptr(Y), P_herm=ptr(P), eig1=ptr(eig), directions=ptr(directions), Htrue=ptr(H),
                                        H_hat=ptr(H_hat), nmse=ptr(nmse), h_log=ptr(logs.get('h')), z_log=ptr(logs.get('z')),
                                        div_log=ptr(logs.get('div')), eps_log=ptr(logs.get('eps')), workspace=ptr(ws),
                                        seed=int(seed) & (2 ** 64 - 1), sample0=sample0, B=B, Np=Np, Nt=NT, Nr=NR, num_unrolls=U)
            _lib.check(_lib.lib().sbc_ldamp_run(self._h, C.byref(d), C.c_void_p(s.cuda_stream)))
            for t in (Y, P, eig, directions, H, ws):
                if t is not None:
                    t.record_stream(s)
        self.last_workspace = (ws, 2 * B)
        return (H_hat, logs) if (return_logs or H is not None) else H_hat
