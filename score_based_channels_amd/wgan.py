"""WGAN latent optimisation (the WGAN baseline of Fig. 5c) on the HIP library: counterpart of the reference's generator
``aux_gan.DCGAN_G_Ours`` (``src/score_based_channels/aux_gan.py:58-112``) in eval mode and of the optimisation loop of
``test_wgan.py:129-176`` (Adam on the latents against ``||G(z) P - Y||^2 + lambda ||z||^2``).

Supported is the one geometry the reference module's literal ``hidden.view(-1, 128, Nr // 4, Nt // 4)`` admits: ``isize = [16, 64]``
(Nr, Nt), ``nz = 60``, ``nc = 2``, ``ngf = 128``, 0 .. 4 extra layers.  Anything else raises ``ValueError`` on the host.

torch only owns the device memory and the stream; every number is computed by the HIP kernels (``csrc/wgan.hip`` behind ``sbc_wgan_*``
of ``include/sbc_hip.h``).  ``state_dict_spec`` / ``seeded_state_dict`` / ``check_*`` need neither torch nor the library.
"""
import ctypes as C
import zlib

import numpy as np

from . import _lib

NR, NT, NZ, NC, NGF = 16, 64, 60, 2, 128
MAX_EXTRA = 4
# gain of the seeded conv_out weights over 1 / sqrt(fan_in): gives the generated channels of seeded_state_dict(13), the seed of the
# fixtures, unit variance per entry over N(0, 1) latents (0.98; measured on the CPU oracle).  With only two output filters the figure
# moves with the seed: 0.85 .. 2.6 over seeds 7 .. 14.
SEEDED_OUT_GAIN = 2.8
# sbc_wgan_stage ids (include/sbc_hip.h)
_ST_ACT, _ST_GEN, _ST_DG, _ST_GRAD, _ST_MASK = 0, 16, 17, 32, 48


def _bn_spec(prefix):
    return [(prefix + '.weight', (NGF,)), (prefix + '.bias', (NGF,)), (prefix + '.running_mean', (NGF,)),
            (prefix + '.running_var', (NGF,)), (prefix + '.num_batches_tracked', ())]


def state_dict_spec(n_extra=2):
    """Ordered ``[(name, shape)]`` of the reference ``DCGAN_G_Ours(isize=[16, 64], nz=60, nc=2, ngf=128, n_extra_layers=n_extra)``'s
    ``state_dict()`` (module registration order; ``num_batches_tracked`` is an int64 scalar, every other tensor float32)."""
    n_extra = int(n_extra)
    if not 0 <= n_extra <= MAX_EXTRA:
        raise ValueError('n_extra must be in [0, %d] (got %r)' % (MAX_EXTRA, n_extra))
    t = [('dense.dense_input.weight', (NGF * NR * NT // 16, NZ)), ('dense.dense_input.bias', (NGF * NR * NT // 16,))]
    for k in (1, 2):
        t += [('conv.conv%d.weight' % k, (NGF, NGF, 5, 5)), ('conv.conv%d.bias' % k, (NGF,))] + _bn_spec('conv.bn%d' % k)
    for i in range(n_extra):
        t += [('conv.extra_conv%d.weight' % i, (NGF, NGF, 3, 3))] + _bn_spec('conv.extra_bn%d' % i)
    return t + [('conv.conv_out.weight', (NC, NGF, 5, 5)), ('conv.conv_out.bias', (NC,))]


def n_extra_of(sd):
    """The number of extra layers a state dict holds (its ``conv.extra_conv<i>.weight`` keys, counted from 0)."""
    n = 0
    while 'conv.extra_conv%d.weight' % n in sd:
        n += 1
    return n


def seeded_state_dict(seed, n_extra=2):
    """Deterministic stand-in for trained weights; a tensor's values depend on the seed and its own name only (numpy ``PCG64`` keyed by
    ``(seed, crc32(name))``).  Convolution and dense weights are normal with He scaling, ``sqrt(2 / fan_in)``, where the input went
    through a ReLU and ``sqrt(1 / fan_in)`` where it did not (dense, conv1); their biases are normal of std 0.1.  BatchNorm is
    non-trivial: weight uniform in [0.8, 1.2], bias normal of std 0.1, running mean normal of std 0.2, running variance uniform in
    [0.6, 1.6].  ``conv_out`` is scaled so that the generated channels have about unit variance per entry."""
    sd = {}
    for name, shape in state_dict_spec(n_extra):
        rng = np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(name.encode())]))
        leaf = name.rsplit('.', 1)[1]
        if leaf == 'num_batches_tracked':
            sd[name] = np.asarray(6000, np.int64)
            continue
        if '.bn' in name or '_bn' in name:
            v = {'weight': lambda: rng.uniform(0.8, 1.2, size=shape), 'bias': lambda: 0.1 * rng.standard_normal(shape),
                 'running_mean': lambda: 0.2 * rng.standard_normal(shape), 'running_var': lambda: rng.uniform(0.6, 1.6, size=shape)}[leaf]()
        elif leaf == 'bias':
            v = 0.1 * rng.standard_normal(shape)
        else:
            fan_in = float(np.prod(shape[1:]))
            relu_in = not (name.startswith('dense.') or name.startswith('conv.conv1.'))
            gain = SEEDED_OUT_GAIN if name.startswith('conv.conv_out.') else np.sqrt(2.0 if relu_in else 1.0)
            v = gain / np.sqrt(fan_in) * rng.standard_normal(shape)
        sd[name] = np.asarray(v, np.float32)
    return sd


def check_geometry(isize, nz, nc, ngf, n_extra_layers=0):
    """Host-side refusal of what the kernels do not cover."""
    isize = [int(v) for v in isize]
    if isize != [NR, NT] or int(nz) != NZ or int(nc) != NC or int(ngf) != NGF:
        raise ValueError('only isize = [%d, %d], nz = %d, nc = %d, ngf = %d is supported (got isize %s, nz %s, nc %s, ngf %s)'
                         % (NR, NT, NZ, NC, NGF, isize, nz, nc, ngf))
    if not 0 <= int(n_extra_layers) <= MAX_EXTRA:
        raise ValueError('n_extra_layers must be in [0, %d] (got %r)' % (MAX_EXTRA, n_extra_layers))
    return int(n_extra_layers)


def check_state_dict(sd, n_extra):
    """Raise ``KeyError`` / ``ValueError`` like ``load_state_dict(strict=True)`` would."""
    _lib.check_against_spec(sd, state_dict_spec(n_extra))


def check_run_args(z_shape, Y_shape, P_shape, steps, H_shape=None, first_step=1):
    """Host-side checks of a run that need no data; returns ``(B, Np)``."""
    z_shape = tuple(z_shape)
    if len(z_shape) == 4 and z_shape[2:] == (1, 1):
        z_shape = z_shape[:2]
    if len(z_shape) != 2 or z_shape[1] != NZ:
        raise ValueError('z must be [B, %d] or [B, %d, 1, 1] (got %s)' % (NZ, NZ, z_shape))
    B = z_shape[0]
    if len(Y_shape) != 3 or len(P_shape) != 3:
        raise ValueError('Y must be [B, Nr, Np] and P [B, Nt, Np] (got %s, %s)' % (tuple(Y_shape), tuple(P_shape)))
    if (Y_shape[1], P_shape[1]) != (NR, NT):
        raise ValueError('geometry Nr x Nt = %d x %d is not supported: only %d x %d' % (Y_shape[1], P_shape[1], NR, NT))
    Np = Y_shape[2]
    if Y_shape[0] != B or P_shape[0] != B or P_shape[2] != Np or not 1 <= Np <= NT:
        raise ValueError('need Y [%d, %d, Np] and P [%d, %d, Np], 1 <= Np <= %d (got Y %s, P %s)'
                         % (B, NR, B, NT, NT, tuple(Y_shape), tuple(P_shape)))
    if H_shape is not None and tuple(H_shape) != (B, NR, NT):
        raise ValueError('H must be [%d, %d, %d] (got %s)' % (B, NR, NT, tuple(H_shape)))
    if int(steps) < 0 or int(steps) != steps:
        raise ValueError('steps must be a non-negative integer (got %r)' % (steps,))
    if int(first_step) < 1:
        raise ValueError('the first step is Adam\'s t = 1 (got %r)' % (first_step,))
    return B, Np


def per_sample(value, B, name):
    """A scalar or a length-``B`` sequence as a float32 ``[B]`` numpy array."""
    a = np.asarray(value, np.float64)
    if a.ndim == 0:
        a = np.full((B,), float(a))
    if a.shape != (B,):
        raise ValueError('%s must be a scalar or have shape (%d,) (got %s)' % (name, B, a.shape))
    if not np.all(np.isfinite(a)):
        raise ValueError('%s must be finite' % name)
    return a.astype(np.float32)


def stage_id(name, n_extra):
    """``'dense'``, ``'act<k>'``, ``'gen'``, ``'dG'``, ``'grad<k>'`` (k = 0 .. L), ``'mask<k>'`` (k = 1 .. L), L = 2 + n_extra."""
    L = 2 + int(n_extra)
    if name == 'dense':
        return _ST_ACT
    if name == 'gen':
        return _ST_GEN
    if name == 'dG':
        return _ST_DG
    for prefix, base, lo in (('act', _ST_ACT, 1), ('grad', _ST_GRAD, 0), ('mask', _ST_MASK, 1)):
        if name.startswith(prefix) and name[len(prefix):].isdigit() and lo <= int(name[len(prefix):]) <= L:
            return base + int(name[len(prefix):])
    raise ValueError('no stage %r in a generator with %d extra layers' % (name, n_extra))


def unpack_mask(words, width):
    """Sign-mask words ``[..., H, W / 32]`` (int32, bit j of word q: pixel 32 q + j) -> bool ``[..., H, W]``."""
    w = np.asarray(words).astype(np.int64) & 0xffffffff
    bits = (w[..., None] >> np.arange(32)) & 1
    return bits.reshape(w.shape[:-1] + (width,)).astype(bool)


class DCGAN_G_Ours(_lib.DeviceHandle):
    """``DCGAN_G_Ours(isize, nz, nc, ngf, ngpu, n_extra_layers)`` / ``load_state_dict`` / ``cuda`` / ``eval`` / ``__call__(z)`` as the
    reference module.  ``z``: float32 ``[B, 60, 1, 1]`` or ``[B, 60]`` (B = 1 also after the reference's ``squeeze``: ``[60]``) ->
    ``[B, 2, 16, 64]``.  ``stage(name)`` returns a view of the last call's workspace."""

    _destroy = 'sbc_wgan_destroy'

    def __init__(self, isize, nz, nc, ngf, ngpu=1, n_extra_layers=0, device=None):
        super().__init__(device)
        self.n_extra = check_geometry(isize, nz, nc, ngf, n_extra_layers)
        self.Nr, self.Nt = NR, NT
        self.ngpu = ngpu

    def load_state_dict(self, state):
        sd = _lib.numpy_state_dict(state)
        check_state_dict(sd, self.n_extra)
        return self._load(sd, [n for n, _ in state_dict_spec(self.n_extra) if not n.endswith('num_batches_tracked')],
                          _lib.lib().sbc_wgan_create)

    def _workspace(self, B, dev):
        return self._workspace_of(_lib.lib().sbc_wgan_workspace_floats(self._h, int(B)), dev)

    def _latents(self, z, dev):
        import torch
        if not isinstance(z, torch.Tensor):
            z = torch.from_numpy(np.ascontiguousarray(z))
        if z.dim() == 1 and z.shape[0] == NZ:
            z = z[None]
        if z.dim() == 4 and tuple(z.shape[2:]) == (1, 1):
            z = z[:, :, 0, 0]
        if z.dim() != 2 or z.shape[1] != NZ:
            raise ValueError('z must be [B, %d] or [B, %d, 1, 1] (got %s)' % (NZ, NZ, tuple(z.shape)))
        return z.detach().to(dev, torch.float32).contiguous()

    def __call__(self, z, stream=None):
        import torch
        self._need_weights()
        dev = self._torch_device()
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):           # whatever torch has to copy or convert is ordered on the same stream
            z = self._latents(z, dev)
        B = z.shape[0]
        out = torch.empty((B, NC, NR, NT), dtype=torch.float32, device=dev)
        if B == 0:
            return out
        with torch.cuda.device(dev):
            ws = self._workspace(B, dev)
            _lib.check(_lib.lib().sbc_wgan_generate(self._h, C.c_void_p(z.data_ptr()), C.c_void_p(out.data_ptr()), B,
                                                    C.c_void_p(ws.data_ptr()), C.c_void_p(s.cuda_stream)))
            for t in (z, ws, out):
                t.record_stream(s)
        self.last_workspace = (ws, B)
        return out

    forward = __call__

    def stage(self, name):
        """A stage ``[B, C, H, W]`` of the last call, a view of its workspace: ``'dense'`` / ``'act<k>'`` activations, ``'gen'``,
        ``'dG'``, ``'grad<k>'`` = d loss / d (activation k), ``'mask<k>'`` the ReLU sign words of layer k as int32 ``[B, 128, H, W / 32]``
        (``unpack_mask``)."""
        import torch
        ws, B = self.last_workspace
        off, c, h, w = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().sbc_wgan_stage(self._h, stage_id(name, self.n_extra), int(B), C.byref(off), C.byref(c), C.byref(h), C.byref(w)))
        t = ws[off.value:off.value + B * c.value * h.value * w.value]
        if name.startswith('mask'):
            t = t.view(torch.int32)
        return t.view(B, c.value, h.value, w.value)


class LatentOptimizer:
    """The loop of ``test_wgan.py:145-176`` for a batch of independent samples.

    ``run(z0, Y, P, lr, l2_lam, steps, H=None, loss_scale=None, state=None, return_logs=True)`` -> ``(z, state, logs)``:
    ``z0`` float32 ``[B, 60]`` (or ``[B, 60, 1, 1]``), ``Y`` complex64 ``[B, 16, Np]``, ``P`` complex64 ``[B, 64, Np]``, ``H`` complex64
    ``[B, 16, 64]``; ``lr``, ``l2_lam`` and ``loss_scale`` are scalars or per-sample sequences, held as float32 (``loss_scale`` defaults
    to ``1 / B``, the reference's ``torch.mean`` over its batch).  ``state`` (``{'m', 'v', 'step'}``, as returned) continues a run:
    Adam's moments and the number of steps taken.  ``logs``: ``meas`` and ``reg`` ``[steps, B]`` (and ``oracle`` with ``H``), taken at
    ``z_k`` before the update; with ``return_logs='full'`` also ``z`` and ``g`` ``[steps, B, 60]``."""

    def __init__(self, netG):
        self.netG = netG

    def run(self, z0, Y, P, lr, l2_lam, steps, H=None, loss_scale=None, state=None, return_logs=True, stream=None):
        import torch
        G = self.netG
        G._need_weights()
        for name, t in (('Y', Y), ('P', P)) + ((('H', H),) if H is not None else ()):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.complex64:
                raise ValueError('%s must be a complex64 tensor (got %s)' % (name, getattr(t, 'dtype', type(t))))
        first = 1 + (int(state['step']) if state is not None else 0)
        B, Np = check_run_args(tuple(np.shape(z0)), tuple(Y.shape), tuple(P.shape), steps, None if H is None else tuple(H.shape), first)
        steps = int(steps)
        dev = G._torch_device()
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        # the copies, conversions and zero fills torch launches here are ordered on the stream the kernels run on
        with torch.cuda.device(dev), torch.cuda.stream(s):
            z = G._latents(z0, dev).clone()
            Y, P = Y.to(dev).resolve_conj().contiguous(), P.to(dev).resolve_conj().contiguous()
            H = H.to(dev).resolve_conj().contiguous() if H is not None else None
            arr = {k: torch.from_numpy(per_sample(v, B, k)).to(dev)
                   for k, v in (('lr', lr), ('l2_lam', l2_lam), ('loss_scale', 1.0 / max(B, 1) if loss_scale is None else loss_scale))}
            if state is not None:
                m, v = (state[k].detach().to(dev, torch.float32).clone().contiguous() for k in ('m', 'v'))
                if tuple(m.shape) != (B, NZ) or tuple(v.shape) != (B, NZ):
                    raise ValueError('state m and v must be [%d, %d]' % (B, NZ))
            else:
                m, v = torch.zeros_like(z), torch.zeros_like(z)
        logs = {}
        if return_logs:
            logs = {'meas': torch.empty((steps, B), dtype=torch.float32, device=dev), 'reg': torch.empty((steps, B), dtype=torch.float32, device=dev)}
            if H is not None:
                logs['oracle'] = torch.empty((steps, B), dtype=torch.float32, device=dev)
            if return_logs == 'full':
                logs['z'] = torch.empty((steps, B, NZ), dtype=torch.float32, device=dev)
                logs['g'] = torch.empty((steps, B, NZ), dtype=torch.float32, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None           # noqa: E731
        if B == 0 or steps == 0:
            return z, {'m': m, 'v': v, 'step': first - 1 + steps}, logs
        with torch.cuda.device(dev):
            ws = G._workspace(B, dev)
            d = _lib.sbc_wgan_run_desc(Y=ptr(Y), P=ptr(P), H=ptr(H), z=ptr(z), m=ptr(m), v=ptr(v), lr=ptr(arr['lr']), l2_lam=ptr(arr['l2_lam']),
                                       loss_scale=ptr(arr['loss_scale']), oracle_log=ptr(logs.get('oracle')), meas_log=ptr(logs.get('meas')),
                                       reg_log=ptr(logs.get('reg')), z_log=ptr(logs.get('z')), g_log=ptr(logs.get('g')), workspace=ptr(ws),
                                       B=B, Np=Np, first_step=first, n_steps=steps)
            _lib.check(_lib.lib().sbc_wgan_run(G._h, C.byref(d), C.c_void_p(s.cuda_stream)))
            for t in (Y, P, H, ws, z, m, v) + tuple(arr.values()) + tuple(logs.values()):
                if t is not None:
                    t.record_stream(s)
            for t in (z, m, v):                                       # allocated under `s`, handed to a caller on the current stream
                t.record_stream(torch.cuda.current_stream(dev))
        G.last_workspace = (ws, B)
        return z, {'m': m, 'v': v, 'step': first - 1 + steps}, logs
