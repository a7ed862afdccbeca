"""Learned D-AMP (the L-DAMP baseline of Fig. 5c) on the HIP library: counterpart of the reference's ``aux_models.LDAMP``
(``src/score_based_channels/aux_models.py:62-190``) with ``aux_unet.FlippedNormUnet`` denoisers: inference (``LDAMP``) and training
(``Trainer``: the model and optimiser of the reference's ``train_ldamp.py``).

Supported is the configuration ``train_ldamp.py:41-47`` trains: ``backbone='FlippedUNet'``, ``shared_nets=False``, one U-Net
(``chans=16``, ``num_pools=3``) per unroll, Nt x Nr = 64 x 16.  Other settings raise ``ValueError`` on the host.

torch only owns the device memory and the stream; every number is computed by the HIP kernels (``csrc/ldamp.hip`` and
``csrc/ldamp_train.hip`` behind ``sbc_ldamp_*`` of ``include/sbc_hip.h``).  ``state_dict_spec`` / ``seeded_state_dict`` need neither torch nor the library.
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


# ---- training (train_ldamp.py of the reference) ---------------------------------------------------------------------------------------
MAX_TRAIN_BATCH = 128
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
# sbc_ldamp_trainer_stage kinds (include/sbc_hip.h)
TRAIN_FORWARD, TRAIN_GRAD, TRAIN_RSTD, TRAIN_GH, TRAIN_GZ, TRAIN_DIV = range(6)


def check_trainer_args(capacity, lr):
    if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= int(capacity) <= MAX_TRAIN_BATCH:
        raise ValueError('capacity must be an integer in [1, %d] (got %r)' % (MAX_TRAIN_BATCH, capacity))
    check_lr(lr)


def check_lr(lr):
    if not isinstance(lr, (int, float)) or isinstance(lr, bool) or not lr >= 0 or lr == float('inf'):
        raise ValueError('lr must be a finite number >= 0 (got %r)' % (lr,))


def check_step_args(Y_shape, P_shape, eig_shape, H_shape, num_unrolls, max_unrolls, capacity, directions_shape=None):
    """Host-side checks of a training step that need no data."""
    check_run_args(Y_shape, P_shape, eig_shape, num_unrolls, max_unrolls, directions_shape)
    B = Y_shape[0]
    if B > capacity:
        raise ValueError('a batch must hold at most %d samples, the trainer\'s capacity (got %d)' % (capacity, B))
    if tuple(H_shape) != (B, NT, NR):
        raise ValueError('H_herm_cplx must be [%d, %d, %d] (got %s)' % (B, NT, NR, tuple(H_shape)))


def adam_param_group(lr, n_params):
    """``torch.optim.Adam(params, lr).state_dict()['param_groups'][0]``"""
    return {'lr': float(lr), 'betas': ADAM_BETAS, 'eps': ADAM_EPS, 'weight_decay': 0, 'amsgrad': False, 'maximize': False, 'foreach': None,
            'capturable': False, 'differentiable': False, 'fused': None, 'params': list(range(n_params))}


class Trainer(_lib.DeviceHandle):
    """The model and optimiser of the reference's ``train_ldamp.py`` on the device: ``Trainer(hparams, state_dict=None, lr=1e-3,
    capacity=128)``; ``state_dict=None`` starts from ``seeded_state_dict(init_seed)``, whose bounds are torch's default initialisation.

    ``step(sample, num_unrolls=None, directions=None, seed=0, sample_ids=None, stream=None)`` -> ``(loss, nmse)`` as python floats
    (waits for the step): forward as ``LDAMP.__call__``, ``loss = mean_b sum |h - H|^2``, backward and one Adam step with the current
    ``lr`` (``set_lr``; the caller schedules it).  ``update=False`` stops after the gradients; ``return_logs=True`` appends the dict of
    per-unroll ``h``, ``z``, ``div``, ``eps``.  ``state_dict()`` has the reference's names, ``optimizer_state_dict()`` the form of
    ``torch.optim.Adam.state_dict()``.  ``stage(name, unroll)`` / ``grad(name, unroll)`` are views of the last step's workspace
    (``grad`` of a ``state_dict`` name: that tensor's gradient as numpy).

    Adam's step count is one number for the whole model, as it is when every step runs the same ``num_unrolls`` (the reference always
    trains ``max_unrolls``): an updating step with another ``num_unrolls`` than the earlier ones raises ``ValueError``."""

    _destroy = 'sbc_ldamp_trainer_destroy'

    def __init__(self, hparams, state_dict=None, lr=1e-3, capacity=MAX_TRAIN_BATCH, device=None, init_seed=0):
        super().__init__(device)
        import torch
        self.max_unrolls = check_hparams(hparams)
        check_trainer_args(capacity, lr)
        self.capacity, self.lr = int(capacity), float(lr)
        sd = seeded_state_dict(init_seed, self.max_unrolls) if state_dict is None else _lib.numpy_state_dict(state_dict)
        check_state_dict(sd, self.max_unrolls)
        self._spec = state_dict_spec(self.max_unrolls)
        self._net_floats = sum(int(np.prod(s)) for _, s in unet_spec())
        self.steps = 0                                   # Adam steps taken
        self.trained_unrolls = 0                         # nets 0 .. trained_unrolls - 1 have optimiser state
        refs, keep = _lib.tensor_refs(sd, [n for n, _ in self._spec])
        handle = C.c_void_p()
        with torch.cuda.device(self._torch_device()):
            _lib.check(_lib.lib().sbc_ldamp_trainer_create(refs, len(refs), self.max_unrolls, C.byref(handle)))
        self._h = handle
        self.last_step = None                            # (workspace, B, num_unrolls, Np)

    def set_lr(self, lr):
        check_lr(lr)
        self.lr = float(lr)

    # -- state ---------------------------------------------------------------------------------------------------------------------
    def _get(self, what):
        import torch
        flat = np.empty(self.max_unrolls * self._net_floats, np.float32)
        step = C.c_int64()
        with torch.cuda.device(self._torch_device()):
            _lib.check(_lib.lib().sbc_ldamp_trainer_get_state(self._h, what, flat.ctypes.data_as(C.c_void_p), C.byref(step)))
        return flat

    def _set(self, what, flat):
        import torch
        flat = np.ascontiguousarray(flat, np.float32)
        with torch.cuda.device(self._torch_device()):
            _lib.check(_lib.lib().sbc_ldamp_trainer_set_state(self._h, what, flat.ctypes.data_as(C.c_void_p), self.steps))

    def _split(self, flat):
        out, o = {}, 0
        for name, shape in self._spec:
            n = int(np.prod(shape))
            out[name] = flat[o:o + n].reshape(shape).copy()
            o += n
        return out

    def _join(self, tensors):
        return np.concatenate([np.asarray(tensors[n], np.float32).reshape(-1) for n, _ in self._spec])

    def state_dict(self):
        """``{name: float32 array}`` with the names and shapes of the reference's ``LDAMP.state_dict()``"""
        return self._split(self._get(0))

    def load_state_dict(self, model_state):
        sd = _lib.numpy_state_dict(model_state)
        check_state_dict(sd, self.max_unrolls)
        self._set(0, self._join(sd))
        return self

    def gradients(self):
        """``{name: float32 array}`` of the last step (zeros for nets that have never run)"""
        return self._split(self._get(1))

    def optimizer_state_dict(self):
        import torch
        m, v = self._split(self._get(2)), self._split(self._get(3))
        n_state = self.trained_unrolls * N_NET_TENSORS if self.steps else 0
        state = {i: {'step': torch.tensor(float(self.steps)), 'exp_avg': torch.from_numpy(m[name]), 'exp_avg_sq': torch.from_numpy(v[name])}
                 for i, (name, _) in enumerate(self._spec[:n_state])}
        return {'state': state, 'param_groups': [adam_param_group(self.lr, len(self._spec))]}

    def load_optimizer_state_dict(self, opt_state):
        state, groups = opt_state['state'], opt_state['param_groups']
        if len(groups) != 1 or list(groups[0]['params']) != list(range(len(self._spec))):
            raise ValueError('the optimiser state must have one parameter group over the %d tensors in state_dict order' % len(self._spec))
        g = groups[0]
        if tuple(g.get('betas', ADAM_BETAS)) != ADAM_BETAS or g.get('eps', ADAM_EPS) != ADAM_EPS or g.get('weight_decay', 0) != 0 or g.get('amsgrad', False):
            raise ValueError('only torch.optim.Adam defaults are supported (betas %s, eps %g, no weight decay, no amsgrad)' % (ADAM_BETAS, ADAM_EPS))
        check_lr(g['lr'])
        idx = sorted(int(i) for i in state)
        if idx != list(range(len(idx))) or len(idx) % N_NET_TENSORS:
            raise ValueError('optimiser state must cover the tensors of nets 0 .. k - 1 (got %d entries)' % len(idx))
        steps = {int(float(state[i]['step'])) for i in idx}
        if len(steps) > 1:
            raise ValueError('every tensor must have the same Adam step count (got %s)' % sorted(steps))
        zeros = {n: np.zeros(s, np.float32) for n, s in self._spec}
        m, v = dict(zeros), dict(zeros)
        for i in idx:
            name, shape = self._spec[i]
            for dst, key in ((m, 'exp_avg'), (v, 'exp_avg_sq')):
                a = _lib.numpy_state_dict({name: state[i][key]})[name]
                if tuple(a.shape) != tuple(shape):
                    raise ValueError('size mismatch for %s of %s: %s vs %s' % (key, name, tuple(a.shape), tuple(shape)))
                dst[name] = a
        self.steps = steps.pop() if idx else 0
        self.trained_unrolls = len(idx) // N_NET_TENSORS
        self.lr = float(g['lr'])
        self._set(2, self._join(m))
        self._set(3, self._join(v))
        return self

    # -- one step --------------------------------------------------------------------------------------------------------------------
    def step(self, sample, num_unrolls=None, directions=None, seed=0, sample_ids=None, stream=None, update=True, return_logs=False):
        import torch
        Y, P, eig, H = sample['Y_herm'], sample['P_herm'], sample['eig1'], sample['H_herm_cplx']
        for name, t in (('Y_herm', Y), ('P_herm', P), ('H_herm_cplx', H)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.complex64:
                raise ValueError('%s must be a complex64 tensor (got %s)' % (name, getattr(t, 'dtype', type(t))))
        if not isinstance(eig, torch.Tensor):
            raise ValueError('eig1 must be a tensor (got %s)' % type(eig))
        U = self.max_unrolls if num_unrolls is None else num_unrolls
        if isinstance(U, bool) or int(U) != U:
            raise ValueError('num_unrolls must be an integer (got %r)' % (U,))
        U = int(U)
        if directions is not None and not isinstance(directions, torch.Tensor):
            directions = torch.from_numpy(np.ascontiguousarray(directions, dtype=np.float32))
        check_step_args(tuple(Y.shape), tuple(P.shape), tuple(eig.shape), tuple(H.shape), U, self.max_unrolls, self.capacity,
                        None if directions is None else tuple(directions.shape))
        if update and self.steps and U != self.trained_unrolls:
            raise ValueError('this trainer\'s Adam state belongs to steps of %d unrolls: an updating step of %d would need per-net step counts'
                             % (self.trained_unrolls, U))
        B, Np = Y.shape[0], Y.shape[1]
        sample0 = 0
        if sample_ids is not None:
            ids = np.asarray(sample_ids.cpu().numpy() if isinstance(sample_ids, torch.Tensor) else sample_ids).astype(np.int64)
            if ids.shape != (B,) or (B and not np.array_equal(ids, ids[0] + np.arange(B))):
                raise ValueError('sample_ids must be %d consecutive integers (got %s)' % (B, ids))
            sample0 = int(ids[0]) if B else 0
        if B == 0:                                       # an empty batch launches nothing and changes nothing
            nan = float('nan')
            return ((nan, nan), {}) if return_logs else (nan, nan)
        dev = self._torch_device()
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(s):
            Y, P, H = (t.to(dev).resolve_conj().contiguous() for t in (Y, P, H))
            eig = eig.to(dev, torch.float32).contiguous()
            if directions is not None:
                directions = directions.to(dev, torch.float32).contiguous()
            out = torch.empty(2, dtype=torch.float32, device=dev)
            logs = {}
            if return_logs:
                logs = {'h': torch.empty((U, B, NT, NR), dtype=torch.complex64, device=dev),
                        'z': torch.empty((U, B, Np, NR), dtype=torch.complex64, device=dev),
                        'div': torch.empty((U, B), dtype=torch.float32, device=dev),
                        'eps': torch.empty((U, B), dtype=torch.float32, device=dev)}
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None           # noqa: E731
        with torch.cuda.device(dev):
            ws = self._workspace_of(_lib.lib().sbc_ldamp_trainer_workspace_floats(B, U, int(directions is None)), dev)
            d = _lib.sbc_ldamp_step_desc(Y_herm=ptr(Y), P_herm=ptr(P), eig1=ptr(eig), directions=ptr(directions), Htrue=ptr(H), loss=ptr(out),
                                         h_log=ptr(logs.get('h')), z_log=ptr(logs.get('z')), div_log=ptr(logs.get('div')),
                                         eps_log=ptr(logs.get('eps')), workspace=ptr(ws), seed=int(seed) & (2 ** 64 - 1), sample0=sample0,
                                         lr=self.lr, step=self.steps + 1 if update else 0, B=B, Np=Np, Nt=NT, Nr=NR, num_unrolls=U)
            _lib.check(_lib.lib().sbc_ldamp_trainer_step(self._h, C.byref(d), C.c_void_p(s.cuda_stream)))
            for t in [Y, P, H, eig, directions, ws, out] + list(logs.values()):
                if t is not None:
                    t.record_stream(s)
            with torch.cuda.stream(s):
                loss, nmse = (float(x) for x in out.cpu())
        if update:
            self.steps += 1
            self.trained_unrolls = U
        self.last_step = (ws, B, U, Np)
        return ((loss, nmse), logs) if return_logs else (loss, nmse)

    def adam(self, grads, lr=None, stream=None):
        """One Adam step on given gradients (``{name: array}`` for nets ``0 .. k - 1``, or None: those of the last step)."""
        import torch
        dev = self._torch_device()
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if lr is not None:
            self.set_lr(lr)
        k = self.trained_unrolls or self.max_unrolls
        g = None
        if grads is not None:
            names = [n for n, _ in self._spec if n in grads]
            k = len(names) // N_NET_TENSORS
            if names != [n for n, _ in self._spec[:k * N_NET_TENSORS]] or not k:
                raise ValueError('grads must hold every tensor of nets 0 .. k - 1')
            flat = np.concatenate([np.asarray(grads[n], np.float32).reshape(-1) for n in names])
            with torch.cuda.device(dev), torch.cuda.stream(s):
                g = torch.from_numpy(flat).to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().sbc_ldamp_trainer_adam(self._h, C.c_void_p(g.data_ptr()) if g is not None else None, k, self.lr, self.steps + 1,
                                                         C.c_void_p(s.cuda_stream)))
            if g is not None:
                g.record_stream(s)
        self.steps += 1
        self.trained_unrolls = k

    # -- debug access ------------------------------------------------------------------------------------------------------------------
    def _view(self, kind, stage, unroll):
        ws, B, U, Np = self.last_step
        u = U - 1 if unroll is None else int(unroll) % U
        off, n, c, h, w = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().sbc_ldamp_trainer_stage(kind, stage, u, B, U, C.byref(off), C.byref(n), C.byref(c), C.byref(h), C.byref(w)))
        return ws[off.value:off.value + n.value * c.value * h.value * w.value], (n.value, c.value, h.value, w.value)

    def _shaped(self, t, name, shape):
        n = shape[0]
        return t.view(n, NT, NR, 2) if name == 'r' else t.view(n, 4) if name == 'stat' else t.view(*shape)

    def stage(self, name, unroll=None):
        """A forward stage of the last step (``STAGES``; unroll default: the last), ``[2B, C, H, W]``: image ``b`` clean, ``B + b``
        perturbed; ``'rstd:<stage>'``: ``[2B, C]`` of that stage's InstanceNorm; ``'div'``: ``[B]``."""
        if name == 'div':
            return self._view(TRAIN_DIV, 0, unroll)[0]
        if name.startswith('rstd:'):
            t, shape = self._view(TRAIN_RSTD, STAGES.index(name[5:]), unroll)
            return t.view(shape[0], shape[1])
        t, shape = self._view(TRAIN_FORWARD, STAGES.index(name), unroll)
        return self._shaped(t, name, shape)

    def grad(self, name, unroll=None):
        """Of the last step: the gradient of a parameter (a ``state_dict`` name -> numpy), or the loss gradient with respect to a clean
        stage ``[B, C, H, W]`` (``'r'``: ``[B, 64, 16, 2]``; ``'stat'``: the finish's share, ``[B, 4]``), ``'gh'`` (``dL/dh_u`` as it
        reaches unroll ``u``, ``[B, 64, 16, 2]``) or ``'gz'`` (``dL/dz_u``, ``[B, Np, 16, 2]``)."""
        if name in dict(self._spec):
            return self.gradients()[name]
        B, Np = self.last_step[1], self.last_step[3]
        if name == 'gh':
            return self._view(TRAIN_GH, 0, unroll)[0].view(B, NT, NR, 2)
        if name == 'gz':
            return self._view(TRAIN_GZ, 0, unroll)[0][:B * Np * NR * 2].view(B, Np, NR, 2)
        t, shape = self._view(TRAIN_GRAD, STAGES.index(name), unroll)
        return self._shaped(t, name, shape)


N_NET_TENSORS = len(unet_spec())
