"""WGAN latent optimisation (the WGAN baseline of Fig. 5c) on the HIP library: counterpart of the reference's generator
``aux_gan.DCGAN_G_Ours`` (``src/score_based_channels/aux_gan.py:58-112``) in eval mode and of the optimisation loop of
``test_wgan.py:129-176`` (Adam on the latents against ``||G(z) P - Y||^2 + lambda ||z||^2``).

Supported is the one geometry the reference module's literal ``hidden.view(-1, 128, Nr // 4, Nt // 4)`` admits: ``isize = [16, 64]``
(Nr, Nt), ``nz = 60``, ``nc = 2``, ``ngf = 128``, 0 .. 4 extra layers.  Anything else raises ``ValueError`` on the host.

The second half of the module is the training of that generator (``train_wgan.py:96-202``): the critic ``aux_gan.DCGAN_D``'s state-dict
surface, the reference's initial distributions and ``Trainer`` with its critic and generator iterations (``csrc/wgan_train.hip`` behind
``sbc_wgan_trainer_*``).

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


def _bn_spec(prefix, c=NGF):
    return [(prefix + '.weight', (c,)), (prefix + '.bias', (c,)), (prefix + '.running_mean', (c,)), (prefix + '.running_var', (c,)),
            (prefix + '.num_batches_tracked', ())]


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


def _named_rng(seed, name):
    """The generator of tensor ``name``: numpy ``PCG64`` keyed by ``(seed, crc32(name))``"""
    return np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(name.encode())]))


def _draw_state_dict(seed, spec, batches, bn, weight):
    """A state dict of ``spec`` whose tensors are drawn from their own ``_named_rng``: ``num_batches_tracked`` is ``batches``, a BatchNorm
    tensor ``bn[leaf](rng, shape)``, every other one ``weight(rng, name, leaf, shape)``, as float32."""
    sd = {}
    for name, shape in spec:
        leaf = name.rsplit('.', 1)[1]
        if leaf == 'num_batches_tracked':
            sd[name] = np.asarray(batches, np.int64)
        elif '.bn' in name or '_bn' in name or 'batchnorm' in name:
            sd[name] = np.asarray(bn[leaf](_named_rng(seed, name), shape), np.float32)
        else:
            sd[name] = np.asarray(weight(_named_rng(seed, name), name, leaf, shape), np.float32)
    return sd


def seeded_state_dict(seed, n_extra=2):
    """Deterministic stand-in for trained weights; a tensor's values depend on the seed and its own name only (numpy ``PCG64`` keyed by
    ``(seed, crc32(name))``).  Convolution and dense weights are normal with He scaling, ``sqrt(2 / fan_in)``, where the input went
    through a ReLU and ``sqrt(1 / fan_in)`` where it did not (dense, conv1); their biases are normal of std 0.1.  BatchNorm is
    non-trivial: weight uniform in [0.8, 1.2], bias normal of std 0.1, running mean normal of std 0.2, running variance uniform in
    [0.6, 1.6].  ``conv_out`` is scaled so that the generated channels have about unit variance per entry."""
    def weight(rng, name, leaf, shape):
        if leaf == 'bias':
            return 0.1 * rng.standard_normal(shape)
        fan_in = float(np.prod(shape[1:]))
        relu_in = not (name.startswith('dense.') or name.startswith('conv.conv1.'))
        gain = SEEDED_OUT_GAIN if name.startswith('conv.conv_out.') else np.sqrt(2.0 if relu_in else 1.0)
        return gain / np.sqrt(fan_in) * rng.standard_normal(shape)

    bn = {'weight': lambda rng, shape: rng.uniform(0.8, 1.2, size=shape), 'bias': lambda rng, shape: 0.1 * rng.standard_normal(shape),
          'running_mean': lambda rng, shape: 0.2 * rng.standard_normal(shape), 'running_var': lambda rng, shape: rng.uniform(0.6, 1.6, size=shape)}
    return _draw_state_dict(seed, state_dict_spec(n_extra), 6000, bn, weight)


def _check_geometry(isize, nz, nc, width, width_name, expected, n_extra_layers):
    isize = [int(v) for v in isize]
    if isize != [NR, NT] or int(nz) != NZ or int(nc) != NC or int(width) != expected:
        raise ValueError('only isize = [%d, %d], nz = %d, nc = %d, %s = %d is supported (got isize %s, nz %s, nc %s, %s %s)'
                         % (NR, NT, NZ, NC, width_name, expected, isize, nz, nc, width_name, width))
    if not 0 <= int(n_extra_layers) <= MAX_EXTRA:
        raise ValueError('n_extra_layers must be in [0, %d] (got %r)' % (MAX_EXTRA, n_extra_layers))
    return int(n_extra_layers)


def check_geometry(isize, nz, nc, ngf, n_extra_layers=0):
    """Host-side refusal of what the kernels do not cover."""
    return _check_geometry(isize, nz, nc, ngf, 'ngf', NGF, n_extra_layers)


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


def _stage_view(ws, off, B, c, h, w, is_mask):
    """``[B, c, h, w]`` at float offset ``off`` of the workspace tensor ``ws``; a mask's words as int32"""
    import torch
    t = ws[off:off + B * c * h * w]
    if is_mask:
        t = t.view(torch.int32)
    return t.view(B, c, h, w)


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
        ws, B = self.last_workspace
        off, c, h, w = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().sbc_wgan_stage(self._h, stage_id(name, self.n_extra), int(B), C.byref(off), C.byref(c), C.byref(h), C.byref(w)))
        return _stage_view(ws, off.value, B, c.value, h.value, w.value, name.startswith('mask'))


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


# ---- WGAN training (train_wgan.py:96-202 on csrc/wgan_train.hip behind sbc_wgan_trainer_*) ---------------------------------------------
NDF = 64
_KINDS = {'act': 0, 'raw': 1, 'pre': 2, 'mask': 3, 'mean': 4, 'var': 5, 'gact': 6, 'draw': 7}
_NETS = {'g': 0, 'd0': 1, 'd1': 2}                     # the generator; the critic's pass over real; its pass over fake
_NET_INDEX = {'g': 0, 'd': 1}                          # sbc_wgan_trainer_copy's net
RMSPROP_DEFAULTS = dict(lr=5e-5, alpha=0.99, eps=1e-8)
CLAMP = (-0.01, 0.01)


def disc_state_dict_spec(n_extra=1):
    """Ordered ``[(name, shape)]`` of the reference ``DCGAN_D(isize=[16, 64], nz=60, nc=2, ndf=64, ngpu=1, n_extra_layers=n_extra)``'s
    ``state_dict()`` (``aux_gan.py:9-47``; no convolution has a bias)."""
    n_extra = int(n_extra)
    if not 0 <= n_extra <= MAX_EXTRA:
        raise ValueError('n_extra must be in [0, %d] (got %r)' % (MAX_EXTRA, n_extra))
    t = [('main.initial:%d-%d:conv.weight' % (NC, NDF), (NDF, NC, 4, 4))]
    for i in range(n_extra):
        t += [('main.extra-layers-%d:%d:conv.weight' % (i, NDF), (NDF, NDF, 3, 3))] + _bn_spec('main.extra-layers-%d:%d:batchnorm' % (i, NDF), NDF)
    t += [('main.pyramid:%d-%d:conv.weight' % (NDF, 2 * NDF), (2 * NDF, NDF, 4, 4))] + _bn_spec('main.pyramid:%d:batchnorm' % (2 * NDF), 2 * NDF)
    return t + [('main.final:%d-1:conv.weight' % (2 * NDF), (1, 2 * NDF, NR // 4, NT // 4))]


def check_disc_geometry(isize, nz, nc, ndf, n_extra_layers=0):
    return _check_geometry(isize, nz, nc, ndf, 'ndf', NDF, n_extra_layers)


def init_state_dicts(seed, n_extra=1):
    """``(gen_state, disc_state)`` drawn as ``train_wgan.py:78-94`` initialises them: convolution weights N(0, 0.02), BatchNorm weights
    N(1, 0.02) and biases 0, running statistics (0, 1, 0 batches); the dense layer and the convolution biases, which ``weights_init`` does
    not touch, keep torch's default U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)).  A tensor's values depend on the seed and its own name only
    (numpy ``PCG64`` keyed by ``(seed, crc32(name))``, like ``seeded_state_dict``)."""
    def weight(rng, name, leaf, shape):
        if name.startswith('dense.') or leaf == 'bias':
            return rng.uniform(-1.0, 1.0, size=shape) / np.sqrt(NZ if name.startswith('dense.') else NGF * 25)
        return 0.02 * rng.standard_normal(shape)

    bn = {'weight': lambda rng, shape: 1.0 + 0.02 * rng.standard_normal(shape), 'bias': lambda rng, shape: np.zeros(shape),
          'running_mean': lambda rng, shape: np.zeros(shape), 'running_var': lambda rng, shape: np.ones(shape)}
    return tuple(_draw_state_dict(seed, spec, 0, bn, weight) for spec in (state_dict_spec(n_extra), disc_state_dict_spec(n_extra)))


class DCGAN_D:
    """``DCGAN_D(isize, nz, nc, ndf, ngpu, n_extra_layers)`` with the reference module's ``state_dict`` surface: the critic exists on the
    device inside a ``Trainer`` only, so this object holds its tensors on the host (numpy) and checks names and shapes."""

    def __init__(self, isize, nz, nc, ndf, ngpu=1, n_extra_layers=0):
        self.n_extra = check_disc_geometry(isize, nz, nc, ndf, n_extra_layers)
        self.ngpu = ngpu
        self._sd = None

    def load_state_dict(self, state):
        sd = _lib.numpy_state_dict(state)
        _lib.check_against_spec(sd, disc_state_dict_spec(self.n_extra))
        self._sd = {n: np.array(sd[n]) for n, _ in disc_state_dict_spec(self.n_extra)}
        return self

    def state_dict(self):
        if self._sd is None:
            raise RuntimeError('DCGAN_D has no weights: call load_state_dict first')
        return dict(self._sd)


def trainer_stage_id(name, n_extra):
    """``'<net>.<kind><layer>'``: net ``g`` (layer 0 .. L, 0 the dense output), ``d0`` / ``d1`` the critic's pass over real / fake (layer
    0 .. M = n_extra + 2); kind ``act raw pre mask mean var gact`` (d loss / d activation) ``draw`` (d loss / d raw); and ``g.gen``,
    ``g.dgen``, ``d0.err``, ``d1.err``."""
    net, _, rest = name.partition('.')
    if net in _NETS:
        special = {('g', 'gen'): 128, ('g', 'dgen'): 129, ('d0', 'err'): 130, ('d1', 'err'): 130}
        if (net, rest) in special:
            return 256 * _NETS[net] + special[(net, rest)]
        for kind, q in _KINDS.items():
            if rest.startswith(kind) and rest[len(kind):].isdigit() and int(rest[len(kind):]) <= (2 + n_extra if net == 'g' else n_extra + 2):
                return 256 * _NETS[net] + 16 * q + int(rest[len(kind):])
    raise ValueError('no stage %r in networks with %d extra layers' % (name, n_extra))


class Trainer(_lib.DeviceHandle):
    """Both networks of ``train_wgan.py`` in training mode on the device, with their RMSprop states.

    ``Trainer(gen_state, disc_state, batch_size=200)``; ``critic_step(real [Br, 2, 16, 64], noise [Bf, 60])`` -> float32 ``[2]`` on the
    device (``errD_real``, ``errD_fake``); ``generator_step(noise [B, 60])`` -> ``[1]`` (``errG``); ``state_dicts()`` and
    ``optimizer_state_dicts()`` (``torch.optim.RMSprop.state_dict()`` form) as numpy on the host; ``stage(name)`` a view of the last
    call's workspace (``trainer_stage_id``); ``tensor(net, name, what)`` / ``set_tensor`` a parameter, its gradient or its square average."""

    _destroy = 'sbc_wgan_trainer_destroy'

    def __init__(self, gen_state, disc_state, batch_size=200, lrD=5e-5, lrG=5e-5, alpha=0.99, eps=1e-8, clamp=CLAMP, device=None):
        super().__init__(device)
        import torch
        gsd, dsd = _lib.numpy_state_dict(gen_state), _lib.numpy_state_dict(disc_state)
        self.n_extra = n_extra_of(gsd)
        if not 0 <= self.n_extra <= MAX_EXTRA:
            raise ValueError('at most %d extra layers are supported (got %d)' % (MAX_EXTRA, self.n_extra))
        check_state_dict(gsd, self.n_extra)
        _lib.check_against_spec(dsd, disc_state_dict_spec(self.n_extra))
        if int(batch_size) < 1 or int(batch_size) > 32768:
            raise ValueError('batch_size must be in [1, 32768] (got %r)' % (batch_size,))
        self.capacity = int(batch_size)
        self.hyper = dict(lrD=float(lrD), lrG=float(lrG), alpha=float(alpha), eps=float(eps), clamp=(float(clamp[0]), float(clamp[1])))
        self._names = [[n for n, _ in spec if not n.endswith('num_batches_tracked')] for spec in (state_dict_spec(self.n_extra), disc_state_dict_spec(self.n_extra))]
        self._shapes = [dict(state_dict_spec(self.n_extra)), dict(disc_state_dict_spec(self.n_extra))]
        self._tracked = [int(next(v for k, v in sd.items() if k.endswith('num_batches_tracked'))) for sd in (gsd, dsd)]
        self.steps = [0, 0]                              # optimiser steps taken: generator, critic
        desc = _lib.sbc_wgan_trainer_desc(self.hyper['lrD'], self.hyper['lrG'], self.hyper['alpha'], self.hyper['eps'], *self.hyper['clamp'])
        grefs, gkeep = _lib.tensor_refs(gsd, self._names[0])
        drefs, dkeep = _lib.tensor_refs(dsd, self._names[1])
        handle = C.c_void_p()
        with torch.cuda.device(self._torch_device()):
            _lib.check(_lib.lib().sbc_wgan_trainer_create(C.byref(desc), grefs, len(grefs), drefs, len(drefs), C.byref(handle)))
        self._h = handle
        self.last_batch = {}

    def _prepare(self, stream):
        import torch
        dev = self._torch_device()
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            ws = self._workspace_of(_lib.lib().sbc_wgan_trainer_workspace_floats(self._h, self.capacity), dev)
        return dev, s, ws

    def _input(self, x, shape, name, dev, s):
        import torch
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dim() == 4 and len(shape) == 1 and tuple(x.shape[2:]) == (1, 1):
            x = x[:, :, 0, 0]
        if x.dim() != 1 + len(shape) or tuple(x.shape[1:]) != shape:
            raise ValueError('%s must be [B, %s] (got %s)' % (name, ', '.join(map(str, shape)), tuple(x.shape)))
        if not 1 <= x.shape[0] <= self.capacity:
            raise ValueError('%s: a batch must hold 1 .. %d samples, the trainer\'s batch_size (got %d)' % (name, self.capacity, x.shape[0]))
        with torch.cuda.device(dev), torch.cuda.stream(s):
            return x.detach().to(dev, torch.float32).contiguous()

    def _step(self, launch, inputs, n_out, stream):
        """One iteration: ``launch(handle, (pointer, batch) of every input, out, workspace, capacity, stream)`` on ``inputs``
        ``[(array, shape of a sample, name)]`` -> (its float32 ``[n_out]`` losses on the device, the batch of every input)"""
        import torch
        dev, s, ws = self._prepare(stream)
        xs = [self._input(x, shape, name, dev, s) for x, shape, name in inputs]
        with torch.cuda.device(dev):
            with torch.cuda.stream(s):
                out = torch.empty(n_out, dtype=torch.float32, device=dev)
            args = [a for x in xs for a in (C.c_void_p(x.data_ptr()), x.shape[0])]
            _lib.check(launch(self._h, *args, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), self.capacity, C.c_void_p(s.cuda_stream)))
            for t in xs + [ws, out]:
                t.record_stream(s)
            out.record_stream(torch.cuda.current_stream(dev))
        return out, [x.shape[0] for x in xs]

    def critic_step(self, real, noise, stream=None):
        out, (b_real, b_fake) = self._step(_lib.lib().sbc_wgan_trainer_critic_step, [(real, (NC, NR, NT), 'real'), (noise, (NZ,), 'noise')], 2, stream)
        self._tracked[0] += 1
        self._tracked[1] += 2
        self.steps[1] += 1
        self.last_batch = {'g': b_fake, 'd0': b_real, 'd1': b_fake}
        return out

    def generator_step(self, noise, stream=None):
        out, (b,) = self._step(_lib.lib().sbc_wgan_trainer_generator_step, [(noise, (NZ,), 'noise')], 1, stream)
        self._tracked[0] += 1
        self._tracked[1] += 1
        self.steps[0] += 1
        self.last_batch.update({'g': b, 'd1': b})
        return out

    def stage(self, name):
        """A stage of the last call as a view of the workspace: ``[B, C, H, W]`` of the batch that wrote it, ``[C]`` for ``mean`` / ``var`` /
        ``err``; masks as int32 words (``unpack_mask``)."""
        off, c, h, w, per = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().sbc_wgan_trainer_stage(self._h, trainer_stage_id(name, self.n_extra), self.capacity, C.byref(off), C.byref(c),
                                                     C.byref(h), C.byref(w), C.byref(per)))
        if not per.value:
            return self._ws[off.value:off.value + c.value]
        return _stage_view(self._ws, off.value, self.last_batch[name.partition('.')[0]], c.value, h.value, w.value, '.mask' in name)

    def _copy(self, net, name, what, arr, to_device):
        import torch
        net_i, what_i = _NET_INDEX[net], {'value': 0, 'grad': 1, 'square_avg': 2}[what]
        with torch.cuda.device(self._torch_device()):
            _lib.check(_lib.lib().sbc_wgan_trainer_copy(self._h, net_i, what_i, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.size, int(to_device)))

    def tensor(self, net, name, what='value'):
        """Tensor ``name`` of net ``'g'`` / ``'d'`` as a numpy array: its ``'value'``, ``'grad'`` or ``'square_avg'``.  Waits for the device."""
        arr = np.empty(self._shapes[_NET_INDEX[net]][name], np.float32)
        self._copy(net, name, what, arr, False)
        return arr

    def set_tensor(self, net, name, value, what='value'):
        arr = np.ascontiguousarray(value, np.float32)
        if arr.shape != tuple(self._shapes[_NET_INDEX[net]][name]):
            raise ValueError('size mismatch for %s: %s vs %s' % (name, arr.shape, self._shapes[_NET_INDEX[net]][name]))
        self._copy(net, name, what, arr, True)

    def parameter_names(self, net):
        """The trainable tensors in ``parameters()`` order"""
        return [n for n in self._names[_NET_INDEX[net]] if not n.endswith(('running_mean', 'running_var'))]

    def state_dicts(self):
        out = []
        for i, net in enumerate('gd'):
            sd = {}
            for n, _ in (state_dict_spec, disc_state_dict_spec)[i](self.n_extra):
                sd[n] = np.asarray(self._tracked[i], np.int64) if n.endswith('num_batches_tracked') else self.tensor(net, n)
            out.append(sd)
        return tuple(out)

    def optimizer_state_dicts(self):
        """``(gen_opt_state, disc_opt_state)`` as ``torch.optim.RMSprop(...).state_dict()`` lays them out (numpy in place of tensors)"""
        out = []
        for i, net in enumerate('gd'):
            names = self.parameter_names(net)
            state = {}
            if self.steps[i]:
                state = {k: {'step': np.asarray(float(self.steps[i]), np.float32), 'square_avg': self.tensor(net, n, 'square_avg')} for k, n in enumerate(names)}
            group = dict(lr=self.hyper['lrG' if net == 'g' else 'lrD'], momentum=0, alpha=self.hyper['alpha'], eps=self.hyper['eps'], centered=False,
                         weight_decay=0, capturable=False, foreach=None, maximize=False, differentiable=False, params=list(range(len(names))))
            out.append({'state': state, 'param_groups': [group]})
        return tuple(out)


def bn_backward(gact, raw, mask_words, mean, var, weight, slope):
    """One BatchNorm backward (``sbc_wgan_bn_backward``) on device tensors -> ``(draw, dweight, dbias)``"""
    import torch
    B, Cn, H, W = gact.shape
    draw, dw, db = torch.empty_like(gact), torch.empty(Cn, dtype=torch.float32, device=gact.device), torch.empty(Cn, dtype=torch.float32, device=gact.device)
    scratch = torch.empty(2 * Cn, dtype=torch.float32, device=gact.device)
    p = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    s = torch.cuda.current_stream(gact.device)
    with torch.cuda.device(gact.device):
        _lib.check(_lib.lib().sbc_wgan_bn_backward(p(gact), p(raw), p(mask_words), p(mean), p(var), p(weight), float(slope), p(draw), p(dw), p(db),
                                                   p(scratch), B, Cn, H, W, C.c_void_p(s.cuda_stream)))
    return draw, dw, db


def wgrad128(draw, inp, ks, up):
    """``sbc_wgan_wgrad128`` on device tensors: draw ``[B, 128, H, W]``, inp ``[B, 128, H >> up, W >> up]`` -> ``[128, 128, ks, ks]``"""
    import torch
    B, _, H, W = draw.shape
    n = _lib.lib().sbc_wgan_wgrad128_scratch_floats(B, H, W, int(ks))
    if n < 0:
        raise ValueError('wgrad128: unsupported shape %s, ks %r' % (tuple(draw.shape), ks))
    scratch = torch.empty(n, dtype=torch.float32, device=draw.device)
    dW = torch.empty((NGF, NGF, ks, ks), dtype=torch.float32, device=draw.device)
    s = torch.cuda.current_stream(draw.device)
    with torch.cuda.device(draw.device):
        _lib.check(_lib.lib().sbc_wgan_wgrad128(C.c_void_p(draw.data_ptr()), C.c_void_p(inp.data_ptr()), C.c_void_p(dW.data_ptr()),
                                                C.c_void_p(scratch.data_ptr()), B, H, W, int(ks), int(up), C.c_void_p(s.cuda_stream)))
    return dW


def rmsprop(p, g, sq, lr=5e-5, alpha=0.99, eps=1e-8, clamp=None, stream=None):
    """``sbc_wgan_rmsprop`` in place on flat float32 device tensors: one RMSprop step, or with ``clamp=(lo, hi)`` the clamp alone"""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(p.device)
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None           # noqa: E731
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().sbc_wgan_rmsprop(ptr(p), ptr(g), ptr(sq), p.numel(), float(lr), float(alpha), float(eps), float(lo), float(hi),
                                               0 if clamp is not None else 1, C.c_void_p(s.cuda_stream)))
