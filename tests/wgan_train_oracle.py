"""torch-CPU restatement of WGAN training (reference: ``train_wgan.py:123-184`` on ``aux_gan.py`` ``DCGAN_G_Ours`` and ``DCGAN_D`` in TRAINING
mode), in float32 or float64, layer by layer, with the option of ``wgan_oracle.py``: every ReLU / LeakyReLU can be replaced by a
multiplication with a GIVEN sign mask.  Training-mode BatchNorm couples the whole batch, so one flipped unit moves every upstream
gradient: an implementation is compared with float64 UNDER ITS OWN masks, and its masks with float64's only away from zero.

    g_forward(gsd, z, dtype, masks)            -> dict raw, mean, var, pre, act (lists over k = 0 .. L), gen; tensors stay in the graph
    d_forward(dsd, x, dtype, masks)            -> dict raw, mean, var, pre, act (lists over j = 0 .. M), err
    critic_terms / generator_terms             -> losses, parameter gradients, stages of one iteration (numpy)
    layer_backward / conv_wgrad / conv_dgrad   -> single backward launches on given operands
    rmsprop / clamp / running_update           -> the optimiser step (pinned to torch.optim.RMSprop), the weight clamp, the running statistics
    flipped(...)                               -> the same quantities in another summation order (the spatially flipped twin)
"""
import numpy as np
import torch
import torch.nn.functional as F

from wgan_oracle import NR, NT, NZ, _t, flip, flip_state_dict, layer_names, n_layers

BN_EPS = 1e-5
MOMENTUM = 0.1
SLOPE_D = 0.2


def _act(pre, mask, slope, dtype):
    if mask is None:
        return F.leaky_relu(pre, slope) if slope else torch.relu(pre)
    m = _t(np.asarray(mask), dtype)
    return pre * (m + (1 - m) * slope)


def bn_train(raw, w, b):
    """BatchNorm on batch statistics in the reference's order -> (pre, mean, biased var)"""
    mean = raw.mean(dim=(0, 2, 3))
    var = raw.var(dim=(0, 2, 3), unbiased=False)
    s = (None, slice(None), None, None)
    return (raw - mean[s]) / torch.sqrt(var[s] + BN_EPS) * w[s] + b[s], mean, var


def g_forward(gsd, z, dtype, masks=None):
    z = _t(z, dtype).reshape(-1, NZ)
    a = F.linear(z, _t(gsd['dense.dense_input.weight'], dtype), _t(gsd['dense.dense_input.bias'], dtype)).view(-1, 128, NR // 4, NT // 4)
    out = {k: [None] for k in ('raw', 'mean', 'var', 'pre')}
    out['act'] = [a]
    for k in range(1, n_layers(gsd) + 1):
        conv, bn = layer_names(k)
        x = a.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if k <= 2 else a
        w = _t(gsd[conv + '.weight'], dtype)
        raw = F.conv2d(x, w, _t(gsd[conv + '.bias'], dtype) if conv + '.bias' in gsd else None, padding=w.shape[-1] // 2)
        pre, mean, var = bn_train(raw, _t(gsd[bn + '.weight'], dtype), _t(gsd[bn + '.bias'], dtype))
        a = _act(pre, None if masks is None else masks[k - 1], 0.0, dtype)
        for key, v in (('raw', raw), ('mean', mean), ('var', var), ('pre', pre), ('act', a)):
            out[key].append(v)
    out['gen'] = F.conv2d(a, _t(gsd['conv.conv_out.weight'], dtype), _t(gsd['conv.conv_out.bias'], dtype), padding=2)
    return out


def d_n_extra(dsd):
    n = 0
    while 'main.extra-layers-%d:64:conv.weight' % n in dsd:
        n += 1
    return n


def d_layer_table(n_extra):
    """[(conv prefix, batchnorm prefix or None, stride, padding)] for layers 0 .. M"""
    t = [('main.initial:2-64:conv', None, 2, 1)]
    t += [('main.extra-layers-%d:64:conv' % i, 'main.extra-layers-%d:64:batchnorm' % i, 1, 1) for i in range(n_extra)]
    return t + [('main.pyramid:64-128:conv', 'main.pyramid:128:batchnorm', 2, 1), ('main.final:128-1:conv', None, 1, 0)]


def d_forward(dsd, x, dtype, masks=None):
    a = _t(x, dtype) if not isinstance(x, torch.Tensor) else x
    table = d_layer_table(d_n_extra(dsd))
    out = {k: [] for k in ('raw', 'mean', 'var', 'pre', 'act')}
    for j, (conv, bn, stride, pad) in enumerate(table):
        raw = F.conv2d(a, _t(dsd[conv + '.weight'], dtype), None, stride=stride, padding=pad)
        out['raw'].append(raw)
        if j == len(table) - 1:
            break
        pre, mean, var = bn_train(raw, _t(dsd[bn + '.weight'], dtype), _t(dsd[bn + '.bias'], dtype)) if bn else (raw, None, None)
        a = _act(pre, None if masks is None else masks[j], SLOPE_D, dtype)
        for key, v in (('mean', mean), ('var', var), ('pre', pre), ('act', a)):
            out[key].append(v)
    out['err'] = out['raw'][-1].mean(0).view(1)
    return out


def _leaves(sd, dtype, trainable_only=True):
    """the state dict with its trainable tensors as autograd leaves"""
    out = {}
    for k, v in sd.items():
        t = _t(np.asarray(v), dtype) if not k.endswith('num_batches_tracked') else None
        if t is not None and not k.endswith(('running_mean', 'running_var')):
            t.requires_grad_(True)
        if t is not None:
            out[k] = t
    return out


def _np(v):
    if isinstance(v, list):
        return [None if t is None else t.detach().numpy() for t in v]
    return v.detach().numpy()


def _grads(leaves):
    return {k: v.grad.detach().numpy() for k, v in leaves.items() if v.requires_grad and v.grad is not None}


def critic_terms(gsd, dsd, real, noise, dtype, masks=None):
    """One critic iteration up to the optimiser: D's parameters are taken AS GIVEN (clamp them first).  ``masks``: dict ``g``, ``d0``, ``d1`` of lists.
    -> dict errD_real, errD_fake, grads {name: array}, g / d0 / d1 stages"""
    masks = masks or {}
    D = _leaves(dsd, dtype)
    d0 = d_forward(D, _t(real, dtype), dtype, masks.get('d0'))
    d0['err'].backward(torch.ones(1, dtype=dtype))
    with torch.no_grad():
        g = g_forward(gsd, noise, dtype, masks.get('g'))
    d1 = d_forward(D, g['gen'].detach(), dtype, masks.get('d1'))
    d1['err'].backward(-torch.ones(1, dtype=dtype))
    return {'errD_real': _np(d0['err']), 'errD_fake': _np(d1['err']), 'grads': _grads(D), 'g': {k: _np(v) for k, v in g.items()},
            'd0': {k: _np(v) for k, v in d0.items()}, 'd1': {k: _np(v) for k, v in d1.items()}}


def generator_terms(gsd, dsd, noise, dtype, masks=None):
    """One generator iteration up to the optimiser -> dict errG, grads (G's parameters), dgen, g / d1 stages"""
    masks = masks or {}
    G = _leaves(gsd, dtype)
    g = g_forward(G, noise, dtype, masks.get('g'))
    g['gen'].retain_grad()
    d1 = d_forward({k: _t(np.asarray(v), dtype) for k, v in dsd.items() if not k.endswith('num_batches_tracked')}, g['gen'], dtype, masks.get('d1'))
    d1['err'].backward(torch.ones(1, dtype=dtype))
    return {'errG': _np(d1['err']), 'grads': _grads(G), 'dgen': g['gen'].grad.numpy(), 'g': {k: _np(v) for k, v in g.items()},
            'd1': {k: _np(v) for k, v in d1.items()}}


def flipped_state(sd):
    return flip_state_dict({k: v for k, v in sd.items() if not k.endswith('num_batches_tracked')})


def flipped_masks(masks):
    return None if masks is None else {k: [flip(np.asarray(m)) for m in v] for k, v in masks.items()}


def _unflip(stages):
    one = lambda a: flip(a) if (a is not None and np.ndim(a) == 4) else a           # noqa: E731
    return {k: ([one(a) for a in v] if isinstance(v, list) else one(v)) for k, v in stages.items()}


def critic_terms_flipped(gsd, dsd, real, noise, dtype, masks=None):
    """``critic_terms`` through the spatially flipped twin (another summation order, the same function in exact arithmetic): losses and
    gradients only, the gradients flipped back"""
    r = critic_terms(flipped_state(gsd), flipped_state(dsd), flip(np.asarray(real)), noise, dtype, flipped_masks(masks))
    return {'errD_real': r['errD_real'], 'errD_fake': r['errD_fake'], 'grads': flip_state_dict(r['grads']), 'g': _unflip(r['g']), 'd0': _unflip(r['d0']),
            'd1': _unflip(r['d1'])}


def generator_terms_flipped(gsd, dsd, noise, dtype, masks=None):
    r = generator_terms(flipped_state(gsd), flipped_state(dsd), noise, dtype, flipped_masks(masks))
    return {'errG': r['errG'], 'grads': flip_state_dict(r['grads']), 'dgen': flip(r['dgen']), 'g': _unflip(r['g']), 'd1': _unflip(r['d1'])}


# ---- single launches on given operands ------------------------------------------------------------------------------------------------
def layer_backward(gact, raw, mask, w, slope, dtype, bn=True):
    """d loss / d raw, d loss / d (BatchNorm weight), d loss / d (BatchNorm bias) from gact = d loss / d act, the activation being ``* (mask ?
    1 : slope)`` and the statistics those of ``raw``"""
    x = _t(raw, dtype).clone().requires_grad_(True)
    if not bn:
        a = _act(x, mask, slope, dtype)
        return torch.autograd.grad(a, x, _t(gact, dtype))[0].numpy(), None, None
    ww = _t(w, dtype).clone().requires_grad_(True)
    bb = torch.zeros_like(ww).requires_grad_(True)
    pre, _, _ = bn_train(x, ww, bb)
    gx, gw, gb = torch.autograd.grad(_act(pre, mask, slope, dtype), (x, ww, bb), _t(gact, dtype))
    return gx.numpy(), gw.numpy(), gb.numpy()


def conv_wgrad(draw, inp, wshape, stride, pad, up, dtype):
    """d loss / d weight of ``conv2d([nearest x 2] inp, weight, stride, pad)`` from d loss / d output"""
    x = _t(inp, dtype)
    if up:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    w = torch.zeros(tuple(wshape), dtype=dtype, requires_grad=True)
    return torch.autograd.grad(F.conv2d(x, w, None, stride=stride, padding=pad), w, _t(draw, dtype))[0].numpy()


def conv_dgrad(draw, w, in_shape, stride, pad, up, dtype):
    """d loss / d input of the same convolution (through the nearest x 2 map with ``up``)"""
    x = torch.zeros(tuple(in_shape), dtype=dtype, requires_grad=True)
    xx = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if up else x
    return torch.autograd.grad(F.conv2d(xx, _t(w, dtype), None, stride=stride, padding=pad), x, _t(draw, dtype))[0].numpy()


def dense_wgrad(g0, z, dtype):
    g = _t(g0, dtype).reshape(-1, 8192)
    return (g.t() @ _t(z, dtype).reshape(-1, NZ)).numpy(), g.sum(0).numpy()


def spatial_twin(fn, arrays, flip_out=True):
    """``fn`` on spatially flipped 4-D operands, the 4-D results flipped back: the other float32 order of a single launch"""
    out = fn(*[flip(np.asarray(a)) if np.ndim(a) == 4 else a for a in arrays])
    one = not isinstance(out, tuple)
    out = tuple(flip(o) if (o is not None and np.ndim(o) == 4) else o for o in ((out,) if one else out))
    return out[0] if one else out


# ---- optimiser, clamp, running statistics -----------------------------------------------------------------------------------------------
def _fma(a, b, c, dt):
    """round(a * b + c) with ONE rounding for float32 operands (the product is exact in the wider type; on x86 long double has 64 mantissa
    bits, which leaves a double rounding one chance in 2^40); plain arithmetic in float64"""
    if dt != np.float32:
        return a * b + c
    wide = np.longdouble if np.finfo(np.longdouble).nmant > 52 else np.float64
    return (a.astype(wide) * b.astype(wide) + c.astype(wide)).astype(np.float32)


def rmsprop(p, g, sq, lr=5e-5, alpha=0.99, eps=1e-8, dtype=np.float32):
    """One step of ``torch.optim.RMSprop``'s defaults (no momentum, not centred) in ``dtype``, in the order torch's CPU kernels use:
    ``sq = fma((1 - alpha) g, g, sq alpha)`` (``mul_`` then ``addcmul_``, which fuses), ``avg = sqrt(sq) + eps``, ``p = p + (-lr g) / avg``
    (``addcdiv_``).  The scalars are formed in float64 first.  -> (p, sq)"""
    dt = np.dtype(dtype).type
    p, g, sq = (np.asarray(a, dt) for a in (p, g, sq))
    s = _fma(dt(1.0 - alpha) * g, g, sq * dt(alpha), dt)
    avg = np.sqrt(s) + dt(eps)
    return (p + (dt(-lr) * g) / avg).astype(dt), s.astype(dt)


def clamp(p, lo=-0.01, hi=0.01, dtype=np.float32):
    dt = np.dtype(dtype).type
    return np.minimum(np.maximum(np.asarray(p, dt), dt(lo)), dt(hi))


def running_update(running_mean, running_var, mean, var, n, dtype=np.float64):
    """nn.BatchNorm2d in training mode: momentum 0.1, the unbiased variance of the n = B H W values"""
    dt = np.dtype(dtype).type
    unbiased = np.asarray(var, np.float64) * (n / (n - 1.0))
    return ((1 - MOMENTUM) * np.asarray(running_mean, dt) + MOMENTUM * np.asarray(mean, dt),
            (1 - MOMENTUM) * np.asarray(running_var, dt) + MOMENTUM * unbiased.astype(dt))


def normwise_all(a, ref):
    """norm-wise relative error over the whole tensor"""
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))
