"""Differentiable restatement of the project's own oracle -- test infrastructure, NOT product code.

``oracle/ncsnv2_oracle.py::score_forward`` and ``oracle/dsm_oracle.py::perturb`` / ``loss_per_sample`` restated with
``torch.nn.functional`` primitives in a dtype of the caller's choice, so that torch's autograd supplies the gradient of the
denoising-score-matching loss with respect to every parameter.  float64 is the reference the training kernels are held to
(tests/test_gpu_train_autograd.py); the same code in float32 measures how far an honest fp32 evaluation of the same
operation sits from float64 ("e_ref").  tests/test_train_autograd_cpu.py ties the restatement to the numpy oracle (forward)
and to the reference project's own autograd (the digests of tests/golden/train_dsm.npz).

Layout is NCHW, names are the checkpoint's, block by block as the oracle (which cites the reference lines).
"""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
PLAN = [('res1', None, None), ('res2', 'down', None), ('res3', 'down', None), ('res31', 'down', None), ('res4', 'down', 2),
        ('res5', 'down', 4)]


def conv2d(x, w, b=None, dilation=1):
    return F.conv2d(x, w, b, padding=dilation * (w.shape[2] // 2), dilation=dilation)


def instance_norm_plus(x, alpha, gamma, beta):
    """ncsnv2_oracle.instance_norm_plus: biased per-plane variance, unbiased variance of the plane means across channels."""
    means = x.mean(dim=(2, 3))
    m = means.mean(dim=-1, keepdim=True)
    v = means.var(dim=-1, keepdim=True, unbiased=True)
    means_n = (means - m) / torch.sqrt(v + 1e-5)
    mu = means[:, :, None, None]
    var = ((x - mu) ** 2).mean(dim=(2, 3), keepdim=True)
    h = (x - mu) / torch.sqrt(var + 1e-5)
    h = h + means_n[:, :, None, None] * alpha[None, :, None, None]
    return gamma[None, :, None, None] * h + beta[None, :, None, None]


def max_pool5(x):
    return F.max_pool2d(x, 5, 1, 2)


def _axis(inp, out, dtype):
    """ncsnv2_oracle.bilinear_align_corners.axis: the source coordinate is a float32 product of a float32 scale (what torch's
    fp32 kernel and the HIP kernel compute); the interpolation weights derived from it are exact in either dtype."""
    scale = F32(inp - 1) / F32(out - 1) if out > 1 else F32(0)
    src = (scale * np.arange(out, dtype=F32)).astype(F32)
    i0 = np.minimum(np.floor(src).astype(np.int64), inp - 1)
    i1 = np.minimum(i0 + 1, inp - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l0).to(dtype), torch.from_numpy(l1).to(dtype)


def bilinear_align_corners(x, size):
    h, w = x.shape[2:]
    oh, ow = int(size[0]), int(size[1])
    if (oh, ow) == (h, w):
        return x
    h0, h1, lh0, lh1 = _axis(h, oh, x.dtype)
    w0, w1, lw0, lw1 = _axis(w, ow, x.dtype)
    xh0, xh1 = x[:, :, h0], x[:, :, h1]
    top = xh0[:, :, :, w0] * lw0 + xh0[:, :, :, w1] * lw1
    bot = xh1[:, :, :, w0] * lw0 + xh1[:, :, :, w1] * lw1
    return lh0[None, None, :, None] * top + lh1[None, None, :, None] * bot


def mean_pool2(x):
    return (((x[:, :, ::2, ::2] + x[:, :, 1::2, ::2]) + x[:, :, ::2, 1::2]) + x[:, :, 1::2, 1::2]) / 4.


def _norm(p, prefix, x):
    return instance_norm_plus(x, p[prefix + 'alpha'], p[prefix + 'gamma'], p[prefix + 'beta'])


def residual_block(p, prefix, x, resample, dilation):
    d = 1 if dilation is None else dilation
    pooled = resample == 'down' and dilation is None
    out = F.elu(_norm(p, prefix + 'normalize1.', x))
    out = conv2d(out, p[prefix + 'conv1.weight'], p[prefix + 'conv1.bias'], d)
    out = F.elu(_norm(p, prefix + 'normalize2.', out))
    if pooled:
        out = mean_pool2(conv2d(out, p[prefix + 'conv2.conv.weight'], p[prefix + 'conv2.conv.bias']))
        shortcut = mean_pool2(conv2d(x, p[prefix + 'shortcut.conv.weight'], p[prefix + 'shortcut.conv.bias']))
    else:
        out = conv2d(out, p[prefix + 'conv2.weight'], p[prefix + 'conv2.bias'], d)
        if (prefix + 'shortcut.weight') in p:
            shortcut = conv2d(x, p[prefix + 'shortcut.weight'], p[prefix + 'shortcut.bias'], d)
        else:
            shortcut = x
    return shortcut + out


def rcu_block(p, prefix, x, n_blocks, n_stages=2):
    for i in range(n_blocks):
        residual = x
        for j in range(n_stages):
            x = conv2d(F.elu(x), p[prefix + '%d_%d_conv.weight' % (i + 1, j + 1)])
        x = x + residual
    return x


def crp_block(p, prefix, x, n_stages=2):
    x = F.elu(x)
    path = x
    for i in range(n_stages):
        path = conv2d(max_pool5(path), p[prefix + 'convs.%d.weight' % i])
        x = path + x
    return x


def msf_block(p, prefix, xs, shape):
    sums = None
    for i, xi in enumerate(xs):
        h = conv2d(xi, p[prefix + 'convs.%d.weight' % i], p[prefix + 'convs.%d.bias' % i])
        h = bilinear_align_corners(h, shape)
        sums = h if sums is None else sums + h
    return sums


def refine_block(p, prefix, xs, shape, end=False):
    hs = [rcu_block(p, prefix + 'adapt_convs.%d.' % i, xi, 2) for i, xi in enumerate(xs)]
    h = msf_block(p, prefix + 'msf.', hs, shape) if len(xs) > 1 else hs[0]
    h = crp_block(p, prefix + 'crp.', h)
    return rcu_block(p, prefix + 'output_convs.', h, 3 if end else 1)


def score_forward(p, x, used_sigmas):
    """ncsnv2_oracle.score_forward on torch tensors: ``p`` name -> tensor, ``x [B, 2, Nt, Nr]``, ``used_sigmas [B]``."""
    out = conv2d(2 * x - 1., p['begin_conv.weight'], p['begin_conv.bias'])
    layers = []
    for name, resample, dil in PLAN:
        out = residual_block(p, name + '.0.', out, resample, dil)
        out = residual_block(p, name + '.1.', out, None, dil)
        layers.append(out)
    l1, l2, l3, l31, l4, l5 = layers
    ref1 = refine_block(p, 'refine1.', [l5], l5.shape[2:])
    ref2 = refine_block(p, 'refine2.', [l4, ref1], l4.shape[2:])
    ref31 = refine_block(p, 'refine31.', [l31, ref2], l31.shape[2:])
    ref3 = refine_block(p, 'refine3.', [l3, ref31], l3.shape[2:])
    ref4 = refine_block(p, 'refine4.', [l2, ref3], l2.shape[2:])
    out = refine_block(p, 'refine5.', [l1, ref4], l1.shape[2:], end=True)
    out = F.elu(_norm(p, 'normalizer.', out))
    out = conv2d(out, p['end_conv.weight'], p['end_conv.bias'])
    return out / used_sigmas.reshape(-1, 1, 1, 1)


def parameters(sd, dtype, requires_grad=True):
    """The 229 trainable tensors of a numpy state dict as leaves of ``dtype`` (``sigmas`` is a buffer, not a parameter)."""
    return {k: torch.from_numpy(np.array(v, F32)).to(dtype).requires_grad_(requires_grad) for k, v in sd.items() if k != 'sigmas'}


def dsm_loss(p, sigmas, x, labels, z, anneal_power=2.):
    """dsm_oracle.perturb + the network + dsm_oracle.loss_per_sample.  The perturbed samples and the noise are formed in
    float32 exactly as the oracle (and SBC_OP_DSM_PERTURB) forms them -- they are the float32 INPUT of the network and of the
    loss -- and everything behind them runs in the dtype of ``p``.  Returns (scores, per-sample loss) as torch tensors."""
    dtype = next(iter(p.values())).dtype
    used = np.asarray(sigmas, F32)[np.asarray(labels)]
    noise = (np.asarray(z, F32) * used.reshape(-1, 1, 1, 1)).astype(F32)
    pert = (np.asarray(x, F32) + noise).astype(F32)
    us = torch.from_numpy(used).to(dtype)
    scores = score_forward(p, torch.from_numpy(pert).to(dtype), us)
    B = scores.shape[0]
    target = (-1 / us.reshape(B, 1) ** 2) * torch.from_numpy(noise).to(dtype).reshape(B, -1)
    d = scores.reshape(B, -1) - target
    return scores, 0.5 * (d * d).sum(dim=-1) * us ** anneal_power


def loss_and_grads(sd, x, labels, z, anneal_power=2., grad_scale=1., dtype=torch.float64):
    """``sd``: numpy state dict under the checkpoint's names (with ``sigmas``); ``x``, ``z`` ``[B, 2, Nt, Nr]``.
    Returns (scores ``[B, 2, Nt, Nr]``, per-sample loss ``[B]``, {name: d(mean loss * grad_scale) / d(parameter)}) as numpy
    arrays of ``dtype`` -- the names are those of ``TrainNet.grad_dict()``."""
    p = parameters(sd, dtype)
    scores, per = dsm_loss(p, sd['sigmas'], x, labels, z, anneal_power)
    (per.mean() * grad_scale).backward()
    return scores.detach().numpy(), per.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()}


def forward(sd, x, labels, dtype=torch.float64):
    """The scores alone (no perturbation): what ``ncsnv2_oracle.score_forward(sd, x, labels)`` computes."""
    with torch.no_grad():
        p = parameters(sd, dtype, requires_grad=False)
        us = torch.from_numpy(np.asarray(sd['sigmas'], F32)[np.asarray(labels)]).to(dtype)
        return score_forward(p, torch.from_numpy(np.asarray(x, F32)).to(dtype), us).numpy()


# ----------------------------------------------------------------------------------------------------------- comparison
def gradient_errors(got, ref):
    """The metric of test_gpu_train.py::test_parameter_gradients_match_reference_autograd over EVERY element: per tensor the
    norm ratio ``| |got| / |ref| - 1 |`` and ``max |got - ref| / max(max |ref|, |ref|_2 / sqrt(size))``.
    Returns (worst norm error, its tensor, worst element error, its tensor); a non-finite tensor counts as infinitely wrong."""
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))[:5]
    wn, we = (0.0, ''), (0.0, '')
    for name in ref:
        g, r = np.asarray(got[name], np.float64), np.asarray(ref[name], np.float64)
        assert g.shape == r.shape, name
        if not np.isfinite(g).all():
            return float('inf'), name, float('inf'), name
        nr = np.sqrt(np.sum(r * r))
        en = abs(np.sqrt(np.sum(g * g)) / nr - 1)
        ee = np.max(np.abs(g - r)) / max(np.max(np.abs(r)), nr / np.sqrt(r.size))
        if en > wn[0]:
            wn = (float(en), name)
        if ee > we[0]:
            we = (float(ee), name)
    return wn[0], wn[1], we[0], we[1]
