"""torch-CPU restatement of the WGAN latent-optimisation baseline (reference: ``aux_gan.py:58-112`` ``DCGAN_G_Ours`` in eval mode and the
loop of ``test_wgan.py:145-176``), in float32 or float64, layer by layer, with an option the reference does not have: every ReLU can be
replaced by a multiplication with a GIVEN sign mask.  The gradient of the loss is not continuous in the masks (one unit whose input is
within rounding of zero moves d loss / d z by 1e-3 while the forward output does not move), so an implementation is compared with float64
UNDER ITS OWN masks, and its masks with float64's only away from zero.

    generate(sd, z, dtype, masks=None)                      -> gen [B, 2, 16, 64], pre-activations [L x [B, 128, H, W]], activations
    step_terms(sd, z, Y, P, H, lam, scale, dtype, masks)    -> dict gen, meas, reg, nmse, g (= d sum_b scale_b (meas_b + lam_b reg_b) / d z)
    adam(g_history, z0, lr, dtype, first_step, m0, v0)      -> the iterates z_1 .. z_K of torch.optim.Adam's defaults fed these gradients
    flip_state_dict / generate_flipped / *_vjp_flipped      -> the same functions in another summation order (the spatially flipped twin)
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NR, NT, NZ = 16, 64, 60
BN_EPS = 1e-5


def _t(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def n_layers(sd):
    n = 0
    while 'conv.extra_conv%d.weight' % n in sd:
        n += 1
    return 2 + n


def layer_names(k):
    """(conv, bn) state-dict prefixes of hidden layer k = 1 .. L"""
    return ('conv.conv%d' % k, 'conv.bn%d' % k) if k <= 2 else ('conv.extra_conv%d' % (k - 3), 'conv.extra_bn%d' % (k - 3))


def dense_forward(sd, z, dtype):
    """z [B, 60] -> [B, 128, 4, 16]"""
    h = F.linear(z, _t(sd['dense.dense_input.weight'], dtype), _t(sd['dense.dense_input.bias'], dtype))
    return h.view(-1, 128, NR // 4, NT // 4)


def layer_pre(sd, k, x, dtype):
    """Hidden layer k up to (not including) its ReLU: [nearest x 2 for k <= 2], convolution (+ bias), BatchNorm on running statistics in
    the reference's order (x - mean) / sqrt(var + eps) * w + b."""
    conv, bn = layer_names(k)
    if k <= 2:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    w = _t(sd[conv + '.weight'], dtype)
    b = _t(sd[conv + '.bias'], dtype) if (conv + '.bias') in sd else None
    x = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
    p = lambda name: _t(sd[bn + '.' + name], dtype)[None, :, None, None]       # noqa: E731
    return (x - p('running_mean')) / torch.sqrt(p('running_var') + BN_EPS) * p('weight') + p('bias')


def layer_forward(sd, k, x, dtype, mask=None):
    """-> (pre-activation, activation); with ``mask`` (bool [B, 128, H, W]) the ReLU is ``pre * mask``"""
    pre = layer_pre(sd, k, x, dtype)
    return pre, (torch.relu(pre) if mask is None else pre * _t(mask, dtype))


def out_forward(sd, a, dtype):
    return F.conv2d(a, _t(sd['conv.conv_out.weight'], dtype), _t(sd['conv.conv_out.bias'], dtype), padding=2)


def generate(sd, z, dtype, masks=None):
    """z [B, 60] (torch tensor of ``dtype``, or numpy) -> (gen, [pre-activations], [activations 0 .. L]); ``masks``: L bool arrays"""
    z = _t(z, dtype).reshape(-1, NZ)
    acts, pres = [dense_forward(sd, z, dtype)], []
    for k in range(1, n_layers(sd) + 1):
        pre, a = layer_forward(sd, k, acts[-1], dtype, None if masks is None else masks[k - 1])
        pres.append(pre)
        acts.append(a)
    return out_forward(sd, acts[-1], dtype), pres, acts


def _cplx(a, dtype):
    a = np.asarray(a)
    return torch.complex(_t(a.real, dtype), _t(a.imag, dtype))


def loss_terms(gen, z, Y, P, H, dtype):
    """(meas [B], reg [B], nmse [B] or None) as test_wgan.py:147-172 forms them"""
    G = torch.complex(gen[:, 0], gen[:, 1])
    R = torch.matmul(G, _cplx(P, dtype)) - _cplx(Y, dtype)
    meas = torch.sum(torch.square(torch.abs(R)), dim=(-1, -2))
    reg = torch.sum(torch.square(torch.abs(z)), dim=-1)
    nmse = None
    if H is not None:
        Hc = _cplx(H, dtype)
        nmse = torch.sum(torch.square(torch.abs(G - Hc)), dim=(-1, -2)) / torch.sum(torch.square(torch.abs(Hc)), dim=(-1, -2))
    return meas, reg, nmse


def step_terms(sd, z, Y, P, H, lam, scale, dtype, masks=None, gen_fn=None):
    """One evaluation at z [B, 60]: numpy dict gen, meas, reg, nmse, g, dG (= d loss / d gen) and the pre-activations ``pre``.
    ``gen_fn``: another evaluation order of the generator (``generate_flipped`` with ``sd`` a ``flip_state_dict``)."""
    z = _t(np.asarray(z).reshape(-1, NZ), dtype).requires_grad_(True)
    B = z.shape[0]
    lam = _t(np.broadcast_to(np.asarray(lam, np.float64), (B,)).copy(), dtype)
    scale = _t(np.broadcast_to(np.asarray(scale, np.float64), (B,)).copy(), dtype)
    gen, pres, _ = (gen_fn or generate)(sd, z, dtype, masks)
    gen.retain_grad()
    meas, reg, nmse = loss_terms(gen, z, Y, P, H, dtype)
    loss = torch.sum(scale * (meas + lam * reg))
    loss.backward()
    out = {'gen': gen, 'meas': meas, 'reg': reg, 'g': z.grad, 'dG': gen.grad}
    if nmse is not None:
        out['nmse'] = nmse
    out = {k: v.detach().numpy() for k, v in out.items()}
    out['pre'] = [p.detach().numpy() for p in pres]
    return out


def layer_vjp(sd, k, grad_out, mask, dtype):
    """d loss / d (input of layer k) from d loss / d (its activation), the ReLU being ``* mask``; layer k is linear under a fixed mask"""
    g = _t(grad_out, dtype)
    h, w = g.shape[2] // (2 if k <= 2 else 1), g.shape[3] // (2 if k <= 2 else 1)
    x = torch.zeros((g.shape[0], 128, h, w), dtype=dtype, requires_grad=True)
    _, a = layer_forward(sd, k, x, dtype, mask)
    return torch.autograd.grad(a, x, g)[0].numpy()


def out_vjp(sd, dG, dtype):
    g = _t(dG, dtype)
    x = torch.zeros((g.shape[0], 128, NR, NT), dtype=dtype, requires_grad=True)
    return torch.autograd.grad(out_forward(sd, x, dtype), x, g)[0].numpy()


def residual_vjp(gen, Y, P, scale, dtype):
    """d sum_b scale_b ||G_b P_b - Y_b||^2 / d gen for GIVEN gen [B, 2, 16, 64]"""
    x = _t(gen, dtype).clone().requires_grad_(True)
    meas, _, _ = loss_terms(x, torch.zeros((x.shape[0], NZ), dtype=dtype), Y, P, None, dtype)
    return torch.autograd.grad(torch.sum(_t(np.asarray(scale, np.float64), dtype) * meas), x)[0].numpy()


def forward_terms(sd, z, Y, P, H, dtype, gen_fn=None):
    """gen, meas, reg, nmse and the pre-activations at z, without the backward pass"""
    with torch.no_grad():
        zt = _t(np.asarray(z).reshape(-1, NZ), dtype)
        gen, pres, _ = (gen_fn or generate)(sd, zt, dtype)
        meas, reg, nmse = loss_terms(gen, zt, Y, P, H, dtype)
    return {'gen': gen.numpy(), 'meas': meas.numpy(), 'reg': reg.numpy(), 'nmse': nmse.numpy(), 'pre': [p.numpy() for p in pres]}


def dense_vjp(sd, g0, dtype):
    """[B, 128, 4, 16] -> [B, 60]"""
    return (_t(g0, dtype).reshape(-1, 8192) @ _t(sd['dense.dense_input.weight'], dtype)).numpy()


def adam(g_history, z0, lr, dtype, first_step=1, m0=None, v0=None, return_state=False):
    """The iterates z_1 .. z_K [K, ...] of ``torch.optim.Adam`` (betas 0.9 / 0.999, eps 1e-8, bias correction) started at ``z0`` and fed
    the gradients ``g_history`` [K, ...]; every operation in ``dtype``, the scalars formed in float64 first as torch forms them.
    ``lr``: a scalar or an array broadcastable against z (float64).  A run is continued with ``first_step`` (Adam's t of the first
    gradient) and the moments ``m0``, ``v0`` it had reached; ``return_state``: also the moments after the last step."""
    dt = np.dtype(dtype)
    z = np.asarray(z0, dt).copy()
    m = np.zeros_like(z) if m0 is None else np.asarray(m0, dt).copy()
    v = np.zeros_like(z) if v0 is None else np.asarray(v0, dt).copy()
    b1, b2 = 0.9, 0.999
    w1, c2, w2, eps = dt.type(1.0 - b1), dt.type(b2), dt.type(1.0 - b2), dt.type(1e-8)
    out = []
    for t, g in enumerate(np.asarray(g_history, dt), start=int(first_step)):
        m = m + (g - m) * w1
        v = v * c2 + (w2 * g) * g
        denom = np.sqrt(v) / dt.type(np.sqrt(1.0 - b2 ** t)) + eps
        step = (np.asarray(lr, np.float64) / (1.0 - b1 ** t)).astype(dt)
        z = z - step * (m / denom)
        out.append(z.copy())
    return (np.stack(out), m, v) if return_state else np.stack(out)


# ---- the flipped twin: the same function in another valid summation order ---------------------------------------------------------
# Every 5 x 5 / 3 x 3 filter flipped in its last two axes, the dense rows and bias permuted to the flipped [128, 4, 16] view, the masks
# flipped, every output flipped back.  Nearest x 2, the convolutions, BatchNorm and ReLU commute with the flip, so in exact arithmetic the
# twin is the identity; in float32 its sums run in another order.
def flip(x):
    return torch.flip(x, (-2, -1)) if isinstance(x, torch.Tensor) else np.asarray(x)[..., ::-1, ::-1].copy()


def flip_state_dict(sd):
    out = {}
    for k, v in sd.items():
        v = np.asarray(v)
        if v.ndim == 4:
            v = v[..., ::-1, ::-1].copy()
        elif k == 'dense.dense_input.weight':
            v = v.reshape(128, NR // 4, NT // 4, NZ)[:, ::-1, ::-1].reshape(-1, NZ).copy()
        elif k == 'dense.dense_input.bias':
            v = v.reshape(128, NR // 4, NT // 4)[:, ::-1, ::-1].reshape(-1).copy()
        out[k] = v
    return out


def generate_flipped(fsd, z, dtype, masks=None):
    """``generate`` through the twin; ``fsd = flip_state_dict(sd)``"""
    gen, pres, acts = generate(fsd, z, dtype, None if masks is None else [flip(np.asarray(m)) for m in masks])
    return flip(gen), [flip(p) for p in pres], [flip(a) for a in acts]


def layer_vjp_flipped(fsd, k, grad_out, mask, dtype):
    return flip(layer_vjp(fsd, k, flip(np.asarray(grad_out)), flip(np.asarray(mask)), dtype))


def out_vjp_flipped(fsd, dG, dtype):
    return flip(out_vjp(fsd, flip(np.asarray(dG)), dtype))


def dense_vjp_flipped(fsd, g0, dtype):
    return dense_vjp(fsd, flip(np.asarray(g0)), dtype)


def residual_vjp_flipped(gen, Y, P, scale, dtype):
    """the antenna axes reversed (receive rows of G and Y, transmit columns of G = rows of P): the sums over t run the other way"""
    return flip(residual_vjp(flip(np.asarray(gen)), np.asarray(Y)[:, ::-1].copy(), np.asarray(P)[:, ::-1].copy(), scale, dtype))


def normwise(a, ref):
    """per-sample norm-wise relative error, maximum over samples (axis 0 = sample)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    B = ref.shape[0]
    num = np.sqrt(np.sum(np.abs(a.reshape(B, -1) - ref.reshape(B, -1)) ** 2, axis=1))
    den = np.sqrt(np.sum(np.abs(ref.reshape(B, -1)) ** 2, axis=1))
    return float(np.max(num / den))


def synthetic_problem(B, Np, snr_db=10.0, seed=3):
    """CDL-like channels H [B, 16, 64] of unit entry variance, QPSK pilots P [B, 64, Np] and Y = H P + n [B, 16, Np] with the reference's
    noise, sqrt(noise) / sqrt(2) times a complex normal of TOTAL variance 1 (test_wgan.py:131-132), noise = 10^(-snr / 10)."""
    from score_based_channels_amd import synth
    raw = synth.generate_channels('CDL-C', max(B, 16), NT, NR, 0.5, seed)          # [N, Nr, Nt]
    H = (raw[:B] / np.std(raw)).astype(np.complex64)
    rng = np.random.default_rng(seed + 1)
    P = synth.qpsk_pilots(rng, B, NT, Np).astype(np.complex64)
    Y = H @ P
    n = (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape)) / np.sqrt(2)
    Y = Y + np.sqrt(10 ** (-snr_db / 10.)) / np.sqrt(2.) * n
    return Y.astype(np.complex64), P, H


def init_z(B):
    """The first B of the reference's ``global_init_z`` (test_wgan.py:96-97), [B, 60] float32"""
    rs = np.random.RandomState(2021)
    return rs.normal(size=(B, NZ, 1, 1)).astype(np.float32)[:, :, 0, 0]


def golden_step():
    """tests/golden/wgan_step.npz (tests/gen_golden_wgan.py) with the float64 values rebuilt from fp32 value + fp32 residual"""
    with np.load(os.path.join(GOLDEN, 'wgan_step.npz'), allow_pickle=False) as f:
        g = {k: f[k] for k in f.files}
    for k in ('gen', 'meas', 'reg', 'nmse', 'g'):
        g[k + '64'] = g[k + '32'].astype(np.float64) + g[k + '64_minus_32'].astype(np.float64)
    return g
