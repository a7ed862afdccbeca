"""CPU restatement of Learned D-AMP (the counterpart of tests/cs_oracle.py for score_based_channels_amd/ldamp.py): the FlippedNormUnet
denoiser layer by layer and the unrolled loop around it, on torch CPU tensors in a chosen dtype (float32 or float64).

Layer order (aux_unet.py of the reference): norm -> 3 x [ConvBlock, 2x2 mean pool] -> bottleneck ConvBlock -> 3 x [transposed conv
stage, concat [up, skip], ConvBlock] -> 1x1 conv + bias -> unnorm; D(x) = x - that.  ConvBlock = 2 x [conv3x3 pad 1 no bias,
InstanceNorm (biased variance, eps 1e-5, no affine), LeakyReLU 0.2].
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# stage names of score_based_channels_amd.ldamp.STAGES, with (kind, inputs, weight key suffix)
DOWN = [('d0a', 'd0', 'p0', 'down_sample_layers.0'), ('d1a', 'd1', 'p1', 'down_sample_layers.1'), ('d2a', 'd2', 'p2', 'down_sample_layers.2')]
UP = [('t0', 'u0a', 'u0', 'd2', 'up_transpose_conv.0', 'up_conv.0'), ('t1', 'u1a', 'u1', 'd1', 'up_transpose_conv.1', 'up_conv.1'),
      ('t2', 'u2a', 'u2', 'd0', 'up_transpose_conv.2', 'up_conv.2.0')]


def _t(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).to(dtype)


def conv_half(x, w):
    """conv3x3 (pad 1, no bias) -> InstanceNorm -> LeakyReLU(0.2)"""
    return F.leaky_relu(F.instance_norm(F.conv2d(x, w, padding=1), eps=1e-5), 0.2)


def pool(x):
    return F.avg_pool2d(x, 2, 2)


def tconv_stage(x, w):
    """ConvTranspose 2x2 stride 2 (no bias) -> InstanceNorm -> LeakyReLU(0.2)"""
    return F.leaky_relu(F.instance_norm(F.conv_transpose2d(x, w, stride=2), eps=1e-5), 0.2)


def norm(x):
    """per sample and plane: mean and unbiased std over the H*W entries; x [B, 2, H, W]"""
    mean = x.mean(dim=(2, 3), keepdim=True)
    std = x.std(dim=(2, 3), keepdim=True)
    return (x - mean) / std, mean, std


def final(u2, w, b, mean, std, x):
    """1x1 conv + bias, unnorm, residual: x - (conv(u2) * std + mean)"""
    return x - (F.conv2d(u2, w, b) * std + mean)


def _planes(r, dtype):
    """complex [B, 64, 16] -> real [B, 2, 64, 16]"""
    r = np.asarray(r)
    return torch.stack((_t(r.real, dtype), _t(r.imag, dtype)), dim=1)


def _cplx(x):
    a = x.numpy()
    return a[:, 0] + 1j * a[:, 1]


def denoise_planes(sd, net, x, dtype, stages=None):
    """D_net on real planes x [B, 2, 64, 16] (torch, dtype); fills ``stages`` (name -> tensor) if given."""
    W = lambda k: _t(sd['update_nets.%d.unet.%s' % (net, k)], dtype)       # noqa: E731
    st = {} if stages is None else stages
    st['x'], mean, std = norm(x)
    cur = st['x']
    for a, b, p, key in DOWN:
        st[a] = conv_half(cur, W(key + '.layers.0.weight'))
        st[b] = conv_half(st[a], W(key + '.layers.4.weight'))
        st[p] = pool(st[b])
        cur = st[p]
    st['ba'] = conv_half(cur, W('conv.layers.0.weight'))
    st['bb'] = conv_half(st['ba'], W('conv.layers.4.weight'))
    cur = st['bb']
    for t, a, b, skip, tkey, ckey in UP:
        st[t] = tconv_stage(cur, W(tkey + '.layers.0.weight'))
        st[a] = conv_half(torch.cat([st[t], st[skip]], dim=1), W(ckey + '.layers.0.weight'))
        st[b] = conv_half(st[a], W(ckey + '.layers.4.weight'))
        cur = st[b]
    st['stat'] = torch.stack((mean[:, 0, 0, 0], std[:, 0, 0, 0], mean[:, 1, 0, 0], std[:, 1, 0, 0]), dim=1)
    return final(cur, W('up_conv.2.1.weight'), W('up_conv.2.1.bias'), mean, std, x)


def denoise(sd, net, r, dtype=torch.float64, stages=None):
    """complex ndarray r [B, 64, 16] -> complex ndarray D_net(r) computed in ``dtype``"""
    with torch.no_grad():
        return _cplx(denoise_planes(sd, net, _planes(r, dtype), dtype, stages))


def run(denoiser, Y, P, eig, directions, num_unrolls, dtype=torch.float64, logs=True):
    """The unrolled loop around ``denoiser(u, planes [B, 2, 64, 16]) -> planes``.  Y [B, Np, 16], P [B, Np, 64] complex, eig [B],
    directions [U, B, 64, 16, 2] (arrays, or tensors on the device to compute on).  Returns per-unroll logs as numpy arrays: h [U, B, 64, 16],
    z [U, B, Np, 16] complex, div, eps [U, B]; with ``logs=False`` only the last h, as a tensor."""
    ctype = torch.complex64 if dtype == torch.float32 else torch.complex128
    with torch.no_grad():
        y, Pm, e = _t(Y, ctype), _t(P, ctype), _t(eig, dtype)
        h = torch.zeros(y.shape[0], Pm.shape[-1], y.shape[-1], dtype=ctype, device=y.device)
        z = y
        log = {'h': [], 'z': [], 'div': [], 'eps': []}
        for u in range(num_unrolls):
            r = h + 1 / e[:, None, None] * torch.matmul(Pm.transpose(-1, -2).conj(), z)
            rr = torch.view_as_real(r)                                   # [B, 64, 16, 2]
            d = _t(directions[u], dtype)
            hr = denoiser(u, rr.permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous()
            eps = torch.clamp(torch.amax(torch.abs(r), dim=(-1, -2)) * 1e-3, min=1e-5)
            rp = rr + eps[:, None, None, None] * d
            hp = denoiser(u, rp.permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous()
            div = 1 / eps * torch.mean(d * (hp - hr), dim=(-1, -2, -3))
            h = torch.view_as_complex(hr)
            z = y - torch.matmul(Pm, h) + z * div[:, None, None]
            if logs:
                for k, v in (('h', h), ('z', z), ('div', div), ('eps', eps)):
                    log[k].append(v.cpu().numpy().copy())
        return {k: np.stack(v) for k, v in log.items()} if logs else h


def run_oracle(sd, Y, P, eig, directions, num_unrolls, dtype=torch.float64):
    return run(lambda u, x: denoise_planes(sd, u, x, dtype), Y, P, eig, directions, num_unrolls, dtype)


# ---- the flipped twin: the same function in another valid summation order ---------------------------------------------------------
# Every filter flipped in its last two axes, the input flipped, the output flipped back.  Every operation of the net commutes with the
# flip (the statistics are over whole planes, the 2 x 2 pool and the stride-2 transposed convolution tile even extents), so in exact
# arithmetic the twin is the identity; in float32 its sums run in another order and it gives different bits.
def flip(x):
    return torch.flip(x, (-2, -1))


def flip_state_dict(sd):
    return {k: (v[..., ::-1, ::-1].copy() if np.ndim(v) == 4 else v) for k, v in sd.items()}


def twin(layer):
    """a layer function f(x, ..., w) -> f on flipped tensors, flipped back (every >= 3-D tensor argument is flipped)"""
    def f(*args):
        return flip(layer(*[flip(a) if (isinstance(a, torch.Tensor) and a.dim() >= 3 and a.shape[-1] * a.shape[-2] > 1) else a for a in args]))
    return f


def denoise_planes_flipped(fsd, net, x, dtype, stages=None):
    """``denoise_planes`` through the twin; ``fsd = flip_state_dict(sd)``"""
    st = {}
    out = flip(denoise_planes(fsd, net, flip(x).contiguous(), dtype, st))
    if stages is not None:
        stages.update({k: (v if k == 'stat' else flip(v)) for k, v in st.items()})
    return out


def run_oracle_flipped(fsd, Y, P, eig, directions, num_unrolls, dtype=torch.float32):
    return run(lambda u, x: denoise_planes_flipped(fsd, u, x, dtype), Y, P, eig, directions, num_unrolls, dtype)


# ---- the error measure of the tests ---------------------------------------------------------------------------------------------
def normwise(a, ref):
    """per-sample norm-wise relative error, maximum over samples (axis 0 = sample)"""
    a, ref = np.asarray(a), np.asarray(ref)
    B = ref.shape[0]
    num = np.sqrt(np.sum(np.abs(a.reshape(B, -1) - ref.reshape(B, -1)) ** 2, axis=1))
    den = np.sqrt(np.sum(np.abs(ref.reshape(B, -1)) ** 2, axis=1))
    return float(np.max(num / den))


def absolute(a, ref):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64))))


def synthetic_problem(B, Np, snr_db=10.0, seed=11):
    """A loader-shaped problem without the loader: CDL-like channels, QPSK pilots, (Y_herm, P_herm, eig1, H_herm_cplx)."""
    from score_based_channels_amd import synth
    raw = synth.generate_channels('CDL-C', max(B, 16), 64, 16, 0.5, seed)        # [N, Nr, Nt]
    h = (raw[:B] / np.std(raw)).astype(np.complex64)
    rng = np.random.default_rng(seed + 1)
    pil = synth.qpsk_pilots(rng, B, 64, Np).astype(np.complex64)                    # [B, Nt, Np]
    y = h @ pil
    sigma = 10 ** (-snr_db / 20.) * np.sqrt(64) / np.sqrt(2)
    y = y + sigma * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    herm = lambda a: np.conj(np.transpose(a, (0, 2, 1)))                            # noqa: E731
    eig = np.array([np.linalg.eigvalsh(p @ np.conj(p.T))[-1] for p in pil], np.float32)          # largest eigenvalue of P P^H
    return herm(y).astype(np.complex64), herm(pil).astype(np.complex64), eig, herm(h).astype(np.complex64)


# ---- fixtures of tests/gen_golden_ldamp.py (the float64 values are stored as fp32 value + fp32 residual) ---------------------------
def _load(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def golden_unroll():
    g, g64 = _load('ldamp_unroll.npz'), _load('ldamp_unroll_f64.npz')
    g['directions'] = g['directions'].astype(np.float32)
    g['h64'] = g['h32'].astype(np.complex128) + g64['h64_minus_h32'].astype(np.complex128)
    g['z64'] = g['z32'].astype(np.complex128) + g64['z64_minus_z32'].astype(np.complex128)
    g['div64'], g['eps64'] = g64['div64'], g64['eps64']
    return g


def golden_unet():
    g = _load('ldamp_unet.npz')
    g['out64'] = g['out32'].astype(np.complex128) + g['out64_minus_out32'].astype(np.complex128)
    return g
