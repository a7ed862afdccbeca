"""Operands for the conv-family launches whose mathematically exact result is known.  Test infrastructure only:
numpy and torch, no GPU and no library needed.

Every operand is a multiple of a power-of-two quantum and small, so that every product and every partial sum of the launch -- in any
order, through Winograd F(2x2,3x3), through the one-, two- and three-term 16-bit operand forms, the pooled filters and the mean pool --
is exactly representable in fp32.  A kernel must then return the float64 result bit for bit: there is no tolerance to choose.

Families
  int    activations in -8..8 (0..8 where an ELU sits in front of the matrix cores: ELU is the identity there), weights in -2..2
         with a third of them zero, integer biases and residual operands, dyadic statistics (mu an integer <= min x where an ELU
         follows, scale in {1, 2, 0.5}, shift a non-negative integer), sigmas powers of two;
  lo-x   activations a + b 2^-11 (a in 0..2, b in -1..1) against integer weights in -1..1: a nonzero LOW term of the activation split;
  lo-w   integer activations in -2..2 against weights {-1,0,1} + {-1,0,1} 2^-12: a nonzero low (middle) term of the weight forms;
         (never both: the two-term form drops lo x lo by design)
  pool   planes for the 5x5 max pool: negative everywhere, one spike on a negative ramp (its window puts the maximum at each of the
         25 offsets), ties, random; images smaller than the window.

Every builder returns a record whose ``expected`` is float64, computed here with shifted slices and float64 matrix products, and
whose ``span`` -- the largest magnitude any staged, accumulated or written value can reach, over the smallest quantum in play (for a
Winograd form: the bound on the Winograd-domain sums over q_x q_w / 4) -- is asserted to be below 2^22: a factor four under
fp32's 24 bits.  The span is a condition of the case, not a tolerance; the ranges (and the number of nonzero taps per output channel)
are chosen so that it holds.
"""
import zlib
from types import SimpleNamespace

import numpy as np

F32 = np.float32
SPAN_LIMIT = 2.0 ** 22
FAMILIES = ('int', 'lo-x', 'lo-w')
LO_ALGOS = ('direct', 'bf16x3', 'f16x2')          # the algorithms the low-term families run on (direct forms only)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _t(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).double()


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def conv64(v, w, bias=None, dil=1):
    """float64 cross-correlation, stride 1, zero padding dil * (k // 2): NHWC tensor ``v``, torch-layout weight ``w`` [O, C, k, k],
    as k * k matrix products over shifted views (every term is exact for the operands of this module, so is any order of them)."""
    import torch
    B, H, W, C = v.shape
    k = w.shape[2]
    p = dil * (k // 2)
    vp = torch.zeros((B, H + 2 * p, W + 2 * p, C), dtype=torch.float64, device=v.device)
    vp[:, p:p + H, p:p + W] = v
    out = _valid_conv(vp, w, dil)
    if bias is not None:
        out += bias
    return out


def elu64(v):
    import torch
    return torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0.0)))


def meanpool64(v):
    return 0.25 * (v[:, ::2, ::2] + v[:, 1::2, ::2] + v[:, ::2, 1::2] + v[:, 1::2, 1::2])


def maxpool64(v, pad=-np.inf):
    """5 x 5 maximum, stride 1, of an NHWC tensor padded with ``pad`` (-inf: nn.MaxPool2d; the mutation check pads with 0)."""
    import torch
    B, H, W, C = v.shape
    vp = torch.full((B, H + 4, W + 4, C), pad, dtype=v.dtype, device=v.device)
    vp[:, 2:2 + H, 2:2 + W] = v
    out = vp[:, 0:H, 0:W].clone()
    for i in range(5):
        for j in range(5):
            out = torch.maximum(out, vp[:, i:i + H, j:j + W])
    return out


def norm64(x, stats):
    """(x - mu) * scale + shift with ``stats`` [B, 3, C]"""
    return (x - stats[:, None, None, 0]) * stats[:, None, None, 1] + stats[:, None, None, 2]


# ---------------------------------------------------------------------------------------------------------------- operand builders
_WINO_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)


def wino_u(w):
    return np.einsum('ij,ocjk,lk->ocil', _WINO_G, np.asarray(w, np.float64), _WINO_G)


def sparse_weight(rng, cout, cin, k, values, n_nz):
    """[cout, cin, k, k] float32 with exactly ``n_nz`` taps per output channel drawn from ``values`` (none of them 0), the rest 0."""
    taps = cin * k * k
    n_nz = int(max(1, min(n_nz, taps)))
    rank = np.argsort(rng.random((cout, taps)), axis=1)
    w = np.zeros((cout, taps), np.float64)
    vals = rng.choice(np.asarray(values, np.float64), size=(cout, n_nz))
    np.put_along_axis(w, rank[:, :n_nz], vals, axis=1)
    return w.reshape(cout, cin, k, k).astype(F32)


def dyadic_stats(rng, x, elu, scales=(1.0, 2.0, 0.5), max_shift=3):
    """[B, 3, C] (mu, scale, shift): mu an integer (<= the plane's minimum where an ELU follows), scale a power of two, shift a
    non-negative integer -- (x - mu) * scale + shift is exact and, with ``elu``, never negative."""
    B, C = x.shape[0], x.shape[-1]
    lo = np.floor(x.min(axis=(1, 2)).astype(np.float64))
    mu = lo - rng.integers(0, 3, (B, C)) if elu else rng.integers(-3, 4, (B, C)).astype(np.float64)
    scale = rng.choice(np.asarray(scales, np.float64), size=(B, C))
    shift = rng.integers(0, max_shift + 1, (B, C)).astype(np.float64)
    return np.stack((mu, scale, shift), axis=1).astype(F32)


def activations(rng, shape, family, nonneg):
    if family == 'lo-x':
        a = rng.integers(0, 3, shape)
        b = rng.integers(-1, 2, shape)
        if nonneg:
            b = np.where(a == 0, np.abs(b), b)
        return (a + b * 2.0 ** -11).astype(F32)
    if family == 'lo-w':
        return rng.integers(0 if nonneg else -2, 3, shape).astype(F32)
    return rng.integers(0 if nonneg else -8, 9, shape).astype(F32)


def conv_weight(rng, cout, cin, k, family, amax, q_out, extra=0.0):
    """The family's weight with as many nonzero taps per output channel as the span allows: amax * sum |w| + extra < 0.9 * 2^22 q_out."""
    taps = cin * k * k
    if family == 'lo-w':
        hi = np.array([-1.0, 0.0, 1.0])[:, None] + np.array([-1.0, 0.0, 1.0])[None, :] * 2.0 ** -12
        values, wmax = [v for v in hi.ravel() if abs(v) > 0.5], 1 + 2.0 ** -12
    elif family == 'lo-x':
        values, wmax = [-1.0, 1.0], 1.0
    else:
        values, wmax = [-2.0, -1.0, 1.0, 2.0], 2.0
    budget = int((0.9 * SPAN_LIMIT * q_out - extra) / (amax * wmax))
    assert budget >= 4, 'no room for a convolution inside the span'
    return sparse_weight(rng, cout, cin, k, values, min(2 * taps // 3, budget))


def _quantum(family):
    return {'int': (1.0, 1.0), 'lo-x': (2.0 ** -11, 1.0), 'lo-w': (1.0, 2.0 ** -12)}[family]


def _check_span(case):
    assert case.span < SPAN_LIMIT, ('span %g is not below 2^22' % case.span, case.name)
    return case


def low_term_fraction(a, shift=0):
    """Fraction of the elements of ``a`` whose fp16 two-term split (after scaling by 2^shift) has a nonzero low term."""
    from score_based_channels_amd.weights import split_f16x2
    return float((split_f16x2(np.ldexp(np.asarray(a, F32), shift))[1] != 0).mean())


# ---------------------------------------------------------------------------------------------------------------- SBC_OP_CONV
def conv_case(cin, cout, k, dil, B, H, W, mode, family='int', device='cpu', wino=False, mutate=None):
    """One SBC_OP_CONV record of tests/test_gpu_ops.py's CONV_PARAMS (same shape, batch and flag set ``mode``; ``wino``: the span is
    taken in the Winograd domain as well) with exact operands.  ``mutate`` (CPU mutation checks) changes the REFERENCE only:
    'drop_tap' (the tap (0, 1) is not added at the image's last row), 'transpose_tap' (w[kh][kw] -> w[kw][kh]), 'res_before_elu',
    'norm_on_padding' (the zero padding is normalised too), 'drop_hi_lo' / 'drop_lo_hi' (a missing cross term of the operand split)."""
    import torch
    mode = mode.replace('_top', '')
    assert 'selfnorm' not in mode and mode != 'up_2x', 'inexact by construction: left on their tolerance tests'
    elu, norm, pool, crp = 'elu' in mode, 'norm' in mode, 'pool' in mode, mode == 'crp2'
    rng = _rng('conv', cin, cout, k, dil, B, H, W, mode, family)
    q_x, q_w = _quantum(family)
    x = activations(rng, (B, H, W, cin), family, nonneg=elu and not norm)
    stats = None
    v = x.astype(np.float64)
    if norm:
        stats = dyadic_stats(rng, x, elu) if family == 'int' else dyadic_stats(rng, x, elu, scales=(1.0, 2.0), max_shift=1)
        v = norm64(v, stats.astype(np.float64))
    amax = float(np.abs(v).max())
    if elu:
        assert v.min() >= 0                                            # ELU is the identity on every staged value
    q_out = q_x * q_w / (4 if (pool or wino) else 1)
    w = conv_weight(rng, cout, cin, k, family, amax * (4 if wino else 1) * (2.25 if wino else 1), q_out, extra=64.0)
    bias = rng.integers(-4, 5, cout).astype(F32) if not crp else None
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    res1 = res2 = up = None
    if 'res' in mode:
        res1 = rng.integers(-8, 9, (B, Ho, Wo, cout)).astype(F32)
    if crp:
        res1 = rng.integers(0, 9, (B, Ho, Wo, cout)).astype(F32)      # ELU'd in the epilogue: the identity
        res2 = rng.integers(-8, 9, (B, Ho, Wo, cout)).astype(F32)
    if mode == 'up_same':
        up = rng.integers(-8, 9, (B, H, W, cout)).astype(F32)

    # the reference, float64
    tv, tw = _t(x, device), _t(w, device)
    if norm and mutate != 'norm_on_padding':
        tv = norm64(tv, _t(stats, device))
    if mutate == 'transpose_tap':
        tw = tw.transpose(2, 3)
    if mutate in ('drop_hi_lo', 'drop_lo_hi'):
        from score_based_channels_amd.weights import f16x2_shift, split_f16x2
        s = f16x2_shift(w)
        xh, xl = (_t(t.astype(F32), device) for t in split_f16x2(tv.cpu().numpy().astype(F32)))
        wh, wl = (_t(np.ldexp(t.astype(np.float64), -s), device) for t in split_f16x2(np.ldexp(w, s).astype(F32)))
        y = conv64(xh, wh, None, dil) + (conv64(xl, wh, None, dil) if mutate == 'drop_hi_lo' else conv64(xh, wl, None, dil))
    elif mutate == 'norm_on_padding':
        p = dil * (k // 2)
        xp = torch.zeros((B, H + 2 * p, W + 2 * p, cin), dtype=torch.float64, device=device)
        xp[:, p:p + H, p:p + W] = tv
        xp = norm64(xp, _t(stats, device))                             # the padding becomes (0 - mu) * scale + shift
        y = _valid_conv(elu64(xp) if elu else xp, tw, dil)
    else:
        if elu:
            tv = elu64(tv)
        y = conv64(tv, tw, None, dil)
    if mutate == 'drop_tap':                                           # the last row does not get its tap (kh, kw) = (0, 1)
        assert k == 3 and H - 1 - dil >= 0
        y[:, H - 1] -= tv[:, H - 1 - dil] @ tw[:, :, 0, 1].t()
    if bias is not None:
        y = y + _t(bias, device)
    if pool:
        y = meanpool64(y)
    if res1 is not None:
        r = _t(res1, device)
        if crp:
            r = elu64(r)
        if res2 is not None:
            r = _t(res2, device) + r
        if mutate == 'res_before_elu':
            y = elu64(y + _t(res1, device)) + _t(res2, device)
        else:
            y = y + r
    if up is not None:
        y = y + _t(up, device)
    span = (amax * float(np.abs(w).reshape(cout, -1).sum(1).max()) + 64.0) / q_out      # (64: bias and residual operands)
    if wino:
        u = wino_u(w)
        span = max(span, 4 * amax * float(np.abs(u).sum(1).max()) / (q_x * q_w / 4))
    return _check_span(SimpleNamespace(name=('conv', cin, cout, k, dil, B, H, W, mode, family), x=x, w=w, bias=bias, stats=stats, res1=res1,
                                       res2=res2, up=up, mode=mode, expected=y, span=span, q=q_out, amax=amax, dil=dil))


def _valid_conv(xp, w, dil):
    """float64 convolution WITHOUT padding of an already padded NHWC tensor"""
    import torch
    B, Hp, Wp, C = xp.shape
    k = w.shape[2]
    H, W = Hp - 2 * dil * (k // 2), Wp - 2 * dil * (k // 2)
    out = torch.zeros((B, H, W, w.shape[0]), dtype=torch.float64, device=xp.device)
    for i in range(k):
        for j in range(k):
            out += xp[:, i * dil:i * dil + H, j * dil:j * dil + W] @ w[:, :, i, j].t()
    return out


# ---------------------------------------------------------------------------------------------------------------- pool planes
def pool_planes(rng, B, H, W, C, nonneg=False):
    """[B, H, W, C] float32 integers, one kind of plane per (sample, channel) in turn: negative everywhere (random), a single spike on a
    negative ramp (the spike's 5 x 5 neighbourhood sees it at each of the 25 window offsets), ties (two values only), random signed.
    ``nonneg`` lifts everything by 30 (an ELU behind the pool is then the identity; the order of the values is what a maximum sees)."""
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ramp = -1.0 - ((3 * hh + 5 * ww) % 29)
    x = np.empty((B, H, W, C), F32)
    kind = (np.arange(B)[:, None] * 3 + np.arange(C)[None, :]) % 4
    x[:] = rng.integers(-8, 9, (B, H, W, C))
    neg = rng.integers(-9, 0, (B, H, W, C)).astype(F32)
    ties = rng.integers(-3, -1, (B, H, W, C)).astype(F32)
    sp = ramp[None, :, :, None].repeat(B, 0).repeat(C, 3).astype(F32)
    sh, sw = rng.integers(0, H, (B, C)), rng.integers(0, W, (B, C))
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing='ij')
    sp[bi, sh, sw, ci] = 7.0
    for kd, src in ((0, neg), (1, sp), (2, ties)):
        m = (kind == kd)[:, None, None, :]
        x = np.where(m, src, x)
    return (x + (30.0 if nonneg else 0.0)).astype(F32)


def maxpool_case(C, B, H, W, elu, device='cpu', specials=True):
    """SBC_OP_MAXPOOL5: the pool family; without ELU any float is exact under a maximum, so +-inf, the largest and the smallest fp32
    numbers and denormals are planted too.  With ``elu`` the planes are lifted to where ELU is the identity."""
    rng = _rng('maxpool', C, B, H, W, elu)
    x = pool_planes(rng, B, H, W, C, nonneg=elu)
    if specials and not elu:
        flat = x.reshape(-1)
        idx = rng.choice(flat.size, size=min(12, flat.size), replace=False)
        vals = np.array([np.inf, -np.inf, 3.4028235e38, -3.4028235e38, 1e-45, -1e-45, 1.17549435e-38, -0.0, 0.0, 2.0 ** -30, -2.0 ** -30, 1.5], F32)
        flat[idx] = vals[:idx.size]
        if B * C >= 2:
            x[-1, :, :, -1] = -np.inf                                  # a plane of -inf: the padding value itself
    y = maxpool64(_t(x, device))
    return SimpleNamespace(name=('maxpool', C, B, H, W, elu), x=x, expected=y, span=64.0)


def conv_pool_case(B, H, stage, device='cpu', mutate=None):
    """SBC_OP_CONV_POOL, W = 16, 32 channels: ``pool_elu`` = conv(ELU(maxpool(x))) on non-negative planes (ELU the identity),
    ``pool_crp2`` = conv(maxpool(x)) + (res2 + ELU(res1)) on the signed pool family: an all-negative window pools to a negative
    number, which a pool padded with 0 (``mutate='pad0'``) cannot return."""
    W, C = 16, 32
    elu = stage == 'pool_elu'
    rng = _rng('conv_pool', B, H, stage)
    x = pool_planes(rng, B, H, W, C, nonneg=elu)
    amax = float(np.abs(x).max())
    w = conv_weight(rng, C, C, 3, 'int', amax, 1.0, extra=64.0)
    res1 = res2 = None
    v = maxpool64(_t(x, device), pad=0.0 if mutate == 'pad0' else -np.inf)
    if elu:
        assert float(v.min()) >= 0
        v = elu64(v)
    y = conv64(v, _t(w, device))
    if not elu:
        res1 = rng.integers(0, 9, (B, H, W, C)).astype(F32)
        res2 = rng.integers(-8, 9, (B, H, W, C)).astype(F32)
        y = y + (_t(res2, device) + elu64(_t(res1, device)))
    span = amax * float(np.abs(w).reshape(C, -1).sum(1).max()) + 64.0
    return _check_span(SimpleNamespace(name=('conv_pool', B, H, stage), x=x, w=w, res1=res1, res2=res2, expected=y, span=span, amax=amax))


# ---------------------------------------------------------------------------------------------------------------- fused kinds
def pair_case(B, H, W, C=32, device='cpu'):
    """SBC_OP_CONV_PAIR, out = x + conv2(ELU(conv1(ELU(x)))): x in 0..8, conv1 with 24 taps of 1 or 2 per output channel (the
    intermediate is a non-negative integer of at most 384 <= 2048: fp16-exact, ELU the identity), conv2 signed."""
    rng = _rng('pair', B, H, W, C)
    x = rng.integers(0, 9, (B, H, W, C)).astype(F32)
    w1 = sparse_weight(rng, C, C, 3, [1.0, 2.0], 24)
    tmax = 8.0 * float(np.abs(w1).reshape(C, -1).sum(1).max())
    assert tmax <= 2048
    w2 = sparse_weight(rng, C, C, 3, [-2.0, -1.0, 1.0, 2.0], 2 * C * 9 // 3)
    tx = _t(x, device)
    t = conv64(elu64(tx), _t(w1, device))
    assert float(t.min()) >= 0 and float(t.max()) <= 2048
    y = tx + conv64(elu64(t), _t(w2, device))
    span = tmax * float(np.abs(w2).reshape(C, -1).sum(1).max()) + 8.0
    return _check_span(SimpleNamespace(name=('pair', B, H, W, C), x=x, w1=w1, w2=w2, expected=y, span=span, tmax=tmax))


def conv_down_case(cin, cout, H, W, B, device='cpu'):
    """SBC_OP_CONV_DOWN: meanpool2(conv3x3(ELU(norm(a))) + b3) + meanpool2(conv1x1(x) + b1); the pooled filters are quarter-integers."""
    rng = _rng('down', cin, cout, H, W, B)
    a = rng.integers(-8, 9, (B, H, W, cin)).astype(F32)
    x = rng.integers(-8, 9, (B, H, W, cin)).astype(F32)
    st = dyadic_stats(rng, a, True)
    v = norm64(a.astype(np.float64), st.astype(np.float64))
    assert v.min() >= 0
    amax = float(v.max())
    w3 = conv_weight(rng, cout, cin, 3, 'int', amax, 0.25, extra=256.0)
    w1 = conv_weight(rng, cout, cin, 1, 'int', 8.0, 0.25, extra=256.0)
    b3, b1 = rng.integers(-4, 5, cout).astype(F32), rng.integers(-4, 5, cout).astype(F32)
    tv = elu64(norm64(_t(a, device), _t(st, device)))
    y = meanpool64(conv64(tv, _t(w3, device), _t(b3, device))) + meanpool64(conv64(_t(x, device), _t(w1, device), _t(b1, device)))
    span = (amax * float(np.abs(w3).reshape(cout, -1).sum(1).max()) + 8.0 * float(np.abs(w1).reshape(cout, -1).sum(1).max()) + 16.0) / 0.25
    return _check_span(SimpleNamespace(name=('down', cin, cout, H, W, B), a=a, x=x, stats=st, w3=w3, w1=w1, b3=b3, b1=b1, expected=y, span=span))


CHAIN_BLOCKS = [('R',), ('C',), ('R', 'R'), ('C', 'R'), ('R', 'R', 'C', 'R')]


def chain_reference(tx, blocks, ws, pad=-np.inf):
    """RCU ('R') and CRP ('C') blocks in sequence, float64 (layers.py:76-83, 126-134)."""
    out = tx
    for tok, (w1, w2) in zip(blocks, ws):
        if tok == 'R':
            t = conv64(elu64(out), w1)
            out = out + conv64(elu64(t), w2)
        else:
            out = elu64(out)
            path = conv64(maxpool64(out, pad), w1)
            out = path + out
            path = conv64(maxpool64(path, pad), w2)
            out = path + out
    return out


def chain_case(Cc, H, W, B, blocks, device='cpu', mutate=None):
    """SBC_OP_CHAIN over RCU / CRP blocks: x in 0..8 (0..2 for more than two blocks) and three taps per output channel, so that up to
    eight convolutions stay inside the span and every staged activation inside the two-term form's range (below 16000 at act_scale 1).
    Every tensor that meets an ELU is a non-negative integer (non-negative weights); the LAST block's weights are signed where no ELU
    follows them: the second convolution of an RCU block, both convolutions of a CRP block -- the second pool of a final CRP block
    then sees negative planes (``mutate='pad0'``: the reference pools with 0 padding)."""
    rng = _rng('chain', Cc, H, W, B, blocks)
    xmax = 8 if len(blocks) <= 2 else 2
    x = rng.integers(0, xmax + 1, (B, H, W, Cc)).astype(F32)
    ws, bound, staged = [], float(xmax), 0.0
    for kblk, tok in enumerate(blocks):
        last = kblk == len(blocks) - 1
        pos, sgn = [1.0], [-1.0, 1.0]
        w1 = sparse_weight(rng, Cc, Cc, 3, sgn if (last and tok == 'C') else pos, 3)
        w2 = sparse_weight(rng, Cc, Cc, 3, sgn if last else pos, 3)
        ws.append((w1, w2))
        staged = max(staged, 3.0 * bound)                              # what the block's second convolution stages
        bound = bound * 10.0 if tok == 'R' else bound * 13.0          # R: x + 3 * 3 x; C: x + 3 x + 9 x
    assert staged < 16000
    tx = _t(x, device)
    tws = [(_t(a, device), _t(b, device)) for a, b in ws]
    y = chain_reference(tx, blocks, tws, pad=0.0 if mutate == 'pad0' else -np.inf)
    return _check_span(SimpleNamespace(name=('chain', Cc, H, W, B, blocks), x=x, ws=ws, expected=y, span=bound, staged=staged))


def begin_case(B, H, W, device='cpu'):
    """SBC_OP_BEGIN_CONV: conv3x3(2 x - 1) + bias, 2 -> 32 channels, weights in torch layout"""
    rng = _rng('begin', B, H, W)
    x = rng.integers(-8, 9, (B, H, W, 2)).astype(F32)
    w = rng.integers(-2, 3, (32, 2, 3, 3)).astype(F32)
    b = rng.integers(-4, 5, 32).astype(F32)
    y = conv64(2.0 * _t(x, device) - 1.0, _t(w, device), _t(b, device))
    return _check_span(SimpleNamespace(name=('begin', B, H, W), x=x, w=w, bias=b, expected=y, span=17.0 * 36 + 4))


def end_case(B, H, W, device='cpu'):
    """SBC_OP_END_CONV (stats given): conv3x3(ELU(norm(x))) + bias, 32 -> 2 channels, divided by sigma[label] -- powers of two."""
    rng = _rng('end', B, H, W)
    x = rng.integers(-8, 9, (B, H, W, 32)).astype(F32)
    st = dyadic_stats(rng, x, True)
    w = rng.integers(-2, 3, (2, 32, 3, 3)).astype(F32)
    b = rng.integers(-4, 5, 2).astype(F32)
    sigmas = (2.0 ** np.arange(5, -12, -1)).astype(F32)                 # 32 ... 2^-11
    labels = rng.integers(0, sigmas.size, B).astype(np.int64)
    tv = elu64(norm64(_t(x, device), _t(st, device)))
    assert float(tv.min()) >= 0
    y = conv64(tv, _t(w, device), _t(b, device)) / _t(sigmas[labels], device)[:, None, None, None]
    span = float(tv.max()) * 2 * 288 + 4                                # in units of the output's own quantum (a power of two per sample)
    return _check_span(SimpleNamespace(name=('end', B, H, W), x=x, stats=st, w=w, bias=b, sigmas=sigmas, labels=labels, expected=y, span=span))


# ---------------------------------------------------------------------------------------------------------------- ELU probes
ELU_BANDS = ((-3, 4), (-10, -5), (-16, -11))                           # |v| log-uniform in [2^lo, 2^hi]
_M = float(np.float32(-0.03125))
ELU_PLANTED = np.array([0.0, -0.0, _M, np.nextafter(F32(_M), F32(0)), np.nextafter(F32(_M), F32(-1)), 3e-4, -3e-4, -20.0, -90.0], F32)


def elu_probe_values(shape, band, limit=None, key=0):
    """float32 [B >= 2, ...] of both signs, |v| log-uniform in the band.  Sample 0 holds nothing else (the library's calibration looks at
    the first sample: its staged maximum is the band's); the samples behind it also hold the planted values -- zeros, the polynomial's
    switch point and its two fp32 neighbours, +-3e-4 where the error of exp(x) - 1 meets x^2 / 2, and two inputs deep in the saturated
    tail -- three times each.  ``limit``: plant only values with |ELU(v)| <= limit (a two-term fp16 layer calibrated on the band
    overflows, and says so, 31 x above the band's maximum)."""
    rng = _rng('elu', tuple(shape), tuple(band), key)
    lo, hi = band
    v = (np.exp2(rng.uniform(lo, hi, shape)) * rng.choice([-1.0, 1.0], shape)).astype(F32)
    staged = np.where(ELU_PLANTED > 0, ELU_PLANTED, np.expm1(np.minimum(ELU_PLANTED.astype(np.float64), 0)))
    planted = ELU_PLANTED if limit is None else ELU_PLANTED[np.abs(staged) <= limit]
    flat = v[1:].reshape(-1)
    pos = rng.choice(flat.size, size=3 * planted.size, replace=False)
    flat[pos] = np.tile(planted, 3)
    return v


def elu_bound(v, form, s=None):
    """The derived bound on |kernel ELU(v) - expm1-ELU(v)| per element, float64 array.
    ``form``: 'fast' (exp(x) - 1 on the hardware exponential) or 'acc' (SBC_PRO_ELU_ACC); ``s``: the layer's act_scale where the value
    then passes through the two-term fp16 split (None: fp32 / three-bf16 staging, which is exact)."""
    v = np.asarray(v, np.float64)
    y = np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    rep = np.maximum(2.0 ** -22 * np.abs(y), 2.0 ** -25 / s) if s is not None else np.zeros_like(v)
    absb = np.full_like(v, 2.0 ** -23)
    b = np.where(v >= 0, 0.0, absb)
    if form == 'acc':
        b = np.where((v < 0) & (v > -0.03125), 2.0 ** -22 * np.abs(y), b)
    return b + rep


def identity_filter(C, k=3):
    w = np.zeros((C, C, k, k), F32)
    w[np.arange(C), np.arange(C), k // 2, k // 2] = 1.0
    return w
