"""The conv-family kernels on inputs whose exact answer is known (tests/exact_cases.py), through the C ABI
(``sbc_op_launch``) on guarded operands.

(a) Bit for bit.  Small-integer (and integer + one low term) operands make every product and every partial sum exact in fp32 in any
    order, so every algorithm of every kind must return the float64 reference itself: no tolerance.  The records are the ones
    tests/test_gpu_ops.py launches (same shapes, batches, tags and weight forms), so the same kernel instantiations are selected.
(b) Element by element.  With identity filters a launch moves single activations around its prologue and epilogue: every ELU site is
    held to float64 expm1 with bounds derived from IEEE rounding and the hardware exponential's stated accuracy (exact_cases.elu_bound).
"""
import ctypes as C

import numpy as np
import pytest

import exact_cases as X
from guarded import current as _G, dev as _dev, out as _out
from test_gpu_ops import CONV_PARAMS, PAIR_CASES, _guard, _launch, _p, gpu   # noqa: F401  (fixtures and helpers of the operator tests)

pytestmark = pytest.mark.gpu

F32 = np.float32


def _assert_exact(torch, out, expected, what=''):
    got = out.double()
    if not torch.equal(got, expected):
        bad = got != expected
        first = [int(i) for i in torch.nonzero(bad)[0]]
        d = (got - expected)[bad & torch.isfinite(got) & torch.isfinite(expected)].abs()
        raise AssertionError('%s: %d of %d elements differ from the exact result, first at %s (got %r, exact %r), largest finite difference %g'
                             % (what, int(bad.sum()), bad.numel(), first, float(got[tuple(first)]), float(expected[tuple(first)]),
                                float(d.max()) if d.numel() else float('nan')))


def _bind_conv_weight(torch, P, op, algo, w, flags, calibrated=False):
    """The weight forms of ``algo`` on a CONV record, as test_conv_matches_oracle binds them (``calibrated``: sbc_f16x2_calibrate is
    going to write the trailers of the f16x2 forms)."""
    from score_based_channels_amd import weights as Wt
    v32 = lambda a: a.view(np.float32)                                                  # noqa: E731
    keep = []

    def up(a, inout=False):
        keep.append(_dev(torch, a, None, inout))
        return _p(keep[-1])
    if algo in ('direct', 'winograd', 'winograd_bf16x3', 'winograd_raw_f16w'):
        op.weight = up(Wt.pack_conv_weight(w))
    if algo == 'winograd_raw_f16w':
        op.weight_wino_split, op.flags = up(v32(Wt.pack_conv_weight_winograd_f16(w))), flags | P.CONV_F16W
    if algo == 'winograd':
        op.weight_wino = up(Wt.pack_conv_weight_winograd(w))
    if algo == 'winograd_bf16x3':
        op.weight_wino_split = up(v32(Wt.pack_conv_weight_winograd_split(w)))
    if algo == 'bf16x3':
        op.weight_split = up(v32(Wt.pack_conv_weight_split(w)))
    if algo in ('f16w', 'winograd_f16w'):
        op.weight_split, op.flags = up(v32(Wt.pack_conv_weight_f16(w))), flags | P.CONV_F16W
    if algo == 'winograd_f16w':
        op.weight_wino_split = up(v32(Wt.pack_conv_weight_winograd_f16(w)))
    if algo in ('f16x2', 'winograd_f16x2'):
        op.weight_split, op.flags = up(v32(Wt.pack_conv_weight_f16x2(w)), calibrated), flags | P.CONV_F16X2
    if algo == 'winograd_f16x2':
        op.weight_wino_split = up(v32(Wt.pack_conv_weight_winograd_f16x2(w)), calibrated)
    return keep


# ======================================================================================================================== (a) bit for bit
def _exact_conv_params():
    out = []
    for cin, cout, k, dil, B, H, W, mode, algo in CONV_PARAMS:
        if 'selfnorm' in mode or mode == 'up_2x':
            continue                                  # statistics of the launch's own input / the bilinear x2 weights: inexact by construction
        if algo.startswith('winograd') and (k != 3 or dil != 1):
            continue
        for fam in X.FAMILIES if algo in X.LO_ALGOS else ('int',):
            out.append((cin, cout, k, dil, B, H, W, mode, algo, fam))
    return out


@pytest.mark.parametrize('cin,cout,k,dil,B,H,W,mode,algo,family', _exact_conv_params())
def test_conv_is_exact(gpu, cin, cout, k, dil, B, H, W, mode, algo, family):
    """SBC_OP_CONV, every (case, algorithm) of test_conv_matches_oracle that is exact by construction, on the int family -- and, for
    the direct forms, with a nonzero low term on the activation side (lo-x) and on the weight side (lo-w)."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    c = X.conv_case(cin, cout, k, dil, B, H, W, mode, family, device='cuda', wino=algo.startswith('winograd'))
    flags = ((P.PRO_NORM if c.stats is not None else 0) | (P.PRO_ELU if 'elu' in c.mode else 0) | (P.EPI_POOL if 'pool' in c.mode else 0)
             | (P.EPI_RES1_ELU if c.mode == 'crp2' else 0) | (P.EPI_UP if c.up is not None else 0))
    d = {n: _dev(torch, a, n) for n, a in dict(x=c.x, bias=c.bias, stats=c.stats, res1=c.res1, res2=c.res2, up=c.up).items() if a is not None}
    out = _out(tuple(c.expected.shape), 'out')
    op = _lib.sbc_op(kind=P.CONV, flags=flags, B=B, H=H, W=W, cin=cin, cout=cout, ksize=k, dil=dil, in_=_p(d['x']), out=_p(out))
    for name in ('bias', 'stats', 'res1', 'res2', 'up'):
        if name in d:
            setattr(op, name, _p(d[name]))
    if c.up is not None:
        op.up_h, op.up_w = H, W
    if mode.endswith('_top'):
        op.tag = 1
    keep = _bind_conv_weight(torch, P, op, algo, c.w, flags)
    _lib.range_flag()
    _launch(gpu, op)
    assert _lib.range_flag() == 0
    _assert_exact(torch, out, c.expected, 'conv %s %s' % (algo, family))
    del keep


# (32- / 64-pixel rows and 64 channels: the pair kernel exists in the fp16-weight mode only)
PAIR_PARAMS = [(c, m) for c in PAIR_CASES for m in ('f16x2', 'f16w') if m == 'f16w' or (c[2] < 32 and len(c) == 3)]


@pytest.mark.parametrize('case,mode', PAIR_PARAMS)
def test_conv_pair_is_exact(gpu, case, mode):
    """SBC_OP_CONV_PAIR: the tile-at-a-time kernel, the row-ring kernel (1024 tiles and more) and its sub-1024 pieces."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.weights import pack_conv_weight_f16, pack_conv_weight_f16x2
    B, H, W = case[:3]
    Cc = case[3] if len(case) > 3 else 32
    c = X.pair_case(B, H, W, Cc, device='cuda')
    pack, flag = (pack_conv_weight_f16x2, P.CONV_F16X2) if mode == 'f16x2' else (pack_conv_weight_f16, P.CONV_F16W)
    dx = _dev(torch, c.x)
    d1, d2 = _dev(torch, pack(c.w1).view(np.float32)), _dev(torch, pack(c.w2).view(np.float32))
    _lib.range_flag()

    def run(lo, hi):
        out = _out((hi - lo, H, W, Cc))
        _launch(gpu, _lib.sbc_op(kind=P.CONV_PAIR, flags=flag, B=hi - lo, H=H, W=W, cin=Cc, cout=Cc, ksize=3, dil=1, in_=_p(dx[lo:hi]),
                                 out=_p(out), weight_split=_p(d1), weight2_split=_p(d2)))
        return out
    _assert_exact(torch, run(0, B), c.expected, 'pair')
    assert _lib.range_flag() == 0
    if W == 16 and Cc == 32 and B * (H // 8) >= 1024:
        piece = 1023 // (H // 8)
        for lo in sorted({0, ((B - 1) // piece) * piece}):                # the first and the last (ragged) piece
            _assert_exact(torch, run(lo, min(lo + piece, B)), c.expected[lo:lo + piece], 'pair piece at %d' % lo)


@pytest.mark.parametrize('mode', ['f16x2', 'f16w'])
@pytest.mark.parametrize('stage', ['pool_elu', 'pool_crp2'])
@pytest.mark.parametrize('B,H', [(3, 64), (130, 64), (600, 64), (1, 8), (5, 16), (37, 24)])
def test_conv_pool_is_exact(gpu, B, H, stage, mode):
    """SBC_OP_CONV_POOL on the pool family: planes that are negative everywhere (a pool padded with 0 returns 0 at the border),
    single spikes, ties."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.weights import pack_conv_weight_f16, pack_conv_weight_f16x2
    c = X.conv_pool_case(B, H, stage, device='cuda')
    pack, mflag = (pack_conv_weight_f16x2, P.CONV_F16X2) if mode == 'f16x2' else (pack_conv_weight_f16, P.CONV_F16W)
    flags = (P.PRO_ELU if stage == 'pool_elu' else P.EPI_RES1_ELU) | mflag
    dx, dw = _dev(torch, c.x), _dev(torch, pack(c.w).view(np.float32))
    out = _out(c.x.shape)
    op = _lib.sbc_op(kind=P.CONV_POOL, flags=flags, B=B, H=H, W=16, cin=32, cout=32, ksize=3, dil=1, in_=_p(dx), out=_p(out), weight_split=_p(dw))
    if c.res1 is not None:
        keep = [_dev(torch, c.res1), _dev(torch, c.res2)]
        op.res1, op.res2 = _p(keep[0]), _p(keep[1])
    _lib.range_flag()
    _launch(gpu, op)
    assert _lib.range_flag() == 0
    _assert_exact(torch, out, c.expected, 'conv_pool')


MAXPOOL_SHAPES = [(32, 3, 64, 16, True), (64, 5, 16, 4, False), (128, 9, 8, 2, True), (64, 4, 32, 8, True), (32, 2, 32, 8, False), (32, 1, 256, 64, True),
                  (64, 2, 128, 32, False), (128, 3, 32, 16, True), (32, 2, 48, 24, True),
                  (32, 3, 8, 2, False), (32, 2, 2, 2, False), (64, 3, 2, 2, True)]          # images smaller than the window


@pytest.mark.parametrize('C_,B,H,W,elu', MAXPOOL_SHAPES)
def test_maxpool5_is_exact(gpu, C_, B, H, W, elu):
    """SBC_OP_MAXPOOL5: a maximum is exact for any float -- the pool family with +-inf, the extreme fp32 numbers, denormals and a plane
    of -inf (the padding value itself); with SBC_PRO_ELU, planes lifted to where ELU is the identity."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    for with_elu in ((False, True) if elu else (False,)):
        c = X.maxpool_case(C_, B, H, W, with_elu, device='cuda')
        dx = _dev(torch, c.x)
        out = _out(c.x.shape, must_write=with_elu)                  # (infinite results are part of the case: the comparison catches an unwritten NaN)
        _launch(gpu, _lib.sbc_op(kind=P.MAXPOOL5, flags=P.PRO_ELU if with_elu else 0, B=B, H=H, W=W, cin=C_, cout=C_, in_=_p(dx), out=_p(out)))
        _assert_exact(torch, out, c.expected, 'maxpool5 elu=%s' % with_elu)


@pytest.mark.parametrize('B', [1, 3, 40])
@pytest.mark.parametrize('cin,cout,H,W', [(32, 64, 64, 16), (32, 64, 16, 16), (64, 64, 32, 8), (64, 64, 16, 8)])
def test_conv_down_is_exact(gpu, cin, cout, H, W, B):
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.weights import pack_conv_weight_pooled_f16x2
    c = X.conv_down_case(cin, cout, H, W, B, device='cuda')
    da, dx, dst = _dev(torch, c.a), _dev(torch, c.x), _dev(torch, c.stats)
    d3, d1 = _dev(torch, pack_conv_weight_pooled_f16x2(c.w3).view(np.float32)), _dev(torch, pack_conv_weight_pooled_f16x2(c.w1).view(np.float32))
    db3, db1 = _dev(torch, c.b3), _dev(torch, c.b1)
    out = _out((B, H // 2, W // 2, cout))
    _lib.range_flag()
    _launch(gpu, _lib.sbc_op(kind=P.CONV_DOWN, flags=P.CONV_F16X2, B=B, H=H, W=W, cin=cin, cout=cout, ksize=3, dil=1, in_=_p(da), out=_p(out),
                             res1=_p(dx), stats=_p(dst), weight_split=_p(d3), weight2_split=_p(d1), bias=_p(db3), bias2=_p(db1)))
    assert _lib.range_flag() == 0
    _assert_exact(torch, out, c.expected, 'conv_down')


def _chain_record(torch, _lib, blocks, ws, inout=False):
    from score_based_channels_amd.weights import pack_conv_weight_f16x2
    keep = []
    ch = _lib.sbc_chain(n_blocks=len(blocks))
    for k, (tok, (w1, w2)) in enumerate(zip(blocks, ws)):
        ch.type[k] = {'R': 0, 'C': 1}[tok]
        keep += [_dev(torch, pack_conv_weight_f16x2(w1).view(np.float32), None, inout), _dev(torch, pack_conv_weight_f16x2(w2).view(np.float32), None, inout)]
        ch.w1[k], ch.w2[k] = keep[-2].data_ptr(), keep[-1].data_ptr()
    return ch, keep


@pytest.mark.parametrize('blocks', X.CHAIN_BLOCKS, ids=['-'.join(b) for b in X.CHAIN_BLOCKS])
@pytest.mark.parametrize('B', [1, 8, 13, 203])
@pytest.mark.parametrize('Cc,H,W', [(64, 8, 2), (128, 8, 2), (64, 16, 4), (32, 32, 8), (64, 32, 8)])
def test_chain_is_exact(gpu, Cc, H, W, B, blocks):
    """SBC_OP_CHAIN over RCU / CRP blocks; a final CRP block has signed weights, so its second pool sees negative planes."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    if W == 8 and B > 100:
        B = 37
    c = X.chain_case(Cc, H, W, B, blocks, device='cuda')
    ch, keep = _chain_record(torch, _lib, blocks, c.ws)
    dx = _dev(torch, c.x)
    out = _out(c.x.shape)
    _lib.range_flag()
    _launch(gpu, _lib.sbc_op(kind=P.CHAIN, flags=P.CONV_F16X2, B=B, H=H, W=W, cin=Cc, cout=Cc, ksize=3, dil=1, in_=_p(dx), out=_p(out),
                             ext=C.cast(C.pointer(ch), C.c_void_p)))
    assert _lib.range_flag() == 0
    _assert_exact(torch, out, c.expected, 'chain')


@pytest.mark.parametrize('B,H,W', [(3, 64, 16), (1, 256, 64), (5, 8, 8)])
def test_begin_conv_is_exact(gpu, B, H, W):
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    c = X.begin_case(B, H, W, device='cuda')
    dx, dw, db = _dev(torch, c.x), _dev(torch, c.w), _dev(torch, c.bias)
    out = _out((B, H, W, 32))
    _launch(gpu, _lib.sbc_op(kind=P.BEGIN_CONV, B=B, H=H, W=W, cin=2, cout=32, ksize=3, dil=1, in_=_p(dx), out=_p(out), weight=_p(dw), bias=_p(db)))
    _assert_exact(torch, out, c.expected, 'begin_conv')


@pytest.mark.parametrize('B,H,W', [(5, 64, 16), (1, 256, 64), (40, 8, 8)])
def test_end_conv_is_exact(gpu, B, H, W):
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    c = X.end_case(B, H, W, device='cuda')
    d = [_dev(torch, a) for a in (c.x, c.stats, c.w, c.bias, c.sigmas, c.labels)]
    out = _out((B, H, W, 2))
    ext = _lib.sbc_endconv(sigmas=_p(d[4]), labels=_p(d[5]))
    _launch(gpu, _lib.sbc_op(kind=P.END_CONV, B=B, H=H, W=W, cin=32, cout=2, ksize=3, dil=1, in_=_p(d[0]), out=_p(out), weight=_p(d[2]),
                             bias=_p(d[3]), stats=_p(d[1]), ext=C.cast(C.pointer(ext), C.c_void_p)))
    _assert_exact(torch, out, c.expected, 'end_conv')


# ============================================================================================ (b) element by element, identity filters
BANDS = list(X.ELU_BANDS)


def _elu64np(v):
    v = np.asarray(v, np.float64)
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))


def _hold(site, band, got, ref, bound):
    """|got - ref| <= bound element by element; records the worst ratio for the table of DESIGN.md 2.4."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(got).all(), site
    err = np.abs(got - ref)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    neg = ref < 0
    print('ELU-PROBE site=%s band=%s max_abs_err=%.3e max_rel_err_neg=%.3e worst_err_over_bound=%.3f'
          % (site, band, err.max(), (err[neg] / np.abs(ref[neg])).max() if neg.any() else 0.0, ratio.max()))
    if (err > bound).any():
        i = int(np.argmax(err - bound))
        raise AssertionError('%s, band %s: %d elements beyond the derived bound; worst: got %.9g, float64 %.9g, error %.3e, bound %.3e'
                             % (site, band, int((err > bound).sum()), got.flat[i], ref.flat[i], err.flat[i], bound.flat[i]))


def _calibrate(gpu, ops):
    torch, _lib = gpu
    _lib.calibrate_f16x2(ops, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _G.check(written=False)
    assert _lib.range_flag() == 0


def _trailer(t):
    return t[-4:].cpu().numpy()


def _expect_trailer(tr, amax0):
    """act_scale = 2^(9 - exponent of the first sample's staged maximum); the fourth word asks for the accurate ELU exactly below 2^-4"""
    assert tr[0] == 2.0 ** (9 - int(np.frexp(np.float32(amax0))[1])) and tr[1] == tr[2] / tr[0], (tr, amax0)
    assert tr[3] == (1.0 if 0 < amax0 < 2.0 ** -4 else 0.0), (tr, amax0)
    return float(tr[0]), bool(tr[3])


CONV_PROBE_SITES = [
    # algo, ELU_ACC in flags, cin = cout, H, W, label of the staging implementation
    ('direct', False, 32, 64, 16, 'conv_mfma'), ('direct', True, 32, 64, 16, 'conv_mfma'),
    ('bf16x3', False, 32, 64, 16, 'conv_x3 / tile.h'), ('bf16x3', True, 32, 64, 16, 'conv_x3 / tile.h'),
    ('f16x2', False, 32, 64, 16, 'conv_x3 / tile.h'), ('f16x2', False, 64, 8, 2, 'conv_dp 8x2'), ('f16x2', False, 64, 16, 4, 'conv_dp 16x4'),
    ('f16x2', False, 64, 32, 8, 'direct form of a Winograd-eligible shape'),
]


@pytest.mark.parametrize('band', BANDS, ids=str)
@pytest.mark.parametrize('algo,acc,Cc,H,W,label', CONV_PROBE_SITES)
def test_conv_prologue_elu_element_by_element(gpu, algo, acc, Cc, H, W, label, band):
    """SBC_OP_CONV with SBC_PRO_ELU and the identity filter: out = ELU(x) element by element, in the fast and the accurate form; the
    f16x2 records go through the library's calibration, which must ask for the accurate form exactly when the layer is small."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    f16x2 = algo == 'f16x2'
    x = X.elu_probe_values((2, H, W, Cc), band, limit=16.0 * 2.0 ** band[1] if f16x2 else None)
    ref = _elu64np(x)
    dx = _dev(torch, x)
    out = _out(x.shape)
    flags = P.PRO_ELU | (0x20000 if acc else 0)                       # SBC_PRO_ELU_ACC (include/sbc_hip.h)
    op = _lib.sbc_op(kind=P.CONV, flags=flags, B=2, H=H, W=W, cin=Cc, cout=Cc, ksize=3, dil=1, in_=_p(dx), out=_p(out))
    keep = _bind_conv_weight(torch, P, op, algo, X.identity_filter(Cc), flags, calibrated=True)
    s = None
    if f16x2:
        _calibrate(gpu, [op])
        s, acc = _expect_trailer(_trailer(keep[-1]), np.abs(ref[0]).max())
    _lib.range_flag()
    _launch(gpu, op)
    assert _lib.range_flag() == 0                                      # a CONV record has the accurate form: it never needs SBC_RANGE_ELU
    _hold('CONV %s%s (%s)' % (algo, ' acc' if acc else '', label), band, out.cpu().numpy(), ref, X.elu_bound(x, 'acc' if acc else 'fast', s))


@pytest.mark.parametrize('band', BANDS, ids=str)
@pytest.mark.parametrize('algo,Cc,H,W', [('direct', 32, 64, 16), ('f16x2', 32, 64, 16), ('f16x2', 64, 8, 2), ('winograd_f16x2', 32, 64, 16)])
def test_epilogue_res1_elu_element_by_element(gpu, algo, Cc, H, W, band):
    """SBC_EPI_RES1_ELU with zero weights: out = res2 + ELU(res1) with res2 = 0 -- the epilogue's ELU is the accurate form everywhere."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    r = X.elu_probe_values((2, H, W, Cc), band)
    x = np.ones(r.shape, F32)
    d = [_dev(torch, a) for a in (x, r, np.zeros(r.shape, F32))]
    out = _out(r.shape)
    op = _lib.sbc_op(kind=P.CONV, flags=P.EPI_RES1_ELU, B=2, H=H, W=W, cin=Cc, cout=Cc, ksize=3, dil=1, in_=_p(d[0]), out=_p(out), res1=_p(d[1]), res2=_p(d[2]))
    keep = _bind_conv_weight(torch, P, op, algo, np.zeros((Cc, Cc, 3, 3), F32), P.EPI_RES1_ELU)
    _lib.range_flag()
    _launch(gpu, op)
    assert _lib.range_flag() == 0
    _hold('EPI_RES1_ELU %s %dx%d' % (algo, H, W), band, out.cpu().numpy(), _elu64np(r), X.elu_bound(r, 'acc'))
    del keep


@pytest.mark.parametrize('band', BANDS, ids=str)
@pytest.mark.parametrize('C_,H,W', [(32, 64, 16), (128, 8, 2)])
def test_maxpool5_elu_element_by_element(gpu, C_, H, W, band):
    """SBC_OP_MAXPOOL5 with SBC_PRO_ELU (both kernels): out = ELU(max of the window), the accurate form."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    x = _negate_some(X.elu_probe_values((2, H, W, C_), band), 10)
    p = X.maxpool64(torch.from_numpy(x).double()).numpy()
    dx = _dev(torch, x)
    out = _out(x.shape)
    _launch(gpu, _lib.sbc_op(kind=P.MAXPOOL5, flags=P.PRO_ELU, B=2, H=H, W=W, cin=C_, cout=C_, in_=_p(dx), out=_p(out)))
    _hold('MAXPOOL5 %dx%d' % (H, W), band, out.cpu().numpy(), _elu64np(p), X.elu_bound(p, 'acc'))


def _negate_some(x, key):
    """(pooled probes: make most windows negative, or the maximum hides every negative value)"""
    rng = np.random.default_rng(key)
    planes = rng.random((x.shape[0], 1, 1, x.shape[3])) < 0.7
    return np.where(planes, -np.abs(x), x).astype(F32)


@pytest.mark.parametrize('band', BANDS, ids=str)
def test_conv_pool_elu_element_by_element(gpu, band):
    """SBC_OP_CONV_POOL, stage pool_elu, identity filter: out = ELU(max of the window) through the two-term staging.  The kernel has
    the fast form only: where the calibration asks for the accurate one it must leave SBC_RANGE_ELU (and still meet the fast bound)."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.weights import pack_conv_weight_f16x2
    x = _negate_some(X.elu_probe_values((2, 64, 16, 32), band, limit=16.0 * 2.0 ** band[1]), 11)
    p = X.maxpool64(torch.from_numpy(x).double()).numpy()
    ref = _elu64np(p)
    dx, dw = _dev(torch, x), _dev(torch, pack_conv_weight_f16x2(X.identity_filter(32)).view(np.float32), 'w', True)
    out = _out(x.shape)
    op = _lib.sbc_op(kind=P.CONV_POOL, flags=P.PRO_ELU | P.CONV_F16X2, B=2, H=64, W=16, cin=32, cout=32, ksize=3, dil=1, in_=_p(dx), out=_p(out), weight_split=_p(dw))
    _calibrate(gpu, [op])
    s, small = _expect_trailer(_trailer(dw), np.abs(ref[0]).max())
    _launch(gpu, op)
    assert _lib.range_flag() == (_lib.RANGE_ELU if small else 0)
    _hold('CONV_POOL pool_elu', band, out.cpu().numpy(), ref, X.elu_bound(p, 'fast', s))


def _pair_like_bound(x, form1, s1, form2, s2):
    """out = x + ELU(t), t = ELU(x), both activations staged through the two-term split: ELU is 1-Lipschitz, so the first stage's error
    passes through the second at most unchanged; the final sum rounds once (twice if the convolution is descaled first)."""
    y1 = _elu64np(x)
    y2 = _elu64np(y1)
    ref = x.astype(np.float64) + y2
    return ref, X.elu_bound(x, form1, s1) + X.elu_bound(y1, form2, s2) + 2.0 ** -23 * np.abs(ref) + 2.0 ** -24 * np.abs(y2)


@pytest.mark.parametrize('band', BANDS, ids=str)
def test_conv_pair_elu_element_by_element(gpu, band):
    """SBC_OP_CONV_PAIR with two identity filters: out = x + ELU(ELU(x)); the fast form only, SBC_RANGE_ELU where either layer is small."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.weights import pack_conv_weight_f16x2
    x = X.elu_probe_values((2, 64, 16, 32), band, limit=16.0 * 2.0 ** band[1])
    dx = _dev(torch, x)
    d1, d2 = (_dev(torch, pack_conv_weight_f16x2(X.identity_filter(32)).view(np.float32), 'w%d' % i, True) for i in (1, 2))
    out = _out(x.shape)
    op = _lib.sbc_op(kind=P.CONV_PAIR, flags=P.CONV_F16X2, B=2, H=64, W=16, cin=32, cout=32, ksize=3, dil=1, in_=_p(dx), out=_p(out), weight_split=_p(d1), weight2_split=_p(d2))
    _calibrate(gpu, [op])
    y1 = _elu64np(x)
    s1, small1 = _expect_trailer(_trailer(d1), np.abs(y1[0]).max())
    s2, small2 = _expect_trailer(_trailer(d2), np.abs(_elu64np(y1)[0]).max())
    _launch(gpu, op)
    assert _lib.range_flag() == (_lib.RANGE_ELU if (small1 or small2) else 0)
    ref, bound = _pair_like_bound(x, 'fast', s1, 'fast', s2)
    _hold('CONV_PAIR', band, out.cpu().numpy(), ref, bound)


@pytest.mark.parametrize('band', BANDS, ids=str)
@pytest.mark.parametrize('Cc,H,W', [(64, 8, 2), (32, 32, 8)])
def test_chain_rcu_elu_element_by_element(gpu, Cc, H, W, band):
    """SBC_OP_CHAIN ('R',) with identity filters: out = x + ELU(ELU(x)); the chain kernel honours the calibration's request for the
    accurate form per convolution, so it meets the accurate bound with a clear range word."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    x = X.elu_probe_values((2, H, W, Cc), band, limit=16.0 * 2.0 ** band[1])
    ident = X.identity_filter(Cc)
    ch, keep = _chain_record(torch, _lib, ('R',), [(ident, ident)], inout=True)
    dx = _dev(torch, x)
    out = _out(x.shape)
    op = _lib.sbc_op(kind=P.CHAIN, flags=P.CONV_F16X2, B=2, H=H, W=W, cin=Cc, cout=Cc, ksize=3, dil=1, in_=_p(dx), out=_p(out), ext=C.cast(C.pointer(ch), C.c_void_p))
    _calibrate(gpu, [op])
    y1 = _elu64np(x)
    s1, a1 = _expect_trailer(_trailer(keep[0]), np.abs(y1[0]).max())
    s2, a2 = _expect_trailer(_trailer(keep[1]), np.abs(_elu64np(y1)[0]).max())
    _launch(gpu, op)
    assert _lib.range_flag() == 0
    ref, bound = _pair_like_bound(x, 'acc' if a1 else 'fast', s1, 'acc' if a2 else 'fast', s2)
    _hold('CHAIN R %dx%d' % (H, W), band, out.cpu().numpy(), ref, bound)


@pytest.mark.parametrize('band', BANDS, ids=str)
@pytest.mark.parametrize('Cc,H,W', [(64, 8, 2), (32, 32, 8)])
def test_chain_crp_elu_element_by_element(gpu, Cc, H, W, band):
    """SBC_OP_CHAIN ('C',) with identity filters: e = ELU(x) (always the accurate form), p1 = maxpool(e), p2 = maxpool(p1), both staged
    through the two-term split, out = (p1 + e) + p2.  A maximum passes an error on at most unchanged: the error of a pooled value is
    bounded by the largest bound in its window."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    x = _negate_some(X.elu_probe_values((2, H, W, Cc), band, limit=16.0 * 2.0 ** band[1]), 12)
    ident = X.identity_filter(Cc)
    ch, keep = _chain_record(torch, _lib, ('C',), [(ident, ident)], inout=True)
    dx = _dev(torch, x)
    out = _out(x.shape)
    op = _lib.sbc_op(kind=P.CHAIN, flags=P.CONV_F16X2, B=2, H=H, W=W, cin=Cc, cout=Cc, ksize=3, dil=1, in_=_p(dx), out=_p(out), ext=C.cast(C.pointer(ch), C.c_void_p))
    _calibrate(gpu, [op])
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))        # noqa: E731
    e = _elu64np(x)
    p1 = X.maxpool64(t64(e)).numpy()
    p2 = X.maxpool64(t64(p1)).numpy()
    s1, _ = _expect_trailer(_trailer(keep[0]), np.abs(p1[0]).max())
    s2, _ = _expect_trailer(_trailer(keep[1]), np.abs(p2[0]).max())
    _launch(gpu, op)
    assert _lib.range_flag() == 0
    be = X.elu_bound(x, 'acc')
    rep = lambda y, s: np.maximum(2.0 ** -22 * np.abs(y), 2.0 ** -25 / s)   # noqa: E731
    b1 = X.maxpool64(t64(be), pad=0.0).numpy() + rep(p1, s1)
    b2 = X.maxpool64(t64(b1), pad=0.0).numpy() + rep(p2, s2)
    ref = (p1 + e) + p2
    # (two sums; the high and the low product of a staged value may enter the accumulator separately: two roundings per sum)
    bound = be + b1 + b2 + 2.0 ** -23 * (np.abs(p1 + e) + np.abs(ref)) * 1.0000001
    _hold('CHAIN C %dx%d' % (H, W), band, out.cpu().numpy(), ref, bound)


@pytest.mark.parametrize('band', BANDS, ids=str)
@pytest.mark.parametrize('cin,cout,H,W', [(32, 64, 64, 16), (64, 64, 32, 8)])
def test_conv_down_elu_element_by_element(gpu, cin, cout, H, W, band):
    """SBC_OP_CONV_DOWN with the identity 3x3 filter (its pooled form is 1/4 at four taps), a zero shortcut and the identity norm:
    out = the mean of four staged activations.  Eight nonzero products (high and low term of four values) enter the accumulator:
    at most eight roundings of at most 2^-24 of the sum of magnitudes."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.weights import pack_conv_weight_pooled_f16x2
    a = X.elu_probe_values((2, H, W, cin), band, limit=16.0 * 2.0 ** band[1])
    w3 = np.zeros((cout, cin, 3, 3), F32)
    w3[np.arange(cin), np.arange(cin), 1, 1] = 1.0
    st = np.stack([np.zeros((2, cin), F32), np.ones((2, cin), F32), np.zeros((2, cin), F32)], 1)
    d = [_dev(torch, t) for t in (a, np.zeros(a.shape, F32), st, np.zeros(cout, F32), np.zeros(cout, F32))]
    d3 = _dev(torch, pack_conv_weight_pooled_f16x2(w3).view(np.float32), 'w3', True)
    d1 = _dev(torch, pack_conv_weight_pooled_f16x2(np.zeros((cout, cin, 1, 1), F32)).view(np.float32), 'w1', True)
    out = _out((2, H // 2, W // 2, cout))
    op = _lib.sbc_op(kind=P.CONV_DOWN, flags=P.CONV_F16X2, B=2, H=H, W=W, cin=cin, cout=cout, ksize=3, dil=1, in_=_p(d[0]), out=_p(out), res1=_p(d[1]),
                     stats=_p(d[2]), weight_split=_p(d3), weight2_split=_p(d1), bias=_p(d[3]), bias2=_p(d[4]))
    _calibrate(gpu, [op])
    y = _elu64np(a)
    s, acc = _expect_trailer(_trailer(d3), np.abs(y[0]).max())
    _launch(gpu, op)
    assert _lib.range_flag() == 0
    quad = lambda t: t[:, ::2, ::2] + t[:, 1::2, ::2] + t[:, ::2, 1::2] + t[:, 1::2, 1::2]   # noqa: E731
    ref = np.zeros((2, H // 2, W // 2, cout))
    bound = np.zeros_like(ref)
    ref[..., :cin] = 0.25 * quad(y)
    bound[..., :cin] = 0.25 * quad(X.elu_bound(a, 'acc' if acc else 'fast', s)) + 8 * 2.0 ** -24 * 0.25 * quad(np.abs(y)) * 1.0000001
    _hold('CONV_DOWN %d->%d' % (cin, cout), band, out.cpu().numpy(), ref, bound)


@pytest.mark.parametrize('band', BANDS, ids=str)
def test_end_conv_elu_element_by_element(gpu, band):
    """SBC_OP_END_CONV with filters that pick one channel each, the identity norm and sigma = 1: out = ELU(x[..., c]) in fp32, the
    fast form."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    B, H, W = 2, 64, 16
    x = X.elu_probe_values((B, H, W, 32), band)
    w = np.zeros((2, 32, 3, 3), F32)
    w[0, 5, 1, 1] = w[1, 20, 1, 1] = 1.0
    st = np.stack([np.zeros((B, 32), F32), np.ones((B, 32), F32), np.zeros((B, 32), F32)], 1)
    d = [_dev(torch, a) for a in (x, st, w, np.zeros(2, F32), np.array([1.0, 2.0], F32), np.zeros(B, np.int64))]
    out = _out((B, H, W, 2))
    ext = _lib.sbc_endconv(sigmas=_p(d[4]), labels=_p(d[5]))
    _launch(gpu, _lib.sbc_op(kind=P.END_CONV, B=B, H=H, W=W, cin=32, cout=2, ksize=3, dil=1, in_=_p(d[0]), out=_p(out), weight=_p(d[2]), bias=_p(d[3]),
                             stats=_p(d[1]), ext=C.cast(C.pointer(ext), C.c_void_p)))
    v = x[..., [5, 20]]
    _hold('END_CONV', band, out.cpu().numpy(), _elu64np(v), X.elu_bound(v, 'fast'))
