"""The exact-answer cases of tests/exact_cases.py, checked without a GPU: the fp32 oracle reproduces every float64 ``expected`` bit
for bit (the second witness), every operand survives the weight forms unchanged, every span is below 2^22 (asserted by the
builders), and mutated references -- the defects the data is meant to see -- differ from ``expected``."""
import numpy as np
import pytest

import exact_cases as X
from oracle import ncsnv2_oracle as O
from test_gpu_ops import CONV_PARAMS, PAIR_CASES

F32 = np.float32


def _nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def _small(B, H, W):
    return min(B, 1 if H * W >= 4096 else 2)


def _conv_keys():
    seen, keys = set(), []
    for cin, cout, k, dil, B, H, W, mode, algo in CONV_PARAMS:
        if 'selfnorm' in mode or mode == 'up_2x' or (algo.startswith('winograd') and (k != 3 or dil != 1)):
            continue
        wino = algo.startswith('winograd')
        for fam in X.FAMILIES if (algo in X.LO_ALGOS) else ('int',):
            key = (cin, cout, k, dil, _small(B, H, W), H, W, mode.replace('_top', ''), fam, wino)
            if key not in seen:
                seen.add(key)
                keys.append(key)
    return keys


CONV_KEYS = _conv_keys()


def _same(got, expected):
    e = expected.cpu().numpy() if hasattr(expected, 'cpu') else expected
    return np.array_equal(np.asarray(got).astype(np.float64), e)


def _oracle_conv(c):
    """The record with the fp32 oracle's primitives, as tests/test_gpu_ops.py composes them."""
    v = c.x
    if c.stats is not None:
        v = (v - c.stats[:, None, None, 0]) * c.stats[:, None, None, 1] + c.stats[:, None, None, 2]
    if 'elu' in c.mode:
        v = O.elu(v)
    y = O.conv2d(_nchw(v), c.w, c.bias, c.dil)
    if 'pool' in c.mode:
        y = O.mean_pool2(y)
    y = _nhwc(y)
    if c.res1 is not None:
        r = O.elu(c.res1) if c.mode == 'crp2' else c.res1
        if c.res2 is not None:
            r = c.res2 + r
        y = y + r
    if c.up is not None:
        y = y + _nhwc(O.bilinear_align_corners(_nchw(c.up), c.x.shape[1:3]))
    return y


@pytest.mark.parametrize('key', CONV_KEYS, ids=lambda k: '-'.join(map(str, k)))
def test_conv_cases_are_exact_under_the_oracle_and_the_weight_forms(key):
    from score_based_channels_amd.weights import f16x2_shift, split_bf16x3, split_f16x2
    *shape, mode, fam, wino = key
    c = X.conv_case(*shape, mode, fam, wino=wino)
    assert c.span < X.SPAN_LIMIT
    y = _oracle_conv(c)
    assert y.dtype == F32 and _same(y, c.expected)
    # operands and weight forms: nothing is rounded away
    forms = [c.w] + ([X.wino_u(c.w).astype(F32)] if wino else [])
    if wino:
        u = X.wino_u(c.w)
        assert np.array_equal(u * 4, np.round(u * 4)) and np.array_equal(u.astype(np.float16).astype(np.float64), u)   # quarter-integers, fp16-exact
    for f in forms:
        s = f16x2_shift(f)
        h, l = split_f16x2(np.ldexp(f, s).astype(F32))
        assert np.array_equal(h.astype(np.float64) + l.astype(np.float64), np.ldexp(f.astype(np.float64), s))
        assert np.array_equal(sum(t.astype(np.float64) for t in split_bf16x3(f)), f.astype(np.float64))
    v = c.x.astype(np.float64)
    if c.stats is not None:
        v = X.norm64(v, c.stats.astype(np.float64))
    h, l = split_f16x2(v.astype(F32))
    assert np.array_equal(h.astype(np.float64) + l.astype(np.float64), v)
    if fam == 'int':
        assert np.array_equal(v.astype(np.float16).astype(np.float64), v) and np.array_equal(c.w.astype(np.float16), c.w)   # the f16w forms
    if fam == 'lo-x':
        assert (l != 0).mean() > 0.1                                     # the activation split's low term is populated ...
        assert (split_bf16x3(v.astype(F32))[1] != 0).mean() > 0.1
    if fam == 'lo-w':
        assert X.low_term_fraction(c.w, f16x2_shift(c.w)) * c.w.size / max(1, (c.w != 0).sum()) > 0.3   # ... or the weight's, among its taps
        assert (split_bf16x3(c.w)[1] != 0).sum() > 0.3 * (c.w != 0).sum()


@pytest.mark.parametrize('case', sorted({(_small(c[0], c[1], c[2]),) + tuple(c[1:]) for c in PAIR_CASES}), ids=str)
def test_pair_cases_are_exact_under_the_oracle(case):
    B, H, W = case[:3]
    c = X.pair_case(B, H, W, case[3] if len(case) > 3 else 32)
    t = O.conv2d(_nchw(O.elu(c.x)), c.w1, None, 1)
    y = c.x + _nhwc(O.conv2d(O.elu(t), c.w2, None, 1))
    assert _same(y, c.expected)
    assert np.array_equal(t.astype(np.float16).astype(F32), t) and t.min() >= 0 and t.max() <= 2048   # the f16w mode stages it exactly


@pytest.mark.parametrize('stage', ['pool_elu', 'pool_crp2'])
@pytest.mark.parametrize('H', [64, 8, 16, 24])
def test_conv_pool_cases_are_exact_and_see_a_zero_padded_pool(H, stage):
    c = X.conv_pool_case(2, H, stage)
    v = _nhwc(O.max_pool5(_nchw(c.x)))
    if stage == 'pool_elu':
        v = O.elu(v)
    y = _nhwc(O.conv2d(_nchw(v), c.w, None, 1))
    if c.res1 is not None:
        y = y + (c.res2 + O.elu(c.res1))
    assert _same(y, c.expected)
    if stage == 'pool_crp2':
        assert not _same(y, X.conv_pool_case(2, H, stage, mutate='pad0').expected)


@pytest.mark.parametrize('C_,B,H,W', [(32, 2, 64, 16), (128, 2, 8, 2), (64, 2, 16, 4), (32, 1, 48, 24), (32, 2, 2, 2), (32, 3, 8, 2)])
def test_maxpool_cases_are_exact_and_see_a_zero_padded_pool(C_, B, H, W):
    import torch
    c = X.maxpool_case(C_, B, H, W, False)
    y = _nhwc(O.max_pool5(_nchw(c.x)))
    assert _same(y, c.expected)
    assert not _same(y, X.maxpool64(torch.from_numpy(c.x).double(), pad=0.0))
    # the spike planes put a maximum at each of the 25 window offsets
    plain = X.maxpool_case(C_, B, H, W, False, specials=False)
    if H >= 5 and W >= 5:
        where = set()
        xs = plain.x
        b, hh, ww, cc = np.nonzero(xs == 7.0)
        for bi, h, w, ci in zip(b, hh, ww, cc):
            if (bi * 3 + ci) % 4 == 1:
                for dh in range(-2, 3):
                    for dw in range(-2, 3):
                        if 0 <= h + dh < H and 0 <= w + dw < W:
                            where.add((dh, dw))
        assert len(where) == 25
    ce = X.maxpool_case(C_, B, H, W, True)
    assert _same(O.elu(_nhwc(O.max_pool5(_nchw(ce.x)))), ce.expected)


@pytest.mark.parametrize('cin,cout,H,W', [(32, 64, 64, 16), (32, 64, 16, 16), (64, 64, 32, 8), (64, 64, 16, 8)])
def test_conv_down_cases_are_exact_under_the_oracle(cin, cout, H, W):
    from score_based_channels_amd.weights import f16x2_shift, pooled_filter, split_f16x2
    c = X.conv_down_case(cin, cout, H, W, 2)
    v = O.elu((c.a - c.stats[:, None, None, 0]) * c.stats[:, None, None, 1] + c.stats[:, None, None, 2])
    y = _nhwc(O.mean_pool2(O.conv2d(_nchw(v), c.w3, c.b3, 1)) + O.mean_pool2(O.conv2d(_nchw(c.x), c.w1, c.b1, 1)))
    assert _same(y, c.expected)
    for w in (c.w3, c.w1):
        pf = pooled_filter(w)
        k = w.shape[2]
        ref = np.zeros(w.shape[:2] + (k + 1, k + 1))
        for a in range(2):
            for b in range(2):
                ref[:, :, a:a + k, b:b + k] += w
        assert np.array_equal(pf.astype(np.float64) * 4, ref)            # quarter-integers, exactly the mean of the four shifts
        s = f16x2_shift(pf)
        h, l = split_f16x2(np.ldexp(pf, s).astype(F32))
        assert np.array_equal(h.astype(np.float64) + l.astype(np.float64), np.ldexp(pf.astype(np.float64), s))


def _oracle_chain(x, blocks, ws):
    out = x
    for tok, (w1, w2) in zip(blocks, ws):
        if tok == 'R':
            t = O.conv2d(_nchw(O.elu(out)), w1, None, 1)
            out = out + _nhwc(O.conv2d(O.elu(t), w2, None, 1))
        else:
            out = O.elu(out)
            path = O.conv2d(O.max_pool5(_nchw(out)), w1, None, 1)
            out = _nhwc(path) + out
            path = O.conv2d(O.max_pool5(path), w2, None, 1)
            out = _nhwc(path) + out
    return out


@pytest.mark.parametrize('blocks', X.CHAIN_BLOCKS, ids=['-'.join(b) for b in X.CHAIN_BLOCKS])
@pytest.mark.parametrize('Cc,H,W', [(64, 8, 2), (128, 8, 2), (64, 16, 4), (32, 32, 8), (64, 32, 8)])
def test_chain_cases_are_exact_under_the_oracle(Cc, H, W, blocks):
    c = X.chain_case(Cc, H, W, 3, blocks)
    assert _same(_oracle_chain(c.x, blocks, c.ws), c.expected)
    if blocks == ('C',):
        assert not _same(c.expected.numpy(), X.chain_case(Cc, H, W, 3, blocks, mutate='pad0').expected)


@pytest.mark.parametrize('B,H,W', [(2, 64, 16), (1, 256, 64), (2, 8, 8)])
def test_begin_and_end_cases_are_exact_under_the_oracle(B, H, W):
    c = X.begin_case(B, H, W)
    assert _same(_nhwc(O.conv2d(_nchw(F32(2) * c.x - F32(1)), c.w, c.bias)), c.expected)
    e = X.end_case(B, H, W)
    v = O.elu((e.x - e.stats[:, None, None, 0]) * e.stats[:, None, None, 1] + e.stats[:, None, None, 2])
    y = _nhwc(O.conv2d(_nchw(v), e.w, e.bias)) / e.sigmas[e.labels][:, None, None, None]
    assert y.dtype == F32 and _same(y, e.expected)


# ---- the data can see the defects it is meant for ------------------------------------------------------------------------------------
MUTATIONS = [('drop_tap', 'int', 'norm_elu_res'), ('transpose_tap', 'int', 'norm_elu_res'), ('drop_hi_lo', 'lo-w', 'norm_elu_res'),
             ('drop_lo_hi', 'lo-x', 'norm_elu_res'), ('res_before_elu', 'int', 'crp2'), ('norm_on_padding', 'int', 'norm_elu_res')]


@pytest.mark.parametrize('mutation,family,mode', MUTATIONS)
def test_a_mutated_reference_differs(mutation, family, mode):
    """Every (shape, flag set) of the family that carries the mutated feature notices it -- not merely one."""
    keys = [k for k in CONV_KEYS if k[8] == family and k[7] == mode and k[2] == 3 and not k[9]]
    assert keys
    seen = 0
    for key in keys[:6]:
        *shape, mode_, fam, wino = key
        good = X.conv_case(*shape, mode_, fam)
        bad = X.conv_case(*shape, mode_, fam, mutate=mutation)
        seen += not _same(bad.expected.numpy(), good.expected)
    assert seen == len(keys[:6]), (mutation, seen)


def test_elu_probe_values_and_bounds():
    """The identity-filter probes: every band holds the planted values, and the derived bounds have the stated sizes."""
    for band in X.ELU_BANDS:
        v = X.elu_probe_values((2, 64, 16, 32), band)
        for p in X.ELU_PLANTED:
            assert (v[1:].view(np.uint32) == np.float32(p).view(np.uint32)).sum() >= 3  # (bitwise: -0 is not +0 here)
        body = np.abs(v[0])                                                              # the first sample: the band alone
        assert body.min() >= 2.0 ** band[0] * (1 - 1e-6) and body.max() <= 2.0 ** band[1] * (1 + 1e-6) and (v[0] < 0).mean() > 0.4
        small = X.elu_probe_values((2, 64, 16, 32), band, limit=16.0 * 2.0 ** band[1])
        assert np.abs(np.where(small > 0, small, np.expm1(np.minimum(small.astype(np.float64), 0)))).max() <= 16.0 * 2.0 ** band[1]
    v = np.array([1.0, 0.0, -0.5, -0.01, -1e-4], np.float64)
    assert np.array_equal(X.elu_bound(v, 'fast'), [0, 0, 2.0 ** -23, 2.0 ** -23, 2.0 ** -23])
    acc = X.elu_bound(v, 'acc')
    assert acc[2] == 2.0 ** -23 and abs(acc[3] - 2.0 ** -22 * abs(np.expm1(-0.01))) < 1e-20 and acc[4] < 3e-11
    assert X.elu_bound(np.array([1.0]), 'fast', s=256.0)[0] == 2.0 ** -22
    w = X.identity_filter(32)
    assert w.sum() == 32 and np.array_equal(w[:, :, 1, 1], np.eye(32, dtype=F32))
