"""The regimes of the Learned D-AMP tests off the fixture (tests/test_gpu_ldamp.py on the GPU, tests/test_ldamp_cpu.py for their
admissibility without one) -- test infrastructure; nothing of the library's kernels is involved.

The geometry is fixed (64 x 16), so what varies is what a trained checkpoint and a caller bring: the scale of the convolution weights
(InstanceNorm removes it, up to IN_EPS), the scale and offset of the denoiser's input (``norm`` removes them), the scale of the
measurements (the floor of ``eps = max(1e-3 max|r|, 1e-5)``), the SNR, the net's position in the weight block and the batch size.
All weights are ``ldamp.seeded_state_dict`` and then transformed.

The rule (FACTOR = 4): error(x, float64) <= 4 e_ref.  For these cases e_ref is the LARGER of two float32
evaluations of the oracle in different valid summation orders, the native one and the flipped twin of tests/ldamp_oracle.py; a
scalar log gets one fp32 rounding of the logged value itself, 2^-23 |ref|, on top.
"""
import collections

import numpy as np
import torch

import ldamp_oracle as O

F32, F64 = torch.float32, torch.float64
FACTOR = 4.0
ULP = 2.0 ** -23
IN_EPS = 1e-5
EPS_FLOOR = 1e-5
SEED_WEIGHTS = 7
UNROLLS = 3

# the 17 normed layers in forward order (the 1 x 1 output convolution is not followed by a norm: it keeps its scale)
NORMED = ['down_sample_layers.0.layers.0', 'down_sample_layers.0.layers.4', 'down_sample_layers.1.layers.0', 'down_sample_layers.1.layers.4',
          'down_sample_layers.2.layers.0', 'down_sample_layers.2.layers.4', 'conv.layers.0', 'conv.layers.4',
          'up_transpose_conv.0.layers.0', 'up_conv.0.layers.0', 'up_conv.0.layers.4', 'up_transpose_conv.1.layers.0', 'up_conv.1.layers.0',
          'up_conv.1.layers.4', 'up_transpose_conv.2.layers.0', 'up_conv.2.0.layers.0', 'up_conv.2.0.layers.4']
WEIGHT_REGIMES = {
    'plain': None,
    'w_2m10': lambda i: 2.0 ** -10,                               # conv output variance ~ 2^-20 << IN_EPS: eps dominates every norm
    'w_2p8': lambda i: 2.0 ** 8,
    'w_alt': lambda i: 2.0 ** -6 if i % 2 == 0 else 2.0 ** 6,     # from layer to layer
}


def transform_weights(sd, regime):
    """every convolution / transposed-convolution weight in front of a norm times the regime's power of two, in every net"""
    f = WEIGHT_REGIMES[regime]
    if f is None:
        return sd
    out = dict(sd)
    for name in sd:
        for i, key in enumerate(NORMED):
            if name.endswith('.unet.' + key + '.weight'):
                out[name] = (sd[name] * np.float32(f(i))).astype(np.float32)
    return out


_SD = {}


def weights(regime='plain', max_unrolls=10):
    """(state dict, its flipped twin), shared"""
    key = (regime, max_unrolls)
    if key not in _SD:
        from score_based_channels_amd import ldamp
        sd = transform_weights(ldamp.seeded_state_dict(SEED_WEIGHTS, max_unrolls), regime)
        _SD[key] = (sd, O.flip_state_dict(sd))
    return _SD[key]


# ---- 1. one evaluation, layer by layer ------------------------------------------------------------------------------------------------
LayerCase = collections.namedtuple('LayerCase', 'name weights input net B')
LAYER_CASES = [
    LayerCase('w_2m10', 'w_2m10', 'plain', 0, 4),
    LayerCase('w_2p8', 'w_2p8', 'plain', 0, 4),
    LayerCase('w_alt', 'w_alt', 'plain', 0, 4),
    LayerCase('in_2m20', 'plain', 'in_2m20', 0, 4),
    LayerCase('in_2p12', 'plain', 'in_2p12', 0, 4),
    LayerCase('in_offset', 'plain', 'in_offset', 0, 4),           # mean >> std in both planes
    LayerCase('net4', 'plain', 'plain', 4, 4),                    # the offset into the weight block
    LayerCase('net9', 'plain', 'plain', 9, 4),
    LayerCase('b1', 'plain', 'plain', 0, 1),
    LayerCase('b5', 'plain', 'plain', 0, 5),
]
INPUT_REGIMES = {'plain': lambda r: r, 'in_2m20': lambda r: r * 2.0 ** -20, 'in_2p12': lambda r: r * 2.0 ** 12,
                 'in_offset': lambda r: r + 30 * (1 + 0.5j)}


def layer_input(case):
    """complex64 [B, 64, 16]: the fixture's denoiser input (more samples: the same, rolled and rescaled), through the input regime"""
    r = O.golden_unet()['r']
    more = [np.roll(r[i % len(r)], (3 + i, 1 + i), (0, 1)) * (1.5 + i) for i in range(max(0, case.B - len(r)))]
    r = np.concatenate([r] + [m[None] for m in more])[:case.B]
    return np.ascontiguousarray(INPUT_REGIMES[case.input](r).astype(np.complex64))


def planes_of(c):
    return np.ascontiguousarray(np.stack((c.real, c.imag), axis=1))


CHAIN = [('d0a', 'x', 'down_sample_layers.0.layers.0.weight'), ('d0', 'd0a', 'down_sample_layers.0.layers.4.weight'),
         ('d1a', 'p0', 'down_sample_layers.1.layers.0.weight'), ('d1', 'd1a', 'down_sample_layers.1.layers.4.weight'),
         ('d2a', 'p1', 'down_sample_layers.2.layers.0.weight'), ('d2', 'd2a', 'down_sample_layers.2.layers.4.weight'),
         ('ba', 'p2', 'conv.layers.0.weight'), ('bb', 'ba', 'conv.layers.4.weight'),
         ('u0', 'u0a', 'up_conv.0.layers.4.weight'), ('u1', 'u1a', 'up_conv.1.layers.4.weight'), ('u2', 'u2a', 'up_conv.2.0.layers.4.weight')]
POOLED = [('p0', 'd0a', 'down_sample_layers.0.layers.4.weight'), ('p1', 'd1a', 'down_sample_layers.1.layers.4.weight'),
          ('p2', 'd2a', 'down_sample_layers.2.layers.4.weight')]
TCONV = [('t0', 'bb', 'up_transpose_conv.0.layers.0.weight'), ('t1', 'u0', 'up_transpose_conv.1.layers.0.weight'),
         ('t2', 'u1', 'up_transpose_conv.2.layers.0.weight')]
TWO_SOURCE = [('u0a', 't0', 'd2', 'up_conv.0.layers.0.weight'), ('u1a', 't1', 'd1', 'up_conv.1.layers.0.weight'),
              ('u2a', 't2', 'd0', 'up_conv.2.0.layers.0.weight')]


def layer_refs(sd, net, st, planes):
    """Every launch of one evaluation on its own: the stage's INPUT as ``st`` holds it (name -> array; the kernel's workspace on the GPU, a
    float32 oracle's stages without one) goes through the oracle's layer in float64, in float32 and in float32 through the flipped
    twin.  -> [(what, name of the output stage, ref64, ref32, ref32 flipped)]; the output of the 1 x 1 + unnorm + residual is 'out'."""
    W = lambda k, dt: torch.from_numpy(sd['update_nets.%d.unet.%s' % (net, k)]).to(dt)        # noqa: E731
    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)                         # noqa: E731
    ident = lambda f: f                                                                        # noqa: E731

    def three(f):
        with torch.no_grad():
            return f(F64, ident).numpy(), f(F32, ident).numpy(), f(F32, O.twin).numpy()

    res = [('norm', 'x', three(lambda dt, tw: tw(lambda x: O.norm(x)[0])(T(planes, dt))))]
    for o, i, k in CHAIN:
        res.append(('conv half %s -> %s' % (i, o), o, three(lambda dt, tw: tw(O.conv_half)(T(st[i], dt), W(k, dt)))))
    for p, i, k in POOLED:
        res.append(('pooled conv half %s -> %s' % (i, p), p, three(lambda dt, tw: tw(lambda x, w: O.pool(O.conv_half(x, w)))(T(st[i], dt), W(k, dt)))))
    for t, i, k in TCONV:
        res.append(('transposed conv %s -> %s' % (i, t), t, three(lambda dt, tw: tw(O.tconv_stage)(T(st[i], dt), W(k, dt)))))
    for o, a, b, k in TWO_SOURCE:
        res.append(('two-source conv half %s+%s -> %s' % (a, b, o), o,
                    three(lambda dt, tw: tw(lambda x, y, w: O.conv_half(torch.cat([x, y], dim=1), w))(T(st[a], dt), T(st[b], dt), W(k, dt)))))

    def fin(dt, tw):
        s = T(st['stat'], dt)
        mean, std = s[:, [0, 2]][:, :, None, None], s[:, [1, 3]][:, :, None, None]
        return tw(O.final)(T(st['u2'], dt), W('up_conv.2.1.weight', dt), W('up_conv.2.1.bias', dt), mean, std, T(planes, dt))
    res.append(('1x1 + unnorm + residual', 'out', three(fin)))
    return [(what, name) + refs for what, name, refs in res]


def oracle_stages(sd, net, r, dtype=F32):
    """name -> numpy array of every stage of one oracle evaluation, 'out' included"""
    st = {}
    with torch.no_grad():
        out = O.denoise_planes(sd, net, torch.from_numpy(planes_of(r)).to(dtype), dtype, st)
    st = {k: v.numpy() for k, v in st.items()}
    st['out'] = out.numpy()
    return st


def conv_variances(sd, net, st):
    """[17 x [B, C]] biased variance of every convolution output in front of a norm, the stages ``st`` as its inputs"""
    import torch.nn.functional as Fn
    W = lambda k: torch.from_numpy(sd['update_nets.%d.unet.%s' % (net, k)]).double()           # noqa: E731
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()                          # noqa: E731
    var = lambda y: y.var(dim=(2, 3), unbiased=False).numpy()                                 # noqa: E731
    out = []
    with torch.no_grad():
        for o, i, k in CHAIN + POOLED:
            out.append(var(Fn.conv2d(T(st[i]), W(k), padding=1)))
        for t, i, k in TCONV:
            out.append(var(Fn.conv_transpose2d(T(st[i]), W(k), stride=2)))
        for o, a, b, k in TWO_SOURCE:
            out.append(var(Fn.conv2d(torch.cat([T(st[a]), T(st[b])], dim=1), W(k), padding=1)))
    return out


# ---- 2. the loop ------------------------------------------------------------------------------------------------------------------------
LoopCase = collections.namedtuple('LoopCase', 'name y_scale snr_db weights floor')
LOOP_CASES = [
    LoopCase('y_2m12', 2.0 ** -12, 10.0, 'plain', True),         # max|r| < 1e-2: eps sits on its floor
    LoopCase('y_2m20', 2.0 ** -20, 10.0, 'plain', True),         # and the perturbation eps d is larger than r
    LoopCase('y_2p12', 2.0 ** 12, 10.0, 'plain', False),
    LoopCase('snr_m10', 1.0, -10.0, 'plain', False),
    LoopCase('snr_30', 1.0, 30.0, 'plain', False),
    LoopCase('w_2m10', 1.0, 10.0, 'w_2m10', False),
]
LOOP_B, LOOP_NP, LOOP_SEED = 4, 38, 5
# 3. one batch of four regimes: sample i of the batch is sample i of the problem of MIXED[i]
MIXED = [LoopCase('plain', 1.0, 10.0, 'plain', False), LOOP_CASES[1], LOOP_CASES[2], LOOP_CASES[4]]


def loop_problem(case):
    """(Y, P, eig, directions) of a loop case; the channels, pilots and directions are the same in every case"""
    Y, P, eig, _ = O.synthetic_problem(LOOP_B, LOOP_NP, case.snr_db, LOOP_SEED)
    d = np.random.default_rng(1).standard_normal((UNROLLS, LOOP_B, 64, 16, 2)).astype(np.float32)
    return (Y * np.float32(case.y_scale)).astype(np.complex64), P, eig, d


def mixed_problem():
    parts = [loop_problem(c) for c in MIXED]
    Y = np.stack([parts[i][0][i] for i in range(len(MIXED))])
    return Y, parts[0][1], parts[0][2], parts[0][3]


_LOOP = {}


def loop_refs(case):
    """(float64, float32, float32 flipped) logs of the oracle's three unrolls, computed once"""
    if case.name not in _LOOP:
        sd, fsd = weights(case.weights, UNROLLS)
        Y, P, eig, d = loop_problem(case)
        _LOOP[case.name] = (O.run_oracle(sd, Y, P, eig, d, UNROLLS, F64), O.run_oracle(sd, Y, P, eig, d, UNROLLS, F32),
                            O.run_oracle_flipped(fsd, Y, P, eig, d, UNROLLS, F32))
    return _LOOP[case.name]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def errors(a, ref64, kind):
    """'norm': per-sample norm-wise relative error [B]; 'abs': per-sample absolute error of a scalar [B]"""
    a, ref64 = np.asarray(a), np.asarray(ref64)
    B = ref64.shape[0]
    if kind == 'abs':
        return np.abs(a.astype(np.float64) - ref64.astype(np.float64)).reshape(B)
    num = np.sqrt(np.sum(np.abs(a.reshape(B, -1) - ref64.reshape(B, -1)) ** 2, axis=1))
    return num / np.sqrt(np.sum(np.abs(ref64.reshape(B, -1)) ** 2, axis=1))


def rule(what, got, ref64, ref32, ref32f, kind='norm'):
    """error(got) <= 4 e_ref [+ 2^-23 |ref| for a scalar], e_ref = the larger of the two float32 orders' errors (maximum over
    samples).  Prints the figures; -> (ok, info)."""
    err = errors(got, ref64, kind)
    e_ref = max(float(np.max(errors(ref32, ref64, kind))), float(np.max(errors(ref32f, ref64, kind))))
    slack = ULP * np.abs(np.asarray(ref64, np.float64)).reshape(-1) if kind == 'abs' else 0.0
    worst = float(np.max(err))
    print('%-40s error %.3e   e_ref %.3e   ratio %.2f' % (what, worst, e_ref, worst / max(e_ref, 1e-300)))
    ok = bool(np.all(np.isfinite(err)) and np.isfinite(e_ref) and e_ref > 0 and np.all(err <= FACTOR * e_ref + slack))
    return ok, (what, worst, e_ref)


def mutual(what, ref64, ref32, ref32f, kind='norm'):
    """The reference alone under the rule: each float32 order's error is within 4 x the OTHER's (which is then its e_ref), and both
    are finite and non-zero.  A case that fails this cannot be tested by the rule and is re-parametrised."""
    ea, eb = errors(ref32, ref64, kind), errors(ref32f, ref64, kind)
    a, b = float(np.max(ea)), float(np.max(eb))
    slack = ULP * np.abs(np.asarray(ref64, np.float64)).reshape(-1) if kind == 'abs' else 0.0
    print('%-40s native %.3e   flipped %.3e   ratio %.2f' % (what, a, b, a / max(b, 1e-300)))
    ok = bool(np.isfinite(a) and np.isfinite(b) and a > 0 and b > 0 and np.all(ea <= FACTOR * b + slack) and np.all(eb <= FACTOR * a + slack))
    return ok, (what, a, b)


def assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad
