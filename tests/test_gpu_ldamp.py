"""Learned D-AMP on the GPU (score_based_channels_amd/ldamp.py, csrc/ldamp.hip) against the reference fixtures and the float64 oracle.

The tolerance rule of every comparison here: the fp32 reference itself drifts from float64 (the divergence estimate divides a
difference of two network outputs by eps ~ 1e-3 max|r|), so for a quantity q let e_ref = error of the fp32 reference (fixture; where
there is no fixture, the oracle run in fp32) against float64 -- norm-wise per sample, maximum over samples, for tensors; absolute for
the scalar div -- and require  error(kernel, float64) <= 4 e_ref.  The factor covers another, equally valid fp32 summation order and
the ~2x scatter of a maximum over four samples.  Every figure is printed before it is asserted.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ldamp_cases as LC
import ldamp_oracle as O
from conftest import load_golden
from guarded import cplx as _cplx, planes as _planes
from score_based_channels_amd import _lib, ldamp

pytestmark = pytest.mark.gpu
HP = {'backbone': 'FlippedUNet', 'shared_nets': False, 'max_unrolls': 10, 'in_channels': 2}
FACTOR = 4.0


@pytest.fixture(scope='module')
def weights():
    return ldamp.seeded_state_dict(int(load_golden('ldamp_unet.npz')['seed_weights']))


@pytest.fixture(scope='module')
def model(weights):
    return ldamp.LDAMP(HP, device='cuda:0').load_state_dict(weights).eval()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def sample_of(Y, P, eig):
    return {'Y_herm': dev(Y), 'P_herm': dev(P), 'eig1': dev(eig)}


def host_logs(logs):
    return {k: v.cpu().numpy() for k, v in logs.items()}


def check(what, got, ref64, ref32, kind='norm'):
    f = O.normwise if kind == 'norm' else O.absolute
    err, e_ref = f(got, ref64), f(ref32, ref64)
    print('%-28s kernel %.3e   e_ref %.3e   ratio %.2f' % (what, err, e_ref, err / max(e_ref, 1e-300)))
    return err <= FACTOR * e_ref, (what, err, e_ref)


def assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad


@pytest.mark.parametrize('net', [0, 9])
def test_one_evaluation(model, weights, net):
    """net 0 against the reference fixture; net 9 (no fixture) against the oracle, fp32 oracle as the stand-in for the reference"""
    g = O.golden_unet()
    got = model.denoise(net, dev(g['r'])).cpu().numpy()
    if net == 0:
        ref64, ref32 = g['out64'], g['out32']
    else:
        ref64, ref32 = O.denoise(weights, net, g['r'], torch.float64), O.denoise(weights, net, g['r'], torch.float32)
    assert_all([check('denoise net %d' % net, got, ref64, ref32)])


def kernel_stages(model, net, r):
    """one evaluation on the GPU -> every stage as the kernel left it in the workspace (name -> array), the output planes as 'out'"""
    out = model.denoise(net, dev(r)).cpu().numpy()
    st = {n: model.stage(n).cpu().numpy() for n in ldamp.STAGES}
    st['out'] = np.stack((out.real, out.imag), axis=1)
    assert np.array_equal(st['r'][..., 0] + 1j * st['r'][..., 1], r)
    return st


def each_layer_kind(model, state_dict, r, net, twin=False):
    """Every launch of one evaluation on its own: the stage's input as the kernel left it in the workspace goes through the oracle's layer in
    float64 and float32; the kernel's output of that stage is held to the rule.  Kinds: norm, first ConvBlock (x -> d0a -> d0), pooled
    ConvBlock (-> p0 / p1 / p2: the pool is the producer's epilogue), the 8x2 bottleneck (ba, bb), transposed-conv stages (t0, t1, t2),
    two-source ConvBlocks (u0a, u1a, u2a), and the 1x1 with unnorm and residual (the output).  ``twin``: e_ref is the larger of the
    native and the flipped float32 order (tests/ldamp_cases.py) instead of the native one alone."""
    st = kernel_stages(model, net, r)
    res = []
    for what, name, ref64, ref32, ref32f in LC.layer_refs(state_dict, net, st, LC.planes_of(r)):
        res.append(LC.rule(what, st[name], ref64, ref32, ref32f) if twin else check(what, st[name], ref64, ref32))
    assert len(res) == 22
    assert_all(res)


def test_each_layer_kind(model, weights):
    each_layer_kind(model, weights, O.golden_unet()['r'], 0)


_MODELS = {}


def model_of(regime, max_unrolls):
    """the model of a weight regime of tests/ldamp_cases.py, made once"""
    if (regime, max_unrolls) not in _MODELS:
        sd, _ = LC.weights(regime, max_unrolls)
        _MODELS[regime, max_unrolls] = ldamp.LDAMP(dict(HP, max_unrolls=max_unrolls), device='cuda:0').load_state_dict(sd).eval()
    return _MODELS[regime, max_unrolls]


@pytest.mark.parametrize('case', LC.LAYER_CASES, ids=lambda c: c.name)
def test_each_layer_kind_under_regimes(case):
    """Weight scales at which IN_EPS dominates every norm or vanishes, input scales and an offset that ``norm`` has to remove, nets 4
    and 9 (the offset into the weight block), B = 1 and 5: every stage by the rule."""
    n = 10 if case.weights == 'plain' else LC.UNROLLS
    each_layer_kind(model_of(case.weights, n), LC.weights(case.weights, n)[0], LC.layer_input(case), case.net, twin=True)


def test_ten_unrolls_against_the_reference(model):
    u = O.golden_unroll()
    H_hat, logs = model(sample_of(u['Y_herm'], u['P_herm'], u['eig1']), 10, directions=u['directions'], return_logs=True, H=dev(u['H_herm_cplx']))
    L = host_logs(logs)
    res = []
    for k in range(10):
        res.append(check('unroll %d h' % k, L['h'][k], u['h64'][k], u['h32'][k]))
        res.append(check('unroll %d z' % k, L['z'][k], u['z64'][k], u['z32'][k]))
        res.append(check('unroll %d div' % k, L['div'][k], u['div64'][k], u['div32'][k], 'abs'))
        # eps = fp32(1e-3) * max hypot(re, im) of r: three fp32 roundings (r's last, the hypot, the product) on top of r's inherited error,
        # which the reference's own eps error measures
        rel = np.max(np.abs(L['eps'][k] / u['eps64'][k] - 1))
        rel_ref = np.max(np.abs(u['eps32'][k].astype(np.float64) / u['eps64'][k] - 1))
        print('unroll %d eps                 kernel %.3e   e_ref %.3e' % (k, rel, rel_ref))
        res.append((rel <= FACTOR * rel_ref + 3 * 2.0 ** -24, ('eps', k, rel, rel_ref)))
    assert np.array_equal(H_hat.cpu().numpy(), L['h'][9])
    nm = np.sum(np.abs(L['h'][9] - u['H_herm_cplx']) ** 2, (1, 2)) / np.sum(np.abs(u['H_herm_cplx']) ** 2, (1, 2))
    assert np.max(np.abs(L['nmse'] / nm - 1)) < 1e-5                  # the kernel's NMSE of its own h (fp32 differences, double sums)
    assert_all(res)


@pytest.mark.parametrize('Np', [1, 12, 38, 64])
def test_pilot_counts(model, weights, Np):
    Y, P, eig, _ = O.synthetic_problem(4, Np, 10.0, 21 + Np)
    d = np.random.default_rng(Np).standard_normal((3, 4, 64, 16, 2)).astype(np.float32)
    _, logs = model(sample_of(Y, P, eig), 3, directions=d, return_logs=True)
    L = host_logs(logs)
    r64, r32 = O.run_oracle(weights, Y, P, eig, d, 3, torch.float64), O.run_oracle(weights, Y, P, eig, d, 3, torch.float32)
    res = []
    for k in range(3):
        res.append(check('Np %d unroll %d h' % (Np, k), L['h'][k], r64['h'][k], r32['h'][k]))
        res.append(check('Np %d unroll %d z' % (Np, k), L['z'][k], r64['z'][k], r32['z'][k]))
        res.append(check('Np %d unroll %d div' % (Np, k), L['div'][k], r64['div'][k], r32['div'][k], 'abs'))
    assert_all(res)


def run_logs(m, Y, P, eig, d, unrolls=LC.UNROLLS, **kw):
    H_hat, logs = m(sample_of(Y, P, eig), unrolls, directions=d, return_logs=True, **kw)
    L = host_logs(logs)
    L['H_hat'] = H_hat.cpu().numpy()
    return L


@pytest.mark.parametrize('case', LC.LOOP_CASES, ids=lambda c: c.name)
def test_the_loop_under_regimes(case):
    """Three unrolls, B = 4, fixed directions: measurements so small that eps sits on its floor (and, at 2^-20, the perturbation is larger
    than r), large ones, -10 and 30 dB, weights at which IN_EPS dominates.  h, z, div, eps per unroll by the rule."""
    Y, P, eig, d = LC.loop_problem(case)
    L = run_logs(model_of(case.weights, LC.UNROLLS), Y, P, eig, d)
    r64, r32, r32f = LC.loop_refs(case)
    print('eps: kernel %s, float64 %s' % (L['eps'][:, 0], r64['eps'][:, 0]))
    if case.floor:                                                    # the floor branch is what ran, at every unroll
        assert L['eps'].dtype == np.float32 and np.all(L['eps'] == np.float32(LC.EPS_FLOOR)) and np.all(r64['eps'] == LC.EPS_FLOOR)
    else:
        assert np.all(L['eps'] > 2 * LC.EPS_FLOOR)
    res = []
    for k in range(LC.UNROLLS):
        for q, kind in (('h', 'norm'), ('z', 'norm'), ('div', 'abs'), ('eps', 'abs')):
            res.append(LC.rule('%s unroll %d %s' % (case.name, k, q), L[q][k], r64[q][k], r32[q][k], r32f[q][k], kind))
    assert np.array_equal(L['H_hat'], L['h'][-1])
    assert_all(res)


def test_a_mixed_batch_equals_its_single_sample_calls():
    """normal, Y x 2^-20, Y x 2^12 and 30 dB in one call: the per-sample eps / stat reductions do not leak between samples"""
    m = model_of('plain', LC.UNROLLS)
    Y, P, eig, d = LC.mixed_problem()
    mixed = run_logs(m, Y, P, eig, d)
    assert mixed['eps'][0, 1] == np.float32(LC.EPS_FLOOR) and mixed['eps'][0, 2] > 1 and np.all(np.isfinite(mixed['h']))
    for i in range(4):
        one = run_logs(m, Y[i:i + 1], P[i:i + 1], eig[i:i + 1], d[:, i:i + 1])
        for k in ('h', 'z', 'div', 'eps'):
            assert np.array_equal(one[k][:, 0], mixed[k][:, i]), (i, k)
        assert np.array_equal(one['H_hat'][0], mixed['H_hat'][i]), i


def test_fewer_nets_one_unroll_and_an_empty_batch():
    ten, three = model_of('plain', 10), model_of('plain', LC.UNROLLS)
    Y, P, eig, d = LC.loop_problem(LC.MIXED[0])
    a, b = run_logs(ten, Y, P, eig, d), run_logs(three, Y, P, eig, d)
    for k in ('h', 'z', 'div', 'eps', 'H_hat'):
        assert np.array_equal(a[k], b[k]), k                          # the first three nets of ten are the three-net model
    one = run_logs(ten, Y, P, eig, d[:1], unrolls=1)
    for k in ('h', 'z', 'div', 'eps'):
        assert one[k].shape[0] == 1 and np.array_equal(one[k][0], a[k][0]), k
    assert np.array_equal(one['H_hat'], a['h'][0])
    with pytest.raises(ValueError, match='num_unrolls'):
        three(sample_of(Y, P, eig), 4)
    empty = run_logs(ten, Y[:0], P[:0], eig[:0], d[:, :0])
    assert empty['H_hat'].shape == (0, 64, 16) and empty['h'].shape == (3, 0, 64, 16) and empty['z'].shape == (3, 0, 38, 16)
    assert empty['div'].shape == (3, 0) and empty['eps'].shape == (3, 0)
    assert tuple(ten.denoise(0, dev(np.zeros((0, 64, 16), np.complex64))).shape) == (0, 64, 16)


def behind_a_matmul(stream, sources):
    """Fresh device tensors that become copies of ``sources`` ON ``stream``, queued behind a large matrix product: until that has run
    they hold zeros, so a launch on another stream would read them unready.  The side stream first waits for the current one."""
    a = torch.randn(4096, 4096, device='cuda:0')
    src = [dev(s) for s in sources]
    out = [torch.zeros_like(s) for s in src]
    torch.cuda.synchronize()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        b = a @ a
        b = b @ a
        for o, s in zip(out, src):
            o.copy_(s).mul_(2.0).mul_(0.5)
    return out, b


def test_a_callers_stream():
    m = model_of('plain', LC.UNROLLS)
    Y, P, eig, d = LC.loop_problem(LC.MIXED[0])
    r = LC.layer_input(LC.LAYER_CASES[-1])
    want = run_logs(m, Y, P, eig, d)
    want_d = m.denoise(1, dev(r)).cpu().numpy()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    (rs,), keep = behind_a_matmul(side, [r])
    got_d = m.denoise(1, rs, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(got_d.cpu().numpy(), want_d)
    torch.cuda.synchronize()
    (Ys, Ps, es, ds), keep = behind_a_matmul(side, [Y, P, eig, d])
    H_hat, logs = m({'Y_herm': Ys, 'P_herm': Ps, 'eig1': es}, LC.UNROLLS, directions=ds, return_logs=True, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    got = host_logs(logs)
    for k in ('h', 'z', 'div', 'eps'):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(H_hat.cpu().numpy(), want['H_hat'])
    torch.cuda.synchronize()
    del keep


def test_batch_size_and_repetition_do_not_change_a_bit(model):
    Y, P, eig, _ = O.synthetic_problem(100, 38, 5.0, 33)
    d = np.random.default_rng(8).standard_normal((3, 100, 64, 16, 2)).astype(np.float32)
    runs = {}
    for B in (100, 3, 1, 100):
        _, logs = model(sample_of(Y[:B], P[:B], eig[:B]), 3, directions=d[:, :B], return_logs=True)
        L = host_logs(logs)
        if B in runs:
            assert all(np.array_equal(L[k], runs[B][k]) for k in L), 'a repeated run differs'
        runs[B] = L
    assert np.all(np.isfinite(runs[100]['h']))
    for B in (3, 1):
        for k in ('h', 'z', 'div', 'eps'):
            assert np.array_equal(runs[B][k], runs[100][k][:, :B]), (B, k)
    # the same sample at another position of the batch
    _, logs = model(sample_of(Y[2:7], P[2:7], eig[2:7]), 3, directions=d[:, 2:7], return_logs=True)
    L = host_logs(logs)
    assert all(np.array_equal(L[k], runs[100][k][:, 2:7]) for k in ('h', 'z', 'div', 'eps'))


def test_device_directions_and_their_host_replay(model):
    Y, P, eig, _ = O.synthetic_problem(4, 38, 10.0, 44)
    ids = np.arange(10, 14)
    _, logs = model(sample_of(Y, P, eig), 3, seed=5, sample_ids=ids, return_logs=True)
    L = host_logs(logs)
    replay = ldamp.replay_directions(5, ids, 3)
    # the directions the run drew lie behind the evaluations, z and eps in its workspace (include/sbc_hip.h)
    ws, n = model.last_workspace
    off, _ = ldamp.stage_layout('stat', 1)
    start = n * (off + 4) + 4 * (2 * 1024 + 16)
    used = ws[start:start + replay.size].cpu().numpy().reshape(replay.shape)
    assert np.array_equal(used, replay)
    assert abs(replay.mean()) < 0.02 and abs(replay.std() - 1) < 0.02 and np.all(np.isfinite(replay))
    assert not np.array_equal(replay[0, 0], replay[0, 1]) and not np.array_equal(replay[0, 0], replay[1, 0])
    assert not np.array_equal(ldamp.replay_directions(6, ids[:1], 1), replay[:1, :1])
    _, logs2 = model(sample_of(Y, P, eig), 3, directions=replay, return_logs=True)
    L2 = host_logs(logs2)
    assert all(np.array_equal(L[k], L2[k]) for k in L)
    # a sample's draws depend on its global id, not on its position
    _, logs3 = model(sample_of(Y[1:3], P[1:3], eig[1:3]), 3, seed=5, sample_ids=ids[1:3], return_logs=True)
    assert np.array_equal(host_logs(logs3)['h'], L['h'][:, 1:3])


CLI = ['--synthetic', '--seed', '1', '--noise', 'host', '--snr_range', '0', '20', '--num_channels', '8', '--no_plot']


def test_cli_end_to_end_against_the_oracle(tmp_path, monkeypatch):
    from score_based_channels_amd import test_ldamp as T
    monkeypatch.chdir(tmp_path)
    got = T.main(CLI + ['--synthetic_weights', '7'])['nmse_log']
    sd = ldamp.seeded_state_dict(7)
    ref = {}

    def oracle(dtype):
        def f(model, batch, num_unrolls, directions, seed, device):
            h = O.run_oracle(sd, batch['Y_herm'], batch['P_herm'], batch['eig1'], directions, num_unrolls, dtype)['h'][-1]
            H = batch['H_herm_cplx']
            return np.sum(np.abs(h - H) ** 2, (1, 2)) / np.sum(np.abs(H) ** 2, (1, 2))
        return f
    for dtype in (torch.float64, torch.float32):           # the same numpy stream: the same data, noise and directions
        ref[dtype] = T.main(CLI + ['--synthetic_weights', '7'], estimate_fn=oracle(dtype))['nmse_log']
    assert got.shape == (1, 1, 2, 8) and np.all(np.isfinite(got))
    res = [check('CLI nmse, SNR point %d' % s, got[0, 0, s], ref[torch.float64][0, 0, s], ref[torch.float32][0, 0, s], 'abs') for s in range(2)]
    assert_all(res)


def test_cli_from_checkpoints(tmp_path, monkeypatch):
    """Checkpoints written with save_checkpoint under the reference's path pattern give what --synthetic_weights gives."""
    from score_based_channels_amd import test_ldamp as T
    from score_based_channels_amd.checkpoint import save_checkpoint
    monkeypatch.chdir(tmp_path)
    want = T.main(CLI + ['--synthetic_weights', '7'])['nmse_log']
    for snr in (0.0, 20.0):
        path = T.checkpoint_path('CDL-C', snr, 0.6)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        save_checkpoint(path, ldamp.seeded_state_dict(7), T.ldamp_config('CDL-C', 0.6))
    got = T.main(CLI)['nmse_log']
    assert np.array_equal(got, want)
    assert os.path.exists('results/ldamp/train-CDL-C_test-CDL-C/results.pt')


def test_rejected_settings_raise(model, weights):
    for bad in ({'backbone': 'DnCNN'}, {'backbone': 'UNet'}, {'shared_nets': True}):
        with pytest.raises(ValueError):
            ldamp.LDAMP(dict(HP, **bad))
    Y, P, eig, _ = O.synthetic_problem(2, 38, 10.0, 3)
    with pytest.raises(ValueError, match='geometry'):
        model(sample_of(Y[:, :, :8], P, eig), 3)
    with pytest.raises(ValueError, match='num_unrolls'):
        model(sample_of(Y, P, eig), 11)
    with pytest.raises(RuntimeError):
        ldamp.LDAMP(HP)(sample_of(Y, P, eig), 3)                      # no weights
    short = dict(weights)
    short.pop('update_nets.9.unet.up_conv.2.1.bias')
    with pytest.raises(KeyError):
        ldamp.LDAMP(HP).load_state_dict(short)
    # the library refuses by itself too, before any launch
    s = sample_of(Y, P, eig)
    out = torch.full((2, 64, 16), 7.0, dtype=torch.complex64, device='cuda:0')
    ws = torch.empty(int(_lib.lib().sbc_ldamp_workspace_floats(2, 3)), device='cuda:0')
    p = lambda t: C.c_void_p(t.data_ptr())                          # noqa: E731
    for field, val in (('Nt', 32), ('Nr', 8), ('Np', 65), ('Np', 0), ('num_unrolls', 11), ('B', -1)):
        kw = dict(Y_herm=p(s['Y_herm']), P_herm=p(s['P_herm']), eig1=p(s['eig1']), H_hat=p(out), workspace=p(ws), B=2, Np=38, Nt=64, Nr=16, num_unrolls=3)
        kw[field] = val
        d = _lib.sbc_ldamp_run_desc(**kw)
        assert _lib.lib().sbc_ldamp_run(model._h, C.byref(d), None) == -1, field
        assert field in _lib.lib().sbc_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)


# ---- guarded operands, and a workspace of exactly sbc_ldamp_workspace_floats(B, num_unrolls) floats (tests/guarded.py) -----------------
# Through the C calls directly, as test_rejected_settings_raise does: every operand, output and log is a view into a larger allocation
# with guarded margins, the workspace has exactly the documented size between pads of one per-sample stride and starts as NaN (the
# library promises nothing about what it holds), and the results are held to the rule with the references the tests above share.

def _guarded_workspace(g, B, U):
    f = _lib.lib().sbc_ldamp_workspace_floats
    n = int(f(B, U))
    assert n > 0
    return g.out('workspace (%d floats, B %d unrolls %d)' % (n, B, U), (n,), must_write=False, pad=max(1024, int(f(B + 1, U)) - n))


def guarded_denoise(m, net, r):
    from guarded import Guard
    g = Guard(torch, 'cuda:0')
    B = r.shape[0]
    p = lambda t: C.c_void_p(t.data_ptr())                           # noqa: E731
    dr, out, ws = g.inp('r', _planes(r)), g.out('out', (B, 64, 16, 2)), _guarded_workspace(g, B, 0)
    _lib.check(_lib.lib().sbc_ldamp_denoise(m._h, int(net), p(dr), p(out), B, p(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    g.check()
    return _cplx(out)


def guarded_run(m, Y, P, eig, d, U, H=None):
    from guarded import Guard
    g = Guard(torch, 'cuda:0')
    B, Np = Y.shape[:2]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    inp = {k: g.inp(k, a) for k, a in dict(Y_herm=_planes(Y), P_herm=_planes(P), eig1=np.asarray(eig, np.float32), directions=d[:U]).items()}
    dH = g.inp('Htrue', _planes(H)) if H is not None else None
    out = dict(H_hat=g.out('H_hat', (B, 64, 16, 2)), h_log=g.out('h_log', (U, B, 64, 16, 2)), z_log=g.out('z_log', (U, B, Np, 16, 2)),
               div_log=g.out('div_log', (U, B)), eps_log=g.out('eps_log', (U, B)))
    nmse = g.out('nmse', (B,)) if H is not None else None
    ws = _guarded_workspace(g, B, U)
    desc = _lib.sbc_ldamp_run_desc(Htrue=p(dH), nmse=p(nmse), workspace=p(ws), B=B, Np=Np, Nt=64, Nr=16, num_unrolls=U,
                                   **{k: p(t) for k, t in list(inp.items()) + list(out.items())})
    _lib.check(_lib.lib().sbc_ldamp_run(m._h, C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    g.check()
    L = {'H_hat': _cplx(out['H_hat']), 'h': _cplx(out['h_log']), 'z': _cplx(out['z_log']), 'div': out['div_log'].cpu().numpy(),
         'eps': out['eps_log'].cpu().numpy()}
    if nmse is not None:
        L['nmse'] = nmse.cpu().numpy()
    return L


@pytest.mark.parametrize('B', [1, 3])
def test_denoise_with_guarded_operands_and_an_exact_workspace(model, B):
    """unrolls = 0: one evaluation.  The first B samples of the reference fixture, held to the fixture's bound; and the Python host's call
    (its workspace is the allocator's) returns the same bits."""
    g = O.golden_unet()
    got = guarded_denoise(model, 0, g['r'][:B])
    err, e_ref = O.normwise(got, g['out64'][:B]), O.normwise(g['out32'], g['out64'])
    print('guarded denoise B %d: kernel %.3e   e_ref %.3e' % (B, err, e_ref))
    assert err <= FACTOR * e_ref
    assert np.array_equal(got, model.denoise(0, dev(g['r'][:B])).cpu().numpy())


@pytest.mark.parametrize('U', [1, 3])
@pytest.mark.parametrize('B', [1, 3])
def test_the_loop_with_guarded_operands_and_an_exact_workspace(B, U):
    """The first B samples and the first U unrolls of the plain loop case: h, z, div, eps per unroll within the bound test_the_loop_under_regimes
    holds the whole case to (e_ref of its four samples), the NMSE of the library's own estimate, and the same bits as the Python host's call."""
    case = LC.MIXED[0]
    m = model_of(case.weights, LC.UNROLLS)
    Y, P, eig, d = LC.loop_problem(case)
    H = O.synthetic_problem(Y.shape[0], Y.shape[1], case.snr_db, LC.LOOP_SEED)[3]
    L = guarded_run(m, Y[:B], P[:B], eig[:B], d[:, :B], U, H[:B])
    r64, r32, r32f = LC.loop_refs(case)
    bad = []
    for k in range(U):
        for q, kind in (('h', 'norm'), ('z', 'norm'), ('div', 'abs'), ('eps', 'abs')):
            err = LC.errors(L[q][k], r64[q][k][:B], kind)
            e_ref = max(float(np.max(LC.errors(r32[q][k], r64[q][k], kind))), float(np.max(LC.errors(r32f[q][k], r64[q][k], kind))))
            slack = LC.ULP * np.abs(np.asarray(r64[q][k][:B], np.float64)).reshape(-1) if kind == 'abs' else 0.0
            print('guarded B %d U %d unroll %d %-3s error %.3e   e_ref %.3e' % (B, U, k, q, float(np.max(err)), e_ref))
            if not (np.all(np.isfinite(err)) and e_ref > 0 and np.all(err <= FACTOR * e_ref + slack)):
                bad.append((k, q, float(np.max(err)), e_ref))
    assert not bad, bad
    assert np.array_equal(L['H_hat'], L['h'][U - 1])
    nm = np.sum(np.abs(L['H_hat'] - H[:B]) ** 2, (1, 2)) / np.sum(np.abs(H[:B]) ** 2, (1, 2))
    assert np.max(np.abs(L['nmse'] / nm - 1)) < 1e-5
    want = run_logs(m, Y[:B], P[:B], eig[:B], d[:U, :B], unrolls=U)
    for k in ('h', 'z', 'div', 'eps', 'H_hat'):
        assert np.array_equal(L[k], want[k]), k


def test_a_mixed_batch_with_guarded_operands_and_an_exact_workspace():
    """The batch of test_a_mixed_batch_equals_its_single_sample_calls: guarded, it returns the bits the Python host's call returns.  The link
    to a reference is indirect here: that test ties the host call's bits to the single-sample calls, and test_the_loop_under_regimes holds
    those to the oracle; the guarded B / unroll grid above compares with the references itself."""
    m = model_of('plain', LC.UNROLLS)
    Y, P, eig, d = LC.mixed_problem()
    L = guarded_run(m, Y, P, eig, d, LC.UNROLLS)
    want = run_logs(m, Y, P, eig, d)
    assert L['eps'][0, 1] == np.float32(LC.EPS_FLOOR) and np.all(np.isfinite(L['h']))
    for k in ('h', 'z', 'div', 'eps', 'H_hat'):
        assert np.array_equal(L[k], want[k]), k
