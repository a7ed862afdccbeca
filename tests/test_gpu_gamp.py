"""sbc_em_gm_amp_run (csrc/cs_gamp.hip) against the float64 restatement of its definition (tests/gamp_oracle.py).

The bound is the project's standing one: the kernel's distance from float64 is at most 4 x the float32 restatement's own distance
from float64, with a floor of 8 * 2^-24 of the largest magnitude (gamp_oracle.assert_within), per problem and per quantity.  Every
launch of this module reads and writes guarded operands (tests/guarded.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import gamp_cases as K
import gamp_oracle as O
import guarded
from conftest import rel_err_elementwise

pytestmark = pytest.mark.gpu

NT, NR = 64, 16
OK, INVALID, UNSUPPORTED = 0, -1, -3


@pytest.fixture(autouse=True)
def _guard():
    import torch
    g = guarded.begin(torch)
    yield g
    guarded.end()


def _ri(a):
    a = np.ascontiguousarray(a)
    return a.view(a.real.dtype)


def _desc(P, Y, H, nit, em_iters, tol, theta, p_index, h_index, outs=('nmse', 'H_hat', 'X', 'params', 'stop_iter'), over=None):
    """A descriptor over guarded operands; returns (desc, {name: output tensor})."""
    import torch
    from score_based_channels_amd import _lib
    B, Np = Y.shape[0], Y.shape[1]
    f = dict(P=guarded.ptr(guarded.dev(torch, guarded.planes(P), 'P')), Y=guarded.ptr(guarded.dev(torch, guarded.planes(Y), 'Y')),
             B=B, nP=P.shape[0], nH=H.shape[0] if H is not None else 0, Nt=P.shape[2], Nr=Y.shape[2], Np=Np, nit=nit, em_iters=em_iters,
             theta=theta, tol=tol)
    if H is not None:
        f['Htrue'] = guarded.ptr(guarded.dev(torch, guarded.planes(H), 'Htrue'))
    if p_index is not None:
        f['p_index'] = guarded.ptr(guarded.dev(torch, np.asarray(p_index, np.int32), 'p_index'))
    if h_index is not None and H is not None:
        f['h_index'] = guarded.ptr(guarded.dev(torch, np.asarray(h_index, np.int32), 'h_index'))
    shapes = dict(nmse=(em_iters, B), H_hat=(B, NT, NR, 2), X=(B, NT, NR, 2), params=(B, 10), stop_iter=(B,))
    o = {}
    for name in outs:
        if name == 'nmse' and H is None:
            continue
        o[name] = guarded.out(shapes[name], name, dtype=torch.int32 if name == 'stop_iter' else None,
                              **({'fill': -7} if name == 'stop_iter' else {}))
        f[name] = guarded.ptr(o[name])
    f.update(over or {})
    return _lib.sbc_em_gm_amp_desc(**f), o


def _call(desc, stream=None):
    import torch
    from score_based_channels_amd import _lib
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = _lib.lib().sbc_em_gm_amp_run(C.byref(desc), C.c_void_p(s.cuda_stream))
    return rc, (_lib.lib().sbc_last_error() or b'').decode()


def _fetch(o):
    r = {}
    for name, t in o.items():
        r[name] = guarded.cplx(t) if name in ('H_hat', 'X') else t.cpu().numpy()
    return r


def _run(P, Y, H, nit=10, em_iters=200, tol=0.0, theta=0.3, p_index=None, h_index=None, check_inf=True, **kw):
    import torch
    desc, o = _desc(P, Y, H, nit, em_iters, tol, theta, p_index, h_index, **kw)
    rc, msg = _call(desc)
    assert rc == OK, msg
    torch.cuda.synchronize()
    guarded.current.check(written=check_inf)
    return _fetch(o)


def _compare(tag, got, r32, r64, figures):
    """X, H_hat, the four parameter groups and the log of every problem under the standing bound."""
    B = r64['X'].shape[0]
    groups = dict(lam=slice(0, 1), om=slice(1, 5), phi=slice(5, 9), psi=slice(9, 10))
    for b in range(B):
        for name in ('X', 'H_hat'):
            figures.append((tag, b, name) + O.assert_within('%s problem %d %s' % (tag, b, name), got[name][b], r32[name][b], r64[name][b]))
        for name, sl in groups.items():
            figures.append((tag, b, name) + O.assert_within('%s problem %d %s' % (tag, b, name), got['params'][b, sl], r32['params'][b, sl],
                                                             r64['params'][b, sl]))
        figures.append((tag, b, 'log') + O.assert_within('%s problem %d log' % (tag, b), got['nmse'][:, b], r32['log'][:, b], r64['log'][:, b]))
        assert got['stop_iter'][b] == r64['stop_iter'][b]


def _report(figures):
    worst = {}
    for tag, b, name, err, lim in figures:
        k = (tag, name)
        if k not in worst or err / lim > worst[k][0] / worst[k][1]:
            worst[k] = (err, lim)
    for (tag, name), (err, lim) in sorted(worst.items()):
        print('%-28s %-6s error %.3e  bound %.3e  (%.2f of it)' % (tag, name, err, lim, err / lim))


SNRS = (-30.0, 0.0, 15.0)


def _oracle(*args, **kw):
    """The restatement on the very inputs the kernel gets: the descriptor carries theta as a float, so 0.3 reaches the kernel as
    0.3f, and over hundreds of iterations that difference alone moves a trajectory (tests/test_gamp_cpu.py:
    test_early_stop_cases_are_clear_of_the_tolerance)."""
    kw['theta'] = float(np.float32(kw.get('theta', 0.3)))
    return O.run(*args, **kw)


@pytest.mark.parametrize('n_pilots', [1, 6, 12, 16, 17, 38, 48, 64])
def test_first_em_iterations_match_the_oracle(n_pilots):
    """Short horizon, elementwise: after 1, 2 and 3 EM iterations of 10 GAMP iterations (no stopping) and after 3 EM iterations of
    1 and of 3, at -30, 0 and 15 dB, three problems per SNR on two pilot matrices through p_index."""
    P, Y, H, pidx, hidx, _ = K.problem(n_pilots, SNRS, 3)
    figures = []
    try:
        for nit, em_iters in ((10, 1), (10, 2), (10, 3), (1, 3), (3, 3)):
            got = _run(P, Y, H, nit=nit, em_iters=em_iters, tol=0.0, p_index=pidx, h_index=hidx)
            r64 = _oracle(P, Y, H, nit=nit, em_iters=em_iters, tol=0.0, p_index=pidx, h_index=hidx)
            r32 = _oracle(P, Y, H, nit=nit, em_iters=em_iters, tol=0.0, p_index=pidx, h_index=hidx, dtype=np.float32)
            _compare('Np=%d nit=%d em=%d' % (n_pilots, nit, em_iters), got, r32, r64, figures)
    finally:
        _report(figures)


@functools.lru_cache(maxsize=None)
def _long_case(n_pilots):
    P, Y, H, pidx, hidx, _ = K.problem(n_pilots, (-10.0, 0.0, 10.0, 15.0), 1, seed=3)
    r64 = _oracle(P, Y, H, tol=0.0, p_index=pidx, h_index=hidx)
    r32 = _oracle(P, Y, H, tol=0.0, p_index=pidx, h_index=hidx, dtype=np.float32)
    return P, Y, H, pidx, hidx, r64, r32


def _self_consistent(got, H):
    """H_hat = Fl X Fr of the returned X (float64) to 1e-5 elementwise (5 % floor); log[-1] = the float64 NMSE of the returned
    H_hat to 1e-6 relative: the kernel forms the log from the very fp32 H_hat it returns, in a float64 sum of squares of fp32
    differences (the bounds and their derivation: tests/cs_checks.py, check_l1_consistency)."""
    Fl, Fr = O.idft_factor(NT), O.idft_factor(NR)
    fwd = O.spatial(got['X'].astype(np.complex128), Fl, Fr)
    H64, Hh = H.astype(np.complex128), got['H_hat'].astype(np.complex128)
    nm = np.sum(np.abs(Hh - H64) ** 2, axis=(1, 2)) / np.sum(np.abs(H64) ** 2, axis=(1, 2))
    last = got['nmse'][got['stop_iter'] - 1, np.arange(len(nm))].astype(np.float64)
    f = dict(forward=rel_err_elementwise(_ri(got['H_hat']), _ri(fwd)), log=float(np.max(np.abs(last / nm - 1))))
    assert f['forward'] <= 1e-5 and f['log'] <= 1e-6, f
    return f


@pytest.mark.parametrize('n_pilots', [12, 38, 64])
def test_full_schedule(n_pilots):
    """Long horizon, 200 x 10 without stopping.  Elementwise agreement is NOT asserted: the float32 restatement itself ends up to
    0.6 of max|X| from float64 after 2000 iterations (the iteration is not contractive at that resolution).  Asserted: (a) finite
    outputs; (b) self-consistency of X, H_hat and log[-1]; (c) a k-iteration run gives the first k log rows bit for bit; (d) the
    final NMSE in dB within twice the largest |float32 restatement - float64| over the same problems, measured here."""
    P, Y, H, pidx, hidx, r64, r32 = _long_case(n_pilots)
    got = _run(P, Y, H, tol=0.0, p_index=pidx, h_index=hidx)
    assert all(np.all(np.isfinite(_ri(v))) for v in got.values()) and np.all(got['stop_iter'] == 200)
    print('Np=%d self-consistency after 200 x 10: %s' % (n_pilots, _self_consistent(got, H[hidx])))
    for k in (1, 7):
        gk = _run(P, Y, H, em_iters=k, tol=0.0, p_index=pidx, h_index=hidx)
        assert gk['nmse'].tobytes() == got['nmse'][:k].tobytes(), k
        _self_consistent(gk, H[hidx])
    db = lambda v: 10 * np.log10(np.asarray(v, np.float64))
    own = float(np.max(np.abs(db(r32['log'][-1]) - db(r64['log'][-1]))))
    err = float(np.max(np.abs(db(got['nmse'][-1]) - db(r64['log'][-1]))))
    print('Np=%d final NMSE: float64 %s dB, kernel %s dB, float32 restatement %s dB; kernel off by %.4f dB, restatement by %.4f dB, '
          'margin %.4f dB' % (n_pilots, np.round(db(r64['log'][-1]), 3), np.round(db(got['nmse'][-1]), 3), np.round(db(r32['log'][-1]), 3),
                              err, own, 2 * own))
    assert err <= 2 * own, (err, own)


STOP_CASES = K.STOP_CASES


@functools.lru_cache(maxsize=None)
def _stop_case(n_pilots, tol):
    P, Y, H, pidx, hidx, _ = K.problem(n_pilots, (-10.0, 0.0, 15.0), 2, seed=5)
    r64 = _oracle(P, Y, H, em_iters=40, tol=tol, p_index=pidx, h_index=hidx, return_crit=True)
    return P, Y, H, pidx, hidx, r64


def clear_of_the_tolerance(crit, tol):
    """problems whose float64 criterion stays outside tol (1 +- 1e-3) at every EM iteration that ran"""
    near = np.abs(crit / tol - 1) <= 1e-3
    return ~np.any(near & np.isfinite(crit), axis=0)


@pytest.mark.parametrize('n_pilots,tol', STOP_CASES)
def test_early_stop(n_pilots, tol):
    """stop_iter and the position of the sentinel rows equal float64's on every problem whose float64 criterion is clear of the
    tolerance; the seeds are chosen so that this is all of them (tests/test_gamp_cpu.py checks it on the CPU as well)."""
    P, Y, H, pidx, hidx, r64 = _stop_case(n_pilots, tol)
    clear = clear_of_the_tolerance(r64['crit'], tol)
    assert np.all(clear), 'a problem was left out'
    got = _run(P, Y, H, em_iters=40, tol=tol, p_index=pidx, h_index=hidx)
    print('Np=%d tol=%g: stop_iter %s (float64 %s)' % (n_pilots, tol, got['stop_iter'], r64['stop_iter']))
    assert np.array_equal(got['stop_iter'], r64['stop_iter'])
    assert np.array_equal(got['nmse'] == O.SENTINEL, r64['log'] == O.SENTINEL)
    assert np.any(r64['stop_iter'] < 40) and np.all(r64['stop_iter'] >= 2)
    _self_consistent(got, H[hidx])


def test_batch_position_and_repeat_are_bit_identical():
    """A problem alone, first, in the middle and last of batches of 1, 5 and 257 gives identical bits; the batch run twice too."""
    P, Y, H, pidx, hidx, _ = K.problem(17, (0.0,), 1)
    one = _run(P, Y, H, em_iters=3, tol=1e-1, p_index=pidx, h_index=hidx)
    rng = np.random.default_rng(3)
    for B in (5, 257):
        Pb, Yb, Hb, pb, hb, _ = K.problem(17, (-5.0, 5.0), (B + 1) // 2, seed=1)
        Yb, pb, hb = Yb[:B].copy(), pb[:B].copy(), hb[:B].copy()
        Pn, Hn = np.concatenate([Pb, P[:1]]), np.concatenate([Hb, H[:1]])
        spots = (0, B // 2, B - 1)
        for s in spots:
            Yb[s], pb[s], hb[s] = Y[0], len(Pb), len(Hb)
        got = _run(Pn, Yb, Hn, em_iters=3, tol=1e-1, p_index=pb, h_index=hb)
        for s in spots:
            for name in ('X', 'H_hat', 'params', 'stop_iter'):
                assert got[name][s].tobytes() == one[name][0].tobytes(), (B, s, name)
            assert got['nmse'][:, s].tobytes() == one['nmse'][:, 0].tobytes(), (B, s)
        again = _run(Pn, Yb, Hn, em_iters=3, tol=1e-1, p_index=pb, h_index=hb)
        assert all(got[k].tobytes() == again[k].tobytes() for k in got), B


def test_poisoned_problems_stay_isolated():
    """A NaN in one problem's Y and an out-of-range p_index / h_index mark only their own problem (the bad indices: NaN outputs,
    stop_iter -1, nothing read through them)."""
    P, Y, H, pidx, hidx, _ = K.problem(38, (0.0, 10.0), 3)
    clean = _run(P, Y, H, em_iters=2, p_index=pidx, h_index=hidx)
    Yp, pp, hp = Y.copy(), pidx.copy(), hidx.copy()
    Yp[1, 5, 3] = np.nan
    pp[2], hp[4] = 10 ** 6, -1
    got = _run(P, Yp, H, em_iters=2, p_index=pp, h_index=hp, check_inf=False)
    for b in range(6):
        if b in (1, 2, 4):
            assert np.all(np.isnan(got['nmse'][:, b])) and np.all(np.isnan(_ri(got['X'][b]))) and np.all(np.isnan(_ri(got['H_hat'][b])))
            assert np.all(np.isnan(got['params'][b])) and got['stop_iter'][b] == (2 if b == 1 else -1)
        else:
            assert all(got[k][b].tobytes() == clean[k][b].tobytes() for k in ('X', 'H_hat', 'params', 'stop_iter')), b
            assert got['nmse'][:, b].tobytes() == clean['nmse'][:, b].tobytes(), b


def test_null_outputs_streams_and_the_empty_batch():
    """Every output is optional (without Htrue there is no log); a caller's stream works; B = 0 is accepted and writes nothing."""
    import torch
    P, Y, H, pidx, hidx, _ = K.problem(16, (5.0,), 3)
    full = _run(P, Y, H, em_iters=2, p_index=pidx, h_index=hidx)
    for outs in (('nmse',), ('H_hat',), ('X',), ('params', 'stop_iter'), ('nmse', 'X')):
        got = _run(P, Y, H, em_iters=2, p_index=pidx, h_index=hidx, outs=outs)
        assert set(got) == set(outs) and all(got[k].tobytes() == full[k].tobytes() for k in outs), outs
    got = _run(P, Y, None, em_iters=2, p_index=pidx, outs=('H_hat', 'X', 'params', 'stop_iter'))
    assert all(got[k].tobytes() == full[k].tobytes() for k in got)
    got = _run(P[pidx], Y, H, em_iters=2)                      # NULL index maps: problem b reads matrix b
    assert all(got[k].tobytes() == full[k].tobytes() for k in got)
    side = torch.cuda.Stream()
    desc, o = _desc(P, Y, H, 10, 2, 0.0, 0.3, pidx, hidx)
    side.wait_stream(torch.cuda.current_stream())
    rc, msg = _call(desc, side)
    assert rc == OK, msg
    side.synchronize()
    guarded.current.check()
    assert all(v.tobytes() == full[k].tobytes() for k, v in _fetch(o).items())
    desc, o = _desc(P, Y, H, 10, 2, 0.0, 0.3, pidx, hidx, over=dict(B=0))
    assert _call(desc)[0] == OK
    torch.cuda.synchronize()
    guarded.current.check(written=False)
    assert all(np.all(np.isnan(v.cpu().numpy())) for k, v in o.items() if k != 'stop_iter') and np.all(o['stop_iter'].cpu().numpy() == -7)


REFUSALS = [
    (dict(Nt=32), UNSUPPORTED, 'unsupported'), (dict(Nr=8), UNSUPPORTED, 'unsupported'), (dict(Np=0), UNSUPPORTED, 'unsupported'),
    (dict(Np=65), UNSUPPORTED, 'unsupported'), (dict(nit=0), UNSUPPORTED, 'unsupported'), (dict(em_iters=0), UNSUPPORTED, 'unsupported'),
    (dict(theta=0.0), UNSUPPORTED, 'unsupported'), (dict(theta=1.5), UNSUPPORTED, 'unsupported'),
    (dict(theta=float('nan')), UNSUPPORTED, 'unsupported'),
    (dict(tol=-1.0), INVALID, 'tol'), (dict(tol=float('nan')), INVALID, 'tol'), (dict(tol=float('inf')), INVALID, 'tol'),
    (dict(B=-1), INVALID, 'B >= 0'), (dict(nP=0), INVALID, 'nP >= 1'), (dict(nH=0), INVALID, 'nH >= 1'),
    (dict(P=None), INVALID, 'NULL P'), (dict(Y=None), INVALID, 'NULL Y'), (dict(Htrue=None), INVALID, 'nmse needs Htrue'),
]


def test_refusals_write_nothing():
    """Every refusal of the header returns its code and message and leaves every output as it was."""
    import torch
    from score_based_channels_amd import _lib
    P, Y, H, pidx, hidx, _ = K.problem(16, (5.0,), 2)
    for over, code, text in REFUSALS:
        desc, o = _desc(P, Y, H, 10, 2, 1e-1, 0.3, pidx, hidx, over=over)
        rc, msg = _call(desc)
        assert rc == code and text in msg and 'sbc_em_gm_amp_run' in msg, (over, rc, msg)
        torch.cuda.synchronize()
        guarded.current.check(written=False)
        assert all(np.all(np.isnan(v.cpu().numpy())) for k, v in o.items() if k != 'stop_iter'), over
        assert np.all(o['stop_iter'].cpu().numpy() == -7), over
    assert _lib.lib().sbc_em_gm_amp_run(None, None) == INVALID


def test_python_entry_matches_the_raw_call():
    """baselines.em_gm_amp hands the same problem to the same launch: identical bits, on a caller's stream too."""
    import torch
    from score_based_channels_amd.baselines import em_gm_amp
    P, Y, H, pidx, hidx, _ = K.problem(38, (0.0,), 3)
    raw = _run(P, Y, H, em_iters=3, tol=1e-1, p_index=pidx, h_index=hidx)
    for stream in (None, torch.cuda.Stream()):
        log, Hh, stop, X, par = em_gm_amp(P, Y, H, em_iters=3, p_index=pidx, h_index=hidx, want_x=True, want_params=True, stream=stream)
        (stream or torch.cuda.current_stream()).synchronize()
        assert log.cpu().numpy().tobytes() == raw['nmse'].tobytes() and stop.cpu().numpy().tobytes() == raw['stop_iter'].tobytes()
        assert Hh.cpu().numpy().tobytes() == raw['H_hat'].tobytes() and X.cpu().numpy().tobytes() == raw['X'].tobytes()
        assert par.cpu().numpy().tobytes() == raw['params'].tobytes()
    log, Hh, stop = em_gm_amp(P, Y, None, em_iters=3, p_index=pidx)
    assert log is None and Hh.cpu().numpy().tobytes() == raw['H_hat'].tobytes()


def test_cli_against_the_oracle(tmp_path):
    """``--synthetic --num_samples 4 --snr_range -10 15 --em_iters 3 --noise host`` on one profile against the oracle on the same
    draws (the CLI around the oracle as its solver): the logs within the short-horizon bound."""
    import torch
    from score_based_channels_amd import test_em_gm_amp as cli
    argv = ['--synthetic', '--num_samples', '4', '--snr_range', '-10', '15', '--em_iters', '3', '--noise', 'host', '--seed', '1',
            '--channels', 'CDL-C']
    got = cli.main(argv + ['--result_dir', str(tmp_path / 'gpu')])['CDL-C']

    def oracle(dtype):
        def solve(P, Y, H, index, args, device):
            r = _oracle(P, Y, H, nit=args.nit, em_iters=args.em_iters, tol=args.tol, theta=args.theta, p_index=index, h_index=index, dtype=dtype)
            return r['log'], r['stop_iter']
        return solve
    r64 = cli.main(argv + ['--result_dir', str(tmp_path / 'f64')], solve_fn=oracle(np.float64))['CDL-C']
    r32 = cli.main(argv + ['--result_dir', str(tmp_path / 'f32')], solve_fn=oracle(np.float32))['CDL-C']
    saved = torch.load(str(tmp_path / 'gpu' / 'CDL-C_nit10.pt'), weights_only=False)
    assert saved['complete_log'].shape == (1, 2, 3, 4) and saved['oracle_log'].shape == (1, 2, 4) and saved['best_log'].shape == (1, 2, 4)
    assert np.array_equal(saved['complete_log'], got['complete_log'])
    for si in range(2):
        for n in range(4):
            ran = r64['complete_log'][0, si, :, n] != O.SENTINEL               # the sentinel rows must agree and stay out of the scale
            assert np.array_equal(got['complete_log'][0, si, :, n] != O.SENTINEL, ran)
            assert np.array_equal(r32['complete_log'][0, si, :, n] != O.SENTINEL, ran)
            for name in ('complete_log', 'oracle_log', 'best_log'):
                pick = (lambda a: a[0, si, :, n][ran] if a.ndim == 4 else a[0, si, n:n + 1])
                err, lim = O.assert_within('%s snr %d sample %d' % (name, si, n), pick(got[name]), pick(r32[name]), pick(r64[name]))
    print('CLI logs within the bound; last cell: error %.3e bound %.3e' % (err, lim))
