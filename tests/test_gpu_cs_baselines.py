"""The classical baselines on the GPU (csrc/cs_l1.hip, csrc/cs_ls.hip through baselines.py and the two CLIs), all against the
float64 numpy oracle of tests/cs_oracle.py."""
import numpy as np
import pytest
import torch

import cs_checks as K
import cs_oracle as O
from conftest import rel_err, rel_err_elementwise
from guarded import cplx as _cplx, planes as _planes, ptr as _ptr

pytestmark = pytest.mark.gpu


_data = K.cdl_data
_ri = K.ri


def _gpu_l1(P, Y, H, lam, lr, L, steps, **kw):
    from score_based_channels_amd.baselines import l1_lifted
    out = l1_lifted(torch.from_numpy(P).cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(H).cuda(), lam, lr, lifting=L,
                    steps=steps, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


@pytest.mark.parametrize('L', [1, 2, 4])
@pytest.mark.parametrize('steps', [1, 2, 3])
def test_l1_first_steps_match_the_oracle(L, steps):
    P, Y, H = _data(3, 38, 11, 10.0)
    log, Hh, X = _gpu_l1(P, Y, H, 0.3, 3e-3, L, steps, want_x=True)
    rlog, rH, rX = O.l1_run(P, Y, H, 0.3, 3e-3, L, steps)
    # the bound first holds for the oracle itself in complex64 (the DFT sums cancel, so it is not trivially loose)
    _, cH, cX = O.l1_run(P, Y, H, 0.3, 3e-3, L, steps, dtype=np.complex64)
    assert rel_err_elementwise(_ri(cX), _ri(rX)) < 1e-5 and rel_err_elementwise(_ri(cH), _ri(rH)) < 1e-5
    assert X.shape == (3, 64 * L, 16 * L) and Hh.shape == (3, 64, 16) and log.shape == (steps, 3)
    assert rel_err_elementwise(_ri(X), _ri(rX)) < 1e-5, rel_err_elementwise(_ri(X), _ri(rX))
    assert rel_err_elementwise(_ri(Hh), _ri(rH)) < 1e-5, rel_err_elementwise(_ri(Hh), _ri(rH))
    assert np.max(np.abs(log / rlog - 1)) < 5e-6


@pytest.mark.parametrize('L', [1, 2, 4])
@pytest.mark.parametrize('npil', [1, 2, 12, 25, 51, 63, 64])
def test_l1_first_steps_at_every_pilot_count(npil, L):
    """Np decides G = P^H P, b = P^H Y and the loop bounds of the prologue: the reference's alpha grid (12, 25, 38, 51, 64), the
    ends of the documented range and an odd neighbour, 3 steps, the bounds of test_l1_first_steps_match_the_oracle."""
    P, Y, H = _data(3, npil, 100 + npil, 10.0)
    log, Hh, X = _gpu_l1(P, Y, H, 0.3, 3e-3, L, 3, want_x=True)
    rlog, rH, rX = O.l1_run(P, Y, H, 0.3, 3e-3, L, 3)
    clog, cH, cX = O.l1_run(P, Y, H, 0.3, 3e-3, L, 3, dtype=np.complex64)
    fc, failures = K.check_l1_iterate(clog, cH, cX, rlog, rH, rX)
    assert not failures, failures                               # the oracle itself in complex64 meets the bounds
    fk, failures = K.check_l1_iterate(log, Hh, X, rlog, rH, rX)
    print('l1 3 steps Np=%d L=%d: kernel %s, complex64 oracle %s, H_hat norm-wise %.3g' % (npil, L, fk, fc, rel_err(Hh, rH)))
    assert not failures, failures


@pytest.mark.parametrize('L', [1, 2, 4])
@pytest.mark.parametrize('steps', [1, 2, 3, 10])
def test_l1_partly_sparse_iterate_matches_the_oracle(L, steps):
    """The regime fsAD exists for: lambda per problem at the median of the first gradient step, so that half of the first iterate
    is zero and more later (float64 oracle on these problems: 50 / 52 / 53 / 70 % zeros after 1 / 2 / 3 / 10 steps at L = 1,
    50 / 53 / 56 / 76 % at L = 4).  The zero pattern of X equals the oracle's exactly except where the oracle's pre-threshold |v|
    lies within 1e-5 max|v| of the threshold -- at most 0.073 % of X per problem on these data (3 of 4096 entries at L = 2) (tests/test_cs_baselines_cpu.py::
    test_half_sparse_lambda_on_the_gpu_tests_data; cap 0.1 %) -- and the values meet the bounds of the first-steps test."""
    P, Y, H = _data(4, 38, 31, 10.0)
    lam = K.half_sparse_lambda(P, Y, L)
    log, Hh, X = _gpu_l1(P, Y, H, lam, 3e-3, L, steps, want_x=True)
    rlog, rH, rX, rv = O.l1_run(P, Y, H, lam, 3e-3, L, steps, return_v=True)
    figures, failures = K.check_l1_iterate(log, Hh, X, rlog, rH, rX, rv, lam * 3e-3)
    print('l1 partly sparse L=%d steps=%d: %s' % (L, steps, figures))
    assert not failures, failures
    assert 0.45 <= figures['zero_share'][0] and figures['zero_share'][1] <= 0.85 and np.mean(X == 0) >= 0.45


@pytest.mark.parametrize('L', [1, 2, 4])
def test_l1_thousand_steps_are_self_consistent(L):
    """Free of the null-space drift that limits the comparison with the oracle after 1000 steps: the returned H_hat, X and
    log[-1] are one iterate (cs_checks.check_l1_consistency: H_hat = Ld X Rd to 1e-5 element-wise, log[-1] = NMSE of H_hat to
    1e-6), with and without the l1 term; and the step loop does not depend on ``steps``: a run of k steps gives the first k log
    rows of the 1000-step run bit for bit, and its own H_hat / X / log[-1] are consistent in the same way."""
    lam = np.array([0.0, 0.3, 0.0, 0.3])
    P, Y, H = _data(4, 38, 61, np.array([10.0, 10.0, 30.0, -10.0]))
    log, Hh, X = _gpu_l1(P, Y, H, lam, 3e-3, L, 1000, want_x=True)
    assert np.all(np.isfinite(log))
    figures, failures = K.check_l1_consistency(log[-1], Hh, X, H, L)
    print('l1 self-consistency L=%d after 1000 steps: %s' % (L, figures))
    assert not failures, failures
    for k in (1, 7, 250):
        lk, hk, xk = _gpu_l1(P, Y, H, lam, 3e-3, L, k, want_x=True)
        assert lk.tobytes() == log[:k].tobytes(), k
        figures, failures = K.check_l1_consistency(lk[-1], hk, xk, H, L)
        print('l1 self-consistency L=%d after %d steps: %s' % (L, k, figures))
        assert not failures, (k, failures)


def test_l1_poisoned_problems_stay_isolated():
    """A NaN in one problem's Y and an Inf in a pilot matrix that one other problem uses (through p_index): their logs are
    non-finite from the first step on, and every other problem of the batch of 64 is bit-identical to the clean batch."""
    B, nch, steps = 64, 8, 40
    P0, _, H = _data(nch, 38, 71, 10.0)
    rng = np.random.default_rng(71)
    idx = np.arange(B) % nch
    z = (rng.standard_normal((B, 38, 16)) + 1j * rng.standard_normal((B, 38, 16))) / np.sqrt(2)
    Y = (P0[idx] @ H[idx] + np.sqrt(1.6) * z).astype(np.complex64)
    P = np.concatenate([P0, P0[3:4]])                          # matrix nch: a copy of matrix 3, used by problem 43 only
    pidx = idx.copy()
    pidx[43] = nch
    lam = np.where(np.arange(B) % 2, 0.3, 0.0)
    from score_based_channels_amd.baselines import l1_lifted

    def run(Pm, Ym):
        log, Hh = l1_lifted(torch.from_numpy(Pm).cuda(), torch.from_numpy(Ym).cuda(), torch.from_numpy(H).cuda(), lam, 3e-3, lifting=4,
                            steps=steps, p_index=pidx, h_index=idx)
        torch.cuda.synchronize()
        return log.cpu().numpy(), Hh.cpu().numpy()

    log0, H0 = run(P, Y)
    assert np.all(np.isfinite(log0))
    Pp, Yp = P.copy(), Y.copy()
    Yp[17, 5, 3] = np.nan
    Pp[nch, 20, 11] = np.inf
    log1, H1 = run(Pp, Yp)
    assert not np.any(np.isfinite(log1[:, [17, 43]])), log1[:3, [17, 43]]
    keep = np.setdiff1d(np.arange(B), [17, 43])
    assert log1[:, keep].tobytes() == log0[:, keep].tobytes() and H1[keep].tobytes() == H0[keep].tobytes()


def _full_run_check(L, npil, seed, snr, lam):
    B = len(snr)
    P, Y, H = _data(B, npil, seed, snr)
    log, Hh = _gpu_l1(P, Y, H, lam, 3e-3, L, 1000)
    rlog, rH, _ = O.l1_run(P, Y, H, lam, 3e-3, L, 1000)
    err = np.abs(log / rlog - 1)
    eH = [np.linalg.norm(Hh[b] - rH[b]) / np.linalg.norm(rH[b]) for b in range(B)]
    print('l1 full run L=%d Np=%d: log error %.3g (20 steps) %.3g (100) %.3g (1000); H_hat %s'
          % (L, npil, np.max(err[:20]), np.max(err[:100]), np.max(err), ' '.join('%.2g' % e for e in eH)))
    assert np.max(err[:20]) <= 5e-6, np.max(err[:20])
    assert np.max(err[:100]) <= 2e-4, np.max(err[:100])
    assert np.max(err) <= 5e-3, np.max(err)
    # final estimate, norm-wise.  With lambda = 0 the problem is unregularised and under-determined (Np = 38 < Nt = 64): rounding
    # drifts along the null space.  The kernel's formulation (G = P^H P, Hz by linearity) restated in numpy complex64 ends
    # 2.0e-3 .. 2.4e-3 from the float64 oracle on these lambda = 0 cells and <= 5.2e-4 on the lambda = 0.3 cells (L = 1 and 4).
    for b in range(B):
        assert eH[b] <= (2e-3 if lam[b] > 0 else 5e-3), (b, lam[b], eH[b])


@pytest.mark.parametrize('L', [1, 2, 4])
def test_l1_full_run_log_matches_the_oracle(L):
    snrs, lams, per = [-10.0, 10.0, 30.0], [0.0, 0.3], 2
    cells = [(s, lam) for s in snrs for lam in lams]
    snr = np.repeat([c[0] for c in cells], per)
    lam = np.repeat([c[1] for c in cells], per)
    _full_run_check(L, 38, 21, snr, lam)


@pytest.mark.parametrize('npil', [12, 64])
def test_l1_full_run_at_other_pilot_counts(npil):
    """1000 steps at the ends of the reference's alpha range (Np = 12: G of rank 12; Np = 64: square), L = 4, the bounds of the
    Np = 38 run; 4 problems: 10 dB with and without the l1 term, -10 and 30 dB with it."""
    _full_run_check(4, npil, 200 + npil, np.array([10.0, 10.0, -10.0, 30.0]), np.array([0.0, 0.3, 0.3, 0.3]))


def test_l1_threshold_above_the_first_gradient_keeps_x_zero():
    P, Y, H = _data(4, 38, 31, 10.0)
    Ld, Rd = O.dictionaries(64, 16, 4)
    g0 = O.fw_op_H(P.astype(np.complex128), Ld, Rd, -Y.astype(np.complex128))
    lr = 3e-3
    lam = 1.5 * np.max(np.abs(lr * g0), axis=(1, 2)) / lr
    log, Hh, X = _gpu_l1(P, Y, H, lam, lr, 4, 50, want_x=True)
    assert np.all(X == 0) and np.all(Hh == 0)
    assert np.max(np.abs(log - 1)) <= 1e-6


def test_l1_grid_is_batch_independent_and_reproducible():
    nch, steps = 16, 200
    P, Y0, H = _data(nch, 38, 41, 10.0)
    rng = np.random.default_rng(7)
    B = 2048
    idx = np.arange(B) % nch
    snr = np.array([-10.0, 0.0, 10.0, 20.0])[(np.arange(B) // nch) % 4]
    noise = 10 ** (-snr / 10.) * 16
    z = (rng.standard_normal((B, 38, 16)) + 1j * rng.standard_normal((B, 38, 16))) / np.sqrt(2)
    Y = (P[idx] @ H[idx] + np.sqrt(noise)[:, None, None] * z).astype(np.complex64)
    lam = np.array([0.0, 0.1, 0.3, 1.0])[(np.arange(B) // 64) % 4]
    lr = np.array([1e-3, 3e-3])[(np.arange(B) // 256) % 2]
    lr[1234] = 1e-2                                             # one diverging cell (step above 1 / ||P||^2)
    from score_based_channels_amd.baselines import l1_lifted

    def run(sel):
        log, Hh = l1_lifted(torch.from_numpy(P).cuda(), torch.from_numpy(Y[sel]).cuda(), torch.from_numpy(H).cuda(), lam[sel],
                            lr[sel], lifting=4, steps=steps, p_index=idx[sel], h_index=idx[sel])
        torch.cuda.synchronize()
        return log.cpu().numpy(), Hh.cpu().numpy()

    full = np.arange(B)
    log1, H1 = run(full)
    log2, H2 = run(full)
    assert log1.tobytes() == log2.tobytes() and H1.tobytes() == H2.tobytes()
    for b in (0, 777, 1234, 2047):
        lb, hb = run(np.array([b]))
        assert lb[:, 0].tobytes() == log1[:, b].tobytes(), b
        assert hb[0].tobytes() == H1[b].tobytes(), b
    d = log1[:, 1234]
    assert not np.isfinite(d[-1]) or d[-1] > 1e3 * d[0], d[[0, -1]]
    assert np.all(np.isfinite(np.delete(log1, 1234, axis=1)))


def _gpu_ls(P, Y, noise, H=None, **kw):
    from score_based_channels_amd.baselines import ls_regularized
    Hh, nmse = ls_regularized(torch.from_numpy(P).cuda(), torch.from_numpy(Y).cuda(), noise,
                              H=torch.from_numpy(H).cuda() if H is not None else None, **kw)
    torch.cuda.synchronize()
    return Hh.cpu().numpy(), nmse.cpu().numpy() if nmse is not None else None


def _report(tag, figures):
    for f in figures:
        print('ML %s s2=%-8.3g kappa %-8.2g H_hat: restatement %.2e kernel %.2e ratio %.2f | residual: %.2e %.2e ratio %.2f | nmse %.2e (bound %.2e)'
              % (tag, f['noise'], f['kappa'], f['e_c'], f['e_k'], f['e_ratio'], f['r_c'], f['r_k'], f['r_ratio'],
                 f.get('nmse_err', np.nan), f.get('nmse_bound', np.nan)))


def test_ls_regularized_matches_lstsq():
    snr = np.arange(-30, 17.5, 2.5)
    for npil in (38, 64):
        P, _, H = _data(8, npil, 51 + npil, 0.0)
        B = len(snr) * 8
        idx = np.tile(np.arange(8), len(snr))
        noise = np.repeat(10 ** (-snr / 10.), 8)
        rng = np.random.default_rng(npil)
        z = (rng.standard_normal((B, npil, 16)) + 1j * rng.standard_normal((B, npil, 16))) / np.sqrt(2)
        Y = (P[idx] @ H[idx] + np.sqrt(noise)[:, None, None] * z).astype(np.complex64)
        Hh, nmse = _gpu_ls(P, Y, noise, H, p_index=idx, h_index=idx)
        rH, rn = O.lstsq_run(P[idx].astype(np.complex128), Y.astype(np.complex128), H[idx].astype(np.complex128), noise)
        eH = np.linalg.norm((Hh - rH).reshape(B, -1), axis=1) / np.linalg.norm(rH.reshape(B, -1), axis=1)
        assert np.max(eH) <= 1e-4, (npil, np.max(eH))
        assert np.max(np.abs(nmse / rn - 1)) <= 3e-4, (npil, np.max(np.abs(nmse / rn - 1)))
        # and the conditioning-aware yardstick: 4 x the single-precision restatement per SNR point (cs_checks.check_ls)
        figures, failures = K.check_ls(Hh, nmse, P[idx], Y, H[idx], noise)
        _report('CDL-C SNR grid Np=%d' % npil, figures)
        assert not failures, (npil, failures)


@pytest.mark.parametrize('npil,nt,nr', K.LS_GRID)
def test_ls_geometry_grid(npil, nt, nr):
    """Every geometry class the header accepts (cs_checks.LS_GRID), 16 problems on 4 pilot matrices and 4 channels through
    p_index / h_index, noise variances 1e-3, 10^-1.5, 1, 1e3 in one launch, against lstsq in float64 under the bounds of
    cs_checks.check_ls: 4 x the error and 4 x the residual of the single-precision restatement of the same problems."""
    P, Y, H, pidx, hidx, noise = K.ls_problem(npil, nt, nr, 1000 + 7 * npil + nt + nr)
    Hh, nmse = _gpu_ls(P, Y, noise, H, p_index=pidx, h_index=hidx)
    assert Hh.shape == (16, nt, nr) and nmse.shape == (16,)
    figures, failures = K.check_ls(Hh, nmse, P[pidx], Y, H[hidx], noise)
    _report('(%d, %d, %d)' % (npil, nt, nr), figures)
    assert len(figures) == 4 and not failures, failures


def test_ls_on_cdl_channels_with_index_maps():
    """The grid's bounds on the CDL-C channels of _data(): 16 problems on 4 pilot matrices and 4 channels, Np = 38."""
    P, _, H = _data(4, 38, 81, 0.0)
    _, Y, _, pidx, hidx, noise = K.ls_problem(38, 64, 16, 81)
    rng = np.random.default_rng(82)
    z = (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape)) / np.sqrt(2)
    Y = (P[pidx] @ H[hidx] + np.sqrt(noise)[:, None, None] * z).astype(np.complex64)
    Hh, nmse = _gpu_ls(P, Y, noise, H, p_index=pidx, h_index=hidx)
    figures, failures = K.check_ls(Hh, nmse, P[pidx], Y, H[hidx], noise)
    _report('CDL-C (38, 64, 16)', figures)
    assert len(figures) == 4 and not failures, failures


@pytest.mark.parametrize('npil,nt,nr', [(38, 64, 16), (12, 64, 16), (100, 33, 5)])
def test_ls_noise_variance_beyond_the_cli_range(npil, nt, nr):
    """noise_var is a float32: 1e-6 and 1e6 (the CLI spans 10^-1.5 .. 1e3) under the bounds of the grid.  The system of size
    min(Np, Nt) has full rank, so a tiny s2 does not make it ill-conditioned."""
    P, Y, H, pidx, hidx, noise = K.ls_problem(npil, nt, nr, 7 + npil, noises=(1e-6, 1e6))
    Hh, nmse = _gpu_ls(P, Y, noise, H, p_index=pidx, h_index=hidx)
    figures, failures = K.check_ls(Hh, nmse, P[pidx], Y, H[hidx], noise)
    _report('(%d, %d, %d)' % (npil, nt, nr), figures)
    assert len(figures) == 2 and not failures, failures


@pytest.mark.parametrize('npil,nt,nr', [(38, 64, 16), (100, 33, 5)])
def test_ls_without_h_alone_and_twice(npil, nt, nr):
    """Bit-identity between launches, for one case of each solution form: without H the estimate is the same and nmse is None;
    a problem run alone equals its row of the batch; the same batch twice gives the same bits."""
    P, Y, H, pidx, hidx, noise = K.ls_problem(npil, nt, nr, 90 + npil)
    Hh, nmse = _gpu_ls(P, Y, noise, H, p_index=pidx, h_index=hidx)
    H2, n2 = _gpu_ls(P, Y, noise, H, p_index=pidx, h_index=hidx)
    assert H2.tobytes() == Hh.tobytes() and n2.tobytes() == nmse.tobytes()
    H3, n3 = _gpu_ls(P, Y, noise, None, p_index=pidx)
    assert n3 is None and H3.tobytes() == Hh.tobytes()
    for b in (0, 6, 15):
        hb, nb = _gpu_ls(P, Y[b:b + 1], noise[b:b + 1], H, p_index=pidx[b:b + 1], h_index=hidx[b:b + 1])
        assert hb[0].tobytes() == Hh[b].tobytes() and nb.tobytes() == nmse[b:b + 1].tobytes(), b
    assert np.all(np.isfinite(_ri(Hh))) and np.all(np.isfinite(nmse))


def _load(path):
    return torch.load(path, weights_only=False)


def test_l1_cli_end_to_end(tmp_path, monkeypatch):
    from score_based_channels_amd import test_l1Fourier_lifted as cli
    monkeypatch.chdir(tmp_path)
    argv = ['--synthetic', '--seed', '1', '--kept_samples', '3', '--steps', '60', '--lmbda', '0.1', '0.3', '--lr', '1e-3',
            '3e-3', '--no_plot']
    cli.main(argv)
    path = tmp_path / 'results' / 'l1CS_lifted4' / 'train-CDL-C_test-CDL-C' / 'results.pt'
    got = _load(path)
    ref = O.l1_script(seed=1, kept_samples=3, steps=60, lmbda=(0.1, 0.3), lr=(1e-3, 3e-3))
    assert set(got) == set(ref) | {'config', 'args'}
    for k, v in ref.items():
        assert np.asarray(got[k]).shape == v.shape and np.asarray(got[k]).dtype == v.dtype, k
    for k in ('snr_range', 'spacing_range', 'alpha_range', 'lmbda_range', 'lr_range'):
        assert np.array_equal(got[k], ref[k]), k
    err = np.abs(got['complete_log'] / ref['complete_log'] - 1)
    assert np.max(err[..., :20, :]) <= 5e-6 and np.max(err) <= 2e-4, (np.max(err[..., :20, :]), np.max(err))
    assert np.array_equal(got['nmse_log'], got['complete_log'][..., -1, :])
    avg = got['nmse_log'].mean(-1)[0, 0]
    for s in range(avg.shape[-1]):
        i = np.argmin(avg[..., s].flatten())
        assert got['best_nmse'][0, s] == avg[..., s].flatten()[i]
        assert got['best_lmbda'][0, s] == [0.1, 0.3][i // 2] and got['best_lr'][0, s] == [1e-3, 3e-3][i % 2]
    cli.main(argv)
    again = _load(path)
    for k in ref:
        assert np.array_equal(again[k], got[k]), k


def test_ml_cli_end_to_end(tmp_path, monkeypatch):
    from score_based_channels_amd import test_ml as cli
    monkeypatch.chdir(tmp_path)
    argv = ['--synthetic', '--seed', '1', '--kept_samples', '3', '--alpha', '0.6', '1.0']
    cli.main(argv)
    path = tmp_path / 'results_ml_baseline' / 'model_CDL-D_channel_CDL-D' / 'results_Nt64_Nr16.pt'
    got = _load(path)
    ref = O.ml_script(seed=1, kept_samples=3, alpha=(0.6, 1.0))
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert np.asarray(got[k]).shape == v.shape and np.asarray(got[k]).dtype == v.dtype, k
    assert got['oracle_log'].shape == (1, 2, 19, 3)
    assert np.max(np.abs(got['oracle_log'] / ref['oracle_log'] - 1)) <= 3e-4
    cli.main(argv)
    assert np.array_equal(_load(path)['oracle_log'], got['oracle_log'])



@pytest.mark.parametrize('extra,name', [(['--alpha', '0.4', '0.8'], 'l1CS_lifted4'), (['--lifting', '1'], 'l1CS_lifted1')])
def test_l1_cli_at_other_alphas_and_liftings(tmp_path, monkeypatch, extra, name):
    """Np = 25 and 51 in one run, and --lifting 1, against the script's restatement; the bounds of test_l1_cli_end_to_end."""
    from score_based_channels_amd import test_l1Fourier_lifted as cli
    monkeypatch.chdir(tmp_path)
    cli.main(['--synthetic', '--seed', '1', '--kept_samples', '3', '--steps', '60', '--no_plot'] + extra)
    results = tmp_path / 'results'
    assert [p.name for p in results.iterdir()] == [name]
    got = _load(results / name / 'train-CDL-C_test-CDL-C' / 'results.pt')
    kw = dict(alpha=(0.4, 0.8)) if '--alpha' in extra else dict(lifting=1)
    ref = O.l1_script(seed=1, kept_samples=3, steps=60, **kw)
    assert set(got) == set(ref) | {'config', 'args'}
    for k, v in ref.items():
        assert np.asarray(got[k]).shape == v.shape and np.asarray(got[k]).dtype == v.dtype, k
    for k in ('snr_range', 'spacing_range', 'alpha_range', 'lmbda_range', 'lr_range', 'best_lmbda', 'best_lr'):
        assert np.array_equal(got[k], ref[k]), k
    err = np.abs(got['complete_log'] / ref['complete_log'] - 1)
    print('l1 CLI %s: log error %.3g (20 steps) %.3g (60)' % (extra, np.max(err[..., :20, :]), np.max(err)))
    assert np.max(err[..., :20, :]) <= 5e-6 and np.max(err) <= 2e-4, (np.max(err[..., :20, :]), np.max(err))
    assert np.array_equal(got['nmse_log'], got['complete_log'][..., -1, :])
    assert np.array_equal(got['best_nmse'], got['nmse_log'].mean(-1)[0, :, 0, 0])
    assert got['args'].lifting == kw.get('lifting', 4) and got['complete_log'].shape[1] == len(kw.get('alpha', (0.6,)))


def test_ml_cli_at_alpha_0p2(tmp_path, monkeypatch):
    """Np = 12.  The bound is the yardstick of test_ls_geometry_grid carried to the NMSE: at (12, 64, 16) the single-precision
    restatement is within 2e-7 of lstsq at every noise variance (kappa <= 5), so the kernel within 8e-7; an estimate from 12
    pilots leaves NMSE >= 0.5 (at most 12 of 64 dimensions are seen), so the propagation factor 2 ||H_ref|| / ||H_ref - H|| is
    at most 2 sqrt(2) / sqrt(0.5) = 4 and the relative NMSE error at most 3.2e-6 + 2^-23: 1e-5 is asserted."""
    from score_based_channels_amd import test_ml as cli
    monkeypatch.chdir(tmp_path)
    cli.main(['--synthetic', '--seed', '1', '--kept_samples', '3', '--alpha', '0.2'])
    got = _load(tmp_path / 'results_ml_baseline' / 'model_CDL-D_channel_CDL-D' / 'results_Nt64_Nr16.pt')
    ref = O.ml_script(seed=1, kept_samples=3, alpha=(0.2,))
    assert set(got) == set(ref) and got['oracle_log'].shape == (1, 1, 19, 3)
    assert np.array_equal(got['alpha_range'], ref['alpha_range']) and np.array_equal(got['snr_range'], ref['snr_range'])
    err = np.max(np.abs(got['oracle_log'] / ref['oracle_log'] - 1))
    print('ML CLI alpha 0.2: NMSE error %.3g, smallest NMSE %.3g' % (err, ref['oracle_log'].min()))
    assert ref['oracle_log'].min() >= 0.5
    assert err <= 1e-5, err



# ---- outputs and logs between guarded margins (tests/guarded.py): one geometry per dispatch path --------------------------------------
@pytest.mark.parametrize('L', [1, 2, 4])
def test_l1_with_guarded_operands(L):
    """l1_lifted_kernel<1>, <2>, <4> through sbc_l1_lifted_run directly: the problem and the bounds of test_l1_first_steps_match_the_oracle
    (three steps), no write outside H_hat, X and the log, no input touched, and the bits the Python wrapper returns."""
    import ctypes as C
    from guarded import Guard
    from score_based_channels_amd import _lib
    P, Y, H = _data(3, 38, 11, 10.0)
    B, steps, lam, lr = 3, 3, 0.3, 3e-3
    g = Guard(torch)
    d = {k: g.inp(k, a) for k, a in dict(P=_planes(P), Y=_planes(Y), Htrue=_planes(H), p_index=np.arange(B, dtype=np.int32),
                                         h_index=np.arange(B, dtype=np.int32), lmbda=np.full(B, lam, np.float32), lr=np.full(B, lr, np.float32)).items()}
    log, Hh, X = g.out('nmse log', (steps, B)), g.out('H_hat', (B, 64, 16, 2)), g.out('X', (B, 64 * L, 16 * L, 2))
    desc = _lib.sbc_l1_lifted_desc(nmse=_ptr(log), H_hat=_ptr(Hh), X=_ptr(X), B=B, nP=B, nH=B, Nt=64, Nr=16, Np=38, lifting=L, steps=steps,
                                   **{k: _ptr(t) for k, t in d.items()})
    _lib.check(_lib.lib().sbc_l1_lifted_run(C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    g.check()
    log, Hh, X = log.cpu().numpy(), _cplx(Hh), _cplx(X)
    rlog, rH, rX = O.l1_run(P, Y, H, lam, lr, L, steps)
    assert rel_err_elementwise(_ri(X), _ri(rX)) < 1e-5 and rel_err_elementwise(_ri(Hh), _ri(rH)) < 1e-5
    assert np.max(np.abs(log / rlog - 1)) < 5e-6
    wlog, wH, wX = _gpu_l1(P, Y, H, lam, lr, L, steps, want_x=True)
    assert log.tobytes() == wlog.tobytes() and Hh.tobytes() == wH.tobytes() and X.tobytes() == wX.tobytes()


@pytest.mark.parametrize('with_h', [True, False])
def test_ls_with_guarded_operands(with_h):
    """sbc_ls_regularized directly, with and without Htrue: a problem and the bounds of test_ls_geometry_grid, no write outside H_hat
    and nmse, no input touched, and the bits the Python wrapper returns."""
    import ctypes as C
    from guarded import Guard
    from score_based_channels_amd import _lib
    npil, nt, nr = 38, 64, 16
    P, Y, H, pidx, hidx, noise = K.ls_problem(npil, nt, nr, 1000 + 7 * npil + nt + nr)
    B = Y.shape[0]
    g = Guard(torch)
    d = {k: g.inp(k, a) for k, a in dict(P=_planes(P), Y=_planes(Y), p_index=np.asarray(pidx, np.int32), noise_var=np.asarray(noise, np.float32)).items()}
    if with_h:
        d.update(Htrue=g.inp('Htrue', _planes(H)), h_index=g.inp('h_index', np.asarray(hidx, np.int32)))
    Hh, nmse = g.out('H_hat', (B, nt, nr, 2)), g.out('nmse', (B,)) if with_h else None
    desc = _lib.sbc_ls_desc(H_hat=_ptr(Hh), nmse=_ptr(nmse), B=B, nP=P.shape[0], nH=H.shape[0] if with_h else 0, Nt=nt, Nr=nr, Np=npil,
                            **{k: _ptr(t) for k, t in d.items()})
    _lib.check(_lib.lib().sbc_ls_regularized(C.byref(desc), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    g.check()
    wH, wn = _gpu_ls(P, Y, noise, H if with_h else None, p_index=pidx, **(dict(h_index=hidx) if with_h else {}))
    Hh = _cplx(Hh)
    assert Hh.tobytes() == wH.tobytes()
    if with_h:
        nmse = nmse.cpu().numpy()
        assert nmse.tobytes() == wn.tobytes()
        figures, failures = K.check_ls(Hh, nmse, P[pidx], Y, H[hidx], noise)
        assert len(figures) == 4 and not failures, failures
    else:
        assert wn is None
        figures, failures = K.check_ls(Hh, None, P[pidx], Y, None, noise)          # the bounds of test_ls_geometry_grid on the estimate
        assert len(figures) == 4 and not failures, failures
        assert Hh.tobytes() == _gpu_ls(P, Y, noise, H, p_index=pidx, h_index=hidx)[0].tobytes()      # and the bits of the Htrue case
