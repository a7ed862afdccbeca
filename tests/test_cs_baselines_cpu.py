"""CPU checks of the classical baselines (Lasso / fsAD, ML): the numpy oracle's algebra (tests/cs_oracle.py), the CLIs' arguments
and result paths, and the host-side refusals of score_based_channels_amd/baselines.py (no GPU needed: they raise before any
launch)."""
import os

import numpy as np
import pytest

import cs_checks as K
import cs_oracle as O
from score_based_channels_amd import baselines, test_l1Fourier_lifted as l1cli, test_ml as mlcli


def _problem(rng, B=2, np_=38, nt=64, nr=16):
    H = (rng.standard_normal((B, nt, nr)) + 1j * rng.standard_normal((B, nt, nr))) / np.sqrt(2)
    P = ((2 * rng.integers(0, 2, (B, np_, nt)) - 1) + 1j * (2 * rng.integers(0, 2, (B, np_, nt)) - 1)) / np.sqrt(2)
    Y = P @ H + 0.1 * (rng.standard_normal((B, np_, nr)) + 1j * rng.standard_normal((B, np_, nr)))
    return P, Y, H


@pytest.mark.parametrize('L', [1, 2, 4])
def test_dictionaries_are_tight_frames_and_the_adjoint_is_the_adjoint(L):
    Ld, Rd = O.dictionaries(64, 16, L)
    assert Ld.shape == (64, 64 * L) and Rd.shape == (16 * L, 16)
    assert np.allclose(Ld @ Ld.conj().T, np.eye(64), atol=1e-12)
    assert np.allclose(Rd.conj().T @ Rd, np.eye(16), atol=1e-12)
    k, m = np.meshgrid(np.arange(64), np.arange(64 * L), indexing='ij')
    assert np.allclose(Ld, np.exp(-2j * np.pi * k * m / (64 * L)) / np.sqrt(64 * L), atol=1e-12)
    m, k = np.meshgrid(np.arange(16 * L), np.arange(16), indexing='ij')
    assert np.allclose(Rd, np.exp(2j * np.pi * k * m / (16 * L)) / np.sqrt(16 * L), atol=1e-12)
    rng = np.random.default_rng(L)
    P, Y, _ = _problem(rng, B=1)
    x = rng.standard_normal((1, 64 * L, 16 * L)) + 1j * rng.standard_normal((1, 64 * L, 16 * L))
    lhs = np.vdot(Y, O.fw_op(P, Ld, Rd, x))
    rhs = np.vdot(O.fw_op_H(P, Ld, Rd, Y), x)
    assert abs(lhs - rhs) < 1e-9 * abs(lhs)


def test_one_step_from_zero_is_a_thresholded_adjoint():
    rng = np.random.default_rng(5)
    P, Y, H = _problem(rng)
    lam, lr = 0.3, 3e-3
    _, _, x = O.l1_run(P, Y, H, lam, lr, 4, 1)
    Ld, Rd = O.dictionaries(64, 16, 4)
    v = lr * (Ld.conj().T @ (np.conj(np.swapaxes(P, 1, 2)) @ Y) @ Rd.conj().T)
    assert np.allclose(x, O.soft_thresh(lam * lr, v), rtol=1e-12, atol=1e-15)
    assert np.count_nonzero(x) < x.size                          # the threshold bites


def test_momentum_sequence_and_soft_threshold_at_zero():
    t, c = O.t_sequence(5)
    assert t[0] == 1.0 and c[0] == 0.0
    assert np.allclose(t[1], (1 + np.sqrt(5)) / 2)
    assert np.allclose(c[1:], (t[1:] - 1) / np.append(t[2:], (1 + np.sqrt(1 + 4 * t[-1] ** 2)) / 2))
    assert np.all(np.diff(c) > 0) and np.all(c < 1)
    z = np.array([0j, 1e-3 + 0j, -2 + 2j])
    out = O.soft_thresh(0.5, z)
    assert out[0] == 0 and out[1] == 0
    assert np.allclose(out[2], (-2 + 2j) * (1 - 0.5 / np.abs(-2 + 2j)))


def test_l1_cli_arguments_and_result_path():
    a = l1cli.parse_args([])
    assert (a.train, a.test, a.antennas, a.array, a.spacing, a.alpha, a.lmbda, a.lifting, a.steps, a.lr) == \
        ('CDL-C', 'CDL-C', [16, 64], 'ULA', 0.5, [0.6], [0.3], 4, 1000, [3e-3])
    assert (a.gpu, a.seed, a.synthetic, a.kept_samples, a.no_plot) == (0, None, False, 50, False)
    assert l1cli.result_dir(a) == './results/l1CS_lifted4/train-CDL-C_test-CDL-C'
    b = l1cli.parse_args(['--lifting', '1', '--train', 'CDL-B', '--lmbda', '0.1', '0.3', '--lr', '1e-3', '3e-3', '--seed', '3'])
    assert l1cli.result_dir(b) == './results/l1CS_lifted1/train-CDL-B_test-CDL-C' and b.lmbda == [0.1, 0.3] and b.seed == 3


def test_ml_cli_arguments_and_result_path():
    a = mlcli.parse_args([])
    assert (a.model, a.channel, a.antennas, a.array, a.spacing, a.alpha) == ('CDL-D', 'CDL-D', [16, 64], 'ULA', [0.5], [0.6])
    assert (a.gpu, a.seed, a.synthetic, a.kept_samples, a.no_plot) == (0, None, False, 50, False)
    assert mlcli.result_path(a) == os.path.join('results_ml_baseline/model_CDL-D_channel_CDL-D', 'results_Nt64_Nr16.pt')


def test_best_selection_is_the_argmin_of_the_mean():
    rng = np.random.default_rng(2)
    nmse = rng.random((1, 1, 3, 2, 9, 5))
    bn, bl, br = l1cli.select_best(nmse, np.array([0.6]), np.arange(9), np.array([0.1, 0.2, 0.3]), np.array([1e-3, 3e-3]),
                                   verbose=False)
    avg = nmse.mean(-1)[0, 0]
    for s in range(9):
        i = np.argmin(avg[..., s].flatten())
        assert bn[0, s] == avg[..., s].flatten()[i]
        assert (bl[0, s], br[0, s]) == ([0.1, 0.2, 0.3][i // 2], [1e-3, 3e-3][i % 2])


def test_l1_lifted_refuses_bad_arguments_on_the_host():
    rng = np.random.default_rng(0)
    P, Y, H = (a.astype(np.complex64) for a in _problem(rng))
    with pytest.raises(ValueError, match='lifting'):
        baselines.l1_lifted(P, Y, H, 0.3, 3e-3, lifting=3)
    with pytest.raises(ValueError, match='Nt = 64'):
        baselines.l1_lifted(P[:, :, :32], Y, H[:, :32], 0.3, 3e-3)
    with pytest.raises(ValueError, match='Np'):
        baselines.l1_lifted(P, Y[:, :20], H, 0.3, 3e-3)
    with pytest.raises(ValueError, match='complex'):
        baselines.l1_lifted(P.real, Y, H, 0.3, 3e-3)
    with pytest.raises(ValueError, match='lr'):
        baselines.l1_lifted(P, Y, H, 0.3, 0.0)
    with pytest.raises(ValueError, match='lmbda'):
        baselines.l1_lifted(P, Y, H, [0.3, 0.1, 0.2], 3e-3)
    with pytest.raises(ValueError, match='p_index'):
        baselines.l1_lifted(P, Y, H, 0.3, 3e-3, p_index=[0, 2])
    with pytest.raises(ValueError, match='steps'):
        baselines.l1_lifted(P, Y, H, 0.3, 3e-3, steps=0)


def test_ls_regularized_refuses_bad_arguments_on_the_host():
    rng = np.random.default_rng(1)
    P, Y, H = (a.astype(np.complex64) for a in _problem(rng))
    with pytest.raises(ValueError, match='> 0'):
        baselines.ls_regularized(P, Y, 0.0, H)
    with pytest.raises(ValueError, match='> 0'):
        baselines.ls_regularized(P, Y, [0.1, -1.0], H)
    with pytest.raises(ValueError, match='Np'):
        baselines.ls_regularized(P, Y[:, :10], 0.1, H)
    with pytest.raises(ValueError, match='H must be'):
        baselines.ls_regularized(P, Y, 0.1, H[:, :, :8])
    with pytest.raises(ValueError, match='supports'):
        big = np.zeros((1, 100, 100), np.complex64)
        baselines.ls_regularized(big, np.zeros((1, 100, 16), np.complex64), 0.1)


# ---- the single-precision restatement of the ML solver and the assertion helpers of the GPU tests (tests/cs_checks.py)

@pytest.mark.parametrize('npil,nt,nr', K.LS_GRID)
def test_ls_c64_restatement_on_the_geometry_grid(npil, nt, nr):
    """lstsq_run_c64 factorises every problem of the grid (no NaN at kappa up to ~1e5), stays within the forward-error bound of a
    single-precision Cholesky solve -- gamma_{3n+1} kappa for the solve (Higham, Accuracy and Stability, thm 10.4) plus
    (Np + Nt) u for the products around it -- of lstsq_run, and passes the GPU test's own check when offered as the answer."""
    P, Y, H, pidx, hidx, noise = K.ls_problem(npil, nt, nr, 1000 + 7 * npil + nt + nr)
    Pb, Hb = P[pidx], H[hidx]
    cH, cn = O.lstsq_run_c64(Pb, Y, Hb, noise)
    assert cH.dtype == np.complex64 and np.all(np.isfinite(K.ri(cH))) and np.all(np.isfinite(cn))
    figures, failures = K.check_ls(cH, cn.astype(np.float32), Pb, Y, Hb, noise)
    print(figures)
    assert not failures, failures
    assert len(figures) == 4 and all(f['c_over_theory'] <= 1 for f in figures)


def test_ls_grid_holds_what_the_library_documents():
    assert len(K.LS_GRID) == 18 and len(set(K.LS_GRID)) == 18
    assert sum(npil > nt for npil, nt, _ in K.LS_GRID) >= 5
    assert all(min(npil, nt) <= baselines.LS_MAX_N and nr <= baselines.LS_MAX_NR and max(npil, nt) <= baselines.LS_MAX_DIM
               for npil, nt, nr in K.LS_GRID)
    assert {(63, 64, 17), (64, 64, 64), (65, 64, 16), (1024, 64, 16), (64, 1024, 16), (1, 1, 1), (2, 3, 1)} <= set(K.LS_GRID)
    n, nr = 64, 64
    assert (4 + n * (n + 1) + n * nr) * 8 > 64 * 1024           # the (64, 64, 64) case asks for more than 64 KiB of LDS


@pytest.mark.parametrize('npil,nt,nr', [(76, 64, 16), (100, 33, 5), (7, 5, 3)])
def test_check_ls_trips_on_a_wrong_normal_equations_branch(npil, nt, nr):
    """Mutation of the yardstick: the Np > Nt right-hand side un-conjugated (P^T Y for P^H Y), and the system solved with the
    regulariser's sign flipped -- each trips check_ls, the second one on the residual and the NMSE as well."""
    P, Y, H, pidx, hidx, noise = K.ls_problem(npil, nt, nr, 5)
    Pb, Hb = P[pidx], H[hidx]
    good, gn = O.lstsq_run_c64(Pb, Y, Hb, noise)
    assert not K.check_ls(good, gn.astype(np.float32), Pb, Y, Hb, noise)[1]
    eye = np.eye(nt, dtype=np.complex64)
    unconj = np.stack([np.linalg.solve(np.conj(Pb[b].T) @ Pb[b] + np.float32(noise[b]) * eye, Pb[b].T @ Y[b]) for b in range(16)])
    _, failures = K.check_ls(unconj.astype(np.complex64), None, Pb, Y, Hb, noise)
    assert any('H_hat error' in f for f in failures) and any('residual' in f for f in failures), failures
    minus = np.stack([np.linalg.solve(np.conj(Pb[b].T) @ Pb[b] - np.float32(noise[b]) * eye, np.conj(Pb[b].T) @ Y[b])
                      for b in range(16)]).astype(np.complex64)
    mn = np.sum(np.abs(minus - Hb) ** 2, axis=(1, 2)) / np.sum(np.abs(Hb) ** 2, axis=(1, 2))
    _, failures = K.check_ls(minus, mn.astype(np.float32), Pb, Y, Hb, noise)
    assert any('residual' in f for f in failures) and any('nmse' in f for f in failures), failures
    # a right answer with a wrong NMSE (that of another problem), and a NaN, trip too
    _, failures = K.check_ls(good, np.roll(gn, 1).astype(np.float32), Pb, Y, Hb, noise)
    assert any('nmse' in f for f in failures), failures
    bad = good.copy()
    bad[3, 0, 0] = np.nan
    assert 'non-finite H_hat or nmse' in K.check_ls(bad, None, Pb, Y, Hb, noise)[1]


def _l1_data(B, npil, seed):
    rng = np.random.default_rng(seed)
    P, Y, H = (a.astype(np.complex64) for a in _problem(rng, B=B, np_=npil))
    return P, Y, H


@pytest.mark.parametrize('L', [1, 2, 4])
def test_half_sparse_lambda_on_the_gpu_tests_data(L):
    """On the very problems of the GPU test (cdl_data(4, 38, 31, 10 dB)): the threshold bites -- half of the first iterate is zero
    and more later --, the complex64 oracle has the float64 oracle's support outside the excused window (1e-5 max|v| around the
    threshold) and meets the value bounds, and the window holds at most 0.1 % of X per problem."""
    P, Y, H = K.cdl_data(4, 38, 31, 10.0)
    lam = K.half_sparse_lambda(P, Y, L)
    for steps in (1, 2, 3, 10):
        rlog, rH, rX, rv = O.l1_run(P, Y, H, lam, 3e-3, L, steps, return_v=True)
        clog, cH, cX = O.l1_run(P, Y, H, lam, 3e-3, L, steps, dtype=np.complex64)
        figures, failures = K.check_l1_iterate(clog, cH, cX, rlog, rH, rX, rv, lam * 3e-3)
        print(L, steps, figures)
        assert not failures, failures
        assert 0.45 <= figures['zero_share'][0] and figures['zero_share'][1] <= 0.85
        if steps == 1:
            assert figures['zero_share'] == (0.5, 0.5)
        assert np.array_equal(rX, O.soft_thresh((lam * 3e-3)[:, None, None], rv))


def test_check_l1_iterate_trips_on_a_threshold_of_lambda_instead_of_lambda_lr():
    """Mutation of the yardstick: tau = lambda (an oracle run at lambda / lr) offered as the answer."""
    P, Y, H = _l1_data(2, 38, 4)
    lam, lr = K.half_sparse_lambda(P, Y, 2), 3e-3
    rlog, rH, rX, rv = O.l1_run(P, Y, H, lam, lr, 2, 2, return_v=True)
    wlog, wH, wX = O.l1_run(P, Y, H, lam / lr, lr, 2, 2, dtype=np.complex64)
    _, failures = K.check_l1_iterate(wlog, wH, wX, rlog, rH, rX, rv, lam * lr)
    assert any('differ in support' in f for f in failures) and any(f.startswith('log') for f in failures), failures
    # one entry away from the threshold switched off: the support check alone trips
    clog, cH, cX = O.l1_run(P, Y, H, lam, lr, 2, 2, dtype=np.complex64)
    i = np.unravel_index(np.argsort(np.abs(rX[0]).ravel())[-rX[0].size // 4], rX[0].shape)
    cX[0][i] = 0
    _, failures = K.check_l1_iterate(clog, cH, cX, rlog, rH, rX, rv, lam * lr)
    assert any('differ in support' in f for f in failures), failures


def test_check_l1_consistency_trips_on_a_wrong_dictionary(monkeypatch):
    """Mutation of the yardstick: at L = 2 the forward product formed with the right dictionary of L = 4 truncated to its first
    32 rows; and a log that belongs to the previous iterate."""
    P, Y, H = _l1_data(2, 38, 6)
    log, Hh, X = O.l1_run(P, Y, H, 0.3, 3e-3, 2, 5, dtype=np.complex64)
    figures, failures = K.check_l1_consistency(log[-1].astype(np.float32), Hh, X, H, 2)
    assert not failures, (figures, failures)
    Ld, _ = O.dictionaries(64, 16, 2)
    _, Rd4 = O.dictionaries(64, 16, 4)
    wrong = O.array_op(Ld, Rd4[:32], X.astype(np.complex128)).astype(np.complex64)
    wl = np.sum(np.abs(wrong - H) ** 2, axis=(1, 2)) / np.sum(np.abs(H) ** 2, axis=(1, 2))
    _, failures = K.check_l1_consistency(wl.astype(np.float32), wrong, X, H, 2)
    assert failures == [f for f in failures if 'not Ld X Rd' in f] and failures
    _, failures = K.check_l1_consistency(log[-2].astype(np.float32), Hh, X, H, 2)
    assert failures and all('log[-1]' in f for f in failures), failures
    # the same mutation through the oracle: a run with the truncated dictionary is caught by the step comparison
    monkeypatch.setattr(O, 'dictionaries', lambda nt, nr, L: (Ld, Rd4[:32]))
    wlog, wH, wX = O.l1_run(P, Y, H, 0.3, 3e-3, 2, 3, dtype=np.complex64)
    monkeypatch.undo()
    rlog, rH, rX = O.l1_run(P, Y, H, 0.3, 3e-3, 2, 3)
    assert K.check_l1_iterate(wlog, wH, wX, rlog, rH, rX)[1]
