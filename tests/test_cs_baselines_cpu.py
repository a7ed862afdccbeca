"""CPU checks of the classical baselines (Lasso / fsAD, ML): the numpy oracle's algebra (tests/cs_oracle.py), the CLIs' arguments
and result paths, and the host-side refusals of score_based_channels_amd/baselines.py (no GPU needed: they raise before any
launch)."""
import os

import numpy as np
import pytest

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
