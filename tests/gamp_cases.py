"""Inputs of the EM-GM-AMP tests (tests/test_gamp_cpu.py, tests/test_gpu_gamp.py): channels of the project's synthetic CDL-C
generator in the script's layout (conjugate transpose, unit mean power, test_em_gm_amp.m:18-34), QPSK pilots and one noisy
measurement per problem (:104-113), all from ``default_rng`` seeds."""
import numpy as np

NT, NR = 64, 16
THETA32 = float(np.float32(0.3))          # the damping as the descriptor carries it (float theta)
STOP_CASES = ((38, 1e-1), (38, 3e-2), (64, 3e-2), (12, 1e-1))     # (Np, tol) of the early-stop tests


def channels(num, seed=7):
    """[num, Nt, Nr] complex64, mean |h|^2 = 1"""
    from score_based_channels_amd.synth import generate_channels
    h = generate_channels('CDL-C', num, NT, NR, 0.5, seed)                    # [num, Nr, Nt]
    h = np.conj(np.swapaxes(h, -1, -2)).astype(np.complex128)
    return (h / np.sqrt(np.mean(np.abs(h) ** 2))).astype(np.complex64)


def pilots(num, n_pilots, seed=11):
    """[num, Np, Nt] complex64 QPSK"""
    rng = np.random.default_rng([seed, n_pilots])
    re = 2 * rng.integers(0, 2, size=(num, n_pilots, NT)) - 1
    im = 2 * rng.integers(0, 2, size=(num, n_pilots, NT)) - 1
    return ((re + 1j * im) / np.sqrt(2)).astype(np.complex64)


def measure(P, H, snr_db, p_index, h_index, seed=13):
    """Y[b] = P[p_index[b]] H[h_index[b]] + CN(0, 10^(-snr/10)), complex64 [B, Np, Nr]; ``snr_db`` a scalar or [B]"""
    rng = np.random.default_rng([seed, P.shape[1]])
    p_index, h_index = np.asarray(p_index), np.asarray(h_index)
    clean = np.matmul(P[p_index].astype(np.complex128), H[h_index].astype(np.complex128))
    nv = 10.0 ** (-np.broadcast_to(np.asarray(snr_db, np.float64), (len(p_index),)) / 10.0)
    noise = rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape)
    return (clean + np.sqrt(nv / 2)[:, None, None] * noise).astype(np.complex64)


def problem(n_pilots, snrs, per_snr, n_matrices=2, seed=0):
    """The grid cell of the GPU tests: ``per_snr`` problems at each SNR of ``snrs``, pilot matrices shared through ``p_index``,
    one channel per problem.  Returns (P, Y, H, p_index, h_index, snr_of_problem)."""
    B = len(snrs) * per_snr
    H = channels(B, seed=7 + seed)
    P = pilots(n_matrices, n_pilots, seed=11 + seed)
    p_index = (np.arange(B) % n_matrices).astype(np.int32)
    h_index = np.arange(B, dtype=np.int32)
    snr = np.repeat(np.asarray(snrs, np.float64), per_snr)
    return P, measure(P, H, snr, p_index, h_index, seed=13 + seed), H, p_index, h_index, snr
