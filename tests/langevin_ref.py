"""Float64 reference of the step around the score network -- SBC_OP_MEASURE and SBC_OP_LANGEVIN (csrc/ops.hip) -- with the
table of geometries the tests walk and a restatement of the dispatcher's choice of kernel for each.  Test infrastructure:
plain numpy, nothing of the library is imported.

The arithmetic follows the reference's ``test_score.py:122-124`` (measurements) and ``:156-170`` (update and NMSE) as
oracle/ald_oracle.py cites them; the oracle restates them in complex64 (what the goldens pin), this file in complex128 with
the float32 scalars exactly as the kernels read them, so that a kernel is held to the operation and not to another float32
summation order.
"""
import collections

import numpy as np

C128 = np.complex128


def _col(v, n):
    """A per-trajectory float32 scalar (or ``[B]`` of them) as float64 ``[B, 1, 1]``."""
    return np.broadcast_to(np.asarray(v, np.float32).astype(np.float64).reshape(-1), (n,)).reshape(n, 1, 1)


def measure64(P, H, scale, noise):
    """``Y = P H + scale * n`` (test_score.py:122-124).  P ``[B, Np, Nt]``, H ``[B, Nt, Nr]``, noise ``[B, Np, Nr]``, ``scale``
    the float32 ``sqrt(local_noise)`` per trajectory (SBC_OP_MEASURE's ``meas_scale``).  complex128 ``[B, Np, Nr]``."""
    P, H, noise = np.asarray(P, C128), np.asarray(H, C128), np.asarray(noise, C128)
    return np.matmul(P, H) + _col(scale, P.shape[0]) * noise


def nmse64(X, H):
    """``sum |X - H|^2 / sum |H|^2`` per trajectory (test_score.py:168-170), float64."""
    X, H = np.asarray(X, C128), np.asarray(H, C128)
    return np.sum(np.abs(X - H) ** 2, axis=(-1, -2)) / np.sum(np.abs(H) ** 2, axis=(-1, -2))


def langevin64(X, S, P, Y, alpha, dc_div, nscale, dc_boost, noise, Htrue=None):
    """One update of test_score.py:156-165, ``X + alpha (S - dc_boost P^H (P X - Y) / dc_div) + nscale n``, and the NMSE
    against ``Htrue`` (:168-170).  All tensors ``[B, ...]``; the four scalars are float32 (or ``[B]`` of them) as the sched
    row holds them, a ``dc_boost`` of 0 reading as 1 like in the kernels.  Returns (X complex128, nmse float64 or None)."""
    X, S, P, Y, noise = (np.asarray(a, C128) for a in (X, S, P, Y, noise))
    B = X.shape[0]
    dcb = np.asarray(dc_boost, np.float32)
    dcb = np.where(dcb != 0, dcb, np.float32(1))
    grad = np.matmul(np.conj(np.transpose(P, (0, 2, 1))), np.matmul(P, X) - Y)
    Xn = X + _col(alpha, B) * (S - _col(dcb, B) * grad / _col(dc_div, B)) + _col(nscale, B) * noise
    return Xn, (None if Htrue is None else nmse64(Xn, Htrue))


def philox_noise(seed, traj_ids, step, shape):
    """The draws the kernels make themselves when ``noise`` is NULL, from the host restatement of the stream
    (oracle/ald_oracle.py::device_complex_normal): ``[len(traj_ids)] + shape`` complex64; ``step = -1`` for SBC_OP_MEASURE."""
    from oracle import ald_oracle as A
    n = int(np.prod(shape))
    return np.stack([A.device_complex_normal(seed, int(t), step, n).reshape(shape) for t in traj_ids])


# ---------------------------------------------------------------------------------------------------------- dispatch
# RESTATEMENT of the predicate in csrc/ops.hip::launch_langevin (and of the constants J = 32, KC = 16, 512 threads of
# langevin_tiled_kernel).  It MUST BE KEPT IN STEP with the dispatcher: its one use is to prove that CASES below reaches every
# code path the dispatcher can pick -- nothing in the product reads it.
TILED_J, TILED_KC, TILED_THREADS = 32, 16, 512
Path = collections.namedtuple('Path', 'kernel cols G nt_mod16 np_mod16 q0_passes m0_passes nt_lt_gj nt_lt_kc')
FLAT_XP_LDS, FLAT_X_LDS, FLAT_X_GLOBAL, TILED = 'flat, X and P in LDS', 'flat, X in LDS, P global', 'flat, X global', 'tiled'


def dispatch_path(nt, nr, np_):
    """Which kernel ``launch_langevin`` runs for (Nt, Nr, Np) and the tail properties of that shape.  ``cols``: receive
    antennas per thread in the flat kernel's first product (4 when ``Nr % 4 == 0``, else 1; 0 for the tiled kernel)."""
    lds_all = (nt + np_) * nr * 8
    x_in_lds = lds_all <= 64 * 1024
    lds_p = np_ * (nt + 2) * 8
    p_in_lds = x_in_lds and nt % 2 == 0 and lds_all + lds_p <= 40 * 1024
    if not x_in_lds and TILED_THREADS % nr == 0:
        G = TILED_THREADS // nr
        lds_t = (np_ * nr + G * TILED_J * TILED_KC + TILED_KC * nr) * 8
        if lds_t <= 156 * 1024:
            gj = G * TILED_J
            return Path(TILED, 0, G, nt % 16, np_ % 16, -(-nt // gj), -(-np_ // gj), nt < gj, nt < TILED_KC)
    kernel = FLAT_XP_LDS if p_in_lds else FLAT_X_LDS if x_in_lds else FLAT_X_GLOBAL
    return Path(kernel, 4 if nr % 4 == 0 else 1, 0, nt % 16, np_ % 16, 1, 1, False, nt < TILED_KC)


def path_label(p):
    return p.kernel if p.kernel == TILED else '%s, %d col' % (p.kernel, p.cols)


def accepted(nt, nr, np_):
    """What check_langevin lets through of a shape: Nr even and R = [Np][Nr] within 150 KB of LDS."""
    return nr % 2 == 0 and np_ * nr * 8 <= 150 * 1024


# (Nt, Nr, Np) -> the path each was chosen for (test_langevin_cases_cpu.py holds dispatch_path to this column)
CASES = [
    ((64, 16, 38), (FLAT_XP_LDS, 4)), ((16, 64, 10), (FLAT_XP_LDS, 4)), ((32, 32, 19), (FLAT_XP_LDS, 4)), ((24, 24, 14), (FLAT_XP_LDS, 4)),
    ((64, 18, 38), (FLAT_XP_LDS, 1)), ((64, 2, 38), (FLAT_XP_LDS, 1)),
    ((64, 16, 64), (FLAT_X_LDS, 4)), ((128, 8, 77), (FLAT_X_LDS, 4)), ((128, 32, 77), (FLAT_X_LDS, 4)),
    ((7, 2, 3), (FLAT_X_LDS, 1)), ((33, 6, 20), (FLAT_X_LDS, 1)), ((9, 10, 5), (FLAT_X_LDS, 1)), ((1024, 6, 300), (FLAT_X_LDS, 1)),
    ((400, 24, 90), (FLAT_X_GLOBAL, 4)), ((2000, 4, 100), (FLAT_X_GLOBAL, 4)), ((40, 256, 70), (FLAT_X_GLOBAL, 4)),
    ((1200, 6, 400), (FLAT_X_GLOBAL, 1)),
    ((256, 64, 154), (TILED, 0)), ((256, 64, 26), (TILED, 0)), ((500, 64, 37), (TILED, 0)), ((300, 128, 100), (TILED, 0)),
    ((600, 16, 100), (TILED, 0)), ((264, 32, 300), (TILED, 0)), ((8, 512, 20), (TILED, 0)),
    ((256, 64, 128), (TILED, 0)),                              # no tail in either product: Nt % 16 == Np % 16 == 0
]
SHAPES = [c[0] for c in CASES]
MEASURE_ONLY_SHAPES = [(33, 5, 20), (7, 1, 3)]                 # odd Nr: SBC_OP_MEASURE takes it, SBC_OP_LANGEVIN refuses it

# the batch every case runs as: 5 trajectories over 3 pilot matrices and 4 channels (repeats, not in order), two sched groups
B, N_P, N_H, N_STEPS = 5, 3, 4, 3
P_INDEX = np.array([2, 0, 2, 1, 0], np.int32)
H_INDEX = np.array([3, 1, 0, 1, 2], np.int32)
GROUP = np.array([0, 1, 1, 0, 1], np.int32)


def make_sched(n_steps=N_STEPS):
    """``[2][n_steps][4]`` float32 (alpha, dc_div, noise_scale, dc_boost): group 0 starts at (0.3, 7.0, 0.05, 2.5), group 1 has
    dc_boost = 0 ("not set", read as 1); every row differs from every other, so a row read at the wrong step is a wrong number."""
    s = np.zeros((2, n_steps, 4), np.float32)
    for k in range(n_steps):
        s[0, k] = (0.3 / (1 + k), 7.0 + k, 0.05 * (1 + k), 2.5)
        s[1, k] = (0.2 / (1 + k), 5.0 + 2 * k, 0.04 * (1 + k), 0.0)
    return s


def cnormal(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def make_inputs(shape, seed=None, b=B, n_p=N_P, n_h=N_H, n_steps=N_STEPS):
    """Seeded complex64 inputs of one case: X, S (score), Y ``[b, ...]``, P ``[n_p, Np, Nt] / sqrt(Nt)``, H ``[n_h, Nt, Nr]``,
    step noise ``[n_steps, b, Nt, Nr]``, measurement noise ``[b, Np, Nr]`` and ``meas_scale [b]``.  Standard normals keep the NMSE
    (|X' - H|^2 / |H|^2 of unrelated X' and H) at order 1, so its ratio to the reference is well conditioned."""
    nt, nr, np_ = shape
    rng = np.random.default_rng(1000003 * nt + 1009 * nr + np_ if seed is None else seed)
    return dict(X=cnormal(rng, b, nt, nr), S=cnormal(rng, b, nt, nr), H=cnormal(rng, n_h, nt, nr), Y=cnormal(rng, b, np_, nr),
                P=(cnormal(rng, n_p, np_, nt) / np.float32(np.sqrt(nt))).astype(np.complex64),
                noise=cnormal(rng, n_steps, b, nt, nr), mnoise=cnormal(rng, b, np_, nr),
                meas_scale=(0.25 + 0.5 * rng.random(b)).astype(np.float32))


def rel_err64(a, b):
    """Norm-wise (max-norm) relative error of ``a`` against the reference ``b``, per leading index."""
    a, b = np.asarray(a, C128), np.asarray(b, C128)
    ax = tuple(range(1, a.ndim))
    return np.max(np.abs(a - b), axis=ax) / np.max(np.abs(b), axis=ax)
