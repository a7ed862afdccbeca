"""Assertion helpers of the baseline-solver tests (tests/test_gpu_cs_baselines.py) and the problems they run on, kept apart from the
GPU tests so that tests/test_cs_baselines_cpu.py can feed them deliberately wrong answers and see them trip.  numpy only.

Every helper returns ``(figures, failures)``: the measured numbers (printed by the caller before it asserts) and a list of
messages, empty when every bound holds."""
import numpy as np

import cs_oracle as O
from conftest import rel_err_elementwise

EPS = 2.0 ** -24                                  # unit roundoff of float32

# (Np, Nt, Nr) of the ML solver: both solution forms with the boundary on either side (Np = Nt - 1, Nt, Nt + 1), systems of size
# 1 and 2, odd and prime extents, Nr on both sides of 16 (one right-hand-side column per thread) and at 64, both 1024 limits, and
# the LDS request above 64 KiB (n = 64, Nr = 64)
LS_GRID = [(1, 1, 1), (1, 64, 16), (2, 3, 1), (7, 5, 3), (12, 64, 16), (25, 64, 16), (51, 64, 16), (63, 64, 17), (64, 64, 64),
           (65, 64, 16), (76, 64, 16), (100, 33, 5), (200, 64, 64), (1024, 64, 16), (1024, 1, 1), (64, 1024, 16), (38, 256, 64),
           (64, 65, 2)]
LS_NOISES = (1e-3, 10 ** -1.5, 1.0, 1e3)


def ri(a):
    """complex -> interleaved (re, im) components, for the element-wise comparison of conftest.rel_err_elementwise"""
    return np.ascontiguousarray(a).astype(np.complex128).view(np.float64)


def _cn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def cdl_data(B, npil, seed, snr_db, channels=None):
    """B synthetic CDL-C channels [B, 64, 16], QPSK pilots [B, Np, 64], measurements at snr_db ([B] or scalar) -- complex64."""
    from score_based_channels_amd import synth
    raw = synth.generate_channels('CDL-C', B, 64, 16, 0.5, seed) if channels is None else channels
    H = np.conj(np.transpose(raw / np.std(raw), (0, 2, 1))).astype(np.complex64)
    rng = np.random.default_rng(seed)
    P = np.conj(np.transpose(synth.qpsk_pilots(rng, B, 64, npil), (0, 2, 1))).astype(np.complex64)
    noise = 10 ** (-np.broadcast_to(np.asarray(snr_db, np.float64), (B,)) / 10.) * 16
    z = (rng.standard_normal((B, npil, 16)) + 1j * rng.standard_normal((B, npil, 16))) / np.sqrt(2)
    Y = (P @ H + np.sqrt(noise)[:, None, None] * z).astype(np.complex64)
    return P, Y, H


def ls_problem(npil, nt, nr, seed, B=16, nP=4, nH=4, noises=LS_NOISES):
    """B problems on nP QPSK pilot matrices and nH Gaussian channels: problem b uses pilots b % nP, noise variance
    noises[(b // nP) % len(noises)] and channel (b + b // nP) % nH, so every (pilot matrix, noise variance) pair occurs.
    Returns complex64 P [nP, Np, Nt], Y [B, Np, Nr], H [nH, Nt, Nr], int p_index / h_index [B], float64 noise [B]."""
    rng = np.random.default_rng(seed)
    P = (((2 * rng.integers(0, 2, (nP, npil, nt)) - 1) + 1j * (2 * rng.integers(0, 2, (nP, npil, nt)) - 1)) / np.sqrt(2))
    P = P.astype(np.complex64)
    H = _cn(rng, (nH, nt, nr)).astype(np.complex64)
    b = np.arange(B)
    pidx, hidx = b % nP, (b + b // nP) % nH
    noise = np.asarray(noises, np.float64)[(b // nP) % len(noises)]
    Y = (P[pidx] @ H[hidx] + np.sqrt(noise)[:, None, None] * _cn(rng, (B, npil, nr))).astype(np.complex64)
    return P, Y, H, pidx, hidx, noise


def ls_condition(P, noise):
    """kappa = (s_max^2 + s2) / (s_min^2 + s2) of the regularised system of size min(Np, Nt), per problem"""
    out = []
    for b in range(P.shape[0]):
        s = np.linalg.svd(P[b].astype(np.complex128), compute_uv=False)
        out.append((s[0] ** 2 + noise[b]) / (s[-1] ** 2 + noise[b]))
    return np.asarray(out)


def ls_residual(P, Y, noise, est):
    """|| (P^H P + s2 I) est - P^H Y || / || P^H Y || in float64, per problem: needs no solve"""
    out = np.empty(P.shape[0])
    for b in range(P.shape[0]):
        Pb, Ph = P[b].astype(np.complex128), np.conj(P[b].astype(np.complex128).T)
        rhs = Ph @ Y[b].astype(np.complex128)
        eb = est[b].astype(np.complex128)
        out[b] = np.linalg.norm(Ph @ (Pb @ eb) + noise[b] * eb - rhs) / np.linalg.norm(rhs)
    return out


def _fro_err(a, ref):
    B = ref.shape[0]
    return np.linalg.norm((a - ref).reshape(B, -1), axis=1) / np.linalg.norm(ref.reshape(B, -1), axis=1)


def check_ls(est, nmse, P, Y, H, noise, factor=4.0, yardstick=O.lstsq_run_c64):
    """A candidate answer (``est`` [B, Nt, Nr], ``nmse`` [B] or None) of the ML solver on per-problem ``P`` [B, Np, Nt], ``Y``,
    ``H`` (or None), ``noise`` [B], against ``lstsq_run`` in float64.  Problems are grouped by noise variance (one geometry per
    call); within a group, with e_c / r_c the forward error / residual of the single-precision restatement:

    * every value finite;
    * forward error <= max(factor max e_c, 8 EPS)  -- the floor where the restatement is at rounding level;
    * residual <= max(factor max r_c, 8 EPS)       -- the same floor: est is stored in float32, so no answer has less than a
      few EPS of residual, and at n = 1 the restatement's own can happen to vanish;
    * |nmse / nmse64 - 1| <= forward bound * 2 ||H_ref|| / ||H_ref - H|| + 2 EPS  (first-order propagation; float32 store)."""
    P64, Y64 = P.astype(np.complex128), Y.astype(np.complex128)
    B = P.shape[0]
    H64 = H.astype(np.complex128) if H is not None else np.zeros((B,) + est.shape[1:], np.complex128)
    rH, rn = O.lstsq_run(P64, Y64, H64, noise)
    cH, _ = yardstick(P, Y, H, noise)
    e_k, e_c = _fro_err(est.astype(np.complex128), rH), _fro_err(cH.astype(np.complex128), rH)
    r_k, r_c = ls_residual(P, Y, noise, est), ls_residual(P, Y, noise, cH)
    kappa = ls_condition(P, noise)
    figures, failures = [], []
    if not np.all(np.isfinite(ri(est))) or (nmse is not None and not np.all(np.isfinite(nmse))):
        failures.append('non-finite H_hat or nmse')
    if not np.all(np.isfinite(ri(cH))):
        failures.append('the single-precision restatement does not factorise every problem')
    for s in np.unique(noise):
        g = np.flatnonzero(noise == s)
        bound_e, bound_r = max(factor * np.max(e_c[g]), 8 * EPS), max(factor * np.max(r_c[g]), 8 * EPS)
        row = dict(noise=float(s), kappa=float(np.max(kappa[g])), e_c=float(np.max(e_c[g])), e_k=float(np.max(e_k[g])),
                   r_c=float(np.max(r_c[g])), r_k=float(np.max(r_k[g])))
        # the restatement against the textbook forward bound of a Cholesky solve, gamma_{3n+1} kappa (Higham, Accuracy and Stability
        # of Numerical Algorithms, thm 10.4), plus (Np + Nt) u for the products around it: <= 1 for a sound yardstick
        n = min(P.shape[1], P.shape[2])
        row['c_over_theory'] = float(np.max(e_c[g] / (((3 * n + 1) * kappa[g] + P.shape[1] + P.shape[2]) * EPS)))
        row['e_ratio'], row['r_ratio'] = row['e_k'] / row['e_c'], row['r_k'] / max(row['r_c'], 1e-300)
        if not np.max(e_k[g]) <= bound_e:
            failures.append('s2=%g: H_hat error %.3g > %.3g (restatement %.3g)' % (s, np.max(e_k[g]), bound_e, np.max(e_c[g])))
        if not np.max(r_k[g]) <= bound_r:
            failures.append('s2=%g: residual %.3g > %.3g (restatement %.3g)' % (s, np.max(r_k[g]), bound_r, np.max(r_c[g])))
        if nmse is not None:
            amp = 2 * np.linalg.norm(rH[g].reshape(len(g), -1), axis=1) / np.linalg.norm((rH[g] - H64[g]).reshape(len(g), -1), axis=1)
            dn = np.abs(np.asarray(nmse, np.float64)[g] / rn[g] - 1)
            row['nmse_err'], row['nmse_bound'] = float(np.max(dn)), float(np.min(bound_e * amp + 2 * EPS))
            bad = np.flatnonzero(~(dn <= bound_e * amp + 2 * EPS))
            if len(bad):
                failures.append('s2=%g: nmse off by %.3g > %.3g (problem %d)' % (s, dn[bad[0]], (bound_e * amp + 2 * EPS)[bad[0]], g[bad[0]]))
        figures.append(row)
    return figures, failures


def half_sparse_lambda(P, Y, L):
    """Per problem, the lambda that zeroes about half of the first iterate: the first step thresholds lr |g0| at lambda lr with
    g0 = fw_op_H(P, Ld, Rd, -Y), so lambda is the midpoint between the two middle order statistics of |g0| (no entry sits on the
    threshold by construction), rounded to the float32 the solver takes."""
    Ld, Rd = O.dictionaries(P.shape[2], Y.shape[2], L)
    g0 = np.abs(O.fw_op_H(P.astype(np.complex128), Ld, Rd, -Y.astype(np.complex128))).reshape(P.shape[0], -1)
    a = np.sort(g0, axis=1)
    n = a.shape[1]
    return ((a[:, n // 2 - 1] + a[:, n // 2]) / 2).astype(np.float32).astype(np.float64)


def check_l1_iterate(log, Hh, X, rlog, rH, rX, rv=None, tau=None, window=1e-5, cap=1e-3):
    """A candidate (log [steps, B], H_hat, X) of the l1 solver against the float64 oracle's: X and H_hat within 1e-5 element-wise
    above the 5 % floor, the log within 5e-6.  With ``rv`` (the oracle's last pre-threshold v) and ``tau`` [B] also the support:
    per problem, entries with ||rv| - tau| <= window max|rv| may differ (at most ``cap`` of X); everywhere else the zero pattern
    of X equals the oracle's exactly."""
    figures = dict(X=rel_err_elementwise(ri(X), ri(rX)) if np.any(rX) else float(np.max(np.abs(X))),
                   H=rel_err_elementwise(ri(Hh), ri(rH)) if np.any(rH) else float(np.max(np.abs(Hh))),
                   log=float(np.max(np.abs(log / rlog - 1))))
    failures = ['%s off by %.3g' % (k, v) for k, v, bnd in (('X', figures['X'], 1e-5), ('H_hat', figures['H'], 1e-5),
                                                            ('log', figures['log'], 5e-6)) if not v < bnd]
    if rv is not None:
        shares, zeros, mism = [], [], 0
        for b in range(X.shape[0]):
            a = np.abs(rv[b])
            near = np.abs(a - tau[b]) <= window * np.max(a)
            shares.append(float(np.mean(near)))
            zeros.append(float(np.mean(rX[b] == 0)))
            mism += int(np.sum(((X[b] == 0) != (rX[b] == 0)) & ~near))
        figures.update(near_share=max(shares), zero_share=(min(zeros), max(zeros)), support_mismatches=mism)
        if max(shares) > cap:
            failures.append('%.3g of X within the threshold window (cap %.3g)' % (max(shares), cap))
        if mism:
            failures.append('%d entries away from the threshold differ in support' % mism)
    return figures, failures


def check_l1_consistency(log_last, Hh, X, H, L):
    """The returned H_hat, X and log[-1] belong to one iterate: array_op(Ld, Rd, X) in float64 equals H_hat to 1e-5 element-wise
    (5 % floor), and ||H_hat - H||^2 / ||H||^2 in float64 equals log[-1] to 1e-6 relative.  The second bound is derived: the kernel
    forms the log from the very fp32 H_hat it returns, in a float64 sum of squares of fp32 differences, and stores it as float32,
    so the two differ by a few EPS (the fp32 subtraction is exact to EPS of the larger operand; 1e-6 is about 16 EPS)."""
    Ld, Rd = O.dictionaries(Hh.shape[1], Hh.shape[2], L)
    fwd = O.array_op(Ld, Rd, X.astype(np.complex128))
    H64, Hh64 = H.astype(np.complex128), Hh.astype(np.complex128)
    nm = np.sum(np.abs(Hh64 - H64) ** 2, axis=(1, 2)) / np.sum(np.abs(H64) ** 2, axis=(1, 2))
    figures = dict(forward=rel_err_elementwise(ri(Hh), ri(fwd)), log=float(np.max(np.abs(np.asarray(log_last, np.float64) / nm - 1))))
    failures = []
    if not figures['forward'] <= 1e-5:
        failures.append('H_hat is not Ld X Rd: %.3g' % figures['forward'])
    if not figures['log'] <= 1e-6:
        failures.append('log[-1] is not the NMSE of H_hat: %.3g' % figures['log'])
    return figures, failures
