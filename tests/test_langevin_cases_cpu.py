"""The case table and float64 reference that tests/test_gpu_langevin.py holds SBC_OP_LANGEVIN / SBC_OP_MEASURE to
(tests/langevin_ref.py), checked without a GPU: the table reaches every path of the dispatcher, and the reference agrees with
the complex64 restatement the goldens pin to the original code (oracle/ald_oracle.py)."""
import numpy as np
import pytest

import langevin_ref as R
from oracle import ald_oracle as A


def test_cases_reach_every_dispatch_path_and_tail():
    paths = {s: R.dispatch_path(*s) for s in R.SHAPES}
    for shape, (kernel, cols) in R.CASES:
        assert R.accepted(*shape), shape
        assert (paths[shape].kernel, paths[shape].cols) == (kernel, cols), (shape, paths[shape])
    # every flat variant: where X and P live x columns per thread of the first product
    flat = {(p.kernel, p.cols) for p in paths.values() if p.kernel != R.TILED}
    assert flat == {(k, c) for k in (R.FLAT_XP_LDS, R.FLAT_X_LDS, R.FLAT_X_GLOBAL) for c in (4, 1)}
    # P global because Nt is odd, and because P does not fit beside X
    assert any(p.kernel == R.FLAT_X_LDS and s[0] % 2 for s, p in paths.items())
    assert any(p.kernel == R.FLAT_X_LDS and s[0] % 2 == 0 for s, p in paths.items())
    # X global because Nr does not divide 512, and because the tiled kernel's LDS need is over its limit
    assert any(p.kernel == R.FLAT_X_GLOBAL and 512 % s[1] for s, p in paths.items())
    assert any(p.kernel == R.FLAT_X_GLOBAL and 512 % s[1] == 0 for s, p in paths.items())
    tiled = [p for p in paths.values() if p.kernel == R.TILED]
    assert any(p.nt_mod16 == 0 and p.q0_passes == 1 and not p.nt_lt_gj for p in tiled)      # no Nt tail at all
    assert any(p.nt_mod16 for p in tiled) and any(p.np_mod16 for p in tiled) and any(p.np_mod16 == 0 for p in tiled)
    assert any(p.q0_passes == 2 for p in tiled) and any(p.q0_passes >= 3 for p in tiled)
    assert any(p.nt_lt_gj and not p.nt_lt_kc for p in tiled) and any(p.nt_lt_kc for p in tiled)
    assert {p.G for p in tiled} >= {1, 4, 8, 16, 32}
    assert paths[(500, 64, 37)][3:6] == (4, 5, 2) and paths[(300, 128, 100)].q0_passes == 3


def test_tiled_kernel_never_takes_a_second_m0_pass():
    """over every Nr that divides 512, no Np passes both LDS limits (R within 150 KB, the tiled kernel's need within
    156 KB) and exceeds G * J -- the ``m0`` loop of langevin_tiled_kernel runs once, which is why CASES has no shape for it."""
    reached = []
    for nr in (2, 4, 8, 16, 32, 64, 128, 256, 512):
        gj = 512 // nr * R.TILED_J
        fits = [n for n in range(1, 150 * 1024 // (nr * 8) + 2) if R.accepted(4096, nr, n) and R.dispatch_path(4096, nr, n).kernel == R.TILED]
        if fits:                                               # (Nr <= 8: the P slab [G*J][KC] alone is over the limit)
            reached.append(nr)
            assert max(fits) <= gj, (nr, max(fits), gj)
            assert R.dispatch_path(4096, nr, max(fits)).m0_passes == 1
    assert reached == [16, 32, 64, 128, 256, 512]


@pytest.mark.parametrize('shape', R.SHAPES + R.MEASURE_ONLY_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_reference_agrees_with_the_complex64_oracle(shape):
    """langevin64 / measure64 against oracle.ald_oracle.langevin_step / nmse / make_measurements on the cases' own inputs:
    norm-wise within 1e-6 and 1e-6 relative on the NMSE (measured: at most 2.0e-7 each)."""
    d = R.make_inputs(shape)
    sched = R.make_sched()
    P, H = d['P'][R.P_INDEX], d['H'][R.H_INDEX]
    ln = d['meas_scale'].astype(np.float64) ** 2
    Y64 = R.measure64(P, H, d['meas_scale'], d['mnoise'])
    for b in range(R.B):
        # (the oracle takes local_noise and rounds its root to float32: hand it the float64 root's square)
        Yo = A.make_measurements(P[b:b + 1], H[b:b + 1], ln[b], d['mnoise'][b:b + 1])
        assert abs(np.float32(np.sqrt(ln[b])) - d['meas_scale'][b]) <= np.spacing(d['meas_scale'][b])
        assert R.rel_err64(Yo, Y64[b:b + 1])[0] < 1e-6
    for k in (0, 1):
        a, dv, ns, dcb = (sched[R.GROUP, k, i] for i in range(4))
        X64, nm64 = R.langevin64(d['X'], d['S'], P, d['Y'], a, dv, ns, dcb, d['noise'][k], H)
        for b in range(R.B):
            s = slice(b, b + 1)
            Xo = A.langevin_step(d['X'][s], d['S'][s], P[s], d['Y'][s], a[b], dv[b], ns[b], d['noise'][k][s],
                                 dc_boost32=dcb[b] if dcb[b] != 0 else None)
            assert R.rel_err64(Xo, X64[s])[0] < 1e-6, (b, k)
            assert abs(A.nmse(Xo, H[s])[0] / nm64[b] - 1) < 1e-6, (b, k)
            assert 0.1 < nm64[b] < 20                          # order 1: the ratio above is well conditioned


def test_dc_boost_zero_reads_as_one():
    d = R.make_inputs((7, 2, 3))
    P, H = d['P'][R.P_INDEX], d['H'][R.H_INDEX]
    X0, n0 = R.langevin64(d['X'], d['S'], P, d['Y'], 0.3, 7.0, 0.05, 0.0, d['noise'][0], H)
    X1, n1 = R.langevin64(d['X'], d['S'], P, d['Y'], 0.3, 7.0, 0.05, 1.0, d['noise'][0], H)
    assert np.array_equal(X0, X1) and np.array_equal(n0, n1)


def test_philox_fed_reference_has_unit_complex_normal_moments():
    """The variant of the reference that draws what the kernels draw themselves (step >= 0: Langevin, -1: measurements).
    Loose moments only: the stream itself is pinned in tests/test_oracle_golden.py and on the device in test_gpu_parity.py."""
    seed, ids = 2 ** 63 + 12345, [11, 2 ** 33 + 1, 5, 0, 7]
    for step, shape in ((1, (64, 16)), (-1, (38, 16))):
        n = R.philox_noise(seed, ids, step, shape)
        assert n.shape == (5,) + shape and n.dtype == np.complex64
        assert abs(np.mean(n)) < 0.05 and abs(np.mean(np.abs(n) ** 2) - 1) < 0.05
        assert abs(np.mean(n.real ** 2) - 0.5) < 0.05 and abs(np.mean(n.real * n.imag)) < 0.05
        assert len({n[i].tobytes() for i in range(5)}) == 5       # one stream per trajectory id
        assert np.array_equal(n[1], A.device_complex_normal(seed, ids[1], step, shape[0] * shape[1]).reshape(shape))
    assert not np.array_equal(R.philox_noise(seed, [11], 1, (64, 16)), R.philox_noise(seed, [11], 2, (64, 16)))
