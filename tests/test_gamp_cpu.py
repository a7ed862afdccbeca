"""EM-GM-AMP off the GPU: the yardstick (tests/gamp_oracle.py) against dense-matrix algebra written out by hand, its float32 and
float64 forms over the full schedule, mutations of it that the GPU tests' assertion helper must catch, the declarations of the
entry point, the host refusals and the CLI around a stubbed solver."""
import os
import re

import numpy as np
import pytest

import gamp_cases as K
import gamp_oracle as O
from conftest import ROOT

NT, NR = 64, 16


def test_operator_equals_the_dense_kronecker_matrix():
    """Y = A1 X Fr is full_A * fft2(H)(:) with full_A = kron(right_idft, local_A * left_idft) (test_em_gm_amp.m:99-105), and both
    are local_A * local_H, to the script's own tolerance (max squared error 1e-8, :106-109)."""
    H, P = K.channels(1)[0].astype(np.complex128), K.pilots(1, 38)[0]
    A1, a2, Fl, Fr = O.operator(P[None], NR)
    X = np.fft.fft2(H)
    full_A = O.dense_operator(P, NR)
    flat_Y = full_A @ X.flatten('F')
    assert full_A.shape == (38 * NR, NT * NR)
    assert np.max(np.abs((A1[0] @ X @ Fr).flatten('F') - flat_Y) ** 2) < 1e-20
    assert np.max(np.abs((P.astype(np.complex128) @ H).flatten('F') - flat_Y) ** 2) < 1e-8
    assert np.allclose(a2[0], np.abs(A1[0]) ** 2) and np.allclose(O.spatial(X, Fl, Fr), H, atol=1e-12)


def _dense_step(P, Y, theta):
    """One EM iteration of one GAMP iteration on vectors and the dense matrix, every line of the definition written out."""
    Np = P.shape[0]
    A = O.dense_operator(P, NR)                                   # [(r, p)], [(j, i)]: column-major flattening
    A2 = np.abs(A) ** 2
    y = Y.astype(np.complex128).flatten('F')
    M, N = A.shape
    A1 = P.astype(np.complex128) @ O.idft_factor(NT)
    lam = 0.5 * Np / NT
    psi = np.sum(np.abs(y) ** 2) / (101 * M)
    phibar = (np.sum(np.abs(y) ** 2) - M * psi) / (np.sum(np.abs(A1) ** 2) * lam)
    om = np.full(4, 0.25)
    phi = phibar * 4.0 ** np.arange(4) * 4 / 85
    xhat, taux, s = np.zeros(N, complex), np.full(N, lam * phibar), np.zeros(M, complex)
    taup = A2 @ taux
    phat = A @ xhat - taup * s
    s_new = (y - phat) / (taup + psi)
    taus = 1 / (taup + psi)                                       # the first iteration is undamped
    zhat = phat + taup * s_new
    tauz = taup * psi / (taup + psi)
    s = s_new
    taur = 1 / (A2.T @ taus)
    rhat = xhat + taur * (A.conj().T @ s)
    r2 = np.abs(rhat) ** 2
    a = np.empty((5, N))
    a[0] = (1 - lam) / taur * np.exp(-r2 / taur)
    for l in range(4):
        a[1 + l] = lam * om[l] / (phi[l] + taur) * np.exp(-r2 / (phi[l] + taur))
    beta = a / a.sum(0)
    g = phi[:, None] / (phi[:, None] + taur)
    m = phi[:, None] * taur / (phi[:, None] + taur) + g ** 2 * r2
    xhat = (beta[1:] * g).sum(0) * rhat
    taux = (beta[1:] * m).sum(0) - np.abs(xhat) ** 2
    pi = beta[1:].sum(0)
    new = dict(lam=min(max(pi.mean(), 1 / N), 1), om=beta[1:].sum(1) / pi.sum(), phi=(beta[1:] * m).sum(1) / beta[1:].sum(1),
               psi=np.mean(np.abs(y - zhat) ** 2 + tauz))
    unflat = lambda v, rows: v.reshape(NR, rows).T                # column-major vector -> [rows, Nr]
    return dict(taup=unflat(taup, Np), phat=unflat(phat, Np), s_new=unflat(s_new, Np), zhat=unflat(zhat, Np), tauz=unflat(tauz, Np),
                taur=unflat(taur, NT), rhat=unflat(rhat, NT), beta=np.stack([unflat(b, NT) for b in beta[1:]], -1),
                m=np.stack([unflat(v, NT) for v in m], -1), xhat=unflat(xhat, NT), taux=unflat(taux, NT), **new)


@pytest.mark.parametrize('n_pilots,snr', [(38, 0.0), (5, 15.0)])
def test_one_step_equals_a_dense_matrix_gamp_step(n_pilots, snr):
    """B = 1, nit = 1, em_iters = 1: every intermediate of the restatement equals the dense-matrix step."""
    P, Y, H, pidx, hidx, _ = K.problem(n_pilots, (snr,), 1, n_matrices=1)
    H = H.astype(np.complex128)
    ref = _dense_step(P[0], Y[0], 0.3)
    A1, a2, Fl, Fr = O.operator(P, NR)
    st = O.initial_state(A1, a2, Y.astype(np.complex128), np.float64)
    q = O.gamp_iteration(st, A1, a2, Fr, Y.astype(np.complex128), 0.3, True)
    close = lambda a, b: np.allclose(a, b, rtol=1e-9, atol=1e-12 * np.max(np.abs(b)))
    for name in ('phat', 's_new', 'zhat', 'rhat', 'beta', 'm'):
        assert close(q[name][0], ref[name]), name
    for name in ('taup', 'tauz'):                                 # the same for every column
        assert close(q[name][0][:, None] * np.ones(NR), ref[name]), name
    assert close(q['taur'][0][:, None] * np.ones(NR), ref['taur'])
    assert close(st['xhat'][0], ref['xhat']) and close(st['taux'][0], ref['taux'])
    O.em_update(st, q, Y.astype(np.complex128))
    for name in ('lam', 'om', 'phi', 'psi'):
        assert close(st[name][0], ref[name]), name
    r = O.run(P, Y, H, nit=1, em_iters=1, tol=0.0)
    assert close(r['X'][0], ref['xhat']) and close(r['params'][0], np.concatenate([[ref['lam']], ref['om'], ref['phi'], [ref['psi']]]))
    assert close(r['log'][0, 0], np.sum(np.abs(O.spatial(ref['xhat'], Fl, Fr) - H[0]) ** 2) / np.sum(np.abs(H[0]) ** 2))


@pytest.mark.parametrize('n_pilots', [1, 2, 3, 16, 17, 64])
def test_both_precisions_stay_finite_over_the_full_schedule(n_pilots):
    """200 x 10 at theta = 0.3, at -30, 0, 15 and 40 dB, in float64 and in float32 / complex64"""
    P, Y, H, pidx, hidx, _ = K.problem(n_pilots, (-30.0, 0.0, 15.0, 40.0), 1, n_matrices=1)
    for dtype in (np.float64, np.float32):
        r = O.run(P, Y, H, tol=0.0, p_index=pidx, h_index=hidx, dtype=dtype)
        assert r['X'].dtype == (np.complex128 if dtype == np.float64 else np.complex64) and r['log'].dtype == dtype
        assert all(np.all(np.isfinite(r[k])) for k in ('X', 'H_hat', 'params', 'log')), dtype
        assert np.all(r['stop_iter'] == 200) and not np.any(r['log'] == O.SENTINEL)


@pytest.mark.parametrize('mutation', [dict(theta=1.0), dict(onsager=False), dict(nr_factor=False)])
def test_mutations_of_the_yardstick_trip_the_assertion(mutation):
    """theta = 1 instead of 0.3, the Onsager term dropped, taur without the Nr factor: each, handed to the GPU tests' assertion helper
    in the kernel's place (after 2 EM iterations at Np = 38, 0 dB), fails it; the unmutated float32 restatement passes."""
    P, Y, H, pidx, hidx, _ = K.problem(38, (0.0,), 2)
    kw = dict(em_iters=2, tol=0.0, p_index=pidx, h_index=hidx)
    r64, r32 = O.run(P, Y, H, **kw), O.run(P, Y, H, dtype=np.float32, **kw)
    bad = O.run(P, Y, H, dtype=np.float32, **dict(kw, **mutation))
    for b in range(2):
        O.assert_within('restatement', r32['X'][b], r32['X'][b], r64['X'][b])
        for name, ref in (('X', 'X'), ('H_hat', 'H_hat'), ('log', 'log')):
            pick = (lambda a: a[:, b]) if name == 'log' else (lambda a: a[b])
            with pytest.raises(AssertionError, match='exceeds the bound|not finite'):      # theta = 1 diverges
                O.assert_within(name, pick(bad[name]), pick(r32[ref]), pick(r64[ref]))


def test_early_stop_cases_are_clear_of_the_tolerance():
    """The seeds of the GPU early-stop test: the float64 criterion of every problem stays outside tol (1 +- 1e-3) at every iteration,
    some problems stop early and none before the second iteration; the rows behind a stop keep the sentinel.  The oracle is given the
    theta the descriptor carries (the fp32 value of 0.3): at Np = 12 the iteration is sensitive enough for 0.3 against 0.3f to move a
    stop (float64 with 0.3: [40 40 12 25 6 4]; with 0.3f: [40 40 12 20 6 4])."""
    for n_pilots, tol in K.STOP_CASES:
        P, Y, H, pidx, hidx, _ = K.problem(n_pilots, (-10.0, 0.0, 15.0), 2, seed=5)
        r = O.run(P, Y, H, em_iters=40, tol=tol, theta=K.THETA32, p_index=pidx, h_index=hidx, return_crit=True)
        with np.errstate(invalid='ignore'):
            near = np.abs(r['crit'] / tol - 1) <= 1e-3
        assert not np.any(near & np.isfinite(r['crit']))
        assert np.any(r['stop_iter'] < 40) and np.all(r['stop_iter'] >= 2)
        for b, k in enumerate(r['stop_iter']):
            assert np.all(r['log'][k:, b] == O.SENTINEL) and not np.any(r['log'][:k, b] == O.SENTINEL)
            assert np.all(np.isnan(r['crit'][k:, b])) and r['crit'][k - 1, b] < tol or k == 40


def test_header_and_binding_declare_the_entry_point():
    from score_based_channels_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'sbc_hip.h')).read()
    assert 'sbc_em_gm_amp_run' in _lib.EXPORTS and _lib.ABI_VERSION == 16
    assert re.search(r'int sbc_em_gm_amp_run\(const sbc_em_gm_amp_desc\* desc, void\* stream\);', header)
    body = re.search(r'typedef struct sbc_em_gm_amp_desc \{(.*?)\} sbc_em_gm_amp_desc;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'[\s\*,]([A-Za-z_]\w*)\s*(?=[,;])', body)
    assert names == [f[0] for f in _lib.sbc_em_gm_amp_desc._fields_], names
    # the limit is stated where the entry point is declared
    assert 'not available' in header[header.index('sbc_em_gm_amp_run: '):header.index('typedef struct sbc_em_gm_amp_desc')]


def test_host_refusals():
    from score_based_channels_amd import baselines
    P, Y, H = K.pilots(2, 38), np.zeros((2, 38, NR), np.complex64), K.channels(2)
    ok = dict(nit=10, em_iters=200, tol=1e-1, theta=0.3)
    baselines.check_em_gm_amp_args(P.shape, Y.shape, H.shape, **ok)
    baselines.check_em_gm_amp_args(P.shape, Y.shape, None, **ok)
    for over in (dict(nit=0), dict(nit=2.5), dict(em_iters=0), dict(theta=0.0), dict(theta=1.01), dict(theta=float('nan')),
                 dict(tol=-1e-3), dict(tol=float('inf')), dict(tol=float('nan'))):
        with pytest.raises(ValueError, match=list(over)[0]):
            baselines.check_em_gm_amp_args(P.shape, Y.shape, H.shape, **dict(ok, **over))
    for shapes in (((2, 38, 32), (2, 38, NR), (2, 32, NR)), ((2, 38, NT), (2, 38, 8), (2, NT, 8)), ((2, 38, NT), (2, 37, NR), (2, NT, NR)),
                   ((2, 65, NT), (2, 65, NR), (2, NT, NR)), ((2, 0, NT), (2, 0, NR), (2, NT, NR)), ((2, 38, NT), (2, 38, NR), (2, NT, 8))):
        with pytest.raises(ValueError):
            baselines.check_em_gm_amp_args(*shapes, **ok)
    # the data checks of the entry point come before any launch (and before any device is touched)
    with pytest.raises(ValueError, match='complex'):
        baselines.em_gm_amp(P.real, Y, H)
    with pytest.raises(ValueError, match='p_index'):
        baselines.em_gm_amp(P, np.zeros((3, 38, NR), np.complex64), H, h_index=[0, 1, 0])
    with pytest.raises(ValueError, match='out of range'):
        baselines.em_gm_amp(P, Y, H, h_index=[0, 2])
    with pytest.raises(ValueError, match='theta'):
        baselines.em_gm_amp(P, Y, H, theta=0)


def test_cli_defaults_are_the_scripts():
    from score_based_channels_amd import test_em_gm_amp as cli
    a = cli.parse_args([])
    assert list(a.channels) == ['CDL-A', 'CDL-B', 'CDL-C', 'CDL-D'] and list(a.alpha) == [0.6] and a.num_samples == 100
    assert np.array_equal(np.asarray(a.snr_range), np.arange(-30, 15.1, 2.5)) and len(a.snr_range) == 19
    assert (a.em_iters, a.tol, a.nit, a.theta, a.noise) == (200, 1e-1, 10, 0.3, 'host') and not a.synthetic and a.seed is None
    assert cli.SENTINEL == 1000 and (cli.TRAIN_SEED, cli.TEST_SEED) == (1234, 4321)
    assert cli.data_file('./data', 'CDL-C', 4321) == './data/CDL-C_Nt64_Nr16_ULA0.50_seed4321.mat'
    assert cli.data_file('./data', 'CDL-D', 1234) == './data/CDL-D_Nt64_Nr16_ULA0.5_seed1234.mat'
    assert cli.result_file('out', 'CDL-B', 10) == os.path.join('out', 'CDL-B_nit10.pt')
    assert 4 * len(a.snr_range) * a.num_samples == 7600


def test_cli_writes_the_three_logs_around_a_stubbed_solver(tmp_path):
    """Two profiles, 3 SNR points, 5 samples, 4 EM iterations; the stub stops sample n after 1 + n % 4 iterations.  Shapes, the
    sentinel, the final and the best NMSE, the file names, the operands the solver is handed."""
    import torch
    from score_based_channels_amd import test_em_gm_amp as cli
    seen = []

    def stub(P, Y, H, index, args, device):
        seen.append((P.shape, Y.shape, H.shape, index.copy(), P.dtype, Y.dtype))
        B = Y.shape[0]
        stop = 1 + index % 4
        log = np.full((args.em_iters, B), cli.SENTINEL)
        for b in range(B):
            log[:stop[b], b] = 0.5 - 0.1 * np.arange(stop[b]) + 0.25 * (np.arange(stop[b]) == 2) + 0.001 * b
        return log, stop
    out = cli.main(['--synthetic', '--seed', '3', '--num_samples', '5', '--snr_range', '-10', '0', '10', '--em_iters', '4', '--channels',
                    'CDL-A', 'CDL-D', '--result_dir', str(tmp_path)], solve_fn=stub)
    assert sorted(os.listdir(tmp_path)) == ['CDL-A_nit10.pt', 'CDL-D_nit10.pt'] and len(seen) == 2
    shapes = seen[0]
    assert shapes[0] == (5, 38, NT) and shapes[1] == (15, 38, NR) and shapes[2] == (5, NT, NR) and shapes[4] == shapes[5] == np.complex64
    assert np.array_equal(shapes[3], np.tile(np.arange(5), 3))
    for profile in ('CDL-A', 'CDL-D'):
        saved = torch.load(str(tmp_path / ('%s_nit10.pt' % profile)), weights_only=False)
        cl, ol, bl = saved['complete_log'], saved['oracle_log'], saved['best_log']
        assert cl.shape == (1, 3, 4, 5) and ol.shape == (1, 3, 5) and bl.shape == (1, 3, 5)
        assert np.array_equal(cl, out[profile]['complete_log'])
        for si in range(3):
            for n in range(5):
                stop = 1 + n % 4
                col = cl[0, si, :, n]
                assert np.all(col[stop:] == cli.SENTINEL) and np.all(col[:stop] < 1)
                assert ol[0, si, n] == col[stop - 1] and bl[0, si, n] == col[:stop].min()
        assert bl[0, 0, 2] < ol[0, 0, 2]                         # the best row is not always the last one


def test_cli_measurements_follow_the_noise_model(tmp_path):
    """Y - P H has the variance 10^(-snr/10) of :85-86, :112-113 at every SNR point, and the same seed gives the same draws."""
    from score_based_channels_amd import test_em_gm_amp as cli
    got = []

    def stub(P, Y, H, index, args, device):
        got.append((Y.astype(np.complex128) - np.matmul(P.astype(np.complex128), H.astype(np.complex128))[index]).reshape(2, 40, -1))
        return np.zeros((args.em_iters, Y.shape[0])), np.full(Y.shape[0], args.em_iters)
    argv = ['--synthetic', '--seed', '9', '--num_samples', '40', '--snr_range', '-20', '10', '--em_iters', '1', '--channels', 'CDL-B',
            '--result_dir', str(tmp_path)]
    cli.main(argv, solve_fn=stub)
    cli.main(argv, solve_fn=stub)
    assert np.array_equal(got[0], got[1])
    for si, snr in enumerate((-20.0, 10.0)):
        var = np.mean(np.abs(got[0][si]) ** 2)
        assert abs(var / 10 ** (-snr / 10) - 1) < 0.03, (snr, var)             # 24320 complex draws: 3 % is 4.7 sigma
