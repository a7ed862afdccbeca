"""The classical baselines on the GPU (csrc/cs_l1.hip, csrc/cs_ls.hip through baselines.py and the two CLIs), all against the
float64 numpy oracle of tests/cs_oracle.py."""
import numpy as np
import pytest
import torch

import cs_oracle as O
from conftest import rel_err_elementwise

pytestmark = pytest.mark.gpu


def _data(B, npil, seed, snr_db, channels=None):
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


def _ri(a):
    """complex -> interleaved (re, im) components, for the element-wise comparison of conftest.rel_err_elementwise"""
    return np.ascontiguousarray(a).astype(np.complex128).view(np.float64)


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


@pytest.mark.parametrize('L', [1, 4])
def test_l1_full_run_log_matches_the_oracle(L):
    snrs, lams, per = [-10.0, 10.0, 30.0], [0.0, 0.3], 2
    cells = [(s, lam) for s in snrs for lam in lams]
    B = len(cells) * per
    snr = np.repeat([c[0] for c in cells], per)
    lam = np.repeat([c[1] for c in cells], per)
    P, Y, H = _data(B, 38, 21, snr)
    log, Hh = _gpu_l1(P, Y, H, lam, 3e-3, L, 1000)
    rlog, rH, _ = O.l1_run(P, Y, H, lam, 3e-3, L, 1000)
    err = np.abs(log / rlog - 1)
    assert np.max(err[:20]) <= 5e-6, np.max(err[:20])
    assert np.max(err[:100]) <= 2e-4, np.max(err[:100])
    assert np.max(err) <= 5e-3, np.max(err)
    # final estimate, norm-wise.  With lambda = 0 the problem is unregularised and under-determined (Np = 38 < Nt = 64): rounding
    # drifts along the null space.  The kernel's formulation (G = P^H P, Hz by linearity) restated in numpy complex64 ends
    # 2.0e-3 .. 2.4e-3 from the float64 oracle on these lambda = 0 cells and <= 5.2e-4 on the lambda = 0.3 cells (L = 1 and 4).
    for b in range(B):
        e = np.linalg.norm(Hh[b] - rH[b]) / np.linalg.norm(rH[b])
        assert e <= (2e-3 if lam[b] > 0 else 5e-3), (b, lam[b], e)


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


def test_ls_regularized_matches_lstsq():
    from score_based_channels_amd.baselines import ls_regularized
    snr = np.arange(-30, 17.5, 2.5)
    for npil in (38, 64):
        P, _, H = _data(8, npil, 51 + npil, 0.0)
        B = len(snr) * 8
        idx = np.tile(np.arange(8), len(snr))
        noise = np.repeat(10 ** (-snr / 10.), 8)
        rng = np.random.default_rng(npil)
        z = (rng.standard_normal((B, npil, 16)) + 1j * rng.standard_normal((B, npil, 16))) / np.sqrt(2)
        Y = (P[idx] @ H[idx] + np.sqrt(noise)[:, None, None] * z).astype(np.complex64)
        Hh, nmse = ls_regularized(torch.from_numpy(P).cuda(), torch.from_numpy(Y).cuda(), noise, H=torch.from_numpy(H).cuda(),
                                  p_index=idx, h_index=idx)
        torch.cuda.synchronize()
        Hh, nmse = Hh.cpu().numpy(), nmse.cpu().numpy()
        rH, rn = O.lstsq_run(P[idx].astype(np.complex128), Y.astype(np.complex128), H[idx].astype(np.complex128), noise)
        eH = np.linalg.norm((Hh - rH).reshape(B, -1), axis=1) / np.linalg.norm(rH.reshape(B, -1), axis=1)
        assert np.max(eH) <= 1e-4, (npil, np.max(eH))
        assert np.max(np.abs(nmse / rn - 1)) <= 3e-4, (npil, np.max(np.abs(nmse / rn - 1)))


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
