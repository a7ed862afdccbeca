"""CPU tests of the WGAN baseline's host side: the oracle against the reference's fixture, the state-dict spec, the argument checks, the
oracle's Adam against torch.optim.Adam, and the command-line script's file contract with an injected estimate function (no GPU here)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import wgan_oracle as O
from score_based_channels_amd import test_wgan as cli
from score_based_channels_amd import wgan


@pytest.fixture(scope='module')
def fix():
    g = O.golden_step()
    return g, wgan.seeded_state_dict(int(g['seed_weights']), int(g['n_extra']))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_oracle_matches_the_reference_fixture(fix, dtype):
    """float64: the restatement computes what the reference module computes (1e-11: summation order only); float32: it is one more
    fp32 implementation, so it is held to rule R, error against float64 <= 4 x the reference's own fp32 error."""
    g, sd = fix
    r = O.step_terms(sd, g['z'], g['Y'], g['P'], g['H'], g['lam'], g['scale'], dtype)
    for k in ('gen', 'meas', 'reg', 'nmse', 'g'):
        B = g['z'].shape[0]
        err = O.normwise(r[k].reshape(B, -1), g[k + '64'].reshape(B, -1))
        e_ref = O.normwise(g[k + '32'].reshape(B, -1), g[k + '64'].reshape(B, -1))
        print('%s %s: err %.2e, e_ref %.2e' % (dtype, k, err, e_ref))
        assert err <= (1e-11 if dtype == torch.float64 else 4 * e_ref), (k, err, e_ref)


def test_masked_oracle_equals_the_free_one_under_its_own_masks(fix):
    g, sd = fix
    free = O.step_terms(sd, g['z'][:2], g['Y'][:2], g['P'][:2], g['H'][:2], g['lam'][:2], g['scale'][:2], torch.float64)
    masks = [p > 0 for p in free['pre']]
    held = O.step_terms(sd, g['z'][:2], g['Y'][:2], g['P'][:2], g['H'][:2], g['lam'][:2], g['scale'][:2], torch.float64, masks=masks)
    for k in ('gen', 'meas', 'g', 'dG'):
        assert O.normwise(held[k], free[k]) < 1e-13, k
    # the layer-wise adjoints chain up to the same gradient
    L = O.n_layers(sd)
    grad = O.out_vjp(sd, free['dG'], torch.float64)
    for k in range(L, 0, -1):
        grad = O.layer_vjp(sd, k, grad, masks[k - 1], torch.float64)
    gz = O.dense_vjp(sd, grad, torch.float64) + 2 * (g['scale'][:2] * g['lam'][:2]).astype(np.float64)[:, None] * g['z'][:2]
    assert O.normwise(gz, free['g']) < 1e-12


def test_state_dict_spec_matches_the_reference_module():
    with open(os.path.join(GOLDEN, 'wgan_state_dict_keys.json')) as f:
        ref = json.load(f)
    assert [(n, list(s)) for n, s in wgan.state_dict_spec(ref['n_extra'])] == [(n, list(s)) for n, s in ref['keys']]
    for n_extra in range(5):
        sd = wgan.seeded_state_dict(5, n_extra)
        wgan.check_state_dict(sd, n_extra)
        assert wgan.n_extra_of(sd) == n_extra and len(sd) == 18 + 6 * n_extra
    a, b = wgan.seeded_state_dict(5, 1), wgan.seeded_state_dict(5, 3)
    assert all(np.array_equal(a[k], b[k]) for k in a)          # a tensor depends on the seed and its name only
    assert not np.array_equal(a['conv.conv1.weight'], wgan.seeded_state_dict(6, 1)['conv.conv1.weight'])
    assert np.all(a['conv.bn1.running_var'] > 0.5) and a['conv.bn1.num_batches_tracked'].dtype == np.int64


def test_argument_checks():
    with pytest.raises(ValueError):
        wgan.state_dict_spec(5)
    for bad in (([16, 32], 60, 2, 128), ([64, 16], 60, 2, 128), ([16, 64], 100, 2, 128), ([16, 64], 60, 1, 128), ([16, 64], 60, 2, 64)):
        with pytest.raises(ValueError):
            wgan.check_geometry(*bad)
    with pytest.raises(ValueError):
        wgan.check_geometry([16, 64], 60, 2, 128, 5)
    with pytest.raises(ValueError):
        wgan.DCGAN_G_Ours([32, 64], 60, 2, 128, 1, 1)
    assert wgan.check_geometry([16, 64], 60, 2, 128, 4) == 4
    sd = wgan.seeded_state_dict(1, 1)
    with pytest.raises(KeyError):
        wgan.check_state_dict(sd, 2)
    with pytest.raises(KeyError):
        wgan.check_state_dict(dict(sd, extra=np.zeros(1)), 1)
    with pytest.raises(ValueError):
        wgan.check_state_dict(dict(sd, **{'conv.conv_out.bias': np.zeros(3, np.float32)}), 1)
    assert wgan.check_run_args((4, 60), (4, 16, 38), (4, 64, 38), 3, (4, 16, 64)) == (4, 38)
    assert wgan.check_run_args((4, 60, 1, 1), (4, 16, 1), (4, 64, 1), 0) == (4, 1)
    for bad in (((4, 61), (4, 16, 38), (4, 64, 38), 3), ((4, 60), (4, 16, 38), (4, 64, 37), 3), ((4, 60), (3, 16, 38), (4, 64, 38), 3),
                ((4, 60), (4, 8, 38), (4, 64, 38), 3), ((4, 60), (4, 16, 65), (4, 64, 65), 3), ((4, 60), (4, 16, 38), (4, 64, 38), -1),
                ((4, 60), (4, 16, 38), (4, 64, 38), 1.5), ((4, 60), (4, 16, 38), (4, 64, 38), 3, (4, 64, 16)),
                ((4, 60), (4, 16, 38), (4, 64, 38), 3, None, 0), ((4, 60), (4, 16, 38), (4, 38), 3)):
        with pytest.raises(ValueError):
            wgan.check_run_args(*bad)
    assert wgan.per_sample(0.5, 3, 'lr').tolist() == [0.5] * 3 and wgan.per_sample([1, 2], 2, 'lr').dtype == np.float32
    for bad in ([1, 2, 3], np.nan):
        with pytest.raises(ValueError):
            wgan.per_sample(bad, 2, 'lr')
    assert wgan.stage_id('dense', 2) == 0 and wgan.stage_id('act4', 2) == 4 and wgan.stage_id('grad0', 0) == 32 and wgan.stage_id('mask1', 0) == 49
    for bad in ('act5', 'mask0', 'grad7', 'nope'):
        with pytest.raises(ValueError):
            wgan.stage_id(bad, 2)
    words = np.array([[1, -2 ** 31]], np.int32)
    m = wgan.unpack_mask(words, 64)
    assert m.shape == (1, 64) and m[0, 0] and m[0, 63] and m.sum() == 2


@pytest.mark.parametrize('lr', [0.03, 0.001])
def test_oracle_adam_is_torch_adam(lr):
    rng = np.random.default_rng(4)
    z0, gs = rng.standard_normal((3, 60)), rng.standard_normal((12, 3, 60)) * np.geomspace(1, 1e-3, 12)[:, None, None]
    for dtype, tol in ((np.float64, 1e-13), (np.float32, 3e-7)):
        p = torch.tensor(z0.astype(dtype), requires_grad=True)
        opt = torch.optim.Adam([p], lr=lr)
        ref = []
        for g in gs:
            p.grad = torch.from_numpy(g.astype(dtype))
            opt.step()
            ref.append(p.detach().numpy().copy())
        got = O.adam(gs, z0, lr, dtype)
        assert got.dtype == dtype
        for k in range(len(gs)):
            assert O.normwise(got[k], ref[k]) <= tol, (dtype, k)
    per = O.adam(gs, z0, np.array([lr, lr / 2, lr])[:, None], np.float64)          # a per-sample step size
    assert np.array_equal(per[:, 0], O.adam(gs, z0, lr, np.float64)[:, 0]) and not np.array_equal(per[:, 1], O.adam(gs, z0, lr, np.float64)[:, 1])


def test_noise_power_is_half_the_snr_points(fix):
    """test_wgan.py:131-132: sqrt(noise) / sqrt(2) x a complex normal of TOTAL variance 1 -> noise power noise / 2"""
    g, _ = fix
    np.random.seed(9)
    H, P = np.tile(g['H'], (25, 1, 1)), np.tile(g['P'], (25, 1, 1))
    n = cli.host_normal((100, 16, 38))
    assert abs(np.mean(np.abs(n) ** 2) - 1.0) < 0.02
    for noise in (10.0, 0.1):
        Y = cli.noisy_measurements(H, P, noise, n)
        assert Y.dtype == np.complex64
        power = np.mean(np.abs(Y - np.matmul(H, P)) ** 2)
        assert abs(power / (noise / 2) - 1) < 0.03, (noise, power)


def _fake_estimate(calls):
    def f(netG, problem, device):
        calls.append(problem)
        B, steps = problem['z0'].shape[0], problem['steps']
        base = np.arange(steps, dtype=np.float32)[:, None] + problem['lr'][None, :].astype(np.float32) * 1000
        return {'oracle': base + problem['l2_lam'][None, :].astype(np.float32), 'meas': base + 0.25, 'reg': np.tile(np.sum(problem['z0'] ** 2, 1), (steps, 1))}
    return f


def test_cli_file_contract_with_an_injected_estimate(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    calls = []
    argv = ['--synthetic', '--synthetic_weights', '13', '--kept_samples', '4', '--total_steps', '3', '--snr_range', '0', '10',
            '--l2lam_range', '0.1', '1', '--lr_range', '0.01', '--alpha_range', '0.6', '1', '--noise', 'host']
    out = cli.main(argv, estimate_fn=_fake_estimate(calls))
    path = tmp_path / 'wgan_CDL-C_0.50' / 'extra1' / 'wgan_results_modelCDL-C_channelCDL-C_DETAILED.pt'
    assert path.exists()
    saved = torch.load(str(path), weights_only=False)
    assert set(saved) == {'spacing_range', 'pilot_alpha_range', 'config', 'snr_range', 'val_config', 'l2lam_range', 'lr_range', 'oracle_log',
                          'meas_log', 'reg_log', 'args'}
    for k in ('oracle_log', 'meas_log', 'reg_log'):
        assert saved[k].shape == (2, 1, 2, 2, 3, 4) and np.array_equal(saved[k], out[k])
    assert saved['val_config']['data']['num_pilots'] == 64 and saved['config']['data']['norm_channels'] == 'entrywise'
    # one batch per pilot fraction: (l2_lam, lr, SNR) cells x kept samples, the same initial points in every block
    assert [c['P'].shape for c in calls] == [(16, 64, 38), (16, 64, 64)] and all(c['Y'].shape[:2] == (16, 16) for c in calls)
    z0 = O.init_z(4)
    assert all(np.array_equal(c['z0'], np.tile(z0, (4, 1))) for c in calls)
    assert np.allclose(calls[0]['loss_scale'], 0.25) and calls[0]['l2_lam'].tolist() == [0.1] * 8 + [1.0] * 8
    # the logs land in their cells: oracle = step + 1000 lr + l2_lam
    assert np.allclose(saved['oracle_log'][1, 0, 1, 0, 2], 2 + 10 + 1.0) and np.allclose(saved['oracle_log'][0, 0, 0, 1, 0], 10 + 0.1)
    assert np.allclose(saved['reg_log'][0, 0, 0, 0, 0], np.sum(z0 ** 2, 1))
    # the noise of the two SNR points of a cell: power noise / 2 (32 x 16 x 38 complex draws: a few per cent)
    c = calls[0]
    for blk, noise in ((0, 1.0), (1, 0.1)):
        sl = slice(4 * blk, 4 * blk + 4)
        power = np.mean(np.abs(c['Y'][sl] - np.matmul(c['H'][sl], c['P'][sl])) ** 2)
        assert abs(power / (noise / 2) - 1) < 0.15, (noise, power)

    # a checkpoint in the reference's layout is read back (config as a mapping, gen_state under the reference's names, 1 extra layer)
    os.makedirs('wgan_CDL-D_0.50/extra1')
    torch.save({'config': cli.wgan_config('CDL-D', 0.5).toDict(), 'gen_state': {k: torch.from_numpy(np.asarray(v)) for k, v in wgan.seeded_state_dict(3, 1).items()}},
               'wgan_CDL-D_0.50/extra1/weights_epoch6000.pt')
    out = cli.main(['--synthetic', '--model', 'CDL-D', '--channel', 'CDL-D', '--kept_samples', '2', '--total_steps', '1', '--snr_range', '5',
                    '--l2lam_range', '1', '--lr_range', '0.01', '--alpha_range', '0.8'], estimate_fn=_fake_estimate(calls))
    assert out['meas_log'].shape == (1, 1, 1, 1, 1, 2) and 'noise' in calls[-1] and calls[-1]['P'].shape == (2, 64, 51)
    assert os.path.exists('wgan_CDL-D_0.50/extra1/wgan_results_modelCDL-D_channelCDL-D_DETAILED.pt')
    with pytest.raises(FileNotFoundError):
        cli.main(['--synthetic', '--model', 'CDL-A'], estimate_fn=_fake_estimate(calls))


# ---- the regimes of tests/wgan_cases.py: are they reached, and can the rule test them? -------------------------------------------------
import wgan_cases as WC  # noqa: E402

F32, F64 = torch.float32, torch.float64


def _regime_is_reached(case, sd, stand_in):
    plain = wgan.seeded_state_dict(WC.SEED_WEIGHTS, case.n_extra)
    assert O.n_layers(sd) == 2 + case.n_extra and wgan.n_extra_of(sd) == case.n_extra
    z, Y, P, H, lam, scale = WC.problem(case)
    for k in range(1, O.n_layers(sd) + 1):
        bn = O.layer_names(k)[1]
        var, w = sd[bn + '.running_var'], sd[bn + '.weight']
        if case.bn == 'var_1em4':
            assert np.all(var > 5 * O.BN_EPS) and np.all(var < 2e-4) and np.array_equal(var, plain[bn + '.running_var'] * np.float32(1e-4))
        if case.bn == 'w_1em2_signed':
            assert np.all(w[::3] < 0) and np.all(np.delete(w, np.arange(0, 128, 3)) > 0) and np.all(np.abs(w) < 0.013) and np.all(np.abs(w) > 0.007)
        if case.bn == 'w_zero8':
            assert np.count_nonzero(w == 0) == 8 and np.all(w[WC.ZERO_CHANNELS] == 0)
            pre = stand_in['pre'][k - 1][:, WC.ZERO_CHANNELS]
            assert np.all(pre == sd[bn + '.bias'][WC.ZERO_CHANNELS][None, :, None, None])         # the activation is constant
            g = np.zeros_like(stand_in['grad'][k])
            g[:, WC.ZERO_CHANNELS] = stand_in['grad'][k][:, WC.ZERO_CHANNELS]
            assert not np.any(O.layer_vjp(sd, k, g, stand_in['masks'][k - 1], F64))                # and nothing flows back through it
        if case.bn == 'plain':
            assert np.all(var > 0.5) and np.all(w > 0.7)
    assert np.array_equal(z, {'plain': O.init_z(WC.B), 'zero': np.zeros((WC.B, 60), np.float32), 'times8': 8 * O.init_z(WC.B)}[case.z])
    assert np.array_equal(lam, np.zeros(3, np.float32) if case.lam == 'zero' else WC.LAM) and scale == np.float32(case.scale)
    Y1 = WC.problem(case._replace(y_scale=1.0))[1]
    assert np.allclose(Y, Y1 * case.y_scale, rtol=1e-6, atol=0) and np.all(np.isfinite(Y.view(np.float32)))


@pytest.mark.parametrize('case', WC.CASES, ids=lambda c: c.name)
def test_step_case_reaches_its_regime_and_the_reference_satisfies_the_rule(case):
    """A float32 oracle's own masks, gen, dG and backward chain stand in for the kernel's."""
    sd, fsd = WC.state_dict(case)
    own = WC.oracle_step(case)
    _regime_is_reached(case, sd, own)
    refs, pre64 = WC.references(case, own['masks'], own['gen'], own['dG'], own['grad'])
    assert len(refs) == 9 + O.n_layers(sd)
    res = [WC.mutual('%s %s' % (case.name, what), r64, r32, r32f, kind) for what, _, kind, r64, r32, r32f in refs]
    # masks: both float32 orders' pre-activations lie within 1e-5 rms of float64's on every layer, a margin of 10 under the 1e-4 band
    z, Y, P, H, lam, scale = WC.problem(case)
    flipped = O.forward_terms(fsd, z, Y, P, H, F32, O.generate_flipped)['pre']
    for name, pre in (('native', own['pre']), ('flipped', flipped)):
        dist = WC.pre_distance(pre, pre64)
        print('%s pre-activations from float64, in rms of the layer: %s' % (name, ['%.2e' % d for d in dist]))
        assert max(dist) < 1e-5, (name, dist)
    # the flipped twin is the identity in float64
    a = O.step_terms(sd, z, Y, P, H, lam, scale, F64, own['masks'])
    b = O.step_terms(fsd, z, Y, P, H, lam, scale, F64, own['masks'], O.generate_flipped)
    for k in ('gen', 'g', 'dG'):
        d = O.normwise(b[k], a[k])
        print('flipped twin against native in float64, %s: %.2e' % (k, d))
        assert d < 1e-12, (k, d)
    L = O.n_layers(sd)
    assert O.normwise(O.layer_vjp_flipped(fsd, L, own['grad'][L], own['masks'][L - 1], F64), O.layer_vjp(sd, L, own['grad'][L], own['masks'][L - 1], F64)) < 1e-12
    assert O.normwise(O.out_vjp_flipped(fsd, own['dG'], F64), O.out_vjp(sd, own['dG'], F64)) < 1e-12
    assert O.normwise(O.dense_vjp_flipped(fsd, own['grad'][0], F64), O.dense_vjp(sd, own['grad'][0], F64)) < 1e-12
    s = np.full(WC.B, scale, np.float32)
    assert O.normwise(O.residual_vjp_flipped(own['gen'], Y, P, s, F64), O.residual_vjp(own['gen'], Y, P, s, F64)) < 1e-12
    WC.assert_all(res)


@pytest.mark.parametrize('first_step', WC.FIRST_STEPS)
def test_oracle_adam_continues_torch_adam(first_step):
    """``O.adam`` with ``first_step`` and initial moments is ``torch.optim.Adam`` continued from the same state, per-sample step sizes
    as one optimiser per sample."""
    m0, v0 = WC.adam_state(first_step)
    assert np.all(v0 > 0) and v0.min() < 1e-11 and v0.max() > 10 and np.count_nonzero(m0) == m0.size
    rng = np.random.default_rng(first_step + 1)
    z0, gs = rng.standard_normal((WC.B, 60)), rng.standard_normal((3, WC.B, 60)) * np.sqrt(v0)[None]
    for dtype, tol in ((np.float64, 1e-13), (np.float32, 3e-7)):
        got, m, v = O.adam(gs, z0, WC.LR.astype(np.float64)[:, None], dtype, first_step, m0, v0, return_state=True)
        assert got.dtype == dtype and got.shape == (3, WC.B, 60)
        for b in range(WC.B):
            p = torch.tensor(z0[b].astype(dtype), requires_grad=True)
            opt = torch.optim.Adam([p], lr=float(WC.LR[b]))
            opt.state[p] = {'step': torch.tensor(float(first_step - 1)), 'exp_avg': torch.tensor(m0[b].astype(dtype)),
                            'exp_avg_sq': torch.tensor(v0[b].astype(dtype))}
            for k, g in enumerate(gs):
                p.grad = torch.from_numpy(g[b].astype(dtype))
                opt.step()
                assert O.normwise(got[k, b][None], p.detach().numpy()[None]) <= tol, (dtype, b, k)
            assert float(opt.state[p]['step']) == first_step + 2
            assert O.normwise(m[b][None], opt.state[p]['exp_avg'].numpy()[None]) <= tol
            assert O.normwise(v[b][None], opt.state[p]['exp_avg_sq'].numpy()[None]) <= tol
    # from step 1 with zero moments it is the helper as it was
    assert np.array_equal(O.adam(gs, z0, 0.01, np.float64, 1, np.zeros_like(z0), np.zeros_like(z0)), O.adam(gs, z0, 0.01, np.float64))
    # and the bias corrections matter at these steps: Adam's t = 1 .. 3 gives another iterate
    assert O.normwise(O.adam(gs, z0, 0.01, np.float64, 1, m0, v0), O.adam(gs, z0, 0.01, np.float64, first_step, m0, v0)) > 1e-4
