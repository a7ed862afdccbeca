"""Learned D-AMP without a GPU: the project's CPU oracle (tests/ldamp_oracle.py) against the fixtures written from the reference's own
modules (tests/gen_golden_ldamp.py), the state_dict key grammar, the host-side argument checks and the CLI's file layout."""
import json
import os

import numpy as np
import pytest
import torch

import ldamp_oracle as O
from conftest import GOLDEN, load_golden
from score_based_channels_amd import ldamp


@pytest.fixture(scope='module')
def weights():
    return ldamp.seeded_state_dict(int(load_golden('ldamp_unet.npz')['seed_weights']))


def test_oracle_float64_matches_reference_float64(weights):
    """The same arithmetic in float64 from two implementations: agreement to rounding of float64 amplified by the 1/eps of the divergence
    (1e3) over ten unrolls -- 1e-9 leaves three orders of margin below the fp32 effects the GPU tests measure."""
    g = O.golden_unet()
    assert O.normwise(O.denoise(weights, 0, g['r'], torch.float64), g['out64']) < 1e-12
    u = O.golden_unroll()
    log = O.run_oracle(weights, u['Y_herm'], u['P_herm'], u['eig1'], u['directions'], 10, torch.float64)
    for k in range(10):
        assert O.normwise(log['h'][k], u['h64'][k]) < 1e-9 and O.normwise(log['z'][k], u['z64'][k]) < 1e-9, k
        assert O.absolute(log['div'][k], u['div64'][k]) < 1e-9 and O.absolute(log['eps'][k], u['eps64'][k]) < 1e-12, k


def test_oracle_float32_matches_reference_float32(weights):
    """fp32 oracle against the reference's fp32: both are fp32 evaluations of the same expression, so each is within e_ref-like distance
    of float64; their mutual distance is bounded by the rule of the GPU tests, 4 x e_ref (+ e_ref for the reference's own error)."""
    g = O.golden_unet()
    e_ref = O.normwise(g['out32'], g['out64'])
    assert O.normwise(O.denoise(weights, 0, g['r'], torch.float32), g['out64']) <= 4 * e_ref
    u = O.golden_unroll()
    log = O.run_oracle(weights, u['Y_herm'], u['P_herm'], u['eig1'], u['directions'], 10, torch.float32)
    for k in range(10):
        assert O.normwise(log['h'][k], u['h64'][k]) <= 4 * O.normwise(u['h32'][k], u['h64'][k]), k
        assert O.normwise(log['z'][k], u['z64'][k]) <= 4 * O.normwise(u['z32'][k], u['z64'][k]), k
        assert O.absolute(log['div'][k], u['div64'][k]) <= 4 * O.absolute(u['div32'][k], u['div64'][k]), k


def test_state_dict_key_grammar():
    keys = json.load(open(os.path.join(GOLDEN, 'ldamp_state_dict_keys.json')))['keys']
    spec = ldamp.state_dict_spec()
    assert len(keys) == 190 and [(n, list(s)) for n, s in spec] == [(k, list(s)) for k, s in keys]
    sd = ldamp.seeded_state_dict(3)
    assert list(sd) == [n for n, _ in spec] and all(sd[n].shape == tuple(s) and sd[n].dtype == np.float32 for n, s in spec)
    again, other = ldamp.seeded_state_dict(3), ldamp.seeded_state_dict(4)
    n0 = 'update_nets.0.unet.conv.layers.0.weight'
    assert np.array_equal(sd[n0], again[n0]) and not np.array_equal(sd[n0], other[n0])
    assert np.max(np.abs(sd[n0])) <= 1 / np.sqrt(64 * 9) and np.max(np.abs(sd[n0])) > 0.99 / np.sqrt(64 * 9)
    # a tensor depends on the seed and its own name only
    assert np.array_equal(ldamp.seeded_state_dict(3, max_unrolls=2)['update_nets.1.unet.up_conv.2.1.bias'], sd['update_nets.1.unet.up_conv.2.1.bias'])
    ldamp.check_state_dict(sd, 10)
    bad = dict(sd)
    bad.pop(n0)
    with pytest.raises(KeyError):
        ldamp.check_state_dict(bad, 10)
    bad = dict(sd)
    bad[n0] = bad[n0][:, :32]
    with pytest.raises(ValueError):
        ldamp.check_state_dict(bad, 10)


def test_rejected_settings_and_shapes_on_the_host():
    ok = {'backbone': 'FlippedUNet', 'shared_nets': False, 'max_unrolls': 10, 'in_channels': 2}
    assert ldamp.check_hparams(ok) == 10
    for key, val in (('backbone', 'DnCNN'), ('backbone', 'UNet'), ('shared_nets', True), ('in_channels', 4), ('max_unrolls', 0)):
        with pytest.raises(ValueError, match=key):
            ldamp.check_hparams(dict(ok, **{key: val}))
    from score_based_channels_amd.test_ldamp import ldamp_config
    assert ldamp.check_hparams(ldamp_config().model) == 10            # the attribute-style config of a checkpoint
    ldamp.check_run_args((4, 38, 16), (4, 38, 64), (4,), 10, 10, (10, 4, 64, 16, 2))
    for Y, P, e, U, D in (((4, 38, 8), (4, 38, 64), (4,), 10, None), ((4, 38, 16), (4, 38, 32), (4,), 10, None),
                          ((4, 65, 16), (4, 65, 64), (4,), 10, None), ((4, 0, 16), (4, 0, 64), (4,), 10, None),
                          ((4, 38, 16), (3, 38, 64), (4,), 10, None), ((4, 38, 16), (4, 38, 64), (3,), 10, None),
                          ((4, 38, 16), (4, 38, 64), (4,), 11, None), ((4, 38, 16), (4, 38, 64), (4,), 0, None),
                          ((4, 38, 16), (4, 38, 64), (4,), 10, (9, 4, 64, 16, 2))):
        with pytest.raises(ValueError):
            ldamp.check_run_args(Y, P, e, U, 10, D)


def test_cli_parsing_and_result_layout(tmp_path, monkeypatch):
    """The CLI end to end with the estimator stubbed: argument defaults of the reference, the checkpoint path pattern, the loader's
    settings per SNR point and the layout of results.pt."""
    from score_based_channels_amd import test_ldamp as T
    a = T.parse_args([])
    assert (a.gpu, a.train, a.test, a.num_channels, a.noise) == (0, 'CDL-C', 'CDL-C', 100, 'device')
    assert list(a.snr_range) == [-10, -5, 0, 5, 10, 15, 20, 25, 30]
    assert T.checkpoint_path('CDL-C', -10.0, 0.6) == './models/ldamp-FlippedUNet/train-CDL-C/model_snr-10.00_alpha0.60.pt'
    monkeypatch.chdir(tmp_path)
    seen = []

    def stub(model, batch, num_unrolls, directions, seed, device):
        seen.append((batch, num_unrolls, directions, seed))
        return np.full(batch['Y_herm'].shape[0], 0.5 + len(seen))

    out = T.main(['--synthetic', '--synthetic_weights', '7', '--seed', '1', '--noise', 'host', '--snr_range', '0', '20', '--num_channels', '8',
                  '--no_plot'], estimate_fn=stub)
    saved = torch.load(tmp_path / 'results' / 'ldamp' / 'train-CDL-C_test-CDL-C' / 'results.pt', weights_only=False)
    assert set(saved) == {'nmse_log', 'avg_nmse', 'snr_range', 'pilot_alpha_range', 'spacing_range', 'config', 'args'}
    assert saved['nmse_log'].shape == (1, 1, 2, 8) and saved['nmse_log'].dtype == np.float64
    assert np.array_equal(saved['avg_nmse'], [[[1.5, 2.5]]]) and list(saved['snr_range']) == [0.0, 20.0]
    assert saved['pilot_alpha_range'] == [0.6] and saved['spacing_range'] == [0.5] and saved['config']['model']['max_unrolls'] == 10
    assert np.array_equal(out['nmse_log'], saved['nmse_log'])
    assert len(seen) == 2
    for (batch, U, d, seed), snr in zip(seen, (0.0, 20.0)):
        assert U == 10 and seed == 1 and d.shape == (10, 8, 64, 16, 2) and d.dtype == np.float32
        assert batch['Y_herm'].shape == (8, 38, 16) and batch['P_herm'].shape == (8, 38, 64) and batch['eig1'].shape == (8,)
        assert batch['H_herm_cplx'].shape == (8, 64, 16) and batch['Y_herm'].dtype == np.complex64
        # the loader added noise of std 10^(-snr/20) sqrt(64) per complex entry (:83)
        resid = batch['Y_herm'] - batch['P_herm'] @ batch['H_herm_cplx']
        assert abs(np.sqrt(np.mean(np.abs(resid) ** 2)) / (10 ** (-snr / 20) * 8) - 1) < 0.05


# ---- the regimes of tests/ldamp_cases.py: are they reached, and can the rule test them? -----------------------------------------------
import ldamp_cases as LC  # noqa: E402

F32, F64 = torch.float32, torch.float64


def _twin_is_the_identity_in_float64(sd, fsd, net, r):
    x = torch.from_numpy(LC.planes_of(r)).double()
    with torch.no_grad():
        a, b = O.denoise_planes(sd, net, x, F64), O.denoise_planes_flipped(fsd, net, x, F64)
        a32, b32 = O.denoise_planes(sd, net, x.float(), F32), O.denoise_planes_flipped(fsd, net, x.float(), F32)
    d = O.normwise(b.numpy(), a.numpy())
    print('flipped twin against native: float64 %.2e, float32 same bits: %s' % (d, bool(torch.equal(a32, b32))))
    assert d < 1e-12
    assert not torch.equal(a32, b32)                                  # and in float32 it is another order, not the same one


@pytest.mark.parametrize('case', LC.LAYER_CASES, ids=lambda c: c.name)
def test_layer_case_reaches_its_regime_and_the_reference_satisfies_the_rule(case):
    """The float32 oracle's stages stand in for the kernel's: every layer's input from them goes through the layer in float64 and in
    the two float32 orders."""
    sd, fsd = LC.weights(case.weights, 10 if case.weights == 'plain' else LC.UNROLLS)
    r = LC.layer_input(case)
    assert r.shape == (case.B, 64, 16) and np.all(np.isfinite(r.view(np.float32)))
    st = LC.oracle_stages(sd, case.net, r)
    if case.weights != 'plain':
        var = np.concatenate([v.ravel() for v in LC.conv_variances(sd, case.net, st)])
        share = float(np.mean(var < LC.IN_EPS))
        print('share of channels with variance below IN_EPS: %.3f (variance %.2e ... %.2e)' % (share, var.min(), var.max()))
        assert (share > 0.9) if case.weights == 'w_2m10' else (share == 0 if case.weights == 'w_2p8' else 0 < share < 1)
    if case.input == 'in_offset':
        ratio = np.abs(st['stat'][:, [0, 2]]) / st['stat'][:, [1, 3]]
        print('|mean| / std of the planes: %.1f ... %.1f' % (ratio.min(), ratio.max()))
        assert np.all(ratio > 20)
    if case.input in ('in_2m20', 'in_2p12'):
        base = LC.oracle_stages(sd, case.net, LC.layer_input(case._replace(input='plain')))
        assert np.array_equal(st['x'], base['x'])                     # a power of two: norm removes it exactly
    LC.assert_all([LC.mutual(what, ref64, a, b) for what, _, ref64, a, b in LC.layer_refs(sd, case.net, st, LC.planes_of(r))])
    _twin_is_the_identity_in_float64(sd, fsd, case.net, r)


@pytest.mark.parametrize('case', LC.MIXED[:1] + LC.LOOP_CASES, ids=lambda c: c.name)
def test_loop_case_reaches_its_regime_and_the_reference_satisfies_the_rule(case):
    r64, r32, r32f = LC.loop_refs(case)
    Y, P, eig, d = LC.loop_problem(case)
    r0 = np.conj(np.transpose(P, (0, 2, 1))) @ Y / eig[:, None, None]
    print('max|r| at unroll 0: %.2e; eps %s' % (np.abs(r0).max(), r64['eps'][:, 0]))
    if case.floor:
        for k in range(LC.UNROLLS):                                   # the floor branch at EVERY unroll, in both precisions
            assert np.all(r64['eps'][k] == LC.EPS_FLOOR) and np.all(r32['eps'][k] == np.float32(LC.EPS_FLOOR)), k
            assert np.all(r32f['eps'][k] == np.float32(LC.EPS_FLOOR)), k
        assert np.abs(r0).max() < 1e-2
    else:
        assert np.all(r64['eps'] > 2 * LC.EPS_FLOOR)
    if case.name == 'y_2m20':
        assert np.abs(r0).max() < LC.EPS_FLOOR                        # |eps d| ~ eps: the perturbation is larger than r itself
    res = []
    for k in range(LC.UNROLLS):
        res.append(LC.mutual('%s unroll %d h' % (case.name, k), r64['h'][k], r32['h'][k], r32f['h'][k]))
        res.append(LC.mutual('%s unroll %d z' % (case.name, k), r64['z'][k], r32['z'][k], r32f['z'][k]))
        res.append(LC.mutual('%s unroll %d div' % (case.name, k), r64['div'][k], r32['div'][k], r32f['div'][k], 'abs'))
        res.append(LC.mutual('%s unroll %d eps' % (case.name, k), r64['eps'][k], r32['eps'][k], r32f['eps'][k], 'abs'))
    LC.assert_all(res)
    sd, fsd = LC.weights(case.weights, LC.UNROLLS)
    _twin_is_the_identity_in_float64(sd, fsd, 0, r0.astype(np.complex64))


def test_the_mixed_batch_is_one_sample_of_each_regime():
    Y, P, eig, d = LC.mixed_problem()
    assert Y.shape == (4, 38, 16) and d.shape == (3, 4, 64, 16, 2)
    for i, c in enumerate(LC.MIXED):
        Yc, Pc, eigc, dc = LC.loop_problem(c)
        assert np.array_equal(Y[i], Yc[i]) and np.array_equal(P[i], Pc[i]) and eig[i] == eigc[i] and np.array_equal(d, dc)
    amp = np.abs(Y).max(axis=(1, 2))
    assert amp[1] < 1e-4 * amp[0] and amp[2] > 1e3 * amp[0]
