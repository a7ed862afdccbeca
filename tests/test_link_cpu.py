"""Host side of the coded link simulation (no GPU): the code construction and the two numpy restatements (tests/link_oracle.py) on the
inputs of the GPU tests (tests/link_cases.py), the host-side refusals of link.py, the test_end_to_end CLI around a stubbed simulator,
and the sbc_link_ part of the C ABI."""
import os
import re

import numpy as np
import pytest

import link_cases as K
import link_oracle as O
from conftest import ROOT


# ---- the code --------------------------------------------------------------------------------------------------------------------
def test_reference_code_structure():
    from score_based_channels_amd import link
    H = K.code('ref')[0]
    assert H.shape == (324, 648) and H.sum() == 2376 and (O.REF_BASE > -1).sum() == 88
    assert H.sum(axis=1).max() <= 8 and H.sum(axis=0).max() <= 12
    c = link.ldpc_11n_648()
    assert (c.M, c.N, c.K) == (324, 648, 324) and np.array_equal(c.parity_check_matrix(), H)
    assert np.array_equal(c.base, O.REF_BASE) and c.uses(4) == (81, 0) and c.uses(2) == (162, 0)
    # circshift(eye(Z), [0 s]): row i's one in column (i + s) mod Z  (block (1, 0) has shift 22)
    assert H[27 + 3, (3 + 22) % 27] == 1 and H[27:54, :27].sum() == 27
    small = K.code('small')[0]
    assert sorted(set(small.sum(axis=1))) == [3, 4] and not np.triu(small[:, 15:], 1).any()


def test_codes_of_the_shape_tests_and_their_codewords_per_decoder_workgroup():
    """The decoder's LDS formula (decode_lds_bytes in csrc/link.hip) restated against the budget and the largest count read from the
    source: a change of either fails here instead of silently moving every code to another count."""
    src = open(os.path.join(ROOT, 'score_based_channels_amd', 'csrc', 'link.hip')).read()
    budget = re.search(r'constexpr size_t LINK_LDS_BUDGET = (\d+) \* 1024;', src)
    max_cw = int(re.search(r'constexpr int LINK_MAX_CW = (\d+);', src).group(1))
    budget = int(budget.group(1)) * 1024
    assert 'return ((size_t)ncw * (t.E + 2 * t.N) + 32) * 4 + ((size_t)(t.M + 2) + (t.N + 2) + 2 * (size_t)t.E) * 2;' in src

    def ncw(base, Z):
        H = O.parity_check(base, Z)
        (M, N), E = H.shape, int(H.sum())
        fits = [n for n in range(1, max_cw + 1) if (n * (E + 2 * N) + 32) * 4 + ((M + 2) + (N + 2) + 2 * E) * 2 <= budget]
        return max(fits) if fits else 0
    codes = dict(K.BASE_CODES, **K.SHAPE_CODES)
    for name, (base, Z, want) in codes.items():
        assert ncw(base, Z) == want, name
    assert {c[2] for c in codes.values()} == set(range(1, 9)) and max_cw == 8
    assert ncw(O.REF_BASE, 77) == 0                                          # SBC_ERR_UNSUPPORTED: "does not fit"
    sizes = {n: (K.code(n)[0].shape[1], K.code(n)[0].shape[1] - K.code(n)[0].shape[0]) for n in K.SHAPE_CODES}
    assert sizes == {'mixed': (56, 28), 'ref32': (768, 384), 'ref40': (960, 480), 'ref56': (1344, 672), 'small93': (558, 279),
                     'small105': (630, 315), 'small120': (720, 360)}
    mixed = K.code('mixed')[0]
    assert sorted(set(mixed.sum(axis=1))) == [2, 5, 6, 7] and sorted(set(mixed.sum(axis=0))) == [1, 2, 3, 4]
    assert not np.triu(mixed[:, 28:], 1).any() and np.all(np.diag(mixed[:, 28:]) == 1)


@pytest.mark.parametrize('name', ['ref', 'small', 'small10'] + sorted(K.SHAPE_CODES))
def test_encoded_payloads_satisfy_every_check(name):
    H, P, _, _ = K.code(name)
    payload = np.random.default_rng(3).integers(0, 2, (50, H.shape[1] - H.shape[0]))
    cw = O.encode(H, payload)
    assert np.array_equal(cw[:, :payload.shape[1]], payload) and not (H.astype(np.int64) @ cw.T % 2).any()
    R = O.inverse_permutation(P)
    assert np.array_equal(R[P], np.arange(len(P))) and np.array_equal(P[R], np.arange(len(P)))
    x = np.arange(len(P)) * 1.5
    assert np.array_equal(x[P][R], x)                                        # llr(R) undoes bitsEnc(P)


def test_link_module_interleaver_is_the_cases_interleaver():
    from score_based_channels_amd import link
    c = link.Code(O.SMALL_BASE, O.SMALL_Z, K.INTERLEAVER_SEED)
    assert np.array_equal(c.P, K.code('small')[1]) and np.array_equal(c.R[c.P], np.arange(c.N))
    assert c.uses(2) == (7, 2) and c.uses(4) == (3, 6)


# ---- the two restatements agree, and the yardstick is finite on every input of the GPU tests ------------------------------------
def test_tanh_product_in_float32_is_not_usable():
    """Why the kernels use the pairwise form: tanh rounds to 1 in fp32, atanh(1) = inf, inf - inf = NaN."""
    g = K.graph('ref')
    llr = K.decoder_inputs('ref')[2.0][0][:20].astype(np.float32)
    m = llr[:, g.evar]
    padded = np.concatenate([m, np.full((len(m), 1), np.inf, np.float32)], axis=1)[:, g.cidx]
    for _ in range(8):
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            t = np.tanh(padded / np.float32(2))
            prod = np.prod(t, axis=-1, keepdims=True)
            ext = np.float32(2) * np.arctanh((prod / t).astype(np.float32))
        if not np.isfinite(ext[padded != np.inf]).all():
            return
        padded = np.where(padded == np.inf, padded, ext * np.float32(3))     # grow like the totals do over the iterations
    pytest.fail('the fp32 tanh / atanh product stayed finite')


@pytest.mark.parametrize('name', ['ref', 'small'])
def test_fixed_iteration_restatements_agree(name):
    bounds = {1: 1e-5, 3: 2e-5, 8: 1e-4}            # measured on the reference code: 2.4e-6, 5.5e-6, 1.2e-5 on totals up to 17, 26, 77
    for it in K.FIXED_ITERS:
        t64, t32 = K.fixed_iteration_totals(name, it, 'float64'), K.fixed_iteration_totals(name, it, 'float32')
        assert np.isfinite(t64).all() and np.isfinite(t32).all()
        assert 0 < np.max(np.abs(t64 - t32)) < bounds[it] * max(1.0, np.max(np.abs(t64)) / 20)


def test_full_decoder_restatements_agree_on_all_600_codewords():
    stuck = 0
    for snr in K.DECODER_SNRS:
        (t64, i64), (t32, i32) = K.full_decode('ref', snr, 'float64'), K.full_decode('ref', snr, 'float32')
        assert np.isfinite(t64).all()
        differ = (i64 != i32) | ((t64 < 0) != (t32 < 0)).any(axis=1)
        assert np.mean(differ) <= 0.02
        stuck += int((i64 == 50).sum())
    assert stuck == 94                                                       # 79 + 13 + 2: the GPU tests' "never converges" case exists


def _boxplus_before_the_pad_fix(a, b):
    """The pairwise form as it stood while a pad was an ordinary operand (inf [+] inf = NaN)."""
    t = a.dtype.type
    return (np.sign(a) * np.sign(b) * np.minimum(np.abs(a), np.abs(b)) + np.log1p(np.exp(-np.abs(a + b)))
            - np.log1p(np.exp(-np.abs(a - b)))).astype(t)


def test_pads_as_neutral_elements_move_no_float32_result_of_the_earlier_codes(monkeypatch):
    """'ref' and 'small' have checks at most one edge short of the largest degree, where the formula itself returns the other operand:
    every float32 total and iteration count is what the earlier recursion gives, computed here with the earlier form.  On 'mixed'
    (degrees 2, 5, 6, 7) the earlier form is NaN after one iteration and the present one is not."""
    now = {(n, it): K.fixed_iteration_totals(n, it, 'float32') for n in ('ref', 'small') for it in K.FIXED_ITERS}
    full = {(n, snr): K.full_decode(n, snr, 'float32') for n in ('ref', 'small') for snr in K.DECODER_SNRS}
    mixed = K.fixed_iteration_totals('mixed', 1, 'float32')
    monkeypatch.setattr(O, 'boxplus', _boxplus_before_the_pad_fix)
    for (n, it), t in now.items():
        assert np.array_equal(O.decode(K.graph(n), K.fixed_iteration_inputs(n), it, False, np.float32)[0], t), (n, it)
    for (n, snr), (t, i) in full.items():
        with np.errstate(invalid='ignore'):
            t0, i0 = O.decode(K.graph(n), K.decoder_inputs(n)[snr][0], 50, True, np.float32)
        assert np.array_equal(t0, t) and np.array_equal(i0, i), (n, snr)
    with np.errstate(invalid='ignore'):
        before = O.decode(K.graph('mixed'), K.fixed_iteration_inputs('mixed'), 1, False, np.float32)[0]
    assert np.isnan(before).any() and np.isfinite(mixed).all()
    assert np.isfinite(K.fixed_iteration_totals('mixed', 1, 'float64')).all()


@pytest.mark.parametrize('name', sorted(K.SHAPE_CODES))
def test_fixed_iteration_restatements_agree_on_the_codes_of_the_shape_tests(name):
    """The bounds of the two earlier codes; measured here 1.5e-6 .. 1.7e-5 on totals up to 115."""
    bounds = {1: 1e-5, 3: 2e-5, 8: 1e-4}
    assert K.fixed_iteration_inputs(name).shape == (K.SHAPE_CODEWORDS, K.code(name)[0].shape[1])
    for it in K.FIXED_ITERS:
        t64, t32 = K.fixed_iteration_totals(name, it, 'float64'), K.fixed_iteration_totals(name, it, 'float32')
        assert np.isfinite(t64).all() and np.isfinite(t32).all()
        assert 0 < np.max(np.abs(t64 - t32)) < bounds[it] * max(1.0, np.max(np.abs(t64)) / 20)


def test_full_decoder_restatements_agree_on_the_mixed_code_and_the_scaled_codes():
    """The condition of the GPU tests' decision checks -- the restatements may disagree on at most 2 % of the codewords -- on the 600
    'mixed' codewords at 1, 3, 5 dB, on 48 codewords at 1.5 dB of each scaled code, and on the batches whose codewords stop at
    different times."""
    stuck = {}
    for snr in K.MIXED_SNRS:
        (t64, i64), (t32, i32) = K.full_decode('mixed', snr, 'float64'), K.full_decode('mixed', snr, 'float32')
        assert np.isfinite(t64).all() and np.isfinite(t32).all()
        assert np.mean((i64 != i32) | ((t64 < 0) != (t32 < 0)).any(axis=1)) <= 0.02
        stuck[snr] = int((i64 == 50).sum())
    assert stuck[1.0] >= 20 and stuck[5.0] < stuck[1.0], stuck               # "never converges" exists on this code, and SNR helps
    for name in sorted(K.SHAPE_CODES):
        if name == 'mixed':
            continue
        llr = O.bpsk_awgn_llrs(K.code(name)[0], 1.5, 48, np.random.default_rng(4))[0]
        (t64, i64), (t32, i32) = (O.decode(K.graph(name), llr, 50, True, t) for t in (np.float64, np.float32))
        assert np.isfinite(t64).all()
        assert np.mean((i64 != i32) | ((t64 < 0) != (t32 < 0)).any(axis=1)) <= 0.02, name
    for name, groups in K.STAGGERED_GROUPS.items():
        ncw = K.SHAPE_CODES[name][2]
        (t64, i64), (t32, i32) = K.staggered_decode(name, 'float64'), K.staggered_decode(name, 'float32')
        assert len(i64) == groups * ncw and np.isfinite(t64).all()
        assert np.mean((i64 != i32) | ((t64 < 0) != (t32 < 0)).any(axis=1)) <= 0.02, name
        per_group = i64.reshape(groups, ncw)
        # every workgroup: 1, 1 and a slot that runs on; in the batch: codewords that never converge and ones that do, later than 1
        assert np.all(per_group[:, :2] == 1) and np.all((per_group[:, 2:] > 1).any(axis=1)), per_group
        assert (per_group == 50).sum() >= groups // 2 and ((per_group > 1) & (per_group < 50)).sum() >= groups // 2, per_group


@pytest.mark.parametrize('S', [2, 4])
def test_soft_bit_batches_of_the_shape_tests(S):
    """The three-packet cases (an index outside the pool in the GPU test) and the reference code at S = 2 without a padded tail."""
    cases = [('small' if S == 2 else 'small10', S, 3, 3)] + ([('ref', 2, 5, 3)] if S == 2 else [])
    for name, S_, Nr, n in cases:
        c = K.llr_batch(name, S_, Nr, n)
        r64, r32 = K.llr_batch_oracle(name, S_, Nr, n, np.float64), K.llr_batch_oracle(name, S_, Nr, n, np.float32)
        for k in (0, 1):
            assert r64[k].shape == (n, c['H'].shape[1]) and np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all()
            assert 0 < np.max(np.abs(r64[k] - r32[k])) < 1e-5 * max(1.0, np.max(np.abs(r64[k])))
    assert K.llr_batch('ref', 2, 5, 3)['sym'].shape == (3, 162, 2) and 162 * 4 == 648


@pytest.mark.parametrize('geometry', K.SIM_GEOMETRIES, ids=lambda g: '%s-S%d-Nr%d-pool%d' % g[:4])
def test_chain_restatements_agree_at_the_other_geometries(geometry):
    name, S, Nr, pool, npow = geometry
    r64, r32 = K.sim_oracle(name, S, Nr, pool, npow, 'float64'), K.sim_oracle(name, S, Nr, pool, npow, 'float32')
    assert all(np.isfinite(r64[rx]['llr']).all() for rx in ('ideal', 'est'))
    assert np.mean(~K.same_packets(r64, r32)) <= 0.02
    assert 0.2 <= r64['ideal']['bler'].mean() <= 0.8
    idx = K.sim_draws(name, S, Nr, pool)[1]
    assert idx.shape == (K.SIM_PACKETS, 7) and idx.min() >= 0 and idx.max() < pool
    assert (pool >= 7) == all(len(set(r)) == 7 for r in idx)


@pytest.mark.parametrize('S', [2, 4])
@pytest.mark.parametrize('Nr', [1, 3, 16, 17, 33, 64])
def test_soft_bit_restatements_agree_and_the_yardstick_is_finite(S, Nr):
    for kind in K.LLR_NOISE_KINDS:
        r64, r32 = K.llr_oracle(S, Nr, kind, np.float64), K.llr_oracle(S, Nr, kind, np.float32)
        for k in (0, 1):
            assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all()
            assert np.max(np.abs(r64[k] - r32[k])) < 1e-5 * max(1.0, r64[2])
        if kind == 'large-ratio':
            assert 100 < r64[2] < 700, r64[2]       # fp32 exp(-x) of the raw metrics is 0 here, float64's is not
    c = K.llr_case(S, Nr, '63')
    assert c['sym'].shape == (1, 7, S) and c['H'].shape[1] - 7 * 2 * S > 0


@pytest.mark.parametrize('pool', [100, 20])
def test_chain_restatements_agree_and_the_snr_points_are_where_the_cases_say(pool):
    for si in (0, 1):
        r64, r32 = K.chain_oracle(pool, si, np.float64), K.chain_oracle(pool, si, np.float32)
        assert all(np.isfinite(r64[rx]['llr']).all() and np.abs(r64[rx]['llr']).max() <= 6 for rx in ('ideal', 'est'))
        assert np.mean(~K.same_packets(r64, r32)) <= 0.02
        bler = r64['ideal']['bler'].mean()
        assert (0.2 <= bler <= 0.8) if si == 0 else bler < 0.05, bler
    idx = K.host_randomness(pool, 0)[1]
    assert (pool >= 81) == all(len(set(r)) == 81 for r in idx)


# ---- host replay of the device streams -------------------------------------------------------------------------------------------
def test_host_replay_streams_are_keyed_by_packet_not_by_chunk():
    from oracle import ald_oracle
    from score_based_channels_amd import noise as N
    ctr = np.arange(40, dtype=np.uint32).reshape(10, 4)
    assert np.array_equal(N.philox4x32(ctr, 0x123456789ABCDEF0), ald_oracle.philox4x32(ctr, np.array([0x9ABCDEF0, 0x12345678], np.uint32)))
    a = N.link_payload(9, 2, np.arange(10), 324)
    assert np.array_equal(a[4:7], N.link_payload(9, 2, np.arange(4, 7), 324)) and set(np.unique(a)) == {0, 1}
    assert not np.array_equal(a, N.link_payload(9, 3, np.arange(10), 324))
    i = N.link_indices(9, 2, np.arange(10), 81, 100)
    assert np.array_equal(i[4:7], N.link_indices(9, 2, np.arange(4, 7), 81, 100)) and all(len(set(r)) == 81 for r in i)
    assert N.link_indices(9, 2, np.arange(3), 81, 81).shape == (3, 81)       # pool == uses: a full permutation, needs more draws
    j = N.link_indices(9, 2, np.arange(10), 81, 20)
    assert j.min() >= 0 and j.max() < 20
    w = N.link_noise(9, 2, np.arange(4), 81, 3)
    assert w.shape == (4, 81, 3) and w.dtype == np.complex64
    assert np.array_equal(w[2], ald_oracle.device_complex_normal(9, 2, 4 * 2 + N.LINK_NOISE, 81 * 3).reshape(81, 3))


# ---- refusals on the host --------------------------------------------------------------------------------------------------------
def test_host_refusals():
    from score_based_channels_amd import link
    code = link.Code(O.SMALL_BASE, O.SMALL_Z)
    with pytest.raises(ValueError, match='num_streams'):
        link.check_streams(8)
    with pytest.raises(ValueError, match='QPSK'):
        link.check_streams(4, mod_size=4)
    with pytest.raises(ValueError, match='singular'):
        link.Code(np.array([[0, 0, 0, 0], [1, 2, 0, 0]]), 5)                 # two equal parity block columns
    with pytest.raises(ValueError, match='check degrees'):
        link.Code(np.zeros((1, 10), np.int64), 3)
    with pytest.raises(ValueError, match='shifts'):
        link.Code(np.array([[0, 5, 0]]), 5)
    with pytest.raises(ValueError, match='code bits'):
        link.Code(np.zeros((2, 24), np.int64), 400)
    ok = dict(sym_shape=(5, 7, 2), Hp_ideal_shape=(9, 3, 2), Hp_est_shape=(9, 3, 2), idx_shape=(5, 7), noise_shape=(5, 7, 3), noise_power=1.0)
    link.check_llr_args(code, **ok)
    for bad, what in ((dict(Hp_ideal_shape=(9, 3, 8), Hp_est_shape=(9, 3, 8)), 'num_streams'), (dict(Hp_est_shape=(9, 4, 2)), 'Hp_ideal and Hp_est'),
                      (dict(Hp_ideal_shape=(0, 3, 2), Hp_est_shape=(0, 3, 2)), 'at least one channel'),
                      (dict(Hp_ideal_shape=(9, 65, 2), Hp_est_shape=(9, 65, 2)), 'Nr must'), (dict(sym_shape=(5, 6, 2)), 'symbols must'),
                      (dict(idx_shape=(5, 8)), 'chan_index must'), (dict(noise_shape=(5, 7, 4)), 'noise must'), (dict(noise_power=0.0), 'noise_power')):
        with pytest.raises(ValueError, match=what):
            link.check_llr_args(code, **dict(ok, **bad))
    args = dict(real_shape=(64, 16, 10), est_shape=(3, 64, 16, 10), mod_size=2, num_tx=16, num_rx=64, precoding='random', num_streams=4,
                num_packets=10, n_snr=3)
    link.check_packets_args(**args)
    for bad, what in ((dict(num_streams=8), 'num_streams'), (dict(mod_size=4), 'QPSK'), (dict(precoding='svd'), 'precoding'),
                      (dict(real_shape=(64, 16, 0), est_shape=(3, 64, 16, 0)), 'at least one channel'), (dict(est_shape=(2, 64, 16, 10)), 'est_channels'),
                      (dict(real_shape=(16, 64, 10)), 'real_channels'), (dict(num_packets=0), 'num_packets'),
                      (dict(real_shape=(65, 16, 10), est_shape=(3, 65, 16, 10), num_rx=65), 'num_rx')):
        with pytest.raises(ValueError, match=what):
            link.check_packets_args(**dict(args, **bad))


# ---- the CLI around a stubbed simulator ------------------------------------------------------------------------------------------
def test_cli_defaults_are_the_scripts():
    from score_based_channels_amd import test_end_to_end as T
    a = T.parse_args([])
    assert np.allclose(a.channel_snr_range, np.arange(-10, 15.1, 2.5)) and a.precoding_offset == 20
    assert np.allclose(a.snr_range, np.arange(-10, 2.1, 0.5) - 20) and len(a.snr_range) == 25
    assert (a.num_packets, a.mod_size, a.num_streams, a.target_alpha, a.noise, a.gpu) == (100000, 2, 4, 0, 'device', 0)
    assert T.result_path(a) == os.path.join('./e2e_results', 'ours_known_alpha1.00.pt')
    # :38-43: data SNR + offset against the channel SNR grid; a tie goes to the first, as MATLAB's min
    near = T.nearest_channel_snr(a.snr_range, 20, a.channel_snr_range)
    assert near[0] == 0 and near[-1] == 5 and list(near[:4]) == [0, 0, 0, 1] and np.all(np.diff(near) >= 0)
    assert T.nearest_channel_snr([-18.75], 20, [0.0, 2.5])[0] == 0


def _stub_simulator(monkeypatch, seen):
    import torch
    from score_based_channels_amd import link

    def fake(real, est, mod_size, num_tx, num_rx, precoding, num_streams, num_packets, snr_range, run_ideal=True, **kw):
        seen.update(real=np.asarray(real), est=np.asarray(est), num_tx=num_tx, num_rx=num_rx, snr_range=np.asarray(snr_range), kw=kw,
                    num_packets=num_packets, precoding=precoding)
        n = len(snr_range)
        return np.zeros(n), np.zeros(n), np.ones(n), np.full(n, 0.5)
    monkeypatch.setattr(link, 'simulate_packets', fake)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'device_count', lambda: 1)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)

    class _NoDevice:
        def __init__(self, *a):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False
    monkeypatch.setattr(torch.cuda, 'device', _NoDevice)


def test_cli_reads_both_file_layouts(tmp_path, monkeypatch):
    import torch
    from score_based_channels_amd import test_end_to_end as T
    rng = np.random.default_rng(0)
    B, d1, d2 = 5, 6, 3
    ideal = (rng.standard_normal((B, d1, d2)) + 1j * rng.standard_normal((B, d1, d2))).astype(np.complex64)
    # the script's file: est_H [alpha, channel SNR, B, d1, d2] on the default grid of 11 channel SNRs; entry (a, s) = ideal + (10 a + s)
    est = np.stack([np.stack([ideal + (10 * a + s) for s in range(11)]) for a in range(3)]).astype(np.complex64)
    np.savez(tmp_path / 'script.npz', ideal_H=ideal, est_H=est)
    seen = {}
    _stub_simulator(monkeypatch, seen)
    out = T.main(['--channels', str(tmp_path / 'script.npz'), '--num_packets', '7', '--snr_range', '-30', '-24.9', '-18', '--target_alpha', '1',
                  '--out_dir', str(tmp_path / 'res'), '--noise', 'host', '--seed', '5'])
    assert seen['real'].shape == (d1, d2, B) and np.array_equal(seen['real'], np.conj(np.transpose(ideal, (1, 2, 0))))      # conj(permute(., [2 3 1]))
    assert seen['est'].shape == (3, d1, d2, B) and (seen['num_rx'], seen['num_tx'], seen['num_packets']) == (d1, d2, 7)
    # -30 + 20 -> channel SNR -10 (index 0), -24.9 + 20 = -4.9 -> -5 (index 2), -18 + 20 -> 2.5 (index 5); alpha index 1
    for i, s in enumerate((0, 2, 5)):
        assert np.allclose(seen['est'][i], np.conj(np.transpose(ideal + (10 + s), (1, 2, 0))))
    assert seen['kw']['noise'] == 'host' and seen['kw']['seed'] == 5 and seen['precoding'] == 'random'
    saved = torch.load(str(tmp_path / 'res' / 'ours_known_alpha0.80.pt'), weights_only=False)
    assert set(saved) == {'bler_ideal', 'ber_ideal', 'bler_est', 'ber_est', 'target_alpha', 'snr_range', 'alpha_array', 'precoding_offset', 'seed'}
    assert np.array_equal(saved['bler_est'], out['bler_est']) and list(saved['alpha_array']) == [1, 0.8, 0.6]
    # the l1 layout: permute(., [3 2 1]) and permute(., [1 4 3 2]), no conjugate
    T.main(['--channels', str(tmp_path / 'script.npz'), '--layout', 'l1', '--snr_range', '-30', '--out_dir', str(tmp_path / 'res')])
    assert np.array_equal(seen['real'], np.transpose(ideal, (2, 1, 0))) and np.array_equal(seen['est'][0], np.transpose(est[0, 0], (2, 1, 0)))
    # the file test_mmse writes: oracle_H, mmse_H [spacing, alpha, SNR, B, d1, d2] and its own snr_range as the channel SNR grid
    grid = np.arange(-30, 17.5, 2.5)
    mm = np.stack([np.stack([ideal + s for s in range(len(grid))])])[None].astype(np.complex64)
    torch.save({'oracle_H': ideal, 'mmse_H': mm, 'saved_H': mm[:, :, :, :, None], 'snr_range': grid}, str(tmp_path / 'mmse.pt'))
    T.main(['--channels', str(tmp_path / 'mmse.pt'), '--snr_range', '-30', '-20', '--out_dir', str(tmp_path / 'res')])
    assert np.allclose(seen['est'][0], np.conj(np.transpose(ideal + 8, (1, 2, 0))))      # -30 + 20 = -10 dB is entry 8 of -30:2.5:15
    assert np.allclose(seen['est'][1], np.conj(np.transpose(ideal + 12, (1, 2, 0))))
    with pytest.raises(ValueError, match='neither'):
        np.savez(tmp_path / 'bad.npz', H=ideal)
        T.main(['--channels', str(tmp_path / 'bad.npz')])
    with pytest.raises(ValueError, match='num_streams'):
        T.main(['--synthetic', '--num_streams', '8'])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_link_symbols_of_header_and_exports():
    from score_based_channels_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'sbc_hip.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t|void|const char\*)\s+(sbc_link_\w+)\s*\(', header, re.M))
    assert declared == {n for n in _lib.EXPORTS if n.startswith('sbc_link_')} == {
        'sbc_link_code_create', 'sbc_link_code_destroy', 'sbc_link_encode', 'sbc_link_llr', 'sbc_link_decode', 'sbc_link_errors', 'sbc_link_simulate'}
    h = _lib.lib()
    assert all(hasattr(h, n) for n in declared) and h.sbc_abi_version() == 16
    assert '#define SBC_LINK_DEVICE_RANDOM %d' % _lib.LINK_DEVICE_RANDOM in header and '#define SBC_LINK_NO_CLIP %d' % _lib.LINK_NO_CLIP in header
    # the ctypes records follow the header's structs field by field
    for rec in (_lib.sbc_link_code_desc, _lib.sbc_link_random, _lib.sbc_link_encode_desc, _lib.sbc_link_llr_desc, _lib.sbc_link_sim_desc):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (rec.__name__, rec.__name__), header, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        names = [n for decl in body.split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', decl.strip().replace('*', ' '))]
        assert names == [f[0] for f in rec._fields_], (rec.__name__, names)
