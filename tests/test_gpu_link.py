"""The coded link simulation on the GPU (csrc/link.hip through the sbc_link_* calls, link.py and the test_end_to_end CLI) against the
numpy restatement of the reference's MATLAB scripts (tests/link_oracle.py) on the inputs of tests/link_cases.py.  float64 (tanh /
atanh decoder, plain exp sums) is the yardstick; the float32 restatement (pairwise check-node form, log-sum-exp) gives the bound: the
kernels stay within 4x its own distance from float64, and decide like float64 wherever it does.  Every launch runs on guarded
operands (tests/guarded.py; the launches themselves are in tests/link_gpu.py)."""
import numpy as np
import pytest
import torch

import link_cases as K
import link_oracle as O
from link_gpu import _code, gpu_decode, gpu_encode, gpu_errors, gpu_llr, gpu_simulate

pytestmark = pytest.mark.gpu


# ---- 1. encoder ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,S', [('ref', 4), ('ref', 2), ('small', 2), ('small10', 4)])
def test_encoder_equals_the_restatement_bit_for_bit(name, S):
    H, P, _, _ = K.code(name)
    payload = np.random.default_rng(11).integers(0, 2, (64, H.shape[1] - H.shape[0]))
    cw, sym = gpu_encode(name, payload, S)
    ref = O.encode(H, payload)
    assert not (H.astype(np.int64) @ ref.T % 2).any()
    assert np.array_equal(cw, ref)
    assert np.array_equal(sym, O.modulate(ref, P, S).astype(np.complex64))


# ---- 2. soft bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', K.LLR_NOISE_KINDS)
@pytest.mark.parametrize('Nr', [1, 3, 16, 17, 33, 64])
@pytest.mark.parametrize('S', [2, 4])
def test_unclipped_soft_bits_within_four_times_the_float32_restatement(S, Nr, kind):
    """The third noise power puts metric / noise_power ratios above 100: without the subtraction of the smallest metric every fp32
    exp(-x) there is 0 and the soft bit 0 / 0."""
    c = K.llr_case(S, Nr, kind)
    r64, r32 = K.llr_oracle(S, Nr, kind, np.float64), K.llr_oracle(S, Nr, kind, np.float32)
    assert np.isfinite(r64[0]).all() and np.isfinite(r64[1]).all()
    got = gpu_llr(c['name'], c['sym'], c['Hp'], c['Hp_est'], c['idx'], c['w'], c['noise_power'], clip=False)
    e_ref = max(np.max(np.abs(r32[k] - r64[k])) for k in (0, 1))
    e_gpu = max(np.max(np.abs(got[k][0] - r64[k])) for k in (0, 1))
    print('llr S=%d Nr=%d noise %s: kernel %.3e  float32 restatement %.3e  ratio %.2f  largest |llr| %.1f  metric/noise %.0f'
          % (S, Nr, kind, e_gpu, e_ref, e_gpu / e_ref, np.max(np.abs(r64[0])), r64[2]))
    assert e_gpu <= 4 * e_ref, (e_gpu, e_ref)
    # clipping and deinterleaving, exactly: the clipped launch is the clip of the unclipped one, the padded tail is 0 at P[tail]
    clipped = gpu_llr(c['name'], c['sym'], c['Hp'], c['Hp_est'], c['idx'], c['w'], c['noise_power'], clip=True)
    N, uses = c['H'].shape[1], c['sym'].shape[1]
    for k in (0, 1):
        want = got[k].copy()
        big = np.abs(want) >= O.CLIP
        want[big] = O.CLIP * np.sign(want[big])
        assert np.array_equal(clipped[k], want)
        assert np.all(got[k][0][c['P'][uses * 2 * S:]] == 0) and len(c['P'][uses * 2 * S:]) == N - uses * 2 * S > 0


# ---- 3. decoder, fixed iteration counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('iters', K.FIXED_ITERS)
@pytest.mark.parametrize('name', ['ref', 'small'])
def test_decoder_totals_after_fixed_iterations(name, iters):
    llr = K.fixed_iteration_inputs(name)
    t64, t32 = K.fixed_iteration_totals(name, iters, 'float64'), K.fixed_iteration_totals(name, iters, 'float32')
    assert np.isfinite(t64).all()
    soft, totals, its = gpu_decode(name, llr, iters, False)
    e_ref, e_gpu = np.max(np.abs(t32 - t64)), np.max(np.abs(totals - t64))
    print('decoder %s %d iterations: kernel %.3e  float32 restatement %.3e  ratio %.2f  largest total %.1f'
          % (name, iters, e_gpu, e_ref, e_gpu / e_ref, np.max(np.abs(t64))))
    assert e_gpu <= 4 * e_ref, (e_gpu, e_ref)
    assert np.array_equal(soft, totals[:, :soft.shape[1]]) and np.all(its == iters)


# ---- 4. decoder, 50 iterations with early stop -----------------------------------------------------------------------------------
@pytest.mark.parametrize('snr', K.DECODER_SNRS)
def test_full_decoder_decides_like_float64(snr):
    llr, payload = K.decoder_inputs('ref')[snr]
    (t64, i64), (t32, i32) = K.full_decode('ref', snr, 'float64'), K.full_decode('ref', snr, 'float32')
    same = (i64 == i32) & ((t64 < 0) == (t32 < 0)).all(axis=1)
    assert np.mean(~same) <= 0.02
    soft, totals, its = gpu_decode('ref', llr, 50, True)
    bad = same & ((its != i64) | ((totals < 0) != (t64 < 0)).any(axis=1))
    print('full decoder %.1f dB: %d of %d never converge, restatement differs on %d, kernel on %d' % (snr, (i64 == 50).sum(), len(llr), (~same).sum(), bad.sum()))
    assert not bad.any(), np.nonzero(bad)[0]
    # errors of the payload bits, as the script counts them
    ber, bler = gpu_errors('ref', soft, payload)
    rber, rbler = O.packet_errors(t64[:, :payload.shape[1]], payload)
    assert np.array_equal(ber[same], rber[same].astype(np.float32)) and np.array_equal(bler[same], rbler[same].astype(np.float32))


def test_decoder_edge_cases():
    H, _, _, _ = K.code('ref')
    N, Kb = H.shape[1], H.shape[1] - H.shape[0]
    cw = O.encode(H, np.random.default_rng(5).integers(0, 2, (1, Kb)))
    noiseless = O.CLIP * (1.0 - 2.0 * cw)
    llrs, pay = K.decoder_inputs('ref')[1.0]
    stuck = int(np.nonzero(K.full_decode('ref', 1.0, 'float64')[1] == 50)[0][0])
    batch = np.concatenate([noiseless, np.zeros((1, N)), llrs[stuck:stuck + 1]])
    soft, totals, its = gpu_decode('ref', batch, 50, True)
    assert its[0] == 1 and np.array_equal(totals[0] < 0, cw[0] == 1)          # a noiseless +-6 codeword stops after 1 iteration
    assert np.all(totals[1] == 0) and np.all(soft[1] == 0) and its[1] == 1    # all-zero LLRs: all-zero outputs ...
    ber, bler = gpu_errors('ref', soft, np.concatenate([cw[:, :Kb], np.zeros((1, Kb), np.uint8), pay[stuck:stuck + 1]]))
    assert ber[0] == 0 and bler[0] == 0
    assert ber[1] == 1 and bler[1] == 1                                       # ... and every payload bit counts as wrong (0.5 != bit)
    assert its[2] == 50                                                       # a codeword that never converges runs 50 iterations


# ---- 5. batch independence -------------------------------------------------------------------------------------------------------
def test_a_packet_is_bit_identical_whatever_the_batch_and_its_position():
    Hp, Hp_est = K.chain_pool(100)
    payload, idx, w = K.host_randomness(100, 0)
    H, P, _, _ = K.code('ref')
    sym = O.modulate(O.encode(H, payload), P, K.CHAIN_S).astype(np.complex64)
    npow = 10 ** (-K.CHAIN_SNRS[0] / 10)
    rows = {}
    for n, pos in ((1, 0), (3, 2), (257, 256)):
        order = np.array([(j + 1) % 64 for j in range(n)])
        order[pos] = 0                                                       # packet 0 at position pos, other packets around it
        li, le = gpu_llr('ref', sym[order], Hp, Hp_est, idx[order], w[order], npow)
        dec = [gpu_decode('ref', l, 50, True) for l in (li, le)]
        rows[n] = [li[pos], le[pos]] + [a[pos] for d in dec for a in d]
    for n in (3, 257):
        for a, b in zip(rows[1], rows[n]):
            assert np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32)), n


# ---- 6. whole chain, host randomness ---------------------------------------------------------------------------------------------
def _check_chain(got, pool, snr_index, randomness=None):
    r64, r32 = K.chain_oracle(pool, snr_index, np.float64, randomness), K.chain_oracle(pool, snr_index, np.float32, randomness)
    assert all(np.isfinite(r64[rx]['llr']).all() for rx in ('ideal', 'est'))
    same = K.same_packets(r64, r32)
    assert np.mean(~same) <= 0.02
    bad = np.zeros(len(same), bool)
    for rx in ('ideal', 'est'):
        bad |= (got['ber_' + rx] != r64[rx]['ber'].astype(np.float32)) | (got['bler_' + rx] != r64[rx]['bler'].astype(np.float32))
    print('chain pool %d at %.1f dB: BLER ideal %.3f est %.3f; restatement differs on %d packets, kernel on %d of the others'
          % (pool, K.CHAIN_SNRS[snr_index], r64['ideal']['bler'].mean(), r64['est']['bler'].mean(), (~same).sum(), (bad & same).sum()))
    assert not (bad & same).any(), np.nonzero(bad & same)[0]
    return r64


@pytest.mark.parametrize('snr_index', [0, 1])
@pytest.mark.parametrize('pool', [100, 20])
def test_whole_chain_on_host_randomness(pool, snr_index):
    Hp, Hp_est = K.chain_pool(pool)
    rnd = K.host_randomness(pool, snr_index)
    got = gpu_simulate(Hp, Hp_est, 10 ** (-K.CHAIN_SNRS[snr_index] / 10), K.CHAIN_PACKETS, rnd)
    r64 = _check_chain(got, pool, snr_index)
    bler = r64['ideal']['bler'].mean()
    assert (0.2 <= bler <= 0.8) if snr_index == 0 else bler < 0.05


# ---- 7. device randomness --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pool,snr_index', [(100, 0), (20, 1)])
def test_device_randomness_is_replayed_by_the_host_and_independent_of_chunking(pool, snr_index):
    from score_based_channels_amd import noise as N
    Hp, Hp_est = K.chain_pool(pool)
    npow, n, seed = 10 ** (-K.CHAIN_SNRS[snr_index] / 10), K.CHAIN_PACKETS, 2024
    dev = gpu_simulate(Hp, Hp_est, npow, n, None, seed=seed, snr_index=snr_index)
    uses = dev['chan_index'].shape[1]
    packets = np.arange(n)
    pay, idx, w = N.link_payload(seed, snr_index, packets, 324), N.link_indices(seed, snr_index, packets, uses, pool), \
        N.link_noise(seed, snr_index, packets, uses, K.CHAIN_NR)
    assert np.array_equal(dev['payload'], pay) and np.array_equal(dev['chan_index'], idx)
    assert idx.min() >= 0 and idx.max() < pool
    if pool >= uses:
        assert all(len(set(row)) == uses for row in idx)                     # without replacement
    else:
        assert any(len(set(row)) < uses for row in idx)
    assert np.max(np.abs(dev['noise'] - w)) < 2e-6 * max(1.0, np.max(np.abs(w)))      # libm against the GPU's math library, ~ 10 ulp
    # the run on the replayed draws is held to the oracles like the host-randomness chain
    host = gpu_simulate(Hp, Hp_est, npow, n, (pay, idx, w))
    _check_chain(host, pool, snr_index, (pay, idx, w))
    # chunks of 16 with their packet0 give the bits of the one chunk of 64
    parts = [gpu_simulate(Hp, Hp_est, npow, 16, None, seed=seed, snr_index=snr_index, packet0=p0) for p0 in range(0, n, 16)]
    for k in ('payload', 'chan_index', 'ber_ideal', 'bler_ideal', 'ber_est', 'bler_est', 'iters_ideal', 'iters_est'):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), dev[k]), k
    assert np.array_equal(np.concatenate([p['noise'] for p in parts]).view(np.int32), dev['noise'].view(np.int32))
    # 5-sigma moments of the bits and the noise
    bits, z = dev['payload'].astype(np.float64), dev['noise'].astype(np.complex128).ravel()
    assert abs(bits.mean() - 0.5) < 5 * 0.5 / np.sqrt(bits.size)
    assert abs(z.real.mean()) < 5 * np.sqrt(0.5 / z.size) and abs(z.imag.mean()) < 5 * np.sqrt(0.5 / z.size)
    assert abs(np.mean(np.abs(z) ** 2) - 1) < 5 / np.sqrt(z.size)            # |z|^2 is exponential: variance 1
    assert abs(np.mean(z.real * z.imag)) < 5 * 0.5 / np.sqrt(z.size)


# ---- 8. CLI ----------------------------------------------------------------------------------------------------------------------
CLI_SNRS = (-27.0, -23.0)


def test_cli_synthetic_run_writes_the_scripts_result(tmp_path, capsys):
    from score_based_channels_amd import test_end_to_end as T
    out = T.main(['--synthetic', '--seed', '3', '--num_packets', '64', '--snr_range'] + ['%g' % s for s in CLI_SNRS] + ['--out_dir', str(tmp_path)])
    path = tmp_path / 'ours_known_alpha1.00.pt'
    assert path.exists() and 'packets/s' in capsys.readouterr().out
    saved = torch.load(str(path), weights_only=False)
    assert set(saved) == {'bler_ideal', 'ber_ideal', 'bler_est', 'ber_est', 'target_alpha', 'snr_range', 'alpha_array', 'precoding_offset', 'seed'}
    for k in ('bler_ideal', 'ber_ideal', 'bler_est', 'ber_est'):
        assert np.shape(saved[k]) == (2,) and np.array_equal(saved[k], out[k]) and np.all((saved[k] >= 0) & (saved[k] <= 1))
    assert np.array_equal(saved['snr_range'], CLI_SNRS) and saved['seed'] == 3 and saved['precoding_offset'] == 20
    # Both receivers see the same 64 packets, so the difference of the two block error rates is a mean of 64 values in {-1, 0, 1};
    # its standard deviation is at most sqrt(1 / 64) = 0.125 (all packets discordant); slack: three of them.
    slack = 3 * np.sqrt(1.0 / 64)
    assert np.all(saved['bler_ideal'] <= saved['bler_est'] + slack)
    assert np.all(saved['ber_ideal'] <= saved['bler_ideal']) and np.all(saved['ber_est'] <= saved['bler_est'])


# ---- the Python host (link.py) ---------------------------------------------------------------------------------------------------
def test_python_wrappers_return_what_the_library_calls_return():
    """link.encode / ml_llr / decode / errors against the guarded launches above, bit for bit, and simulate_chunk on the host replay of
    the device streams against the device streams themselves: the same payloads and picks, noise equal to fp32 rounding, so at most
    2 % of the packets may decide differently."""
    from score_based_channels_amd import link
    code = _code('ref')
    Hp, Hp_est = K.chain_pool(20)
    payload, idx, w = (a[:5] for a in K.host_randomness(20, 0))
    npow = 10 ** (-K.CHAIN_SNRS[0] / 10)
    cw, sym = link.encode(code, payload, num_streams=4)
    rcw, rsym = gpu_encode('ref', payload, 4)
    assert np.array_equal(cw.cpu().numpy(), rcw) and np.array_equal(sym.cpu().numpy(), rsym)
    li, le = link.ml_llr(code, sym, Hp, Hp_est, idx, w, npow)
    rli, rle = gpu_llr('ref', rsym, Hp, Hp_est, idx, w, npow)
    assert np.array_equal(li.cpu().numpy(), rli) and np.array_equal(le.cpu().numpy(), rle)
    soft, totals, its = link.decode(code, le, want_totals=True, want_iters=True)
    rsoft, rtotals, rits = gpu_decode('ref', rle, 50, True)
    assert np.array_equal(soft.cpu().numpy(), rsoft) and np.array_equal(totals.cpu().numpy(), rtotals) and np.array_equal(its.cpu().numpy(), rits)
    assert np.array_equal(link.decode(code, le).cpu().numpy(), rsoft)
    ber, bler = link.errors(code, soft, payload)
    rber, rbler = gpu_errors('ref', rsoft, payload)
    assert np.array_equal(ber.cpu().numpy(), rber) and np.array_equal(bler.cpu().numpy(), rbler)
    with pytest.raises(ValueError, match='out of range'):
        link.ml_llr(code, sym, Hp, Hp_est, idx + 20, w, npow)
    dev = link.simulate_chunk(code, Hp, Hp_est, npow, 64, seed=11, snr_index=3, packet0=128, want_draws=True)
    draws = link.host_draws(code, 11, 3, 128, 64, 4, 20, K.CHAIN_NR)
    assert np.array_equal(dev['payload'].cpu().numpy(), draws[0]) and np.array_equal(dev['chan_index'].cpu().numpy(), draws[1])
    host = link.simulate_chunk(code, Hp, Hp_est, npow, 64, randomness=draws)
    differ = np.zeros(64, bool)
    for k in ('ber_ideal', 'bler_ideal', 'ber_est', 'bler_est'):
        differ |= dev[k].cpu().numpy() != host[k].cpu().numpy()
    assert np.mean(differ) <= 0.02, differ.sum()
