"""The link kernels (csrc/link.hip) off the geometry of tests/test_gpu_link.py: check degrees 2, 5, 6 (and a code that mixes them), every
count of codewords per decoder workgroup from 1 to 8 with a partly filled last workgroup, slots of one workgroup that stop at different
times, channel indices outside the pool, payload lengths below, at and off a multiple of 32, index pools around the number of channel
uses, the errors kernel on signed zeros, NaN, infinities and denormals, the workspace of sbc_link_simulate growing and shrinking, and
link.simulate_packets.  Inputs and codes in tests/link_cases.py; the criterion is that of tests/test_gpu_link.py -- kernel error against
float64 within 4x the float32 restatement's (tests/link_oracle.py), decisions equal to float64's wherever the restatements agree --
and tests/test_link_cpu.py holds the yardstick to being finite, and the restatements to agreeing, on every input used here.  Every
launch runs on guarded operands (tests/link_gpu.py)."""
import numpy as np
import pytest
import torch

import link_cases as K
import link_oracle as O
from link_gpu import _code, gpu_decode, gpu_encode, gpu_errors, gpu_llr, gpu_simulate

pytestmark = pytest.mark.gpu

NEW_CODES = sorted(K.SHAPE_CODES)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) if a.dtype == np.complex64 else a


# ---- codes -----------------------------------------------------------------------------------------------------------------------
def test_a_code_whose_decoder_tables_exceed_the_lds_budget_is_refused():
    from score_based_channels_amd import _lib, link
    with pytest.raises(_lib.SbcError, match='does not fit'):
        link.Code(O.REF_BASE, 77).handle('cuda:0')


# ---- encoder ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [2, 4])
@pytest.mark.parametrize('name', NEW_CODES)
def test_encoder_on_the_new_codes(name, S):
    H, P, _, _ = K.code(name)
    payload = np.random.default_rng(12).integers(0, 2, (5, H.shape[1] - H.shape[0]))
    cw, sym = gpu_encode(name, payload, S)
    ref = O.encode(H, payload)
    assert not (H.astype(np.int64) @ ref.T % 2).any()
    assert np.array_equal(cw, ref)
    assert np.array_equal(sym, O.modulate(ref, P, S).astype(np.complex64))


@pytest.mark.parametrize('name', NEW_CODES + ['small'])
def test_encoder_payload_from_the_device_stream(name):
    """K = 15 and 28 (one masked word), 279 .. 672 with a masked last word, 384 and 480 (full words only)."""
    from score_based_channels_amd import noise as N
    H, P, _, _ = K.code(name)
    Kb = H.shape[1] - H.shape[0]
    cw, sym, pay = gpu_encode(name, 5, 4, random=True, seed=77, snr_index=3, packet0=9)
    assert np.array_equal(pay, N.link_payload(77, 3, np.arange(9, 14), Kb)) and set(np.unique(pay)) == {0, 1}
    ref = O.encode(H, pay)
    assert np.array_equal(cw, ref) and np.array_equal(sym, O.modulate(ref, P, 4).astype(np.complex64))


# ---- decoder ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('iters', K.FIXED_ITERS)
@pytest.mark.parametrize('name', NEW_CODES)
def test_decoder_totals_after_fixed_iterations_on_the_new_codes(name, iters):
    """19 codewords: the last workgroup is partly filled for every count of codewords per workgroup but 1."""
    llr = K.fixed_iteration_inputs(name)
    t64, t32 = K.fixed_iteration_totals(name, iters, 'float64'), K.fixed_iteration_totals(name, iters, 'float32')
    assert np.isfinite(t64).all() and len(llr) == 19
    soft, totals, its = gpu_decode(name, llr, iters, False)
    e_ref, e_gpu = np.max(np.abs(t32 - t64)), np.max(np.abs(totals - t64))
    print('decoder %s %d iterations: kernel %.3e  float32 restatement %.3e  ratio %.2f  largest total %.1f'
          % (name, iters, e_gpu, e_ref, e_gpu / e_ref, np.max(np.abs(t64))))
    assert e_gpu <= 4 * e_ref, (e_gpu, e_ref)
    assert np.array_equal(soft, totals[:, :soft.shape[1]]) and np.all(its == iters)
    if iters == K.FIXED_ITERS[-1]:
        for row in (0, 9, 18):                                               # alone in a workgroup: the same bits
            s1, t1, i1 = gpu_decode(name, llr[row:row + 1], iters, False)
            assert np.array_equal(_bits(t1[0]), _bits(totals[row])) and np.array_equal(_bits(s1[0]), _bits(soft[row])) and i1[0] == iters


@pytest.mark.parametrize('name', sorted(K.STAGGERED_GROUPS))
def test_decoder_slots_of_a_workgroup_stop_at_different_times(name):
    """Every workgroup holds a noiseless codeword and an all-zero row (1 iteration each), codewords that never converge and ordinary
    ones: a stopped slot's totals stay frozen while its neighbours run on."""
    batch = K.staggered_batch(name)
    (t64, i64), (t32, i32) = K.staggered_decode(name, 'float64'), K.staggered_decode(name, 'float32')
    same = (i64 == i32) & ((t64 < 0) == (t32 < 0)).all(axis=1)
    assert np.mean(~same) <= 0.02
    soft, totals, its = gpu_decode(name, batch, 50, True)
    ncw = K.SHAPE_CODES[name][2]
    print('decoder %s, %d workgroups of %d: iterations %s' % (name, len(batch) // ncw, ncw, its.reshape(-1, ncw).tolist()))
    assert np.array_equal(its[same], i64[same]) and not ((totals < 0) != (t64 < 0))[same].any()
    zero = np.arange(len(batch)) % ncw == 1
    assert np.all(totals[zero] == 0) and np.all(its[zero] == 1) and np.all(its[np.arange(len(batch)) % ncw == 0] == 1)
    for row in range(len(batch)):
        s1, t1, i1 = gpu_decode(name, batch[row:row + 1], 50, True)
        assert np.array_equal(_bits(t1[0]), _bits(totals[row])) and np.array_equal(_bits(s1[0]), _bits(soft[row])) and i1[0] == its[row], row


@pytest.mark.parametrize('snr', K.MIXED_SNRS)
def test_full_decoder_decides_like_float64_on_mixed_check_degrees(snr):
    llr, payload = K.decoder_inputs('mixed')[snr]
    (t64, i64), (t32, i32) = K.full_decode('mixed', snr, 'float64'), K.full_decode('mixed', snr, 'float32')
    same = (i64 == i32) & ((t64 < 0) == (t32 < 0)).all(axis=1)
    assert np.mean(~same) <= 0.02
    soft, totals, its = gpu_decode('mixed', llr, 50, True)
    bad = same & ((its != i64) | ((totals < 0) != (t64 < 0)).any(axis=1))
    print('full decoder mixed %.1f dB: %d of %d never converge, restatement differs on %d, kernel on %d' % (snr, (i64 == 50).sum(), len(llr), (~same).sum(), bad.sum()))
    assert not bad.any(), np.nonzero(bad)[0]
    ber, bler = gpu_errors('mixed', soft, payload)
    rber, rbler = O.packet_errors(t64[:, :payload.shape[1]], payload)
    assert payload.shape[1] == 28
    assert np.array_equal(ber[same], rber[same].astype(np.float32)) and np.array_equal(bler[same], rbler[same].astype(np.float32))


# ---- soft bits -------------------------------------------------------------------------------------------------------------------
def test_soft_bits_on_the_reference_code_with_two_streams_and_no_padded_tail():
    """162 channel uses of 3 packets, Nr = 5, a pool of 9: the criterion per packet."""
    c = K.llr_batch('ref', 2, 5, 3)
    r64, r32 = K.llr_batch_oracle('ref', 2, 5, 3, np.float64), K.llr_batch_oracle('ref', 2, 5, 3, np.float32)
    assert np.isfinite(r64[0]).all() and np.isfinite(r64[1]).all() and c['sym'].shape[1] * 4 == c['H'].shape[1]
    got = gpu_llr('ref', c['sym'], c['Hp'], c['Hp_est'], c['idx'], c['w'], c['noise_power'], clip=False)
    for p in range(3):
        e_ref = max(np.max(np.abs(r32[k][p] - r64[k][p])) for k in (0, 1))
        e_gpu = max(np.max(np.abs(got[k][p] - r64[k][p])) for k in (0, 1))
        print('llr ref S=2 Nr=5 packet %d: kernel %.3e  float32 restatement %.3e  ratio %.2f  largest |llr| %.1f'
              % (p, e_gpu, e_ref, e_gpu / e_ref, np.max(np.abs(r64[0][p]))))
        assert e_gpu <= 4 * e_ref, (p, e_gpu, e_ref)
    clipped = gpu_llr('ref', c['sym'], c['Hp'], c['Hp_est'], c['idx'], c['w'], c['noise_power'], clip=True)
    for k in (0, 1):
        want = got[k].copy()
        big = np.abs(want) >= O.CLIP
        want[big] = O.CLIP * np.sign(want[big])
        assert np.array_equal(clipped[k], want)


@pytest.mark.parametrize('S', [2, 4])
def test_a_channel_index_outside_the_pool_gives_nan_soft_bits_of_that_use_only(S):
    """include/sbc_hip.h: an index outside the pool gives NaN soft bits and no read through it.  The outputs start from 7, so a NaN is
    one the kernel wrote."""
    name = 'small' if S == 2 else 'small10'
    c = K.llr_batch(name, S, 3, 3)
    idx = c['idx'].copy()
    idx[1, 2], idx[1, 5] = c['pool'], -1
    hit = np.concatenate([c['P'][u * 2 * S:(u + 1) * 2 * S] for u in (2, 5)])
    for clip in (False, True):
        good = gpu_llr(name, c['sym'], c['Hp'], c['Hp_est'], c['idx'], c['w'], c['noise_power'], clip=clip, fill=7.0)
        bad = gpu_llr(name, c['sym'], c['Hp'], c['Hp_est'], idx, c['w'], c['noise_power'], clip=clip, fill=7.0)
        for k in (0, 1):
            assert np.isfinite(good[k]).all()
            nan = np.zeros(good[k].shape, bool)
            nan[1, hit] = True
            assert np.array_equal(np.isnan(bad[k]), nan) and nan.sum() == 4 * S
            assert np.array_equal(_bits(bad[k])[~nan], _bits(good[k])[~nan])


# ---- errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['small', 'mixed'])
def test_errors_kernel_on_zeros_nan_infinities_and_denormals(name):
    """K = 15 and 28 (less than a wave), 5 packets (a partly filled workgroup); sign(-soft): +-0 and NaN are errors whatever the bit,
    +-inf and the smallest denormals count by their sign."""
    Kb = _code(name).K
    rng = np.random.default_rng(Kb)
    tiny = np.float32(1e-45)
    assert tiny > 0 and tiny / 2 == 0
    values = np.array([2.5, -2.5, 0.0, -0.0, np.nan, np.inf, -np.inf, tiny, -tiny], np.float32)
    soft = values[rng.integers(0, len(values), (5, Kb))]
    soft[0] = np.where(np.arange(Kb) % 2 == 0, np.inf, -tiny)                 # a packet without an error ...
    payload = rng.integers(0, 2, (5, Kb)).astype(np.uint8)
    payload[0] = np.arange(Kb) % 2
    soft[1] = soft[0]                                                         # ... and one with exactly one
    payload[1] = payload[0]
    payload[1, Kb - 1] ^= 1
    ber, bler = gpu_errors(name, soft, payload)
    rber, rbler = O.packet_errors(soft, payload)
    wrong = np.array([sum(not ((s > 0 and b == 0) or (s < 0 and b == 1)) for s, b in zip(ss, pp)) for ss, pp in zip(soft, payload)])
    assert np.array_equal(rber, wrong / Kb) and wrong[0] == 0 and wrong[1] == 1 and wrong[2:].min() > 1
    assert np.array_equal(ber, (wrong / Kb).astype(np.float32)) and np.array_equal(bler, (wrong > 0).astype(np.float32))
    assert np.array_equal(bler, rbler.astype(np.float32))


# ---- whole chain, device randomness at other geometries --------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', K.SIM_GEOMETRIES, ids=lambda g: '%s-S%d-Nr%d-pool%d' % g[:4])
def test_device_randomness_at_other_geometries(geometry):
    name, S, Nr, pool, npow = geometry
    Hp, Hp_est = K.sim_pool(pool, Nr, S)
    n, seed, si, p0 = K.SIM_PACKETS, K.SIM_SEED, K.SIM_SNR_INDEX, K.SIM_PACKET0
    dev = gpu_simulate(Hp, Hp_est, npow, n, None, seed=seed, snr_index=si, packet0=p0, name=name)
    pay, idx, w = K.sim_draws(name, S, Nr, pool)
    uses = idx.shape[1]
    assert np.array_equal(dev['payload'], pay) and np.array_equal(dev['chan_index'], idx)
    assert idx.min() >= 0 and idx.max() < pool
    assert (pool >= uses) == all(len(set(row)) == uses for row in idx)
    assert np.max(np.abs(dev['noise'] - w)) < 2e-6 * max(1.0, np.max(np.abs(w)))      # libm against the GPU's math library, ~ 10 ulp
    # chunks of 3, 3, 3 and 1 with their packet0 give the bits of the one chunk of 10
    parts = [gpu_simulate(Hp, Hp_est, npow, min(3, n - q), None, seed=seed, snr_index=si, packet0=p0 + q, name=name) for q in range(0, n, 3)]
    assert [len(p['payload']) for p in parts] == [3, 3, 3, 1]
    for k in ('payload', 'chan_index', 'ber_ideal', 'bler_ideal', 'ber_est', 'bler_est', 'iters_ideal', 'iters_est'):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), dev[k]), k
    assert np.array_equal(_bits(np.concatenate([p['noise'] for p in parts])), _bits(dev['noise']))
    # the run on the replayed draws is held to the oracles
    host = gpu_simulate(Hp, Hp_est, npow, n, (pay, idx, w), name=name)
    r64, r32 = K.sim_oracle(name, S, Nr, pool, npow, 'float64'), K.sim_oracle(name, S, Nr, pool, npow, 'float32')
    assert all(np.isfinite(r64[rx]['llr']).all() for rx in ('ideal', 'est'))
    same = K.same_packets(r64, r32)
    assert np.mean(~same) <= 0.02
    bad = np.zeros(n, bool)
    for rx in ('ideal', 'est'):
        bad |= (host['ber_' + rx] != r64[rx]['ber'].astype(np.float32)) | (host['bler_' + rx] != r64[rx]['bler'].astype(np.float32))
    print('chain %s S=%d Nr=%d pool %d: BLER ideal %.2f est %.2f; restatement differs on %d packets, kernel on %d of the others'
          % (name, S, Nr, pool, r64['ideal']['bler'].mean(), r64['est']['bler'].mean(), (~same).sum(), (bad & same).sum()))
    assert not (bad & same).any(), np.nonzero(bad & same)[0]
    assert 0.2 <= r64['ideal']['bler'].mean() <= 0.8


# ---- the workspace of sbc_link_simulate ------------------------------------------------------------------------------------------
def test_simulate_workspace_grows_and_is_reused_at_a_smaller_size():
    """One code handle, a stream of its own: 16, then 64 (the workspace is replaced), then 16 packets again (the larger one is kept),
    each bit-identical to the same call on a fresh handle."""
    from score_based_channels_amd import link
    Hp, Hp_est = K.chain_pool(20)
    rnd = K.host_randomness(20, 0)
    npow = 10 ** (-K.CHAIN_SNRS[0] / 10)
    H, P, base, Z = K.code('ref')
    one = link.Code(base, Z, K.INTERLEAVER_SEED)
    with torch.cuda.stream(torch.cuda.Stream()):
        for n in (16, 64, 16):
            draws = tuple(a[:n] for a in rnd)
            got = gpu_simulate(Hp, Hp_est, npow, n, draws, code=one)
            fresh = link.Code(base, Z, K.INTERLEAVER_SEED)
            want = gpu_simulate(Hp, Hp_est, npow, n, draws, code=fresh)
            fresh.close()
            for k in ('ber_ideal', 'bler_ideal', 'ber_est', 'bler_est', 'iters_ideal', 'iters_est'):
                assert np.array_equal(_bits(got[k]), _bits(want[k])), (n, k)
            assert 0 < got['bler_ideal'].mean() < 1
    one.close()


# ---- link.simulate_packets -------------------------------------------------------------------------------------------------------
def test_simulate_packets_chunks_averages_and_host_noise():
    """Two SNR points, 64 packets, a pool of 20 synthetic channels: the curves do not depend on the chunking (the per-chunk sums are
    exact in float64: at most 64 float32 values between 1 / 324 and 1), they are the means of simulate_chunk's per-packet results at
    snr_index = the point's index, run_ideal = False drops the ideal curves only, and the host replay of the noise may move at most
    2 % of the packets of a point."""
    from score_based_channels_amd import link
    code, device = _code('ref'), torch.device('cuda', 0)
    rng = np.random.default_rng(31)
    real = K._cn(rng, (K.CHAIN_NR, K.CHAIN_NT, 20)).astype(np.complex64)
    est = np.stack([real + K._cn(rng, real.shape) * 10 ** (K.EST_NMSE_DB / 20) for _ in range(2)]).astype(np.complex64)
    snrs, n, seed = K.CHAIN_SNRS, 64, 99
    args = (real, est, 2, K.CHAIN_NT, K.CHAIN_NR, 'random', K.CHAIN_S, n, snrs)
    curves = {chunk: link.simulate_packets(*args, code=code, seed=seed, chunk=chunk) for chunk in (16, 48, 64)}
    for chunk in (16, 48):
        for a, b in zip(curves[chunk], curves[64]):
            assert np.array_equal(a, b), chunk
    bler_i, ber_i, bler_e, ber_e = curves[64]
    assert all(c.shape == (2,) and c.dtype == np.float64 for c in curves[64])
    # the same precoded channels as simulate_packets forms them
    prng = np.random.Generator(np.random.Philox(key=[seed, 3 << 32]))
    Pt = (prng.standard_normal((20, K.CHAIN_NT, K.CHAIN_S, 2)) * np.sqrt(0.5)).view(np.complex128)[..., 0]
    Pt = torch.from_numpy(Pt.astype(np.complex64)).to(device)

    def precoded(Hc):
        Hc = torch.from_numpy(np.ascontiguousarray(np.moveaxis(Hc, 2, 0)).astype(np.complex64)).to(device)
        return torch.matmul(Hc, Pt).contiguous()
    host_curves = link.simulate_packets(*args, code=code, seed=seed, chunk=48, noise='host')
    for si, snr in enumerate(snrs):
        Hi, He = precoded(real), precoded(est[si])
        dev = link.simulate_chunk(code, Hi, He, 10.0 ** (-snr / 10.0), n, seed=seed, snr_index=si)
        dev = {k: v.cpu().numpy() for k, v in dev.items()}
        for curve, k in ((bler_i, 'bler_ideal'), (ber_i, 'ber_ideal'), (bler_e, 'bler_est'), (ber_e, 'ber_est')):
            assert curve[si] == dev[k].astype(np.float64).sum() / n, (si, k)
        host = link.simulate_chunk(code, Hi, He, 10.0 ** (-snr / 10.0), n, randomness=link.host_draws(code, seed, si, 0, n, K.CHAIN_S, 20, K.CHAIN_NR))
        host = {k: v.cpu().numpy() for k, v in host.items()}
        differ = np.zeros(n, bool)
        for j, k in enumerate(('bler_ideal', 'ber_ideal', 'bler_est', 'ber_est')):
            differ |= dev[k] != host[k]
            assert host_curves[j][si] == host[k].astype(np.float64).sum() / n, (si, k)
        assert np.mean(differ) <= 0.02, (si, differ.sum())
    assert 0.2 <= bler_i[0] <= 0.9 and bler_i[1] < 0.1 and np.all(ber_i <= bler_i) and np.all(ber_e <= bler_e)
    no_ideal = link.simulate_packets(*args, run_ideal=False, code=code, seed=seed, chunk=64)
    assert no_ideal[0] is None and no_ideal[1] is None
    assert np.array_equal(no_ideal[2], bler_e) and np.array_equal(no_ideal[3], ber_e)
