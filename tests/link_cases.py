"""The inputs of the link-simulation tests, shared by tests/test_link_cpu.py (which holds the float64 yardstick to being finite on
them, and the float32 restatement to agreeing with it), tests/test_gpu_link.py and tests/test_gpu_link_shapes.py (the geometries off
the reference code's: the last part of this file).  Everything is derived from fixed seeds; the
oracle results are computed once per process and must not be modified by a test."""
import functools

import numpy as np

import link_oracle as L

INTERLEAVER_SEED = 1111
DECODER_SNRS = (1.0, 1.5, 2.0)          # Eb/N0 of the BPSK-AWGN decoder inputs, 200 codewords each, default_rng(0)
FIXED_ITERS = (1, 3, 8)
# whole chain (S = 4, Nr = 16, 64 packets, i.i.d. CN(0, 1) channels [16, 64] with CN(0, 1) precoders, estimates at -15 dB NMSE): data
# SNR points chosen with the float64 restatement -- BLER with ideal CSI is 0.2 .. 0.8 at the first and below 0.05 at the second, for
# the pool of 100 and the pool of 20 (tests/test_link_cpu.py asserts it)
CHAIN_SNRS = (-29.0, -27.0)
CHAIN_PACKETS, CHAIN_S, CHAIN_NR, CHAIN_NT, EST_NMSE_DB = 64, 4, 16, 64, -15.0
LLR_NOISE_KINDS = ('1000', '63', 'large-ratio')
LARGE_RATIO = 300.0                     # the third noise power puts the largest metric / noise_power near this (100 < ratio < 700)
# check degrees 2, 5, 6, 7 and variable degrees 1 .. 4; the parity part is lower triangular with an identity diagonal
MIXED_BASE = np.array([[3, -1, -1, -1, 0, -1, -1, -1],
                       [1, 2, 0, -1, 4, 0, -1, -1],
                       [0, 4, 1, 2, -1, 3, 0, -1],
                       [2, 0, 3, 1, 1, -1, 2, 0]], np.int32)
# name: (base, Z, codewords of one decoder workgroup): with 'ref' (4) and 'small' / 'small10' (8) every count from 1 to 8 occurs
# (tests/test_link_cpu.py restates the kernel's LDS formula and asserts the column)
SHAPE_CODES = {'mixed': (MIXED_BASE, 7, 8), 'ref32': (L.REF_BASE, 32, 3), 'ref40': (L.REF_BASE, 40, 2), 'ref56': (L.REF_BASE, 56, 1),
               'small93': (L.SMALL_BASE, 93, 7), 'small105': (L.SMALL_BASE, 105, 6), 'small120': (L.SMALL_BASE, 120, 5)}
BASE_CODES = {'ref': (L.REF_BASE, L.REF_Z, 4), 'small': (L.SMALL_BASE, L.SMALL_Z, 8), 'small10': (L.SMALL_BASE, 10, 8)}
MIXED_SNRS = (1.0, 3.0, 5.0)            # Eb/N0 of the 'mixed' decoder inputs, 200 codewords each, default_rng(0)
SHAPE_CODEWORDS = 19                    # a partly filled last decoder workgroup for every count above 1


@functools.lru_cache(None)
def code(name):
    """(H, P, base, Z) of 'ref' (802.11n, Z = 27), 'small' (Z = 5), 'small10' (the small base at Z = 10: N = 60) and the codes of
    SHAPE_CODES."""
    base, Z, _ = dict(BASE_CODES, **SHAPE_CODES)[name]
    H = L.parity_check(base, Z)
    P = np.random.default_rng(INTERLEAVER_SEED).permutation(H.shape[1]).astype(np.int32)
    return H, P, base, Z


@functools.lru_cache(None)
def graph(name):
    return L.Graph(code(name)[0])


@functools.lru_cache(None)
def decoder_inputs(name='ref'):
    """Clipped BPSK-AWGN LLRs ``{snr: (llr [200, N], payload)}`` from ONE ``default_rng(0)``, in the order of DECODER_SNRS
    ('mixed': of MIXED_SNRS)."""
    rng = np.random.default_rng(0)
    return {snr: L.bpsk_awgn_llrs(code(name)[0], snr, 200, rng) for snr in (MIXED_SNRS if name == 'mixed' else DECODER_SNRS)}


@functools.lru_cache(None)
def fixed_iteration_inputs(name):
    """64 codewords of clipped BPSK-AWGN LLRs at 1.5 dB (the codes of SHAPE_CODES: 19)."""
    return L.bpsk_awgn_llrs(code(name)[0], 1.5, SHAPE_CODEWORDS if name in SHAPE_CODES else 64, np.random.default_rng(1))[0]


@functools.lru_cache(None)
def fixed_iteration_totals(name, iters, dtype):
    return L.decode(graph(name), fixed_iteration_inputs(name), iters, False, np.dtype(dtype).type)[0]


@functools.lru_cache(None)
def full_decode(name, snr, dtype):
    return L.decode(graph(name), decoder_inputs(name)[snr][0], 50, True, np.dtype(dtype).type)


def _cn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


@functools.lru_cache(None)
def llr_case(S, Nr, kind):
    """7 channel uses of one packet (the small code at Z = 5 for S = 2, at Z = 10 for S = 4): a pool of 9 precoded channels, an
    estimate at -15 dB NMSE, random symbols and CN(0, 1) noise.  Returns a dict; ``noise_power`` per ``kind``."""
    name = 'small' if S == 2 else 'small10'
    H, P, _, _ = code(name)
    N = H.shape[1]
    uses = N // (2 * S)
    assert uses == 7
    rng = np.random.default_rng(1000 * S + Nr)
    pool = 9
    Hp = (_cn(rng, (pool, Nr, S)) * 8).astype(np.complex64)
    Hp_est = (Hp + _cn(rng, Hp.shape) * 8 * 10 ** (EST_NMSE_DB / 20)).astype(np.complex64)
    payload = rng.integers(0, 2, (1, N - H.shape[0]))
    sym = L.modulate(L.encode(H, payload), P, S).astype(np.complex64)
    idx = rng.integers(0, pool, (1, uses)).astype(np.int32)
    w = _cn(rng, (1, uses, Nr)).astype(np.complex64)
    if kind == 'large-ratio':
        # noiseless metrics of the wrong candidates: |Hp (x - s)|^2; their largest over LARGE_RATIO is the noise power
        _, pts = L.candidates(S)
        d = np.einsum('urs,ucs->urc', Hp[idx[0]].astype(np.complex128), sym[0][:, None, :] - pts[None, :, :])
        noise_power = float((np.abs(d) ** 2).sum(axis=1).max() / LARGE_RATIO)
    else:
        noise_power = float(kind)
    return dict(name=name, H=H, P=P, S=S, Nr=Nr, pool=pool, Hp=Hp, Hp_est=Hp_est, sym=sym, idx=idx, w=w, noise_power=noise_power)


@functools.lru_cache(None)
def llr_oracle(S, Nr, kind, dtype):
    """Unclipped, deinterleaved soft bits (ideal, est) ``[N]`` of ``llr_case`` and the largest metric / noise_power ratio."""
    c = llr_case(S, Nr, kind)
    y = L.received(c['sym'][0], c['Hp'], c['idx'][0], c['w'][0], c['noise_power'], dtype)
    N = c['H'].shape[1]
    out = [L.finish_llr(L.ml_llr(y, pool[c['idx'][0]], c['noise_power'], dtype), c['P'], N, clip=False) for pool in (c['Hp'], c['Hp_est'])]
    _, pts = L.candidates(S)
    ratio = 0.0
    for pool in (c['Hp'], c['Hp_est']):
        d = y.astype(np.complex128)[:, :, None] - np.einsum('urs,cs->urc', pool[c['idx'][0]].astype(np.complex128), pts)
        ratio = max(ratio, float((np.abs(d) ** 2).sum(axis=1).max() / c['noise_power']))
    return out[0], out[1], ratio


@functools.lru_cache(None)
def chain_pool(pool):
    """Precoded ideal and estimated channels ``[pool, Nr, S]`` complex64 of the whole-chain tests."""
    rng = np.random.default_rng(500 + pool)
    Hc = _cn(rng, (pool, CHAIN_NR, CHAIN_NT))
    He = Hc + _cn(rng, Hc.shape) * 10 ** (EST_NMSE_DB / 20)
    Pt = _cn(rng, (pool, CHAIN_NT, CHAIN_S))
    return (Hc @ Pt).astype(np.complex64), (He @ Pt).astype(np.complex64)


def host_randomness(pool, snr_index, n=CHAIN_PACKETS):
    """Payloads, channel picks (without replacement when the pool allows, as testPackets.m:136-140) and noise of the host-randomness
    chain test."""
    H, _, _, _ = code('ref')
    uses = H.shape[1] // (2 * CHAIN_S)
    rng = np.random.default_rng(7000 + 10 * pool + snr_index)
    payload = rng.integers(0, 2, (n, H.shape[1] - H.shape[0])).astype(np.uint8)
    if pool >= uses:
        idx = np.stack([rng.permutation(pool)[:uses] for _ in range(n)]).astype(np.int32)
    else:
        idx = rng.integers(0, pool, (n, uses)).astype(np.int32)
    w = _cn(rng, (n, uses, CHAIN_NR)).astype(np.complex64)
    return payload, idx, w


def chain_oracle(pool, snr_index, dtype, randomness=None):
    """``link_oracle.chain`` of the whole-chain case (not cached for caller-supplied randomness)."""
    if randomness is None:
        return _chain_cached(pool, snr_index, np.dtype(dtype).name)
    H, P, _, _ = code('ref')
    Hp, Hp_est = chain_pool(pool)
    payload, idx, w = randomness
    return L.chain(H, P, CHAIN_S, payload, idx, w, Hp, Hp_est, 10 ** (-CHAIN_SNRS[snr_index] / 10), np.dtype(dtype).type)


@functools.lru_cache(None)
def _chain_cached(pool, snr_index, dtype):
    return chain_oracle(pool, snr_index, dtype, host_randomness(pool, snr_index))


def same_packets(a, b):
    """Mask of the packets on which two chain results agree in per-packet BER and BLER of both receivers."""
    ok = np.ones(len(a['ideal']['ber']), bool)
    for rx in ('ideal', 'est'):
        ok &= (a[rx]['ber'] == b[rx]['ber']) & (a[rx]['bler'] == b[rx]['bler'])
    return ok


# ---- other geometries (tests/test_gpu_link_shapes.py) ----------------------------------------------------------------------------
@functools.lru_cache(None)
def llr_batch(name, S, Nr, n, pool=9, noise_power=63.0):
    """``n`` packets of random symbols on code ``name`` through a pool of precoded channels as in ``llr_case``; the generator is keyed by
    the geometry."""
    H, P, _, _ = code(name)
    N = H.shape[1]
    uses = N // (2 * S)
    rng = np.random.default_rng([N, S, Nr, n, pool])
    Hp = (_cn(rng, (pool, Nr, S)) * 8).astype(np.complex64)
    Hp_est = (Hp + _cn(rng, Hp.shape) * 8 * 10 ** (EST_NMSE_DB / 20)).astype(np.complex64)
    payload = rng.integers(0, 2, (n, N - H.shape[0]))
    sym = L.modulate(L.encode(H, payload), P, S).astype(np.complex64)
    idx = rng.integers(0, pool, (n, uses)).astype(np.int32)
    w = _cn(rng, (n, uses, Nr)).astype(np.complex64)
    return dict(name=name, H=H, P=P, S=S, Nr=Nr, pool=pool, Hp=Hp, Hp_est=Hp_est, sym=sym, idx=idx, w=w, noise_power=float(noise_power))


@functools.lru_cache(None)
def llr_batch_oracle(name, S, Nr, n, dtype):
    """Unclipped, deinterleaved soft bits (ideal, est) ``[n, N]`` of ``llr_batch``."""
    c = llr_batch(name, S, Nr, n)
    N = c['H'].shape[1]
    out = ([], [])
    for p in range(n):
        y = L.received(c['sym'][p], c['Hp'], c['idx'][p], c['w'][p], c['noise_power'], dtype)
        for k, pool in enumerate((c['Hp'], c['Hp_est'])):
            out[k].append(L.finish_llr(L.ml_llr(y, pool[c['idx'][p]], c['noise_power'], dtype), c['P'], N, clip=False))
    return np.stack(out[0]), np.stack(out[1])


STAGGERED_GROUPS = {'mixed': 3, 'ref32': 6}           # decoder workgroups of the batch below (8 and 3 codewords each)


@functools.lru_cache(None)
def staggered_batch(name):
    """LLRs ``[groups * ncw, N]`` whose codewords stop at different times inside every decoder workgroup: slot 0 a noiseless +-6
    codeword (1 iteration), slot 1 all zeros (1 iteration), the other slots BPSK-AWGN codewords at 1 dB, alternately (counted through
    the whole batch, so with one such slot per workgroup: workgroup by workgroup) one the float64 restatement never converges on and
    one it does, as far as there are enough of each."""
    H = code(name)[0]
    ncw, groups = SHAPE_CODES[name][2], STAGGERED_GROUPS[name]
    rng = np.random.default_rng(17)
    llr = decoder_inputs(name)[1.0][0] if name == 'mixed' else L.bpsk_awgn_llrs(H, 1.0, 40, rng)[0]
    its = L.decode(graph(name), llr, 50, True, np.float64)[1]
    stuck, fine = list(np.nonzero(its == 50)[0]), list(np.nonzero(its < 50)[0])
    assert stuck and fine
    clean = L.CLIP * (1.0 - 2.0 * L.encode(H, rng.integers(0, 2, (groups, H.shape[1] - H.shape[0]))))
    rows = []
    for g in range(groups):
        rows += [clean[g], np.zeros(H.shape[1])]
        for s in range(ncw - 2):
            pick = stuck if ((g * (ncw - 2) + s) % 2 == 0 and stuck) or not fine else fine
            rows.append(llr[pick.pop(0)])
    return np.stack(rows)


@functools.lru_cache(None)
def staggered_decode(name, dtype):
    return L.decode(graph(name), staggered_batch(name), 50, True, np.dtype(dtype).type)


# whole chain with device randomness at other geometries: (code, S, Nr, pool, noise power).  The noise powers were chosen with the
# float64 restatement so that BLER with ideal CSI lies in 0.2 .. 0.8 on the SIM_PACKETS packets of the replayed device streams and both
# restatements agree on every packet (tests/test_link_cpu.py asserts both).  uses = 7 in all of them: pools of 1, uses - 1, uses, uses + 1.
SIM_SEED, SIM_SNR_INDEX, SIM_PACKET0, SIM_PACKETS = 2025, 2, 5, 10
SIM_GEOMETRIES = (('small10', 4, 3, 1, 10 ** 0.2), ('small10', 4, 3, 6, 10 ** 0.1), ('small10', 4, 3, 7, 1.0), ('small10', 4, 3, 8, 1.0),
                  ('small', 2, 5, 9, 10 ** 0.6))


@functools.lru_cache(None)
def sim_pool(pool, Nr, S):
    """Precoded ideal and estimated (-15 dB NMSE) channels ``[pool, Nr, S]`` complex64, i.i.d. CN(0, 1)."""
    rng = np.random.default_rng([900, pool, Nr, S])
    Hp = _cn(rng, (pool, Nr, S))
    return Hp.astype(np.complex64), (Hp + _cn(rng, Hp.shape) * 10 ** (EST_NMSE_DB / 20)).astype(np.complex64)


@functools.lru_cache(None)
def sim_draws(name, S, Nr, pool):
    """The host replay of the device streams for the SIM_PACKETS packets from SIM_PACKET0 on: (payload, chan_index, noise)."""
    from score_based_channels_amd import noise as N
    H = code(name)[0]
    packets = np.arange(SIM_PACKET0, SIM_PACKET0 + SIM_PACKETS)
    uses = H.shape[1] // (2 * S)
    return (N.link_payload(SIM_SEED, SIM_SNR_INDEX, packets, H.shape[1] - H.shape[0]), N.link_indices(SIM_SEED, SIM_SNR_INDEX, packets, uses, pool),
            N.link_noise(SIM_SEED, SIM_SNR_INDEX, packets, uses, Nr))


@functools.lru_cache(None)
def sim_oracle(name, S, Nr, pool, noise_power, dtype):
    """``link_oracle.chain`` of one of SIM_GEOMETRIES on ``sim_draws``."""
    H, P, _, _ = code(name)
    Hp, Hp_est = sim_pool(pool, Nr, S)
    payload, idx, w = sim_draws(name, S, Nr, pool)
    return L.chain(H, P, S, payload, idx, w, Hp, Hp_est, noise_power, np.dtype(dtype).type)
