"""The inputs of the link-simulation tests, shared by tests/test_link_cpu.py (which holds the float64 yardstick to being finite on
them, and the float32 restatement to agreeing with it) and tests/test_gpu_link.py.  Everything is derived from fixed seeds; the
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


@functools.lru_cache(None)
def code(name):
    """(H, P, base, Z) of 'ref' (802.11n, Z = 27), 'small' (Z = 5) and 'small10' (the small base at Z = 10: N = 60)."""
    base, Z = {'ref': (L.REF_BASE, L.REF_Z), 'small': (L.SMALL_BASE, L.SMALL_Z), 'small10': (L.SMALL_BASE, 10)}[name]
    H = L.parity_check(base, Z)
    P = np.random.default_rng(INTERLEAVER_SEED).permutation(H.shape[1]).astype(np.int32)
    return H, P, base, Z


@functools.lru_cache(None)
def graph(name):
    return L.Graph(code(name)[0])


@functools.lru_cache(None)
def decoder_inputs(name='ref'):
    """Clipped BPSK-AWGN LLRs ``{snr: (llr [200, N], payload)}`` from ONE ``default_rng(0)``, in the order of DECODER_SNRS."""
    rng = np.random.default_rng(0)
    return {snr: L.bpsk_awgn_llrs(code(name)[0], snr, 200, rng) for snr in DECODER_SNRS}


@functools.lru_cache(None)
def fixed_iteration_inputs(name):
    """64 codewords of clipped BPSK-AWGN LLRs at 1.5 dB."""
    return L.bpsk_awgn_llrs(code(name)[0], 1.5, 64, np.random.default_rng(1))[0]


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
