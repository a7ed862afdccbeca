"""Host-side Gaussian streams for reproducible ("external noise") annealed-Langevin runs.

The reference never seeds its RNG (``test_score.py:115,124,161`` call ``torch.randn_like`` on the
default CUDA generator), so "identical seeds" has to be defined by the build: every draw the loop
makes is keyed by ``(seed, purpose, snr index)`` on a counter-based numpy ``Philox`` generator whose
float32 ziggurat stream does not depend on platform or thread count.  The draw order inside one
stream follows the reference: one initial estimate per (spacing,
pilot_alpha) combination shared by all SNR points, then per SNR point one measurement-noise draw
followed by one draw per Langevin step.

A complex64 standard normal is two float32 N(0, 1/2) values, interleaved (re, im), exactly what
``torch.randn_like`` produces for a complex tensor.
"""
import numpy as np

_SQRT_HALF = np.float32(np.sqrt(0.5))
INIT, MEAS, STEP = 0, 1, 2


def _gen(seed, purpose, index):
    return np.random.Generator(np.random.Philox(key=[int(seed), (int(purpose) << 32) | int(index)]))


def complex_normal(rng, shape):
    z = rng.standard_normal(tuple(shape) + (2,), dtype=np.float32) * _SQRT_HALF
    return np.ascontiguousarray(z).view(np.complex64)[..., 0]


class HostNoise:
    """Keyed CN(0,1) draws for one (spacing, pilot_alpha) combination / grid cell ``combo``."""

    def __init__(self, seed, combo=0):
        self.seed = int(seed)
        self.combo = int(combo)

    def init(self, shape):
        """``init_val_H = randn_like(val_H)`` (test_score.py:115)."""
        return complex_normal(_gen(self.seed, INIT, self.combo << 16), shape)

    def measurement(self, snr_idx, shape):
        """The ``randn_like(val_Y)`` of test_score.py:124 for SNR point ``snr_idx``."""
        return complex_normal(_gen(self.seed, MEAS, (self.combo << 16) | snr_idx), shape)

    def step_stream(self, snr_idx, shape):
        """Returns ``f(k)`` giving the ``randn_like(current)`` of Langevin step ``k`` (test_score.py:161)
        for SNR point ``snr_idx``; steps must be requested in increasing order."""
        rng = _gen(self.seed, STEP, (self.combo << 16) | snr_idx)
        state = {'k': 0}

        def draw(k):
            if k != state['k']:
                raise ValueError('step noise must be drawn sequentially (got %d, expected %d)' % (k, state['k']))
            state['k'] += 1
            return complex_normal(rng, shape)
        return draw

    def step_block(self, snr_idx, shape, n_steps):
        """All ``n_steps`` step draws of one SNR point as ``[n_steps, *shape]`` complex64."""
        rng = _gen(self.seed, STEP, (self.combo << 16) | snr_idx)
        return np.stack([complex_normal(rng, shape) for _ in range(n_steps)])


# ---- host replay of the coded link simulation's device streams (csrc/link.hip; include/sbc_hip.h "Randomness") ---------------------
# Philox4x32-10 under key = seed, counter (q, 4 snr_index + purpose, packet lo, packet hi): a packet's draws depend on nothing but
# (seed, SNR index, packet index, purpose) -- not on the chunk, the batch size or the rank that simulates it.
LINK_PAYLOAD, LINK_INDEX, LINK_NOISE = 0, 1, 2
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32(counter, seed):
    """Philox4x32-10 of uint32 counters ``[..., 4]`` under the 64-bit key ``seed``: uint32 ``[..., 4]``."""
    c = np.asarray(counter, np.uint32)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    lo32 = np.uint64(0xFFFFFFFF)
    with np.errstate(over='ignore'):
        for _ in range(10):
            p0, p1 = c0.astype(np.uint64) * _M0, c2.astype(np.uint64) * _M1
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & lo32).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & lo32).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0, k1 = np.uint32(k0 + _W0), np.uint32(k1 + _W1)
    return np.stack((c0, c1, c2, c3), axis=-1)


def _link_blocks(seed, snr_index, purpose, packets, n_blocks):
    """uint32 ``[len(packets), 4 n_blocks]``: the words of blocks 0 .. n_blocks - 1 of every packet's stream, in order."""
    packets = np.asarray(packets, np.int64).reshape(-1)
    ctr = np.zeros((len(packets), n_blocks, 4), np.uint32)
    ctr[..., 0] = np.arange(n_blocks, dtype=np.uint32)[None, :]
    ctr[..., 1] = np.uint32(4 * int(snr_index) + purpose)
    ctr[..., 2] = (packets & 0xFFFFFFFF).astype(np.uint32)[:, None]
    ctr[..., 3] = (packets >> 32).astype(np.uint32)[:, None]
    return philox4x32(ctr, seed).reshape(len(packets), 4 * n_blocks)


def link_payload(seed, snr_index, packets, K):
    """Payload bits uint8 ``[len(packets), K]``: bit k is bit ``k & 31`` of word ``k >> 5`` of the packet's payload stream."""
    words = _link_blocks(seed, snr_index, LINK_PAYLOAD, packets, (K + 127) // 128)
    k = np.arange(K)
    return ((words[:, k >> 5] >> (k & 31).astype(np.uint32)) & np.uint32(1)).astype(np.uint8)


def link_indices(seed, snr_index, packets, uses, pool):
    """Channel indices int32 ``[len(packets), uses]``: draw t gives ``(word_t * pool) >> 32``; with ``pool >= uses`` a draw that repeats an
    earlier index of the packet is skipped (the first ``uses`` entries of a random permutation), otherwise every draw counts."""
    packets = np.asarray(packets, np.int64).reshape(-1)
    out = np.empty((len(packets), uses), np.int32)
    if pool < uses:
        words = _link_blocks(seed, snr_index, LINK_INDEX, packets, (uses + 3) // 4)[:, :uses]
        return ((words.astype(np.uint64) * np.uint64(pool)) >> np.uint64(32)).astype(np.int32)
    n_blocks = (uses + 3) // 4
    while True:
        words = _link_blocks(seed, snr_index, LINK_INDEX, packets, n_blocks)
        cand = ((words.astype(np.uint64) * np.uint64(pool)) >> np.uint64(32)).astype(np.int32)
        short = False
        for i, row in enumerate(cand):
            _, first = np.unique(row, return_index=True)
            first.sort()
            if len(first) < uses:
                short = True
                break
            out[i] = row[first[:uses]]
        if not short:
            return out
        n_blocks *= 2


def link_noise(seed, snr_index, packets, uses, Nr):
    """Standard CN(0, 1) draws complex64 ``[len(packets), uses, Nr]``: element e = use Nr + r takes words (x, y) (e even) or (z, w) (e odd)
    of block e >> 1; u = ((word >> 8) + 0.5) / 2^24 and (re, im) = sqrt(-ln u1) (cos 2 pi u2, sin 2 pi u2), in float32 like the kernel
    (libm against the GPU's math library: equal to fp32 rounding, not bit for bit)."""
    n = uses * Nr
    words = _link_blocks(seed, snr_index, LINK_NOISE, packets, (n + 1) // 2).reshape(-1, 2)
    f32 = np.float32
    u = ((words >> np.uint32(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)
    rad = np.sqrt(-np.log(u[:, 0], dtype=f32), dtype=f32)
    ang = (f32(6.283185307179586) * u[:, 1]).astype(f32)
    z = ((rad * np.cos(ang, dtype=f32)).astype(f32) + 1j * (rad * np.sin(ang, dtype=f32)).astype(f32)).astype(np.complex64)
    return z.reshape(-1, 2 * ((n + 1) // 2))[:, :n].reshape(-1, uses, Nr)
