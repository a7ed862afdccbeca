"""Coded link simulation on the HIP library: what a channel estimate is worth to a receiver, as coded BER / BLER with ideal against
estimated CSI (the reference's ``matlab/testPackets.m`` with ``ComputeLLRMIMO.m``'s ``'ml'`` branch).

Thin wrappers over the ``sbc_link_*`` calls (include/sbc_hip.h; csrc/link.hip): a quasi-cyclic LDPC code from a base matrix of circulant
shifts, the systematic encoder with interleaver and QPSK mapper, exhaustive ML soft demapping on S in {2, 4} streams, flooding
sum-product decoding and the error counts.  torch owns the device memory and the stream and forms ``Hp = H Pt``; every other number
is computed by the HIP kernels.  Shapes, dtypes and values are checked here, on the host, before anything is launched.

Deviations from the script, both documented in DESIGN.md section 17: the soft bits are log-sum-exps around the smallest metric, so the
script's ``NaN -> 0`` line (a 0 / 0 of underflowed sums) is never reached -- the true value is formed and then clipped; and MATLAB's
``randperm`` / ``randi`` / ``randn`` streams cannot be reproduced, so interleaver, payloads, channel picks and noise are this build's own
streams (numpy for the interleaver and precoders, the library's Philox for the per-packet draws, replayed by ``noise.py``).
"""
import ctypes as C

import numpy as np

from . import _lib
from . import noise as _noise

MAX_NR, STREAMS, MAX_N, MAX_CHECK_DEGREE, CLIP = 64, (2, 4), 8192, 8, 6.0

# IEEE 802.11n HT LDPC, N = 648, rate 1/2, Z = 27 (testPackets.m:29-42): circulant shifts, -1 = zero block
_BASE_11N_648 = (
    (0, -1, -1, -1, 0, 0, -1, -1, 0, -1, -1, 0, 1, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (22, 0, -1, -1, 17, -1, 0, 0, 12, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    (6, -1, 0, -1, 10, -1, -1, -1, 24, -1, 0, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1),
    (2, -1, -1, 0, 20, -1, -1, -1, 25, 0, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1),
    (23, -1, -1, -1, 3, -1, -1, -1, 0, -1, 9, 11, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1),
    (24, -1, 23, 1, 17, -1, 3, -1, 10, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1),
    (25, -1, -1, -1, 8, -1, -1, -1, 7, 18, -1, -1, 0, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1),
    (13, 24, -1, -1, 0, -1, 8, -1, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1),
    (7, 20, -1, 16, 22, 10, -1, -1, 23, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1),
    (11, -1, -1, -1, 19, -1, -1, -1, 13, -1, 3, 17, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1),
    (25, -1, 8, -1, 23, 18, -1, 14, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0),
    (3, -1, -1, -1, 16, -1, -1, 2, 25, 5, -1, -1, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0))


def _gf2_invertible(B):
    B = B.copy()
    n = B.shape[0]
    for col in range(n):
        piv = np.nonzero(B[col:, col])[0]
        if not len(piv):
            return False
        p = col + piv[0]
        if p != col:
            B[[col, p]] = B[[p, col]]
        rows = np.nonzero(B[:, col])[0]
        B[rows[rows != col]] ^= B[col]
    return True


class Code:
    """A quasi-cyclic LDPC code: ``base`` ``[rows, cols]`` circulant shifts (-1 = zero block) lifted by ``Z``; the codeword is
    ``[payload; parity]`` with ``H c = 0``.  ``interleaver_seed`` seeds the bit interleaver ``P`` (``bitsInt = bitsEnc[P]``, 0-based) as
    ``numpy.random.default_rng(seed).permutation(N)``: the script's ``rng(1111); randperm(N)`` is MATLAB's Mersenne-Twister stream,
    which cannot be reproduced here, so the permutation differs from the script's (any fixed permutation serves the same purpose).

    Raises ``ValueError`` for what the library does not support: more than 8192 code bits, a check of degree above 8 or below 2, a
    parity part that is singular over GF(2).  The library handle is created on first use, per device."""

    def __init__(self, base, Z, interleaver_seed=1111):
        base = np.asarray(base)
        if base.ndim != 2 or not np.issubdtype(base.dtype, np.integer):
            raise ValueError('base must be a 2-D integer array of circulant shifts (got %s %s)' % (base.dtype, base.shape))
        Z = int(Z)
        rows, cols = base.shape
        if Z < 1 or rows < 1 or cols <= rows:
            raise ValueError('need Z >= 1 and a base matrix with more columns than rows (got Z=%d, base %s)' % (Z, base.shape))
        if base.min() < -1 or base.max() >= Z:
            raise ValueError('shifts must lie in [-1, Z) (got %d .. %d with Z=%d)' % (base.min(), base.max(), Z))
        if cols * Z > MAX_N:
            raise ValueError('at most %d code bits are supported (got %d)' % (MAX_N, cols * Z))
        self.base, self.Z = np.ascontiguousarray(base, np.int32), Z
        self.M, self.N = rows * Z, cols * Z
        self.K = self.N - self.M
        H = self.parity_check_matrix()
        dc = H.sum(axis=1)
        if dc.max() > MAX_CHECK_DEGREE or dc.min() < 2 or H.sum(axis=0).min() < 1:
            raise ValueError('check degrees must lie in [2, %d] and every bit in a check (got check degrees %d .. %d)'
                             % (MAX_CHECK_DEGREE, dc.min(), dc.max()))
        if not _gf2_invertible(H[:, self.K:]):
            raise ValueError('the parity part of the check matrix is singular over GF(2): no systematic encoder [payload; parity]')
        self.interleaver_seed = int(interleaver_seed)
        self.P = np.random.default_rng(self.interleaver_seed).permutation(self.N).astype(np.int32)
        self.R = np.empty_like(self.P)
        self.R[self.P] = np.arange(self.N, dtype=np.int32)
        self._handles = {}

    def parity_check_matrix(self):
        """Dense ``[M, N]`` uint8: block (r, c) is ``circshift(eye(Z), [0 s])``, row i's one in column (i + s) mod Z."""
        rows, cols = self.base.shape
        H = np.zeros((self.M, self.N), np.uint8)
        i = np.arange(self.Z)
        for r in range(rows):
            for c in range(cols):
                if self.base[r, c] > -1:
                    H[r * self.Z + i, c * self.Z + (i + self.base[r, c]) % self.Z] = 1
        return H

    def uses(self, num_streams):
        """Channel uses of one codeword, and the padded soft bits: ``floor(N / 2S)``, ``N - 2 S uses`` (testPackets.m:74-83)."""
        u = self.N // (2 * int(num_streams))
        return u, self.N - u * 2 * int(num_streams)

    def handle(self, device):
        import torch
        key = torch.device(device).index
        if key not in self._handles:
            h = C.c_void_p()
            d = _lib.sbc_link_code_desc(base=self.base.ctypes.data_as(C.c_void_p), interleaver=self.P.ctypes.data_as(C.c_void_p),
                                        rows=self.base.shape[0], cols=self.base.shape[1], Z=self.Z)
            with torch.cuda.device(device):
                _lib.check(_lib.lib().sbc_link_code_create(C.byref(d), C.byref(h)))
            self._handles[key] = h
        return self._handles[key]

    def close(self):
        for h in self._handles.values():
            _lib.lib().sbc_link_code_destroy(h)
        self._handles = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ldpc_11n_648(interleaver_seed=1111):
    """The reference's code: IEEE 802.11n, (648, 324), Z = 27 -- 88 blocks, 2376 edges, check degree <= 8, variable degree <= 12."""
    return Code(np.array(_BASE_11N_648, np.int32), 27, interleaver_seed)


# ---- host-side checks --------------------------------------------------------------------------------------------------------------
def check_streams(num_streams, mod_size=2):
    if int(mod_size) != 2:
        raise ValueError('only mod_size = 2 (QPSK) is supported, as in the reference (testPackets.m:7-8) (got %r)' % (mod_size,))
    if int(num_streams) not in STREAMS:
        raise ValueError('num_streams must be one of %s: the ML soft bits search all 4^S candidates (S = 8 would be 65 536) (got %r)'
                         % (STREAMS, num_streams))
    return int(num_streams)


def _device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('the link simulation needs a HIP device (there is no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def _device_of(*tensors):
    import torch
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return _device()


def _as_tensor(name, x, dtype, shape, device):
    """``x`` (tensor or array) as a contiguous device tensor of ``dtype`` and exactly ``shape`` (None entries: any size)."""
    import torch
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dim() != len(shape) or any(s is not None and s != n for s, n in zip(shape, x.shape)):
        raise ValueError('%s must have shape %s (got %s)' % (name, tuple('*' if s is None else s for s in shape), tuple(x.shape)))
    if dtype == torch.complex64:
        if not x.is_complex():
            raise ValueError('%s must be complex (got %s)' % (name, x.dtype))
    elif x.is_complex() or (dtype in (torch.uint8, torch.int32) and x.is_floating_point()):
        raise ValueError('%s must be %s (got %s)' % (name, dtype, x.dtype))
    return x.to(device=device, dtype=dtype).resolve_conj().contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device, stream):
    import torch
    return stream if stream is not None else torch.cuda.current_stream(device)


def _random(seed, snr_index, packet0, flags):
    return _lib.sbc_link_random(seed=int(seed) & (2 ** 64 - 1), packet0=int(packet0), snr_index=int(snr_index), flags=int(flags))


def _check_bits(name, t):
    if t.numel() and int(t.max()) > 1:
        raise ValueError('%s must hold bits 0 / 1' % name)


# ---- the stages ------------------------------------------------------------------------------------------------------------------
def encode(code, payload, num_streams=4, stream=None):
    """``payload`` ``[Npk, K]`` bits -> (codeword uint8 ``[Npk, N]``, symbols complex64 ``[Npk, uses, S]``): systematic encoding,
    interleaving, QPSK (testPackets.m:123-133).  Device tensors; asynchronous on ``stream``."""
    import torch
    S = check_streams(num_streams)
    device = _device_of(payload)
    pay = _as_tensor('payload', payload, torch.uint8, (None, code.K), device)
    _check_bits('payload', pay)
    Npk, (uses, _) = pay.shape[0], code.uses(S)
    cw = torch.empty((Npk, code.N), dtype=torch.uint8, device=device)
    sym = torch.empty((Npk, uses, S), dtype=torch.complex64, device=device)
    d = _lib.sbc_link_encode_desc(payload=_ptr(pay), codeword=_ptr(cw), symbols=_ptr(sym), Npk=Npk, S=S, rnd=_random(0, 0, 0, 0))
    with torch.cuda.device(device):
        s = _stream(device, stream)
        _lib.check(_lib.lib().sbc_link_encode(code.handle(device), C.byref(d), C.c_void_p(s.cuda_stream)))
        pay.record_stream(s)
    return cw, sym


def check_llr_args(code, sym_shape, Hp_ideal_shape, Hp_est_shape, idx_shape, noise_shape, noise_power):
    """Host-side checks of ``ml_llr`` that need no data."""
    if len(Hp_ideal_shape) != 3 or tuple(Hp_ideal_shape) != tuple(Hp_est_shape):
        raise ValueError('Hp_ideal and Hp_est must both be [pool, Nr, S] (got %s, %s)' % (tuple(Hp_ideal_shape), tuple(Hp_est_shape)))
    pool, Nr, S = Hp_ideal_shape
    check_streams(S)
    if pool < 1:
        raise ValueError('the channel pool must hold at least one channel (got %d)' % pool)
    if not 1 <= Nr <= MAX_NR:
        raise ValueError('Nr must lie in 1 .. %d (got %d)' % (MAX_NR, Nr))
    uses, _ = code.uses(S)
    if len(sym_shape) != 3 or tuple(sym_shape[1:]) != (uses, S):
        raise ValueError('symbols must be [Npk, %d, %d] (got %s)' % (uses, S, tuple(sym_shape)))
    Npk = sym_shape[0]
    if tuple(idx_shape) != (Npk, uses):
        raise ValueError('chan_index must be [%d, %d] (got %s)' % (Npk, uses, tuple(idx_shape)))
    if tuple(noise_shape) != (Npk, uses, Nr):
        raise ValueError('noise must be [%d, %d, %d] (got %s)' % (Npk, uses, Nr, tuple(noise_shape)))
    if not (np.isfinite(noise_power) and noise_power > 0):
        raise ValueError('noise_power must be finite and > 0 (got %r)' % (noise_power,))


def ml_llr(code, symbols, Hp_ideal, Hp_est, chan_index, noise, noise_power, clip=True, stream=None):
    """Received vectors ``y = Hp_ideal[idx] x + sqrt(noise_power) w`` and the exact ML soft bits of every stream and bit under
    ``Hp_ideal`` and under ``Hp_est`` (ComputeLLRMIMO 'ml'), flattened, padded, deinterleaved and (``clip``) clipped at 6
    (testPackets.m:160-200).  symbols ``[Npk, uses, S]``, Hp ``[pool, Nr, S]``, chan_index ``[Npk, uses]``, noise ``w``
    ``[Npk, uses, Nr]`` standard CN(0, 1).  Returns two float32 ``[Npk, N]`` device tensors."""
    import torch
    device = _device_of(symbols, Hp_ideal, Hp_est)
    check_llr_args(code, tuple(np.shape(symbols)), tuple(np.shape(Hp_ideal)), tuple(np.shape(Hp_est)), tuple(np.shape(chan_index)),
                   tuple(np.shape(noise)), float(noise_power))
    pool, Nr, S = np.shape(Hp_ideal)
    sym = _as_tensor('symbols', symbols, torch.complex64, (None, None, S), device)
    Hi = _as_tensor('Hp_ideal', Hp_ideal, torch.complex64, (pool, Nr, S), device)
    He = _as_tensor('Hp_est', Hp_est, torch.complex64, (pool, Nr, S), device)
    idx = _as_tensor('chan_index', chan_index, torch.int32, (sym.shape[0], sym.shape[1]), device)
    w = _as_tensor('noise', noise, torch.complex64, (sym.shape[0], sym.shape[1], Nr), device)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= pool):
        raise ValueError('chan_index out of range [0, %d)' % pool)
    Npk = sym.shape[0]
    out = [torch.empty((Npk, code.N), dtype=torch.float32, device=device) for _ in range(2)]
    d = _lib.sbc_link_llr_desc(symbols=_ptr(sym), Hp_ideal=_ptr(Hi), Hp_est=_ptr(He), chan_index=_ptr(idx), noise=_ptr(w),
                               llr_ideal=_ptr(out[0]), llr_est=_ptr(out[1]), noise_power=float(noise_power), Npk=Npk, pool=pool, Nr=Nr, S=S,
                               rnd=_random(0, 0, 0, 0 if clip else _lib.LINK_NO_CLIP))
    with torch.cuda.device(device):
        s = _stream(device, stream)
        _lib.check(_lib.lib().sbc_link_llr(code.handle(device), C.byref(d), C.c_void_p(s.cuda_stream)))
        for t in (sym, Hi, He, idx, w):
            t.record_stream(s)
    return out[0], out[1]


def decode(code, llr, max_iters=50, early_stop=True, want_totals=False, want_iters=False, stream=None):
    """Flooding sum-product decoding of ``llr`` ``[Npk, N]`` (positive = bit 0): soft outputs of the K payload bits float32
    ``[Npk, K]``, then (``want_totals``) the soft totals of all N bits and (``want_iters``) the iterations each codeword ran.  With
    ``early_stop`` a codeword stops after the first iteration whose hard decisions satisfy every check."""
    import torch
    if int(max_iters) < 1:
        raise ValueError('max_iters must be >= 1 (got %r)' % (max_iters,))
    device = _device_of(llr)
    l = _as_tensor('llr', llr, torch.float32, (None, code.N), device)
    Npk = l.shape[0]
    soft = torch.empty((Npk, code.K), dtype=torch.float32, device=device)
    totals = torch.empty((Npk, code.N), dtype=torch.float32, device=device) if want_totals else None
    iters = torch.empty((Npk,), dtype=torch.int32, device=device) if want_iters else None
    with torch.cuda.device(device):
        s = _stream(device, stream)
        _lib.check(_lib.lib().sbc_link_decode(code.handle(device), _ptr(l), Npk, int(max_iters), 1 if early_stop else 0, _ptr(soft),
                                              _ptr(totals), _ptr(iters), C.c_void_p(s.cuda_stream)))
        l.record_stream(s)
    return (soft,) + ((totals,) if want_totals else ()) + ((iters,) if want_iters else ()) if (want_totals or want_iters) else soft


def errors(code, soft, payload, stream=None):
    """Per packet (ber, bler) of ``payload_hat = (sign(-soft) + 1) / 2`` against ``payload`` (testPackets.m:206-222)."""
    import torch
    device = _device_of(soft, payload)
    sf = _as_tensor('soft', soft, torch.float32, (None, code.K), device)
    pay = _as_tensor('payload', payload, torch.uint8, (sf.shape[0], code.K), device)
    ber, bler = (torch.empty((sf.shape[0],), dtype=torch.float32, device=device) for _ in range(2))
    with torch.cuda.device(device):
        s = _stream(device, stream)
        _lib.check(_lib.lib().sbc_link_errors(code.handle(device), _ptr(sf), _ptr(pay), sf.shape[0], _ptr(ber), _ptr(bler),
                                              C.c_void_p(s.cuda_stream)))
        sf.record_stream(s)
        pay.record_stream(s)
    return ber, bler


def simulate_chunk(code, Hp_ideal, Hp_est, noise_power, n_packets, seed=0, snr_index=0, packet0=0, randomness=None, max_iters=50,
                   want_draws=False, stream=None):
    """One SNR point for one chunk of packets (``sbc_link_simulate``: encode -> soft bits -> decode x 2 -> errors).  ``randomness``:
    None -- the library's Philox streams keyed by (seed, snr_index, packet0 + position, purpose) -- or ``(payload, chan_index, noise)``
    caller buffers.  Returns a dict of device tensors: ``ber_ideal``, ``bler_ideal``, ``ber_est``, ``bler_est`` ``[n_packets]`` float32,
    ``iters_ideal``, ``iters_est`` int32, and with ``want_draws`` the ``payload``, ``chan_index`` and ``noise`` that were used."""
    import torch
    device = _device_of(Hp_ideal, Hp_est)
    if tuple(np.shape(Hp_ideal)) != tuple(np.shape(Hp_est)) or len(np.shape(Hp_ideal)) != 3:
        raise ValueError('Hp_ideal and Hp_est must both be [pool, Nr, S] (got %s, %s)' % (tuple(np.shape(Hp_ideal)), tuple(np.shape(Hp_est))))
    pool, Nr, S = np.shape(Hp_ideal)
    check_streams(S)
    if pool < 1 or not 1 <= Nr <= MAX_NR:
        raise ValueError('need a pool of at least one channel and Nr in 1 .. %d (got pool=%d, Nr=%d)' % (MAX_NR, pool, Nr))
    if not (np.isfinite(noise_power) and noise_power > 0):
        raise ValueError('noise_power must be finite and > 0 (got %r)' % (noise_power,))
    Npk, (uses, _) = int(n_packets), code.uses(S)
    Hi = _as_tensor('Hp_ideal', Hp_ideal, torch.complex64, (pool, Nr, S), device)
    He = _as_tensor('Hp_est', Hp_est, torch.complex64, (pool, Nr, S), device)
    if randomness is None:
        flags = _lib.LINK_DEVICE_RANDOM
        pay = torch.empty((Npk, code.K), dtype=torch.uint8, device=device)
        idx = torch.empty((Npk, uses), dtype=torch.int32, device=device)
        w = torch.empty((Npk, uses, Nr), dtype=torch.complex64, device=device) if want_draws else None
    else:
        flags = 0
        pay = _as_tensor('payload', randomness[0], torch.uint8, (Npk, code.K), device)
        idx = _as_tensor('chan_index', randomness[1], torch.int32, (Npk, uses), device)
        w = _as_tensor('noise', randomness[2], torch.complex64, (Npk, uses, Nr), device)
        _check_bits('payload', pay)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= pool):
            raise ValueError('chan_index out of range [0, %d)' % pool)
    res = {k: torch.empty((Npk,), dtype=torch.float32, device=device) for k in ('ber_ideal', 'bler_ideal', 'ber_est', 'bler_est')}
    res.update({k: torch.empty((Npk,), dtype=torch.int32, device=device) for k in ('iters_ideal', 'iters_est')})
    d = _lib.sbc_link_sim_desc(Hp_ideal=_ptr(Hi), Hp_est=_ptr(He), payload=_ptr(pay), chan_index=_ptr(idx), noise=_ptr(w),
                               noise_power=float(noise_power), Npk=Npk, pool=pool, Nr=Nr, S=S, max_iters=int(max_iters),
                               rnd=_random(seed, snr_index, packet0, flags), **{k: _ptr(v) for k, v in res.items()})
    with torch.cuda.device(device):
        s = _stream(device, stream)
        _lib.check(_lib.lib().sbc_link_simulate(code.handle(device), C.byref(d), C.c_void_p(s.cuda_stream)))
        for t in (Hi, He, pay, idx) + ((w,) if w is not None else ()):
            t.record_stream(s)
    if want_draws:
        res.update(payload=pay, chan_index=idx, noise=w)
    return res


def host_draws(code, seed, snr_index, packet0, n_packets, num_streams, pool, Nr):
    """The (payload, chan_index, noise) the device streams give these packets, replayed on the host (``noise.link_*``): the
    ``--noise host`` convention of this project."""
    packets = np.arange(int(packet0), int(packet0) + int(n_packets))
    uses, _ = code.uses(num_streams)
    return (_noise.link_payload(seed, snr_index, packets, code.K), _noise.link_indices(seed, snr_index, packets, uses, pool),
            _noise.link_noise(seed, snr_index, packets, uses, Nr))


def check_packets_args(real_shape, est_shape, mod_size, num_tx, num_rx, precoding, num_streams, num_packets, n_snr):
    """Host-side checks of ``simulate_packets`` that need no data (``ValueError`` on anything unsupported)."""
    check_streams(num_streams, mod_size)
    if precoding != 'random':
        raise ValueError('only precoding = \'random\' is implemented, as in the reference (testPackets.m:87-94) (got %r)' % (precoding,))
    if len(real_shape) != 3 or tuple(real_shape[:2]) != (num_rx, num_tx):
        raise ValueError('real_channels must be [num_rx, num_tx, pool] = [%d, %d, *] (got %s)' % (num_rx, num_tx, tuple(real_shape)))
    if real_shape[2] < 1:
        raise ValueError('the channel pool must hold at least one channel')
    if tuple(est_shape) != (n_snr,) + tuple(real_shape):
        raise ValueError('est_channels must be [len(snr_range), num_rx, num_tx, pool] = %s (got %s)'
                         % ((n_snr,) + tuple(real_shape), tuple(est_shape)))
    if not 1 <= num_rx <= MAX_NR:
        raise ValueError('num_rx must lie in 1 .. %d (got %d)' % (MAX_NR, num_rx))
    if int(num_packets) < 1:
        raise ValueError('num_packets must be >= 1 (got %r)' % (num_packets,))


def simulate_packets(real_channels, est_channels, mod_size, num_tx, num_rx, precoding, num_streams, num_packets, snr_range, run_ideal=True,
                     code=None, seed=1234, noise='device', chunk=16384, device=None, max_iters=50):
    """``testPackets`` of the reference: ``real_channels`` ``[num_rx, num_tx, pool]`` (the same at every data SNR), ``est_channels``
    ``[len(snr_range), num_rx, num_tx, pool]`` (per data-SNR point), QPSK (``mod_size`` 2), ``'random'`` precoding with ``num_streams``
    streams, ``num_packets`` codewords per point of ``snr_range`` (data SNR in dB; ``noise_power = 10^(-snr/10)``).

    Returns ``(bler_ideal, ber_ideal, bler_est, ber_est)``, float64 arrays of ``len(snr_range)`` -- per-packet rates averaged over
    the packets of a point (``run_ideal`` False: the two ideal curves are None).  ``noise``: ``'device'`` (the library's Philox streams)
    or ``'host'`` (the same streams replayed on the host and uploaded: equal payloads and picks, noise equal to fp32 rounding).
    Packets are simulated in chunks of ``chunk``; a packet's draws do not depend on the chunking."""
    import torch
    real_channels, est_channels = np.asarray(real_channels), np.asarray(est_channels)
    snr_range = np.atleast_1d(np.asarray(snr_range, np.float64))
    check_packets_args(real_channels.shape, est_channels.shape, mod_size, int(num_tx), int(num_rx), precoding, num_streams, num_packets,
                       len(snr_range))
    if noise not in ('device', 'host'):
        raise ValueError('noise must be \'device\' or \'host\' (got %r)' % (noise,))
    code = code if code is not None else ldpc_11n_648()
    device = torch.device(device) if device is not None else _device()
    S, pool = int(num_streams), real_channels.shape[2]
    # testPackets.m:88-89: one CN(0, 1) precoder [num_tx, S] per pool channel
    rng = np.random.Generator(np.random.Philox(key=[int(seed) & (2 ** 64 - 1), 3 << 32]))
    Pt = (rng.standard_normal((pool, num_tx, S, 2)) * np.sqrt(0.5)).view(np.complex128)[..., 0]
    Pt = torch.from_numpy(Pt.astype(np.complex64)).to(device)

    def precoded(Hc):                                     # [num_rx, num_tx, pool] -> Hp [pool, num_rx, S]  (plumbing, torch)
        Hc = torch.from_numpy(np.ascontiguousarray(np.moveaxis(Hc, 2, 0)).astype(np.complex64)).to(device)
        return torch.matmul(Hc, Pt).contiguous()
    Hp_ideal = precoded(real_channels)
    out = np.zeros((4, len(snr_range)))
    for si, snr in enumerate(snr_range):
        Hp_est = precoded(est_channels[si])
        sums = torch.zeros(4, dtype=torch.float64, device=device)
        for p0 in range(0, int(num_packets), int(chunk)):
            n = min(int(chunk), int(num_packets) - p0)
            draws = host_draws(code, seed, si, p0, n, S, pool, int(num_rx)) if noise == 'host' else None
            r = simulate_chunk(code, Hp_ideal, Hp_est, 10.0 ** (-snr / 10.0), n, seed=seed, snr_index=si, packet0=p0, randomness=draws,
                               max_iters=max_iters)
            sums += torch.stack([r[k].double().sum() for k in ('bler_ideal', 'ber_ideal', 'bler_est', 'ber_est')])
        out[:, si] = (sums / int(num_packets)).cpu().numpy()
    if not run_ideal:
        return None, None, out[2], out[3]
    return out[0], out[1], out[2], out[3]
