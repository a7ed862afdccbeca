"""numpy restatement of the reference's coded link simulation (matlab/testPackets.m, ComputeLLRMIMO.m 'ml' branch, and the
sum-product decoder behind comm.LDPCDecoder), parameterised by dtype:

* ``np.float64``: the yardstick -- the script's plain ``exp`` sums and the tanh / atanh check-node update;
* ``np.float32``: what the fp32 kernels are held to -- per-class log-sum-exp (smallest metric subtracted before ``exp``) and
  the exact pairwise form  a [+] b = sign(a) sign(b) min(|a|, |b|) + log1p(e^-|a+b|) - log1p(e^-|a-b|)  as a forward / backward
  recursion over a check's edges.  The distance of this restatement from the yardstick is the bound of the GPU tests.

Conventions (0-based): ``P`` the interleaver (``bitsInt = bitsEnc[P]``), ``R`` its inverse (``R[P] = arange(N)``); edges are
numbered check by check, inside a check by ascending column; a variable's edges by ascending check.  A sum over a variable's edges
is the running sum ``llr + m0 + m1 + ...`` in that order, as the kernel adds them."""
import itertools

import numpy as np

# IEEE 802.11n HT LDPC, N = 648, rate 1/2 (testPackets.m:29-42): circulant shifts, -1 = zero block
REF_Z = 27
REF_BASE = np.array([
    [0, -1, -1, -1, 0, 0, -1, -1, 0, -1, -1, 0, 1, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1],
    [22, 0, -1, -1, 17, -1, 0, 0, 12, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1],
    [6, -1, 0, -1, 10, -1, -1, -1, 24, -1, 0, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1],
    [2, -1, -1, 0, 20, -1, -1, -1, 25, 0, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1],
    [23, -1, -1, -1, 3, -1, -1, -1, 0, -1, 9, 11, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1],
    [24, -1, 23, 1, 17, -1, 3, -1, 10, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1, -1],
    [25, -1, -1, -1, 8, -1, -1, -1, 7, 18, -1, -1, 0, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1, -1],
    [13, 24, -1, -1, 0, -1, 8, -1, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1, -1],
    [7, 20, -1, 16, 22, 10, -1, -1, 23, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1, -1],
    [11, -1, -1, -1, 19, -1, -1, -1, 13, -1, 3, 17, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, -1],
    [25, -1, 8, -1, 23, 18, -1, 14, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0],
    [3, -1, -1, -1, 16, -1, -1, 2, 25, 5, -1, -1, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0]], np.int32)
# a small code: check degrees 3 and 4, lower-triangular parity part
SMALL_Z = 5
SMALL_BASE = np.array([[0, 1, -1, 0, -1, -1], [2, -1, 3, 0, 0, -1], [-1, 4, 1, -1, 0, 0]], np.int32)

# qammod(., 4, 'InputType', 'bit', 'UnitAveragePower', true): the pair's first bit is the MSB of the integer, and MATLAB's default
# Gray map sends the integers 0, 1, 2, 3 to these points
QPSK = np.array([-1 + 1j, -1 - 1j, 1 + 1j, 1 - 1j]) / np.sqrt(2.0)
CLIP = 6.0


def parity_check(base, Z):
    """testPackets.m:44-60: block (r, c) is ``circshift(eye(Z), [0 s])`` -- row i has its one in column (i + s) mod Z."""
    base = np.asarray(base)
    H = np.zeros((base.shape[0] * Z, base.shape[1] * Z), np.uint8)
    for r, c in itertools.product(range(base.shape[0]), range(base.shape[1])):
        if base[r, c] > -1:
            i = np.arange(Z)
            H[r * Z + i, c * Z + (i + base[r, c]) % Z] = 1
    return H


def inverse_permutation(P):
    R = np.empty_like(P)
    R[P] = np.arange(len(P))
    return R


def generator(H):
    """``G = B^-1 A`` over GF(2) for ``H = [A | B]`` (so that parity = G payload); ``ValueError`` when B is singular."""
    M, N = H.shape
    K = N - M
    aug = np.concatenate([H[:, K:], H[:, :K]], axis=1).astype(np.uint8)       # [B | A] -> [I | B^-1 A]
    for col in range(M):
        piv = np.nonzero(aug[col:, col])[0]
        if not len(piv):
            raise ValueError('the parity part of the check matrix is singular over GF(2)')
        p = col + piv[0]
        if p != col:
            aug[[col, p]] = aug[[p, col]]
        rows = np.nonzero(aug[:, col])[0]
        rows = rows[rows != col]
        aug[rows] ^= aug[col]
    return aug[:, M:]


def encode(H, payload):
    """``[payload; parity]`` with ``H c = 0`` (comm.LDPCEncoder); payload ``[..., K]`` of 0 / 1."""
    G = generator(H).astype(np.int64)
    payload = np.asarray(payload).astype(np.int64)
    parity = (payload @ G.T) % 2
    return np.concatenate([payload, parity], axis=-1).astype(np.uint8)


def modulate(codeword, P, S):
    """testPackets.m:126-133: interleave, drop the padded tail, QPSK; symbol k is stream k mod S of channel use k div S.
    Returns complex128 ``[..., uses, S]``."""
    N = codeword.shape[-1]
    uses = N // (2 * S)
    bits = codeword[..., P][..., :uses * 2 * S].astype(np.int64)
    sym = QPSK[2 * bits[..., 0::2] + bits[..., 1::2]]
    return sym.reshape(sym.shape[:-1] + (uses, S))


def candidates(S):
    """``[4^S, S]`` symbol integers of every transmit vector and the complex points; candidate c sends ``(c >> 2 s) & 3`` on stream s."""
    c = np.arange(4 ** S)
    ints = np.stack([(c >> (2 * s)) & 3 for s in range(S)], axis=1)
    return ints, QPSK[ints]


def ml_llr(y, Hp, noise_power, dtype=np.float64):
    """ComputeLLRMIMO 'ml': y ``[U, Nr]``, Hp ``[U, Nr, S]`` -> ``[U, S, 2]`` with
    ``log(sum_{bit = 0} exp(-|y - Hp s|^2 / noise_power) / sum_{bit = 1} ...)`` over all 4^S candidates.  float64: the script's sums
    as they stand (0 / 0 where they underflow); float32: log-sum-exp per class."""
    real = np.dtype(dtype)
    cplx = np.complex128 if real == np.float64 else np.complex64
    S = Hp.shape[-1]
    ints, pts = candidates(S)
    y, Hp, pts = np.asarray(y).astype(cplx), np.asarray(Hp).astype(cplx), pts.astype(cplx)
    cand = np.einsum('urs,cs->urc', Hp, pts).astype(cplx)
    d = y[:, :, None] - cand
    err = (d.real * d.real + d.imag * d.imag).sum(axis=1, dtype=real)                  # [U, ncand]
    npow = real.type(noise_power)
    out = np.zeros((y.shape[0], S, 2), real)
    for s in range(S):
        for b in range(2):
            one = ((ints[:, s] >> (1 - b)) & 1).astype(bool)
            if real == np.float64:
                sim = np.exp(-1.0 / npow * err)
                with np.errstate(divide='ignore', invalid='ignore'):
                    out[:, s, b] = np.log(sim[:, ~one].sum(axis=1) / sim[:, one].sum(axis=1))
            else:
                cls = []
                for m in (err[:, ~one], err[:, one]):
                    lo = m.min(axis=1, keepdims=True)
                    e = np.exp(((lo - m) / npow).astype(real)).astype(real)
                    cls.append((-lo[:, 0] / npow).astype(real) + np.log(e.sum(axis=1, dtype=real)).astype(real))
                out[:, s, b] = cls[0] - cls[1]
    return out


def finish_llr(llr, P, N, clip=True):
    """testPackets.m:166-178: flatten as bit + 2 stream + 2S use, pad with erasures, deinterleave with R, clip."""
    flat = llr.reshape(-1)
    flat = np.concatenate([flat, np.zeros(N - flat.size, flat.dtype)])[inverse_permutation(P)]
    if clip:
        big = np.abs(flat) >= CLIP
        flat[big] = CLIP * np.sign(flat[big])
        flat[np.isnan(flat)] = 0
    return flat


def received(sym, Hp_ideal, idx, w, noise_power, dtype=np.float64):
    """``y = Hp_ideal[idx] x + sqrt(noise_power) w`` for one packet: sym ``[U, S]``, w ``[U, Nr]`` standard CN(0, 1)."""
    cplx = np.complex128 if np.dtype(dtype) == np.float64 else np.complex64
    Hp = np.asarray(Hp_ideal)[idx].astype(cplx)
    y = np.einsum('urs,us->ur', Hp, np.asarray(sym).astype(cplx)).astype(cplx)
    return (y + np.dtype(dtype).type(np.sqrt(np.dtype(dtype).type(noise_power))) * np.asarray(w).astype(cplx)).astype(cplx)


class Graph:
    """Edge tables of a check matrix, padded to the largest degrees (pad slots point at a neutral element)."""

    def __init__(self, H):
        self.M, self.N = H.shape
        self.K = self.N - self.M
        rows, cols = np.nonzero(H)                     # row-major: check by check, ascending column
        self.E = len(rows)
        self.echeck, self.evar = rows, cols
        self.dc, self.dv = int(H.sum(1).max()), int(H.sum(0).max())
        self.cidx = np.full((self.M, self.dc), self.E, np.int64)
        fill = np.zeros(self.M, np.int64)
        for e, r in enumerate(rows):
            self.cidx[r, fill[r]] = e
            fill[r] += 1
        self.vidx = np.full((self.N, self.dv), self.E, np.int64)
        fill = np.zeros(self.N, np.int64)
        for e in np.lexsort((rows, cols)):             # a variable's edges by ascending check
            v = cols[e]
            self.vidx[v, fill[v]] = e
            fill[v] += 1


def boxplus(a, b):
    """The exact pairwise check-node form in the dtype of its operands.  +inf (the pad of a check with fewer edges than the largest
    degree) is the neutral element: a [+] inf = a, also where both operands are pads (the formula alone gives inf - inf = NaN
    there, which a check more than one edge short of the largest degree then carries into its backward recursion)."""
    t = a.dtype.type
    with np.errstate(invalid='ignore'):
        r = (np.sign(a) * np.sign(b) * np.minimum(np.abs(a), np.abs(b)) + np.log1p(np.exp(-np.abs(a + b)))
             - np.log1p(np.exp(-np.abs(a - b)))).astype(t)
    return np.where(b == np.inf, a, np.where(a == np.inf, b, r))


def _check_update(m, g, dtype):
    """m ``[B, M, dc]`` variable-to-check messages (pad: +inf) -> extrinsic check-to-variable messages."""
    dc = m.shape[-1]
    if np.dtype(dtype) == np.float64:
        t = np.tanh(m / 2)
        op = np.multiply
    else:
        t = m
        op = boxplus
    f, b = [t[..., 0]], [t[..., dc - 1]]
    for i in range(1, dc):
        f.append(op(f[-1], t[..., i]))
        b.append(op(b[-1], t[..., dc - 1 - i]))
    b = b[::-1]                                        # b[i] = t[i] op ... op t[dc - 1]
    out = np.empty_like(m)
    for i in range(dc):
        if i == 0:
            out[..., i] = b[1] if dc > 1 else t[..., 0]
        elif i == dc - 1:
            out[..., i] = f[dc - 2]
        else:
            out[..., i] = op(f[i - 1], b[i + 1])
    if np.dtype(dtype) == np.float64:
        with np.errstate(divide='ignore'):
            out = 2 * np.arctanh(out)
    return out


def decode(H_or_graph, llr, max_iters=50, early_stop=True, dtype=np.float64):
    """Flooding sum-product decoding of ``llr`` ``[B, N]``: returns (totals ``[B, N]``, iterations ``[B]``).  With ``early_stop`` a
    codeword stops after the first iteration whose hard decisions (total < 0 -> 1) satisfy every check."""
    g = H_or_graph if isinstance(H_or_graph, Graph) else Graph(H_or_graph)
    real = np.dtype(dtype).type
    llr = np.asarray(llr).astype(real)
    B = llr.shape[0]
    v2c = llr[:, g.evar].copy()
    totals = llr.copy()
    iters = np.zeros(B, np.int32)
    active = np.ones(B, bool)
    for _ in range(int(max_iters)):
        if not active.any():
            break
        a = np.nonzero(active)[0]
        padded = np.concatenate([v2c[a], np.full((len(a), 1), np.inf, real)], axis=1)
        c2v_c = _check_update(padded[:, g.cidx], g, dtype)                       # [b, M, dc]
        c2v = np.zeros((len(a), g.E + 1), real)
        c2v[:, g.cidx.reshape(-1)] = c2v_c.reshape(len(a), -1)
        c2v[:, g.E] = 0
        tot = llr[a].copy()
        for j in range(g.dv):
            tot = (tot + c2v[:, g.vidx[:, j]]).astype(real)
        v2c[a] = (tot[:, g.evar] - c2v[:, :g.E]).astype(real)
        totals[a] = tot
        iters[a] += 1
        if early_stop:
            hard = (tot < 0).astype(np.int64)
            syn = np.zeros((len(a), g.M), np.int64)
            np.add.at(syn, (slice(None), g.echeck), hard[:, g.evar])
            active[a[(syn % 2 == 0).all(axis=1)]] = False
    return totals, iters


def packet_errors(soft, payload):
    """testPackets.m:206-222: ``payload_hat = (sign(-out) + 1) / 2``; a soft output of exactly 0 is 0.5, an error."""
    hat = (np.sign(-np.asarray(soft, np.float64)) + 1) / 2
    wrong = hat != np.asarray(payload)
    return wrong.mean(axis=-1), wrong.any(axis=-1).astype(np.float64)


def chain(H, P, S, payload, idx, w, Hp_ideal, Hp_est, noise_power, dtype=np.float64, max_iters=50):
    """The packet loop of testPackets.m on given randomness: payload ``[Npk, K]``, idx ``[Npk, U]``, w ``[Npk, U, Nr]``.  Returns the
    clipped LLRs (ideal, est) ``[Npk, N]``, the decoders' totals and iteration counts, and per-packet (ber, bler) of both."""
    g = Graph(H)
    cw = encode(H, payload)
    sym = modulate(cw, P, S)
    out = {}
    llrs = {'ideal': [], 'est': []}
    for p in range(len(payload)):
        y = received(sym[p], Hp_ideal, idx[p], w[p], noise_power, dtype)
        for name, pool in (('ideal', Hp_ideal), ('est', Hp_est)):
            llrs[name].append(finish_llr(ml_llr(y, np.asarray(pool)[idx[p]], noise_power, dtype), P, g.N))
    for name in ('ideal', 'est'):
        llr = np.stack(llrs[name])
        tot, it = decode(g, llr, max_iters, True, dtype)
        ber, bler = packet_errors(tot[:, :g.K], payload)
        out[name] = {'llr': llr, 'totals': tot, 'iters': it, 'ber': ber, 'bler': bler}
    out['codeword'], out['symbols'] = cw, sym
    return out


def bpsk_awgn_llrs(H, snr_db, n, rng):
    """Clipped channel LLRs of ``n`` random codewords sent as BPSK (0 -> +1) over AWGN at Eb/N0 = ``snr_db``; also the payloads."""
    M, N = H.shape
    payload = rng.integers(0, 2, (n, N - M))
    cw = encode(H, payload)
    sigma2 = 10 ** (-snr_db / 10) / (2 * (N - M) / N)
    r = (1 - 2.0 * cw) + np.sqrt(sigma2) * rng.standard_normal(cw.shape)
    return np.clip(2 * r / sigma2, -CLIP, CLIP), payload
