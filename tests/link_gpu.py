"""The guarded launches of the sbc_link_* calls that tests/test_gpu_link.py and tests/test_gpu_link_shapes.py share: every operand of every
launch is a tests/guarded.py buffer, checked after the stream is synchronised.  The code handles are created once per process."""
import ctypes as C

import numpy as np
import torch

import link_cases as K
from guarded import Guard, NAN, ptr as _ptr

_codes = {}


def _code(name):
    from score_based_channels_amd import link
    if name not in _codes:
        H, P, base, Z = K.code(name)
        c = link.Code(base, Z, K.INTERLEAVER_SEED)
        assert np.array_equal(c.P, P) and np.array_equal(c.parity_check_matrix(), H)
        _codes[name] = c
    return _codes[name]


def _lib():
    from score_based_channels_amd import _lib
    return _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rnd(seed=0, snr_index=0, packet0=0, flags=0):
    return _lib().sbc_link_random(seed=seed, packet0=packet0, snr_index=snr_index, flags=flags)


def _c64(g, name, a):
    return g.inp(name, np.ascontiguousarray(a, np.complex64).view(np.float32).reshape(a.shape + (2,)))


def _cplx(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.complex64)[..., 0]


def gpu_encode(name, payload, S, random=False, seed=0, snr_index=0, packet0=0):
    """With ``random`` the payload comes from the device stream (``payload``: the number of packets) and is returned as well."""
    L, code, g = _lib(), _code(name), Guard(torch)
    Npk, (uses, _) = (payload if random else len(payload)), _code(name).uses(S)
    if random:
        pay = g.out('payload', (Npk, code.K), fill=7, dtype=torch.uint8)
    else:
        pay = g.inp('payload', np.ascontiguousarray(payload, np.uint8))
    cw = g.out('codeword', (Npk, code.N), fill=7, dtype=torch.uint8)
    sym = g.out('symbols', (Npk, uses, S, 2))
    d = L.sbc_link_encode_desc(payload=_ptr(pay), codeword=_ptr(cw), symbols=_ptr(sym), Npk=Npk, S=S,
                               rnd=_rnd(seed, snr_index, packet0, L.LINK_DEVICE_RANDOM) if random else _rnd())
    L.check(L.lib().sbc_link_encode(code.handle('cuda:0'), C.byref(d), _stream()))
    torch.cuda.synchronize()
    g.check()
    return (cw.cpu().numpy(), _cplx(sym)) + ((pay.cpu().numpy(),) if random else ())


def gpu_llr(name, sym, Hp, Hp_est, idx, w, noise_power, clip=True, fill=NAN):
    """``fill``: what the two outputs hold before the launch (NaN: every element must come back finite)."""
    L, code, g = _lib(), _code(name), Guard(torch)
    Npk, uses, S = sym.shape
    pool, Nr, _ = Hp.shape
    out = [g.out('llr_%s' % k, (Npk, code.N), fill=fill) for k in ('ideal', 'est')]
    d = L.sbc_link_llr_desc(symbols=_ptr(_c64(g, 'symbols', sym)), Hp_ideal=_ptr(_c64(g, 'Hp_ideal', Hp)), Hp_est=_ptr(_c64(g, 'Hp_est', Hp_est)),
                            chan_index=_ptr(g.inp('chan_index', np.ascontiguousarray(idx, np.int32))), noise=_ptr(_c64(g, 'noise', w)),
                            llr_ideal=_ptr(out[0]), llr_est=_ptr(out[1]), noise_power=noise_power, Npk=Npk, pool=pool, Nr=Nr, S=S,
                            rnd=_rnd(flags=0 if clip else L.LINK_NO_CLIP))
    L.check(L.lib().sbc_link_llr(code.handle('cuda:0'), C.byref(d), _stream()))
    torch.cuda.synchronize()
    g.check()
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def gpu_decode(name, llr, max_iters, early_stop):
    L, code, g = _lib(), _code(name), Guard(torch)
    Npk = len(llr)
    l = g.inp('llr', np.ascontiguousarray(llr, np.float32))
    soft, totals = g.out('soft', (Npk, code.K)), g.out('totals', (Npk, code.N))
    iters = g.out('iters', (Npk,), fill=-1, dtype=torch.int32)
    L.check(L.lib().sbc_link_decode(code.handle('cuda:0'), _ptr(l), Npk, max_iters, 1 if early_stop else 0, _ptr(soft), _ptr(totals), _ptr(iters),
                                    _stream()))
    torch.cuda.synchronize()
    g.check()
    return soft.cpu().numpy(), totals.cpu().numpy(), iters.cpu().numpy()


def gpu_errors(name, soft, payload):
    L, code, g = _lib(), _code(name), Guard(torch)
    Npk = len(soft)
    ber, bler = g.out('ber', (Npk,)), g.out('bler', (Npk,))
    L.check(L.lib().sbc_link_errors(code.handle('cuda:0'), _ptr(g.inp('soft', np.ascontiguousarray(soft, np.float32))),
                                    _ptr(g.inp('payload', np.ascontiguousarray(payload, np.uint8))), Npk, _ptr(ber), _ptr(bler), _stream()))
    torch.cuda.synchronize()
    g.check()
    return ber.cpu().numpy(), bler.cpu().numpy()


def gpu_simulate(Hp, Hp_est, noise_power, n, randomness=None, seed=0, snr_index=0, packet0=0, name='ref', code=None):
    """sbc_link_simulate on code ``name`` (``code``: another handle of it, such as a fresh one); with ``randomness`` None the draws come
    from the device streams and are returned.  Runs on torch's current stream."""
    L, code, g = _lib(), code if code is not None else _code(name), Guard(torch)
    pool, Nr, S = Hp.shape
    uses, _ = code.uses(S)
    if randomness is None:
        flags = L.LINK_DEVICE_RANDOM
        pay = g.out('payload', (n, code.K), fill=7, dtype=torch.uint8)
        idx = g.out('chan_index', (n, uses), fill=-1, dtype=torch.int32)
        w = g.out('noise', (n, uses, Nr, 2))
    else:
        flags = 0
        pay = g.inp('payload', np.ascontiguousarray(randomness[0], np.uint8))
        idx = g.inp('chan_index', np.ascontiguousarray(randomness[1], np.int32))
        w = _c64(g, 'noise', randomness[2])
    res = {k: g.out(k, (n,)) for k in ('ber_ideal', 'bler_ideal', 'ber_est', 'bler_est')}
    res.update({k: g.out(k, (n,), fill=-1, dtype=torch.int32) for k in ('iters_ideal', 'iters_est')})
    d = L.sbc_link_sim_desc(Hp_ideal=_ptr(_c64(g, 'Hp_ideal', Hp)), Hp_est=_ptr(_c64(g, 'Hp_est', Hp_est)), payload=_ptr(pay), chan_index=_ptr(idx),
                            noise=_ptr(w), noise_power=noise_power, Npk=n, pool=pool, Nr=Nr, S=S, max_iters=50,
                            rnd=_rnd(seed, snr_index, packet0, flags), **{k: _ptr(v) for k, v in res.items()})
    L.check(L.lib().sbc_link_simulate(code.handle('cuda:0'), C.byref(d), _stream()))
    torch.cuda.synchronize()
    g.check()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    out.update(payload=pay.cpu().numpy(), chan_index=idx.cpu().numpy(), noise=_cplx(w))
    return out
