"""EM-GM-AMP as ``sbc_em_gm_amp_run`` defines it (include/sbc_hip.h), restated in numpy: the yardstick of
tests/test_gamp_cpu.py and tests/test_gpu_gamp.py, the way tests/cs_oracle.py stands in for sigpy.

The reference script (matlab/test_em_gm_amp.m) only *calls* ``EMGMAMP(...)`` from a MATLAB toolbox that is not in its tree, so this is
NOT a port of that toolbox: it is Bernoulli Gaussian-mixture GAMP with an EM-learned prior and noise variance, restated from the
published method, on the script's operator (:99-101), noise model (:112-113), schedule (:58-59, :67) and logs (:123-138).

Everything is batched over problems that share ``Np`` and runs in the dtype asked for: ``np.float64`` (complex128, the yardstick) or
``np.float32`` (complex64, the restatement whose own distance from float64 sets the bound of the GPU tests).  The keyword switches
of ``run`` (``onsager``, ``nr_factor``) exist for the mutation tests only.
"""
import numpy as np

SENTINEL = 1000.0          # complete_log's fill (test_em_gm_amp.m:71)
N_COMP = 4                 # Gaussian components of the heavy-tailed prior
PARAMS = 2 + 2 * N_COMP    # lambda, omega_1..4, phi_1..4, psi


def _ctype(rt):
    return np.complex64 if np.dtype(rt) == np.float32 else np.complex128


def idft_factor(n, rt=np.float64):
    """conj(dftmtx(n)) / n  (:37-38), evaluated in float64 and rounded to the working precision"""
    k = np.arange(n)
    return (np.exp(2j * np.pi * (np.outer(k, k) % n) / n) / n).astype(_ctype(rt))


def operator(P, nr, rt=np.float64):
    """A1 = P Fl [.., Np, Nt], a2 = |A1|^2, Fl, Fr: Y = A1 X Fr is full_A * fft2(H)(:) of :99-105"""
    ct = _ctype(rt)
    Fl, Fr = idft_factor(P.shape[-1], rt), idft_factor(nr, rt)
    A1 = np.matmul(P.astype(ct), Fl)
    a2 = (A1.real ** 2 + A1.imag ** 2).astype(rt)
    return A1, a2, Fl, Fr


def dense_operator(P, nr):
    """kron(right_idft, local_A * left_idft) of :101 for one pilot matrix, float64"""
    return np.kron(idft_factor(nr), P.astype(np.complex128) @ idft_factor(P.shape[-1]))


def _abs2(z):
    return z.real ** 2 + z.imag ** 2


def initial_state(A1, a2, Y, rt):
    B, Np, Nt = A1.shape
    Nr = Y.shape[-1]
    M = Np * Nr
    nY = _abs2(Y).sum((-1, -2)).astype(rt)
    nA = a2.sum((-1, -2)).astype(rt)
    lam = np.full(B, 0.5 * Np / Nt, rt)
    psi = nY / rt(101 * M)
    phibar = (nY - rt(M) * psi) / (nA * lam)
    om = np.full((B, N_COMP), 0.25, rt)
    phi = phibar[:, None] * (4.0 ** np.arange(N_COMP) * 4.0 / 85.0).astype(rt)[None, :]
    return dict(lam=lam, om=om, phi=phi, psi=psi, phibar=phibar,
                xhat=np.zeros((B, Nt, Nr), _ctype(rt)), taux=(lam * phibar)[:, None, None] * np.ones((B, Nt, Nr), rt),
                s=np.zeros((B, Np, Nr), _ctype(rt)), taus=np.zeros((B, Np), rt))


def gamp_iteration(st, A1, a2, Fr, Y, theta, first, onsager=True, nr_factor=True):
    """One GAMP iteration on the state ``st`` (updated in place); returns the quantities the EM step and the tests read."""
    rt = a2.dtype.type
    Nr = Fr.shape[0]
    with np.errstate(all='ignore'):
        taup = np.matmul(a2, st['taux'].sum(-1)[..., None])[..., 0] / rt(Nr * Nr)                  # [B, Np]
        z = np.matmul(np.matmul(A1, st['xhat']), Fr)
        phat = z - taup[..., None] * st['s'] if onsager else z
        den = taup + st['psi'][:, None]
        s_new = (Y - phat) / den[..., None]
        taus_new = 1 / den
        zhat = phat + taup[..., None] * s_new
        tauz = taup * st['psi'][:, None] / den
        if first:
            st['s'], st['taus'] = s_new, taus_new
        else:
            st['s'] = (1 - theta) * st['s'] + theta * s_new
            st['taus'] = (1 - theta) * st['taus'] + theta * taus_new
        st['s'] = st['s'].astype(A1.dtype)
        st['taus'] = st['taus'].astype(a2.dtype)
        taur = rt(Nr if nr_factor else 1) / np.matmul(np.swapaxes(a2, -1, -2), st['taus'][..., None])[..., 0]   # [B, Nt]
        back = np.matmul(np.matmul(np.conj(np.swapaxes(A1, -1, -2)), st['s']), np.conj(Fr.T))
        rhat = st['xhat'] + taur[..., None] * back
        # the denoiser, in the log domain
        r2 = _abs2(rhat)
        tr = taur[..., None]
        v = st['phi'][:, None, None, :] + tr[..., None]                                              # [B, Nt, Nr, 4]
        loga0 = np.log(1 - st['lam'])[:, None, None] - np.log(tr) - r2 / tr
        logal = np.log(st['lam'][:, None] * st['om'])[:, None, None, :] - np.log(v) - r2[..., None] / v
        mx = np.maximum(loga0, logal.max(-1))
        a0, al = np.exp(loga0 - mx), np.exp(logal - mx[..., None])
        beta = al / (a0 + al.sum(-1))[..., None]
        g = st['phi'][:, None, None, :] / v
        m = st['phi'][:, None, None, :] * tr[..., None] / v + g * g * r2[..., None]
        st['xhat'] = ((beta * g).sum(-1) * rhat).astype(A1.dtype)
        st['taux'] = ((beta * m).sum(-1) - _abs2(st['xhat'])).astype(a2.dtype)
    return dict(taup=taup, phat=phat, s_new=s_new, taus_new=taus_new, zhat=zhat, tauz=tauz, taur=taur, rhat=rhat, beta=beta, m=m)


def em_update(st, q, Y):
    rt = st['lam'].dtype.type
    B, Nt, Nr = st['xhat'].shape
    N = Nt * Nr
    with np.errstate(all='ignore'):
        sb = q['beta'].sum((1, 2))                                   # [B, 4]
        sbm = (q['beta'] * q['m']).sum((1, 2))
        spi = q['beta'].sum(-1).sum((1, 2))                          # [B]
        st['lam'] = np.clip(spi / rt(N), rt(1.0 / N), rt(1)).astype(rt)
        st['om'] = (sb / spi[:, None]).astype(rt)
        new = np.maximum(sbm / sb, rt(1e-12) * st['phibar'][:, None])
        st['phi'] = np.where(sb == 0, st['phi'], new).astype(rt)
        st['psi'] = ((_abs2(Y - q['zhat']) + q['tauz'][..., None]).mean((1, 2))).astype(rt)


def spatial(X, Fl, Fr):
    """ifft2(X) = Fl X Fr  (:119)"""
    return np.matmul(np.matmul(Fl, X), Fr)


def run(P, Y, H=None, nit=10, em_iters=200, tol=1e-1, theta=0.3, p_index=None, h_index=None, dtype=np.float64, onsager=True,
        nr_factor=True, return_crit=False):
    """``em_iters`` EM iterations of ``nit`` GAMP iterations for every problem b.  P [nP, Np, Nt], Y [B, Np, Nr], H [nH, Nt, Nr].
    Returns a dict: X, H_hat [B, Nt, Nr], params [B, 10], log [em_iters, B] (None without H), stop_iter [B] -- the number of EM
    iterations problem b ran -- and, with ``return_crit``, crit [em_iters, B] = ||x - x_prev||^2 / ||x||^2 of the rows that ran (NaN elsewhere)."""
    rt = np.dtype(dtype).type
    ct = _ctype(rt)
    B, Np, Nr = Y.shape
    pi = np.arange(B) if p_index is None else np.asarray(p_index)
    A1u, a2u, Fl, Fr = operator(np.asarray(P), Nr, rt)
    A1, a2 = A1u[pi], a2u[pi]
    Y = np.asarray(Y).astype(ct)
    if H is not None:
        Ht = np.asarray(H)[np.arange(B) if h_index is None else np.asarray(h_index)].astype(ct)
        hn = _abs2(Ht).sum((1, 2))
    st = initial_state(A1, a2, Y, rt)
    log = np.full((em_iters, B), SENTINEL, rt) if H is not None else None
    crit = np.full((em_iters, B), np.nan)
    stop_iter = np.full(B, em_iters, np.int32)
    keys = ('lam', 'om', 'phi', 'psi', 'phibar', 'xhat', 'taux', 's', 'taus')
    act = np.arange(B)
    first = True
    for k in range(em_iters):
        if act.size == 0:
            break
        sub = {key: st[key][act] for key in keys}
        prev = sub['xhat']
        for _ in range(nit):
            q = gamp_iteration(sub, A1[act], a2[act], Fr, Y[act], theta, first, onsager, nr_factor)
            first = False
        em_update(sub, q, Y[act])
        for key in keys:
            st[key][act] = sub[key]
        with np.errstate(all='ignore'):
            if H is not None:
                log[k, act] = _abs2(spatial(sub['xhat'], Fl, Fr) - Ht[act]).sum((1, 2)) / hn[act]
            dx, nx = _abs2(sub['xhat'] - prev).sum((1, 2)), _abs2(sub['xhat']).sum((1, 2))
            crit[k, act] = dx.astype(np.float64) / nx.astype(np.float64)
            stopped = dx < rt(tol) * nx if tol > 0 else np.zeros(act.size, bool)
        stop_iter[act[stopped]] = k + 1
        act = act[~stopped]
    out = dict(X=st['xhat'], H_hat=spatial(st['xhat'], Fl, Fr), log=log, stop_iter=stop_iter,
               params=np.concatenate([st['lam'][:, None], st['om'], st['phi'], st['psi'][:, None]], axis=1))
    if return_crit:
        out['crit'] = crit
    return out


def bound(f32, f64, factor=4.0, floor=8 * 2.0 ** -24):
    """The project's standing bound on a kernel's distance from float64: ``factor`` x the float32 restatement's own distance, and
    at least ``floor`` of the largest magnitude."""
    f64 = np.asarray(f64)
    scale = float(np.max(np.abs(f64))) if f64.size else 0.0
    own = float(np.max(np.abs(np.asarray(f32).astype(f64.dtype) - f64))) if f64.size else 0.0
    return max(factor * own, floor * scale), own, scale


def assert_within(name, got, f32, f64, factor=4.0, floor=8 * 2.0 ** -24):
    """``got`` is within ``bound(f32, f64)`` of ``f64`` elementwise -- the assertion helper of the GPU tests (and of the mutation
    tests, which hand it a deliberately wrong restatement as ``got``).  Returns (error, bound) for the figures a test prints."""
    f64 = np.asarray(f64)
    got = np.asarray(got)
    assert got.shape == f64.shape, '%s: shape %s, expected %s' % (name, got.shape, f64.shape)
    lim, own, scale = bound(f32, f64, factor, floor)
    assert np.all(np.isfinite(got)), '%s: not finite' % name
    err = float(np.max(np.abs(got.astype(f64.dtype) - f64))) if f64.size else 0.0
    assert err <= lim, '%s: error %.3e exceeds the bound %.3e (float32 restatement: %.3e, scale %.3e)' % (name, err, lim, own, scale)
    return err, lim
