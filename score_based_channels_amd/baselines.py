"""Classical channel-estimation baselines of Fig. 5c on the HIP library: Lasso / fsAD (lifted-DFT l1), ML (regularised
least squares) and EM-GM-AMP, batched over independent problems.

Thin wrappers over ``sbc_l1_lifted_run``, ``sbc_ls_regularized`` and ``sbc_em_gm_amp_run`` (include/sbc_hip.h).  torch only owns the
device memory and the stream; every number is computed by the HIP kernels (csrc/cs_l1.hip, csrc/cs_ls.hip, csrc/cs_gamp.hip).  Shapes, dtypes, indices and values
are checked here, on the host, before anything is launched.

Layouts (as in the reference scripts): pilots ``P`` ``[nP, Np, Nt]`` (``val_P``, the conj-transposed loader pilots), measurements
``Y`` ``[B, Np, Nr]``, channels ``H`` ``[nH, Nt, Nr]`` (``val_H``), complex64; ``p_index`` / ``h_index`` map problem ``b`` to its
pilot matrix and channel (default: ``b``).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

L1_NT, L1_NR, L1_LIFTINGS = 64, 16, (1, 2, 4)
LS_MAX_N, LS_MAX_NR, LS_MAX_DIM = 64, 64, 1024
GAMP_NT, GAMP_NR = 64, 16


def _device_of(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device('cuda', torch.cuda.current_device())


def _complex(name, x, ndim):
    if isinstance(x, np.ndarray):
        if not np.iscomplexobj(x):
            raise ValueError('%s must be complex (got %s)' % (name, x.dtype))
        x = torch.from_numpy(np.ascontiguousarray(x.astype(np.complex64)))
    if not isinstance(x, torch.Tensor) or x.dtype != torch.complex64:
        raise ValueError('%s must be a complex64 tensor or a complex ndarray (got %s)' % (name, getattr(x, 'dtype', type(x))))
    if x.dim() != ndim:
        raise ValueError('%s must have %d dimensions (got shape %s)' % (name, ndim, tuple(x.shape)))
    return x


def _upload(device, x):
    return x.to(device).resolve_conj().contiguous()


def _per_problem(name, v, B):
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(B, float(a))
    if a.shape != (B,):
        raise ValueError('%s must be a scalar or have shape (%d,) (got %s)' % (name, B, a.shape))
    return a


def _index(name, idx, B, n):
    if idx is None:
        if n != B:
            raise ValueError('%s is needed: %d problems but %d matrices' % (name, B, n))
        idx = np.arange(B)
    a = np.asarray(idx.cpu().numpy() if isinstance(idx, torch.Tensor) else idx)
    if a.shape != (B,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('%s must be an integer array of shape (%d,) (got %s %s)' % (name, B, a.dtype, a.shape))
    if B and (a.min() < 0 or a.max() >= n):
        raise ValueError('%s out of range [0, %d)' % (name, n))
    return torch.from_numpy(a.astype(np.int32))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def check_l1_args(P_shape, Y_shape, H_shape, lifting, steps):
    """Host-side checks of ``l1_lifted`` that need no data: raises ``ValueError`` on a shape or setting the kernel does not support."""
    if int(lifting) not in L1_LIFTINGS:
        raise ValueError('lifting must be one of %s (got %r)' % (L1_LIFTINGS, lifting))
    if int(steps) < 1:
        raise ValueError('steps must be >= 1 (got %r)' % (steps,))
    nP, Np, Nt = P_shape
    B, Npy, Nr = Y_shape
    nH, Nth, Nrh = H_shape
    if (Nt, Nr) != (L1_NT, L1_NR) or (Nth, Nrh) != (Nt, Nr):
        raise ValueError('l1_lifted supports Nt = %d, Nr = %d (got P %s, Y %s, H %s)' % (L1_NT, L1_NR, P_shape, Y_shape, H_shape))
    if Npy != Np or not 1 <= Np <= Nt:
        raise ValueError('need 1 <= Np <= Nt and Y with the pilots\' Np (got P %s, Y %s)' % (P_shape, Y_shape))


def l1_lifted(P, Y, H, lmbda, lr, lifting=4, steps=1000, p_index=None, h_index=None, want_x=False, stream=None):
    """``steps`` iterations of accelerated proximal gradient on the lifted-DFT l1 problem of every problem b
    (test_l1Fourier_lifted.py:125-190; semantics in include/sbc_hip.h).  ``lmbda`` / ``lr``: scalars or ``[B]``.

    Returns ``(log, H_hat)`` -- ``log`` float32 ``[steps, B]``, the NMSE of the new iterate after every step; ``H_hat`` complex64
    ``[B, Nt, Nr]`` -- or ``(log, H_hat, X)`` with ``X`` complex64 ``[B, L Nt, L Nr]`` when ``want_x``.  Device tensors; the launch
    is asynchronous on ``stream`` (default: the current stream)."""
    P, Y, H = _complex('P', P, 3), _complex('Y', Y, 3), _complex('H', H, 3)
    check_l1_args(tuple(P.shape), tuple(Y.shape), tuple(H.shape), lifting, steps)
    B = Y.shape[0]
    lam_np, lr_np = _per_problem('lmbda', lmbda, B), _per_problem('lr', lr, B)
    if not (np.all(np.isfinite(lam_np)) and np.all(lam_np >= 0)):
        raise ValueError('lmbda must be finite and >= 0')
    if not (np.all(np.isfinite(lr_np)) and np.all(lr_np > 0)):
        raise ValueError('lr must be finite and > 0')
    pidx = _index('p_index', p_index, B, P.shape[0])
    hidx = _index('h_index', h_index, B, H.shape[0])
    device = _device_of(P, Y, H)
    P, Y, H, pidx, hidx = (_upload(device, t) for t in (P, Y, H, pidx, hidx))
    lam = torch.from_numpy(lam_np.astype(np.float32)).to(device)
    lrt = torch.from_numpy(lr_np.astype(np.float32)).to(device)
    L, steps = int(lifting), int(steps)
    nt, nr = P.shape[2], Y.shape[2]
    log = torch.empty((steps, B), dtype=torch.float32, device=device)
    H_hat = torch.empty((B, nt, nr), dtype=torch.complex64, device=device)
    X = torch.empty((B, L * nt, L * nr), dtype=torch.complex64, device=device) if want_x else None
    d = _lib.sbc_l1_lifted_desc(P=_ptr(P), p_index=_ptr(pidx), Y=_ptr(Y), Htrue=_ptr(H), h_index=_ptr(hidx), lmbda=_ptr(lam),
                                lr=_ptr(lrt), nmse=_ptr(log), H_hat=_ptr(H_hat), X=_ptr(X), B=B, nP=P.shape[0], nH=H.shape[0],
                                Nt=nt, Nr=nr, Np=P.shape[1], lifting=L, steps=steps)
    with torch.cuda.device(device):
        s = stream if stream is not None else torch.cuda.current_stream(device)
        _lib.check(_lib.lib().sbc_l1_lifted_run(C.byref(d), C.c_void_p(s.cuda_stream)))
        # the inputs must outlive the asynchronous launch
        for t in (P, Y, H, pidx, hidx, lam, lrt):
            t.record_stream(s)
    return (log, H_hat, X) if want_x else (log, H_hat)


def check_em_gm_amp_args(P_shape, Y_shape, H_shape, nit, em_iters, tol, theta):
    """Host-side checks of ``em_gm_amp`` that need no data: raises ``ValueError`` on everything ``sbc_em_gm_amp_run`` excludes.
    ``H_shape``: None when there is no reference channel."""
    if int(nit) != nit or int(nit) < 1:
        raise ValueError('nit must be an integer >= 1 (got %r)' % (nit,))
    if int(em_iters) != em_iters or int(em_iters) < 1:
        raise ValueError('em_iters must be an integer >= 1 (got %r)' % (em_iters,))
    if not 0 < float(theta) <= 1:
        raise ValueError('theta must be in (0, 1] (got %r)' % (theta,))
    if not (np.isfinite(float(tol)) and float(tol) >= 0):
        raise ValueError('tol must be finite and >= 0 (got %r)' % (tol,))
    nP, Np, Nt = P_shape
    B, Npy, Nr = Y_shape
    if (Nt, Nr) != (GAMP_NT, GAMP_NR):
        raise ValueError('em_gm_amp supports Nt = %d, Nr = %d (got P %s, Y %s)' % (GAMP_NT, GAMP_NR, P_shape, Y_shape))
    if H_shape is not None and tuple(H_shape[1:]) != (Nt, Nr):
        raise ValueError('H must be [nH, %d, %d] (got %s)' % (Nt, Nr, tuple(H_shape)))
    if Npy != Np or not 1 <= Np <= Nt:
        raise ValueError('need 1 <= Np <= Nt and Y with the pilots\' Np (got P %s, Y %s)' % (P_shape, Y_shape))


def em_gm_amp(P, Y, H, nit=10, em_iters=200, tol=1e-1, theta=0.3, p_index=None, h_index=None, want_x=False, want_params=False,
              stream=None):
    """EM-GM-AMP on every problem b (matlab/test_em_gm_amp.m; the algorithm is the one defined in include/sbc_hip.h, restated from the
    published method -- the MATLAB toolbox the script calls is not reproduced): ``em_iters`` EM iterations of ``nit`` damped GAMP
    iterations, stopping early per problem at ``tol`` (0: never).  ``H``: the reference channels, or None (then there is no log).

    Returns ``(log, H_hat, stop_iter)`` -- ``log`` float32 ``[em_iters, B]``, the NMSE after every EM iteration that ran and the
    script's sentinel 1000 behind a stop (None without ``H``); ``H_hat`` complex64 ``[B, Nt, Nr]``; ``stop_iter`` int32 ``[B]``, the EM
    iterations run -- followed by ``X`` complex64 ``[B, Nt, Nr]`` (the estimate of fft2(H)) when ``want_x`` and by ``params`` float32
    ``[B, 10]`` (lambda, omega_1..4, phi_1..4, psi) when ``want_params``.  Device tensors; asynchronous on ``stream``."""
    P, Y = _complex('P', P, 3), _complex('Y', Y, 3)
    if H is not None:
        H = _complex('H', H, 3)
    check_em_gm_amp_args(tuple(P.shape), tuple(Y.shape), tuple(H.shape) if H is not None else None, nit, em_iters, tol, theta)
    B, nit, em_iters = Y.shape[0], int(nit), int(em_iters)
    pidx = _index('p_index', p_index, B, P.shape[0])
    hidx = _index('h_index', h_index, B, H.shape[0]) if H is not None else None
    device = _device_of(P, Y, H)
    P, Y, pidx = _upload(device, P), _upload(device, Y), _upload(device, pidx)
    if H is not None:
        H, hidx = _upload(device, H), _upload(device, hidx)
    nt, nr = P.shape[2], Y.shape[2]
    log = torch.empty((em_iters, B), dtype=torch.float32, device=device) if H is not None else None
    H_hat = torch.empty((B, nt, nr), dtype=torch.complex64, device=device)
    stop_iter = torch.empty((B,), dtype=torch.int32, device=device)
    X = torch.empty((B, nt, nr), dtype=torch.complex64, device=device) if want_x else None
    params = torch.empty((B, 10), dtype=torch.float32, device=device) if want_params else None
    d = _lib.sbc_em_gm_amp_desc(P=_ptr(P), p_index=_ptr(pidx), Y=_ptr(Y), Htrue=_ptr(H), h_index=_ptr(hidx), nmse=_ptr(log),
                                H_hat=_ptr(H_hat), X=_ptr(X), params=_ptr(params), stop_iter=_ptr(stop_iter), B=B, nP=P.shape[0],
                                nH=H.shape[0] if H is not None else 0, Nt=nt, Nr=nr, Np=P.shape[1], nit=nit, em_iters=em_iters,
                                theta=float(theta), tol=float(tol))
    with torch.cuda.device(device):
        s = stream if stream is not None else torch.cuda.current_stream(device)
        _lib.check(_lib.lib().sbc_em_gm_amp_run(C.byref(d), C.c_void_p(s.cuda_stream)))
        for t in (P, Y, pidx) + ((H, hidx) if H is not None else ()):
            t.record_stream(s)
    return (log, H_hat, stop_iter) + ((X,) if want_x else ()) + ((params,) if want_params else ())


def ls_regularized(P, Y, noise_var, H=None, p_index=None, h_index=None, stream=None):
    """Per problem b, ``H_hat = (P^H P + noise_var I_Nt)^-1 P^H Y`` (test_ml.py:132-138), solved in its equivalent form of size
    min(Np, Nt) by an fp32 Cholesky factorisation.  ``noise_var``: scalar or ``[B]``, > 0.  Returns ``(H_hat, nmse)`` -- complex64
    ``[B, Nt, Nr]`` and, when ``H`` is given, float32 ``[B]`` NMSE against ``H[h_index]`` (else ``None``)."""
    P, Y = _complex('P', P, 3), _complex('Y', Y, 3)
    nP, Np, Nt = P.shape
    B, Npy, Nr = Y.shape
    if Npy != Np:
        raise ValueError('Y must have the pilots\' Np (got P %s, Y %s)' % (tuple(P.shape), tuple(Y.shape)))
    if min(Np, Nt) > LS_MAX_N or Nr > LS_MAX_NR or max(Np, Nt) > LS_MAX_DIM:
        raise ValueError('ls_regularized supports min(Np, Nt) <= %d, Nr <= %d, Np, Nt <= %d (got P %s, Y %s)'
                         % (LS_MAX_N, LS_MAX_NR, LS_MAX_DIM, tuple(P.shape), tuple(Y.shape)))
    nv_np = _per_problem('noise_var', noise_var, B)
    if not (np.all(np.isfinite(nv_np)) and np.all(nv_np > 0)):
        raise ValueError('noise_var must be finite and > 0 (the regularised system is only solved for s2 > 0)')
    pidx = _index('p_index', p_index, B, nP)
    hidx = None
    if H is not None:
        H = _complex('H', H, 3)
        if tuple(H.shape[1:]) != (Nt, Nr):
            raise ValueError('H must be [nH, %d, %d] (got %s)' % (Nt, Nr, tuple(H.shape)))
        hidx = _index('h_index', h_index, B, H.shape[0])
    device = _device_of(P, Y, H)
    P, Y, pidx = _upload(device, P), _upload(device, Y), _upload(device, pidx)
    if H is not None:
        H, hidx = _upload(device, H), _upload(device, hidx)
    nv = torch.from_numpy(nv_np.astype(np.float32)).to(device)
    H_hat = torch.empty((B, Nt, Nr), dtype=torch.complex64, device=device)
    nmse = torch.empty((B,), dtype=torch.float32, device=device) if H is not None else None
    d = _lib.sbc_ls_desc(P=_ptr(P), p_index=_ptr(pidx), Y=_ptr(Y), noise_var=_ptr(nv), Htrue=_ptr(H), h_index=_ptr(hidx),
                         H_hat=_ptr(H_hat), nmse=_ptr(nmse), B=B, nP=nP, nH=H.shape[0] if H is not None else 0, Nt=Nt, Nr=Nr, Np=Np)
    with torch.cuda.device(device):
        s = stream if stream is not None else torch.cuda.current_stream(device)
        _lib.check(_lib.lib().sbc_ls_regularized(C.byref(d), C.c_void_p(s.cuda_stream)))
        for t in (P, Y, nv, pidx) + ((H, hidx) if H is not None else ()):
            t.record_stream(s)
    return H_hat, nmse
