"""CPU restatement of one L-DAMP training step (train_ldamp.py:107-141 of the reference) on top of tests/ldamp_oracle.py's layer
functions, with torch autograd, in float64 or float32: the unrolled loop of ``LDAMP.forward`` with the perturbed evaluation under
``no_grad``, loss = mean_b sum |h - H|^2, the logged NMSE, the gradient with respect to every tensor, ``torch.optim.Adam``.

Summation orders: ``axes=()`` is the native order; ``axes=(-2, -1)`` the flipped twin of ldamp_oracle (every filter and the input flipped,
the output flipped back: the identity in exact arithmetic, other bits in float32); ``(-2,)`` and ``(-1,)`` flip one axis only.

Imposed masks: the gradient of this net is discontinuous in the LeakyReLU signs, so two float32 evaluations of one input can differ by
1e-2 where one sign differs.  With ``masks`` (per unroll, stage name -> array of 1 / 0.2 for the clean images) every LeakyReLU of the
DIFFERENTIATED evaluation becomes a multiplication by that mask; the no_grad perturbed evaluation keeps its natural activation."""
import numpy as np
import torch
import torch.nn.functional as F

import ldamp_oracle as lo

NORMED = ('d0a', 'd0', 'd1a', 'd1', 'd2a', 'd2', 'ba', 'bb', 't0', 'u0a', 'u0', 't1', 'u1a', 'u1', 't2', 'u2a', 'u2')
SLOPE = 0.2


def act(y, mask):
    return F.leaky_relu(y, SLOPE) if mask is None else y * mask


def conv_half(x, w, mask=None):
    return act(F.instance_norm(F.conv2d(x, w, padding=1), eps=1e-5), mask)


def tconv_stage(x, w, mask=None):
    return act(F.instance_norm(F.conv_transpose2d(x, w, stride=2), eps=1e-5), mask)


def mask_of(y):
    """the 1 / 0.2 mask an activation was produced with (slope 0.2 > 0 keeps the sign; y = 0 counts as positive, as in the kernels)"""
    y = np.asarray(y)
    return np.where(y >= 0, 1.0, SLOPE)


def unet(W, x, masks=None, stages=None):
    """norm(x) ... 1x1 conv, unnorm, residual, on planes x [B, 2, 64, 16]; W: key (without 'update_nets.<u>.unet.') -> tensor"""
    st = {} if stages is None else stages
    m = (lambda k: None) if masks is None else (lambda k: masks[k])
    st['x'], mean, std = lo.norm(x)
    cur = st['x']
    for a, b, p, key in lo.DOWN:
        st[a] = conv_half(cur, W[key + '.layers.0.weight'], m(a))
        st[b] = conv_half(st[a], W[key + '.layers.4.weight'], m(b))
        st[p] = lo.pool(st[b])
        cur = st[p]
    st['ba'] = conv_half(cur, W['conv.layers.0.weight'], m('ba'))
    st['bb'] = conv_half(st['ba'], W['conv.layers.4.weight'], m('bb'))
    cur = st['bb']
    for t, a, b, skip, tkey, ckey in lo.UP:
        st[t] = tconv_stage(cur, W[tkey + '.layers.0.weight'], m(t))
        st[a] = conv_half(torch.cat([st[t], st[skip]], dim=1), W[ckey + '.layers.0.weight'], m(a))
        st[b] = conv_half(st[a], W[ckey + '.layers.4.weight'], m(b))
        cur = st[b]
    return lo.final(cur, W['up_conv.2.1.weight'], W['up_conv.2.1.bias'], mean, std, x)


def _flipw(w, axes):
    return torch.flip(w, axes) if (axes and w.dim() == 4 and w.shape[-1] > 1) else w


def denoiser(W, x, axes=(), masks=None, stages=None):
    """``unet`` in the summation order ``axes``; ``masks`` and ``stages`` are in the native orientation"""
    if not axes:
        return unet(W, x, masks, stages)
    fl = lambda t: torch.flip(t, axes)                                              # noqa: E731
    st = {}
    out = fl(unet({k: _flipw(w, axes) for k, w in W.items()}, fl(x).contiguous(),
                  None if masks is None else {k: fl(v).contiguous() for k, v in masks.items()}, st))
    if stages is not None:
        stages.update({k: (v if v.dim() < 4 else fl(v)) for k, v in st.items()})
    return out


def net_weights(params, u):
    pre = 'update_nets.%d.unet.' % u
    return {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}


def make_params(sd, dtype):
    return {k: lo._t(v, dtype).clone().requires_grad_(True) for k, v in sd.items()}


def forward(params, Y, P, eig, directions, num_unrolls, dtype, axes=(), masks=None, keep=None):
    """The loop of LDAMP.forward in train mode -> h (complex tensor with a graph).  ``keep``: a list that receives, per unroll, the dict
    of the clean evaluation's stage tensors plus 'r' (planes), 'h', 'z' (complex), 'div', 'eps'."""
    ctype = torch.complex64 if dtype == torch.float32 else torch.complex128
    y, Pm, e = lo._t(Y, ctype), lo._t(P, ctype), lo._t(eig, dtype)
    h = torch.zeros(y.shape[0], Pm.shape[-1], y.shape[-1], dtype=ctype, device=y.device)
    z = y
    for u in range(num_unrolls):
        W = net_weights(params, u)
        r = h + 1 / e[:, None, None] * torch.matmul(Pm.transpose(-1, -2).conj(), z)
        rr = torch.view_as_real(r)
        st = {}
        mk = None if masks is None else {k: lo._t(v, dtype) for k, v in masks[u].items()}
        hr = denoiser(W, rr.permute(0, 3, 1, 2), axes, mk, st).permute(0, 2, 3, 1).contiguous()
        with torch.no_grad():
            d = lo._t(directions[u], dtype)
            eps = torch.clamp(torch.amax(torch.abs(r), dim=(-1, -2)) * 1e-3, min=1e-5)
            rp = rr + eps[:, None, None, None] * d
            hp = denoiser(W, rp.permute(0, 3, 1, 2), axes).permute(0, 2, 3, 1).contiguous()
            div = 1 / eps * torch.mean(d * (hp - hr), dim=(-1, -2, -3))
        h = torch.view_as_complex(hr)
        z = y - torch.matmul(Pm, h) + z * div[:, None, None]
        if keep is not None:
            st.update(r=rr, h=h, z=z, div=div, eps=eps)
            keep.append(st)
    return h


def loss_nmse(h, H):
    err = torch.sum(torch.square(torch.abs(h - H)), dim=(-1, -2))
    return torch.mean(err), torch.mean(err / torch.sum(torch.square(torch.abs(H)), dim=(-1, -2)))


def step_gradients(sd, Y, P, eig, H, directions, num_unrolls, dtype=torch.float64, axes=(), masks=None, stage_grads=False):
    """One forward / backward.  Returns dict: loss, nmse (floats), grads (name -> float64 ndarray, nets 0 .. num_unrolls - 1), unrolls
    (per unroll: stage name -> ndarray of the clean evaluation; with ``stage_grads`` also 'g:<stage>' for the 4-D stages and r)."""
    ctype = torch.complex64 if dtype == torch.float32 else torch.complex128
    params = make_params(sd, dtype)
    keep = []
    h = forward(params, Y, P, eig, directions, num_unrolls, dtype, axes, masks, keep)
    if stage_grads:
        for st in keep:
            for k, v in st.items():
                if isinstance(v, torch.Tensor) and v.requires_grad and not v.is_complex():
                    v.retain_grad()
    loss, nmse = loss_nmse(h, lo._t(H, ctype))
    loss.backward()
    used = [k for k in sd if int(k.split('.')[1]) < num_unrolls]
    out = {'loss': float(loss.detach()), 'nmse': float(nmse.detach()), 'grads': {k: params[k].grad.numpy().astype(np.float64) for k in used}, 'unrolls': []}
    for st in keep:
        d = {k: v.detach().numpy() for k, v in st.items()}
        if stage_grads:
            d.update({'g:' + k: v.grad.numpy() for k, v in st.items() if isinstance(v, torch.Tensor) and v.grad is not None})
        out['unrolls'].append(d)
    return out


def natural_masks(res):
    """the masks of a step's own activations: what ``masks=`` takes to repeat that step's signs in another precision or order"""
    return [{k: mask_of(st[k]) for k in NORMED} for st in res['unrolls']]


def adam_reference(p0, grads, lrs, dtype=torch.float64):
    """torch.optim.Adam (defaults) on one flat tensor: p0, then one step per (grads[i], lrs[i]); returns the parameters after every step"""
    p = torch.nn.Parameter(torch.as_tensor(np.asarray(p0)).to(dtype).clone())
    opt = torch.optim.Adam([p], lr=1e-3)
    out = []
    for g, lr in zip(grads, lrs):
        for grp in opt.param_groups:
            grp['lr'] = lr
        p.grad = torch.as_tensor(np.asarray(g)).to(dtype)
        opt.step()
        out.append(p.detach().numpy().copy())
    return out, opt.state[p]['exp_avg'].numpy().copy(), opt.state[p]['exp_avg_sq'].numpy().copy()


def grad_error(a, ref):
    """norm-wise relative error of one tensor (or a concatenation)"""
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def per_net(grads, u):
    """the 19 gradients of net u concatenated, in state_dict order"""
    pre = 'update_nets.%d.' % u
    return np.concatenate([np.asarray(v, np.float64).ravel() for k, v in grads.items() if k.startswith(pre)])
