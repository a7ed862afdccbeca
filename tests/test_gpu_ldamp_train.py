"""GPU tests of L-DAMP training (csrc/ldamp_train.hip behind ldamp.Trainer): the forward against the inference run, the LeakyReLU signs,
every kind of backward launch alone, the assembled gradient, Adam alone, and the properties a training loop relies on.

Rule R (as tests/test_gpu_wgan_train.py): norm of (kernel - float64) <= 4 x e_ref, e_ref the larger such norm of the float32 oracle's two
summation orders (tests/ldamp_train_oracle.py: native and spatially flipped).

The gradient of this net is not continuous in the LeakyReLU signs: one sign that differs moves a parameter gradient by
1e-3 .. 1e-2, so the raw gradient of two valid float32 evaluations is bimodal against float64.  Hence: the forward is held bit for bit to
sbc_ldamp_run (which the inference tests hold to float64); the kernel's signs may differ from float64's only where the normalised value is
within 8 x the float32 oracles' own distance from float64; and every gradient is held to float64 UNDER THE KERNEL'S OWN MASKS.  Per tensor
at 1, 2, 3 unrolls, per net (19 tensors concatenated) at 10: tests/test_ldamp_train_cpu.py shows other float32 orders keep these rules.

Measured on 1x MI355X (the tests print every figure): worst error / e_ref 2.51 of the 4 allowed over the single launches, 2.16 over the
per-tensor gradients, 0.85 per net at ten unrolls, 1.01 for Adam; no sign differs from float64's; the fixture's three losses are off by
1.2e-4, 1.7e-4 and 3.6e-2 where 2.0e-3, 1.0e-1 and 3.5e-1 are allowed.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ldamp_oracle as lo
import ldamp_train_cases as cases
import ldamp_train_oracle as T
from conftest import ROOT, load_golden
from score_based_channels_amd import _lib, ldamp

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rule_r(what, got, r64, *r32):
    wide = lambda a: np.asarray(a).astype(np.complex128 if np.iscomplexobj(a) else np.float64).ravel()           # noqa: E731
    n = lambda a: float(np.linalg.norm(wide(a) - wide(r64)))                        # noqa: E731
    err, e_ref, scale = n(got), max(n(r) for r in r32), float(np.linalg.norm(wide(r64)))
    print('%-60s err %.2e  e_ref %.2e  (|ref| %.2e)  ratio %.2f' % (what, err, e_ref, scale, err / max(e_ref, 1e-300)))
    assert np.shape(got) == np.shape(r64) and err <= cases.FACTOR * e_ref, (what, err, e_ref)


class GuardedTrainer(ldamp.Trainer):
    """The trainer with ``DeviceHandle._workspace_of`` overridden: a workspace of EXACTLY the floats the library asks for, NaN-filled (the
    library promises nothing about what it holds), between pads of at least one sample's stride (tests/guarded.py)."""
    guard, _n = None, None

    def _workspace_of(self, n, dev):
        from guarded import Guard
        if self.guard is None or self._n != int(n):
            self.guard, self._n = Guard(torch), int(n)
            self._ws = self.guard.out('trainer workspace (%d floats)' % n, (int(n),), must_write=False, pad=2 * 1024 * 1024)
        return self._ws

    def check_guards(self):
        torch.cuda.synchronize()
        self.guard.check()


class Case:
    """one gradient-only step of a guarded trainer on the shared problem, and what the oracles say about it under the kernel's own masks"""

    def __init__(self, B, Np, U):
        self.B, self.Np, self.U = B, Np, U
        self.sd, self.Y, self.P, self.eig, self.H, self.dirs = cases.problem(B, Np, U)
        self.sample = cases.torch_sample(self.Y, self.P, self.eig, self.H)
        self.tr = GuardedTrainer({'max_unrolls': U}, self.sd, capacity=B)
        (self.loss, self.nmse), logs = self.tr.step(self.sample, U, directions=self.dirs, update=False, return_logs=True)
        self.tr.check_guards()
        self.logs = {k: v.cpu().numpy() for k, v in logs.items()}
        self.masks = [{k: T.mask_of(self.tr.stage(k, u)[:B].cpu().numpy()) for k in T.NORMED} for u in range(U)]
        self.grads = self.tr.gradients()

    @functools.lru_cache(maxsize=None)
    def masked(self, dtype, order='native', stage_grads=False):
        return cases.oracle(self.B, self.Np, self.U, dtype, order, self.masks, stage_grads)

    @functools.lru_cache(maxsize=None)
    def natural(self, dtype, order='native'):
        return cases.oracle(self.B, self.Np, self.U, dtype, order)

    def fwd(self, name, u):
        """a clean forward stage as the kernel left it"""
        return self.tr.stage(name, u)[:self.B].cpu().numpy()

    def g(self, name, u):
        return self.tr.grad(name, u).cpu().numpy()

    def w(self, key, u):
        return self.sd['update_nets.%d.unet.%s' % (u, key)]

    def gw(self, key, u):
        return self.grads['update_nets.%d.unet.%s' % (u, key)]


@functools.lru_cache(maxsize=None)
def case(B, Np, U):
    return Case(B, Np, U)


SMALL = [(1, 1, 1), (3, 38, 2), (4, 64, 3)]


# ---- 1. forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Np,U', SMALL)
def test_training_forward_is_the_inference_run_bit_for_bit(B, Np, U):
    c = case(B, Np, U)
    model = ldamp.LDAMP({'max_unrolls': U}).load_state_dict(c.sd)
    for u in range(U):                                   # the run keeps the stages of its last unroll only
        _, logs = model(c.sample, u + 1, directions=c.dirs[:u + 1], return_logs=True)
        torch.cuda.synchronize()
        for k in ('h', 'z', 'div', 'eps'):
            assert same_bits(logs[k].cpu().numpy(), c.logs[k][:u + 1]), (k, u)
        for name in ldamp.STAGES:
            assert same_bits(model.stage(name).cpu().numpy(), c.tr.stage(name, u).cpu().numpy()), (name, u)
    assert same_bits(c.tr.stage('div', U - 1).cpu().numpy(), c.logs['div'][U - 1])
    n64, n32 = c.natural(F64), [c.natural(F32), c.natural(F32, 'flipped')]
    rule_r('loss', c.loss, n64['loss'], *[r['loss'] for r in n32])
    rule_r('nmse', c.nmse, n64['nmse'], *[r['nmse'] for r in n32])
    for name in T.NORMED:                                # the stored rstd is the norm's: 1 / sqrt(var + eps) of the convolution output
        r = c.tr.stage('rstd:' + name, U - 1).cpu().numpy()
        assert r.shape == (2 * B, c.fwd(name, U - 1).shape[1]) and np.all(np.isfinite(r)) and np.all(r > 0), name


def test_first_loss_is_the_reference_fixtures():
    """Step 0 of the fixture run (B = 4, Np = 38, 2 unrolls): rule R with the reference's own float32 run among the float32 evaluations."""
    g = load_golden('ldamp_train_step.npz')
    c = case(4, 38, 2)
    assert same_bits(c.Y, g['Y_herm']) and same_bits(c.dirs, g['directions'][0].astype(np.float32)) and same_bits(c.H, g['H_herm_cplx'])
    n32 = [c.natural(F32), c.natural(F32, 'flipped')]
    rule_r('loss against the reference', c.loss, g['loss64'][0], g['loss32'][0], *[r['loss'] for r in n32])
    rule_r('nmse against the reference', c.nmse, g['nmse64'][0], g['nmse32'][0], *[r['nmse'] for r in n32])


# ---- 2. masks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Np,U', SMALL)
def test_kernel_signs_differ_from_float64_only_near_zero(B, Np, U):
    """tau = 8 x the larger max-abs distance of the two float32 oracle orders from float64 on that stage's normalised values: a margin over
    the oracle's own error (rule R's 4, doubled because a maximum over one run underestimates the tail), never over the kernel's."""
    c = case(B, Np, U)
    unleak = lambda y: np.where(y >= 0, y, y / T.SLOPE)                             # noqa: E731
    n64, n32 = c.natural(F64), [c.natural(F32), c.natural(F32, 'flipped')]
    for u in range(U):
        for name in T.NORMED:
            x64 = unleak(n64['unrolls'][u][name])
            tau = 8 * max(np.max(np.abs(unleak(r['unrolls'][u][name]) - x64)) for r in n32)
            differ = c.masks[u][name] != T.mask_of(x64)
            near = np.abs(x64) <= tau
            print('unroll %d %-4s: %d signs differ, %d of %d values within tau = %.1e' % (u, name, differ.sum(), near.sum(), x64.size, tau))
            assert not np.any(differ & ~near), (u, name)


# ---- 3. single backward launches on the kernel's own inputs ----------------------------------------------------------------------------------
def layer_grads(fn, inputs, gout, dtype, flipped=False, mask=None, planes=True):
    """autograd of ``fn(*inputs, mask=, flipped=)`` against the upstream gradient ``gout`` in ``dtype``.  ``flipped``: the other summation
    order -- with ``planes``, every [N, C, H, W] operand with H, W > 1, the mask and the output are flipped in H and W (the twin of
    tests/ldamp_oracle.py); a function of other layouts (``planes=False``) flips for itself."""
    sp = lambda t: planes and torch.is_tensor(t) and t.dim() == 4 and t.shape[-1] > 1 and t.shape[-2] > 1          # noqa: E731
    fl = (lambda t: torch.flip(t, (-2, -1)) if sp(t) else t) if flipped else (lambda t: t)
    xs = [lo._t(a, dtype).clone().requires_grad_(True) for a in inputs]
    out = fl(fn(*[fl(x) for x in xs], mask=None if mask is None else fl(lo._t(mask, dtype)), flipped=flipped))
    out.backward(lo._t(gout, dtype))
    return [x.grad.numpy() for x in xs]


def check_layer(what, fn, inputs, gout, got, mask=None, add=None, planes=True):
    """rule R of every output of one backward launch; ``got``: the kernel's gradients, one per input (None: not an output of the launch);
    ``add``: per input, a float64 array the launch adds to that gradient (the pool's share of a skip tensor) or None"""
    r64 = layer_grads(fn, inputs, gout, F64, False, mask, planes)
    r32 = [layer_grads(fn, inputs, gout, F32, f, mask, planes) for f in (False, True)]
    for i, gk in enumerate(got):
        if gk is not None:
            a = 0 if (add is None or add[i] is None) else add[i]
            rule_r('%s input %d' % (what, i), gk, r64[i] + a, r32[0][i].astype(np.float64) + a, r32[1][i].astype(np.float64) + a)


def half(x, w, mask, flipped):
    return T.conv_half(x, w, mask)


def cat_half(a, b, w, mask, flipped):
    return T.conv_half(torch.cat([a, b], 1), w, mask)


def thalf(x, w, mask, flipped):
    return T.tconv_stage(x, w, mask)


def fin(u2, w, b, st, mask, flipped):
    """-(conv1x1(u2) std + mean): the part of h = r - (...) that the finish differentiates; st [B, 4] = (mean_re, std_re, mean_im, std_im)"""
    return -(F.conv2d(u2, w, b) * st[:, 1::2, None, None] + st[:, 0::2, None, None])


def nrm(rr, mask, flipped):
    """r [B, 64, 16, 2] -> (x, mean, std, r) flattened: what the gradients of S_X, S_STAT and the direct path multiply"""
    B = rr.shape[0]
    x, mean, std = lo.norm((torch.flip(rr, (1, 2)) if flipped else rr).permute(0, 3, 1, 2))
    x = torch.flip(x, (-2, -1)) if flipped else x
    return torch.cat([x.reshape(B, -1), mean.reshape(B, -1), std.reshape(B, -1), rr.reshape(B, -1)], 1)


def cplx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def gz32(c, u, flipped):
    """gz_u in float32 from the kernel's own float32 inputs, summing over the antennas forwards or backwards"""
    dr = cplx(c.g('r', u)).astype(np.complex64)
    s = (np.flip(c.P, 2) @ np.flip(dr, 1)) if flipped else (c.P @ dr)
    out = (s / c.eig[:, None, None]).astype(np.complex64)
    if u < c.U - 1:
        out = out + c.logs['div'][u][:, None, None] * cplx(c.g('gz', u + 1)).astype(np.complex64)
    return out.astype(np.complex64)


@pytest.mark.parametrize('B,Np,U', SMALL)
def test_backward_launches_alone(B, Np, U):
    c = case(B, Np, U)
    for u in sorted({0, U - 1}):
        m = c.masks[u]
        W = lambda k: (c.w(k, u), c.gw(k, u))                                        # noqa: E731
        up = lambda g: 0.25 * np.repeat(np.repeat(g.astype(np.float64), 2, axis=2), 2, axis=3)           # noqa: E731
        # 3 x 3 stages: last of the net, first of the net, bottleneck
        for out, inp, key in (('u2', 'u2a', 'up_conv.2.0.layers.4.weight'), ('d0a', 'x', 'down_sample_layers.0.layers.0.weight'),
                              ('ba', 'p2', 'conv.layers.0.weight'), ('bb', 'ba', 'conv.layers.4.weight')):
            w, gw = W(key)
            check_layer('u%d %s' % (u, out), half, [c.fwd(inp, u), w], c.g(out, u), [c.g(inp, u), gw], m[out])
        # ... whose output is also pooled: the stage's gradient (read back: skip share + pool share) is the upstream gradient
        for out, inp, key in (('d0', 'd0a', 'down_sample_layers.0.layers.4.weight'), ('d2', 'd2a', 'down_sample_layers.2.layers.4.weight')):
            w, gw = W(key)
            check_layer('u%d %s (pooled)' % (u, out), half, [c.fwd(inp, u), w], c.g(out, u), [c.g(inp, u), gw], m[out])
        # the two-source concat stage; its skip source also receives 1/4 of its pool's gradient
        for out, a, b, pool, key in (('u1a', 't1', 'd1', 'p1', 'up_conv.1.layers.0.weight'), ('u2a', 't2', 'd0', 'p0', 'up_conv.2.0.layers.0.weight')):
            w, gw = W(key)
            check_layer('u%d %s (concat)' % (u, out), cat_half, [c.fwd(a, u), c.fwd(b, u), w], c.g(out, u), [c.g(a, u), c.g(b, u), gw], m[out],
                        add=[None, up(c.g(pool, u)), None])
        # transposed-convolution stages
        for out, inp, key in (('t0', 'bb', 'up_transpose_conv.0.layers.0.weight'), ('t2', 'u1', 'up_transpose_conv.2.layers.0.weight')):
            w, gw = W(key)
            check_layer('u%d %s (transposed)' % (u, out), thalf, [c.fwd(inp, u), w], c.g(out, u), [c.g(inp, u), gw], m[out])
        # loop algebra in front of the finish: gh_total = gh - P^H gz'
        P, eig = c.P.astype(np.complex128), c.eig.astype(np.float64)
        gz_next = cplx(c.g('gz', u + 1)) if u < U - 1 else None
        gh_tot = cplx(c.g('gh', u)) - (0 if gz_next is None else np.conj(np.transpose(P, (0, 2, 1))) @ gz_next)
        gh_tot = np.stack((gh_tot.real, gh_tot.imag), -1)                             # [B, 64, 16, 2]
        # 1 x 1 convolution + unnorm + residual; the gradient of 'stat' is the finish's share
        stat = c.tr.stage('stat', u)[:B].cpu().numpy()
        (w, gw), (b, gb) = W('up_conv.2.1.weight'), W('up_conv.2.1.bias')
        check_layer('u%d finish' % u, fin, [c.fwd('u2', u), w, b, stat], np.transpose(gh_tot, (0, 3, 1, 2)), [c.g('u2', u), gw, gb, c.g('stat', u)])
        # norm: dL/dr = direct (gh_total) + through x, mean and std
        gs = c.g('stat', u)
        gout = np.concatenate([c.g('x', u).reshape(B, -1), gs[:, 0::2], gs[:, 1::2], gh_tot.reshape(B, -1)], 1)
        check_layer('u%d norm' % u, nrm, [c.tr.stage('r', u)[:B].cpu().numpy()], gout, [c.g('r', u)], planes=False)
        # loop algebra behind it: gh_{u-1} = dr (the same bits), gz_u = div gz' + P dr / eig
        if u > 0:
            assert same_bits(c.g('gh', u - 1), c.g('r', u))
        ref = (P @ cplx(c.g('r', u))) / eig[:, None, None] + (0 if gz_next is None else c.logs['div'][u].astype(np.float64)[:, None, None] * gz_next)
        rule_r('u%d gz' % u, cplx(c.g('gz', u)), ref, gz32(c, u, False), gz32(c, u, True))
    # loss: gh of the last unroll = (2 / B) (h - H); the float32 evaluations: that formula, and (2 h - 2 H) / B
    h, Ht = c.logs['h'][U - 1], c.H
    ref = 2.0 / B * (h.astype(np.complex128) - Ht.astype(np.complex128))
    a32 = (np.float32(2.0 / B) * (h - Ht)).astype(np.complex64)
    b32 = ((np.float32(2) * h - np.float32(2) * Ht) / np.float32(B)).astype(np.complex64)
    rule_r('loss gradient', cplx(c.g('gh', U - 1)), ref, a32, b32)


# ---- 4. the assembled gradient under the kernel's own masks ---------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Np,U', SMALL)
def test_assembled_gradient_per_tensor(B, Np, U):
    c = case(B, Np, U)
    r64, r32 = c.masked(F64), [c.masked(F32), c.masked(F32, 'flipped')]
    assert sorted(r64['grads']) == sorted(c.sd)
    for k in r64['grads']:
        rule_r(k, c.grads[k], r64['grads'][k], *[r['grads'][k] for r in r32])


def test_assembled_gradient_per_net_at_ten_unrolls():
    """At this depth a 2-element bias of another valid float32 order reached 5.2 x e_ref: the 19 tensors of a net are
    concatenated, where the worst such ratio was 1.25."""
    c = case(4, 38, 10)
    r64, r32 = c.masked(F64), [c.masked(F32), c.masked(F32, 'flipped')]
    for u in range(10):
        rule_r('net %d' % u, T.per_net(c.grads, u), T.per_net(r64['grads'], u), *[T.per_net(r['grads'], u) for r in r32])


# ---- 5. Adam alone ----------------------------------------------------------------------------------------------------------------------------
def test_adam_alone_three_steps():
    U = 1
    sd = ldamp.seeded_state_dict(cases.SEED_WEIGHTS, U)
    tr = GuardedTrainer({'max_unrolls': U}, sd, capacity=1)
    rng = np.random.default_rng(3)
    names = list(sd)
    grads = [{k: (rng.standard_normal(sd[k].shape) * 10.0 ** rng.integers(-6, 1)).astype(np.float32) for k in names} for _ in range(3)]
    lrs = [1e-3, 1e-3, 1e-4]
    flat = lambda d: np.concatenate([np.asarray(d[k]).ravel() for k in names])          # noqa: E731
    p64, m64, v64 = T.adam_reference(flat(sd), [flat(g) for g in grads], lrs, F64)
    p32, m32, v32 = T.adam_reference(flat(sd), [flat(g) for g in grads], lrs, F32)
    for s in range(3):
        tr.adam(grads[s], lr=lrs[s])
        torch.cuda.synchronize()
        got = flat(tr.state_dict())
        # the parameters move by lr per step: the error that matters is the update's
        rule_r('update of step %d' % s, got.astype(np.float64) - flat(sd), p64[s] - flat(sd).astype(np.float64), p32[s].astype(np.float64) - flat(sd))
    osd = tr.optimizer_state_dict()
    assert len(osd['state']) == 19 and float(osd['state'][0]['step']) == 3.0 and osd['param_groups'][0]['lr'] == 1e-4
    rule_r('exp_avg', np.concatenate([osd['state'][i]['exp_avg'].numpy().ravel() for i in range(19)]), m64, m32)
    rule_r('exp_avg_sq', np.concatenate([osd['state'][i]['exp_avg_sq'].numpy().ravel() for i in range(19)]), v64, v32)


def test_three_steps_follow_the_reference_losses():
    """The fixture's three steps (Adam at 1e-3, 1e-3, 1e-4): each loss within 4 x the reference's own float32-to-float64 distance."""
    g = load_golden('ldamp_train_step.npz')
    U = int(g['unrolls'])
    sample = cases.torch_sample(g['Y_herm'], g['P_herm'], g['eig1'], g['H_herm_cplx'])
    tr = GuardedTrainer({'max_unrolls': U}, ldamp.seeded_state_dict(int(g['seed_weights']), U), capacity=4)
    out = []
    for s in range(3):
        tr.set_lr(float(g['lrs'][s]))
        out.append(tr.step(sample, U, directions=g['directions'][s].astype(np.float32)))
    tr.check_guards()
    for s, (loss, nmse) in enumerate(out):
        print('step %d: loss %.6f (float64 %.6f, reference float32 off by %.2e, kernel by %.2e)  nmse %.6f (float64 %.6f)'
              % (s, loss, g['loss64'][s], abs(g['loss32'][s] - g['loss64'][s]), abs(loss - g['loss64'][s]), nmse, g['nmse64'][s]))
    for s, (loss, nmse) in enumerate(out):
        assert abs(loss - g['loss64'][s]) <= cases.FACTOR * abs(g['loss32'][s] - g['loss64'][s]), s
    assert tr.steps == 3


# ---- 6. properties ------------------------------------------------------------------------------------------------------------------------------
def _everything(tr, U):
    out = [tr.stage(n, u).cpu().numpy() for u in range(U) for n in ldamp.STAGES]
    out += [tr.grad(n, u).cpu().numpy() for u in range(U) for n in ldamp.STAGES + ('gh', 'gz')]
    return out + [tr._get(k) for k in range(4)]


def test_a_step_is_bit_reproducible_and_streams_do_not_matter():
    B, Np, U = 3, 38, 2
    sd, Y, P, eig, H, dirs = cases.problem(B, Np, U)
    sample = cases.torch_sample(Y, P, eig, H)
    runs = []
    for stream in (None, None, torch.cuda.Stream()):
        tr = GuardedTrainer({'max_unrolls': U}, sd, capacity=B)
        res = tr.step(sample, U, directions=dirs, stream=stream)
        tr.check_guards()
        runs.append((res, _everything(tr, U)))
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        assert all(same_bits(a, b) for a, b in zip(other[1], runs[0][1]))


def test_stage_gradients_of_a_sample_do_not_depend_on_the_batch():
    """B = 4 against the same samples alone (B = 1) and in pairs at other positions (B = 2): the loss is a mean over the batch, so the
    gradients differ by the factor B' / B, a power of two, which every launch carries through exactly."""
    Np, U = 38, 2
    sd, Y, P, eig, H, dirs = cases.problem(4, Np, U)
    full = case(4, Np, U)
    for idx in ([2], [3, 1]):
        tr = GuardedTrainer({'max_unrolls': U}, sd, capacity=len(idx))
        tr.step(cases.torch_sample(Y[idx], P[idx], eig[idx], H[idx]), U, directions=dirs[:, idx], update=False)
        tr.check_guards()
        scale = np.float32(len(idx) / 4.0)
        for u in range(U):
            for n in ldamp.STAGES + ('gh', 'gz'):
                assert same_bits(tr.grad(n, u).cpu().numpy() * scale, full.g(n, u)[idx]), (idx, u, n)


def test_caller_directions_equal_the_replayed_philox_directions():
    B, Np, U = 3, 38, 2
    sd, Y, P, eig, H, _ = cases.problem(B, Np, U)
    sample = cases.torch_sample(Y, P, eig, H)
    a = GuardedTrainer({'max_unrolls': U}, sd, capacity=B)
    ra = a.step(sample, U, seed=77, sample_ids=np.arange(5, 5 + B))
    a.check_guards()
    b = GuardedTrainer({'max_unrolls': U}, sd, capacity=B)
    rb = b.step(sample, U, directions=ldamp.replay_directions(77, range(5, 5 + B), U))
    b.check_guards()
    assert ra == rb and all(same_bits(x, y) for x, y in zip(_everything(a, U), _everything(b, U)))


def test_state_round_trip_continues_bit_for_bit():
    B, Np, U = 3, 38, 2
    sd, Y, P, eig, H, dirs = cases.problem(B, Np, U)
    sample = cases.torch_sample(Y, P, eig, H)
    a = GuardedTrainer({'max_unrolls': U}, sd, capacity=B)
    a.step(sample, U, directions=dirs)
    b = GuardedTrainer({'max_unrolls': U}, a.state_dict(), lr=0.5, capacity=B)
    b.load_optimizer_state_dict(a.optimizer_state_dict())
    assert (b.steps, b.trained_unrolls, b.lr) == (1, U, 1e-3)
    ra, rb = a.step(sample, U, directions=dirs), b.step(sample, U, directions=dirs)
    assert ra == rb and all(same_bits(a._get(k), b._get(k)) for k in range(4))
    with pytest.raises(_lib.SbcError):                   # the library checks its own arguments too
        _lib.check(_lib.lib().sbc_ldamp_trainer_stage(9, 0, 0, B, U, *[None] * 5))


def test_cli_writes_a_checkpoint_that_test_ldamp_loads(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ['--synthetic', '--snr_range', '10']
    p = subprocess.run([sys.executable, '-m', 'score_based_channels_amd.train_ldamp', '--max_steps', '2', '--batch_size', '4'] + common,
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('Epoch 0, Step')]
    assert len(lines) == 2 and os.path.exists(tmp_path / 'models' / 'ldamp-FlippedUNet' / 'train-CDL-C' / 'model_snr10.00_alpha0.60.pt')
    p = subprocess.run([sys.executable, '-m', 'score_based_channels_amd.test_ldamp', '--no_plot', '--num_channels', '4', '--seed', '1'] + common,
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert p.returncode == 0 and 'Learned D-AMP: SNR = 10.00 dB' in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
