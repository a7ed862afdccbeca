"""GPU tests of WGAN training (csrc/wgan_train.hip behind wgan.Trainer): every launch of a critic and of a generator iteration, alone and
assembled.

Rule R (DESIGN sections 13, 14, 16): error against float64 <= 4 x e_ref, norm-wise per tensor; e_ref is the larger error of the float32
oracle's two summation orders (tests/wgan_train_oracle.py: native and spatially flipped).  Both sides are measured against the same float64
value, so the comparison is made on the norms of the differences: that is the norm-wise relative rule, and it also covers the tensors
whose true value is zero (the generator's convolution biases in front of BatchNorm).

Training-mode BatchNorm couples the batch, and the gradient is not continuous in the activation signs: the forward pass is held to
float64 directly; the kernel's masks may differ from float64's only within 1e-4 rms of zero; everything downstream of a mask is held to
float64 UNDER THE KERNEL'S OWN MASKS; single backward launches are held to float64 on the kernel's own inputs.  Nothing is compared after
RMSprop has accumulated: the optimiser is tested alone, bit for bit against the float32 formula.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import wgan_train_oracle as T
from score_based_channels_amd import _lib, wgan

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TRAINABLE = lambda k: not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))           # noqa: E731


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rule_r(what, got, r64, r32a, r32b):
    n = lambda a: float(np.linalg.norm(np.asarray(a, np.float64).ravel() - np.asarray(r64, np.float64).ravel()))           # noqa: E731
    err, e_ref, scale = n(got), max(n(r32a), n(r32b)), float(np.linalg.norm(np.asarray(r64, np.float64).ravel()))
    print('%-52s err %.2e  e_ref %.2e  (|ref| %.2e)  ratio %.2f' % (what, err, e_ref, scale, err / max(e_ref, 1e-300)))
    assert np.shape(got) == np.shape(r64) and err <= 4 * e_ref, (what, err, e_ref)


def inputs(Br, Bf, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((Br, 2, 16, 64)).astype(np.float32), rng.standard_normal((3, Bf, 60)).astype(np.float32)


def stage_exists(net, kind, k, n_layers):
    """the stages a network has: G (layers 0 .. L, 0 the dense output) keeps act and gact for every layer and the rest for k >= 1; D (layers
    0 .. M) keeps raw and draw for every layer, pre / act / gact / mask for all but the last, mean / var where there is a BatchNorm"""
    if net == 'g':
        return kind in ('act', 'gact') or k >= 1
    if kind in ('raw', 'draw'):
        return True
    return k < n_layers and (kind not in ('mean', 'var') or k >= 1)


def stages(tr, net, n_layers):
    """every stage of one network of the last call -> dict of lists (None where a layer has none); every stage that exists must be
    readable, every other one refused"""
    out = {}
    for kind in ('raw', 'mean', 'var', 'pre', 'act', 'mask', 'gact', 'draw'):
        out[kind] = []
        for k in range(n_layers + 1):
            name = '%s.%s%d' % (net, kind, k)
            if stage_exists(net, kind, k, n_layers):
                out[kind].append(tr.stage(name).cpu().numpy())
            else:
                with pytest.raises(_lib.SbcError):
                    tr.stage(name)
                out[kind].append(None)
    return out


def widths(net, n_extra):
    return [16, 32] + [64] * (1 + n_extra) if net == 'g' else [32] * (1 + n_extra) + [16]


def masks_of(st, net, n_extra):
    w = widths(net, n_extra)
    return [wgan.unpack_mask(m, 32 * m.shape[-1])[..., :w[k]] for k, m in enumerate(st['mask']) if m is not None]


def assert_masks(what, masks, pres):
    for k, (m, x) in enumerate(zip(masks, [p for p in pres if p is not None])):
        rms = np.sqrt(np.mean(x ** 2))
        differ, near = m != (x > 0), np.abs(x) <= 1e-4 * rms
        print('%s layer %d: %d signs differ, %d of %d units within 1e-4 rms of zero' % (what, k, differ.sum(), near.sum(), x.size))
        assert m.shape == x.shape and not np.any(differ & ~near), (what, k)


def forward_checks(what, st, f64, f32, twin):
    for kind in ('raw', 'mean', 'var', 'pre', 'act'):
        for k, r in enumerate(f64[kind]):
            if r is not None and st[kind][k] is not None:
                rule_r('%s %s%d' % (what, kind, k), st[kind][k], r, f32[kind][k], twin[kind][k])


class GuardedTrainer(wgan.Trainer):
    """The trainer with ``DeviceHandle._workspace_of`` overridden: a workspace of EXACTLY sbc_wgan_trainer_workspace_floats(h, capacity)
    floats, NaN-filled (the library promises nothing about what it holds), between pads of one per-sample stride (tests/guarded.py)."""
    guard = None

    def _workspace_of(self, n, dev):
        from guarded import Guard
        f = _lib.lib().sbc_wgan_trainer_workspace_floats
        assert int(n) == int(f(self._h, self.capacity))
        if self.guard is None:
            self.guard = Guard(torch)
            stride = int(f(self._h, self.capacity + 1)) - int(n)
            self._ws = self.guard.out('trainer workspace (%d floats, capacity %d)' % (n, self.capacity), (int(n),), must_write=False,
                                      pad=max(1024, stride))
        return self._ws

    def check_guards(self):
        torch.cuda.synchronize()
        self.guard.check()


class Case:
    """a trainer at the reference's initial distributions, and what one critic and one generator iteration leave behind"""

    def __init__(self, n_extra, Br, Bf, seed):
        self.n_extra, self.Br, self.Bf = n_extra, Br, Bf
        self.gsd, self.dsd = wgan.init_state_dicts(seed, n_extra)
        self.real, self.noise = inputs(Br, Bf, seed)
        # (both batches at the capacity in '4-4-extra1'; the real batch below it in '3-5-extra1'; the fake batch -- and with it the
        # generator iteration -- below it in '5-3-extra1')
        self.tr = GuardedTrainer(self.gsd, self.dsd, batch_size=max(Br, Bf))

    def critic(self, noise):
        """-> everything about one critic iteration from the trainer's CURRENT state"""
        tr, n = self.tr, self.n_extra
        gsd, dsd = tr.state_dicts()
        dsd = {k: (T.clamp(v) if TRAINABLE(k) else v) for k, v in dsd.items()}
        sq0 = {k: tr.tensor('d', k, 'square_avg') for k in dsd if TRAINABLE(k)}
        losses = tr.critic_step(self.real, noise).cpu().numpy()
        tr.check_guards()
        got = {'losses': losses, 'gsd': gsd, 'dsd': dsd, 'sq0': sq0, 'g': stages(tr, 'g', 2 + n), 'd0': stages(tr, 'd0', n + 2), 'd1': stages(tr, 'd1', n + 2),
               'gen': tr.stage('g.gen').cpu().numpy(), 'grads': {k: tr.tensor('d', k, 'grad') for k in dsd if TRAINABLE(k)}}
        got['after'] = tr.state_dicts()
        got['sq'] = {k: tr.tensor('d', k, 'square_avg') for k in sq0}
        got['masks'] = {net: masks_of(got[net], net[0], n) for net in ('g', 'd0', 'd1')}
        a = (gsd, dsd, self.real, noise)
        got['free64'] = T.critic_terms(*a, F64)
        got['held64'], got['held32'], got['twin32'] = T.critic_terms(*a, F64, got['masks']), T.critic_terms(*a, F32, got['masks']), T.critic_terms_flipped(*a, F32, got['masks'])
        return got

    def generator(self, noise):
        tr, n = self.tr, self.n_extra
        gsd, dsd = tr.state_dicts()
        sq0 = {k: tr.tensor('g', k, 'square_avg') for k in gsd if TRAINABLE(k)}
        loss = tr.generator_step(noise).cpu().numpy()
        tr.check_guards()
        got = {'loss': loss, 'gsd': gsd, 'dsd': dsd, 'sq0': sq0, 'g': stages(tr, 'g', 2 + n), 'd1': stages(tr, 'd1', n + 2), 'gen': tr.stage('g.gen').cpu().numpy(),
               'dgen': tr.stage('g.dgen').cpu().numpy(), 'grads': {k: tr.tensor('g', k, 'grad') for k in gsd if TRAINABLE(k)}}
        got['after'] = tr.state_dicts()
        got['sq'] = {k: tr.tensor('g', k, 'square_avg') for k in sq0}
        got['masks'] = {net: masks_of(got[net], net[0], n) for net in ('g', 'd1')}
        a = (gsd, dsd, noise)
        got['free64'] = T.generator_terms(*a, F64)
        got['held64'], got['held32'], got['twin32'] = T.generator_terms(*a, F64, got['masks']), T.generator_terms(*a, F32, got['masks']), T.generator_terms_flipped(*a, F32, got['masks'])
        return got


# (n_extra, real batch, fake batch): the fixture geometry; unequal batches; B = 1 (statistics over H W alone); the other depths
# ... and a fake batch below the trainer's capacity ('5-3': G, the critic's fake pass and the generator iteration on 3 of 5 samples' room)
CASES = {'4-4-extra1': (1, 4, 4, 101), '3-5-extra1': (1, 3, 5, 102), '1-1-extra0': (0, 1, 1, 103), '2-2-extra2': (2, 2, 2, 104),
         '5-3-extra1': (1, 5, 3, 106)}
_cache = {}


def run_case(name):
    """critic, critic, generator: each iteration is compared one step ahead, from the state the kernels themselves reached"""
    if name not in _cache:
        c = Case(*CASES[name])
        c.c1 = c.critic(c.noise[0])
        c.c2 = c.critic(c.noise[1]) if name == '4-4-extra1' else None
        c.g1 = c.generator(c.noise[2])
        _cache.clear()                                   # one case's stages at a time
        _cache[name] = c
    return _cache[name]


@pytest.mark.parametrize('name', CASES)
def test_critic_iteration(name):
    c = run_case(name)
    for tag, r in (('c1', c.c1), ('c2', c.c2)):
        if r is None:
            continue
        # forward: every layer of G and of both passes of D against float64, free-running; the masks by the band rule
        f32 = T.critic_terms(r['gsd'], r['dsd'], c.real, c.noise[0 if tag == 'c1' else 1], F32)
        twin = T.critic_terms_flipped(r['gsd'], r['dsd'], c.real, c.noise[0 if tag == 'c1' else 1], F32)
        for net in ('g', 'd0', 'd1'):
            forward_checks('%s %s' % (tag, net), r[net], r['free64'][net], f32[net], twin[net])
            assert_masks('%s %s' % (tag, net), r['masks'][net], r['free64'][net]['pre'])
        rule_r(tag + ' gen', r['gen'], r['free64']['g']['gen'], f32['g']['gen'], twin['g']['gen'])
        rule_r(tag + ' errD_real', r['losses'][:1], r['free64']['errD_real'], f32['errD_real'], twin['errD_real'])
        rule_r(tag + ' errD_fake', r['losses'][1:], r['free64']['errD_fake'], f32['errD_fake'], twin['errD_fake'])
        # backward: every parameter gradient (real + fake, accumulated) under the kernel's masks
        assert set(r['grads']) == set(r['held64']['grads'])
        for k in r['grads']:
            rule_r('%s grad %s' % (tag, k), r['grads'][k], r['held64']['grads'][k], r['held32']['grads'][k], r['twin32']['grads'][k])
        # the clamp and RMSprop inside the step: bit for bit the float32 formula on the kernel's own gradients
        for k in r['grads']:
            p, sq = T.rmsprop(r['dsd'][k], r['grads'][k], r['sq0'][k])
            assert same_bits(p, r['after'][1][k]) and same_bits(sq, r['sq'][k]), k
        # BatchNorm weights start at N(1, 0.02): all of them sit at the clamp value in the first iteration (later ones move by 10 lr per step)
        assert tag != 'c1' or all(np.all(v == np.float32(0.01)) for k, v in r['dsd'].items() if k.endswith('batchnorm.weight'))


@pytest.mark.parametrize('name', CASES)
def test_running_statistics(name):
    """after one critic iteration G has seen one batch and D two (real, then fake); num_batches_tracked counts them"""
    c = run_case(name)
    r = c.c1
    n = c.n_extra
    for net, sd0, sd1, passes in (('g', r['gsd'], r['after'][0], ['g']), ('d', r['dsd'], r['after'][1], ['d0', 'd1'])):
        names = [T.layer_names(k)[1] for k in range(1, 3 + n)] if net == 'g' else [t[1] for t in T.d_layer_table(n)]
        for k, bn in enumerate(names, start=1 if net == 'g' else 0):
            if bn is None:
                continue
            rm, rv = sd0[bn + '.running_mean'].astype(np.float64), sd0[bn + '.running_var'].astype(np.float64)
            mag_m, mag_v = np.abs(rm), np.abs(rv)
            for p in passes:                             # the update formula in float64 on the kernel's own batch statistics (held to float64 above)
                x = r[p]['raw'][k]
                rm, rv = T.running_update(rm, rv, r[p]['mean'][k], r[p]['var'][k], x.size // x.shape[1])
                mag_m, mag_v = np.maximum(mag_m, np.abs(r[p]['mean'][k])), np.maximum(mag_v, 2 * np.abs(r[p]['var'][k]))
            # per update three float32 roundings (two products, one sum) of terms no larger than `mag`, one more for the unbiased variance:
            # 4 x 2^-24 = 2.4e-7 per pass, taken as 4e-7
            assert np.all(np.abs(sd1[bn + '.running_mean'] - rm) <= 4e-7 * len(passes) * mag_m), bn
            assert np.all(np.abs(sd1[bn + '.running_var'] - rv) <= 4e-7 * len(passes) * mag_v), bn
            assert int(sd1[bn + '.num_batches_tracked']) == len(passes)
    if c.c2 is not None:                                 # three forwards of G, five of D by the end of critic, critic, generator
        for k in range(1, 3 + n):
            bn = T.layer_names(k)[1]
            rm, rv = r['gsd'][bn + '.running_mean'].astype(np.float64), r['gsd'][bn + '.running_var'].astype(np.float64)
            mag_m, mag_v = np.abs(rm), np.abs(rv)
            for q in (c.c1, c.c2, c.g1):
                x = q['g']['raw'][k]
                rm, rv = T.running_update(rm, rv, q['g']['mean'][k], q['g']['var'][k], x.size // x.shape[1])
                mag_m, mag_v = np.maximum(mag_m, np.abs(q['g']['mean'][k])), np.maximum(mag_v, 2 * np.abs(q['g']['var'][k]))
            after = c.g1['after'][0]
            assert np.all(np.abs(after[bn + '.running_mean'] - rm) <= 4e-7 * 3 * mag_m) and np.all(np.abs(after[bn + '.running_var'] - rv) <= 4e-7 * 3 * mag_v), bn
        assert int(c.g1['after'][0]['conv.bn1.num_batches_tracked']) == 3 and int(c.g1['after'][1]['main.pyramid:128:batchnorm.num_batches_tracked']) == 5


@pytest.mark.parametrize('name', CASES)
def test_generator_iteration(name):
    c = run_case(name)
    r = c.g1
    f32, twin = T.generator_terms(r['gsd'], r['dsd'], c.noise[2], F32), T.generator_terms_flipped(r['gsd'], r['dsd'], c.noise[2], F32)
    for net in ('g', 'd1'):                              # D's BatchNorm weights are NOT clamped here: the critic's step moved them off 0.01
        forward_checks('g1 %s' % net, r[net], r['free64'][net], f32[net], twin[net])
        assert_masks('g1 %s' % net, r['masks'][net], r['free64'][net]['pre'])
    rule_r('errG', r['loss'], r['free64']['errG'], f32['errG'], twin['errG'])
    rule_r('dgen', r['dgen'], r['held64']['dgen'], r['held32']['dgen'], r['twin32']['dgen'])
    assert set(r['grads']) == set(r['held64']['grads'])
    for k in r['grads']:
        rule_r('grad %s' % k, r['grads'][k], r['held64']['grads'][k], r['held32']['grads'][k], r['twin32']['grads'][k])
    for k in r['grads']:
        p, sq = T.rmsprop(r['gsd'][k], r['grads'][k], r['sq0'][k])
        assert same_bits(p, r['after'][0][k]) and same_bits(sq, r['sq'][k]), k
    for k, v in r['dsd'].items():                        # the critic's parameters received no update
        if TRAINABLE(k):
            assert same_bits(v, r['after'][1][k]), k


def alone(what, fn, arrays, got):
    """one launch on the kernel's own inputs: float64, float32 and the flipped float32 order of the oracle (every 4-D operand is flipped,
    filters included, and every 4-D result flipped back: the same function)"""
    r64, r32 = fn(*arrays, F64), fn(*arrays, F32)
    tw = T.spatial_twin(lambda *a: fn(*a, F32), arrays)
    if not isinstance(r64, tuple):
        r64, r32, tw, got = (r64,), (r32,), (tw,), (got,)
    for i, g in enumerate(got):
        if g is not None:
            rule_r('%s [%d]' % (what, i), g, r64[i], r32[i], tw[i])


@pytest.mark.parametrize('name', ['4-4-extra1', '1-1-extra0'])
def test_generator_backward_launches_alone(name):
    c = run_case(name)
    r, sd, L = c.g1, c.g1['gsd'], 2 + c.n_extra
    g, masks, grads = r['g'], r['masks']['g'], r['grads']
    alone('out adjoint', lambda d, w, dt: T.conv_dgrad(d, w, (c.Bf, 128, 16, 64), 1, 2, 0, dt), [r['dgen'], sd['conv.conv_out.weight']], g['gact'][L])
    alone('out weight gradient', lambda d, a, dt: T.conv_wgrad(d, a, (2, 128, 5, 5), 1, 2, 0, dt), [r['dgen'], g['act'][L]], grads['conv.conv_out.weight'])
    alone('out bias gradient', lambda d, dt: d.astype(np.float64 if dt == F64 else np.float32).sum((0, 2, 3)), [r['dgen']], grads['conv.conv_out.bias'])
    for k in range(L, 0, -1):
        conv, bn = T.layer_names(k)
        ks, up = (5, 1) if k <= 2 else (3, 0)
        alone('layer %d BatchNorm backward' % k, lambda ga, raw, m, dt: T.layer_backward(ga, raw, m, sd[bn + '.weight'], 0.0, dt),
              [g['gact'][k], g['raw'][k], masks[k - 1]], (g['draw'][k], grads[bn + '.weight'], grads[bn + '.bias']))
        alone('layer %d weight gradient' % k, lambda d, a, dt: T.conv_wgrad(d, a, (128, 128, ks, ks), 1, ks // 2, up, dt), [g['draw'][k], g['act'][k - 1]],
              grads[conv + '.weight'])
        alone('layer %d input gradient' % k, lambda d, w, dt: T.conv_dgrad(d, w, g['act'][k - 1].shape, 1, ks // 2, up, dt), [g['draw'][k], sd[conv + '.weight']],
              g['gact'][k - 1])
    r64, r32 = T.dense_wgrad(g['gact'][0], c.noise[2], F64), T.dense_wgrad(g['gact'][0], c.noise[2], F32)
    tw = T.dense_wgrad(g['gact'][0][::-1].copy(), c.noise[2][::-1].copy(), F32)          # the other order: the batch summed backwards
    rule_r('dense weight gradient', grads['dense.dense_input.weight'], r64[0], r32[0], tw[0])
    rule_r('dense bias gradient', grads['dense.dense_input.bias'], r64[1], r32[1], tw[1])


@pytest.mark.parametrize('name', ['4-4-extra1', '2-2-extra2'])
def test_critic_backward_launches_alone(name):
    """the generator iteration's pass through D (no weight gradient), then the critic iteration's weight gradients: real - fake, accumulated"""
    c = run_case(name)
    r, sd = c.g1, c.g1['dsd']
    table, d, masks = T.d_layer_table(c.n_extra), r['d1'], r['masks']['d1']
    M = len(table) - 1
    assert np.all(d['draw'][M] == np.float32(1.0) / np.float32(c.Bf))
    for j in range(M, -1, -1):
        conv, bn, stride, pad = table[j]
        shape = (c.Bf, 2, 16, 64) if j == 0 else d['act'][j - 1].shape
        alone('D layer %d input gradient' % j, lambda g, w, dt: T.conv_dgrad(g, w, shape, stride, pad, 0, dt), [d['draw'][j], sd[conv + '.weight']],
              r['dgen'] if j == 0 else d['gact'][j - 1])
        if j > 0:
            pbn = table[j - 1][1]
            w = sd[pbn + '.weight'] if pbn else None
            alone('D layer %d activation backward' % (j - 1), lambda ga, raw, m, dt: T.layer_backward(ga, raw, m, w, 0.2, dt, bn=pbn is not None)[0],
                  [d['gact'][j - 1], d['raw'][j - 1], masks[j - 1]], d['draw'][j - 1])
    q = c.c1
    for j, (conv, bn, stride, pad) in enumerate(table):
        ins = [c.real if j == 0 else q['d0']['act'][j - 1], q['gen'] if j == 0 else q['d1']['act'][j - 1]]
        fn = lambda g0, a0, g1, a1, dt: (T.conv_wgrad(g0, a0, sd[conv + '.weight'].shape, stride, pad, 0, dt)            # noqa: E731
                                         + T.conv_wgrad(g1, a1, sd[conv + '.weight'].shape, stride, pad, 0, dt))
        alone('D layer %d weight gradient' % j, fn, [q['d0']['draw'][j], ins[0], q['d1']['draw'][j], ins[1]], q['grads'][conv + '.weight'])


@pytest.mark.parametrize('ks,up,B,H,W', [(5, 1, 3, 16, 64), (5, 0, 3, 8, 32), (5, 1, 1, 8, 32), (3, 0, 3, 16, 64), (3, 0, 5, 4, 32)])
def test_wgrad128_alone(ks, up, B, H, W):
    """drawn operands; 3 and 5 samples split unevenly over the 16 / 32 partial sums, one sample of 8 rows gives fewer tiles than splits"""
    rng = np.random.default_rng(ks * 100 + H)
    draw = rng.standard_normal((B, 128, H, W)).astype(np.float32)
    inp = rng.standard_normal((B, 128, H >> up, W >> up)).astype(np.float32)
    # operands between guarded margins, a scratch of exactly sbc_wgan_wgrad128_scratch_floats(...) floats (tests/guarded.py)
    from guarded import Guard
    g = Guard(torch)
    n = int(_lib.lib().sbc_wgan_wgrad128_scratch_floats(B, H, W, ks))
    assert n > 0
    ddraw, dinp, dW = g.inp('draw', draw), g.inp('inp', inp), g.out('dW', (128, 128, ks, ks))
    scratch = g.out('scratch (%d floats)' % n, (n,), must_write=False, pad=max(1024, -(-n // B)))
    p = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731
    _lib.check(_lib.lib().sbc_wgan_wgrad128(p(ddraw), p(dinp), p(dW), p(scratch), B, H, W, ks, up, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    g.check()
    got = dW.cpu().numpy()
    alone('wgrad128<%d> up %d' % (ks, up), lambda d, a, dt: T.conv_wgrad(d, a, (128, 128, ks, ks), 1, ks // 2, up, dt), [draw, inp], got)
    assert same_bits(got, wgan.wgrad128(dev(draw), dev(inp), ks, up).cpu().numpy())


def pack_mask(m):
    B, C, H, W = m.shape
    words = (W + 31) // 32
    bits = np.zeros((B, C, H, words * 32), np.int64)
    bits[..., :W] = m
    return (bits.reshape(B, C, H, words, 32) << np.arange(32)).sum(-1).astype(np.uint32).view(np.int32)


@pytest.mark.parametrize('C,H,W,slope,B', [(64, 8, 32, 0.2, 3), (128, 4, 16, 0.2, 5), (128, 16, 64, 0.0, 2), (128, 4, 16, 0.2, 1)])
def test_batchnorm_backward_alone(C, H, W, slope, B):
    """drawn operands: the critic's two shapes with LeakyReLU, the generator's with ReLU; the weights at the clamp value and of order one"""
    rng = np.random.default_rng(C + W + B)
    raw = (rng.standard_normal((B, C, H, W)) * rng.uniform(0.5, 2, (1, C, 1, 1)) + rng.standard_normal((1, C, 1, 1))).astype(np.float32)
    gact = rng.standard_normal((B, C, H, W)).astype(np.float32)
    w = np.where(np.arange(C) % 2 == 0, 0.01, rng.uniform(0.5, 1.5, C)).astype(np.float32)
    mask = rng.random((B, C, H, W)) < 0.5
    x = torch.from_numpy(raw).double()
    mean, var = x.mean((0, 2, 3)).float().numpy(), x.var((0, 2, 3), unbiased=False).float().numpy()
    got = wgan.bn_backward(dev(gact), dev(raw), dev(pack_mask(mask)), dev(mean), dev(var), dev(w), slope)
    alone('BatchNorm backward C %d' % C, lambda ga, r, m, dt: T.layer_backward(ga, r, m, w, slope, dt), [gact, raw, mask], tuple(t.cpu().numpy() for t in got))


def test_rmsprop_and_clamp_alone():
    rng = np.random.default_rng(9)
    n = 100003                                           # no multiple of the workgroup
    p = rng.standard_normal(n).astype(np.float32) * 0.02
    sq = (10.0 ** rng.uniform(-16, 2, n)).astype(np.float32)
    sq[:1000] = 0
    dp, dsq = dev(p), dev(sq)
    for _ in range(3):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 3, n)).astype(np.float32)
        g[::7] = 0
        wgan.rmsprop(dp, dev(g), dsq)
        p, sq = T.rmsprop(p, g, sq)
        assert same_bits(dp.cpu().numpy(), p) and same_bits(dsq.cpu().numpy(), sq)
    edge = np.array([-1, -0.010000001, -0.01, -0.0099999, -0.0, 0.0, 1e-30, 0.0099999, 0.01, 0.010000001, 3, np.inf, -np.inf], np.float32)
    de = dev(np.concatenate([edge, p]))
    wgan.rmsprop(de, None, None, clamp=(-0.01, 0.01))
    assert same_bits(de.cpu().numpy(), T.clamp(np.concatenate([edge, p])))


def final_state(tr):
    out = {}
    for sd in tr.state_dicts() + tuple({'%s.sq.%s' % (n, k): tr.tensor(n, k, 'square_avg') for k in tr.parameter_names(n)} for n in 'gd'):
        out.update(sd)
    return out


def sequence(stream=None, sync=False, seed=101):
    gsd, dsd = wgan.init_state_dicts(seed, 1)
    real, noise = inputs(3, 4, seed)
    tr = wgan.Trainer(gsd, dsd, batch_size=4)
    losses = []
    for step in (lambda: tr.critic_step(real, noise[0], stream=stream), lambda: tr.critic_step(real[:2], noise[1], stream=stream),
                 lambda: tr.generator_step(noise[2], stream=stream)):
        losses.append(step())
        if sync:
            torch.cuda.synchronize()
    if stream is not None:
        stream.synchronize()
    return np.concatenate([t.cpu().numpy() for t in losses]), final_state(tr)


def test_bit_reproducibility():
    """the same sequence again; with a host synchronisation between the steps; on a caller's stream: the same bits in every loss, parameter,
    running statistic and square average"""
    l0, s0 = sequence()
    for kw in ({}, {'sync': True}, {'stream': torch.cuda.Stream()}):
        l1, s1 = sequence(**kw)
        assert same_bits(l0, l1), kw
        assert all(same_bits(s0[k], s1[k]) for k in s0), kw
    assert np.all(np.isfinite(l0)) and all(np.all(np.isfinite(v)) for v in s0.values())


def test_optimizer_state_dicts_load_into_torch():
    gsd, dsd = wgan.init_state_dicts(7, 0)
    real, noise = inputs(2, 2, 7)
    tr = wgan.Trainer(gsd, dsd, batch_size=2)
    assert tr.optimizer_state_dicts()[0]['state'] == {}
    tr.critic_step(real, noise[0])
    tr.generator_step(noise[1])
    for i, net in enumerate('gd'):
        names = tr.parameter_names(net)
        params = [torch.nn.Parameter(torch.from_numpy(tr.tensor(net, k))) for k in names]
        opt = torch.optim.RMSprop(params, lr=5e-5)
        osd = tr.optimizer_state_dicts()[i]
        osd['state'] = {k: {a: torch.from_numpy(np.asarray(b)) for a, b in v.items()} for k, v in osd['state'].items()}
        assert set(opt.state_dict()['param_groups'][0]) <= set(osd['param_groups'][0])
        opt.load_state_dict(osd)
        assert same_bits(opt.state[params[0]]['square_avg'].numpy(), tr.tensor(net, names[0], 'square_avg')) and float(opt.state[params[0]]['step']) == 1


def test_refusals_launch_nothing():
    gsd, dsd = wgan.init_state_dicts(7, 1)
    real, noise = inputs(2, 2, 7)
    with pytest.raises(KeyError):
        wgan.Trainer(gsd, wgan.init_state_dicts(7, 2)[1])                   # another depth: names
    with pytest.raises(KeyError):
        wgan.Trainer({k: v for k, v in gsd.items() if k != 'conv.bn1.bias'}, dsd)
    with pytest.raises(ValueError):
        wgan.Trainer(gsd, dict(dsd, **{'main.final:128-1:conv.weight': np.zeros((1, 128, 4, 8), np.float32)}))
    with pytest.raises(ValueError):
        wgan.check_disc_geometry([16, 64], 60, 2, 32)
    tr = wgan.Trainer(gsd, dsd, batch_size=2)
    before = final_state(tr)
    for bad in (lambda: tr.critic_step(real[:0], noise[0]), lambda: tr.critic_step(real, noise[0][:0]), lambda: tr.generator_step(np.zeros((3, 60), np.float32)),
                lambda: tr.critic_step(real[:, :1], noise[0]), lambda: tr.generator_step(np.zeros((2, 61), np.float32))):
        with pytest.raises(ValueError):
            bad()
    h, lib = tr._h, _lib.lib()
    ws = tr._workspace_of(lib.sbc_wgan_trainer_workspace_floats(h, 2), torch.device('cuda', 0))
    p = lambda t: t.data_ptr()           # noqa: E731
    r, z = dev(real), dev(noise[0])
    for rc in (lib.sbc_wgan_trainer_critic_step(h, None, 2, p(z), 2, None, p(ws), 2, None), lib.sbc_wgan_trainer_critic_step(h, p(r), 2, p(z), 2, None, None, 2, None),
               lib.sbc_wgan_trainer_critic_step(h, p(r), 0, p(z), 2, None, p(ws), 2, None), lib.sbc_wgan_trainer_critic_step(h, p(r), 2, p(z), 3, None, p(ws), 2, None),
               lib.sbc_wgan_trainer_generator_step(h, None, 2, None, p(ws), 2, None), lib.sbc_wgan_trainer_generator_step(None, p(z), 2, None, p(ws), 2, None),
               lib.sbc_wgan_wgrad128(p(r), p(r), p(r), p(r), 2, 16, 48, 5, 0, None), lib.sbc_wgan_rmsprop(None, None, None, 4, 5e-5, 0.99, 1e-8, 0, 0, 1, None)):
        assert rc != 0 and lib.sbc_last_error()
    assert lib.sbc_wgan_trainer_workspace_floats(h, 0) == -1 and lib.sbc_wgan_wgrad128_scratch_floats(2, 16, 48, 5) == -1
    torch.cuda.synchronize()
    after = final_state(tr)
    assert all(same_bits(before[k], after[k]) for k in before)


def test_generator_iteration_from_an_unclamped_critic():
    """a generator iteration before any critic iteration: D's BatchNorm weights are N(1, 0.02), not 0.01"""
    c = Case(1, 3, 3, 105)
    r = c.generator(c.noise[0])
    assert all(np.all(np.abs(v - 1) < 0.2) for k, v in r['dsd'].items() if k.endswith('batchnorm.weight'))
    f32, twin = T.generator_terms(r['gsd'], r['dsd'], c.noise[0], F32), T.generator_terms_flipped(r['gsd'], r['dsd'], c.noise[0], F32)
    for net in ('g', 'd1'):
        forward_checks('unclamped %s' % net, r[net], r['free64'][net], f32[net], twin[net])
        assert_masks('unclamped %s' % net, r['masks'][net], r['free64'][net]['pre'])
    rule_r('unclamped errG', r['loss'], r['free64']['errG'], f32['errG'], twin['errG'])
    rule_r('unclamped dgen', r['dgen'], r['held64']['dgen'], r['held32']['dgen'], r['twin32']['dgen'])
    for k in r['grads']:
        rule_r('unclamped grad %s' % k, r['grads'][k], r['held64']['grads'][k], r['held32']['grads'][k], r['twin32']['grads'][k])


# ---- the fixture written from the reference modules: e_ref is the reference's own float32 distance from float64 ------------------------
def rule_r_fixture(what, got, r64, e_ref):
    err = float(np.linalg.norm(np.asarray(got, np.float64).ravel() - np.asarray(r64, np.float64).ravel()))
    print('%-52s err %.2e  e_ref %.2e  ratio %.2f' % (what, err, e_ref, err / max(e_ref, 1e-300)))
    assert np.shape(got) == np.shape(r64) and err <= 4 * e_ref, (what, err, e_ref)


def test_fixture_critic_and_generator_iteration():
    """tests/golden/wgan_train_step.npz (4 real, 4 noise, n_extra = 1): losses against the reference's float64 by its own float32 error;
    every parameter gradient against float64 under the kernel's masks by the reference's per-tensor e_ref; the masks by the band rule"""
    from conftest import load_golden
    g = load_golden('wgan_train_step.npz')
    n = int(g['n_extra'])
    gsd, dsd = wgan.init_state_dicts(int(g['seed']), n)
    clamped = {k: (T.clamp(v) if TRAINABLE(k) else v) for k, v in dsd.items()}
    tr = wgan.Trainer(gsd, dsd, batch_size=4)
    losses = tr.critic_step(g['real'], g['noise_c']).cpu().numpy()
    st = {net: stages(tr, net, 2 + n if net == 'g' else n + 2) for net in ('g', 'd0', 'd1')}
    masks = {net: masks_of(st[net], net[0], n) for net in st}
    free64, held64 = T.critic_terms(gsd, clamped, g['real'], g['noise_c'], F64), T.critic_terms(gsd, clamped, g['real'], g['noise_c'], F64, masks)
    for net in st:
        assert_masks('fixture %s' % net, masks[net], free64[net]['pre'])
    for i, k in enumerate(('errD_real', 'errD_fake')):
        rule_r_fixture('fixture ' + k, losses[i:i + 1], g[k + '64'], float(np.abs(g[k + '32'].astype(np.float64) - g[k + '64'])[0]))
    for k, ref in held64['grads'].items():
        rule_r_fixture('fixture grad ' + k, tr.tensor('d', k, 'grad'), ref, float(g['d/eref/' + k]))
    tr = wgan.Trainer(gsd, clamped, batch_size=4)                           # the fixture's generator iteration starts from the clamped critic
    loss = tr.generator_step(g['noise_g']).cpu().numpy()
    st = {net: stages(tr, net, 2 + n if net == 'g' else n + 2) for net in ('g', 'd1')}
    masks = {net: masks_of(st[net], net[0], n) for net in st}
    free64, held64 = T.generator_terms(gsd, clamped, g['noise_g'], F64), T.generator_terms(gsd, clamped, g['noise_g'], F64, masks)
    for net in st:
        assert_masks('fixture generator %s' % net, masks[net], free64[net]['pre'])
    rule_r_fixture('fixture errG', loss, g['errG64'], float(np.abs(g['errG32'].astype(np.float64) - g['errG64'])[0]))
    assert set(held64['grads']) == {k for k in gsd if TRAINABLE(k)}
    for k, ref in held64['grads'].items():
        rule_r_fixture('fixture grad ' + k, tr.tensor('g', k, 'grad'), ref, float(g['g/eref/' + k]))


# ---- the command line -------------------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, monkeypatch):
    """train_wgan for two generator iterations with a reduced Diters: its logs equal a Trainer driven with the same inputs, bit for bit; its
    checkpoint loads into wgan.DCGAN_G_Ours, and test_wgan --total_steps 2 runs on it"""
    from score_based_channels_amd import test_wgan, train_wgan as cli
    from score_based_channels_amd.checkpoint import load_checkpoint
    monkeypatch.chdir(tmp_path)
    out_dir = 'wgan_CDL-C_0.50/extra1'
    argv = ['--synthetic', '--seed', '1', '--max_gen_iterations', '2', '--batch_size', '4', '--Diters', '2', '--Diters_initial', '2', '--out_dir', out_dir, '--save_last']
    logs = cli.main(argv)
    assert len(logs['lines']) == 2 and logs['lines'][0].startswith('[0/3000][2/50][1] Loss_D: ') and logs['lines'][1].startswith('[0/3000][4/50][2] ')
    # the same inputs through a Trainer
    args = cli.parse_args(argv)
    config = cli.make_config(args)
    data = cli.load_data(config, True)
    assert data.shape == (200, 2, 16, 64) and data.dtype == np.float32
    tr = wgan.Trainer(*wgan.init_state_dicts(1, 1), batch_size=4)
    rng = np.random.Generator(np.random.PCG64(1))
    batches = cli.epoch_batches(len(data), 4, rng)
    direct = {k: [] for k in ('d_real_log', 'd_fake_log', 'g_log')}
    for take in cli.epoch_plan(len(batches), 0, 2, 2)[:2]:
        for b in take:
            losses = tr.critic_step(data[batches[b]], cli.draw_noise(rng, 4))
        errG = tr.generator_step(cli.draw_noise(rng, 4))
        for k, v in zip(('d_real_log', 'd_fake_log', 'g_log'), list(losses.cpu().numpy()) + [errG.cpu().numpy()[0]]):
            direct[k].append(v)
    for k, v in direct.items():
        assert same_bits(logs[k], np.asarray(v, np.float32)), k
    assert same_bits(logs['d_log'], logs['d_real_log'] - logs['d_fake_log'])
    # the checkpoint
    contents = load_checkpoint(out_dir + '/weights_last.pt', required=('config', 'gen_state', 'disc_state', 'gen_opt_state', 'disc_opt_state'))
    want = tr.state_dicts()
    for got, ref in zip((contents['gen_state'], contents['disc_state']), want):
        assert list(got) == list(ref) and all(same_bits(got[k].numpy(), ref[k]) for k in ref)
    assert int(contents['gen_state']['conv.bn1.num_batches_tracked']) == 6 and float(contents['disc_opt_state']['state'][0]['step']) == 4
    netG = wgan.DCGAN_G_Ours([16, 64], 60, 2, 128, 1, 1).load_state_dict(contents['gen_state']).cuda().eval()
    z = np.random.default_rng(0).standard_normal((2, 60)).astype(np.float32)
    assert np.all(np.isfinite(netG(torch.from_numpy(z)).cpu().numpy()))
    # --init continues from it: weights, running statistics, square averages and step counts
    again = cli.make_trainer(cli.parse_args(argv + ['--init', out_dir + '/weights_last.pt']), config)
    assert again.steps == [2, 4] and all(same_bits(a[k], b[k]) for a, b in zip(again.state_dicts(), want) for k in b)
    assert same_bits(again.tensor('d', 'main.final:128-1:conv.weight', 'square_avg'), tr.tensor('d', 'main.final:128-1:conv.weight', 'square_avg'))
    # test_wgan reads weights_epoch6000.pt of its target directory
    import shutil
    shutil.copy(out_dir + '/weights_last.pt', out_dir + '/weights_epoch6000.pt')
    res = test_wgan.main(['--synthetic', '--seed', '1', '--kept_samples', '4', '--total_steps', '2', '--snr_range', '0', '10', '--l2lam_range', '1', '--lr_range', '0.01',
                          '--alpha_range', '0.6', '--noise', 'host', '--gpu', '0'])
    assert res['oracle_log'].shape == (1, 1, 1, 2, 2, 4) and np.all(np.isfinite(res['oracle_log'])) and np.all(res['meas_log'] > 0)
