"""WGAN training without a GPU: the oracle (tests/wgan_train_oracle.py) against torch's own modules and optimiser, its two float32 orders
against each other, the state-dict specs and initial distributions of wgan.py, and the header against the library's exports."""
import os
import re

import numpy as np
import pytest
import torch

import wgan_train_oracle as T
from conftest import ROOT
from score_based_channels_amd import _lib, wgan

F32, F64 = torch.float32, torch.float64


def problem(n_extra, Br, Bf, seed=5):
    gsd, dsd = wgan.init_state_dicts(seed, n_extra)
    dsd = {k: (T.clamp(v) if v.dtype == np.float32 and not k.endswith(('running_mean', 'running_var')) else v) for k, v in dsd.items()}
    rng = np.random.default_rng(seed)
    return gsd, dsd, rng.standard_normal((Br, 2, 16, 64)).astype(np.float32), rng.standard_normal((Bf, 60)).astype(np.float32)


def torch_critic(n_extra):
    """nn.Sequential of the reference critic's layers under the reference's module names"""
    import torch.nn as nn
    main = nn.Sequential()
    main.add_module('initial:2-64:conv', nn.Conv2d(2, 64, 4, 2, 1, bias=False))
    main.add_module('initial:64:relu', nn.LeakyReLU(0.2))
    for t in range(n_extra):
        main.add_module('extra-layers-%d:64:conv' % t, nn.Conv2d(64, 64, 3, 1, 1, bias=False))
        main.add_module('extra-layers-%d:64:batchnorm' % t, nn.BatchNorm2d(64))
        main.add_module('extra-layers-%d:64:relu' % t, nn.LeakyReLU(0.2))
    main.add_module('pyramid:64-128:conv', nn.Conv2d(64, 128, 4, 2, 1, bias=False))
    main.add_module('pyramid:128:batchnorm', nn.BatchNorm2d(128))
    main.add_module('pyramid:128:relu', nn.LeakyReLU(0.2))
    main.add_module('final:128-1:conv', nn.Conv2d(128, 1, (4, 16), 1, (0, 0), bias=False))
    m = nn.Module()
    m.main = main
    return m


@pytest.mark.parametrize('n_extra', [0, 1, 3])
def test_critic_spec_is_the_state_dict_of_the_layer_list(n_extra):
    m = torch_critic(n_extra)
    spec = wgan.disc_state_dict_spec(n_extra)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(s)) for k, s in spec]
    _, dsd = wgan.init_state_dicts(3, n_extra)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in dsd.items()}, strict=True)
    d = wgan.DCGAN_D([16, 64], 60, 2, 64, 1, n_extra).load_state_dict(dsd)
    assert list(d.state_dict()) == [k for k, _ in spec]
    with pytest.raises(KeyError):
        wgan.DCGAN_D([16, 64], 60, 2, 64, 1, n_extra + 1).load_state_dict(dsd)
    with pytest.raises(ValueError):
        wgan.DCGAN_D([32, 64], 60, 2, 64, 1, n_extra)


def test_oracle_critic_is_torchs_module_in_training_mode():
    """forward, running statistics and gradients of the oracle's layer list equal nn.Sequential's in float64"""
    gsd, dsd, real, _ = problem(1, 3, 3)
    m = torch_critic(1).double()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in dsd.items()})
    m.train()
    out = m.main(torch.from_numpy(real).double()).mean(0).view(1)
    out.backward(torch.ones(1, dtype=F64))
    D = T._leaves(dsd, F64)
    o = T.d_forward(D, real, F64)
    o['err'].backward(torch.ones(1, dtype=F64))
    assert abs(float(out) - float(o['err'])) <= 1e-12 * abs(float(out)) + 1e-18
    for name, p in m.named_parameters():
        assert T.normwise_all(D[name].grad.numpy(), p.grad.numpy()) < 1e-9, name
    bn = 'main.extra-layers-0:64:batchnorm'
    rm, rv = T.running_update(dsd[bn + '.running_mean'], dsd[bn + '.running_var'], o['mean'][1].detach().numpy(), o['var'][1].detach().numpy(), 3 * 8 * 32)
    sd = m.state_dict()
    assert np.allclose(rm, sd[bn + '.running_mean'].numpy(), rtol=1e-12, atol=1e-15) and np.allclose(rv, sd[bn + '.running_var'].numpy(), rtol=1e-12)
    assert int(sd[bn + '.num_batches_tracked']) == 1


def test_masks_reproduce_the_free_running_pass_and_both_orders_agree():
    """under its own signs the masked oracle is the free-running one; the flipped twin is the same function in float64 (1e-9) and within
    4 x of the native order's error in float32, on every parameter gradient; pre-activations of float32 lie within 1e-5 rms of float64"""
    gsd, dsd, real, noise = problem(1, 2, 3)
    free = T.critic_terms(gsd, dsd, real, noise, F64)
    masks = {n: [p > 0 for p in free[n]['pre'] if p is not None] for n in ('g', 'd0', 'd1')}
    held = T.critic_terms(gsd, dsd, real, noise, F64, masks)
    twin = T.critic_terms_flipped(gsd, dsd, real, noise, F64, masks)
    a32, b32 = T.critic_terms(gsd, dsd, real, noise, F32, masks), T.critic_terms_flipped(gsd, dsd, real, noise, F32, masks)
    for k, g in free['grads'].items():
        assert T.normwise_all(held['grads'][k], g) < 1e-12 and T.normwise_all(twin['grads'][k], g) < 1e-9, k
        ea, eb = T.normwise_all(a32['grads'][k], g), T.normwise_all(b32['grads'][k], g)
        print('%-48s e32 %.2e  twin %.2e' % (k, ea, eb))
        assert max(ea, eb) <= 4 * min(ea, eb) + 1e-9, (k, ea, eb)
    f32 = T.critic_terms(gsd, dsd, real, noise, F32)
    for n in ('g', 'd0', 'd1'):
        for p32, p64 in zip(f32[n]['pre'], free[n]['pre']):
            if p64 is not None:
                assert np.max(np.abs(p32 - p64)) <= 1e-5 * np.sqrt(np.mean(p64 ** 2)), n


def test_generator_bias_gradients_vanish_behind_batchnorm():
    gsd, dsd, _, noise = problem(1, 2, 2)
    r = T.generator_terms(gsd, dsd, noise, F64)
    for k in ('conv.conv1.bias', 'conv.conv2.bias'):
        assert np.linalg.norm(r['grads'][k]) < 1e-12 * np.linalg.norm(r['grads']['conv.conv1.weight'])
    assert set(r['grads']) == {k for k in gsd if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}


@pytest.mark.parametrize('foreach', [False, True])
def test_oracle_rmsprop_continues_torch_rmsprop(foreach):
    """three steps from a drawn state, sq 1e-16 .. 1e2, gradients 1e-6 .. 1e3: bit-identical to torch.optim.RMSprop in float32"""
    rng = np.random.default_rng(2)
    n = 4096
    p0 = rng.standard_normal(n).astype(np.float32)
    sq0 = (10.0 ** rng.uniform(-16, 2, n)).astype(np.float32)
    pp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.RMSprop([pp], lr=5e-5, foreach=foreach)
    opt.state[pp] = {'step': torch.tensor(7.), 'square_avg': torch.from_numpy(sq0.copy())}
    p, sq = p0, sq0
    for _ in range(3):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
        pp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, sq = T.rmsprop(p, g, sq)
        assert np.array_equal(p, pp.detach().numpy()) and np.array_equal(sq, opt.state[pp]['square_avg'].numpy())
    assert np.array_equal(T.clamp(np.array([-1, -0.01, -0.0099, 0, 0.01, 0.02], np.float32)), np.array([-0.01, -0.01, -0.0099, 0, 0.01, 0.01], np.float32))


def test_initial_distributions():
    g, d = wgan.init_state_dicts(11, 1)
    g2, _ = wgan.init_state_dicts(11, 3)
    assert all(np.array_equal(g[k], g2[k]) for k in g)                      # a tensor depends on the seed and its name only
    for sd in (g, d):
        for k, v in sd.items():
            leaf = k.rsplit('.', 1)[1]
            bn = 'bn' in k or 'batchnorm' in k
            if leaf == 'num_batches_tracked':
                assert v.dtype == np.int64 and int(v) == 0
            elif bn and leaf == 'weight':
                assert abs(v.mean() - 1) < 0.01 and 0.012 < v.std() < 0.03
            elif bn:
                assert np.all(v == (1 if leaf == 'running_var' else 0))
            elif k.startswith('dense.'):
                assert np.max(np.abs(v)) <= 1 / np.sqrt(60) and v.std() > 0.05
            elif leaf == 'weight':
                assert abs(v.mean()) < 2e-3 and abs(v.std() - 0.02) < 2e-3, k
    wgan.check_state_dict(g, 1)
    _lib.check_against_spec(d, wgan.disc_state_dict_spec(1))


def test_stage_names():
    assert wgan.trainer_stage_id('g.act0', 1) == 0 and wgan.trainer_stage_id('g.gen', 0) == 128 and wgan.trainer_stage_id('d1.err', 2) == 512 + 130
    assert wgan.trainer_stage_id('d0.draw3', 1) == 256 + 16 * 7 + 3
    for bad in ('g.act4', 'd0.raw4', 'x.act1', 'g.err', 'd0.gen'):
        with pytest.raises(ValueError):
            wgan.trainer_stage_id(bad, 1)


def test_header_declares_the_training_entry_points():
    header = open(os.path.join(ROOT, 'include', 'sbc_hip.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t|void)\s+(sbc_wgan_(?:trainer_\w+|wgrad128\w*|bn_backward|rmsprop))\s*\(', header, re.M))
    assert declared == {n for n in _lib.EXPORTS if n.startswith(('sbc_wgan_trainer', 'sbc_wgan_wgrad128', 'sbc_wgan_bn_backward', 'sbc_wgan_rmsprop'))}
    assert len(declared) == 11
    h = _lib.lib()
    for n in declared:
        assert hasattr(h, n), n


# ---- the fixture written from the reference modules (tests/gen_golden_wgan_train.py) ------------------------------------------------------
def golden_train():
    import json
    from conftest import GOLDEN, load_golden
    g = load_golden('wgan_train_step.npz')
    with open(os.path.join(GOLDEN, 'wgan_disc_state_dict_keys.json')) as f:
        g['disc_keys'] = json.load(f)
    return g


def fixture_index(numel):
    return np.arange(numel) if numel <= 4096 else np.arange(0, numel, numel // 2048)[:2048]


def test_critic_spec_is_the_reference_modules_state_dict():
    g = golden_train()
    assert g['disc_keys'] == [k for k, _ in wgan.disc_state_dict_spec(int(g['n_extra']))]


def test_oracle_against_the_fixture():
    """the restated loop equals the reference modules': float64 losses and every stored gradient value to 1e-9, and the oracle's float32
    lies within 4 x the reference's own float32 distance from float64 (e_ref of the fixture) on every parameter tensor"""
    g = golden_train()
    gsd, dsd = wgan.init_state_dicts(int(g['seed']), int(g['n_extra']))
    dsd = {k: (T.clamp(v) if v.dtype == np.float32 and not k.endswith(('running_mean', 'running_var')) else v) for k, v in dsd.items()}
    c64, c32 = T.critic_terms(gsd, dsd, g['real'], g['noise_c'], F64), T.critic_terms(gsd, dsd, g['real'], g['noise_c'], F32)
    g64, g32 = T.generator_terms(gsd, dsd, g['noise_g'], F64), T.generator_terms(gsd, dsd, g['noise_g'], F32)
    for k, r in (('errD_real', c64), ('errD_fake', c64), ('errG', g64)):
        assert abs(float(r[k][0]) - float(g[k + '64'][0])) <= 1e-9 * abs(float(g[k + '64'][0])), k
    n = 0
    for net, r64, r32 in (('d', c64, c32), ('g', g64, g32)):
        for name, grad in r64['grads'].items():
            ref = g['%s/grad64/%s' % (net, name)]
            got = grad.ravel()[fixture_index(grad.size)]
            assert np.linalg.norm(got - ref) <= 1e-9 * float(g['%s/norm/%s' % (net, name)]) + 1e-15, name           # (+ 1e-15: conv1 / conv2 bias, true value 0, float64 noise 1e-18)
            e32 = np.linalg.norm(r32['grads'][name].astype(np.float64) - grad)
            print('%-48s oracle e32 %.2e  fixture e_ref %.2e' % (name, e32, float(g['%s/eref/%s' % (net, name)])))
            assert e32 <= 4 * float(g['%s/eref/%s' % (net, name)]), name
            n += 1
    assert n == 8 + 15
    # the fixture is flip-free: float32 and float64 of the oracle agree on every sign too
    for a, b in ((c32, c64), (g32, g64)):
        for netk in ('g', 'd0', 'd1'):
            if netk in a:
                assert all(np.array_equal(p > 0, q > 0) for p, q in zip(a[netk]['pre'], b[netk]['pre']) if q is not None), netk


# ---- the command line: arguments, schedule, checkpoint ------------------------------------------------------------------------------------
def test_cli_schedule():
    from score_based_channels_amd import train_wgan as cli
    assert [cli.diters_for(k) for k in (0, 24, 25, 26, 499, 500, 501, 1000)] == [100, 100, 5, 5, 5, 100, 5, 100]
    assert cli.diters_for(30, diters=3, initial=7) == 3 and cli.diters_for(3, diters=3, initial=7) == 7
    # an epoch of 12 batches at gen_iterations 30: 5 + 5 + 2 (the inner loop ends with the epoch's batches)
    assert cli.epoch_plan(12, 30) == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11]]
    # the first epochs: one generator iteration per epoch, all batches to the critic
    assert cli.epoch_plan(12, 0) == [list(range(12))]
    # Diters changes inside an epoch when gen_iterations reaches 25, and at a multiple of 500
    assert [len(t) for t in cli.epoch_plan(12, 24, diters=2, initial=4)] == [4, 2, 2, 2, 2]
    assert [len(t) for t in cli.epoch_plan(9, 499, diters=2, initial=4)] == [2, 4, 2, 1]
    assert cli.epoch_plan(0, 5) == []
    rng = np.random.Generator(np.random.PCG64(3))
    b = cli.epoch_batches(10, 4, rng)
    assert [len(x) for x in b] == [4, 4, 2] and sorted(np.concatenate(b)) == list(range(10))
    z = cli.draw_noise(np.random.Generator(np.random.PCG64(3)), 5)
    assert z.shape == (5, 60) and z.dtype == np.float32 and np.array_equal(z, cli.draw_noise(np.random.Generator(np.random.PCG64(3)), 5))


def test_cli_arguments_config_and_log_line():
    from score_based_channels_amd import train_wgan as cli
    a = cli.parse_args([])
    c = cli.make_config(a)
    assert (a.seed, a.save_every, a.init, a.out_dir, a.max_gen_iterations) == (2020, 500, None, None, None)
    assert (c.niter, c.batchSize, c.Diters, c.lrD, c.lrG, c.clamp_lower, c.clamp_upper, c.nz, c.ndf, c.ngf, c.n_extra_layers) == (3000, 200, 5, 5e-5, 5e-5, -0.01, 0.01, 60, 64, 128, 1)
    assert cli.model_dir(c) == 'wgan_CDL_D_0.50'
    a = cli.parse_args('--synthetic --seed 1 --niter 3 --max_gen_iterations 2 --batch_size 4 --save_every 1 --out_dir x --Diters 2 --spacing 1.0'.split())
    c = cli.make_config(a)
    assert (c.niter, c.batchSize, c.Diters, c.n_extra_layers, a.synthetic, a.out_dir) == (3, 4, 2, 0, True, 'x') and cli.model_dir(c) == 'wgan_CDL_D_1.00'
    for bad in ('--niter 0', '--batch_size 0', '--save_every 0', '--max_gen_iterations -1', '--Diters 0'):
        with pytest.raises(SystemExit):
            cli.parse_args(bad.split())
    line = cli.log_line(2, 3000, 5, 50, 7, np.float32(0.5), np.float32(0.25), np.float32(-1.5))
    assert line == '[2/3000][5/50][7] Loss_D: 0.250000 Loss_G: -1.500000 Loss_D_real: 0.500000 Loss_D_fake 0.250000'


class HostTrainer:
    """what train_wgan.save asks of a trainer, on the host"""

    def __init__(self, n_extra):
        self.sd = wgan.init_state_dicts(4, n_extra)

    def state_dicts(self):
        return self.sd

    def optimizer_state_dicts(self):
        out = []
        for sd in self.sd:
            names = [k for k in sd if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
            out.append({'state': {i: {'step': np.asarray(3., np.float32), 'square_avg': np.abs(sd[k])} for i, k in enumerate(names)},
                        'param_groups': [dict(lr=5e-5, momentum=0, alpha=0.99, eps=1e-8, centered=False, weight_decay=0, capturable=False, foreach=None,
                                              maximize=False, differentiable=False, params=list(range(len(names))))]})
        return tuple(out)


def test_checkpoint_round_trip_into_test_wgans_loader(tmp_path):
    """a checkpoint of train_wgan.save has the reference's keys, loads through checkpoint.load_checkpoint as test_wgan reads it, its
    states load into torch modules strictly and its optimiser states into torch.optim.RMSprop"""
    from score_based_channels_amd import test_wgan, train_wgan as cli
    from score_based_channels_amd.checkpoint import load_checkpoint
    tr = HostTrainer(1)
    config = cli.make_config(cli.parse_args([]))
    path = str(tmp_path / 'weights_epoch500.pt')
    cli.save(path, tr, config)
    raw = torch.load(path, weights_only=False)
    assert set(raw) == {'gen_state', 'disc_state', 'gen_opt_state', 'disc_opt_state', 'config'}
    c = load_checkpoint(path, required=('config', 'gen_state'))
    state = c['gen_state']
    n_extra = wgan.n_extra_of(state)
    assert n_extra == 1 and wgan.check_geometry(c['config'].imageSize, c['config'].nz, c['config'].nc, c['config'].ngf, n_extra) == 1
    wgan.check_state_dict(_lib.numpy_state_dict(state), 1)
    assert all(np.array_equal(state[k].numpy(), tr.sd[0][k]) for k in tr.sd[0]) and state['conv.bn1.num_batches_tracked'].dtype == torch.int64
    assert c['config'].batchSize == 200 and c['config'].data.spacing_list == [0.5] and test_wgan.wgan_config().toDict() == config.toDict()
    m = torch_critic(1)
    m.load_state_dict(c['disc_state'], strict=True)
    opt = torch.optim.RMSprop(m.parameters(), lr=1.0)
    opt.load_state_dict(c['disc_opt_state'])
    assert opt.param_groups[0]['lr'] == 5e-5 and float(opt.state[next(m.parameters())]['step']) == 3
