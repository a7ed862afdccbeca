"""L-DAMP training without a GPU: the restated training step (tests/ldamp_train_oracle.py) against numbers made by the reference's own modules
(tests/gen_golden_ldamp_train.py), the host-side refusals of ``ldamp.Trainer``, the command line's defaults and checkpoint layout around a
stubbed trainer, the new symbols of the header, and that the rules of tests/test_gpu_ldamp_train.py can test their cases."""
import os
import re

import numpy as np
import pytest
import torch

import ldamp_train_cases as cases
import ldamp_train_oracle as T
from conftest import ROOT, load_golden
from score_based_channels_amd import _lib, ldamp, train_ldamp


@pytest.fixture(scope='module')
def golden():
    return load_golden('ldamp_train_step.npz')


def test_oracle_float64_matches_the_reference_training_step(golden):
    """Loss, NMSE and, per tensor, gradient norm and inner product with a seeded probe, float64 against float64 of two implementations of
    the same arithmetic.  The generator measured a worst relative distance of 1.4e-15; 1e-12 leaves room for another BLAS."""
    g = golden
    U = int(g['unrolls'])
    sd = ldamp.seeded_state_dict(int(g['seed_weights']), U)
    res = T.step_gradients(sd, g['Y_herm'], g['P_herm'], g['eig1'], g['H_herm_cplx'], g['directions'][0].astype(np.float32), U, torch.float64)
    assert abs(res['loss'] / g['loss64'][0] - 1) < 1e-12 and abs(res['nmse'] / g['nmse64'][0] - 1) < 1e-12
    names = [str(n) for n in g['grad_names']]
    assert sorted(res['grads']) == names and len(names) == 19 * U
    for i, k in enumerate(names):
        gr = res['grads'][k]
        assert abs(np.linalg.norm(gr) / g['grad_norm64'][i] - 1) < 1e-12, k
        dot = np.sum(gr * cases.probe(k, gr.shape, g['seed_probe']))
        assert abs(dot - g['grad_dot64'][i]) < 1e-12 * g['grad_norm64'][i] * np.sqrt(gr.size), k


def test_oracle_adam_steps_follow_the_reference_losses(golden):
    """Three steps of the oracle with torch's Adam at the fixture's learning rates: the float64 losses of steps 1 and 2 depend on the updates."""
    g = golden
    U = int(g['unrolls'])
    sd = {k: v.astype(np.float64) for k, v in ldamp.seeded_state_dict(int(g['seed_weights']), U).items()}
    params = {k: torch.nn.Parameter(torch.from_numpy(v)) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), 1e-3)
    for s in range(3):
        for grp in opt.param_groups:
            grp['lr'] = float(g['lrs'][s])
        h = T.forward(params, g['Y_herm'], g['P_herm'], g['eig1'], g['directions'][s].astype(np.float32), U, torch.float64)
        loss, nmse = T.loss_nmse(h, torch.from_numpy(g['H_herm_cplx']).to(torch.complex128))
        assert abs(float(loss.detach()) / g['loss64'][s] - 1) < 1e-10 and abs(float(nmse.detach()) / g['nmse64'][s] - 1) < 1e-10, s
        opt.zero_grad()
        loss.backward()
        opt.step()


def test_imposed_masks_reproduce_the_natural_gradient_and_make_orders_comparable():
    """With its own masks imposed a run repeats itself; and the rules of the GPU tests can test their cases: under one set of masks the
    single-axis-flip float32 orders (stand-ins for a kernel) stay within rule R's factor of the native / flipped pair, per tensor at 1, 2
    and 3 unrolls and per net at 10 unrolls."""
    B, Np = 4, 38
    for U in (1, 2, 3, 10):
        r64n = cases.oracle(B, Np, U, torch.float64)
        masks = T.natural_masks(r64n)
        r64 = cases.oracle(B, Np, U, torch.float64, masks=masks)
        if U == 1:
            for k in r64['grads']:
                assert T.grad_error(r64['grads'][k], r64n['grads'][k]) < 1e-12, k
        r32 = {o: cases.oracle(B, Np, U, torch.float32, o, masks) for o in cases.ORDERS}
        worst = 0.0
        if U <= 3:
            for k in r64['grads']:
                for o in ('rows', 'cols'):
                    e, e_ref = cases.rule_r(r32[o]['grads'][k], r64['grads'][k], [r32['native']['grads'][k], r32['flipped']['grads'][k]])
                    worst = max(worst, e / e_ref)
        else:
            for u in range(U):
                ref = T.per_net(r64['grads'], u)
                for o in ('rows', 'cols'):
                    e, e_ref = cases.rule_r(T.per_net(r32[o]['grads'], u), ref, [T.per_net(r32['native']['grads'], u), T.per_net(r32['flipped']['grads'], u)])
                    worst = max(worst, e / e_ref)
        print('unrolls %d: worst ratio of a single-axis order to e_ref %.2f' % (U, worst))
        assert worst <= cases.FACTOR, U


def _bare_trainer(max_unrolls=3, capacity=4):
    t = ldamp.Trainer.__new__(ldamp.Trainer)
    _lib.DeviceHandle.__init__(t)
    t.max_unrolls, t.capacity, t.lr, t.steps, t.trained_unrolls = max_unrolls, capacity, 1e-3, 0, 0
    return t


def test_trainer_refuses_on_the_host_before_the_library_is_called():
    for kw in (dict(capacity=0), dict(capacity=129), dict(capacity=2.5), dict(lr=-1.0), dict(lr=float('nan')), dict(lr='x')):
        with pytest.raises(ValueError):
            ldamp.Trainer({'max_unrolls': 2}, **kw)
    for hp in ({'backbone': 'DnCNN'}, {'shared_nets': True}, {'max_unrolls': 0}):
        with pytest.raises(ValueError):
            ldamp.Trainer(hp)
    with pytest.raises(KeyError):
        ldamp.Trainer({'max_unrolls': 2}, {'nothing': np.zeros(1)})
    t = _bare_trainer()
    c64 = lambda *s: torch.zeros(*s, dtype=torch.complex64)                          # noqa: E731
    ok = {'Y_herm': c64(2, 38, 16), 'P_herm': c64(2, 38, 64), 'eig1': torch.ones(2), 'H_herm_cplx': c64(2, 64, 16)}
    bad = [dict(ok, H_herm_cplx=c64(2, 16, 64)), dict(ok, H_herm_cplx=c64(3, 64, 16)), dict(ok, Y_herm=c64(2, 38, 8)), dict(ok, eig1=torch.ones(3)),
           dict(ok, P_herm=c64(2, 38, 64).to(torch.complex128)), dict(ok, Y_herm=c64(5, 38, 16), P_herm=c64(5, 38, 64), eig1=torch.ones(5), H_herm_cplx=c64(5, 64, 16)),
           dict(ok, Y_herm=c64(2, 65, 16), P_herm=c64(2, 65, 64))]
    for sample in bad:
        with pytest.raises(ValueError):
            t.step(sample, 2)
    for U in (0, 4, 1.5):
        with pytest.raises(ValueError):
            t.step(ok, U)
    with pytest.raises(ValueError):
        t.step(ok, 2, directions=np.zeros((2, 2, 64, 16), np.float32))
    with pytest.raises(ValueError):
        t.step(ok, 2, sample_ids=[0, 2])
    t.steps, t.trained_unrolls = 5, 3
    with pytest.raises(ValueError, match='per-net step counts'):
        t.step(ok, 2)
    with pytest.raises(ValueError):
        t.set_lr(-1)
    # an empty batch returns without a launch (the bare trainer has no handle to launch with)
    empty = {'Y_herm': c64(0, 38, 16), 'P_herm': c64(0, 38, 64), 'eig1': torch.ones(0), 'H_herm_cplx': c64(0, 64, 16)}
    loss, nmse = t.step(empty, 3)
    assert loss != loss and nmse != nmse and t.steps == 5


def test_cli_defaults_are_the_reference_scripts():
    a = train_ldamp.parse_args([])
    assert (a.gpu, a.alpha, a.train) == (0, 0.6, 'CDL-C') and list(a.snr_range) == [-10, -5, 0, 5, 10, 15, 20, 25, 30]
    assert (a.synthetic, a.n_epochs, a.batch_size, a.max_steps, a.init) == (False, None, None, None, None)
    c = train_ldamp.make_config(a, 5.0)
    assert (c.optim.lr, c.training.batch_size, c.training.n_epochs, c.training.decay_epochs, c.training.decay_gamma) == (1e-3, 128, 24, 16, 0.1)
    assert c.data.num_pilots == 38 and c.model.max_unrolls == 10 and c.model.backbone == 'FlippedUNet' and c.model.shared_nets is False
    assert np.allclose(c.data.noise_std, 10 ** (-5.0 / 20) * np.sqrt(64)) and c.data.norm_channels == 'global'
    assert [train_ldamp.step_lr(e) for e in (0, 15, 16, 23)] == [1e-3, 1e-3, 1e-3 * 0.1, 1e-3 * 0.1]
    sched = torch.optim.lr_scheduler.StepLR(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], 1e-3), 16, gamma=0.1)
    for _ in range(17):
        sched.optimizer.step()
        sched.step()
    ours, theirs = train_ldamp.scheduler_state(17), sched.state_dict()
    assert {k: ours[k] for k in ('step_size', 'gamma', 'base_lrs', 'last_epoch', '_step_count')} == {k: theirs[k] for k in ('step_size', 'gamma', 'base_lrs', 'last_epoch', '_step_count')}
    assert np.isclose(ours['_last_lr'][0], theirs['_last_lr'][0], rtol=1e-12)
    rng = np.random.Generator(np.random.PCG64(0))
    batches = train_ldamp.epoch_batches(300, 128, rng)
    assert [len(b) for b in batches] == [128, 128] and len(set(np.concatenate(batches))) == 256
    assert train_ldamp.log_line(1, 2, 3.14159, 10.0, 0.1) == 'Epoch 1, Step 2, Train Loss 3.142, Train SNR 10.00 dB, Train NMSE -10.000 dB'
    for argv in (['--batch_size', '129'], ['--max_steps', '0'], ['--n_epochs', '0']):
        with pytest.raises(SystemExit):
            train_ldamp.parse_args(argv)


class _StubTrainer:
    """what train_ldamp reads of ldamp.Trainer"""
    def __init__(self, max_unrolls):
        self.sd = ldamp.seeded_state_dict(1, max_unrolls)
        self.spec = ldamp.state_dict_spec(max_unrolls)
        self.calls, self.lr = [], None

    def set_lr(self, lr):
        self.lr = lr

    def step(self, sample, num_unrolls, seed=0, sample_ids=None):
        self.calls.append((tuple(sample['Y_herm'].shape), tuple(sample['H_herm_cplx'].shape), sample['eig1'].dtype, num_unrolls, seed, list(sample_ids), self.lr))
        return 2.0 / len(self.calls), 0.5 / len(self.calls)

    def state_dict(self):
        return self.sd

    def optimizer_state_dict(self):
        n = len(self.spec)
        state = {i: {'step': torch.tensor(float(len(self.calls))), 'exp_avg': torch.zeros(s), 'exp_avg_sq': torch.zeros(s)} for i, (_, s) in enumerate(self.spec)}
        return {'state': state, 'param_groups': [ldamp.adam_param_group(self.lr, n)]}


def test_cli_checkpoint_layout_around_a_stubbed_trainer(tmp_path, monkeypatch, capsys):
    from score_based_channels_amd.checkpoint import load_checkpoint
    from score_based_channels_amd.test_ldamp import checkpoint_path
    monkeypatch.chdir(tmp_path)
    made = []

    def trainer_fn(args, config, device):
        made.append(_StubTrainer(int(config.model.max_unrolls)))
        return made[-1]
    written = train_ldamp.main(['--synthetic', '--snr_range', '0', '10', '--batch_size', '8', '--max_steps', '2', '--seed', '3'], trainer_fn=trainer_fn)
    assert written == [checkpoint_path('CDL-C', 0.0, 0.6), checkpoint_path('CDL-C', 10.0, 0.6)] and len(made) == 2
    assert made[0].calls[0][:5] == ((8, 38, 16), (8, 64, 16), torch.float32, 10, 3) and made[0].calls[1][5] == list(range(8, 16)) and made[0].calls[0][6] == 1e-3
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('Epoch')]
    assert lines[0] == 'Epoch 0, Step 0, Train Loss 2.000, Train SNR 0.00 dB, Train NMSE -3.010 dB' and len(lines) == 4
    c = load_checkpoint(written[1])                      # as test_ldamp reads it
    assert set(c) == {'model_state', 'optimizer_state', 'scheduler_state', 'config', 'args', 'loss_log', 'nmse_log'}
    assert c['loss_log'] == [2.0, 1.0] and c['nmse_log'] == [0.5, 0.25] and c['args']['alpha'] == 0.6
    assert c['config'].model.max_unrolls == 10 and c['config'].data.num_pilots == 38 and c['config'].data.train_snr[0] == 10.0
    assert c['scheduler_state']['last_epoch'] == 0 and c['scheduler_state']['step_size'] == 16
    ldamp.check_state_dict(_lib.numpy_state_dict(c['model_state']), ldamp.check_hparams(c['config'].model))
    # torch's own optimiser accepts the state
    ps = [torch.nn.Parameter(torch.zeros(s)) for _, s in ldamp.state_dict_spec(10)]
    opt = torch.optim.Adam(ps, 1e-3)
    opt.load_state_dict(c['optimizer_state'])
    assert opt.state[ps[0]]['step'] == 2


def test_header_declares_the_trainer_and_python_binds_it():
    text = open(os.path.join(ROOT, 'include', 'sbc_hip.h')).read()
    names = ('create', 'destroy', 'workspace_floats', 'step', 'adam', 'stage', 'get_state', 'set_state')
    for n in names:
        assert re.search(r'\bsbc_ldamp_trainer_%s\(' % n, text), n
    fields = re.search(r'typedef struct sbc_ldamp_step_desc \{(.*?)\} sbc_ldamp_step_desc;', text, re.S).group(1)
    declared = re.findall(r'(\w+)\s*(?:,|;)', re.sub(r'/\*.*?\*/', '', fields, flags=re.S))
    assert declared == [f[0] for f in _lib.sbc_ldamp_step_desc._fields_]
    assert len(ldamp.STAGES) == 23 and ldamp.N_NET_TENSORS == 19 and ldamp.TRAIN_DIV == 5
