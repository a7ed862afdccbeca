"""The training step against float64 autograd on every geometry ``TrainNet`` accepts: per case of tests/train_cases.py,
``TrainNet.backward`` on replayed noise against tests/scorenet_autograd.py in float64 -- the per-sample loss and EVERY element
of all 229 gradient tensors, in the metric and at the bounds of
test_gpu_train.py::test_parameter_gradients_match_reference_autograd (which samples 24 elements per tensor of one case).
The references are computed here, once per case, on the CPU; tests/test_train_autograd_cpu.py pins the restatement and shows
that every case is fair (a float32 evaluation of it stays within half of these bounds: "e_ref")."""
import glob
import os

import numpy as np
import pytest
import torch

import scorenet_autograd as SA
import train_cases as TC
from test_gpu_train import GRAD_ELEM_TOL, GRAD_NORM_RTOL, LOSS_RTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """The 4000-step checkpoint of tests/trained_weights.py.  Training is reproducible bit for bit, so a checkpoint that
    test_gpu_parity.py already wrote under this session's temporary directory is the same one: reuse it, else train."""
    import trained_weights as TW
    from score_based_channels_amd.checkpoint import load_checkpoint
    found = sorted(glob.glob(os.path.join(str(tmp_path_factory.getbasetemp()), 'trained%d*' % TW.LONG_STEPS, 'final_model.pt')))
    if found:
        sd = load_checkpoint(found[0])['model_state']
        return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else v) for k, v in sd.items()}
    return TW.train_checkpoint(tmp_path_factory.mktemp('trained%d_autograd' % TW.LONG_STEPS), TW.LONG_STEPS)[1]


def _trainer(case, sd):
    from score_based_channels_amd.train import TrainNet
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return TrainNet(TC.case_config(case), batch=case.B, nt=case.nt, nr=case.nr, world=case.world).load_state_dict(sd)


def _compare(case, sd):
    """Run the case on the device and hold it to float64; prints the worst figures beside the case's e_ref first."""
    x, labels, z = TC.make_inputs(case, len(sd['sigmas']))
    _, per64, g64 = TC.reference(case, sd, torch.float64)
    _, per32, g32 = TC.reference(case, sd, torch.float32)
    net = _trainer(case, sd)
    per = net.backward(x, labels, z).cpu().numpy()
    grads = net.grad_dict()
    assert len(grads) == 229 and set(grads) == set(g64)
    e_loss = float(np.max(np.abs(per / per64 - 1)))
    e_norm, n_norm, e_elem, n_elem = SA.gradient_errors(grads, g64)
    r_norm, _, r_elem, _ = SA.gradient_errors(g32, g64)
    r_loss = float(np.max(np.abs(per32 / per64 - 1)))
    print('%s: loss %.2e (e_ref %.2e), gradient norm %.2e at %s (e_ref %.2e), element %.2e at %s (e_ref %.2e)'
          % (case.name, e_loss, r_loss, e_norm, n_norm, r_norm, e_elem, n_elem, r_elem))
    if case.weights == TC.TRAINED:          # its weights only exist here: the fairness condition the CPU test holds the others to
        assert r_loss < LOSS_RTOL / 2 and r_norm < GRAD_NORM_RTOL / 2 and r_elem < GRAD_ELEM_TOL / 2, (r_loss, r_norm, r_elem)
    assert all(np.isfinite(v).all() for v in grads.values())
    assert e_loss < LOSS_RTOL, e_loss
    assert e_norm < GRAD_NORM_RTOL, (n_norm, e_norm)
    assert e_elem < GRAD_ELEM_TOL, (n_elem, e_elem)
    return net


@pytest.mark.parametrize('case', TC.CASES, ids=[c.name for c in TC.CASES])
def test_loss_and_all_gradients_match_float64_autograd(weights64, request, case):
    _compare(case, request.getfixturevalue('trained') if case.weights == TC.TRAINED else weights64[1])


def test_world_two_gradients_are_half_of_world_one(weights64):
    """``grad_scale = 1 / world`` multiplies d(loss)/d(scores) by a power of two: every later product and sum scales exactly."""
    sd = weights64[1]
    one = next(c for c in TC.CASES if c.name == '16x16_b5')
    two = next(c for c in TC.CASES if c.name == '16x16_b5_world2')
    x, labels, z = TC.make_inputs(one, len(sd['sigmas']))
    nets = [_trainer(c, sd) for c in (one, two)]
    pers = [n.backward(x, labels, z).clone() for n in nets]
    assert torch.equal(pers[0], pers[1]) and torch.equal(nets[1].grads, 0.5 * nets[0].grads)


def test_a_shape_the_reverse_kernels_cannot_tile_is_refused_at_construction(weights64):
    """Nt24 x Nr8: the forward pass takes it, conv_wgrad's 64-pixel tiling does not take its 12 x 4 level.  Either the whole
    comparison passes or ``TrainNet`` says so when it is built -- never an error out of the middle of a step."""
    nt, nr = TC.UNTILEABLE
    case = TC.Case('%dx%d_b2' % (nt, nr), nt, nr, 2, 2.0, 1, TC.SEEDED, 109, 0.7)
    try:
        _trainer(case, weights64[1])
    except ValueError as e:
        assert '12x4' in str(e)
        return
    _compare(case, weights64[1])


def test_two_optimiser_steps_match_float32_adam_on_the_restatement(weights64):
    """``TrainNet.step`` twice at 16 x 16 on replayed batches against the restatement driven in float32 by
    ``torch.optim.Adam(lr, betas, eps = 1e-3)``: the loss of step 2 sees the parameters step 1 wrote."""
    sd = weights64[1]
    case = TC.TWO_STEP
    net = _trainer(case, sd)
    p = SA.parameters(sd, torch.float32)
    opt = torch.optim.Adam(list(p.values()), lr=net.lr, betas=(net.beta1, 0.999), eps=net.eps, weight_decay=0.0, amsgrad=False)
    assert net.eps == 1e-3
    got, want = [], []
    for k in range(2):
        x, labels, z = TC.make_inputs(case, len(sd['sigmas']), step=k)
        got.append(float(net.step(x, labels, z).cpu().numpy().astype(np.float64).mean()))
        opt.zero_grad()
        loss = SA.dsm_loss(p, sd['sigmas'], x, labels, z, case.anneal_power)[1].mean()
        loss.backward()
        opt.step()
        want.append(float(loss.item()))
    print('two steps: losses %r against %r, relative %.2e / %.2e' % (got, want, abs(got[0] / want[0] - 1), abs(got[1] / want[1] - 1)))
    assert net.optimizer_state()['step'] == 2
    assert abs(got[1] / want[1] - 1) < 5e-5 and abs(got[0] / want[0] - 1) < 5e-5
