"""CPU pins of tests/scorenet_autograd.py, the float64 autograd reference of the training step: its forward against the numpy
oracle, its gradients against the reference project's own autograd (tests/golden/train_dsm.npz), and for every case of
tests/train_cases.py that the case is FAIR -- an honest float32 evaluation of the same operation sits within half of the bounds
the GPU test (tests/test_gpu_train_autograd.py) applies to the kernels."""
import numpy as np
import pytest
import torch

import scorenet_autograd as SA
import train_cases as TC
from conftest import load_golden, rel_err, tensor_digest
from test_gpu_train import GRAD_ELEM_TOL, GRAD_NORM_RTOL, LOSS_RTOL


@pytest.fixture(scope='module')
def golden():
    return load_golden('train_dsm.npz')


@pytest.mark.parametrize('nt,nr', [(64, 16), (16, 64)])
def test_float64_forward_matches_the_numpy_oracle(weights64, nt, nr):
    from oracle import ncsnv2_oracle as O
    cfg, sd = weights64
    rng = np.random.default_rng(nt)
    x = rng.standard_normal((2, 2, nt, nr)).astype(np.float32)
    labels = np.array([3, cfg.model.num_classes - 1])
    err = rel_err(SA.forward(sd, x, labels), O.score_forward(sd, x, labels))
    print('float64 restatement against the fp32 numpy oracle at %dx%d: %.2e' % (nt, nr, err))
    assert err < 2e-5


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['float64', 'float32'])
def test_gradients_match_the_reference_autograd_fixture(weights64, golden, dtype):
    """The digests of the reference's own ``loss.backward()`` at the fixture's batch, in the metric and at the bounds of
    test_gpu_train.py::test_parameter_gradients_match_reference_autograd."""
    cfg, sd = weights64
    _, per, grads = SA.loss_and_grads(sd, golden['x'], golden['labels'], golden['z'], dtype=dtype)
    assert np.max(np.abs(per / golden['loss_per_sample'] - 1)) < LOSS_RTOL
    assert abs(per.astype(np.float64).mean() / golden['loss'] - 1) < LOSS_RTOL
    names = [k[3:] for k in golden if k.startswith('gd_')]
    assert len(names) == 229 and set(names) == set(grads)
    worst_norm, worst_elem = 0.0, 0.0
    for name in names:
        ref, got = golden['gd_' + name], tensor_digest(name, grads[name])
        assert np.isfinite(got).all(), name
        scale = max(np.max(np.abs(ref[2:])), ref[0] / np.sqrt(grads[name].size))
        worst_norm = max(worst_norm, abs(got[0] / ref[0] - 1))
        worst_elem = max(worst_elem, np.max(np.abs(got[2:] - ref[2:])) / scale)
        assert abs(got[0] / ref[0] - 1) < GRAD_NORM_RTOL, (name, got[0], ref[0])
        assert np.max(np.abs(got[2:] - ref[2:])) / scale < GRAD_ELEM_TOL, (name, got[2:6], ref[2:6])
        if 'g_' + name in golden:
            assert rel_err(grads[name], golden['g_' + name]) < GRAD_ELEM_TOL, name
    print('%s restatement against the fixture: worst gradient-norm error %.2e, worst sampled-element error %.2e'
          % (dtype, worst_norm, worst_elem))


@pytest.mark.parametrize('case', TC.CPU_CASES, ids=[c.name for c in TC.CPU_CASES])
def test_case_is_fair_to_a_float32_implementation(weights64, case):
    """e_ref: float32 against float64 of the same restatement, every element of every tensor, within HALF of the GPU bounds."""
    cfg, sd = weights64
    _, per64, g64 = TC.reference(case, sd, torch.float64)
    _, per32, g32 = TC.reference(case, sd, torch.float32)
    assert len(g64) == 229 and all(np.isfinite(v).all() for v in g64.values())
    e_loss = float(np.max(np.abs(per32 / per64 - 1)))
    e_norm, n_norm, e_elem, n_elem = SA.gradient_errors(g32, g64)
    print('e_ref %s: loss %.2e, gradient norm %.2e (%s), element %.2e (%s)' % (case.name, e_loss, e_norm, n_norm, e_elem, n_elem))
    assert e_loss < LOSS_RTOL / 2
    assert e_norm < GRAD_NORM_RTOL / 2, n_norm
    assert e_elem < GRAD_ELEM_TOL / 2, n_elem


def test_world_two_halves_the_reference_exactly(weights64):
    cfg, sd = weights64
    one = next(c for c in TC.CASES if c.name == '16x16_b5')
    two = next(c for c in TC.CASES if c.name == '16x16_b5_world2')
    x, labels, z = TC.make_inputs(two, len(sd['sigmas']))
    _, _, direct = SA.loss_and_grads(sd, x, labels, z, two.anneal_power, 0.5, torch.float64)
    g1, g2 = TC.reference(one, sd, torch.float64)[2], TC.reference(two, sd, torch.float64)[2]
    assert all(np.array_equal(g2[k], 0.5 * g1[k]) and np.array_equal(g2[k], direct[k]) for k in g1)


def test_case_table_holds_what_it_is_meant_to():
    """Both ends of the noise schedule in every batch that has room, and the shapes the reverse kernels treat differently."""
    n = 2311
    for c in TC.CASES:
        _, labels, _ = TC.make_inputs(c, n)
        assert labels[0] == n - 1 and (c.B == 1 or labels[1] == 0), c.name
        assert c.nt % 8 == 0 and c.nr % 8 == 0
    assert {(c.nt, c.nr, c.B) for c in TC.CASES} >= {(64, 16, 1), (64, 16, 3), (16, 64, 2), (32, 32, 2), (128, 8, 2), (16, 16, 5)}
    assert (5 * (16 >> 3) * (16 >> 3)) % 64 == 20


def _two_step_losses(sd, dtype):
    case = TC.TWO_STEP
    p = SA.parameters(sd, dtype)
    opt = torch.optim.Adam(list(p.values()), lr=1e-4, betas=(0.9, 0.999), eps=1e-3)
    out = []
    for k in range(2):
        x, labels, z = TC.make_inputs(case, len(sd['sigmas']), step=k)
        opt.zero_grad()
        loss = SA.dsm_loss(p, sd['sigmas'], x, labels, z, case.anneal_power)[1].mean()
        loss.backward()
        opt.step()
        out.append(float(loss.item()))
    return np.array(out)


def test_two_step_case_is_fair_to_a_float32_implementation(weights64):
    """The loss of the second step after a float32 Adam update against the same loop in float64: half of the 5e-5 the GPU test asks."""
    l64, l32 = _two_step_losses(weights64[1], torch.float64), _two_step_losses(weights64[1], torch.float32)
    print('e_ref two steps: %.2e / %.2e' % tuple(np.abs(l32 / l64 - 1)))
    assert np.max(np.abs(l32 / l64 - 1)) < 2.5e-5 and l64[1] != l64[0]


def test_trainer_refuses_an_array_its_weight_gradient_cannot_tile():
    """``TrainNet`` says at construction (before it touches a device) that Nt24 x Nr8 cannot be trained, and which levels are the
    obstacle; every geometry of the case table passes the same predicate."""
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.config import default_config
    from score_based_channels_amd.train import TrainNet, untileable_levels
    nt, nr = TC.UNTILEABLE
    with pytest.raises(ValueError, match='12x4'):
        TrainNet(default_config('CDL-C', image_size=(nr, nt)), batch=2, nt=nt, nr=nr, device='cpu')
    with pytest.raises(ValueError, match='8x128'):
        TrainNet(default_config('CDL-C', image_size=(128, 8)), batch=2, nt=8, nr=128, device='cpu')
    for c in TC.CASES + [TC.TWO_STEP]:
        assert untileable_levels(P.build_score_plan(32, c.nt, c.nr, 2, share_slots=False)) == [], c.name
    assert untileable_levels(P.build_score_plan(32, 256, 64, 2, share_slots=False)) == []
