"""The cases of the whole-network training comparison (tests/test_gpu_train_autograd.py on the GPU,
tests/test_train_autograd_cpu.py for their admissibility without one) -- test infrastructure, nothing of the library's
kernels is involved.

A case fixes the array (Nt x Nr), the batch, the loss path and the weights; its inputs are drawn from a seed.  Labels
always hold class 0 and class ``num_classes - 1`` (sigma = 39.15 and 4e-4 in one batch) where the batch has room for both.
"""
import collections

import numpy as np

Case = collections.namedtuple('Case', 'name nt nr B anneal_power world weights seed scale')

SEEDED, TRAINED = 'seeded', 'trained'
CASES = [
    # geometry: 64x16 is the network's default; the others put widths of 2 and 1 and images of 16 and 4 pixels at the low levels
    Case('64x16_b1', 64, 16, 1, 2.0, 1, SEEDED, 101, 0.7),
    Case('64x16_b3', 64, 16, 3, 2.0, 1, SEEDED, 102, 0.7),
    Case('16x64_b2', 16, 64, 2, 2.0, 1, SEEDED, 103, 0.7),
    Case('32x32_b2', 32, 32, 2, 2.0, 1, SEEDED, 104, 0.7),
    Case('128x8_b2', 128, 8, 2, 2.0, 1, SEEDED, 105, 0.7),
    Case('16x16_b5', 16, 16, 5, 2.0, 1, SEEDED, 394, 0.7),       # 5 * 4 = 20 pixels at the lowest level: a partial wgrad tile
    # (16 x 16 ends in 2 x 2 images.  InstanceNorm++ over FOUR pixels divides by sqrt(var + 1e-5) of planes that are nearly constant,
    # and the 5 x 5 max pool of a 2 x 2 image picks one pixel for the whole plane, so one near-tie re-routes a whole channel: a
    # float32 evaluation of this geometry sits around the bounds themselves -- median 3 x the half bounds over 120 seeds, and it moves
    # by 2 x with the summation order (1, 3 or 8 threads).  Seed 394 is the one seed of 300 ... 419 whose float32 restatement stays
    # within half of the bounds at both anneal powers and at all three thread counts; it was chosen by that figure alone, on the CPU)
    # loss paths, on the inputs of 16x16_b5
    Case('16x16_b5_power1.5', 16, 16, 5, 1.5, 1, SEEDED, 394, 0.7),   # powf
    Case('16x16_b5_world2', 16, 16, 5, 2.0, 2, SEEDED, 394, 0.7),     # grad_scale = 1/2
    # weights after 4000 optimiser steps (tests/trained_weights.py): small gradients that cancel; the checkpoint only exists
    # on the GPU, so the GPU test checks this case's admissibility itself
    Case('64x16_b2_trained', 64, 16, 2, 2.0, 1, TRAINED, 107, 0.7),
]
CPU_CASES = [c for c in CASES if c.weights == SEEDED]
UNTILEABLE = (24, 8)             # its 12 x 4 level is neither a multiple nor a divisor of conv_wgrad's 64-pixel tile
TWO_STEP = Case('16x16_b5_two_steps', 16, 16, 5, 2.0, 1, SEEDED, 108, 0.7)


def make_inputs(case, num_classes, step=0):
    """x, z ``[B, 2, Nt, Nr]`` float32 and labels ``[B]``: x of the scale of a normalised channel, labels with both ends of
    the noise schedule (a single sample takes the low-noise end, where the 1 / sigma of the output is largest)."""
    rng = np.random.default_rng([case.seed, step])
    shape = (case.B, 2, case.nt, case.nr)
    x = (case.scale * rng.standard_normal(shape)).astype(np.float32)
    z = rng.standard_normal(shape).astype(np.float32)
    labels = rng.integers(0, num_classes, size=case.B).astype(np.int64)
    labels[0] = num_classes - 1
    if case.B > 1:
        labels[1] = 0
    return x, labels, z


def case_config(case):
    from score_based_channels_amd.config import default_config
    cfg = default_config('CDL-C', image_size=(case.nr, case.nt))
    cfg.training.anneal_power = case.anneal_power
    return cfg


_REF = {}


def reference(case, sd, dtype):
    """(scores, per-sample loss, gradients) of the case from tests/scorenet_autograd.py in ``dtype``, computed once per
    (inputs, loss path, dtype) and shared: ``world`` only scales the gradients by the power of two 1 / world, exactly."""
    import scorenet_autograd as SA
    key = (case.nt, case.nr, case.B, case.anneal_power, case.weights, case.seed, case.scale, str(dtype))
    if key not in _REF:
        x, labels, z = make_inputs(case, len(sd['sigmas']))
        _REF[key] = SA.loss_and_grads(sd, x, labels, z, case.anneal_power, 1.0, dtype)
    scores, per, grads = _REF[key]
    if case.world != 1:
        grads = {k: v / case.world for k, v in grads.items()}
    return scores, per, grads
