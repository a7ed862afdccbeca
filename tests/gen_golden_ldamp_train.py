"""Writes the L-DAMP training fixture from the REFERENCE's own denoiser modules (run where the reference checkout is; never on the GPU box):

    python tests/gen_golden_ldamp_train.py /path/to/reference

``aux_unet.FlippedNormUnet`` is imported by file path, as tests/gen_golden_ldamp.py does; around it run the loop of ``LDAMP.forward``
(aux_models.py:111-190, the perturbed evaluation under no_grad), the loss and NMSE of train_ldamp.py:118-129, autograd,
``torch.optim.Adam(params, 1e-3)`` and ``StepLR`` on the CPU: three steps of 2 unrolls at B = 4, Np = 38, in float32 and in float64.
``StepLR(2, 0.1)`` is stepped after every step, so the third step runs at 1e-4.

  tests/golden/ldamp_train_step.npz   inputs, directions of the three steps (fp16-representable), learning rates, loss and NMSE of every
                                      step in float32 and float64 and, of step 0 in float64, per tensor of nets 0 and 1 the gradient's
                                      norm and its inner product with ``probe(name)`` (the full gradient is 19 MB and is not stored)
Data only; the weights are not stored, only their seed.  Prints the distance of tests/ldamp_train_oracle.py from these numbers: the
tolerance tests/test_ldamp_train_cpu.py can hold.
"""
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ldamp_oracle as O                                         # noqa: E402
import ldamp_train_oracle as T                                   # noqa: E402
from gen_golden_ldamp import reference_nets                      # noqa: E402
from score_based_channels_amd import ldamp                       # noqa: E402

SEED_WEIGHTS, SEED_DATA, SEED_DIRS, SEED_PROBE = 2025, 11, 5, 7
B, NP, UNROLLS, STEPS = 4, 38, 2, 3
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def probe(name, shape):
    """the seeded random tensor a gradient's inner product is taken with"""
    return np.random.default_rng([SEED_PROBE, zlib.crc32(name.encode())]).standard_normal(shape)


def train(holder, Y, P, eig, H, dirs, dtype):
    """STEPS steps of the reference loop -> losses, nmses, learning rates, gradients of step 0 ({name: float64 array})"""
    ctype = torch.complex64 if dtype == torch.float32 else torch.complex128
    opt = torch.optim.Adam(holder.parameters(), 1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, gamma=0.1)
    y, Pm, e, Ht = O._t(Y, ctype), O._t(P, ctype), O._t(eig, dtype), O._t(H, ctype)
    losses, nmses, lrs, grads0 = [], [], [], None
    for s in range(STEPS):
        h = torch.zeros(B, 64, 16, dtype=ctype)
        z = y
        for u in range(UNROLLS):
            net = holder.update_nets[u]
            r = h + 1 / e[:, None, None] * torch.matmul(Pm.transpose(-1, -2).conj(), z)
            r_real = torch.view_as_real(r)
            h_real = net(r_real[:, None])[:, 0]
            h = torch.view_as_complex(h_real)
            with torch.no_grad():
                d = O._t(dirs[s, u], dtype)
                eps = torch.maximum(torch.amax(torch.abs(r), dim=(-1, -2)) * 1e-3, torch.tensor(1e-5, dtype=dtype))
                h_p = net((r_real + eps[:, None, None, None] * d)[:, None])[:, 0]
                div = 1 / eps * torch.mean(d * (h_p - h_real), dim=(-1, -2, -3))
            z = y - torch.matmul(Pm, h) + z * div[:, None, None]
        loss = torch.mean(torch.sum(torch.square(torch.abs(h - Ht)), dim=(-1, -2)))
        with torch.no_grad():
            nmse = torch.mean(torch.sum(torch.square(torch.abs(h - Ht)), dim=(-1, -2)) / torch.sum(torch.square(torch.abs(Ht)), dim=(-1, -2)))
        losses.append(loss.item())
        nmses.append(nmse.item())
        lrs.append(opt.param_groups[0]['lr'])
        opt.zero_grad()
        loss.backward()
        if s == 0:
            grads0 = {k: p.grad.double().numpy().copy() for k, p in holder.named_parameters() if p.grad is not None}
        opt.step()
        sched.step()
    return np.asarray(losses, np.float64), np.asarray(nmses, np.float64), np.asarray(lrs, np.float64), grads0


def main(ref_root):
    torch.set_num_threads(4)
    sd = ldamp.seeded_state_dict(SEED_WEIGHTS, UNROLLS)
    full = ldamp.seeded_state_dict(SEED_WEIGHTS)
    h32, _ = reference_nets(ref_root, full)
    h64, _ = reference_nets(ref_root, full)
    h32, h64 = h32.train(), h64.double().train()
    Y, P, eig, H = O.synthetic_problem(B, NP, 10.0, SEED_DATA)
    dirs = np.random.default_rng(SEED_DIRS).standard_normal((STEPS, UNROLLS, B, 64, 16, 2)).astype(np.float16)
    d32 = dirs.astype(np.float32)
    l32, n32, lrs, _ = train(h32, Y, P, eig, H, d32, torch.float32)
    l64, n64, _, g64 = train(h64, Y, P, eig, H, d32, torch.float64)
    names = sorted(g64)
    assert names == sorted(sd), 'the gradients of step 0 are not those of nets 0 .. %d' % (UNROLLS - 1)
    norms = np.asarray([np.linalg.norm(g64[k]) for k in names])
    dots = np.asarray([np.sum(g64[k] * probe(k, g64[k].shape)) for k in names])
    np.savez_compressed(os.path.join(GOLDEN, 'ldamp_train_step.npz'), seed_weights=SEED_WEIGHTS, seed_probe=SEED_PROBE, unrolls=UNROLLS,
                        Y_herm=Y, P_herm=P, eig1=eig, H_herm_cplx=H, directions=dirs, lrs=lrs, loss32=l32, nmse32=n32, loss64=l64, nmse64=n64,
                        grad_names=np.asarray(names), grad_norm64=norms, grad_dot64=dots)
    print('losses f64', l64, 'f32 - f64', l32 - l64, 'nmse f64', n64, 'lrs', lrs)
    # the restated oracle against these numbers (float64 against float64)
    res = T.step_gradients(sd, Y, P, eig, H, d32[0], UNROLLS, torch.float64)
    worst = max(abs(res['loss'] / l64[0] - 1), abs(res['nmse'] / n64[0] - 1))
    for i, k in enumerate(names):
        g = res['grads'][k]
        worst = max(worst, abs(np.linalg.norm(g) / norms[i] - 1), abs(np.sum(g * probe(k, g.shape)) - dots[i]) / (norms[i] * np.sqrt(g.size)))
    print('oracle float64 vs reference float64: worst relative distance %.3e' % worst)


if __name__ == '__main__':
    main(sys.argv[1])
