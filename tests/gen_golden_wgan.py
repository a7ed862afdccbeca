"""Writes the WGAN fixtures from the REFERENCE's own generator module (run where the reference checkout is; never on the GPU box):

    python tests/gen_golden_wgan.py /path/to/reference

``aux_gan.DCGAN_G_Ours`` is imported by file path, loaded with ``wgan.seeded_state_dict`` and evaluated as ``test_wgan.py:145-165`` does
(generator, measurements, loss, ``backward``), in float32 and in float64.

  tests/golden/wgan_step.npz              B = 4, Np = 38, 10 dB: z, Y, P, H, lambda, scale and the fp32 reference's gen / meas / reg / nmse / g,
                                          the float64 ones as fp32 + residual; and, for lr 0.01, lambda 1, 30 steps, the fp32 reference's
                                          relative distance from float64 in mean meas at step 29 on 1 and on 8 threads
  tests/golden/wgan_state_dict_keys.json  names and shapes of the reference module's state_dict
The script asserts that the fp32 and the float64 reference agree on every ReLU sign of the fixture, so the stored fp32 error is that of
rounding alone (otherwise: change SEED_WEIGHTS -- the signs depend on the weights and on z only, not on the data; seeds 7, 8 and 10 have
one flip each at this z).  Fixtures hold data only; the weights are not stored, only their seed.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import wgan_oracle as O                                          # noqa: E402
from score_based_channels_amd import wgan                        # noqa: E402

SEED_WEIGHTS, SEED_DATA, N_EXTRA = 13, 3, 2
B, NP, SNR_DB = 4, 38, 10.0
LAM = np.array([0.1, 0.3, 1.0, 3.0], np.float32).astype(np.float64)      # float32-representable: both dtypes see the same values
LOOP_LR, LOOP_LAM, LOOP_STEPS = 0.01, 1.0, 30
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def reference_generator(ref_root, sd, dtype):
    spec = importlib.util.spec_from_file_location('ref_aux_gan', os.path.join(ref_root, 'src', 'score_based_channels', 'aux_gan.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = mod.DCGAN_G_Ours([16, 64], 60, 2, 128, 1, N_EXTRA)
    keys = [(k, list(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.eval().to(dtype), keys


def reference_step(net, z, Y, P, H, lam, dtype):
    """test_wgan.py:147-172 with a per-sample lambda; -> dict of numpy arrays and the ReLU signs"""
    signs = []
    hooks = [m.register_forward_hook(lambda _m, inp, _out: signs.append((inp[0] > 0).numpy())) for m in net.conv if isinstance(m, torch.nn.ReLU)]
    latent = torch.tensor(z[:, :, None, None], dtype=dtype, requires_grad=True)
    gen = net(latent)
    for h in hooks:
        h.remove()
    G = gen[:, 0] + 1j * gen[:, 1]
    cd = torch.complex64 if dtype == torch.float32 else torch.complex128
    val_P, val_Y, val_H = (torch.from_numpy(np.asarray(a)).to(cd) for a in (P, Y, H))
    meas = torch.sum(torch.square(torch.abs(torch.matmul(G, val_P) - val_Y)), axis=(-1, -2))
    reg = torch.sum(torch.square(torch.abs(latent)), axis=(-1, -2, -3))
    loss = torch.mean(meas + torch.as_tensor(lam, dtype=dtype) * reg)
    loss.backward()
    nmse = torch.sum(torch.square(torch.abs(G - val_H)), dim=(-1, -2)) / torch.sum(torch.square(torch.abs(val_H)), dim=(-1, -2))
    out = {'gen': gen, 'meas': meas, 'reg': reg, 'nmse': nmse, 'g': latent.grad[:, :, 0, 0]}
    return {k: v.detach().numpy() for k, v in out.items()}, signs


def reference_loop(net, z, Y, P, dtype, threads):
    """test_wgan.py:138-165: Adam on the latents; -> mean meas per step"""
    torch.set_num_threads(threads)
    cd = torch.complex64 if dtype == torch.float32 else torch.complex128
    val_P, val_Y = (torch.from_numpy(np.asarray(a)).to(cd) for a in (P, Y))
    latent = torch.tensor(z[:, :, None, None], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam(params=[latent], lr=LOOP_LR)
    log = []
    for _ in range(LOOP_STEPS):
        gen = net(latent)
        G = gen[:, 0] + 1j * gen[:, 1]
        meas = torch.sum(torch.square(torch.abs(torch.matmul(G, val_P) - val_Y)), axis=(-1, -2))
        reg = torch.sum(torch.square(torch.abs(latent)), axis=(-1, -2, -3))
        loss = torch.mean(meas + LOOP_LAM * reg)
        opt.zero_grad()
        loss.backward()
        opt.step()
        log.append(float(meas.detach().double().mean()))
    return np.asarray(log)


def split64(x64, x32):
    return (np.asarray(x64, np.float64) - np.asarray(x32).astype(np.float64)).astype(np.float32)


def main(ref_root):
    torch.set_num_threads(4)
    sd = wgan.seeded_state_dict(SEED_WEIGHTS, N_EXTRA)
    n32, keys = reference_generator(ref_root, sd, torch.float32)
    n64, _ = reference_generator(ref_root, sd, torch.float64)
    assert keys == [(n, list(s)) for n, s in wgan.state_dict_spec(N_EXTRA)], 'state_dict_spec does not match the reference module'
    with open(os.path.join(GOLDEN, 'wgan_state_dict_keys.json'), 'w') as f:
        json.dump({'n_extra': N_EXTRA, 'keys': keys}, f, indent=0)

    Y, P, H = O.synthetic_problem(B, NP, SNR_DB, SEED_DATA)
    z = O.init_z(B)
    r32, s32 = reference_step(n32, z, Y, P, H, LAM, torch.float32)
    r64, s64 = reference_step(n64, z, Y, P, H, LAM, torch.float64)
    flips = [int(np.sum(a != b)) for a, b in zip(s32, s64)]
    assert sum(flips) == 0, 'the fp32 and float64 reference disagree on ReLU signs (%s): change SEED_WEIGHTS' % flips
    e_ref = {k: O.normwise(r32[k].reshape(B, -1), r64[k].reshape(B, -1)) for k in r32}
    print('e_ref:', {k: '%.2e' % v for k, v in e_ref.items()}, ' var(gen) %.3f' % np.var(r64['gen']))

    m64 = reference_loop(n64, z, Y, P, torch.float64, 4)
    dist = {}
    for threads in (1, 8):
        m32 = reference_loop(n32, z, Y, P, torch.float32, threads)
        dist[threads] = abs(m32[-1] - m64[-1]) / m64[-1]
        print('loop, %d thread(s): mean meas step 0 %.6f -> step %d %.6f, fp32 vs float64 at the last step %.3e'
              % (threads, m64[0], LOOP_STEPS - 1, m64[-1], dist[threads]))

    out = {'seed_weights': SEED_WEIGHTS, 'n_extra': N_EXTRA, 'z': z, 'Y': Y, 'P': P, 'H': H, 'lam': LAM.astype(np.float32),
           'scale': np.full((B,), 1.0 / B, np.float32), 'loop_lr': LOOP_LR, 'loop_lam': LOOP_LAM, 'loop_steps': LOOP_STEPS,
           'loop_meas64': m64, 'loop_dist_1thread': dist[1], 'loop_dist_8threads': dist[8]}
    for k in r32:
        out[k + '32'] = r32[k].astype(np.float32)
        out[k + '64_minus_32'] = split64(r64[k], r32[k])
    np.savez_compressed(os.path.join(GOLDEN, 'wgan_step.npz'), **out)


if __name__ == '__main__':
    main(sys.argv[1])
