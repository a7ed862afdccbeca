#!/usr/bin/env python3
"""Timing of the WGAN latent optimisation (score_based_channels_amd/wgan.py, csrc/wgan.hip): one Adam step on the latents, Np = 38,
2 extra layers, at B = 1100 (one pilot fraction's default 11 SNR points x 1 cell x 100 samples) and at B = 100.

    python tools/time_wgan.py [--out profiles/wgan_mi355x.txt]

Three measurements, written as text:
  1. the HIP path: ``LatentOptimizer.run`` of ``--steps`` steps per repetition, CUDA-event time per step after warm-up, >= 20 repetitions;
  2. the same loop with stock torch-ROCm operators and autograd on the same GPU: the layer list of tests/wgan_oracle.py on ``cuda`` in
     float32 (TF32 off), torch.optim.Adam on the latents, same event timing;
  3. kernel times of the HIP path and of the stock loop, each from a ``rocprofv3 --kernel-trace --stats`` run of its own (child
     processes: ``--child hip`` / ``--child stock``).
FLOP count: 2 x MACs of the generator (dense, the 128 -> 128 convolutions, the output convolution), forward and once more backward.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_EXTRA = 2
# (pixels, cin, cout, taps): dense, conv1, conv2, extras, conv_out
LAYERS = [(1, 60, 8192, 1), (256, 128, 128, 25), (1024, 128, 128, 25)] + [(1024, 128, 128, 9)] * N_EXTRA + [(1024, 128, 2, 25)]
MACS_FORWARD = sum(p * ci * co * t for p, ci, co, t in LAYERS)            # 0.83 G MAC
FP32_MATRIX_PEAK_TF = 157.3                                               # MI355X fp32 MFMA (and fp32 FMA) peak


def setup(B):
    import torch
    import wgan_oracle as O
    from score_based_channels_amd import wgan
    sd = wgan.seeded_state_dict(13, N_EXTRA)
    Y, P, H = O.synthetic_problem(4, 38, 10.0, 3)
    rep = lambda a: np.tile(a, (B // 4 + 1,) + (1,) * (a.ndim - 1))[:B]    # noqa: E731
    z = np.random.RandomState(2021).normal(size=(B, 60)).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    return O, wgan, sd, to(z), to(rep(Y)), to(rep(P)), to(rep(H))


def event_times(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.asarray(ms)


def stock_loop(O, sd_dev, z0, Y, P, steps, lr=0.01, lam=1.0):
    """test_wgan.py:140-165 on stock operators: the oracle's layer list, autograd, torch.optim.Adam"""
    import torch
    latent = z0.clone().requires_grad_(True)
    opt = torch.optim.Adam(params=[latent], lr=lr)
    Yc, Pc = Y, P
    meas = None
    for _ in range(steps):
        gen, _, _ = O.generate(sd_dev, latent, torch.float32)
        G = torch.complex(gen[:, 0], gen[:, 1])
        meas = torch.sum(torch.square(torch.abs(torch.matmul(G, Pc) - Yc)), dim=(-1, -2))
        reg = torch.sum(torch.square(latent), dim=-1)
        loss = torch.mean(meas + lam * reg)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return meas.detach()


def child(args):
    O, wgan, sd, z, Y, P, H = setup(args.B)
    import torch
    if args.child == 'stock':
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False
        sd_dev = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in sd.items()}
        stock_loop(O, sd_dev, z, Y, P, args.steps)
        torch.cuda.synchronize()
        return
    opt = wgan.LatentOptimizer(wgan.DCGAN_G_Ours([16, 64], 60, 2, 128, 1, N_EXTRA).load_state_dict(sd))
    opt.run(z, Y, P, 0.01, 1.0, args.steps, H=H)
    torch.cuda.synchronize()


def kernel_stats(args, which):
    """rocprofv3 --kernel-trace --stats of ``--child hip`` or ``--child stock`` -> lines of (kernel, calls, total us, average us, %)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'wgan', '--',
               sys.executable, os.path.abspath(__file__), '--child', which, '--B', str(args.B), '--steps', str(args.steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            return ['rocprofv3 run failed (exit %d): %s' % (r.returncode, r.stdout.decode(errors='replace')[-400:])]
        with open(files[0]) as f:
            rows = list(csv.DictReader(f))
    what = 'HIP path' if which == 'hip' else 'stock torch loop, the first 24 kernels by time (its first steps include the library\'s one-off work)'
    out = ['%-110s %8s %12s %10s %7s' % ('kernel (%s; %d steps, B = %d)' % (what, args.steps, args.B), 'calls', 'total us', 'avg us', '%')]
    for row in rows[:24]:
        name = row.get('Name', '?')
        name = name if len(name) <= 110 else name[:107] + '...'
        out.append('%-110s %8s %12.1f %10.2f %7s' % (name, row.get('Calls', '?'), float(row.get('TotalDurationNs', 0)) / 1e3,
                                                    float(row.get('AverageNs', 0)) / 1e3, row.get('Percentage', '?')))
    return out + ['']


def measure(args, B):
    import torch
    O, wgan, sd, z, Y, P, H = setup(B)
    opt = wgan.LatentOptimizer(wgan.DCGAN_G_Ours([16, 64], 60, 2, 128, 1, N_EXTRA).load_state_dict(sd))
    steps = args.steps
    hip = event_times(lambda: opt.run(z, Y, P, 0.01, 1.0, steps, H=H), 2, args.reps) / steps
    sd_dev = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in sd.items()}
    stock = event_times(lambda: stock_loop(O, sd_dev, z, Y, P, steps), 2, args.reps) / steps
    m_hip = opt.run(z, Y, P, 0.01, 1.0, steps, H=H)[2]['meas'][-1].cpu().numpy()
    m_stock = stock_loop(O, sd_dev, z, Y, P, steps).cpu().numpy()
    flop = 2.0 * MACS_FORWARD * 2 * B
    tf = flop / np.median(hip) / 1e9
    return ['B = %d: %.2f GFLOP per step (%.3f G MAC forward per sample, as much again backward)' % (B, flop / 1e9, MACS_FORWARD / 1e9),
            '  HIP path    : median %.3f ms per step  min %.3f  max %.3f  (%d repetitions of %d steps, CUDA events)  %.1f TFLOP/s = %.1f %% of the fp32 matrix peak'
            % (np.median(hip), hip.min(), hip.max(), len(hip), steps, tf, 100 * tf / FP32_MATRIX_PEAK_TF),
            '  stock torch : median %.3f ms per step  min %.3f  max %.3f  (the oracle\'s layer list on cuda, float32, TF32 off, autograd + torch.optim.Adam)'
            % (np.median(stock), stock.min(), stock.max()),
            '  ratio stock / HIP: %.2f' % (np.median(stock) / np.median(hip)),
            '  mean meas at the last of the %d steps: HIP %.6g, stock %.6g' % (steps, m_hip.mean(), m_stock.mean()), '']


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--B', type=int, default=1100)
    p.add_argument('--steps', type=int, default=2)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--out', type=str, default=None)
    p.add_argument('--child', type=str, default=None, choices=['hip', 'stock'])
    p.add_argument('--no_rocprof', action='store_true')
    args = p.parse_args()
    if args.child:
        return child(args)
    import torch
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    lines = ['WGAN latent optimisation, one step, Np = 38, %d extra layers, %s' % (N_EXTRA, torch.cuda.get_device_name(0)),
             'launches per step: HIP path %d' % (2 * (2 + N_EXTRA) + 4), '']
    for B in (args.B, 100):
        lines += measure(args, B)
    if not args.no_rocprof:
        lines += kernel_stats(args, 'hip') + kernel_stats(args, 'stock')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
