#!/usr/bin/env python3
"""Timing of Learned D-AMP (score_based_channels_amd/ldamp.py, csrc/ldamp.hip): a 10-unroll run of B = 100 samples, Np = 38.

    python tools/time_ldamp.py [--out profiles/ldamp_mi355x.txt]

Three measurements, written as text:
  1. the HIP path: one ``LDAMP.__call__`` per repetition, caller-supplied directions, CUDA-event time after warm-up, >= 20 repetitions;
  2. the same loop with stock torch-ROCm operators on the same GPU: the layer list of tests/ldamp_oracle.py on ``cuda`` in float32
     (conv2d, instance_norm, leaky_relu, avg_pool2d, conv_transpose2d, cat; about 70 launches per evaluation), same event timing;
  3. kernel times of the HIP path from a ``rocprofv3 --kernel-trace --stats`` run of its own (a child process: ``--child``).
FLOP count: 2 x MACs of one denoiser evaluation, from the layer shapes (MACS_PER_EVAL below), x 2 evaluations x unrolls x B.
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

# (pixels, cin, cout, taps) of every convolution of one evaluation
LAYERS = [(1024, 2, 16, 9), (1024, 16, 16, 9), (256, 16, 32, 9), (256, 32, 32, 9), (64, 32, 64, 9), (64, 64, 64, 9),
          (16, 64, 128, 9), (16, 128, 128, 9),
          (16, 128, 64, 4), (64, 128, 64, 9), (64, 64, 64, 9),          # transposed conv: input pixels x 4 taps
          (64, 64, 32, 4), (256, 64, 32, 9), (256, 32, 32, 9),
          (256, 32, 16, 4), (1024, 32, 16, 9), (1024, 16, 16, 9), (1024, 16, 2, 1)]
MACS_PER_EVAL = sum(p * ci * co * t for p, ci, co, t in LAYERS)           # 36 110 336 -> 72.2 MFLOP
FP32_VECTOR_PEAK_TF = 157.3                                               # MI355X fp32 FMA (and fp32 MFMA) peak


def setup(B, unrolls):
    import torch
    import ldamp_oracle as O
    from score_based_channels_amd import ldamp
    sd = ldamp.seeded_state_dict(2025)
    Y, P, eig, H = O.synthetic_problem(B, 38, 10.0, 11)
    d = np.random.default_rng(5).standard_normal((unrolls, B, 64, 16, 2)).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    return O, ldamp, sd, to(Y), to(P), to(eig), to(H), to(d)


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


def child(args):
    O, ldamp, sd, Y, P, eig, H, d = setup(args.B, args.unrolls)
    import torch
    model = ldamp.LDAMP({'max_unrolls': 10}).load_state_dict(sd)
    for _ in range(3):
        model({'Y_herm': Y, 'P_herm': P, 'eig1': eig}, args.unrolls, directions=d)
    torch.cuda.synchronize()


def kernel_stats(args):
    """rocprofv3 --kernel-trace --stats of ``--child`` -> lines of (kernel, calls, total us, average us, %)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'ldamp', '--',
               sys.executable, os.path.abspath(__file__), '--child', '--B', str(args.B), '--unrolls', str(args.unrolls)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            return ['rocprofv3 run failed (exit %d): %s' % (r.returncode, r.stdout.decode(errors='replace')[-400:])]
        rows = list(csv.DictReader(open(files[0])))
    out = ['%-100s %8s %12s %10s %7s' % ('kernel (3 runs of the child)', 'calls', 'total us', 'avg us', '%')]
    for row in rows:
        name = row.get('Name', '?')
        name = name if len(name) <= 100 else name[:97] + '...'
        out.append('%-100s %8s %12.1f %10.2f %7s' % (name, row.get('Calls', '?'), float(row.get('TotalDurationNs', 0)) / 1e3,
                                                    float(row.get('AverageNs', 0)) / 1e3, row.get('Percentage', '?')))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--B', type=int, default=100)
    p.add_argument('--unrolls', type=int, default=10)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--out', type=str, default=None)
    p.add_argument('--child', action='store_true')
    p.add_argument('--no_rocprof', action='store_true')
    args = p.parse_args()
    if args.child:
        return child(args)
    import torch
    O, ldamp, sd, Y, P, eig, H, d = setup(args.B, args.unrolls)
    model = ldamp.LDAMP({'max_unrolls': 10}).load_state_dict(sd)
    sample = {'Y_herm': Y, 'P_herm': P, 'eig1': eig}
    hip = event_times(lambda: model(sample, args.unrolls, directions=d), 3, args.reps)
    sd_dev = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    stock_fn = lambda: O.run(lambda u, x: O.denoise_planes(sd_dev, u, x, torch.float32), Y, P, eig, d, args.unrolls, torch.float32, logs=False)  # noqa: E731
    stock = event_times(stock_fn, 3, args.reps)
    h_hip = model(sample, args.unrolls, directions=d).cpu().numpy()
    h_stock = stock_fn().cpu().numpy()
    flop = 2.0 * MACS_PER_EVAL * 2 * args.unrolls * args.B
    lines = ['Learned D-AMP, %d unrolls, B = %d, Np = 38, %s' % (args.unrolls, args.B, torch.cuda.get_device_name(0)),
             'work: %d MACs = %.1f MFLOP per evaluation; %.1f GFLOP per run (2 evaluations x %d unrolls x %d samples)'
             % (MACS_PER_EVAL, 2 * MACS_PER_EVAL / 1e6, flop / 1e9, args.unrolls, args.B),
             'launches per unroll: HIP path 19 (+ 1 copy per run)',
             'HIP path      : median %.3f ms  min %.3f  max %.3f  (%d repetitions, CUDA events)  %.2f TFLOP/s = %.1f %% of the fp32 FMA peak'
             % (np.median(hip), hip.min(), hip.max(), len(hip), flop / np.median(hip) / 1e9, 100 * flop / np.median(hip) / 1e9 / FP32_VECTOR_PEAK_TF),
             'stock torch   : median %.3f ms  min %.3f  max %.3f  (%d repetitions, the oracle\'s layer list on cuda, float32)'
             % (np.median(stock), stock.min(), stock.max(), len(stock)),
             'ratio stock / HIP: %.2f' % (np.median(stock) / np.median(hip)),
             'agreement of the two final h (norm-wise, max over samples): %.2e' % O.normwise(h_hip, h_stock), '']
    if not args.no_rocprof:
        del model
        lines += kernel_stats(args)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
