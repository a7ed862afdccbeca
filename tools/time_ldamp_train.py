#!/usr/bin/env python3
"""Timing of one L-DAMP training step (ldamp.Trainer, csrc/ldamp_train.hip): B = 128, Np = 38, 10 unrolls.

    python tools/time_ldamp_train.py [--out profiles/ldamp_train_mi355x.txt]      the two event timings
    python tools/time_ldamp_train.py --stats [--out FILE]                         kernel times only (rocprofv3, a run of its own)

  1. the HIP path: one ``Trainer.step`` (forward, loss, backward, Adam) per repetition, caller-supplied directions, CUDA-event time
     around the launches after warm-up;
  2. the same step from stock torch-ROCm operators on the same GPU: the layer list of tests/ldamp_train_oracle.py on ``cuda`` in float32
     with autograd and ``torch.optim.Adam``;
  3. ``--stats``: kernel times of the HIP path from ``rocprofv3 --kernel-trace --stats`` of a child process (``--child``), appended to --out.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), HERE]
from time_ldamp import MACS_PER_EVAL, event_times                # noqa: E402


def setup(B, unrolls):
    import torch
    import ldamp_oracle as O
    from score_based_channels_amd import ldamp
    sd = ldamp.seeded_state_dict(2025, unrolls)
    Y, P, eig, H = O.synthetic_problem(B, 38, 10.0, 11)
    d = np.random.default_rng(5).standard_normal((unrolls, B, 64, 16, 2)).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    sample = {'Y_herm': to(Y), 'P_herm': to(P), 'eig1': to(eig), 'H_herm_cplx': to(H)}
    return ldamp, sd, sample, to(d)


def child(args):
    import torch
    ldamp, sd, sample, d = setup(args.B, args.unrolls)
    tr = ldamp.Trainer({'max_unrolls': args.unrolls}, sd, capacity=args.B)
    for _ in range(3):
        tr.step(sample, args.unrolls, directions=d)
    torch.cuda.synchronize()


def kernel_stats(args):
    import csv
    import glob
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'ldamp_train', '--',
               sys.executable, os.path.abspath(__file__), '--child', '--B', str(args.B), '--unrolls', str(args.unrolls)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            return ['rocprofv3 run failed (exit %d): %s' % (r.returncode, r.stdout.decode(errors='replace')[-400:])]
        rows = list(csv.DictReader(open(files[0])))
    out = ['', '%-100s %8s %12s %10s %7s' % ('kernel (3 steps of the child)', 'calls', 'total us', 'avg us', '%')]
    for row in rows[:24]:
        name = row.get('Name', '?')
        name = name if len(name) <= 100 else name[:97] + '...'
        out.append('%-100s %8s %12.1f %10.2f %7s' % (name, row.get('Calls', '?'), float(row.get('TotalDurationNs', 0)) / 1e3,
                                                    float(row.get('AverageNs', 0)) / 1e3, row.get('Percentage', '?')))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--B', type=int, default=128)
    p.add_argument('--unrolls', type=int, default=10)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--out', type=str, default=None)
    p.add_argument('--child', action='store_true')
    p.add_argument('--stats', action='store_true')
    args = p.parse_args()
    if args.child:
        return child(args)
    if args.stats:
        lines = kernel_stats(args)
    else:
        import torch
        import ldamp_train_oracle as T
        ldamp, sd, sample, d = setup(args.B, args.unrolls)
        tr = ldamp.Trainer({'max_unrolls': args.unrolls}, sd, capacity=args.B)
        hip = event_times(lambda: tr.step(sample, args.unrolls, directions=d), 2, args.reps)
        loss_hip = tr.step(sample, args.unrolls, directions=d, update=False)[0]
        state = tr.state_dict()
        del tr
        params = {k: torch.nn.Parameter(torch.from_numpy(v).cuda()) for k, v in sd.items()}
        opt = torch.optim.Adam(list(params.values()), 1e-3)

        def stock():
            h = T.forward(params, sample['Y_herm'], sample['P_herm'], sample['eig1'], d, args.unrolls, torch.float32)
            loss, _ = T.loss_nmse(h, sample['H_herm_cplx'])
            opt.zero_grad()
            loss.backward()
            opt.step()
            return float(loss.detach())
        st = event_times(stock, 2, args.reps)
        loss_stock = stock()                              # (after the same number of updates as the HIP path's gradient-only step)
        drift = max(float(np.max(np.abs(state[k] - params[k].detach().cpu().numpy()))) for k in sd)
        flop = 2.0 * MACS_PER_EVAL * (2 + 2) * args.unrolls * args.B       # 2 forward evaluations + a backward of twice one evaluation
        lines = ['L-DAMP training step, %d unrolls, B = %d, Np = 38, %s' % (args.unrolls, args.B, torch.cuda.get_device_name(0)),
                 'work: about %.1f GFLOP per step (2 forward evaluations + input and weight gradients of the clean one, x %d unrolls x %d samples)'
                 % (flop / 1e9, args.unrolls, args.B),
                 'HIP path      : median %.3f ms  min %.3f  max %.3f  (%d repetitions, CUDA events, Trainer.step with its host wait)  %.2f TFLOP/s'
                 % (np.median(hip), hip.min(), hip.max(), len(hip), flop / np.median(hip) / 1e9),
                 'stock torch   : median %.3f ms  min %.3f  max %.3f  (%d repetitions, the oracle\'s layer list on cuda with autograd and Adam, float32)'
                 % (np.median(st), st.min(), st.max(), len(st)),
                 'ratio stock / HIP: %.2f' % (np.median(st) / np.median(hip)),
                 'loss after %d updates: HIP %.4f, stock %.4f; largest parameter difference %.2e' % (args.reps + 2, loss_hip, loss_stock, drift)]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'a' if args.stats else 'w').write(text)


if __name__ == '__main__':
    main()
