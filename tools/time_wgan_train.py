#!/usr/bin/env python3
"""Timing of WGAN training (score_based_channels_amd/wgan.py ``Trainer``, csrc/wgan_train.hip): ONE generator iteration with Diters = 5,
i.e. five critic iterations and one generator iteration, at B = 200 (real and fake), n_extra = 1: the steady state of train_wgan.py.

    python tools/time_wgan_train.py [--out profiles/wgan_train_mi355x.txt]

Three measurements, written as text:
  1. the HIP path: 5 x ``critic_step`` + ``generator_step``, CUDA-event time after warm-up, median of ``--reps`` (20) repetitions;
  2. the stock loop on the same GPU: the layer lists of tests/wgan_train_oracle.py on ``cuda`` in float32 (TF32 off), autograd and
     ``torch.optim.RMSprop``, the clamp as ``clamp_`` per parameter (it does not maintain running statistics: that work is left out of it);
  3. kernel times of each path from a ``rocprofv3 --kernel-trace --stats`` run of its own (child processes: ``--child hip`` / ``--child
     stock``), for the HIP path also summed into the groups G convolutions forward / input gradient, G weight gradients, critic
     convolutions, BatchNorm and activations (both networks share those kernels), the rest.
Work: G forward 0.682 G MAC per sample (6 per generator iteration), as much for its input-gradient and for its weight-gradient pass (one
each); D 18.4 M MAC per sample and pass, 11 forward passes, 11 input-gradient and 10 weight-gradient passes.
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

N_EXTRA, DITERS = 1, 5
G_MACS = 60 * 8192 + 256 * 128 * 128 * 25 + 1024 * 128 * 128 * 25 + N_EXTRA * 1024 * 128 * 128 * 9 + 1024 * 128 * 2 * 25
D_MACS = 256 * 2 * 64 * 16 + N_EXTRA * 256 * 64 * 64 * 9 + 64 * 64 * 128 * 16 + 128 * 64
GROUPS = (('G convolutions, forward and input gradient (conv128 raw, dense, out, out adjoint)', ('conv128_kernel', 'dense_kernel', 'out_kernel', 'out_adjoint_kernel')),
          ('G weight gradients (wgrad128 + reduce, dense)', ('wgrad128_kernel', 'wgrad128_reduce_kernel', 'dense_wgrad_kernel')),
          ('critic convolutions on the vector ALUs, all three directions (+ G\'s output-convolution weight gradient, one launch)', ('dconv_fwd_kernel', 'dconv_bwd_kernel', 'dconv_wgrad_kernel', 'final_dot_kernel', 'final_wgrad_kernel')),
          ('BatchNorm statistics, normalise + activation, backward: both networks', ('bn_stats_kernel', 'bn_act_kernel', 'bn_bwd_reduce_kernel', 'bn_bwd_apply_kernel')),
          ('the rest (RMSprop and clamp, repack, bias sums, mean + seed)', ('rmsprop_kernel', 'repack128_kernel', 'chan_sum_kernel', 'mean_seed_kernel')))


def data(B, seed=1):
    import torch
    rng = np.random.default_rng(seed)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()       # noqa: E731
    return to(rng.standard_normal((B, 2, 16, 64))), to(rng.standard_normal((DITERS + 1, B, 60)))


def hip_iteration(tr, real, noise):
    for j in range(DITERS):
        tr.critic_step(real, noise[j])
    return tr.generator_step(noise[DITERS])


def stock_setup():
    import torch
    from score_based_channels_amd import wgan
    gsd, dsd = wgan.init_state_dicts(2020, N_EXTRA)
    nets = []
    for sd in (gsd, dsd):
        net = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in sd.items() if not k.endswith('num_batches_tracked')}
        params = [v.requires_grad_(True) for k, v in net.items() if not k.endswith(('running_mean', 'running_var'))]
        nets.append((net, params, torch.optim.RMSprop(params, lr=5e-5)))
    return nets


def stock_iteration(T, nets, real, noise):
    """train_wgan.py:130-184 on stock operators"""
    import torch
    (G, gp, optG), (D, dp, optD) = nets
    one = torch.ones(1, device='cuda')
    for j in range(DITERS):
        for p in dp:
            p.data.clamp_(-0.01, 0.01)
        optD.zero_grad()
        T.d_forward(D, real, torch.float32)['err'].backward(one)
        with torch.no_grad():
            fake = T.g_forward(G, noise[j], torch.float32)['gen']
        T.d_forward(D, fake, torch.float32)['err'].backward(-one)
        optD.step()
    for p in dp:
        p.requires_grad_(False)
    optG.zero_grad()
    err = T.d_forward(D, T.g_forward(G, noise[DITERS], torch.float32)['gen'], torch.float32)['err']
    err.backward(one)
    optG.step()
    for p in dp:
        p.requires_grad_(True)
    return err.detach()


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


def make_trainer(B):
    from score_based_channels_amd import wgan
    return wgan.Trainer(*wgan.init_state_dicts(2020, N_EXTRA), batch_size=B)


def child(args):
    import torch
    import wgan_train_oracle as T
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    real, noise = data(args.B)
    if args.child == 'stock':
        nets = stock_setup()
        for _ in range(2):
            stock_iteration(T, nets, real, noise)
    else:
        tr = make_trainer(args.B)
        for _ in range(2):
            hip_iteration(tr, real, noise)
    torch.cuda.synchronize()


def kernel_stats(args, which):
    """rocprofv3 --kernel-trace --stats of ``--child hip`` or ``--child stock`` (two iterations each) -> text lines"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'wgan_train', '--',
               sys.executable, os.path.abspath(__file__), '--child', which, '--B', str(args.B)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            return ['rocprofv3 run failed (exit %d): %s' % (r.returncode, r.stdout.decode(errors='replace')[-400:])]
        with open(files[0]) as f:
            rows = list(csv.DictReader(f))
    what = 'HIP path' if which == 'hip' else 'stock torch loop, the first 24 kernels by time (its first iteration includes the library\'s one-off work)'
    total = sum(float(r.get('TotalDurationNs', 0)) for r in rows) / 2e6
    out = ['%s: %.2f ms of kernel time per generator iteration (2 iterations traced, no warm-up, B = %d)' % (what, total, args.B),
           '%-110s %8s %12s %10s %7s' % ('kernel', 'calls', 'total us', 'avg us', '%')]
    for row in rows[:24]:
        name = row.get('Name', '?')
        name = name if len(name) <= 110 else name[:107] + '...'
        out.append('%-110s %8s %12.1f %10.2f %7s' % (name, row.get('Calls', '?'), float(row.get('TotalDurationNs', 0)) / 1e3,
                                                    float(row.get('AverageNs', 0)) / 1e3, row.get('Percentage', '?')))
    if which == 'hip':
        out += ['', 'HIP path by group, ms per generator iteration:']
        for title, names in GROUPS:
            ms = sum(float(r.get('TotalDurationNs', 0)) for r in rows if any(n in r.get('Name', '') for n in names)) / 2e6
            out.append('  %8.3f  %s' % (ms, title))
        conv = sum(float(r.get('TotalDurationNs', 0)) for r in rows if 'conv128_kernel' in r.get('Name', '')) / 2e6
        out.append('  (conv128 raw: %.3f ms in 7 passes of the same launches, 6 forward = %.3f ms and 1 input gradient = %.3f ms by launch count)'
                   % (conv, conv * 6 / 7, conv / 7))
    return out + ['']


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--B', type=int, default=200)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--out', type=str, default=None)
    p.add_argument('--child', type=str, default=None, choices=['hip', 'stock'])
    p.add_argument('--no_rocprof', action='store_true')
    args = p.parse_args()
    if args.child:
        return child(args)
    import torch
    import wgan_train_oracle as T
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    B = args.B
    real, noise = data(B)
    tr = make_trainer(B)
    hip = event_times(lambda: hip_iteration(tr, real, noise), 3, args.reps)
    e_hip = float(hip_iteration(tr, real, noise).cpu()[0])
    del tr
    torch.cuda.empty_cache()
    nets = stock_setup()
    stock = event_times(lambda: stock_iteration(T, nets, real, noise), 3, args.reps)
    e_stock = float(stock_iteration(T, nets, real, noise).cpu()[0])
    g_flop = 2.0 * G_MACS * B * (DITERS + 1 + 2)
    d_flop = 2.0 * D_MACS * B * ((2 * DITERS + 1) * 2 + 2 * DITERS)
    lines = ['WGAN training, one generator iteration = %d critic iterations + 1 generator iteration, B = %d real and fake, n_extra = %d, %s'
             % (DITERS, B, N_EXTRA, torch.cuda.get_device_name(0)),
             'work: G %.3f G MAC per sample and pass x 8 passes = %.1f GFLOP; D %.1f M MAC per sample and pass x 32 passes = %.1f GFLOP'
             % (G_MACS / 1e9, g_flop / 1e9, D_MACS / 1e6, d_flop / 1e9), '',
             '  HIP path    : median %.3f ms  min %.3f  max %.3f  (%d repetitions after 3 warm-up iterations, CUDA events)  %.1f TFLOP/s on G\'s work alone'
             % (np.median(hip), hip.min(), hip.max(), len(hip), g_flop / np.median(hip) / 1e9),
             '  stock torch : median %.3f ms  min %.3f  max %.3f  (the oracle\'s layer lists on cuda, float32, TF32 off, autograd + torch.optim.RMSprop; no running statistics)'
             % (np.median(stock), stock.min(), stock.max()),
             '  ratio stock / HIP: %.2f' % (np.median(stock) / np.median(hip)),
             '  errG after %d iterations of each loop (they part ways: RMSprop steps are +-10 lr whatever the gradient): HIP %.6g, stock %.6g' % (args.reps + 4, e_hip, e_stock), '']
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
