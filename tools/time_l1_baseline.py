#!/usr/bin/env python3
"""Timing of the lifted-DFT l1 solver (csrc/cs_l1.hip) at L = 4 and of its numpy float64 oracle (tests/cs_oracle.py).

    python tools/time_l1_baseline.py default     # the reference's default run: 9 SNR x 50 channels = 450 problems x 1000 steps
    python tools/time_l1_baseline.py grid        # a 6 lambda x 4 lr grid of that run: 10 800 problems x 1000 steps
    python tools/time_l1_baseline.py oracle      # the numpy float64 restatement on this host's CPU, per problem

Prints one JSON line per case.  GPU times are CUDA-event times of the one launch (after a small warm-up launch); kernel times for
DESIGN.md come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.  Synthetic CDL-C channels, QPSK pilots,
Np = 38 (alpha = 0.6), lr = 3e-3 in the default run (the grid also holds diverging step sizes, as the reference's would).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

NT, NR, NP, L, STEPS = 64, 16, 38, 4, 1000
N1, N2 = NT * L, NR * L
# complex MACs of one problem-step (csrc/cs_l1.hip): x Rd, Ld T, G Hz, Ld^H E, U Rd^H; 8 real FLOP per complex MAC
CMAC_PER_STEP = N1 * N2 * NR + NT * N1 * NR + NT * NT * NR + N1 * NT * NR + N1 * NR * N2
FLOP_PER_PROBLEM_STEP = 8 * CMAC_PER_STEP                     # 8 912 896 = 8.91 MFLOP at L = 4
FP32_MATRIX_PEAK_TF = 157.3                                   # MI355X, v_mfma_f32_16x16x4_f32


def problems(n_ch, snr_db, seed=3):
    from score_based_channels_amd import synth
    raw = synth.generate_channels('CDL-C', n_ch, NT, NR, 0.5, seed)
    H = np.conj(np.transpose(raw / np.std(raw), (0, 2, 1))).astype(np.complex64)
    rng = np.random.default_rng(seed)
    P = np.conj(np.transpose(synth.qpsk_pilots(rng, n_ch, NT, NP), (0, 2, 1))).astype(np.complex64)
    B = len(snr_db) * n_ch
    idx = np.tile(np.arange(n_ch), len(snr_db))
    noise = np.repeat(10 ** (-np.asarray(snr_db, np.float64) / 10.) * NR, n_ch)
    z = (rng.standard_normal((B, NP, NR)) + 1j * rng.standard_normal((B, NP, NR))) / np.sqrt(2)
    Y = (P[idx] @ H[idx] + np.sqrt(noise)[:, None, None] * z).astype(np.complex64)
    return P, Y, H, idx


def gpu_case(name, lams, lrs):
    import torch
    from score_based_channels_amd.baselines import l1_lifted
    P, Y1, H, idx1 = problems(50, np.arange(-10, 35, 5))
    cells = [(a, b) for a in lams for b in lrs]
    Y = torch.from_numpy(np.concatenate([Y1] * len(cells))).cuda()
    idx = np.tile(idx1, len(cells))
    lam = np.repeat([c[0] for c in cells], len(idx1))
    lr = np.repeat([c[1] for c in cells], len(idx1))
    Pd, Hd = torch.from_numpy(P).cuda(), torch.from_numpy(H).cuda()
    l1_lifted(Pd, Y[:8], Hd, lam[:8], lr[:8], lifting=L, steps=10, p_index=idx[:8], h_index=idx[:8])   # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    log, _ = l1_lifted(Pd, Y, Hd, lam, lr, lifting=L, steps=STEPS, p_index=idx, h_index=idx)
    e1.record()
    torch.cuda.synchronize()
    s = e0.elapsed_time(e1) / 1e3
    B = Y.shape[0]
    tf = B * STEPS * FLOP_PER_PROBLEM_STEP / s / 1e12
    print(json.dumps({'case': name, 'problems': B, 'steps': STEPS, 'lifting': L, 'launch_s': round(s, 4),
                      'flop_per_problem_step': FLOP_PER_PROBLEM_STEP, 'tflops': round(tf, 2),
                      'share_of_fp32_matrix_peak': round(tf / FP32_MATRIX_PEAK_TF, 4),
                      'final_mean_nmse_db': round(float(10 * np.log10(np.nanmean(log[-1].cpu().numpy()))), 3)}), flush=True)


def oracle_case(n):
    import cs_oracle as O
    P, Y, H, idx = problems(n, [10.0])
    t = time.perf_counter()
    O.l1_run(P[idx], Y, H[idx], 0.3, 3e-3, L, STEPS)
    s = time.perf_counter() - t
    cores = len(os.sched_getaffinity(0))
    print(json.dumps({'case': 'oracle_fp64_numpy', 'problems_per_call': n, 'steps': STEPS, 'lifting': L, 's_total': round(s, 3),
                      's_per_problem': round(s / n, 4), 'cpu_cores_available': cores,
                      'omp_num_threads': os.environ.get('OMP_NUM_THREADS'),
                      'grid_10800_problems_est_s': round(10800 * s / n, 1)}), flush=True)


if __name__ == '__main__':
    for what in sys.argv[1:] or ['default']:
        if what == 'default':
            gpu_case('reference_default_450', [0.3], [3e-3])
        elif what == 'grid':
            gpu_case('grid_6x4_10800', [0.0, 0.03, 0.1, 0.3, 1.0, 3.0], [3e-4, 1e-3, 3e-3, 1e-2])
        elif what == 'oracle':
            oracle_case(1)
            oracle_case(8)
        else:
            raise SystemExit('unknown case %r' % what)
