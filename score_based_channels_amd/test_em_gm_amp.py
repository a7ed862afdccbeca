"""EM-GM-AMP channel estimation: the EM-GM-AMP baseline of Fig. 5c.

Counterpart of the reference ``matlab/test_em_gm_amp.m``: for each of the four CDL profiles the scale factor of the seed-1234 file
(:11-18), the first subcarrier of the seed-4321 channels, conjugate-transposed and scaled (:21-34), the first ``--num_samples``
channels and pilot matrices of ``measurementP_seed4321.mat`` (:41-48), ``floor(alpha * rows)`` pilots (:80-81), per SNR point of
``-30:2.5:15`` one noisy measurement per sample (:85-113), EM-GM-AMP with ``maxEMiter = 200``, ``maxTol = 1e-1``, ``nit = 10``
(:55-67), and the three logs of :123-138 -- ``complete_log`` (NMSE after every EM iteration, the sentinel 1000 behind an early
stop), ``oracle_log`` (final NMSE), ``best_log`` (least NMSE over the rows that ran) -- saved per profile as
``<result_dir>/<profile>_nit<nit>.pt`` (the script's file name with this project's container).

THE LIMIT.  The script only *calls* ``EMGMAMP(...)`` from a MATLAB toolbox that is not in the reference's tree.  The toolbox's source
is not available, so its internals -- adaptive step sizes, the order of its EM updates, its initialisation -- are not reproduced and
cannot be compared against.  Reproduced is the script: operator, noise model, schedule, configuration names, logs, result file.  The
algorithm is the one defined in include/sbc_hip.h (``sbc_em_gm_amp_run``), restated from the published method (Bernoulli
Gaussian-mixture GAMP with an EM-learned prior and noise variance); its yardstick is the float64 numpy restatement tests/gamp_oracle.py.

MATLAB solves the 7600 problems one at a time; here every SNR point and sample of a profile is ONE batched launch
(baselines.em_gm_amp).  The script's Kronecker self-check (:104-109) is a host-side assertion on the first sample.  Noise: numpy's
global stream in the script's order -- per SNR point, per sample, the real block then the imaginary block (``--noise host``) -- or
torch's device generator (``--noise device``); MATLAB's own stream is not reproduced by either.  Additions are marked ``[added]``.
"""
import argparse
import os

import numpy as np

from . import synth
from .loaders import read_output_h

TARGET_CHANNELS = ('CDL-A', 'CDL-B', 'CDL-C', 'CDL-D')                     # :4
SNR_RANGE = np.arange(-30, 15 + 1e-9, 2.5)                                 # :52
ALPHA_RANGE, NUM_SAMPLES = [0.6], 100                                      # :51, :46
MAX_EM_ITER, MAX_TOL, NIT = 200, 1e-1, 10                                  # :58, :59, :67
SENTINEL = 1000.0                                                          # :71
TRAIN_SEED, TEST_SEED = 1234, 4321


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--channels', nargs='+', type=str, default=list(TARGET_CHANNELS), help='[added] profiles to run (:4)')
    p.add_argument('--gpu', type=int, default=0, help='[added] HIP device')
    p.add_argument('--synthetic', action='store_true', help='[added] generated CDL-like channels and QPSK pilots instead of ./data')
    p.add_argument('--seed', type=int, default=None, help='[added] seed of the noise stream (default: not seeded, as the script; device draws then use 0)')
    p.add_argument('--num_samples', type=int, default=NUM_SAMPLES, help='[added] samples per SNR point (:46)')
    p.add_argument('--snr_range', nargs='+', type=float, default=SNR_RANGE, help='[added] SNR points in dB (:52)')
    p.add_argument('--alpha', nargs='+', type=float, default=list(ALPHA_RANGE), help='[added] pilot fractions (:51)')
    p.add_argument('--nit', type=int, default=NIT, help='[added] GAMP iterations per EM iteration (optGAMP.nit, :67)')
    p.add_argument('--em_iters', type=int, default=MAX_EM_ITER, help='[added] EM iterations (optEM.maxEMiter, :58)')
    p.add_argument('--tol', type=float, default=MAX_TOL, help='[added] stopping tolerance (optEM.maxTol, :59); 0: never stop')
    p.add_argument('--theta', type=float, default=0.3, help='[added] GAMP damping')
    p.add_argument('--noise', type=str, default='host', choices=['host', 'device'],
                   help='[added] measurement noise from numpy\'s global stream or from torch\'s device generator')
    p.add_argument('--result_dir', type=str, default='./emgmAMP_results_aug7', help='[added] where the result files go (:155)')
    p.add_argument('--data_dir', type=str, default='./data', help='[added] where the .mat files are')
    return p.parse_args(argv)


def data_file(data_dir, profile, seed):
    """:11-15, :21-25 (the CDL-D files carry one decimal of the spacing)"""
    spacing = '0.5' if profile == 'CDL-D' else '0.50'
    return os.path.join(data_dir, '%s_Nt64_Nr16_ULA%s_seed%d.mat' % (profile, spacing, seed))


def result_file(result_dir, profile, nit):
    """:155"""
    return os.path.join(result_dir, '%s_nit%d.pt' % (profile, nit))


def load_profile(profile, num_samples, synthetic, data_dir):
    """:10-48 -> (val_H [num, Nt, Nr] complex128, val_P [num, rows, Nt] complex128)"""
    if synthetic:
        train = synth.generate_output_h(profile, 200, 64, 16, 0.5, TRAIN_SEED, n_sym=1)
        test = synth.generate_output_h(profile, max(200, num_samples), 64, 16, 0.5, TEST_SEED, n_sym=1)
        val_P = synth.qpsk_pilots(np.random.default_rng(TEST_SEED), max(200, num_samples), 64, 64)
    else:
        train = read_output_h(data_file(data_dir, profile, TRAIN_SEED))
        test = read_output_h(data_file(data_dir, profile, TEST_SEED))
        from .mat73 import loadmat_variable
        val_P = loadmat_variable(os.path.join(data_dir, 'measurementP_seed%d.mat' % TEST_SEED), 'val_P')
    scale_factor = np.sqrt(np.mean(np.abs(np.asarray(train, np.complex128)) ** 2))
    val_H = np.asarray(test, np.complex128)[:, 0]                            # first subcarrier of the first symbol
    val_H = np.conj(np.transpose(val_H, (0, 2, 1))) / scale_factor           # conjugate transpose, normalised power
    val_P = np.asarray(val_P, np.complex128)
    if val_H.shape[0] < num_samples or val_P.shape[0] < num_samples:
        raise ValueError('only %d channels and %d pilot matrices, --num_samples is %d' % (val_H.shape[0], val_P.shape[0], num_samples))
    return val_H[:num_samples], val_P[:num_samples]


def kronecker_check(local_A, local_H):
    """:97-109 on one sample: the flattened operator kron(right_idft, A left_idft) applied to fft2(H)(:) gives (A H)(:)."""
    nt, nr = local_H.shape
    kt, kr = np.arange(nt), np.arange(nr)
    left_idft = np.exp(2j * np.pi * np.outer(kt, kt) / nt) / nt
    right_idft = np.exp(2j * np.pi * np.outer(kr, kr) / nr) / nr
    full_A = np.kron(right_idft, local_A @ left_idft)
    flat_Y = full_A @ np.fft.fft2(local_H).flatten('F')
    square_Y = local_A @ local_H
    max_error = np.max(np.abs(square_Y.flatten('F') - flat_Y) ** 2)
    assert max_error <= 1e-8, 'Kronecker flattening incorrect!'
    return max_error


def draw_noise(args, shape, snr_range, device=None):
    """One CN(0, 10^(-snr/10)) block [S, num, Np, Nr] (:85-86, :112-113)."""
    std = np.sqrt(10.0 ** (-np.asarray(snr_range, np.float64) / 10.0) / 2)
    if args.noise == 'host':
        S, num = shape[:2]
        out = np.empty(shape, np.complex128)
        for si in range(S):
            for n in range(num):
                re = np.random.normal(size=shape[2:])
                out[si, n] = std[si] * (re + 1j * np.random.normal(size=shape[2:]))
        return out
    import torch
    gen = torch.Generator(device=device)
    gen.manual_seed(int(args.seed or 0))
    z = torch.randn(tuple(shape) + (2,), generator=gen, device=device, dtype=torch.float32).cpu().numpy().astype(np.float64)
    return std[:, None, None, None] * (z[..., 0] + 1j * z[..., 1])


def solve(P, Y, H, index, args, device):
    """One batched launch -> (log [em_iters, B] float64, stop_iter [B]).  The only place of this script that computes on the GPU."""
    import torch
    from .baselines import em_gm_amp
    with torch.cuda.device(device):
        log, _, stop = em_gm_amp(torch.from_numpy(P).to(device), torch.from_numpy(Y).to(device), torch.from_numpy(H).to(device),
                                 nit=args.nit, em_iters=args.em_iters, tol=args.tol, theta=args.theta, p_index=index, h_index=index)
        return log.cpu().numpy().astype(np.float64), stop.cpu().numpy()


def main(argv=None, solve_fn=None):
    args = parse_args(argv)
    import torch
    from .baselines import check_em_gm_amp_args
    snr_range = np.asarray(args.snr_range, dtype=np.float64)
    alpha_range = np.asarray(args.alpha, dtype=np.float64)
    num, S = int(args.num_samples), len(snr_range)
    device = None
    if solve_fn is None:
        if not torch.cuda.is_available():
            raise RuntimeError('test_em_gm_amp needs a HIP device (there is no CPU fallback)')
        device = torch.device('cuda', min(args.gpu, torch.cuda.device_count() - 1))
        solve_fn = solve
    elif args.noise == 'device':
        raise ValueError('--noise device needs the HIP device')
    if args.seed is not None:
        np.random.seed(args.seed)
    os.makedirs(args.result_dir, exist_ok=True)

    results = {}
    for profile in args.channels:
        val_H, val_P = load_profile(profile, num, args.synthetic, args.data_dir)
        oracle_log = np.zeros((len(alpha_range), S, num))
        complete_log = SENTINEL * np.ones((len(alpha_range), S, args.em_iters, num))
        best_log = np.zeros((len(alpha_range), S, num))
        for ai, alpha in enumerate(alpha_range):
            num_pilots = int(np.floor(val_P.shape[1] * alpha))
            local_P = val_P[:, :num_pilots]
            check_em_gm_amp_args(local_P.shape, (S * num, num_pilots, val_H.shape[2]), val_H.shape, args.nit, args.em_iters, args.tol,
                                 args.theta)
            kronecker_check(local_P[0], val_H[0])
            square_Y = np.matmul(local_P, val_H)                                                 # [num, Np, Nr]
            noisy_Y = square_Y[None] + draw_noise(args, (S,) + square_Y.shape, snr_range, device)
            index = np.tile(np.arange(num), S)                                                   # problem = (snr, sample)
            log, stop = solve_fn(local_P.astype(np.complex64), noisy_Y.reshape((S * num,) + square_Y.shape[1:]).astype(np.complex64),
                                 val_H.astype(np.complex64), index, args, device)
            log = np.asarray(log, np.float64).reshape(args.em_iters, S, num)
            stop = np.asarray(stop).reshape(S, num)
            complete_log[ai] = np.transpose(log, (1, 0, 2))
            ran = np.arange(args.em_iters)[None, :, None] < stop[:, None, :]                     # [S, em_iters, num]
            oracle_log[ai] = np.take_along_axis(complete_log[ai], np.maximum(stop - 1, 0)[:, None, :], axis=1)[:, 0]
            best_log[ai] = np.min(np.where(ran, complete_log[ai], np.inf), axis=1)
            for si, snr in enumerate(snr_range):
                print('%s, alpha = %.2f, SNR = %.2f dB: EM-GM-AMP NMSE = %.2f dB (best %.2f dB), %.1f EM iterations' % (
                    profile, alpha, snr, 10 * np.log10(np.mean(oracle_log[ai, si])), 10 * np.log10(np.mean(best_log[ai, si])),
                    np.mean(stop[si])))
        out = {'complete_log': complete_log, 'oracle_log': oracle_log, 'best_log': best_log, 'snr_range': snr_range,
               'alpha_range': alpha_range, 'args': vars(args)}
        torch.save(out, result_file(args.result_dir, profile, args.nit))
        results[profile] = out
    return results


if __name__ == '__main__':
    main()
