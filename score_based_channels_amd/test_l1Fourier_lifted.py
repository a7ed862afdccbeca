"""Lasso (``--lifting 1``) and fsAD (``--lifting 4``) channel estimation: the compressed-sensing baselines of Fig. 5c.

Counterpart of the reference ``src/score_based_channels/test_l1Fourier_lifted.py``: for every (spacing, alpha, lambda, lr) cell a
fresh validation set, per SNR point one noisy measurement of the kept channels, ``--steps`` iterations of accelerated proximal
gradient on the lifted-DFT l1 problem, the NMSE after every step (``complete_log``) and at the end (``nmse_log``), then the best
(lambda, lr) per (alpha, SNR) by mean NMSE (:191-211).  The reference solves one problem at a time with sigpy on one CPU thread;
here every cell, SNR point and channel of an alpha is ONE batched launch of ``sbc_l1_lifted_run`` (baselines.l1_lifted).

Random draws follow the script's order on numpy's legacy global RNG (seeded once with ``--seed``): the training set's pilots,
then per cell the validation set's pilots, every validation item's loader draws (the script reads the whole set in one
DataLoader batch, :104-111) and the measurement noise per SNR (real block, then imaginary block, :137-140).  All draws are made on
the host first.  Arguments of the reference are kept (:32-42); additions are marked ``[added]`` in ``--help``.
"""
import argparse
import copy
import itertools
import os

import numpy as np

from .config import Config
from .loaders import Channels


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--train', type=str, default='CDL-C')
    p.add_argument('--test', type=str, default='CDL-C')
    p.add_argument('--antennas', nargs='+', type=int, default=[16, 64])
    p.add_argument('--array', type=str, default='ULA')
    p.add_argument('--spacing', type=float, default=0.5)
    p.add_argument('--alpha', nargs='+', type=float, default=[0.6])
    p.add_argument('--lmbda', nargs='+', type=float, default=[0.3])
    p.add_argument('--lifting', type=int, default=4)
    p.add_argument('--steps', type=int, default=1000)
    p.add_argument('--lr', nargs='+', type=float, default=[3e-3])
    # additions of this build
    p.add_argument('--gpu', type=int, default=0, help='[added] HIP device')
    p.add_argument('--seed', type=int, default=None, help='[added] seed of numpy\'s global RNG (default: not seeded, as the reference)')
    p.add_argument('--synthetic', action='store_true', help='[added] generated CDL-like channels instead of ./data')
    p.add_argument('--kept_samples', type=int, default=50, help='[added] validation channels kept (:73)')
    p.add_argument('--no_plot', action='store_true', help='[added] do not write results.png')
    return p.parse_args(argv)


def result_dir(args):
    """:82-83"""
    return './results/l1CS_lifted%d/train-%s_test-%s' % (int(args.lifting), args.train, args.test)


def make_config(args):
    """The minimal configuration of :45-55."""
    config = Config()
    config.data.channel = args.train
    config.data.array = args.array
    config.data.image_size = [args.antennas[0], args.antennas[1]]
    config.data.num_pilots = args.antennas[1]
    config.data.spacing_list = [args.spacing]
    config.data.noise_std = 1
    config.data.mixed_channels = False
    return config


def validation_set(val_seed, val_config, norm, kept, synthetic):
    """:104-122: every item of the validation set is read (one DataLoader batch -- each item's loader draws), then sliced.
    Returns (val_P [kept, Np, Nt], val_H [kept, Nt, Nr]) complex64."""
    ds = Channels(val_seed, val_config, norm=norm, synthetic=synthetic)
    items = [ds[i] for i in range(len(ds))]
    P = np.stack([it['P'] for it in items[:kept]])
    Hh = np.stack([it['H_herm'] for it in items[:kept]])
    return np.conj(np.swapaxes(P, -1, -2)), (Hh[:, 0] + 1j * Hh[:, 1]).astype(np.complex64)


def select_best(nmse_log, alpha_range, snr_range, lmbda_range, lr_range, verbose=True):
    """:191-211: the (lambda, lr) of least mean NMSE per (alpha, SNR)."""
    avg_nmse = np.mean(nmse_log, axis=-1)
    best_nmse = np.zeros((len(alpha_range), len(snr_range)))
    best_lmbda, best_lr = np.zeros_like(best_nmse), np.zeros_like(best_nmse)
    for ai in range(len(alpha_range)):
        for si, snr in enumerate(snr_range):
            local = avg_nmse[0, ai, ..., si].flatten()
            best = np.argmin(local)
            li, ri = np.unravel_index(best, (len(lmbda_range), len(lr_range)))
            best_nmse[ai, si], best_lmbda[ai, si], best_lr[ai, si] = local[best], lmbda_range[li], lr_range[ri]
            if verbose:
                print('SNR = %.2f dB, NMSE = %.2f dB using lambda = %.1e and step size = %.1e' % (
                    snr, 10 * np.log10(best_nmse[ai, si]), best_lmbda[ai, si], best_lr[ai, si]))
    return best_nmse, best_lmbda, best_lr


def main(argv=None):
    args = parse_args(argv)
    import torch
    from .baselines import check_l1_args, l1_lifted

    if not torch.cuda.is_available():
        raise RuntimeError('test_l1Fourier_lifted needs a HIP device (there is no CPU fallback)')
    device = torch.device('cuda', min(args.gpu, torch.cuda.device_count() - 1))
    nr, nt = args.antennas[0], args.antennas[1]
    if args.seed is not None:
        np.random.seed(args.seed)

    config = make_config(args)
    train_seed, val_seed = 1234, 4321
    dataset = Channels(train_seed, config, norm='global', synthetic=args.synthetic)

    snr_range = np.asarray(np.arange(-10, 35, 5))
    spacing_range = np.asarray([args.spacing])
    alpha_range = np.asarray(args.alpha)
    lmbda_range = np.asarray(args.lmbda)
    lr_range = np.asarray(args.lr)
    lifting = int(args.lifting)
    noise_range = 10 ** (-snr_range / 10.) * args.antennas[1]          # Nr / noise power (:67-69)
    gd_iter, kept = int(args.steps), int(args.kept_samples)
    S = len(snr_range)
    shape = (len(spacing_range), len(alpha_range), len(lmbda_range), len(lr_range))
    nmse_log = np.zeros(shape + (S, kept))
    complete_log = np.zeros(shape + (S, gd_iter, kept))
    rdir = result_dir(args)
    os.makedirs(rdir, exist_ok=True)

    # host-side draws of every cell in the script's order, grouped by alpha for one batched solve per alpha
    groups = {}
    for meta_idx, (spacing, alpha, lmbda, lr) in enumerate(itertools.product(spacing_range, alpha_range, lmbda_range, lr_range)):
        si, ai, li, ri = np.unravel_index(meta_idx, shape)
        val_config = copy.deepcopy(config)
        val_config.data.channel = args.test
        val_config.data.spacing_list = [spacing]
        val_config.data.num_pilots = int(np.floor(args.antennas[1] * alpha))
        val_P, val_H = validation_set(val_seed, val_config, [dataset.mean, dataset.std], kept, args.synthetic)
        if val_P.shape[0] != kept:
            raise ValueError('only %d validation channels, --kept_samples is %d' % (val_P.shape[0], kept))
        check_l1_args(val_P.shape, (kept, val_P.shape[1], nr), val_H.shape, lifting, gd_iter)
        Ys = []
        for local_noise in noise_range:
            val_Y = np.matmul(val_P, val_H)
            val_Y = val_Y + np.sqrt(local_noise) / np.sqrt(2.) * (np.random.normal(size=val_Y.shape) +
                                                                  1j * np.random.normal(size=val_Y.shape))
            Ys.append(val_Y)
        groups.setdefault((si, ai), []).append(((li, ri), float(lmbda), float(lr), val_P, val_H, np.stack(Ys)))

    for (si, ai), cells in groups.items():
        n = len(cells)
        P = np.concatenate([c[3] for c in cells]).astype(np.complex64)               # [n * kept, Np, Nt]
        H = np.concatenate([c[4] for c in cells]).astype(np.complex64)               # [n * kept, Nt, Nr]
        Y = np.concatenate([c[5].reshape(S * kept, *c[5].shape[2:]) for c in cells]).astype(np.complex64)   # (cell, snr, sample)
        cell = np.repeat(np.arange(n), S * kept)
        sample = np.tile(np.arange(kept), n * S)
        idx = cell * kept + sample
        lam = np.repeat([c[1] for c in cells], S * kept)
        lrs = np.repeat([c[2] for c in cells], S * kept)
        with torch.cuda.device(device):
            log, _ = l1_lifted(torch.from_numpy(P).to(device), torch.from_numpy(Y).to(device), torch.from_numpy(H).to(device),
                               lam, lrs, lifting=lifting, steps=gd_iter, p_index=idx, h_index=idx)
            log = log.cpu().numpy().reshape(gd_iter, n, S, kept)
        for j, c in enumerate(cells):
            li, ri = c[0]
            complete_log[si, ai, li, ri] = np.transpose(log[:, j], (1, 0, 2))
            nmse_log[si, ai, li, ri] = log[-1, j]

    best_nmse, best_lmbda, best_lr = select_best(nmse_log, alpha_range, snr_range, lmbda_range, lr_range)

    if not args.no_plot:
        import matplotlib
        matplotlib.use('Agg')
        from matplotlib import pyplot as plt
        plt.rcParams['font.size'] = 14
        plt.figure(figsize=(10, 10))
        for ai, local_alpha in enumerate(alpha_range):
            plt.plot(snr_range, 10 * np.log10(best_nmse[ai]), linewidth=4, label='Alpha=%.2f' % local_alpha)
        plt.grid()
        plt.legend()
        plt.title('Compressed Sensing fsAD, lifting = %d' % args.lifting)
        plt.xlabel('SNR [dB]')
        plt.ylabel('NMSE [dB]')
        plt.tight_layout()
        plt.savefig(os.path.join(rdir, 'results.png'), dpi=300, bbox_inches='tight')
        plt.close()

    out = {'complete_log': complete_log, 'nmse_log': nmse_log, 'best_nmse': best_nmse, 'best_lmbda': best_lmbda,
           'best_lr': best_lr, 'snr_range': snr_range, 'spacing_range': spacing_range, 'alpha_range': alpha_range,
           'lmbda_range': lmbda_range, 'lr_range': lr_range, 'config': config, 'args': args}
    torch.save(out, os.path.join(rdir, 'results.pt'))
    return out


if __name__ == '__main__':
    main()
