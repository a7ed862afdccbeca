"""ML channel estimation (regularised least squares): the ML baseline of Fig. 5c.

Counterpart of the reference ``src/score_based_channels/test_ml.py``: per (spacing, alpha) a fresh validation set, per SNR point
(-30 ... 15 dB in 2.5 dB steps) one noisy measurement of the kept channels and the solution of
``(P^H P + s2 I) H = P^H Y`` with s2 = 10^(-SNR/10) (no Nt factor in this script, :67), stored as ``oracle_log`` NMSE (:124-154).
All SNR points and channels of a (spacing, alpha) are ONE batched launch of ``sbc_ls_regularized`` (baselines.ls_regularized).

Deviation: the reference reads its configuration from a hard-coded checkpoint path (:46-50) that is not distributed; here the
configuration is ``config.default_config(--model)`` -- the settings ``train_score`` writes into that checkpoint.  Random draws
follow the script's order on numpy's legacy global RNG (seeded once with ``--seed``): training pilots, then per (spacing, alpha)
the validation pilots, every validation item's loader draws and the noise per SNR (real block, then imaginary block).
Arguments of the reference are kept (:33-38); additions are marked ``[added]`` in ``--help``.
"""
import argparse
import copy
import itertools
import os

import numpy as np

from .config import default_config
from .loaders import Channels
from .test_l1Fourier_lifted import validation_set


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--model', type=str, default='CDL-D')
    p.add_argument('--channel', type=str, default='CDL-D')
    p.add_argument('--antennas', nargs='+', type=int, default=[16, 64])
    p.add_argument('--array', type=str, default='ULA')
    p.add_argument('--spacing', nargs='+', type=float, default=[0.5])
    p.add_argument('--alpha', nargs='+', type=float, default=[0.6])
    # additions of this build
    p.add_argument('--gpu', type=int, default=0, help='[added] HIP device')
    p.add_argument('--seed', type=int, default=None, help='[added] seed of numpy\'s global RNG (default: not seeded, as the reference)')
    p.add_argument('--synthetic', action='store_true', help='[added] generated CDL-like channels instead of ./data')
    p.add_argument('--kept_samples', type=int, default=50, help='[added] validation channels kept (:70)')
    p.add_argument('--no_plot', action='store_true', help='[added] accepted for symmetry with test_l1Fourier_lifted; this script '
                                                            'plots nothing')
    return p.parse_args(argv)


def result_path(args):
    """:75-76, 152-154"""
    return os.path.join('results_ml_baseline/model_%s_channel_%s' % (args.model, args.channel),
                        'results_Nt%d_Nr%d.pt' % (args.antennas[1], args.antennas[0]))


def main(argv=None):
    args = parse_args(argv)
    import torch
    from .baselines import ls_regularized

    if not torch.cuda.is_available():
        raise RuntimeError('test_ml needs a HIP device (there is no CPU fallback)')
    device = torch.device('cuda', min(args.gpu, torch.cuda.device_count() - 1))
    if args.seed is not None:
        np.random.seed(args.seed)

    config = default_config(args.model, image_size=args.antennas)     # instead of the checkpoint's config (:46-50)
    config.sampling.sigma = 0.
    config.data.channel = args.model
    config.data.array = args.array
    config.data.image_size = [args.antennas[0], args.antennas[1]]
    config.data.spacing_list = [args.spacing[0]]
    train_seed, val_seed = 1234, 4321
    dataset = Channels(train_seed, config, norm=config.data.norm_channels, synthetic=args.synthetic)

    snr_range = np.asarray(np.arange(-30, 17.5, 2.5))
    spacing_range = np.asarray(args.spacing)
    alpha_range = np.asarray(args.alpha)
    noise_range = 10 ** (-snr_range / 10.)
    kept, S = int(args.kept_samples), len(snr_range)
    oracle_log = np.zeros((len(spacing_range), len(alpha_range), S, kept))
    path = result_path(args)
    os.makedirs(os.path.dirname(path), exist_ok=True)

    for meta_idx, (spacing, alpha) in enumerate(itertools.product(spacing_range, alpha_range)):
        si, ai = np.unravel_index(meta_idx, (len(spacing_range), len(alpha_range)))
        val_config = copy.deepcopy(config)
        val_config.purpose = 'val'
        val_config.data.channel = args.channel
        val_config.data.spacing_list = [spacing]
        val_config.data.num_pilots = int(np.floor(args.antennas[1] * alpha))
        val_P, val_H = validation_set(val_seed, val_config, [dataset.mean, dataset.std], kept, args.synthetic)
        if val_P.shape[0] != kept:
            raise ValueError('only %d validation channels, --kept_samples is %d' % (val_P.shape[0], kept))
        Ys = []
        for local_noise in noise_range:
            val_Y = np.matmul(val_P, val_H)
            val_Y = val_Y + np.sqrt(local_noise) / np.sqrt(2.) * (np.random.normal(size=val_Y.shape) +
                                                                  1j * np.random.normal(size=val_Y.shape))
            Ys.append(val_Y)
        Y = np.stack(Ys).reshape(S * kept, *Ys[0].shape[1:]).astype(np.complex64)     # problem = snr * kept + sample
        idx = np.tile(np.arange(kept), S)
        with torch.cuda.device(device):
            _, nmse = ls_regularized(torch.from_numpy(val_P.astype(np.complex64)).to(device), torch.from_numpy(Y).to(device),
                                     np.repeat(noise_range, kept), H=torch.from_numpy(val_H).to(device), p_index=idx, h_index=idx)
            oracle_log[si, ai] = nmse.cpu().numpy().reshape(S, kept)
        print('alpha = %.2f: NMSE [dB] per SNR %s' % (alpha, np.round(10 * np.log10(oracle_log[si, ai].mean(-1)), 2)))

    out = {'snr_range': snr_range, 'spacing_range': spacing_range, 'alpha_range': alpha_range, 'oracle_log': oracle_log}
    torch.save(out, path)
    return out


if __name__ == '__main__':
    main()
