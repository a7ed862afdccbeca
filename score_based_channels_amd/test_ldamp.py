"""Learned D-AMP channel estimation: the L-DAMP baseline of Fig. 5c.

Counterpart of the reference ``src/score_based_channels/test_ldamp.py``: per SNR point one checkpoint
``./models/ldamp-FlippedUNet/train-<train>/model_snr%.2f_alpha%.2f.pt`` (keys ``model_state``, ``config``), a validation set of seed 4321
with the loader's own noise at ``noise_std = 10^(-snr/20) sqrt(Nt)`` (:83, drawn inside ``__getitem__`` from numpy's global stream),
``config.model.max_unrolls`` unrolls of ``ldamp.LDAMP`` on one batch of ``--num_channels`` samples, and the NMSE against the
un-normalised ``H_herm_cplx`` (:105-114).  Results: ``./results/ldamp/train-<train>_test-<test>/results.pt`` (+ ``results.png``).

Deviations: the reference loops over every batch of the loader and keeps the last one's NMSE (:96-114); here the first
``--num_channels`` items are the batch.  The random directions of the divergence estimate are torch's CUDA generator stream in the
reference; here they are the library's Philox stream keyed by ``--seed`` (``--noise device``) or numpy's global stream (``--noise host``,
drawn after the batch is loaded, unroll by unroll).  Arguments of the reference are kept (:16-22); additions are marked ``[added]``.
"""
import argparse
import copy
import os

import numpy as np

from .config import default_config
from .loaders import Channels

TRAIN_BACKBONE = 'FlippedUNet'
SPACING_RANGE, PILOT_ALPHA_RANGE = [0.5], [0.6]
TRAIN_SEED, TEST_SEED = 1234, 4321


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--gpu', type=int, default=0)
    p.add_argument('--train', type=str, default='CDL-C')
    p.add_argument('--test', type=str, default='CDL-C')
    p.add_argument('--snr_range', nargs='+', type=float, default=np.arange(-10, 35, 5))
    # additions of this build
    p.add_argument('--seed', type=int, default=None, help='[added] seed of numpy\'s global RNG and of the device-drawn directions '
                                                           '(default: not seeded, as the reference; device draws then use 0)')
    p.add_argument('--synthetic', action='store_true', help='[added] generated CDL-like channels instead of ./data')
    p.add_argument('--synthetic_weights', type=int, default=None, metavar='SEED',
                   help='[added] seed-derived weights (ldamp.seeded_state_dict) and the default configuration instead of checkpoints')
    p.add_argument('--no_plot', action='store_true', help='[added] do not write results.png')
    p.add_argument('--noise', type=str, default='device', choices=['device', 'host'],
                   help='[added] source of the random directions: the library\'s Philox stream or numpy\'s global stream')
    p.add_argument('--num_channels', type=int, default=100, help='[added] validation channels (:47)')
    return p.parse_args(argv)


def ldamp_config(channel='CDL-C', alpha=0.6):
    """The settings ``train_ldamp.py:38-73`` writes into its checkpoints."""
    c = default_config(channel)
    for k in ('ema', 'ema_rate', 'normalization', 'nonlinearity', 'sigma_dist', 'num_classes', 'ngf', 'sigma_begin', 'sigma_rate', 'sigma_end'):
        del c.model[k]
    c.model.in_channels = 2
    c.model.hidden_channels = 32
    c.model.backbone = TRAIN_BACKBONE
    c.model.kernel_size = 3
    c.model.max_unrolls = 10
    c.model.shared_nets = False
    c.model.logging = False
    c.data.array = 'ULA'
    c.data.num_pilots = int(c.data.image_size[1] * alpha)
    return c


def checkpoint_path(train, snr, alpha):
    """:63-66"""
    return os.path.join('./models/ldamp-%s/train-%s' % (TRAIN_BACKBONE, train), 'model_snr%.2f_alpha%.2f.pt' % (snr, alpha))


def result_dir(args):
    """:51-52"""
    return './results/ldamp/train-%s_test-%s' % (args.train, args.test)


def load_batch(dataset, n):
    """The first ``n`` items stacked like ``DataLoader(dataset, batch_size=n, shuffle=False)`` does, restricted to what the estimator reads."""
    if len(dataset) < n:
        raise ValueError('only %d validation channels, --num_channels is %d' % (len(dataset), n))
    items = [dataset[i] for i in range(n)]
    return {k: np.stack([it[k] for it in items]) for k in ('Y_herm', 'P_herm', 'eig1', 'H_herm_cplx')}


def estimate(model, batch, num_unrolls, directions, seed, device):
    """One batch through the HIP estimator -> per-sample NMSE (numpy float64 ``[B]``).  The only place of this script that touches the GPU."""
    import torch
    sample = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in batch.items()}
    _, logs = model(sample, num_unrolls, directions=directions, seed=seed, H=sample['H_herm_cplx'])
    return logs['nmse'].cpu().numpy().astype(np.float64)


def main(argv=None, estimate_fn=None):
    args = parse_args(argv)
    import torch
    snr_range = np.asarray(args.snr_range, dtype=np.float64)
    num_channels = int(args.num_channels)
    if args.seed is not None:
        np.random.seed(args.seed)
    device = None
    if estimate_fn is None:
        if not torch.cuda.is_available():
            raise RuntimeError('test_ldamp needs a HIP device (there is no CPU fallback)')
        device = torch.device('cuda', min(args.gpu, torch.cuda.device_count() - 1))
        estimate_fn = estimate
    nmse_log = np.zeros((len(SPACING_RANGE), len(PILOT_ALPHA_RANGE), len(snr_range), num_channels))
    out_dir = result_dir(args)
    os.makedirs(out_dir, exist_ok=True)

    model, norm, config = None, None, None
    spacing, pilot_alpha = SPACING_RANGE[0], PILOT_ALPHA_RANGE[0]
    for snr_idx, snr in enumerate(snr_range):
        if args.synthetic_weights is not None:
            from .ldamp import seeded_state_dict
            config = ldamp_config(args.train, pilot_alpha)
            state = seeded_state_dict(args.synthetic_weights, config.model.max_unrolls) if snr_idx == 0 else None
        else:
            from .checkpoint import load_checkpoint
            contents = load_checkpoint(checkpoint_path(args.train, snr, pilot_alpha))
            config, state = contents['config'], contents['model_state']
        if model is None:
            from .ldamp import LDAMP
            model = LDAMP(config.model, device=device)
        if state is not None and device is not None:
            model.load_state_dict(state)
        model.eval()

        val_config = copy.deepcopy(config)
        val_config.data.channel = args.test
        val_config.data.spacing_list = [spacing]
        val_config.data.train_snr = np.asarray([snr])
        val_config.data.noise_std = 10 ** (-val_config.data.train_snr / 20.) * np.sqrt(config.data.image_size[1])
        if norm is None:                                   # the training set, for its normalisation only (:86-89)
            train_dataset = Channels(TRAIN_SEED, config, norm=config.data.norm_channels, synthetic=args.synthetic)
            norm = [train_dataset.mean, train_dataset.std]
        dataset = Channels(TEST_SEED, val_config, norm=norm, synthetic=args.synthetic, compute_eig=True,
                           num_synthetic=max(200, num_channels))
        batch = load_batch(dataset, num_channels)
        num_unrolls = int(config.model.max_unrolls)
        directions = None
        if args.noise == 'host':
            directions = np.stack([np.random.normal(size=(num_channels, 64, 16, 2)) for _ in range(num_unrolls)]).astype(np.float32)
        nmse_log[0, 0, snr_idx] = estimate_fn(model, batch, num_unrolls, directions, args.seed or 0, device)

    avg_nmse = np.mean(nmse_log, axis=-1)
    for alpha_idx, local_alpha in enumerate(PILOT_ALPHA_RANGE):
        for snr_idx, local_snr in enumerate(snr_range):
            print('Learned D-AMP: SNR = %.2f dB, NMSE = %.2f dB' % (local_snr, 10 * np.log10(avg_nmse[0, alpha_idx, snr_idx])))

    if not args.no_plot:
        try:
            import matplotlib
            matplotlib.use('Agg')
            from matplotlib import pyplot as plt
            plt.rcParams['font.size'] = 14
            plt.figure(figsize=(10, 10))
            for alpha_idx, local_alpha in enumerate(PILOT_ALPHA_RANGE):
                plt.plot(snr_range, 10 * np.log10(avg_nmse[0, alpha_idx]), linewidth=4, label='Alpha=%.2f' % local_alpha)
            plt.grid(); plt.legend()
            plt.title('Learned Denoising AMP')
            plt.xlabel('SNR [dB]'); plt.ylabel('NMSE [dB]')
            plt.tight_layout()
            plt.savefig(os.path.join(out_dir, 'results.png'), dpi=300, bbox_inches='tight')
            plt.close()
        except ImportError:
            print('matplotlib not available: skipping results.png')

    out = {'nmse_log': nmse_log, 'avg_nmse': avg_nmse, 'snr_range': snr_range, 'pilot_alpha_range': PILOT_ALPHA_RANGE,
           'spacing_range': SPACING_RANGE, 'config': config.toDict(), 'args': vars(args)}
    torch.save(out, os.path.join(out_dir, 'results.pt'))
    return out


if __name__ == '__main__':
    main()
