"""WGAN latent-optimisation channel estimation: the WGAN baseline of Fig. 5c.

Counterpart of the reference ``src/score_based_channels/test_wgan.py``: the generator of the checkpoint
``wgan_<model>_<spacing>/extra1/weights_epoch6000.pt`` (keys ``config``, ``gen_state``), and for every cell of ``--l2lam_range`` x
``--lr_range`` x ``--alpha_range`` and every SNR point ``--total_steps`` Adam steps on ``kept_samples`` latents against
``||G(z) P - Y||^2 + l2_lam ||z||^2`` (:145-165).  Results: ``<checkpoint dir>/wgan_results_model%s_channel%s_DETAILED.pt`` with the
reference's keys; ``oracle_log`` / ``meas_log`` / ``reg_log`` are ``[l2, lr, alpha, snr, steps, kept]``, taken before each update.

Quirks of the reference that are kept:
  * the training set (seed 1234) is built with ``config.data.norm_channels`` = ``'entrywise'`` and only lends its ``[mean, std]`` to the
    validation set (seed 4321), which is built anew for every cell, so its pilots move along numpy's global stream (:115-116);
  * the batch keys are ``H`` (``[2, 16, 64]``, the normalised channel, not the Hermitian one) and ``P`` (``[64, Np]``), ``num_pilots =
    floor(64 alpha)`` (:110-111); the NMSE is taken against the normalised ``H`` (:168-172);
  * ``global_init_z`` is ``np.random.seed(2021); normal(size=(kept, 60, 1, 1))``, identical for every cell and SNR (:96-97, :139);
  * the noise is ``sqrt(noise) / sqrt(2) * randn_like(complex Y)`` (:131-132): ``randn_like`` of a complex tensor has TOTAL variance 1, so
    the noise power is ``noise / 2``, half of what the SNR point says.  It is drawn afresh per (cell, SNR);
  * the loss is the ``torch.mean`` over the ``kept_samples`` of a cell, so every sample's loss carries the factor ``1 / kept_samples``
    (Adam's ``eps`` makes the scale matter); the number of extra layers is read from the state dict (the reference passes
    ``n_extra_layers + config.extra_gen_layers``).
Deviations: samples are independent, so all (l2_lam, lr, SNR) cells of one pilot fraction run as one batch through the same launches
(chunked to a memory budget); the data are prepared cell by cell in the reference's order first, so numpy's stream is consumed as there.
The reference draws the noise from torch's CUDA generator; here ``--noise device`` draws it on the device from torch's generator seeded
with ``--seed``, ``--noise host`` from numpy's global stream.  Arguments of the reference are kept (:15-26); additions are marked ``[added]``.
"""
import argparse
import copy
import itertools
import os

import numpy as np

from .config import Config
from .loaders import Channels

TRAIN_SEED, VAL_SEED, MANUAL_SEED, INIT_SEED = 1234, 4321, 2020, 2021
WORKSPACE_BUDGET_BYTES = 4 << 30           # of one chunk's activations (a sample holds 2.5 .. 4.5 MB)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--gpu', type=int, default=1)
    p.add_argument('--mode', type=str, default='single')
    p.add_argument('--model', type=str, default='CDL-C')
    p.add_argument('--channel', type=str, default='CDL-C')
    p.add_argument('--spacing', type=float, default=0.5)
    p.add_argument('--l2lam_range', nargs='+', type=float, default=[1e-1, 3e-1, 1., 3.])
    p.add_argument('--lr_range', nargs='+', type=float, default=[0.03, 0.01, 0.003, 0.001])
    p.add_argument('--alpha_range', nargs='+', type=float, default=[0.6, 0.8, 1.])
    # additions of this build
    p.add_argument('--seed', type=int, default=None, help='[added] seed of numpy\'s and torch\'s global generators (default: 2020, as the reference)')
    p.add_argument('--synthetic', action='store_true', help='[added] generated CDL-like channels instead of ./data')
    p.add_argument('--synthetic_weights', type=int, default=None, metavar='SEED',
                   help='[added] seed-derived weights (wgan.seeded_state_dict, 2 extra layers) and the configuration of train_wgan.py instead of a checkpoint')
    p.add_argument('--noise', type=str, default='device', choices=['device', 'host'],
                   help='[added] source of the measurement noise: torch\'s generator on the device or numpy\'s global stream')
    p.add_argument('--total_steps', type=int, default=5000, help='[added] Adam steps per cell (:76)')
    p.add_argument('--kept_samples', type=int, default=100, help='[added] validation channels (:85)')
    p.add_argument('--snr_range', nargs='+', type=float, default=np.arange(-10, 17.5, 2.5), help='[added] SNR points in dB (:74)')
    return p.parse_args(argv)


def wgan_config(channel='CDL-C', spacing=0.5):
    """The settings ``train_wgan.py:36-59,71-74`` writes into its checkpoints."""
    c = Config()
    c.imageSize = [16, 64]
    c.nc = 2
    c.data.spacing_list = [spacing]
    c.data.norm_channels = 'entrywise'
    c.data.channel = channel
    c.nz, c.ndf, c.ngf = 60, 64, 128
    c.niter, c.batchSize, c.lrD, c.lrG, c.beta1 = 3000, 200, 5e-5, 5e-5, 0.5
    c.clamp_lower, c.clamp_upper, c.Diters = -0.01, 0.01, 5
    c.data.image_size = c.imageSize
    c.data.num_pilots = c.data.image_size[1]
    c.data.noise_std = 0.
    c.n_extra_layers = 1 if spacing == 0.5 else 0
    return c


def target_dir(args):
    """:44"""
    return 'wgan_%s_%.2f/extra1' % (args.model, args.spacing)


def checkpoint_path(args):
    """:45"""
    return os.path.join(target_dir(args), 'weights_epoch6000.pt')


def result_path(args):
    """:194-195"""
    return target_dir(args) + '/wgan_results_model%s_channel%s_DETAILED.pt' % (args.model, args.channel)


def load_batch(dataset, n):
    """The first ``n`` items stacked like ``DataLoader(dataset, batch_size=n, shuffle=False)`` does: complex ``H`` ``[n, 16, 64]`` (the
    normalised channel, :126) and ``P`` ``[n, 64, Np]``."""
    if len(dataset) < n:
        raise ValueError('only %d validation channels, --kept_samples is %d' % (len(dataset), n))
    items = [dataset[i] for i in range(n)]
    H = np.stack([it['H'] for it in items])
    return (H[:, 0] + 1j * H[:, 1]).astype(np.complex64), np.stack([it['P'] for it in items]).astype(np.complex64)


def host_normal(shape):
    """A complex normal of total variance 1 (what ``torch.randn_like`` of a complex tensor draws) from numpy's global stream"""
    re = np.random.normal(size=shape)
    return ((re + 1j * np.random.normal(size=shape)) / np.sqrt(2.)).astype(np.complex64)


def noisy_measurements(H, P, local_noise, normal):
    """:130-132: ``Y = H P + sqrt(noise) / sqrt(2) * normal``; with ``normal`` of total variance 1 the noise power is ``noise / 2``."""
    return (np.matmul(H, P) + np.sqrt(local_noise) / np.sqrt(2.) * normal).astype(np.complex64)


def estimate(netG, problem, device):
    """One batch of independent samples through the HIP optimiser -> ``{'oracle', 'meas', 'reg'}`` numpy ``[steps, B]``.  ``problem``:
    ``z0 [B, 60]``, ``H [B, 16, 64]``, ``P [B, 64, Np]``, per-sample ``lr``, ``l2_lam``, ``loss_scale`` and either ``Y [B, 16, Np]`` or
    ``noise [B]`` (the noise levels: Y is formed on the device with torch's generator), ``steps``.  The only place of this script that
    touches the GPU."""
    import torch
    from .wgan import LatentOptimizer
    B, steps = problem['z0'].shape[0], int(problem['steps'])
    opt = LatentOptimizer(netG)
    per = max(1, WORKSPACE_BUDGET_BYTES // (4 * max(1, int(_workspace_floats(netG, 1)))))
    out = {k: np.zeros((steps, B), np.float32) for k in ('oracle', 'meas', 'reg')}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                 # noqa: E731
    for lo in range(0, B, per):
        sl = slice(lo, min(B, lo + per))
        H, P = t(problem['H'][sl]), t(problem['P'][sl])
        if 'Y' in problem:
            Y = t(problem['Y'][sl])
        else:
            Y = torch.matmul(H, P)
            scale = torch.sqrt(t(np.asarray(problem['noise'][sl], np.float32))) / np.sqrt(2.)
            Y = Y + scale[:, None, None] * torch.randn_like(Y)
        _, _, logs = opt.run(t(problem['z0'][sl]), Y, P, problem['lr'][sl], problem['l2_lam'][sl], steps, H=H, loss_scale=problem['loss_scale'][sl])
        for k in out:
            out[k][:, sl] = logs[k].cpu().numpy()
    return out


def _workspace_floats(netG, B):
    from . import _lib
    return _lib.lib().sbc_wgan_workspace_floats(netG._h, int(B))


def main(argv=None, estimate_fn=None):
    args = parse_args(argv)
    import torch
    from . import wgan
    seed = MANUAL_SEED if args.seed is None else int(args.seed)
    np.random.seed(seed)
    torch.manual_seed(seed)

    if args.synthetic_weights is not None:
        config, state = wgan_config(args.model, args.spacing), wgan.seeded_state_dict(args.synthetic_weights, 2)
    else:
        from .checkpoint import load_checkpoint
        contents = load_checkpoint(checkpoint_path(args), required=('config', 'gen_state'))
        config, state = contents['config'], contents['gen_state']
    n_extra = wgan.n_extra_of(state)
    wgan.check_geometry(config.imageSize, config.nz, config.nc, config.ngf, n_extra)

    device, netG = None, None
    if estimate_fn is None:
        if not torch.cuda.is_available():
            raise RuntimeError('test_wgan needs a HIP device (there is no CPU fallback)')
        device = torch.device('cuda', min(args.gpu, torch.cuda.device_count() - 1))
        netG = wgan.DCGAN_G_Ours(config.imageSize, int(config.nz), int(config.nc), int(config.ngf), 1, n_extra, device=device)
        netG.load_state_dict(state).cuda().eval()
        estimate_fn = estimate

    dataset = Channels(TRAIN_SEED, config, norm=config.data.norm_channels, synthetic=args.synthetic)
    snr_range = np.asarray(args.snr_range, dtype=np.float64)
    noise_range = 10 ** (-snr_range / 10.)
    total_steps, kept = int(args.total_steps), int(args.kept_samples)
    spacing_list = np.asarray([args.spacing])
    l2lam_range, lr_range, alpha_range = np.asarray(args.l2lam_range), np.asarray(args.lr_range), np.asarray(args.alpha_range)
    shape = (len(l2lam_range), len(lr_range), len(alpha_range), len(snr_range), total_steps, kept)
    logs = {k: np.zeros(shape) for k in ('oracle', 'meas', 'reg')}
    os.makedirs(target_dir(args), exist_ok=True)

    np.random.seed(INIT_SEED)                           # :96-97 (and numpy's stream goes on from here, as in the reference)
    global_init_z = np.random.normal(size=(kept, int(config.nz), 1, 1))

    # the data of every cell, in the reference's order
    cells, val_config = [], None
    for meta_idx, (l2_lam, lr, pilot_alpha) in enumerate(itertools.product(l2lam_range, lr_range, alpha_range)):
        l2_idx, lr_idx, alpha_idx = np.unravel_index(meta_idx, shape[:3])
        val_config = copy.deepcopy(config)
        val_config.data.spacing_list = spacing_list
        val_config.data.num_pilots = int(np.floor(config.data.num_pilots * pilot_alpha))
        val_config.data.channel = args.channel
        val_dataset = Channels(VAL_SEED, val_config, norm=[dataset.mean, dataset.std], synthetic=args.synthetic, num_synthetic=max(200, kept))
        val_H, val_P = load_batch(val_dataset, kept)
        normals = [host_normal((kept, val_H.shape[1], val_P.shape[2])) for _ in noise_range] if args.noise == 'host' else None
        cells.append({'idx': (l2_idx, lr_idx, alpha_idx), 'l2_lam': float(l2_lam), 'lr': float(lr), 'H': val_H, 'P': val_P, 'normals': normals})

    # all (l2_lam, lr, SNR) cells of one pilot fraction are one batch
    z0 = global_init_z[:, :, 0, 0].astype(np.float32)
    for alpha_idx in range(len(alpha_range)):
        group = [c for c in cells if c['idx'][2] == alpha_idx]
        n_blocks = len(group) * len(noise_range)
        problem = {'z0': np.tile(z0, (n_blocks, 1)), 'steps': total_steps,
                   'H': np.concatenate([c['H'] for c in group for _ in noise_range]),
                   'P': np.concatenate([c['P'] for c in group for _ in noise_range]),
                   'lr': np.concatenate([np.full(kept, c['lr']) for c in group for _ in noise_range]),
                   'l2_lam': np.concatenate([np.full(kept, c['l2_lam']) for c in group for _ in noise_range]),
                   'loss_scale': np.full(n_blocks * kept, 1.0 / kept)}
        if args.noise == 'host':
            problem['Y'] = np.concatenate([noisy_measurements(c['H'], c['P'], ln, c['normals'][s]) for c in group for s, ln in enumerate(noise_range)])
        else:
            problem['noise'] = np.concatenate([np.full(kept, ln) for c in group for ln in noise_range])
        got = estimate_fn(netG, problem, device)
        for j, (c, s) in enumerate((c, s) for c in group for s in range(len(noise_range))):
            for k in logs:
                logs[k][c['idx'][0], c['idx'][1], alpha_idx, s] = got[k][:, j * kept:(j + 1) * kept]

    best = np.min(np.mean(logs['oracle'][..., -1, :], axis=-1), axis=(0, 1)) if total_steps else None
    for alpha_idx, alpha in enumerate(alpha_range):
        for snr_idx, snr in enumerate(snr_range):
            if best is not None:
                print('WGAN: alpha = %.2f, SNR = %.2f dB, best NMSE = %.2f dB' % (alpha, snr, 10 * np.log10(best[alpha_idx, snr_idx])))

    out = {'spacing_range': spacing_list, 'pilot_alpha_range': alpha_range, 'config': config.toDict(), 'snr_range': snr_range,
           'val_config': val_config.toDict(), 'l2lam_range': l2lam_range, 'lr_range': lr_range, 'oracle_log': logs['oracle'],
           'meas_log': logs['meas'], 'reg_log': logs['reg'], 'args': vars(args)}
    torch.save(out, result_path(args))
    return out


if __name__ == '__main__':
    main()
