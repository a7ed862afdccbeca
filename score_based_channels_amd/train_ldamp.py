"""Learned D-AMP training on the HIP library: counterpart of the reference's ``train_ldamp.py`` (``src/score_based_channels/train_ldamp.py``).

Kept from the reference: its arguments and defaults (:19-25), one model per SNR of ``--snr_range`` (:36), the configuration it writes into
its checkpoints (:38-73, ``noise_std = 10^(-snr/20) sqrt(Nt)`` as :66), the training set of seed 1234 with global normalisation (:76-79),
batches of 128 with ``shuffle`` and ``drop_last`` (:80-82), Adam at 1e-3 with ``StepLR(16, 0.1)`` stepped once per epoch over 24 epochs
(:95-97, :144), ``max_unrolls`` unrolls per step (:115), loss and logged NMSE (:118-129), the log line (:135) and the checkpoint
``./models/ldamp-FlippedUNet/train-<train>/model_snr%.2f_alpha%.2f.pt`` with the keys ``model_state, optimizer_state, scheduler_state,
config, args, loss_log, nmse_log`` (:147-155).  A checkpoint written here loads in ``test_ldamp`` unchanged.

Deviations: the batch order comes from a seeded host generator (numpy ``PCG64`` of ``--seed``; the reference uses torch's global generator
through a shuffling ``DataLoader``), the random directions of the divergence estimate from the library's Philox stream keyed by
``(--seed, global sample count, unroll)`` (the reference: torch's CUDA generator), and the initial weights from
``ldamp.seeded_state_dict(--seed)``, uniform within torch's default bounds.  The model, its gradients and Adam run in ``ldamp.Trainer``
(``csrc/ldamp_train.hip``); this script touches the GPU nowhere else.  Arguments marked ``[added]`` are additions.
"""
import argparse
import os
from collections import OrderedDict

import numpy as np

from .loaders import Channels
from .test_ldamp import TRAIN_BACKBONE, TRAIN_SEED, checkpoint_path, ldamp_config

LR, BATCH_SIZE, N_EPOCHS, DECAY_EPOCHS, DECAY_GAMMA = 1e-3, 128, 24, 16, 0.1


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--gpu', type=int, default=0)
    p.add_argument('--alpha', type=float, default=0.6)
    p.add_argument('--train', type=str, default='CDL-C')
    p.add_argument('--snr_range', nargs='+', type=float, default=np.arange(-10, 35, 5))
    p.add_argument('--synthetic', action='store_true', help='[added] generated CDL-like channels instead of ./data')
    p.add_argument('--seed', type=int, default=0, help='[added] seed of the initial weights, the batch order and the random directions')
    p.add_argument('--n_epochs', type=int, default=None, help='[added] config.training.n_epochs (default 24)')
    p.add_argument('--batch_size', type=int, default=None, help='[added] config.training.batch_size (default 128, at most 128)')
    p.add_argument('--max_steps', type=int, default=None, help='[added] stop each model after this many steps')
    p.add_argument('--init', type=str, default=None, help='[added] start every model from this checkpoint\'s model_state')
    a = p.parse_args(argv)
    for name in ('n_epochs', 'batch_size', 'max_steps'):
        v = getattr(a, name)
        if v is not None and v < 1:
            p.error('--%s must be positive (got %d)' % (name, v))
    if a.batch_size is not None and a.batch_size > BATCH_SIZE:
        p.error('--batch_size must be at most %d (got %d)' % (BATCH_SIZE, a.batch_size))
    return a


def make_config(args, train_snr):
    """:38-73"""
    c = ldamp_config(args.train, args.alpha)
    c.device = 'cuda:0'
    c.optim.lr = LR
    c.training.batch_size = BATCH_SIZE if args.batch_size is None else int(args.batch_size)
    c.training.num_workers = 0
    c.training.n_epochs = N_EPOCHS if args.n_epochs is None else int(args.n_epochs)
    c.training.decay_epochs = DECAY_EPOCHS
    c.training.decay_gamma = DECAY_GAMMA
    c.training.eval_freq = 20
    c.data.train_snr = np.asarray([train_snr])
    c.data.noise_std = 10 ** (-c.data.train_snr / 20.) * np.sqrt(c.data.image_size[1])
    c.model.multi_snr = False
    c.data.mixed_channels = False
    c.data.norm_channels = 'global'
    c.data.channel = args.train
    c.data.spacing_list = [0.5]
    c.input_dim = int(np.prod(c.data.image_size) * c.data.channels)
    return c


def step_lr(epoch, lr=LR, decay_epochs=DECAY_EPOCHS, gamma=DECAY_GAMMA):
    """the learning rate ``StepLR(optimizer, decay_epochs, gamma)`` holds during epoch ``epoch`` (stepped once per epoch, :144)"""
    return lr * gamma ** (epoch // decay_epochs)


def scheduler_state(epochs_done, lr=LR, decay_epochs=DECAY_EPOCHS, gamma=DECAY_GAMMA):
    """``StepLR.state_dict()`` after ``epochs_done`` calls of ``scheduler.step()``"""
    return {'step_size': decay_epochs, 'gamma': gamma, 'base_lrs': [lr], 'last_epoch': int(epochs_done), 'verbose': False,
            '_step_count': int(epochs_done) + 1, '_get_lr_called_within_step': False, '_last_lr': [step_lr(epochs_done, lr, decay_epochs, gamma)]}


def epoch_batches(n, batch_size, rng):
    """A shuffled epoch as ``DataLoader(shuffle=True, drop_last=True)`` cuts it"""
    perm = rng.permutation(n)
    return [perm[lo:lo + batch_size] for lo in range(0, n - batch_size + 1, batch_size)]


def collate(dataset, indices):
    items = [dataset[int(i)] for i in indices]
    return {k: np.stack([it[k] for it in items]) for k in ('Y_herm', 'P_herm', 'eig1', 'H_herm_cplx')}


def log_line(epoch, step, loss, train_snr, nmse):
    """:135"""
    return 'Epoch %d, Step %d, Train Loss %.3f, Train SNR %.2f dB, Train NMSE %.3f dB' % (epoch, step, loss, train_snr, 10 * np.log10(nmse))


def config_object(config):
    """`config` as ``train_score`` writes it: the reference pickles its dotmap.DotMap; with dotmap installed the same type is written,
    without it a plain nested dict, which ``checkpoint.load_checkpoint`` re-wraps."""
    try:
        from dotmap import DotMap
        return DotMap(config.toDict())
    except ImportError:
        return config.toDict()


def save(path, trainer, config, args, epochs_done, loss_log, nmse_log):
    """:147-155"""
    import torch
    os.makedirs(os.path.dirname(path), exist_ok=True)
    model_state = OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in trainer.state_dict().items())
    torch.save({'model_state': model_state, 'optimizer_state': trainer.optimizer_state_dict(),
                'scheduler_state': scheduler_state(epochs_done, float(config.optim.lr), int(config.training.decay_epochs),
                                                   float(config.training.decay_gamma)),
                'config': config_object(config), 'args': vars(args), 'loss_log': list(loss_log), 'nmse_log': list(nmse_log)}, path)


def make_trainer(args, config, device=None):
    from . import ldamp
    state = None
    if args.init is not None:
        from .checkpoint import load_checkpoint
        state = load_checkpoint(args.init)['model_state']
    return ldamp.Trainer(config.model, state, lr=float(config.optim.lr), capacity=int(config.training.batch_size), device=device,
                         init_seed=args.seed)


def train_one(args, trainer, dataset, config, train_snr, out=print):
    """The loop of :107-144 for one model -> (loss_log, nmse_log, epochs done)"""
    import torch
    rng = np.random.Generator(np.random.PCG64(int(args.seed)))
    B, U = int(config.training.batch_size), int(config.model.max_unrolls)
    if len(dataset) < B:
        raise ValueError('the training set has %d channels, a batch needs %d (drop_last)' % (len(dataset), B))
    loss_log, nmse_log, steps, epochs_done = [], [], 0, 0
    for epoch in range(int(config.training.n_epochs)):
        trainer.set_lr(step_lr(epoch, float(config.optim.lr), int(config.training.decay_epochs), float(config.training.decay_gamma)))
        for batch_idx, indices in enumerate(epoch_batches(len(dataset), B, rng)):
            if args.max_steps is not None and steps >= args.max_steps:
                return loss_log, nmse_log, epochs_done
            sample = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in collate(dataset, indices).items()}
            loss, nmse = trainer.step(sample, U, seed=args.seed, sample_ids=np.arange(steps * B, (steps + 1) * B))
            steps += 1
            loss_log.append(loss)
            nmse_log.append(nmse)
            out(log_line(epoch, batch_idx, loss, train_snr, nmse))
        epochs_done += 1
    return loss_log, nmse_log, epochs_done


def main(argv=None, trainer_fn=None):
    args = parse_args(argv)
    device = None
    if trainer_fn is None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('train_ldamp needs a HIP device (there is no CPU fallback)')
        device = torch.device('cuda', min(args.gpu, torch.cuda.device_count() - 1))
        trainer_fn = make_trainer
    written = []
    for train_snr in np.asarray(args.snr_range, dtype=np.float64):
        config = make_config(args, train_snr)
        np.random.seed(args.seed)                            # the loader draws its pilots and noise from numpy's global stream
        dataset = Channels(TRAIN_SEED, config, norm=config.data.norm_channels, synthetic=args.synthetic, compute_eig=True)
        trainer = trainer_fn(args, config, device)
        num_params = sum(int(np.prod(v.shape)) for v in trainer.state_dict().values())
        print('Model has %d trainable parameters' % num_params)
        loss_log, nmse_log, epochs_done = train_one(args, trainer, dataset, config, train_snr)
        path = checkpoint_path(args.train, config.data.train_snr[0], args.alpha)
        save(path, trainer, config, args, epochs_done, loss_log, nmse_log)
        written.append(path)
    return written


if __name__ == '__main__':
    main()
