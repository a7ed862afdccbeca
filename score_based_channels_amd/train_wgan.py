"""WGAN training on the HIP library: counterpart of the reference's ``train_wgan.py`` (``src/score_based_channels/train_wgan.py``).

The reference's configuration (:35-54, :71-74), schedule (:123-184), log line (:186-188), output directory (``wgan_CDL_D_%.2f``: the name
is hard-coded there, whatever the channel model, :112) and checkpoint layout (:197-202: every 500th epoch ``weights_epoch%d.pt`` with
``gen_state, disc_state, gen_opt_state, disc_opt_state, config``) are kept:

  * ``Diters = 100`` while ``gen_iterations < 25`` or when ``gen_iterations % 500 == 0``, else ``config.Diters`` = 5; the inner loop ends
    with the epoch's batches; the last batch of an epoch is smaller (no ``drop_last``) while the noise is always ``batchSize``;
  * initialisation: convolutions N(0, 0.02), BatchNorm weights N(1, 0.02) and biases 0, the dense layer torch's default
    (``wgan.init_state_dicts``), n_extra_layers = 1 for spacing 0.5, else 0.
Deviations: the noise and the batch order come from ONE seeded host generator (numpy ``PCG64`` of ``--seed``; the reference uses torch's
CUDA generator and a shuffling ``DataLoader``): per epoch a permutation of the data set, then one ``[batchSize, 60]`` normal draw per
critic and per generator iteration, in the order they run.  Both networks, their gradients and RMSprop run in ``wgan.Trainer``
(``csrc/wgan_train.hip``); this script touches the GPU nowhere else.  A checkpoint it writes loads into ``test_wgan`` (after being placed
at ``wgan_<model>_<spacing>/extra1/weights_epoch6000.pt``, where that script looks) and into the reference modules with ``strict=True``.
Arguments are additions (the reference has none), marked ``[added]``.
"""
import argparse
import os
from collections import OrderedDict

import numpy as np

from .loaders import Channels
from .test_wgan import TRAIN_SEED, wgan_config

MANUAL_SEED = 2020
DITERS_INITIAL = 100


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--gpu', type=int, default=0, help='[added] device index (the reference pins CUDA_VISIBLE_DEVICES=0)')
    p.add_argument('--channel', type=str, default='CDL-C', help='[added] config.data.channel (:40)')
    p.add_argument('--spacing', type=float, default=0.5, help='[added] config.data.spacing_list = [spacing] (:38)')
    p.add_argument('--seed', type=int, default=MANUAL_SEED, help='[added] seed of the initial weights, the batch order and the noise (default: 2020, :29)')
    p.add_argument('--synthetic', action='store_true', help='[added] generated CDL-like channels instead of ./data')
    p.add_argument('--niter', type=int, default=None, help='[added] epochs (config.niter, default 3000)')
    p.add_argument('--max_gen_iterations', type=int, default=None, help='[added] stop after this many generator iterations')
    p.add_argument('--batch_size', type=int, default=None, help='[added] config.batchSize (default 200)')
    p.add_argument('--save_every', type=int, default=500, help='[added] epochs between checkpoints (:197)')
    p.add_argument('--out_dir', type=str, default=None, help='[added] instead of the reference\'s wgan_CDL_D_<spacing>')
    p.add_argument('--init', type=str, default=None, help='[added] continue from a checkpoint of this script or of the reference\'s')
    p.add_argument('--Diters', type=int, default=None, help='[added] config.Diters (default 5)')
    p.add_argument('--Diters_initial', type=int, default=DITERS_INITIAL, help='[added] the 100 of :134-135')
    p.add_argument('--save_last', action='store_true', help='[added] also write a checkpoint when training ends')
    a = p.parse_args(argv)
    for name in ('niter', 'max_gen_iterations', 'batch_size', 'Diters'):
        v = getattr(a, name)
        if v is not None and v < (0 if name == 'max_gen_iterations' else 1):
            p.error('--%s must be positive (got %d)' % (name, v))
    if a.save_every < 1 or a.Diters_initial < 1:
        p.error('--save_every and --Diters_initial must be positive')
    return a


def make_config(args):
    c = wgan_config(args.channel, args.spacing)
    if args.niter is not None:
        c.niter = int(args.niter)
    if args.batch_size is not None:
        c.batchSize = int(args.batch_size)
    if args.Diters is not None:
        c.Diters = int(args.Diters)
    return c


def model_dir(config):
    """:111-115"""
    s = list(config.data.spacing_list)
    return 'wgan_CDL_D_%.2f' % s[0] if len(s) == 1 else 'wgan_CDL_D_min%.2f_max%.2f' % (np.min(s), np.max(s))


def diters_for(gen_iterations, diters=5, initial=DITERS_INITIAL):
    """:134-137"""
    return initial if (gen_iterations < 25 or gen_iterations % 500 == 0) else diters


def epoch_plan(n_batches, gen_iterations, diters=5, initial=DITERS_INITIAL):
    """The loop of :126-184 over one epoch of ``n_batches`` batches -> ``[[batch indices of the critic iterations], ...]``, one list per
    generator iteration (the last one may be short or, never, empty: a generator iteration follows at least one batch)."""
    plan, i = [], 0
    while i < n_batches:
        want = diters_for(gen_iterations, diters, initial)
        take = list(range(i, min(n_batches, i + want)))
        i += len(take)
        plan.append(take)
        gen_iterations += 1
    return plan


def epoch_batches(n, batch_size, rng):
    """A shuffled epoch as ``DataLoader(shuffle=True)`` without ``drop_last`` cuts it: index arrays, the last one the remainder"""
    perm = rng.permutation(n)
    return [perm[lo:lo + batch_size] for lo in range(0, n, batch_size)]


def draw_noise(rng, batch_size, nz=60):
    return rng.standard_normal((batch_size, nz)).astype(np.float32)


def load_data(config, synthetic):
    dataset = Channels(TRAIN_SEED, config, norm=config.data.norm_channels, synthetic=synthetic)
    return np.stack([np.asarray(dataset[i]['H'], np.float32) for i in range(len(dataset))])           # [N, 2, 16, 64]


def to_torch_state(sd):
    import torch
    return OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in sd.items())


def to_torch_opt(osd):
    import torch
    return {'state': {k: {a: torch.from_numpy(np.array(b)) for a, b in v.items()} for k, v in osd['state'].items()}, 'param_groups': osd['param_groups']}


def save(path, trainer, config):
    import torch
    gsd, dsd = trainer.state_dicts()
    gopt, dopt = trainer.optimizer_state_dicts()
    torch.save({'gen_state': to_torch_state(gsd), 'disc_state': to_torch_state(dsd), 'gen_opt_state': to_torch_opt(gopt),
                'disc_opt_state': to_torch_opt(dopt), 'config': config.toDict()}, path)


def make_trainer(args, config, device=None):
    """A ``wgan.Trainer`` at the reference's initial distributions or at the state of ``--init`` (weights, running statistics, square averages, step counts)"""
    from . import wgan
    hyper = dict(batch_size=int(config.batchSize), lrD=float(config.lrD), lrG=float(config.lrG), clamp=(float(config.clamp_lower), float(config.clamp_upper)), device=device)
    if args.init is None:
        gsd, dsd = wgan.init_state_dicts(args.seed, int(config.n_extra_layers))
        return wgan.Trainer(gsd, dsd, **hyper)
    from . import _lib
    from .checkpoint import load_checkpoint
    c = load_checkpoint(args.init, required=('config', 'gen_state', 'disc_state'))
    tr = wgan.Trainer(_lib.numpy_state_dict(c['gen_state']), _lib.numpy_state_dict(c['disc_state']), **hyper)
    for i, (net, key) in enumerate((('g', 'gen_opt_state'), ('d', 'disc_opt_state'))):
        state = (c.get(key) or {}).get('state', {})
        names = tr.parameter_names(net)
        if state and len(state) != len(names):
            raise ValueError('%s of %s holds %d parameters, the network has %d' % (key, args.init, len(state), len(names)))
        for k, name in enumerate(names):
            if k in state:
                tr.set_tensor(net, name, _lib.numpy_state_dict({'s': state[k]['square_avg']})['s'], 'square_avg')
                tr.steps[i] = int(float(np.asarray(state[k]['step'])))
    return tr


def log_line(epoch, niter, i, n_batches, gen_iterations, errD_real, errD_fake, errG):
    """:186-188; errD = errD_real - errD_fake in float32, as the reference subtracts two float tensors"""
    errD = np.float32(errD_real) - np.float32(errD_fake)
    return '[%d/%d][%d/%d][%d] Loss_D: %f Loss_G: %f Loss_D_real: %f Loss_D_fake %f' % (epoch, niter, i, n_batches, gen_iterations, errD, errG, errD_real, errD_fake)


def train(args, trainer, data, config, out=print):
    """The loop of :123-202 -> dict of the reference's four logs (float32 arrays) and ``lines``"""
    rng = np.random.Generator(np.random.PCG64(int(args.seed)))
    B, niter = int(config.batchSize), int(config.niter)
    logs = {k: [] for k in ('d_log', 'g_log', 'd_real_log', 'd_fake_log', 'lines')}
    directory = args.out_dir or model_dir(config)
    os.makedirs(directory, exist_ok=True)
    gen_iterations, done = 0, False
    for epoch in range(niter):
        batches = epoch_batches(len(data), B, rng)
        i = 0
        for take in epoch_plan(len(batches), gen_iterations, int(config.Diters), args.Diters_initial):
            if args.max_gen_iterations is not None and gen_iterations >= args.max_gen_iterations:
                done = True
                break
            for b in take:
                losses = trainer.critic_step(data[batches[b]], draw_noise(rng, B))
                i += 1
            errG = trainer.generator_step(draw_noise(rng, B))
            gen_iterations += 1
            errD_real, errD_fake = (np.float32(v) for v in losses.cpu().numpy())
            errG = np.float32(errG.cpu().numpy()[0])
            line = log_line(epoch, niter, i, len(batches), gen_iterations, errD_real, errD_fake, errG)
            out(line)
            for k, v in (('d_log', errD_real - errD_fake), ('g_log', errG), ('d_real_log', errD_real), ('d_fake_log', errD_fake), ('lines', line)):
                logs[k].append(v)
        if done:
            break
        if (epoch + 1) % args.save_every == 0:
            save(os.path.join(directory, 'weights_epoch%d.pt' % (epoch + 1)), trainer, config)
    if args.save_last:
        save(os.path.join(directory, 'weights_last.pt'), trainer, config)
    return {k: (v if k == 'lines' else np.asarray(v, np.float32)) for k, v in logs.items()}


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('train_wgan needs a HIP device (there is no CPU fallback)')
    config = make_config(args)
    device = torch.device('cuda', min(args.gpu, torch.cuda.device_count() - 1))
    data = load_data(config, args.synthetic)
    trainer = make_trainer(args, config, device)
    return train(args, trainer, data, config)


if __name__ == '__main__':
    main()
