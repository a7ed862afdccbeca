"""End-to-end coded link simulation: BER and BLER of LDPC-coded packets with estimated against ideal CSI.

Counterpart of the reference ``matlab/test_end_to_end.m`` (with ``testPackets.m`` and ``ComputeLLRMIMO.m``): stored channel estimates
-- one set per channel-estimation SNR -- are used to detect (648, 324) 802.11n LDPC packets sent over the true channels on
``num_streams`` randomly precoded QPSK streams; for each data SNR the estimate taken at the nearest channel SNR
(``snr + precoding_offset``, :38-43) serves the receiver.  All of it runs in the HIP kernels of ``csrc/link.hip`` (``link.py``).

``--channels FILE`` (``.pt``, ``.npz`` or ``.mat``) holds ``ideal_H`` ``[B, d1, d2]`` and ``est_H`` ``[alpha, channel SNR, B, d1, d2]``
as in the script, or -- the file ``test_mmse`` writes -- ``oracle_H`` and ``mmse_H`` ``[spacing, alpha, SNR, B, d1, d2]`` (spacing 0 is
used, and the file's own ``snr_range`` as the channel SNR grid).  ``--layout ours`` applies the script's
``conj(permute(., [2 3 1]))`` (:50-51), ``--layout l1`` its ``permute(., [3 2 1])`` (:47-48); either way the first dimension of the
result is the receive side.  ``--synthetic`` draws channels with ``synth.py`` and forms estimates at ``--est_nmse_db``.

Deviations: MATLAB's random streams cannot be reproduced (``link.py``); the result is written with ``torch.save`` under the script's
keys, plus ``seed``.  Arguments that the script hard-codes are options here with the script's values as defaults.
"""
import argparse
import os
import time

import numpy as np

ALPHA_ARRAY = [1, 0.8, 0.6]


def _arange_inclusive(lo, step, hi):
    return lo + step * np.arange(int(np.floor((hi - lo) / step + 1e-9)) + 1)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--channels', type=str, default=None, help='.pt / .npz / .mat file with ideal_H and est_H (or oracle_H and mmse_H)')
    p.add_argument('--target_channels', type=str, default='ours_known', help='name of the result file (:10)')
    p.add_argument('--layout', choices=('ours', 'l1'), default='ours', help='file layout: the script\'s two permutes (:46-52)')
    p.add_argument('--channel_snr_range', nargs='+', type=float, default=list(_arange_inclusive(-10.0, 2.5, 15.0)))
    p.add_argument('--precoding_offset', type=float, default=20.0)
    p.add_argument('--snr_range', nargs='+', type=float, default=list(_arange_inclusive(-10.0, 0.5, 2.0) - 20.0),
                   help='data SNR points [dB] (default (-10:0.5:2) - precoding_offset of 20)')
    p.add_argument('--num_packets', type=int, default=100000)
    p.add_argument('--mod_size', type=int, default=2)
    p.add_argument('--num_streams', type=int, default=4)
    p.add_argument('--target_alpha', type=int, default=0, help='index into the alpha dimension of est_H (0-based; the script\'s 1)')
    p.add_argument('--gpu', type=int, default=0, help='[added] HIP device')
    p.add_argument('--seed', type=int, default=1234, help='[added] seed of precoders, payloads, channel picks and noise')
    p.add_argument('--noise', choices=('device', 'host'), default='device',
                   help='[added] per-packet draws from the library\'s Philox streams, or the same streams replayed on the host')
    p.add_argument('--chunk', type=int, default=16384, help='[added] packets per launch')
    p.add_argument('--synthetic', action='store_true', help='[added] generated CDL-like channels instead of --channels')
    p.add_argument('--synthetic_channels', type=int, default=100, help='[added] size of the synthetic pool')
    p.add_argument('--synthetic_profile', type=str, default='CDL-C')
    p.add_argument('--est_nmse_db', type=float, default=-15.0, help='[added] NMSE of the synthetic estimates at every channel SNR')
    p.add_argument('--out_dir', type=str, default='./e2e_results')
    return p.parse_args(argv)


def nearest_channel_snr(snr_range, precoding_offset, channel_snr_range):
    """:38-43: per data SNR the index of the channel SNR closest to ``snr + precoding_offset`` (the first one on a tie, as ``min``)."""
    d = np.abs(np.asarray(snr_range, np.float64)[:, None] + float(precoding_offset) - np.asarray(channel_snr_range, np.float64)[None, :])
    return np.argmin(d, axis=1)


def _read_file(path):
    ext = os.path.splitext(path)[1].lower()
    if ext == '.pt':
        import torch
        raw = torch.load(path, map_location='cpu', weights_only=False)
        return {k: (v.numpy() if hasattr(v, 'numpy') else v) for k, v in raw.items()}
    if ext == '.npz':
        with np.load(path, allow_pickle=False) as f:
            return {k: f[k] for k in f.files}
    if ext == '.mat':
        try:
            from scipy.io import loadmat
            return {k: v for k, v in loadmat(path).items() if not k.startswith('__')}
        except (ImportError, NotImplementedError, ValueError):
            from .mat73 import list_variables, loadmat_variable       # MATLAB 7.3 files (HDF5)
            return {k: loadmat_variable(path, k) for k in list_variables(path) if k in ('ideal_H', 'est_H', 'oracle_H', 'mmse_H', 'snr_range')}
    raise ValueError('--channels must be a .pt, .npz or .mat file (got %r)' % path)


def load_channels(path):
    """``(ideal_H [B, d1, d2], est_full [alpha, channel SNR, B, d1, d2], channel SNR grid of the file or None)``."""
    f = _read_file(path)
    if 'ideal_H' in f and 'est_H' in f:
        ideal, est, grid = np.asarray(f['ideal_H']), np.asarray(f['est_H']), None
    elif 'oracle_H' in f and 'mmse_H' in f:
        ideal, est = np.asarray(f['oracle_H']), np.asarray(f['mmse_H'])[0]
        grid = np.asarray(f['snr_range'], np.float64).reshape(-1) if 'snr_range' in f else None
    else:
        raise ValueError('%s holds neither ideal_H / est_H nor oracle_H / mmse_H (keys: %s)' % (path, sorted(f)[:12]))
    if ideal.ndim != 3 or est.ndim != 5 or tuple(est.shape[2:]) != tuple(ideal.shape):
        raise ValueError('need ideal_H [B, d1, d2] and est_H [alpha, SNR, B, d1, d2] (got %s, %s)' % (ideal.shape, est.shape))
    return ideal.astype(np.complex64), est.astype(np.complex64), grid


def to_script_layout(ideal, est, layout):
    """:46-52: ideal ``[B, d1, d2]``, est ``[SNR, B, d1, d2]`` -> real_channels ``[rx, tx, B]``, est_channels ``[SNR, rx, tx, B]``."""
    if layout == 'l1':
        return np.transpose(ideal, (2, 1, 0)), np.transpose(est, (0, 3, 2, 1))
    return np.conj(np.transpose(ideal, (1, 2, 0))), np.conj(np.transpose(est, (0, 2, 3, 1)))


def synthetic_channels(args, n_channel_snr):
    """Channels of ``synth.py`` scaled to unit mean power, and estimates ``ideal + CN(0, nmse)`` per (alpha, channel SNR)."""
    from . import synth
    raw = synth.generate_channels(args.synthetic_profile, args.synthetic_channels, 64, 16, 0.5, args.seed)     # [B, Nr = 16, Nt = 64]
    ideal = np.conj(np.transpose(raw / np.std(raw), (0, 2, 1))).astype(np.complex64)                         # val_H layout [B, 64, 16]
    rng = np.random.Generator(np.random.Philox(key=[int(args.seed) & (2 ** 64 - 1), 4 << 32]))
    e = rng.standard_normal((len(ALPHA_ARRAY), n_channel_snr) + ideal.shape + (2,)) * np.sqrt(0.5)
    est = ideal[None, None] + 10 ** (args.est_nmse_db / 20) * e.view(np.complex128)[..., 0]
    return ideal, est.astype(np.complex64)


def result_path(args):
    """:67-68"""
    return os.path.join(args.out_dir, '%s_alpha%.2f.pt' % (args.target_channels, ALPHA_ARRAY[args.target_alpha]))


def main(argv=None):
    args = parse_args(argv)
    import torch
    from . import link

    link.check_streams(args.num_streams, args.mod_size)
    if args.num_packets < 1:
        raise ValueError('--num_packets must be >= 1')
    if not 0 <= args.target_alpha < len(ALPHA_ARRAY):
        raise ValueError('--target_alpha must index alpha_array %s' % ALPHA_ARRAY)
    channel_snr_range = np.asarray(args.channel_snr_range, np.float64)
    if args.synthetic:
        ideal, est_full = synthetic_channels(args, len(channel_snr_range))
    elif args.channels:
        ideal, est_full, grid = load_channels(args.channels)
        if grid is not None:
            channel_snr_range = grid
    else:
        raise ValueError('give --channels FILE or --synthetic')
    if est_full.shape[0] <= args.target_alpha or est_full.shape[1] != len(channel_snr_range):
        raise ValueError('est_H %s does not fit --target_alpha %d and %d channel SNR points' % (est_full.shape, args.target_alpha, len(channel_snr_range)))
    snr_range = np.asarray(args.snr_range, np.float64)
    closest = nearest_channel_snr(snr_range, args.precoding_offset, channel_snr_range)
    real_channels, est_channels = to_script_layout(ideal, est_full[args.target_alpha][closest], args.layout)
    num_rx, num_tx = real_channels.shape[:2]

    if not torch.cuda.is_available():
        raise RuntimeError('test_end_to_end needs a HIP device (there is no CPU fallback)')
    device = torch.device('cuda', min(args.gpu, torch.cuda.device_count() - 1))
    t0 = time.time()
    with torch.cuda.device(device):
        bler_ideal, ber_ideal, bler_est, ber_est = link.simulate_packets(
            real_channels, est_channels, args.mod_size, num_tx, num_rx, 'random', args.num_streams, args.num_packets, snr_range, True,
            seed=args.seed, noise=args.noise, chunk=args.chunk, device=device)
        torch.cuda.synchronize(device)
    dt = time.time() - t0
    for i, snr in enumerate(snr_range):
        print('data SNR %6.1f dB: BLER ideal %.5f est %.5f   BER ideal %.3e est %.3e' % (snr, bler_ideal[i], bler_est[i], ber_ideal[i], ber_est[i]))
    total = args.num_packets * len(snr_range)
    print('%d packets x %d SNR points x 2 receivers in %.2f s: %.0f packets/s' % (args.num_packets, len(snr_range), dt, total / dt))
    out = {'bler_ideal': bler_ideal, 'ber_ideal': ber_ideal, 'bler_est': bler_est, 'ber_est': ber_est, 'target_alpha': args.target_alpha,
           'snr_range': snr_range, 'alpha_array': np.asarray(ALPHA_ARRAY), 'precoding_offset': args.precoding_offset, 'seed': args.seed}
    path = result_path(args)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    torch.save(out, path)
    return out


if __name__ == '__main__':
    main()
