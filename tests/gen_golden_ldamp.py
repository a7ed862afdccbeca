"""Writes the Learned D-AMP fixtures from the REFERENCE's own denoiser modules (run where the reference checkout is; never on the GPU box):

    python tests/gen_golden_ldamp.py /path/to/reference

``aux_unet.FlippedNormUnet`` is imported by file path and loaded with ``ldamp.seeded_state_dict``; ``aux_models.LDAMP`` is not
instantiated (its constructor and forward call ``.cuda()``), so the loop of ``LDAMP.forward`` (aux_models.py:111-190) is restated
around the imported nets (tests/ldamp_oracle.py::run with the reference modules as the denoiser).

  tests/golden/ldamp_unet.npz         one evaluation, B = 4, net 0: input r, output in fp32 and the float64 output as fp32 + residual
  tests/golden/ldamp_unroll.npz       B = 4, Np = 38, 10 unrolls with fixed directions: inputs, directions (fp16-representable), fp32 logs
  tests/golden/ldamp_unroll_f64.npz   the float64 logs of the same run as (fp32 log) + residual: x64 = x32 + dx (two files: each below 1 MiB)
  tests/golden/ldamp_state_dict_keys.json   names and shapes of the reference modules' state_dict (19 per net x 10)
Fixtures hold data only; the weights are not stored, only their seed.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ldamp_oracle as O                                         # noqa: E402
from score_based_channels_amd import ldamp                       # noqa: E402

SEED_WEIGHTS, SEED_DATA, SEED_DIRS = 2025, 11, 5
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def reference_nets(ref_root, sd):
    spec = importlib.util.spec_from_file_location('ref_aux_unet', os.path.join(ref_root, 'src', 'score_based_channels', 'aux_unet.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    nets = torch.nn.ModuleList([mod.FlippedNormUnet(chans=16, num_pools=3) for _ in range(10)])
    holder = torch.nn.Module()
    holder.update_nets = nets
    keys = [(k, list(v.shape)) for k, v in holder.state_dict().items()]
    holder.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return holder.eval(), keys


def ref_denoiser(holder):
    # FlippedNormUnet takes [B, 1, 64, 16, 2]; the oracle loop hands planes [B, 2, 64, 16]
    def f(u, x):
        out = holder.update_nets[u](x.permute(0, 2, 3, 1).contiguous()[:, None])[:, 0]
        return out.permute(0, 3, 1, 2)
    return f


def split64(x64, x32):
    return (np.asarray(x64) - np.asarray(x32).astype(x64.dtype)).astype(np.complex64 if np.iscomplexobj(x64) else np.float32)


def main(ref_root):
    torch.set_num_threads(4)
    sd = ldamp.seeded_state_dict(SEED_WEIGHTS)
    h32, keys = reference_nets(ref_root, sd)
    h64, _ = reference_nets(ref_root, sd)
    h64 = h64.double()
    assert keys == [(n, list(s)) for n, s in ldamp.state_dict_spec()], 'state_dict_spec does not match the reference modules'
    with open(os.path.join(GOLDEN, 'ldamp_state_dict_keys.json'), 'w') as f:
        json.dump({'keys': keys}, f, indent=0)

    Y, P, eig, H = O.synthetic_problem(4, 38, 10.0, SEED_DATA)
    dirs = np.random.default_rng(SEED_DIRS).standard_normal((10, 4, 64, 16, 2)).astype(np.float16)
    d32 = dirs.astype(np.float32)

    # one evaluation: the input is the first unroll's r of the problem above
    r = (np.conj(np.transpose(P, (0, 2, 1))) @ Y / eig[:, None, None]).astype(np.complex64)
    with torch.no_grad():
        o32 = O._cplx(ref_denoiser(h32)(0, O._planes(r, torch.float32))).astype(np.complex64)
        o64 = O._cplx(ref_denoiser(h64)(0, O._planes(r, torch.float64)))
    np.savez_compressed(os.path.join(GOLDEN, 'ldamp_unet.npz'), seed_weights=SEED_WEIGHTS, r=r, out32=o32, out64_minus_out32=split64(o64, o32))

    l32 = O.run(ref_denoiser(h32), Y, P, eig, d32, 10, torch.float32)
    l64 = O.run(ref_denoiser(h64), Y, P, eig, d32, 10, torch.float64)
    np.savez_compressed(os.path.join(GOLDEN, 'ldamp_unroll.npz'), seed_weights=SEED_WEIGHTS, Y_herm=Y, P_herm=P, eig1=eig, H_herm_cplx=H,
                        directions=dirs, h32=l32['h'].astype(np.complex64), z32=l32['z'].astype(np.complex64),
                        div32=l32['div'].astype(np.float32), eps32=l32['eps'].astype(np.float32))
    np.savez_compressed(os.path.join(GOLDEN, 'ldamp_unroll_f64.npz'), h64_minus_h32=split64(l64['h'], l32['h']),
                        z64_minus_z32=split64(l64['z'], l32['z']), div64=l64['div'], eps64=l64['eps'])
    for u in range(10):
        print('unroll %d: e_ref h %.2e z %.2e div %.2e (|div| %.2f) eps %.2e  nmse %.3f' % (
            u, O.normwise(l32['h'][u], l64['h'][u]), O.normwise(l32['z'][u], l64['z'][u]), O.absolute(l32['div'][u], l64['div'][u]),
            np.max(np.abs(l64['div'][u])), np.max(l64['eps'][u]),
            np.mean(np.sum(np.abs(l64['h'][u] - H) ** 2, (1, 2)) / np.sum(np.abs(H) ** 2, (1, 2)))))
    print('unet: e_ref %.2e' % O.normwise(o32, o64))


if __name__ == '__main__':
    main(sys.argv[1])
