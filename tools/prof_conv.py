"""Performance triage helper (not part of the product): time one convolution launch in isolation.

usage: prof_conv.py [cin cout k dil B H W] [--mode f32|wino|bf16x3] [--flags 0x..] [--no-res]
"""
import argparse, ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from score_based_channels_amd import _lib, plan as P
from score_based_channels_amd.weights import (pack_conv_weight, pack_conv_weight_split, pack_conv_weight_winograd,
                                              pack_conv_weight_winograd_split, pack_conv_weight_f16x2,
                                              pack_conv_weight_winograd_f16x2, pack_conv_weight_f16, pack_conv_weight_winograd_f16)
ap = argparse.ArgumentParser()
ap.add_argument('shape', nargs='*', type=int, default=[32, 32, 3, 1, 1700, 64, 16])
ap.add_argument('--mode', default='bf16x3')
ap.add_argument('--flags', default=str(P.PRO_ELU))
ap.add_argument('--no-res', action='store_true')
ap.add_argument('--iters', type=int, default=20)
a = ap.parse_args()
cin, cout, k, dil, B, H, W = a.shape
torch.manual_seed(1); np.random.seed(1)
x = torch.randn(B, H, W, cin, device='cuda'); res = torch.randn(B, H, W, cout, device='cuda')
wn = np.random.randn(cout, cin, k, k).astype(np.float32) / 17
keep = [torch.from_numpy(pack_conv_weight(wn)).cuda()]
out = torch.empty(B, H, W, cout, device='cuda')
op = _lib.sbc_op(kind=P.CONV, flags=int(a.flags, 0), B=B, H=H, W=W, cin=cin, cout=cout, ksize=k, dil=dil,
                 in_=x.data_ptr(), out=out.data_ptr(), weight=keep[0].data_ptr())
if not a.no_res:
    op.res1 = res.data_ptr()
if int(a.flags, 0) & P.PRO_NORM:
    st = torch.randn(B, 3, cin, device='cuda') * 0.3 + torch.tensor([0.0, 1.0, 0.0], device='cuda').view(1, 3, 1); op.stats = st.data_ptr()
if a.mode == 'wino':
    keep.append(torch.from_numpy(pack_conv_weight_winograd(wn)).cuda()); op.weight_wino = keep[-1].data_ptr()
if a.mode == 'bf16x3':
    keep.append(torch.from_numpy(pack_conv_weight_split(wn).view(np.float32)).cuda()); op.weight_split = keep[-1].data_ptr()
if os.environ.get('SBC_LIB_PATH'):
    _lib.LIB_PATH = os.environ['SBC_LIB_PATH']
if a.mode == 'wx3':
    keep.append(torch.from_numpy(pack_conv_weight_winograd_split(wn).view(np.float32)).cuda()); op.weight_wino_split = keep[-1].data_ptr()
if a.mode in ('f16x2', 'wx2'):
    keep.append(torch.from_numpy(pack_conv_weight_f16x2(wn).view(np.float32)).cuda()); op.weight_split = keep[-1].data_ptr()
    op.flags |= P.CONV_F16X2
    if a.mode == 'wx2':
        keep.append(torch.from_numpy(pack_conv_weight_winograd_f16x2(wn).view(np.float32)).cuda()); op.weight_wino_split = keep[-1].data_ptr()
if a.mode in ('f16w', 'wf16w'):
    keep.append(torch.from_numpy(pack_conv_weight_f16(wn).view(np.float32)).cuda()); op.weight_split = keep[-1].data_ptr()
    op.flags |= P.CONV_F16W
    if a.mode == 'wf16w':
        keep.append(torch.from_numpy(pack_conv_weight_winograd_f16(wn).view(np.float32)).cuda()); op.weight_wino_split = keep[-1].data_ptr()
h = _lib.lib()
for _ in range(3):
    _lib.check(h.sbc_op_launch(C.byref(op), None))
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.iters):
    _lib.check(h.sbc_op_launch(C.byref(op), None))
e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) / a.iters * 1e3
fl = 2.0 * k * k * cin * cout * B * H * W
by = 4.0 * B * H * W * (cin + cout * (1 if a.no_res else 2))
if os.environ.get('DUMP'):
    _lib.check(h.sbc_op_launch(C.byref(op), None)); torch.cuda.synchronize()
    np.save(os.environ['DUMP'], out.cpu().numpy())
print('%s %s: %.1f us  %.1f TF(direct-equivalent)  %.2f TB/s(algorithmic)' % (a.mode, a.shape, us, fl / us / 1e6, by / us / 1e6))
