"""GPU parity of the training operators (reverse-mode counterparts of the score-network operators, the
DSM loss and the Adam + EMA step), each launched through the C ABI (``sbc_op_launch``) and compared with PyTorch autograd
of the same operator evaluated in float64 on the CPU.  Run on the MI355X box: ``python -m pytest tests -m gpu``."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
import guarded
from guarded import current as _G, dev as _dev, out as _out, pointer_fields

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 2e-5


@pytest.fixture(scope='module')
def gpu():
    import torch
    from score_based_channels_amd import _lib
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    _lib.lib()
    return torch, _lib


# Every tensor a launch reads or writes is a view into a larger allocation with guarded margins (tests/guarded.py): `_dev` uploads an
# operand between +inf pads (``inout``: one the operator is documented to write as well), `_out` hands out an output or a scratch
# buffer of exactly the stated size between sentinel pads, and `_launch` checks after its synchronise that no pad and no input
# changed and that the outputs were written.  One Guard per test.
@pytest.fixture(autouse=True)
def _guard(gpu):
    yield guarded.begin(gpu[0])
    guarded.end()


def _scratch(n, B):
    """A zeroed weight-gradient scratch of exactly ``n`` floats (arrival counters start at zero); pads of at least one sample's share."""
    return _out(n, 'aux (wgrad scratch, %d floats)' % n, fill=0.0, pad=max(1024, -(-n // B)))


def _launch(gpu, op):
    torch, _lib = gpu
    _lib.check(_lib.lib().sbc_op_launch(C.byref(op), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    _G.check(touched=pointer_fields(op))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _nchw(torch, a):
    """NHWC numpy -> NCHW float64 torch leaf."""
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).double().requires_grad_(True)


def _nhwc(t):
    return t.detach().numpy().transpose(0, 2, 3, 1)


def _inorm_plus(torch, x, alpha, gamma, beta):
    """InstanceNorm2dPlus.forward (normalization.py:163-176) restated with torch primitives, float64."""
    means = x.mean(dim=(2, 3))
    m = means.mean(dim=-1, keepdim=True)
    v = means.var(dim=-1, keepdim=True)
    means_n = (means - m) / torch.sqrt(v + 1e-5)
    h = torch.nn.functional.instance_norm(x, eps=1e-5)
    h = h + means_n[..., None, None] * alpha[None, :, None, None]
    return gamma[None, :, None, None] * h + beta[None, :, None, None]


def _forward_stats(gpu, x, agb):
    """The forward statistics op on the device: [B][3][C]."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    B, H, W, Cc = x.shape
    st = _out((B, 3, Cc), 'stats')
    op = _lib.sbc_op(kind=P.INORM_STATS, B=B, H=H, W=W, cin=Cc, cout=Cc, in_=_p(x), out=_p(st), weight=_p(agb))
    _launch(gpu, op)
    return _G.freeze(st)                                # an output of this launch, an input of the next


@pytest.mark.parametrize('elu,accum', [(False, False), (True, False), (True, True)])
def test_grad_add(gpu, elu, accum):
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 8, 4, 32)).astype(F32) * 2
    g = rng.standard_normal(x.shape).astype(F32)
    o0 = rng.standard_normal(x.shape).astype(F32)
    ref = g * (np.where(x > 0, 1.0, np.exp(x.astype(np.float64))) if elu else 1.0) + (o0 if accum else 0.0)
    dx, dg, do = _dev(torch, x, 'x'), _dev(torch, g, 'grad'), _dev(torch, o0, 'out', inout=True)
    op = _lib.sbc_op(kind=P.GRAD_ADD, flags=(P.PRO_ELU if elu else 0) | (P.BWD_ACCUM if accum else 0), B=3, H=8, W=4, cin=32,
                     in_=_p(dx), grad=_p(dg), out=_p(do))
    _launch(gpu, op)
    assert rel_err(do.cpu().numpy(), ref) < 1e-6


@pytest.mark.parametrize('C_,B,H,W,elu,accum', [(32, 3, 64, 16, True, False), (64, 5, 32, 8, True, True),
                                                 (64, 4, 16, 4, True, False), (128, 7, 8, 2, True, True),
                                                 (32, 2, 64, 16, False, False), (32, 1, 256, 64, True, False),
                                                 (128, 2, 32, 8, True, True)])
def test_inorm_backward_matches_autograd(gpu, C_, B, H, W, elu, accum):
    """d/dx and d/d(alpha, gamma, beta) of ELU(InstanceNorm2dPlus(x)) (normalization.py:163-176, layers.py:444-449)."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(C_ + B)
    x = (rng.standard_normal((B, H, W, C_)) * 1.3 + 0.2 * rng.standard_normal((B, 1, 1, C_))).astype(F32)
    agb = np.stack([1 + 0.1 * rng.standard_normal(C_), 1 + 0.1 * rng.standard_normal(C_), 0.1 * rng.standard_normal(C_)]).astype(F32)
    g = rng.standard_normal(x.shape).astype(F32)
    o0 = rng.standard_normal(x.shape).astype(F32)
    xt = _nchw(torch, x)
    pt = [torch.from_numpy(agb[i]).double().requires_grad_(True) for i in range(3)]
    y = _inorm_plus(torch, xt, *pt)
    if elu:
        y = torch.nn.functional.elu(y)
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    ref_dx = _nhwc(xt.grad) + (o0 if accum else 0.0)
    ref_dp = np.stack([p.grad.numpy() for p in pt])
    dx, dagb, dg, do = _dev(torch, x, 'x'), _dev(torch, agb, 'agb'), _dev(torch, g, 'grad'), _dev(torch, o0, 'out', inout=True)
    st = _forward_stats(gpu, dx, dagb)
    aux = _out(B * 6 * C_, 'aux (B*6*cin floats)', must_write=False)      # exactly the documented size
    dp = _out((3, C_))
    op = _lib.sbc_op(kind=P.INORM_BWD, flags=(P.PRO_ELU if elu else 0) | (P.BWD_ACCUM if accum else 0), B=B, H=H, W=W, cin=C_,
                     in_=_p(dx), stats=_p(st), weight=_p(dagb), grad=_p(dg), out=_p(do), aux=_p(aux), wgrad=_p(dp))
    _launch(gpu, op)
    assert rel_err(do.cpu().numpy(), ref_dx) < TOL
    assert rel_err(dp.cpu().numpy(), ref_dp) < TOL


@pytest.mark.parametrize('C_,B,H,W,elu,accum', [(32, 2, 64, 16, True, False), (64, 3, 32, 8, False, True),
                                                 (128, 5, 8, 2, True, True), (64, 2, 16, 4, False, False)])
def test_maxpool5_backward_matches_autograd(gpu, C_, B, H, W, elu, accum):
    """CRPBlock pooling (layers.py:69,77-80): maxpool(ELU(x)) when ``elu``."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(C_ + H)
    x = rng.standard_normal((B, H, W, C_)).astype(F32)
    g = rng.standard_normal(x.shape).astype(F32)
    o0 = rng.standard_normal(x.shape).astype(F32)
    xt = _nchw(torch, x)
    y = torch.nn.functional.max_pool2d(torch.nn.functional.elu(xt) if elu else xt, 5, 1, 2)
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    ref = _nhwc(xt.grad) + (o0 if accum else 0.0)
    dx, dg, do = _dev(torch, x, 'x'), _dev(torch, g, 'grad'), _dev(torch, o0, 'out', inout=True)
    aux = _out(x.size, 'aux (B*H*W*cin bytes)', fill=0, dtype=torch.uint8)   # exactly the documented size
    op = _lib.sbc_op(kind=P.MAXPOOL5_BWD, flags=(P.PRO_ELU if elu else 0) | (P.BWD_ACCUM if accum else 0), B=B, H=H, W=W,
                     cin=C_, in_=_p(dx), grad=_p(dg), out=_p(do), aux=_p(aux))
    _launch(gpu, op)
    assert rel_err(do.cpu().numpy(), ref) < 1e-6


@pytest.mark.parametrize('C_,B,H,W,uh,uw,accum', [(64, 3, 16, 4, 8, 2, False), (32, 2, 64, 16, 32, 8, True),
                                                   (128, 4, 8, 2, 8, 2, False), (64, 2, 32, 8, 16, 4, True),
                                                   (32, 1, 24, 12, 12, 6, False)])
def test_upsample_backward_matches_autograd(gpu, C_, B, H, W, uh, uw, accum):
    """Adjoint of F.interpolate(mode='bilinear', align_corners=True) (MSFBlock, layers.py:182)."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(H + uh)
    g = rng.standard_normal((B, H, W, C_)).astype(F32)
    o0 = rng.standard_normal((B, uh, uw, C_)).astype(F32)
    u = _nchw(torch, o0)
    y = torch.nn.functional.interpolate(u, size=(H, W), mode='bilinear', align_corners=True)
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    ref = _nhwc(u.grad) + (o0 if accum else 0.0)
    dg, do = _dev(torch, g, 'grad'), _dev(torch, o0, 'out', inout=True)
    op = _lib.sbc_op(kind=P.UPSAMPLE_BWD, flags=P.BWD_ACCUM if accum else 0, B=B, H=H, W=W, cin=C_, up_h=uh, up_w=uw,
                     grad=_p(dg), out=_p(do))
    _launch(gpu, op)
    assert rel_err(do.cpu().numpy(), ref) < 2e-6


def test_pool_backward(gpu):
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(5)
    g = rng.standard_normal((3, 8, 4, 64)).astype(F32)
    dg = _dev(torch, g)
    out = _out((3, 16, 8, 64))
    op = _lib.sbc_op(kind=P.POOL_BWD, B=3, H=16, W=8, cin=64, grad=_p(dg), out=_p(out))
    _launch(gpu, op)
    ref = np.repeat(np.repeat(g, 2, axis=1), 2, axis=2) * 0.25
    assert np.array_equal(out.cpu().numpy(), ref.astype(F32))


WGRAD_CASES = [
    # cin, cout, k, dil, B, H, W, prologue
    (32, 32, 3, 1, 3, 64, 16, 'norm_elu'),
    (32, 32, 3, 1, 5, 64, 16, 'elu'),
    (32, 64, 3, 1, 2, 64, 16, 'norm_elu'),
    (32, 64, 1, 1, 2, 64, 16, ''),
    (64, 64, 3, 1, 3, 32, 8, 'norm_elu'),
    (64, 64, 1, 1, 3, 32, 8, ''),
    (64, 64, 3, 1, 5, 16, 4, 'elu'),
    (64, 64, 3, 2, 9, 8, 2, 'norm_elu'),
    (64, 128, 3, 2, 9, 8, 2, 'norm_elu'),
    (128, 128, 3, 4, 7, 8, 2, 'norm_elu'),
    (128, 128, 3, 1, 7, 8, 2, ''),
    (128, 64, 3, 1, 6, 8, 2, ''),
    (64, 32, 3, 1, 2, 32, 8, ''),
    (32, 32, 3, 1, 70, 64, 16, 'elu'),          # more tiles than chunks: workgroups walk several tiles
    (32, 32, 3, 1, 1, 256, 64, 'norm_elu'),     # large-array config (Nt256 x Nr64): one image row per tile, halo rows
    (64, 64, 3, 1, 1, 128, 32, 'elu'),
    (128, 128, 3, 4, 1, 32, 8, 'norm_elu'),     # dilation 4 with a real halo (tiles of 8 rows inside a 32-row image)
    (64, 128, 3, 2, 2, 32, 8, 'norm_elu'),
    # widths of 1 and 2 under dilation (the 16 x 1 and 8 x 2 levels of 128 x 8 and 64 x 16 arrays): only the centre column of taps
    # reads the image; several images per 64-pixel tile and a partial last tile (48 and 80 pixels)
    (64, 64, 3, 2, 3, 16, 1, 'norm_elu'),
    (128, 128, 3, 4, 5, 8, 2, 'norm_elu'),
    (32, 32, 3, 1, 1, 16, 64, 'norm_elu'),      # 64-pixel rows (a 16 x 64 array): one row per tile
]


@pytest.mark.parametrize('cin,cout,k,dil,B,H,W,pro', WGRAD_CASES)
def test_conv_weight_gradient_matches_autograd(gpu, cin, cout, k, dil, B, H, W, pro):
    """dL/dW, dL/db of nn.Conv2d (layers.py:28-60) behind the forward prologue (InstanceNorm++ affine, ELU)."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(hash((cin, cout, k, dil, B)) % (2 ** 31))
    x = (rng.standard_normal((B, H, W, cin)) * 1.2 + 0.1).astype(F32)
    g = rng.standard_normal((B, H, W, cout)).astype(F32)
    agb = np.stack([1 + 0.1 * rng.standard_normal(cin), 1 + 0.1 * rng.standard_normal(cin), 0.1 * rng.standard_normal(cin)]).astype(F32)
    dx, dg, dagb = _dev(torch, x), _dev(torch, g), _dev(torch, agb)
    a = torch.from_numpy(x.transpose(0, 3, 1, 2).copy()).double()
    flags, st = 0, None
    if 'norm' in pro:
        flags |= P.PRO_NORM
        st = _forward_stats(gpu, dx, dagb)
        a = _inorm_plus(torch, a, *[torch.from_numpy(agb[i]).double() for i in range(3)])
    if 'elu' in pro:
        flags |= P.PRO_ELU
        a = torch.nn.functional.elu(a)
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(a, w, b, padding=dil * (k // 2), dilation=dil)
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    n_scr = int(_lib.lib().sbc_wgrad_scratch_floats(B, H, W, cin, cout, k))
    assert n_scr > 0
    aux = _scratch(n_scr, B)
    dw = _out((cout, cin, k, k))
    db = _out((cout,))
    op = _lib.sbc_op(kind=P.CONV_WGRAD, flags=flags, B=B, H=H, W=W, cin=cin, cout=cout, ksize=k, dil=dil, in_=_p(dx),
                     stats=_p(st), grad=_p(dg), aux=_p(aux), wgrad=_p(dw), bgrad=_p(db))
    _launch(gpu, op)
    assert rel_err(dw.cpu().numpy(), w.grad.numpy()) < TOL
    assert rel_err(db.cpu().numpy(), b.grad.numpy()) < TOL
    first = dw.clone()
    dw.fill_(float('nan'))
    _launch(gpu, op)                                   # same scratch again: the arrival counters were left at zero
    assert torch.equal(dw, first)


@pytest.mark.parametrize('cin,cout,k', [(32, 32, 3), (32, 64, 3), (32, 64, 1), (64, 64, 1), (64, 128, 3), (128, 64, 3),
                                        (128, 128, 3)])
def test_device_weight_packing_matches_host_packer(gpu, cin, cout, k):
    """SBC_OP_PACK_WEIGHT writes exactly what sbc_pack_conv_weight_split writes on the host; with SBC_PACK_ADJOINT, what
    the host packer writes for the flipped, transposed weight."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.weights import pack_conv_weight_split
    rng = np.random.default_rng(cin + cout + k)
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(F32)
    dw = _dev(torch, w)
    from score_based_channels_amd.weights import pack_conv_weight_winograd_split
    for adj in (False, True):
        wa = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)) if adj else w
        for wino in ((False, True) if k == 3 else (False,)):
            host = pack_conv_weight_winograd_split(wa) if wino else pack_conv_weight_split(wa)
            out = _out(host.size, 'out (packed, adj %d wino %d)' % (adj, wino), fill=0, dtype=torch.int16)   # exactly the packed size
            op = _lib.sbc_op(kind=P.PACK_WEIGHT, flags=(P.PACK_ADJOINT if adj else 0) | (P.PACK_WINOGRAD if wino else 0),
                             cin=cin, cout=cout, ksize=k, in_=_p(dw), out=_p(out))
            _launch(gpu, op)
            assert np.array_equal(out.cpu().numpy().view(np.uint16).ravel(), host.ravel()), (adj, wino)


@pytest.mark.parametrize('mode', ['plain', 'elu', 'elu_plus_other', 'elu_in_place'])
@pytest.mark.parametrize('cin,cout,k,dil,B,H,W', [(32, 64, 1, 1, 2, 64, 16), (32, 64, 3, 1, 2, 64, 16), (64, 128, 3, 2, 5, 8, 2),
                                                   (128, 64, 3, 1, 5, 8, 2), (64, 64, 3, 1, 3, 16, 4), (128, 128, 3, 4, 5, 8, 2),
                                                   (32, 32, 3, 1, 3, 64, 16),
                                                   # widths 1 and 2 (16 x 1: the lowest level of a 128 x 8 array; 2 x 2: of 16 x 16), 16 x 64
                                                   (64, 128, 3, 2, 3, 16, 1), (128, 128, 3, 4, 3, 16, 1), (128, 64, 3, 1, 3, 16, 1),
                                                   (128, 128, 3, 1, 5, 2, 2), (64, 128, 3, 2, 5, 2, 2),
                                                   (32, 32, 3, 1, 2, 16, 64), (32, 64, 1, 1, 2, 16, 64)])
def test_input_gradient_is_a_conv_with_adjoint_weights(gpu, cin, cout, k, dil, B, H, W, mode):
    """dL/d(conv input) = SBC_OP_CONV(grad, adjoint-packed weight): the route train.py takes for every convolution.  With
    SBC_EPI_ELUGRAD the epilogue also goes back through the forward ELU prologue (times ELU'(x)) and adds the gradient
    collected so far, from another buffer or from the output buffer itself."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(cin * 3 + cout + k)
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(F32)
    g = rng.standard_normal((B, H, W, cout)).astype(F32)
    x = (rng.standard_normal((B, H, W, cin)) * 1.5).astype(F32)
    other = rng.standard_normal((B, H, W, cin)).astype(F32)
    xt = _nchw(torch, x)
    a = torch.nn.functional.elu(xt) if mode != 'plain' else xt
    y = torch.nn.functional.conv2d(a, torch.from_numpy(w).double(), None, padding=dil * (k // 2), dilation=dil)
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    ref = _nhwc(xt.grad) + (other if mode in ('elu_plus_other', 'elu_in_place') else 0.0)
    # (res1 == out with SBC_EPI_ELUGRAD: the gradient collected so far is read from the output buffer itself)
    dw, dg, dx, dother = _dev(torch, w, 'w'), _dev(torch, g, 'grad'), _dev(torch, x, 'x'), _dev(torch, other, 'other', inout=mode == 'elu_in_place')
    packed = _out(w.size * 3, 'packed', fill=0, dtype=torch.int16)
    op = _lib.sbc_op(kind=P.PACK_WEIGHT, flags=P.PACK_ADJOINT, cin=cin, cout=cout, ksize=k, in_=_p(dw), out=_p(packed))
    _launch(gpu, op)
    _G.freeze(packed)
    out = dother if mode == 'elu_in_place' else _out((B, H, W, cin))
    op = _lib.sbc_op(kind=P.CONV, B=B, H=H, W=W, cin=cout, cout=cin, ksize=k, dil=dil, in_=_p(dg), out=_p(out),
                     weight_split=_p(packed))
    if mode != 'plain':
        op.flags, op.res2 = P.EPI_ELUGRAD, _p(dx)
    if mode in ('elu_plus_other', 'elu_in_place'):
        op.res1 = _p(dother)
    _launch(gpu, op)
    assert rel_err(out.cpu().numpy(), ref) < TOL
    if k == 3 and dil == 1:
        # the same through the Winograd kernel (adjoint Winograd form packed on the device)
        wpacked = _out(cout * cin * 16 * 3, 'packed (Winograd)', fill=0, dtype=torch.int16)
        _launch(gpu, _lib.sbc_op(kind=P.PACK_WEIGHT, flags=P.PACK_ADJOINT | P.PACK_WINOGRAD, cin=cin, cout=cout, ksize=3,
                                 in_=_p(dw), out=_p(wpacked)))
        _G.freeze(wpacked)
        if mode == 'elu_in_place':
            dother.copy_(torch.from_numpy(other))
        else:
            out.fill_(float('nan'))
        op.weight_wino_split = _p(wpacked)
        _launch(gpu, op)
        assert rel_err(out.cpu().numpy(), ref) < TOL


def test_end_conv_backward_matches_autograd(gpu):
    """normalizer -> ELU -> end_conv -> / sigma (ncsnv2.py:291-298): gradient wrt the ELU output, the weight and the bias."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(9)
    B, H, W, Cc = 3, 64, 16, 32
    x = rng.standard_normal((B, H, W, Cc)).astype(F32)
    agb = np.stack([1 + 0.1 * rng.standard_normal(Cc), 1 + 0.1 * rng.standard_normal(Cc), 0.1 * rng.standard_normal(Cc)]).astype(F32)
    w = (rng.standard_normal((2, Cc, 3, 3)) / 17).astype(F32)
    g = rng.standard_normal((B, H, W, 2)).astype(F32)
    sigmas = np.array([3.0, 0.7, 0.05], F32)
    labels = np.array([2, 0, 1], np.int64)
    a = torch.nn.functional.elu(_inorm_plus(torch, torch.from_numpy(x.transpose(0, 3, 1, 2).copy()).double(),
                                            *[torch.from_numpy(agb[i]).double() for i in range(3)])).requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    bt = torch.zeros(2, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(a, wt, bt, padding=1) / torch.from_numpy(sigmas[labels]).double()[:, None, None, None]
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    dx, dagb, dwt, dg = _dev(torch, x), _dev(torch, agb), _dev(torch, w), _dev(torch, g)
    dsig, dlab = _dev(torch, sigmas), _dev(torch, labels)
    st = _forward_stats(gpu, dx, dagb)
    ext = _lib.sbc_endconv(sigmas=_p(dsig), labels=_p(dlab))
    aux = _scratch(int(_lib.lib().sbc_wgrad_scratch_floats(B, H, W, Cc, 2, 3)), B)
    out = _out((B, H, W, Cc))
    gw = _out((2, Cc, 3, 3))
    gb = _out((2,))
    op = _lib.sbc_op(kind=P.END_CONV_BWD, B=B, H=H, W=W, cin=Cc, cout=2, ksize=3, dil=1, in_=_p(dx), stats=_p(st),
                     weight=_p(dwt), grad=_p(dg), out=_p(out), aux=_p(aux), wgrad=_p(gw), bgrad=_p(gb),
                     ext=C.cast(C.pointer(ext), C.c_void_p))
    _launch(gpu, op)
    assert rel_err(out.cpu().numpy(), _nhwc(a.grad)) < TOL
    assert rel_err(gw.cpu().numpy(), wt.grad.numpy()) < TOL
    assert rel_err(gb.cpu().numpy(), bt.grad.numpy()) < TOL


def test_begin_conv_backward_matches_autograd(gpu):
    """h = 2x - 1 -> begin_conv (ncsnv2.py:270-275): weight and bias gradients."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(10)
    B, H, W = 3, 64, 16
    x = rng.standard_normal((B, H, W, 2)).astype(F32)
    g = rng.standard_normal((B, H, W, 32)).astype(F32)
    wt = torch.zeros(32, 2, 3, 3, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(2 * torch.from_numpy(x.transpose(0, 3, 1, 2).copy()).double() - 1, wt, bt, padding=1)
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    dx, dg = _dev(torch, x), _dev(torch, g)
    aux = _scratch(int(_lib.lib().sbc_wgrad_scratch_floats(B, H, W, 2, 32, 3)), B)
    gw = _out((32, 2, 3, 3))
    gb = _out((32,))
    op = _lib.sbc_op(kind=P.BEGIN_CONV_BWD, B=B, H=H, W=W, cin=2, cout=32, ksize=3, dil=1, in_=_p(dx), grad=_p(dg),
                     aux=_p(aux), wgrad=_p(gw), bgrad=_p(gb))
    _launch(gpu, op)
    assert rel_err(gw.cpu().numpy(), wt.grad.numpy()) < TOL
    assert rel_err(gb.cpu().numpy(), bt.grad.numpy()) < TOL


def test_dsm_perturb_and_loss_match_reference_formula(gpu):
    """ncsnv2/losses/dsm.py:14-32 with replayed noise: perturbed samples, per-sample loss and d(mean loss)/d(scores)."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(11)
    B, H, W = 5, 64, 16
    n = H * W * 2
    x = rng.standard_normal((B, n)).astype(F32)
    z = rng.standard_normal((B, n)).astype(F32)
    sigmas = np.exp(np.linspace(np.log(39.15), np.log(0.0004), 50)).astype(F32)
    labels = np.array([0, 49, 17, 30, 5], np.int64)
    dx, dz, dsig, dlab = _dev(torch, x), _dev(torch, z), _dev(torch, sigmas), _dev(torch, labels)
    ext = _lib.sbc_dsm(sigmas=_p(dsig), labels=_p(dlab), noise=_p(dz), anneal_power=2.0)
    pert, noise = _out((B, n), 'perturbed'), _out((B, n), 'noise')
    op = _lib.sbc_op(kind=P.DSM_PERTURB, B=B, H=H, W=W, cin=2, in_=_p(dx), out=_p(pert), aux=_p(noise),
                     ext=C.cast(C.pointer(ext), C.c_void_p))
    _launch(gpu, op)
    us = sigmas[labels][:, None]
    assert np.array_equal(noise.cpu().numpy(), z * us) and np.array_equal(pert.cpu().numpy(), x + z * us)
    _G.freeze(noise)                                    # the loss launch reads it
    s = torch.from_numpy(rng.standard_normal((B, n)) / us.astype(np.float64)).requires_grad_(True)
    ust = torch.from_numpy(us.astype(np.float64))
    target = -1 / ust ** 2 * torch.from_numpy((z * us).astype(np.float64))
    per = 0.5 * ((s - target) ** 2).sum(dim=-1) * ust.squeeze() ** 2.0
    per.mean(dim=0).backward()
    ds_ = _dev(torch, s.detach().numpy().astype(F32))
    loss, dsc = _out((B,), 'loss'), _out((B, n), 'd(scores)')
    op = _lib.sbc_op(kind=P.DSM_LOSS, B=B, H=H, W=W, cin=2, in_=_p(ds_), grad=_p(noise), out=_p(loss), aux=_p(dsc),
                     ext=C.cast(C.pointer(ext), C.c_void_p))
    _launch(gpu, op)
    assert np.max(np.abs(loss.cpu().numpy() / per.detach().numpy() - 1)) < 1e-5
    assert rel_err(dsc.cpu().numpy(), s.grad.numpy()) < 1e-5
    # Philox path: standard-normal moments, reproducible, keyed by (seed, sample id, offset)
    dlab0 = _dev(torch, np.zeros(B, np.int64))
    ext2 = _lib.sbc_dsm(sigmas=_p(dsig), labels=_p(dlab0), seed=7, offset=3, anneal_power=2.0)
    outs = []
    pert, noise = _out((B, n), 'perturbed (Philox)'), _out((B, n), 'noise (Philox)')
    for _ in range(2):
        op = _lib.sbc_op(kind=P.DSM_PERTURB, B=B, H=H, W=W, cin=2, in_=_p(dx), out=_p(pert), aux=_p(noise),
                         ext=C.cast(C.pointer(ext2), C.c_void_p))
        _launch(gpu, op)
        outs.append(noise.cpu().numpy() / sigmas[0])
    assert np.array_equal(outs[0], outs[1])
    assert abs(outs[0].mean()) < 0.02 and abs(outs[0].std() - 1) < 0.02 and not np.array_equal(outs[0][0], outs[0][1])


def test_adam_ema_matches_torch_optimizer(gpu):
    """torch.optim.Adam(lr=1e-4, betas=(0.9, 0.999), eps=1e-3) + EMAHelper(mu=0.999).update (train_score.py:43-49,
    models/ema.py:17-22) over four steps from the device step counter."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(12)
    n = 10007
    p0 = rng.standard_normal(n).astype(F32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(F32) for _ in range(4)]
    pt = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=1e-4, weight_decay=0.0, betas=(0.9, 0.999), amsgrad=False, eps=1e-3)
    shadow = pt.data.clone()
    dp = _dev(torch, p0, 'parameters', inout=True)
    state = _dev(torch, np.stack([np.zeros(n, F32), np.zeros(n, F32), p0]), 'state', inout=True)
    step = _dev(torch, np.zeros(1, np.int32), 'step')
    for k, g in enumerate(grads):
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        shadow = (1. - 0.999) * pt.data + 0.999 * shadow
        dg = _dev(torch, g)
        ext = _lib.sbc_adam(n=n, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-3, ema_mu=0.999, step=_p(step))
        op = _lib.sbc_op(kind=P.ADAM_EMA, in_=_p(dg), out=_p(dp), aux=_p(state), ext=C.cast(C.pointer(ext), C.c_void_p))
        _launch(gpu, op)
        step += 1
        _G.resnap(step)
        assert np.max(np.abs(dp.cpu().numpy() - pt.data.numpy())) < 5e-7 * (k + 1), k
    assert np.max(np.abs(state[2].cpu().numpy() - shadow.numpy())) < 1e-6
    assert rel_err(state[0].cpu().numpy(), opt.state[pt]['exp_avg'].numpy()) < 1e-6
    assert rel_err(state[1].cpu().numpy(), opt.state[pt]['exp_avg_sq'].numpy()) < 1e-6


# ------------------------------------------------------------------------------------------------------------------------------
# The paths the tests above leave out: the forms and arguments train.py actually uses, the shapes of other arrays than 64 x 16
# (widths of 1 and 2, images of 16 and 4 pixels), exact ties, and inputs that cancel.  Each against float64 of the same operator.

NETWORK_WEIGHTS = [(32, 32, 3), (32, 64, 3), (32, 64, 1), (64, 64, 3), (64, 64, 1), (64, 32, 3), (64, 128, 3), (128, 128, 3),
                   (128, 64, 3)]                        # every (cin, cout, k) of a packed convolution weight of the network


def test_batched_weight_packing_packs_every_entry_of_its_table(gpu):
    """SBC_OP_PACK_WEIGHT with ``aux`` = a device table (the only form train.py uses): all four forms of every weight shape of the
    network in ONE launch, at non-zero source and destination offsets; each entry bit-equal to the host packer, and the guard words
    between the entries untouched."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    from score_based_channels_amd.weights import pack_conv_weight_split, pack_conv_weight_winograd_split
    rng = np.random.default_rng(77)
    GUARD, PATTERN = 24, 0x5A5A
    src, rows, want, s_off, d_off = [], [], [], 12, GUARD
    for cin, cout, k in NETWORK_WEIGHTS:
        w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(F32)
        src.append((s_off, w))
        wa = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
        for taps, adj in [(k * k, 0), (k * k, 1)] + ([(16, 0), (16, 1)] if k == 3 else []):
            host = (pack_conv_weight_winograd_split if taps == 16 else pack_conv_weight_split)(wa if adj else w)
            assert host.size == 3 * cout * cin * taps
            rows.append((s_off, d_off, cout, cin, taps, adj))
            want.append((d_off, host.ravel()))
            d_off += host.size + GUARD
        s_off += w.size + 20                            # (a multiple of 4 floats, like the flat parameter buffer's offsets)
    flat = rng.standard_normal(s_off).astype(F32)       # what lies between the weights is not a weight
    for off, w in src:
        flat[off:off + w.size] = w.ravel()
    dflat = _dev(torch, flat)
    d_off -= GUARD                                      # the last entry ends at the last element of `out`: exactly the table's extent
    assert d_off == rows[-1][1] + want[-1][1].size
    out = _out(d_off, 'out (all packed entries)', fill=PATTERN, dtype=torch.int16)
    table = _dev(torch, np.array(rows, np.int32))
    op = _lib.sbc_op(kind=P.PACK_WEIGHT, B=len(rows), cout=128, cin=128, ksize=3, in_=_p(dflat), out=_p(out), aux=_p(table))
    _launch(gpu, op)
    got = out.cpu().numpy().view(np.uint16)
    covered = np.zeros(d_off, bool)
    for (off, host), row in zip(want, rows):
        assert np.array_equal(got[off:off + host.size], host), row
        covered[off:off + host.size] = True
    assert (~covered).sum() == GUARD * len(rows) and np.all(got[~covered] == PATTERN)


def _dsm_reference(s, noise, us, power, B, gs):
    """dsm.py:19-30 in float64 and d(mean loss * gs)/d(scores)."""
    us = us.astype(np.float64)[:, None]
    d = s.astype(np.float64) + noise.astype(np.float64) / us ** 2
    return 0.5 * np.sum(d * d, axis=-1) * us[:, 0] ** power, d * us ** power / B * gs


@pytest.mark.parametrize('B,H,W', [(5, 64, 16), (1, 9, 7), (3, 33, 5)])          # n = 2048, 126, 330 elements per sample
@pytest.mark.parametrize('grad_scale', [0.0, 0.25])
@pytest.mark.parametrize('power', [2.0, 1.5, 0.0])
def test_dsm_loss_paths(gpu, power, grad_scale, B, H, W):
    """``anneal_power`` through the sigma^2 shortcut and through powf, ``grad_scale`` (0 reads as 1), sample sizes that are no
    multiple of the 256 threads, one sample; and ``aux`` = NULL (forward-only plans): the same loss bit for bit."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(int(power * 10) + B)
    n = H * W * 2
    sigmas = np.exp(np.linspace(np.log(39.15), np.log(0.0004), 50)).astype(F32)
    labels = np.array([49, 0, 17, 30, 5][:B], np.int64)
    us = sigmas[labels]
    noise = (rng.standard_normal((B, n)).astype(F32) * us[:, None]).astype(F32)
    s = (rng.standard_normal((B, n)) / us[:, None]).astype(F32)
    ref_loss, ref_ds = _dsm_reference(s, noise, us, power, B, grad_scale if grad_scale else 1.0)
    dsig, dlab, ds_, dnz = _dev(torch, sigmas), _dev(torch, labels), _dev(torch, s), _dev(torch, noise)
    ext = _lib.sbc_dsm(sigmas=_p(dsig), labels=_p(dlab), anneal_power=power, grad_scale=grad_scale)
    loss = _out((B,))
    dsc = _out((B, n))
    op = _lib.sbc_op(kind=P.DSM_LOSS, B=B, H=H, W=W, cin=2, in_=_p(ds_), grad=_p(dnz), out=_p(loss), aux=_p(dsc),
                     ext=C.cast(C.pointer(ext), C.c_void_p))
    _launch(gpu, op)
    assert np.max(np.abs(loss.cpu().numpy() / ref_loss - 1)) < 1e-5
    assert rel_err(dsc.cpu().numpy(), ref_ds) < 1e-5
    for b in range(B):                                  # per sample: a small-sigma row must not hide behind a large one
        assert rel_err(dsc[b].cpu().numpy(), ref_ds[b]) < 1e-5, b
    loss2 = _out((B,))
    op2 = _lib.sbc_op(kind=P.DSM_LOSS, B=B, H=H, W=W, cin=2, in_=_p(ds_), grad=_p(dnz), out=_p(loss2), aux=None,
                      ext=C.cast(C.pointer(ext), C.c_void_p))
    _launch(gpu, op2)
    assert torch.equal(loss, loss2)


def test_dsm_perturb_philox_keying(gpu):
    """The draws of sample b depend on (seed, sample_id[b], offset + *step) only: permuting ``sample_id`` permutes the rows bit
    for bit, NULL reads as arange(B), offset and step add, another seed gives other draws."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    B, H, W = 4, 16, 8
    n = H * W * 2
    x = np.zeros((B, n), F32)
    sigmas = np.array([1.0], F32)
    dx, dsig, dlab = _dev(torch, x), _dev(torch, sigmas), _dev(torch, np.zeros(B, np.int64))

    def draw(seed, ids, offset, step):
        did = _dev(torch, np.asarray(ids, np.int64)) if ids is not None else None
        dstep = _dev(torch, np.array([step], np.int32)) if step is not None else None
        ext = _lib.sbc_dsm(sigmas=_p(dsig), labels=_p(dlab), sample_id=_p(did), seed=seed, offset=offset, step=_p(dstep),
                           anneal_power=2.0)
        pert = _out((B, n))
        noise = _out((B, n))
        _launch(gpu, _lib.sbc_op(kind=P.DSM_PERTURB, B=B, H=H, W=W, cin=2, in_=_p(dx), out=_p(pert), aux=_p(noise),
                                 ext=C.cast(C.pointer(ext), C.c_void_p)))
        assert torch.equal(pert, noise)                 # x = 0, sigma = 1
        return noise.cpu().numpy()

    ids = np.array([5, 2, 9, 0])
    base = draw(7, ids, 3, 0)
    assert np.isfinite(base).all() and len({base[b].tobytes() for b in range(B)}) == B
    perm = np.array([2, 0, 3, 1])
    assert np.array_equal(draw(7, ids[perm], 3, 0), base[perm])
    assert np.array_equal(draw(7, None, 3, 0), draw(7, np.arange(B), 3, 0))
    assert np.array_equal(draw(7, np.arange(B), 3, 0)[0], base[3])          # stream 0, wherever it sits in the batch
    assert np.array_equal(draw(7, ids, 1, 2), base) and np.array_equal(draw(7, ids, 3, None), base)
    assert not np.array_equal(draw(7, ids, 3, 1), base)
    other = draw(8, ids, 3, 0)
    assert np.mean(other == base) < 0.01


@pytest.mark.parametrize('n', [1, 255, 4099])
@pytest.mark.parametrize('t0,ema_mu', [(999, 0.999), (99999, 0.999), (999, -1.0)])
def test_adam_ema_far_from_step_zero(gpu, t0, ema_mu, n):
    """One step from a preset counter and moments, against the formula in float64 with python-float bias corrections (1 - 0.999^t
    is 0.63 at t = 1000 and 1 - 4e-44 at 100 000); ``ema_mu`` < 0 leaves the shadow row alone; sizes below one workgroup."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(t0 + n)
    lr, b1, b2, eps = 1e-4, 0.9, 0.999, 1e-3
    p0 = rng.standard_normal(n).astype(F32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(F32)
    m0 = (0.5 * g + 0.1 * rng.standard_normal(n)).astype(F32)
    v0 = (g.astype(np.float64) ** 2 * rng.uniform(0.5, 2, n)).astype(F32)
    sh0 = rng.standard_normal(n).astype(F32)
    t = t0 + 1
    m = m0.astype(np.float64) + (g.astype(np.float64) - m0) * (1 - b1)
    v = v0.astype(np.float64) * b2 + (1 - b2) * g.astype(np.float64) ** 2
    p = p0 - (lr / (1 - b1 ** t)) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
    dp, dg = _dev(torch, p0, 'parameters', inout=True), _dev(torch, g, 'grad')
    state = _dev(torch, np.stack([m0, v0, sh0]), 'state', inout=True)
    step = _dev(torch, np.array([t0], np.int32), 'step')
    ext = _lib.sbc_adam(n=n, lr=lr, beta1=b1, beta2=b2, eps=eps, ema_mu=ema_mu, step=_p(step))
    _launch(gpu, _lib.sbc_op(kind=P.ADAM_EMA, in_=_p(dg), out=_p(dp), aux=_p(state), ext=C.cast(C.pointer(ext), C.c_void_p)))
    assert int(step.item()) == t0                       # the counter belongs to SBC_OP_STEP_INC
    assert np.max(np.abs(dp.cpu().numpy() - p)) < 5e-7
    assert rel_err(state[0].cpu().numpy(), m) < 1e-6 and rel_err(state[1].cpu().numpy(), v) < 1e-6
    if ema_mu < 0:
        assert np.array_equal(state[2].cpu().numpy(), sh0)
    else:
        assert np.max(np.abs(state[2].cpu().numpy() - ((1 - ema_mu) * p + ema_mu * sh0.astype(np.float64)))) < 1e-6


@pytest.mark.parametrize('elu', [False, True])
@pytest.mark.parametrize('C_,B,H,W,flat', [(32, 2, 8, 2, False), (128, 3, 16, 1, False), (32, 2, 3, 3, False), (128, 2, 16, 4, False),
                                           (32, 1, 16, 4, True), (128, 2, 8, 2, True)])
def test_maxpool5_backward_with_exact_ties(gpu, C_, B, H, W, flat, elu):
    """Inputs quantised to multiples of 0.5 (most 5 x 5 windows hold their maximum several times) and an all-equal image: the
    gradient goes to the FIRST maximum in row-major order, as float64 ``max_pool2d`` autograd on the CPU does it.  Images smaller
    than the window in one or both directions."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(C_ + H + W)
    x = (np.full((B, H, W, C_), -0.5) if flat else np.round(rng.standard_normal((B, H, W, C_)) * 2) / 2).astype(F32)
    g = rng.standard_normal(x.shape).astype(F32)
    xt = _nchw(torch, x)
    y = torch.nn.functional.max_pool2d(torch.nn.functional.elu(xt) if elu else xt, 5, 1, 2)
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    ref = _nhwc(xt.grad)
    assert flat or np.mean(ref == 0) > 0.5              # ties and losers: most elements receive nothing
    dx, dg = _dev(torch, x), _dev(torch, g)
    do = _out(x.shape)
    aux = _out(x.size, 'aux (B*H*W*cin bytes)', fill=0, dtype=torch.uint8)   # exactly the documented size
    op = _lib.sbc_op(kind=P.MAXPOOL5_BWD, flags=P.PRO_ELU if elu else 0, B=B, H=H, W=W, cin=C_, in_=_p(dx), grad=_p(dg),
                     out=_p(do), aux=_p(aux))
    _launch(gpu, op)
    got = do.cpu().numpy()
    assert np.array_equal(got == 0, ref == 0)           # the same elements win
    assert rel_err(got, ref) < 1e-6


SMALL_CONV_SHAPES = [(2, 256, 64, 4), (3, 16, 64, 4), (5, 8, 8, 8), (2, 24, 16, 12), (1, 128, 8, 32)]     # B, H, W, rows per workgroup


def test_small_conv_shapes_reach_the_row_counts_they_are_meant_to():
    """Restatement of small_rows() of csrc/train_conv.hip (KEEP IN STEP): whole rows of at most 256 pixels that divide H."""
    for B, H, W, rows in SMALL_CONV_SHAPES + [(3, 64, 16, 16)]:
        r = min(max(256 // W, 1), H)
        while H % r:
            r -= 1
        assert r == rows, (H, W, r)


@pytest.mark.parametrize('B,H,W,rows', SMALL_CONV_SHAPES)
def test_begin_conv_backward_at_other_images(gpu, B, H, W, rows):
    """begin_conv's weight and bias gradients at images whose workgroups own 4, 8, 12 and 32 rows (64 x 16 gives 16 only)."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(H + W)
    x = rng.standard_normal((B, H, W, 2)).astype(F32)
    g = rng.standard_normal((B, H, W, 32)).astype(F32)
    wt = torch.zeros(32, 2, 3, 3, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(2 * torch.from_numpy(x.transpose(0, 3, 1, 2).copy()).double() - 1, wt, bt, padding=1)
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    dx, dg = _dev(torch, x), _dev(torch, g)
    n_scr = int(_lib.lib().sbc_wgrad_scratch_floats(B, H, W, 2, 32, 3))
    assert n_scr == 16 + B * (H // rows) * (9 * 2 * 32 + 32)
    aux = _scratch(n_scr, B)
    gw = _out((32, 2, 3, 3))
    gb = _out((32,))
    op = _lib.sbc_op(kind=P.BEGIN_CONV_BWD, B=B, H=H, W=W, cin=2, cout=32, ksize=3, dil=1, in_=_p(dx), grad=_p(dg),
                     aux=_p(aux), wgrad=_p(gw), bgrad=_p(gb))
    _launch(gpu, op)
    assert rel_err(gw.cpu().numpy(), wt.grad.numpy()) < TOL
    assert rel_err(gb.cpu().numpy(), bt.grad.numpy()) < TOL


@pytest.mark.parametrize('source', ['labels', 'sigma_of_step'])
@pytest.mark.parametrize('B,H,W,rows', SMALL_CONV_SHAPES)
def test_end_conv_backward_at_other_images_and_noise_sources(gpu, B, H, W, rows, source):
    """normalizer -> ELU -> end_conv -> / sigma at the same images; sigma from ``sigmas[labels[b]]`` or, with ``labels`` = NULL,
    from ``sigma_of_step[*step]`` (one level for the whole batch, as inside a Langevin plan)."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(H * 3 + W)
    Cc = 32
    x = rng.standard_normal((B, H, W, Cc)).astype(F32)
    agb = np.stack([1 + 0.1 * rng.standard_normal(Cc), 1 + 0.1 * rng.standard_normal(Cc), 0.1 * rng.standard_normal(Cc)]).astype(F32)
    w = (rng.standard_normal((2, Cc, 3, 3)) / 17).astype(F32)
    g = rng.standard_normal((B, H, W, 2)).astype(F32)
    sigmas = np.array([3.0, 0.7, 0.05, 11.0, 0.002], F32)
    labels = np.array([2, 0, 4, 1, 3][:B], np.int64)
    used = sigmas[labels] if source == 'labels' else np.full(B, sigmas[2], F32)
    a = torch.nn.functional.elu(_inorm_plus(torch, torch.from_numpy(x.transpose(0, 3, 1, 2).copy()).double(),
                                            *[torch.from_numpy(agb[i]).double() for i in range(3)])).requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    bt = torch.zeros(2, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(a, wt, bt, padding=1) / torch.from_numpy(used).double()[:, None, None, None]
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    dx, dagb, dwt, dg = _dev(torch, x), _dev(torch, agb), _dev(torch, w), _dev(torch, g)
    dsig, dlab, dstep = _dev(torch, sigmas), _dev(torch, labels), _dev(torch, np.array([2], np.int32))
    st = _forward_stats(gpu, dx, dagb)
    if source == 'labels':
        ext = _lib.sbc_endconv(sigmas=_p(dsig), labels=_p(dlab))
    else:
        ext = _lib.sbc_endconv(sigma_of_step=_p(dsig), step=_p(dstep))
    aux = _scratch(int(_lib.lib().sbc_wgrad_scratch_floats(B, H, W, Cc, 2, 3)), B)
    out = _out((B, H, W, Cc))
    gw = _out((2, Cc, 3, 3))
    gb = _out((2,))
    op = _lib.sbc_op(kind=P.END_CONV_BWD, B=B, H=H, W=W, cin=Cc, cout=2, ksize=3, dil=1, in_=_p(dx), stats=_p(st),
                     weight=_p(dwt), grad=_p(dg), out=_p(out), aux=_p(aux), wgrad=_p(gw), bgrad=_p(gb),
                     ext=C.cast(C.pointer(ext), C.c_void_p))
    _launch(gpu, op)
    ref = _nhwc(a.grad)
    for b in range(B):                                  # per sample: 1 / sigma spans 5000x within the batch
        assert rel_err(out[b].cpu().numpy(), ref[b]) < TOL, b
    assert rel_err(gw.cpu().numpy(), wt.grad.numpy()) < TOL
    assert rel_err(gb.cpu().numpy(), bt.grad.numpy()) < TOL


@pytest.mark.parametrize('C_,B,H,W,offset', [(32, 1, 64, 16, 0.0), (64, 1, 16, 1, 0.0), (128, 3, 16, 1, 0.0), (64, 3, 16, 4, 50.0),
                                             (32, 2, 64, 16, 50.0), (128, 40, 8, 2, 0.0)])
def test_inorm_backward_edges(gpu, C_, B, H, W, offset):
    """One sample; 16-pixel planes one pixel wide; planes whose mean is 50 standard deviations from zero (``x - mu`` cancels six
    bits of every float32 input); 40 samples of 128 channels for the batch sum of the parameter gradients in the last workgroup.

    The offset is +50 or -50 per channel.  With the SAME offset for every channel the input would test something else: the "++"
    term divides ``mu_c - m`` by the spread of the channel means, and with all means near 50 that difference of two float32
    numbers is itself only good to ulp(50) / spread = 2e-5 -- a float32 torch evaluation of such an input sits 1.5e-5 ... 2.4e-5
    from float64 (measured on the CPU), at this file's bound, whatever the kernel does.  With means of both signs the same
    evaluation sits at 2.5e-6 ... 4.5e-6, below half of the bound, and the cancellation in ``x - mu`` is still there."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(C_ + B + H)
    sign = np.where(rng.random((1, 1, 1, C_)) < 0.5, -1.0, 1.0)
    x = (rng.standard_normal((B, H, W, C_)) + (offset * sign + 0.2 * rng.standard_normal((B, 1, 1, C_)))).astype(F32)
    agb = np.stack([1 + 0.1 * rng.standard_normal(C_), 1 + 0.1 * rng.standard_normal(C_), 0.1 * rng.standard_normal(C_)]).astype(F32)
    g = rng.standard_normal(x.shape).astype(F32)
    xt = _nchw(torch, x)
    pt = [torch.from_numpy(agb[i]).double().requires_grad_(True) for i in range(3)]
    y = torch.nn.functional.elu(_inorm_plus(torch, xt, *pt))
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    ref_dx, ref_dp = _nhwc(xt.grad), np.stack([p.grad.numpy() for p in pt])
    dx, dagb, dg = _dev(torch, x), _dev(torch, agb), _dev(torch, g)
    do = _out(x.shape)
    st = _forward_stats(gpu, dx, dagb)
    aux = _out(B * 6 * C_, 'aux (B*6*cin floats)', must_write=False)      # exactly the documented size
    dp = _out((3, C_))
    op = _lib.sbc_op(kind=P.INORM_BWD, flags=P.PRO_ELU, B=B, H=H, W=W, cin=C_, in_=_p(dx), stats=_p(st), weight=_p(dagb),
                     grad=_p(dg), out=_p(do), aux=_p(aux), wgrad=_p(dp))
    _launch(gpu, op)
    e_dx, e_dp = rel_err(do.cpu().numpy(), ref_dx), rel_err(dp.cpu().numpy(), ref_dp)
    print('inorm_bwd C%d B%d %dx%d offset %g: dx %.2e, d(alpha, gamma, beta) %.2e' % (C_, B, H, W, offset, e_dx, e_dp))
    assert e_dx < TOL
    assert e_dp < TOL


ELEMENTWISE_SHAPES = [(32, 1, 2, 2), (128, 3, 2, 2), (32, 3, 256, 64), (128, 1, 256, 64)]


@pytest.mark.parametrize('C_,B,H,W', ELEMENTWISE_SHAPES)
def test_pool_backward_shapes(gpu, C_, B, H, W):
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(C_ + H)
    g = rng.standard_normal((B, H // 2, W // 2, C_)).astype(F32)
    dg = _dev(torch, g)
    out = _out((B, H, W, C_))
    _launch(gpu, _lib.sbc_op(kind=P.POOL_BWD, B=B, H=H, W=W, cin=C_, grad=_p(dg), out=_p(out)))
    assert np.array_equal(out.cpu().numpy(), (np.repeat(np.repeat(g, 2, axis=1), 2, axis=2) * 0.25).astype(F32))


@pytest.mark.parametrize('elu,accum', [(False, True), (True, False), (True, True)])
@pytest.mark.parametrize('C_,B,H,W', ELEMENTWISE_SHAPES)
def test_grad_add_shapes(gpu, C_, B, H, W, elu, accum):
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(C_ + H + B)
    x = rng.standard_normal((B, H, W, C_)).astype(F32) * 2
    g = rng.standard_normal(x.shape).astype(F32)
    o0 = rng.standard_normal(x.shape).astype(F32)
    ref = g * (np.where(x > 0, 1.0, np.exp(x.astype(np.float64))) if elu else 1.0) + (o0 if accum else 0.0)
    dx, dg, do = _dev(torch, x, 'x'), _dev(torch, g, 'grad'), _dev(torch, o0, 'out', inout=True)
    op = _lib.sbc_op(kind=P.GRAD_ADD, flags=(P.PRO_ELU if elu else 0) | (P.BWD_ACCUM if accum else 0), B=B, H=H, W=W, cin=C_,
                     in_=_p(dx), grad=_p(dg), out=_p(do))
    _launch(gpu, op)
    assert rel_err(do.cpu().numpy(), ref) < 1e-6


@pytest.mark.parametrize('C_,B,H,W,uh,uw,accum', [(128, 3, 16, 1, 8, 1, False), (128, 2, 2, 8, 1, 4, True), (32, 2, 64, 16, 8, 2, False),
                                                   (32, 1, 256, 64, 32, 8, True), (64, 3, 2, 2, 1, 1, False)])
def test_upsample_backward_degenerate_windows(gpu, C_, B, H, W, uh, uw, accum):
    """One-pixel-wide and one-pixel-high sources (the scale along that axis is 0 and every fine pixel reads source pixel 0), a
    ratio of 8, and the largest resize of a 256 x 64 array.  Reference: autograd through the restatement's resize, which forms the
    source coordinate in float32 as the forward kernel does (torch's float64 ``interpolate`` forms it in float64)."""
    torch, _lib = gpu
    import scorenet_autograd as SA
    from score_based_channels_amd import plan as P
    rng = np.random.default_rng(H + uh + W)
    g = rng.standard_normal((B, H, W, C_)).astype(F32)
    o0 = rng.standard_normal((B, uh, uw, C_)).astype(F32)
    u = _nchw(torch, o0)
    y = SA.bilinear_align_corners(u, (H, W))
    y.backward(torch.from_numpy(g.transpose(0, 3, 1, 2).copy()).double())
    ref = _nhwc(u.grad) + (o0 if accum else 0.0)
    dg, do = _dev(torch, g, 'grad'), _dev(torch, o0, 'out', inout=True)
    op = _lib.sbc_op(kind=P.UPSAMPLE_BWD, flags=P.BWD_ACCUM if accum else 0, B=B, H=H, W=W, cin=C_, up_h=uh, up_w=uw,
                     grad=_p(dg), out=_p(do))
    _launch(gpu, op)
    assert rel_err(do.cpu().numpy(), ref) < 2e-6


def test_conv_weight_gradient_refuses_an_image_it_cannot_tile(gpu):
    """12 x 4 = 48 pixels is neither a multiple nor a divisor of the 64-pixel tile: the launch returns the error status with its
    message and writes nothing."""
    torch, _lib = gpu
    from score_based_channels_amd import plan as P
    B, H, W, c = 2, 12, 4, 64
    dx, dg = _dev(torch, np.zeros((B, H, W, c), F32), 'x'), _dev(torch, np.zeros((B, H, W, c), F32), 'grad')
    aux = _scratch(int(_lib.lib().sbc_wgrad_scratch_floats(B, H, W, c, c, 3)), B)
    dw = _out((c, c, 3, 3))
    db = _out((c,))
    op = _lib.sbc_op(kind=P.CONV_WGRAD, flags=P.PRO_ELU, B=B, H=H, W=W, cin=c, cout=c, ksize=3, dil=1, in_=_p(dx), grad=_p(dg),
                     aux=_p(aux), wgrad=_p(dw), bgrad=_p(db))
    rc = _lib.lib().sbc_op_launch(C.byref(op), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and 'does not tile' in _lib.lib().sbc_last_error().decode()
    with pytest.raises(_lib.SbcError, match='12x4'):
        _lib.check(rc)
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()) and float(aux.abs().max()) == 0.0
    _G.check(written=False)
