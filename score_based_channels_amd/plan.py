"""Launch plan of the NCSNv2Deepest score network (and of one full Langevin step).

``NCSNv2Deepest.forward`` (``ncsnv2/models/ncsnv2.py:269-300``) issues ~700 stock kernels per call; here
the same dataflow is expressed as ~160 fused operator records (``Op``) over NHWC buffers -- one record per
HIP launch of ``libsbc_hip.so`` (``include/sbc_hip.h``).  *What* is launched in which order and which logical tensors
share storage is decided once, inside the library (``csrc/score_wire.cpp``: the fusion rules, the profiling tags, the
launch lanes, the slot assignment, the gates of a conv_mode -- the same unit ``sbc_score_create`` builds a C host's records from);
this module reads that wiring through ``sbc_score_wiring_*`` into the dataclasses below and keeps its handle (``ScorePlan.wiring``).
It needs the built library and no device (no torch, no HIP call).  ``scorenet.py`` hands the handle, its buffers and its packed
weights to the library's binder (``sbc_score_wiring_bind``); ``tests/test_plan_cpu.py`` interprets the very same records with the
CPU oracle's primitives to prove the wiring without a GPU.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

from . import _lib

# op kinds / flags: numerically identical to include/sbc_hip.h
BEGIN_CONV, INORM_STATS, CONV, MAXPOOL5, END_CONV, LANGEVIN, STEP_INC, MEASURE = 1, 2, 3, 4, 5, 6, 7, 8
PRO_ELU, PRO_NORM, PRO_NORM_SELF = 0x001, 0x002, 0x004
PRO_NORM_MOMENTS, EPI_MOMENTS_OUT = 0x4000, 0x8000
EPI_RES1_ELU, EPI_POOL, EPI_UP, EPI_ELUGRAD = 0x010, 0x020, 0x040, 0x080
CONV_F16W = 0x100
CONV_F16X2 = 0x10000
# training operators
(DSM_PERTURB, DSM_LOSS, GRAD_ADD, INORM_BWD, MAXPOOL5_BWD, UPSAMPLE_BWD, POOL_BWD, CONV_WGRAD, PACK_WEIGHT, END_CONV_BWD,
 BEGIN_CONV_BWD, ADAM_EMA) = range(9, 21)
CONV_PAIR = 21
CONV_POOL = 22
RES_BLOCK = 23
CONV_DOWN = 25           # the tail of a downsampling ResidualBlock (pooled conv2 + pooled 1x1 shortcut) in one launch (csrc/conv_down.hip)
CHAIN = 24               # a chain of RCU / CRP blocks at the 8 x 2 level in one launch (csrc/conv_chain.hip)
CHAIN_RCU, CHAIN_CRP, CHAIN_RES, CHAIN_MAX_BLOCKS = 0, 1, 2, 6
BWD_ACCUM, PACK_ADJOINT, OP_SIDE, OP_JOIN, PACK_WINOGRAD = 0x200, 0x400, 0x800, 0x1000, 0x2000

# profiling tags (sbc_op.tag; bench.py times each class by hipEvents in a single-stream segment after its timed region):
TAG_CONV_TOP = 1        # 3x3 convs ngf -> ngf at full resolution (also their own kernel symbol in csrc/conv_wx3.hip)
TAG_PAIR_TOP = 2        # fused RCU blocks (CONV_PAIR) at full resolution
TAG_CONV_MID = 3        # undilated 3x3 convs 2 ngf -> 2 ngf at half resolution (the 32x8 level of a 64x16 array)
TAG_POOL_TOP = 4        # fused CRP stages (CONV_POOL) at full resolution
TAG_RES_TOP = 6         # fused ResidualBlocks (RES_BLOCK) at full resolution
TAG_CHAIN = 7           # CHAIN records (csrc/conv_chain.hip): 7 + the index of their kernel instantiation in CHAIN_KERNELS
CHAIN_KERNELS = ((128, 2), (64, 2), (64, 4), (64, 8), (32, 8))       # (channels, width)
TAG_DOWN = 12           # CONV_DOWN records: 12 at 16-pixel rows (res2.0), 13 at 8 (res3.0)
TAG_DIRECT_MID = 5      # the TAG_CONV_MID layers without a norm prologue / resize / tile-moment output: in conv_mode f16x2 the direct
                        # persistent kernel (csrc/conv_dp.hip) takes them, the Winograd kernel the rest


@dataclass
class Tensor:
    """A logical per-sample NHWC tensor ``[H][W][C]`` (batch dimension implicit)."""
    name: str
    h: int
    w: int
    c: int
    slot: int = -1            # physical buffer (index into ``ScorePlan.slot_elems``)

    @property
    def elems(self):
        return self.h * self.w * self.c


@dataclass
class Op:
    kind: int
    name: str
    src: Optional[Tensor] = None
    dst: Optional[Tensor] = None
    weight: Optional[str] = None        # state_dict key of the conv weight / norm prefix
    weight2: Optional[str] = None       # CONV_PAIR / RES_BLOCK: state_dict key of the second convolution's weight
    bias2: Optional[str] = None         # RES_BLOCK: state_dict key of the second convolution's bias
    norm2: Optional[str] = None         # RES_BLOCK: state_dict prefix of the second norm (its alpha | gamma | beta)
    bias: Optional[str] = None
    stats: Optional[Tensor] = None
    res1: Optional[Tensor] = None
    res2: Optional[Tensor] = None
    up: Optional[Tensor] = None
    flags: int = 0
    ksize: int = 3
    dil: int = 1
    tag: int = 0
    side: bool = False        # may overlap the records that follow it, up to the next ``join`` record (SBC_OP_SIDE)
    join: bool = False        # waits for every side record issued before it (SBC_OP_JOIN)
    moments: Optional[Tensor] = None    # second output: tile moments of dst (EPI_MOMENTS_OUT), [HW/128][C][2] per sample
    geom: Optional[Tensor] = None       # INORM_STATS from tile moments: the tensor whose (H, W, C) the launch describes
    norm_key: Optional[str] = None      # CONV with PRO_NORM_SELF: state_dict prefix of the norm whose (alpha, gamma, beta) `stats` points at
    blocks: Optional[list] = None       # CHAIN: [(CHAIN_RCU | CHAIN_CRP | CHAIN_RES, weight key of conv 1, of conv 2, extra), ...]; extra: None, or for
                                        # a RES block {'bias1', 'bias2', 'norm1', 'norm2', 'dil', 'w3', 'bias3'} (w3 / bias3: shortcut conv or None)
    # launch lanes (sbc_op.lane / signal / wait, include/sbc_hip.h ABI 14; ``skip_overlap``)
    lane: int = 0                       # 0: the run stream; 1 .. MAX_LANES-1: a stream of the plan
    signal: int = 0                     # event id recorded behind the record (0: none)
    wait: tuple = ()                    # event ids the record's lane waits for in front of it (at most two)

    def inputs(self):
        return [t for t in (self.src, self.stats, self.res1, self.res2, self.up) if t is not None]

    def outputs(self):
        return [t for t in (self.dst, self.moments) if t is not None]


class Wiring:
    """Owner of an ``sbc_score_wiring`` handle: what ``sbc_score_wiring_bind`` is called on; freed with the last reference."""

    def __init__(self, handle):
        self.handle, self.n_chains = handle, 0       # n_chains: its SBC_OP_CHAIN records (one sbc_chain each)
        self._destroy = _lib.lib().sbc_score_wiring_destroy

    def __del__(self):
        self._destroy(self.handle)


@dataclass
class ScorePlan:
    ops: List[Op]
    x: Tensor                 # network input  [Nt][Nr][2]   (complex64 view of the current estimate)
    out: Tensor               # network output [Nt][Nr][2]   (complex64 view of the score)
    tensors: List[Tensor]
    slot_elems: List[int] = field(default_factory=list)   # per-sample float32 elements of each physical slot
    wiring: Optional[Wiring] = None     # the library's handle these lists were read from


# (channels, width) of the RCU blocks the library fuses into SBC_OP_CONV_PAIR launches with ``fuse_pairs=True``, and in the fp16-weight
# mode (``conv_mode='f16w'``).  Nothing in the package passes them any more; the tests pass them as explicit tuples and hold the
# library's own lists to them (tests/test_plan_golden_cpu.py).
PAIR_SHAPES = ((32, 16),)
PAIR_SHAPES_F16W = ((32, 16), (32, 32), (32, 64), (64, 16), (64, 32))

MAX_LANES, MAX_EVENTS = 4, 64

# The skip branches of the decoder (``skip_overlap=True``: the library's own list, the same; csrc/score_wire.cpp says why these and why
# one lane): (branch name prefix, the record the branch is issued behind, lane).  Every record is the same launch with the same
# arguments as in the sequential plan -- results are identical bit for bit
# (tests/test_gpu_parity.py::test_skip_overlap_plan_equals_sequential_plan).
DEFAULT_SKIP_SPEC = (('refine5.adapt_convs.0.', 'res3.1.', 1), ('refine4.adapt_convs.0.', 'res3.1.', 1), ('refine3.adapt_convs.0.', 'res3.1.', 1),
                     ('refine31.adapt_convs.0.', 'res31.1.', 1), ('refine2.adapt_convs.0.', 'res4.1.', 1))

# switches of sbc_score_wiring_create: numerically identical to include/sbc_hip.h (SBC_SCORE_* / SBC_WIRING_*)
(SCORE_FUSE_PAIRS, SCORE_FOLD_STATS, SCORE_FUSE_RES, SCORE_FUSE_CHAIN, SCORE_FUSE_DOWN, SCORE_FUSE_END,
 SCORE_SKIP_LANES) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
WIRING_OVERLAP, WIRING_PRIVATE_SLOTS = 0x100, 0x200


def build_score_plan(ngf=32, nt=64, nr=16, channels=2, share_slots=True, overlap=False, fold_stats=False, fuse_pairs=False, fuse_res=False,
                     fuse_chain=False, fuse_down=False, fuse_end=False, skip_overlap=None, conv_mode=None):
    """Op list of one ``NCSNv2Deepest.forward`` for ``[B, 2, nt, nr]`` inputs (ncsnv2.py:269-300), as the library wires it
    (``sbc_score_wiring_create``; what each switch does: include/sbc_hip.h, csrc/score_wire.cpp).  ``fuse_pairs``: True (the library's
    list of shapes), or a tuple of (channels, width); ``skip_overlap``: True, or a spec like ``DEFAULT_SKIP_SPEC``; ``share_slots=False``
    gives every logical tensor its own storage (a training step reads every activation again on the way back, ``train.py``);
    ``conv_mode``: None wires exactly what the switches ask for, a name of ``config.CONV_MODES`` puts that mode's gates in front (no
    ``fold_stats`` in 'f32' or off powers of two, the longer list of pair shapes in 'f16w').  Raises ``ValueError`` with the library's
    reason for what it refuses."""
    L = _lib.lib()
    switches = ((fuse_pairs, SCORE_FUSE_PAIRS), (fold_stats, SCORE_FOLD_STATS), (fuse_res, SCORE_FUSE_RES), (fuse_chain, SCORE_FUSE_CHAIN),
                (fuse_down, SCORE_FUSE_DOWN), (fuse_end, SCORE_FUSE_END), (skip_overlap, SCORE_SKIP_LANES), (overlap, WIRING_OVERLAP),
                (not share_slots, WIRING_PRIVATE_SLOTS))
    desc = _lib.sbc_score_wiring_desc(ngf=ngf, channels=channels, nt=nt, nr=nr, flags=sum(bit for on, bit in switches if on),
                                      conv_mode=-1 if conv_mode is None else _lib.CONV_MODE_IDS[conv_mode])
    if fuse_pairs and isinstance(fuse_pairs, tuple):
        desc.pair_shapes = (C.c_int32 * (2 * len(fuse_pairs)))(*[v for shape in fuse_pairs for v in shape])
        desc.n_pair_shapes = len(fuse_pairs)
    if skip_overlap and skip_overlap is not True:
        spec = [_lib.sbc_skip_branch(prefix.encode(), anchor.encode(), lane) for prefix, anchor, lane in skip_overlap]
        desc.skip, desc.n_skip = (_lib.sbc_skip_branch * len(spec))(*spec), len(spec)
    handle, view = C.c_void_p(), _lib.sbc_score_wiring_view()
    if L.sbc_score_wiring_create(C.byref(desc), C.byref(handle)):
        raise ValueError(L.sbc_last_error().decode())
    wiring = Wiring(handle)            # (owns the handle from here on, also when the read below raises)
    _lib.check(L.sbc_score_wiring_read(handle, C.byref(view)))
    wiring.n_chains = view.n_chains
    text = lambda b: None if b is None else b.decode()
    tensors = [Tensor(text(t.name), t.h, t.w, t.c, t.slot) for t in view.tensors[:view.n_tensors]]
    at = lambda i: None if i < 0 else tensors[i]

    def block(b):
        extra = None
        if b.type == CHAIN_RES:
            extra = dict(dil=b.dil, **{k: text(getattr(b, k)) for k in ('bias1', 'bias2', 'norm1', 'norm2', 'w3', 'bias3')})
        return (b.type, text(b.w1), text(b.w2), extra)

    ops = [Op(r.kind, text(r.name), src=at(r.src), dst=at(r.dst), weight=text(r.weight), weight2=text(r.weight2), bias2=text(r.bias2),
              norm2=text(r.norm2), bias=text(r.bias), stats=at(r.stats), res1=at(r.res1), res2=at(r.res2), up=at(r.up), flags=r.flags,
              ksize=r.ksize, dil=r.dil, tag=r.tag, side=bool(r.side), join=bool(r.join), moments=at(r.moments), geom=at(r.geom),
              norm_key=text(r.norm_key), blocks=[block(b) for b in view.blocks[r.first_block:r.first_block + r.n_blocks]] or None,
              lane=r.lane, signal=r.signal, wait=tuple(e for e in r.wait if e))
           for r in view.records[:view.n_records]]
    return ScorePlan(ops, tensors[view.x], tensors[view.out], tensors, list(view.slot_elems[:view.n_slots]), wiring)


def chain_conv_count(op):
    """Convolutions of a CHAIN record (two per block, three for a RES block with a shortcut convolution)."""
    return sum(3 if (b[3] and b[3]['w3']) else 2 for b in op.blocks)


def chain_live_tap_fraction(op):
    """Fraction of the 9 W products per output the chain kernel executes (csrc/conv_chain.hip): column units skip the taps that
    only read padding -- dx != 0 for the border columns; a dilated convolution at a width of two keeps its three dx = 0 taps."""
    w = op.src.w
    full = (3 * w + 6 * (w - 1)) / (9.0 * w)
    n = live = 0.0
    for b in op.blocks:
        k = 3 if (b[3] and b[3]['w3']) else 2
        n += k
        live += k * (3.0 / 9.0 if (b[3] and b[3]['dil'] > 1) else full)
    return live / n


def count_conv_flops(plan):
    """2 * MACs of every convolution record, per sample (820 772 864 at 64x16)."""
    total = 0
    for op in plan.ops:
        if op.kind == CONV:
            total += 2 * op.src.h * op.src.w * op.src.c * op.dst.c * op.ksize * op.ksize
        elif op.kind in (CONV_PAIR, RES_BLOCK):
            total += 2 * 2 * op.src.h * op.src.w * op.src.c * op.dst.c * 9
        elif op.kind == CONV_POOL:
            total += 2 * op.src.h * op.src.w * op.src.c * op.dst.c * 9
        elif op.kind == CONV_DOWN:               # (counted as the reference runs it: 3x3 + 1x1 at full resolution)
            total += 2 * op.src.h * op.src.w * op.src.c * op.dst.c * (9 + 1)
        elif op.kind == CHAIN:
            total += chain_conv_count(op) * 2 * op.src.h * op.src.w * op.src.c * op.dst.c * 9
        elif op.kind in (BEGIN_CONV, END_CONV):
            total += 2 * op.src.h * op.src.w * op.src.c * op.dst.c * 9
    return total
