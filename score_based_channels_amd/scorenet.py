"""``ScoreNet`` -- host-side stand-in for the reference's ``NCSNv2Deepest`` ``nn.Module``
(``ncsnv2/models/ncsnv2.py:198-300``) whose forward runs on the HIP kernels of ``libsbc_hip.so``.

Interface kept from the reference call sites (``test_score.py:59-63,137,151``):
``ScoreNet(config)``, ``.cuda()``, ``.load_state_dict(contents['model_state'])``, ``.eval()``,
``.sigmas`` (float32 ``[num_classes]`` device tensor) and ``net(x[B,2,Nt,Nr], labels[B]) -> [B,2,Nt,Nr]``.
torch is used for device memory and streams only; no torch operator computes anything on this path.

What this host owns: which forms of the weights it packs (``load_state_dict``: every form of the selected multiplier, so that one
buffer serves every array size), the buffers (``bind``), the calibration pass and which plan a batch takes.  Which records there are
and which form goes into which ``sbc_op`` field is the library's (``plan.build_score_plan``, ``sbc_score_wiring_bind``).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from . import plan as P
from .config import CONV_MODES, DEFAULT_CONV_MODE
from .weights import (check_state_dict, fp16_state_dict, get_sigmas, pack_conv_weight, pack_conv_weight_f16,
                      pack_conv_weight_f16x2, pack_conv_weight_pooled_f16x2, pack_conv_weight_split, pack_conv_weight_winograd,
                      pack_conv_weight_winograd_f16, pack_conv_weight_winograd_f16x2, pack_conv_weight_winograd_split)


def _ptr(t, offset_elems=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_elems)


class BoundScore:
    """A score plan bound to device buffers for a fixed batch size."""

    def __init__(self, ops, x, out, slots, labels, extra_keep, plan=None):
        self.plan = plan            # the plan.ScorePlan the records were made from (record k of ``ops`` is ``plan.ops[k]``)
        self.ops = ops              # list of _lib.sbc_op (ctypes views of one array); every ext points into ``extra_keep``
        self.x = x                  # float32 [B, Nt, Nr, 2]  (view as complex64 [B, Nt, Nr])
        self.out = out              # float32 [B, Nt, Nr, 2]
        self.slots = slots
        self.labels = labels
        self.keep = extra_keep


DEFAULT_OVERLAP = False
DEFAULT_FOLD_STATS = True       # not conv_mode 'f32' (the tile moments are written by the Winograd split kernels); +2 %
DEFAULT_FUSE_PAIRS = True       # applies to the fp16-form modes only ('f16x2', 'f16w')
# ResidualBlocks without resampling at 64x16 as ONE launch (SBC_OP_RES_BLOCK, csrc/conv_res.hip; conv_mode 'f16x2' with fused pairs).
# Measured: 264-280 us per block against 2 x 150 + 10 for the launches it replaces; 1.2 % of a one-stream step,
# 0.6 % of the default two-stream step (three interleaved A/B pairs, sustained 1000 steps: 5.55 against 5.58 ms).
DEFAULT_FUSE_RES = True
# RCU / CRP runs of the 8 x 2 level as SBC_OP_CHAIN records (csrc/conv_chain.hip: eight samples resident per workgroup, only the
# filters stream): conv_mode f16x2 with fused pairs
DEFAULT_FUSE_CHAIN = True
# pooled conv2 + pooled 1x1 shortcut of the downsampling ResidualBlocks res2.0 / res3.0 as one SBC_OP_CONV_DOWN record (csrc/conv_down.hip)
DEFAULT_FUSE_DOWN = True
# the normalizer's statistics inside the end-convolution launch (SBC_PRO_NORM_SELF on the END_CONV record; csrc/ops.hip: end_conv_self_kernel)
DEFAULT_FUSE_END = True
# Small batches (a rank's share when a test_score run is sharded over several GPUs): the decoder's skip branches on launch lanes of
# their own beside the latency-bound low-resolution launches (csrc/score_wire.cpp: hoist_skip_branches; identical results).  Batches of at most this
# many 64 x 16-equivalent trajectories (B Nt Nr / 1024) take that plan
# (ScoreNet(skip_overlap=False) turns it off).
SKIP_OVERLAP_MAX_T = 600


class ScoreNet:
    """``conv_mode`` selects how the 32/64/128-channel convolutions multiply:

    ``'f16x2'`` (default)   fp32-class arithmetic on the fp16 matrix cores: every operand is scaled by a power of two (weights per
                            layer on the host) and split into two fp16 terms ``h + l`` (22-23 significant
                            bits), a product is the three fp16 MFMAs ``hl + lh + hh`` with fp32 accumulation.  Forward error
                            vs the reference 0.85e-6 (true fp32 MFMA: 0.98e-6); half the matrix instructions and a third of
                            the split arithmetic of ``'bf16x3'``.  Every layer's activations are scaled by a power of two
                            chosen once per checkpoint (``_ensure_calibrated``) so that the low fp16 term stays a normal
                            number over 17 binades; an input that leaves that window anyway (overflow, or a region too small
                            for the split to be fp32-class) raises a device flag, and the host runs that call / batch again
                            in ``'bf16x3'`` in the same process instead of returning degraded numbers.
    ``'bf16x3'``            fp32 operands split exactly into three bf16 terms (8 + 8 + 8 significand bits), six bf16 MFMAs
                            per product block, fp32 accumulation: fp32-level accuracy (forward error vs the reference
                            0.8e-6, the fp32 kernels 1.0e-6) on the bf16 matrix cores -- Winograd F(2x2,3x3) for the
                            undilated 3x3 layers (``csrc/conv_wx3.hip``), direct for the rest (``csrc/conv_x3.hip``);
    ``'f32'``               fp32 MFMA kernels (Winograd ``csrc/conv_wino.hip`` + direct ``csrc/conv_mfma.hip``).
    Both stay within the parity tolerance of the reference (tests/test_gpu_parity.py runs every case in each).
    ``'f16w'``              BASELINE config 5, "fp16 score-net weights": every parameter is rounded to fp16 when it is
                            loaded (``module.half()`` semantics; the sigma schedule stays fp32), the 32/64/128-channel
                            convolutions run as single-term ``v_mfma_f32_32x32x16_f16`` (activations fp32 in HBM, rounded
                            to fp16 as they enter the matrix cores, fp32 accumulation) in the same two kernels; begin /
                            end convolutions and InstanceNorm++ use the fp16-rounded parameters in fp32 arithmetic.
                            Oracle: the fp32 reference with fp16-rounded parameters (the reference itself cannot run
                            ``.half()``, layers.py:179); tolerance stated in tests/test_gpu_parity.py.
    """

    def __init__(self, config, device=None, conv_mode=None, overlap=None, fold_stats=None, fuse_pairs=None, fuse_res=None, fuse_chain=None, fuse_down=None, fuse_end=None,
                 skip_overlap=None):
        conv_mode = DEFAULT_CONV_MODE if conv_mode is None else conv_mode
        if conv_mode not in CONV_MODES:
            raise ValueError('conv_mode must be one of %s, got %r' % (CONV_MODES, conv_mode))
        self.conv_mode = conv_mode
        # overlap: run the independent low-resolution branches of the network (shortcut convolutions, the second input's
        # adapt / MSF convolutions of a RefineBlock) on the plan's side stream (plan.py, SBC_OP_SIDE); same arithmetic,
        # bit-identical results
        self.overlap = DEFAULT_OVERLAP if overlap is None else bool(overlap)
        # fold_stats: the full-resolution InstanceNorm++ statistics come from tile moments the producing convolution
        # writes (plan.py `stats`): the statistics launches of those tensors read a few KB per sample instead of the tensor.
        # Needs the Winograd split kernels (not conv_mode 'f32').
        self.fold_stats = (DEFAULT_FOLD_STATS if fold_stats is None else bool(fold_stats)) and conv_mode != 'f32'
        # fuse_pairs: RCU blocks (act -> conv -> act -> conv, + x; layers.py:126-134; shapes: plan.PAIR_SHAPES*) are ONE launch that keeps
        # the intermediate tensor in LDS (csrc/conv_pair.hip); the kernel reads the fp16 weight forms of 'f16x2' / 'f16w'
        self.fuse_pairs = (DEFAULT_FUSE_PAIRS if fuse_pairs is None else bool(fuse_pairs)) and conv_mode in ('f16x2', 'f16w')
        self.fuse_res = ((DEFAULT_FUSE_RES and self.fuse_pairs) if fuse_res is None else bool(fuse_res)) and conv_mode == 'f16x2'
        self.fuse_chain = ((DEFAULT_FUSE_CHAIN and self.fuse_pairs) if fuse_chain is None else bool(fuse_chain)) and conv_mode == 'f16x2'
        self.fuse_down = ((DEFAULT_FUSE_DOWN and self.fuse_pairs) if fuse_down is None else bool(fuse_down)) and conv_mode == 'f16x2'
        # fuse_end: the normalizer's statistics inside the end-convolution launch (fp32 vector arithmetic in every conv_mode; part of the
        # fused default plan, so tied to fuse_pairs like the others: the unfused plan stays what the bf16x3 re-run of a flagged batch uses)
        self.fuse_end = (DEFAULT_FUSE_END and self.fuse_pairs) if fuse_end is None else bool(fuse_end)
        # skip_overlap: True (default; plan.DEFAULT_SKIP_SPEC), False, or a spec like it (plan.build_score_plan) -- applied to small batches only
        self.skip_overlap = True if skip_overlap is None else skip_overlap
        self.config = config
        m, d = config.model, config.data
        if str(m.normalization) != 'InstanceNorm++' or str(m.nonlinearity).lower() != 'elu':
            raise NotImplementedError('the HIP path implements InstanceNorm++ / ELU (train_score.py:39-40), got %r / %r'
                                      % (m.normalization, m.nonlinearity))
        if d.logit_transform or d.rescaled:
            raise NotImplementedError('only the h = 2x - 1 input map is implemented (ncsnv2.py:270-273)')
        self.ngf = int(m.ngf)
        self.num_classes = int(m.num_classes)
        self.channels = int(d.channels)
        if self.ngf != 32 or self.channels != 2:
            raise NotImplementedError('kernels are instantiated for ngf = 32, 2 input channels')
        self.device = torch.device(device if device is not None else 'cuda:0')
        self._sigmas_np = get_sigmas(config)
        self._wdev = None
        self._woff = {}
        self._params = None             # (_wdev, its sbc_named_ptr table, the names' bytes): what bind hands the library's binder
        self._sigmas = None
        self._call_cache = {}
        self._plans = {}
        self._sd_host = None            # the loaded state dict (host arrays): what fallback_net() loads
        self._calibrated = False        # conv_mode f16x2: per-layer activation scales set on the device copy of the weights
        self._calibrating = False
        self._fallback = None
        self.range_fallbacks = 0        # module calls answered by the bf16x3 fallback because the f16x2 range flag was raised
        self.last_range_bits = 0

    # --- nn.Module look-alikes ------------------------------------------------------------------
    def cuda(self, device=None):
        if device is not None:
            self.device = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
        return self

    def to(self, device):
        self.device = torch.device(device)
        return self

    def eval(self):
        return self

    @property
    def sigmas(self):
        if self._sigmas is None:
            self._sigmas = torch.from_numpy(self._sigmas_np).to(self.device)
        return self._sigmas

    def load_state_dict(self, state_dict, strict=True):
        """Accepts the reference ``model_state`` (torch tensors) or numpy arrays; packs conv weights into
        MFMA fragment order and uploads everything as one flat float32 device tensor."""
        sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
              for k, v in state_dict.items()}
        if strict:
            check_state_dict(sd, self.config)
        if self.conv_mode == 'f16w':
            sd = fp16_state_dict(sd)
        if 'sigmas' in sd:
            self._sigmas_np = np.asarray(sd['sigmas'], np.float32)
            self._sigmas = None
        chunks, off, cur = [], {}, 0

        def add(key, arr):
            nonlocal cur
            a = np.ascontiguousarray(arr, dtype=np.float32).ravel()
            pad = (-cur) % 4                      # keep every tensor 16-byte aligned (float4 loads)
            if pad:
                chunks.append(np.zeros(pad, np.float32))
                cur += pad
            off[key] = cur
            chunks.append(a)
            cur += a.size

        for name, w in sd.items():
            if name == 'sigmas':
                continue
            if name.endswith('.weight') and w.ndim == 4 and name not in ('begin_conv.weight', 'end_conv.weight'):
                # only the forms the selected multiplier consumes (a 128 -> 128 layer is 0.6 MB per fp32 form)
                if self.conv_mode == 'f32':
                    add(name, pack_conv_weight(w))
                    if w.shape[2:] == (3, 3):
                        add(name + '#winograd', pack_conv_weight_winograd(w))
                elif self.conv_mode == 'bf16x3':
                    add(name + '#split', pack_conv_weight_split(w).view(np.float32))      # bf16 bit patterns
                    if w.shape[2:] == (3, 3):
                        add(name + '#winograd_split', pack_conv_weight_winograd_split(w).view(np.float32))
                elif self.conv_mode == 'f16x2':
                    add(name + '#split', pack_conv_weight_f16x2(w).view(np.float32))      # 2 fp16 terms + scale trailer
                    if w.shape[2:] == (3, 3):
                        add(name + '#winograd_split', pack_conv_weight_winograd_f16x2(w).view(np.float32))
                    if name.endswith('.conv.weight'):
                        # a ConvMeanPool layer (layers.py:291-313): also the pooled stride-2 filter SBC_OP_CONV_DOWN reads
                        add(name + '#pool', pack_conv_weight_pooled_f16x2(w).view(np.float32))
                else:
                    add(name + '#split', pack_conv_weight_f16(w).view(np.float32))        # fp16 bit patterns
                    if w.shape[2:] == (3, 3):
                        add(name + '#winograd_split', pack_conv_weight_winograd_f16(w).view(np.float32))
            elif name.endswith('.alpha'):
                pre = name[:-len('.alpha')]
                add(pre, np.concatenate([sd[pre + '.alpha'], sd[pre + '.gamma'], sd[pre + '.beta']]))
            elif name.endswith('.gamma') or name.endswith('.beta'):
                continue
            else:
                add(name, w)
        self._wdev = torch.from_numpy(np.concatenate(chunks)).to(self.device)
        self._woff = off
        self._call_cache.clear()
        self._plans.clear()
        self._sd_host = {k: v for k, v in state_dict.items()}
        self._calibrated = False
        self._fallback = None
        return self

    def _ensure_calibrated(self, nt=None, nr=None):
        """conv_mode f16x2: one pass over the library's fixed calibration input sets every layer's activation scale
        (``sbc_f16x2_calibrate``, include/sbc_hip.h) -- once per loaded checkpoint, before anything else uses the weights, ALWAYS
        at the array size of the checkpoint's configuration (``config.data.image_size`` = [Nr, Nt], train_score.py:60), whatever
        size is bound first, and into EVERY packed form of every layer (direct and Winograd).  Input and size are fixed, so the
        scales -- and with them every later result -- depend on the checkpoint only: not on the data, the batch, or the order in
        which array sizes are bound in the process."""
        if self.conv_mode != 'f16x2' or self._calibrated or self._calibrating or os.environ.get('SBC_NO_CALIB'):   # (env: A/B aid, scales stay 1)
            return
        nr0, nt0 = (int(v) for v in self.config.data.image_size[:2])
        if nt0 % 8 or nr0 % 8:                        # (a configuration the kernels cannot run: fall back to the size being bound)
            nt0, nr0 = nt, nr
        self._calibrating = True                      # (bind below comes back here)
        try:
            b = self.bind(1, nt0, nr0)
            b.x.view(-1).copy_(torch.from_numpy(_lib.calibration_input(nt0 * nr0 * self.channels)))
            with torch.cuda.device(self.device):
                _lib.calibrate_f16x2(b.ops, torch.cuda.current_stream(self.device).cuda_stream)
            self._calibrated = True                   # only now: a failed pass is retried by the next bind
        finally:
            self._calibrating = False

    def fallback_net(self):
        """The same checkpoint in ``bf16x3`` (fp32's range and precision everywhere): what a batch that raised the f16x2 range
        flag is run again with (``driver.run_trajectories``); built on first use."""
        if self._fallback is None:
            if self._sd_host is None:
                raise RuntimeError('load_state_dict() must be called before fallback_net()')
            self._fallback = ScoreNet(self.config, self.device, conv_mode='bf16x3', overlap=self.overlap,
                                      fold_stats=self.fold_stats).load_state_dict(self._sd_host, strict=False)
        return self._fallback

    def fallback_plan_slot_elems(self, nt, nr):
        """Activation-slot elements per trajectory of the ``bf16x3`` plan a flagged batch is re-run with (unfused: more slots than
        the fused f16x2 plan) -- ``driver.batch_limit`` sizes chunks for the larger of the two.  Builds no device state."""
        key = ('fallback', nt, nr)
        if key not in self._plans:
            self._plans[key] = sum(P.build_score_plan(self.ngf, nt, nr, self.channels, overlap=self.overlap, fold_stats=self.fold_stats,
                                                      conv_mode='bf16x3').slot_elems)
        return self._plans[key]

    # --- binding ----------------------------------------------------------------------------------
    def skip_overlap_for(self, B, nt, nr):
        """Does a batch of ``B`` ``nt x nr`` arrays take the plan with the skip branches on their own launch lanes?  (``B`` None: no.)"""
        if B is None or self.overlap or not self.skip_overlap:
            return False
        return B * nt * nr <= 1024 * SKIP_OVERLAP_MAX_T

    def score_plan(self, nt, nr, B=None, lanes=None):
        """The launch plan of one score evaluation at ``nt x nr``; ``B`` (the batch it will be bound for) selects the small-batch
        variant with launch lanes (same records, other order; ``skip_overlap_for``) unless ``lanes`` says so explicitly."""
        skip = self.skip_overlap_for(B, nt, nr) if lanes is None else (bool(lanes) and bool(self.skip_overlap) and not self.overlap)
        key = (nt, nr, skip)
        if key not in self._plans:
            # (what the array size and the multiplier rule out of these switches -- folded statistics off powers of two, the pair shapes
            # of 'f16w' -- is the wiring's decision, conv_mode tells it)
            self._plans[key] = P.build_score_plan(self.ngf, nt, nr, self.channels, overlap=self.overlap, fold_stats=self.fold_stats,
                                                  fuse_pairs=self.fuse_pairs, fuse_res=self.fuse_res, fuse_chain=self.fuse_chain and not self.overlap,
                                                  fuse_down=self.fuse_down and not self.overlap, fuse_end=self.fuse_end,
                                                  skip_overlap=(self.skip_overlap if skip else None), conv_mode=self.conv_mode)
        return self._plans[key]

    def bind(self, B, nt, nr, *, step=None, sigma_of_step=None, use_labels=True, lanes=None):
        """Allocate buffers for batch ``B`` and have the library bind the plan's records to them and to the packed weights
        (``sbc_score_wiring_bind``).  ``lanes``: take the plan with launch lanes (True) or the sequential one (False); default: by
        batch size (``skip_overlap_for``) -- a caller that runs several sub-batches side by side passes False (``driver.stream_count``).
        Noise level source of the end conv: per-sample ``labels`` (module-call semantics) or the device step
        counter + ``sigma_of_step`` table (inside an ALD plan)."""
        if self._wdev is None:
            raise RuntimeError('load_state_dict() must be called before the network is used')
        self._ensure_calibrated(nt, nr)
        pl = self.score_plan(nt, nr, None if self._calibrating else B, lanes=False if self._calibrating else lanes)
        dev = self.device
        slots = [torch.empty(B * e, dtype=torch.float32, device=dev) for e in pl.slot_elems]
        labels = torch.zeros(B, dtype=torch.int64, device=dev) if use_labels else None
        ext = _lib.sbc_endconv(sigmas=_ptr(self.sigmas),
                               labels=_ptr(labels) if use_labels else None,
                               sigma_of_step=_ptr(sigma_of_step) if sigma_of_step is not None else None,
                               step=_ptr(step) if step is not None else None)
        if self._params is None or self._params[0] is not self._wdev:
            # what load_state_dict packed, by name (the keys of _woff), for the library's binder: once per loaded state dict
            names, base = [k.encode() for k in self._woff], self._wdev.data_ptr()
            table = (_lib.sbc_named_ptr * len(names))(*[_lib.sbc_named_ptr(n, base + 4 * off) for n, off in zip(names, self._woff.values())])
            self._params = (self._wdev, table, names)
        table = self._params[1]
        # which form goes into which field of which record: csrc/score_wire.cpp (sbc_score_wiring_bind), the same call a C host's records come from
        ops, chains = (_lib.sbc_op * len(pl.ops))(), (_lib.sbc_chain * pl.wiring.n_chains)()
        desc = _lib.sbc_score_bind_desc(batch=B, conv_mode=_lib.CONV_MODE_IDS[self.conv_mode], slots=(C.c_void_p * len(slots))(*[t.data_ptr() for t in slots]),
                                        n_slots=len(slots), params=table, n_params=len(table), endconv=C.pointer(ext))
        _lib.check(_lib.lib().sbc_score_wiring_bind(pl.wiring.handle, C.byref(desc), ops, chains))
        x = slots[pl.x.slot].view(B, nt, nr, self.channels)
        out = slots[pl.out.slot].view(B, nt, nr, self.channels)
        return BoundScore(list(ops), x, out, slots, labels, [ext, self._wdev, self.sigmas, sigma_of_step, step, (ops, chains)], plan=pl)

    # --- module call --------------------------------------------------------------------------------
    def __call__(self, x, labels):
        """``diffuser(current_real, labels)`` (test_score.py:151).  ``x``: float32 ``[B, 2, Nt, Nr]`` (any
        strides; the permuted ``view_as_real`` of the reference is consumed without a copy kernel beyond the
        one staging copy), ``labels``: integer ``[B]``.  Returns a fresh ``[B, 2, Nt, Nr]`` tensor (channels-last strides).

        Non-finite inputs: the reference's ``F.instance_norm`` spreads a NaN / Inf of a sample over that sample's whole score; the
        fused kernels' ``max``-based ELU and pooling would swallow a NaN instead, so samples whose input is not finite are answered
        with NaN here (one small reduction on this non-hot path).  Inside the Langevin plan no such step is needed: a non-finite
        estimate X stays non-finite through the update kernel and shows in the NMSE log, as in the reference."""
        if x.dim() != 4 or x.shape[1] != self.channels:
            raise ValueError('expected x of shape [B, %d, Nt, Nr], got %s' % (self.channels, tuple(x.shape)))
        B, _, nt, nr = x.shape
        key = (B, nt, nr)
        if key not in self._call_cache:
            bound = self.bind(B, nt, nr)
            self._call_cache[key] = (bound, _lib.Plan(bound.ops, keepalive=bound))
        bound, plan = self._call_cache[key]
        bound.x.copy_(x.to(self.device, torch.float32).permute(0, 2, 3, 1))
        bound.labels.copy_(labels.to(self.device).long())
        plan.run(torch.cuda.current_stream(self.device).cuda_stream)
        out = bound.out.permute(0, 3, 1, 2).clone()
        bad = ~torch.isfinite(bound.x).view(B, -1).all(dim=1)
        if bool(bad.any()):
            out[bad] = float('nan')
        if self.conv_mode == 'f16x2':
            # (waits for every stream of the device; the module-call path is not the hot loop)
            bits = _lib.range_flag(True, self.device)
            if bits:
                # outside the window in which the two-term split is fp32-class: the same call in bf16x3, in this process
                self.range_fallbacks += 1
                self.last_range_bits = bits
                return self.fallback_net()(x, labels)
        return out

    forward = __call__
