"""The self-sufficient C boundary (``sbc_score_*``, include/sbc_hip.h): a host that is not Python gets the whole score
network from the checkpoint tensors in one call.  Both hosts take their records from the library's one wiring and one binder
(csrc/score_wire.cpp; tests/test_plan_golden_cpu.py and tests/test_bind_golden_cpu.py hold them); what is held to the Python host
(scorenet.py) here is the rest of ``sbc_score_create`` -- the gates it puts in front of the wiring, weight packing, the choice of
forms it packs, calibration: identical operator records, bit-identical outputs, and a full Langevin-step plan composed from
``sbc_score_ops``.  ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

MODES = {'bf16x3': 0, 'f32': 1, 'f16w': 2, 'f16x2': 3}


def _create(sd, cfg, B, nt, nr, mode, pairs=False, fold=False, res=False, chain=False, down=False, end=False, lanes=False):
    from score_based_channels_amd import _lib
    refs, keep = _lib.tensor_refs(sd, [k for k in sd if k != 'sigmas'])
    sig = np.ascontiguousarray(sd['sigmas'], np.float32)
    desc = _lib.sbc_score_desc(ngf=32, channels=2, nt=nt, nr=nr, batch=B, conv_mode=MODES[mode], sigmas=sig.ctypes.data,
                               num_classes=sig.size, flags=(1 if pairs else 0) | (2 if fold else 0) | (4 if res else 0) | (8 if chain else 0) | (16 if down else 0) | (32 if end else 0) | (64 if lanes else 0))
    h = C.c_void_p()
    _lib.check(_lib.lib().sbc_score_create(C.byref(desc), refs, len(refs), C.byref(h)))
    return h


@pytest.mark.parametrize('mode', ['bf16x3', 'f32', 'f16w', 'f16x2', 'f16x2+pairs', 'f16w+pairs', 'f16x2+pairs+fold', 'bf16x3+fold',
                                  'f16x2+pairs+fold+res', 'f16x2+pairs+fold+res+chain', 'f16x2+pairs+fold+res+chain+down', 'f16x2+pairs+fold+res+chain+down+end',
                                  'bf16x3+end', 'f16x2+pairs+fold+res+chain+down+end+lanes', 'bf16x3+lanes'])
def test_c_built_score_network_equals_python_host(weights64, mode):
    import torch
    from score_based_channels_amd import _lib
    from score_based_channels_amd.scorenet import ScoreNet
    cfg, sd = weights64
    L = _lib.lib()
    B, nt, nr = 3, 64, 16
    mode, *opts = mode.split('+')
    pairs, fold, res, chain, down, end = 'pairs' in opts, 'fold' in opts, 'res' in opts, 'chain' in opts, 'down' in opts, 'end' in opts
    lanes = 'lanes' in opts                 # SBC_SCORE_SKIP_LANES: the skip branches on launch lane 1
    h = _create(sd, cfg, B, nt, nr, mode, pairs, fold, res, chain, down, end, lanes)
    try:
        ops_p, n = C.POINTER(_lib.sbc_op)(), C.c_int32()
        _lib.check(L.sbc_score_ops(h, C.byref(ops_p), C.byref(n)))
        net = ScoreNet(cfg, conv_mode=mode, fuse_pairs=pairs, fold_stats=fold, fuse_res=res, fuse_chain=chain, fuse_down=down, fuse_end=end).cuda().load_state_dict(sd)
        # (record for record against the plan the flags ask for: sequential, or -- SBC_SCORE_SKIP_LANES -- with the skip branches on a launch
        # lane; the forward below runs whatever the Python host picks for a batch this small and must agree bit for bit either way)
        bound = net.bind(B, nt, nr, lanes=lanes)
        assert lanes == any(o.lane for o in bound.ops)
        assert n.value == len(bound.ops)
        assert chain == any(o.kind == 24 for o in bound.ops) and down == any(o.kind == 25 for o in bound.ops)
        # identical records: every scalar field, and the same storage-sharing pattern (pointers renamed by first use)
        ids_c, ids_p = {}, {}
        for i, ref in enumerate(bound.ops):
            got = ops_p[i]
            for f in ('kind', 'flags', 'B', 'H', 'W', 'cin', 'cout', 'ksize', 'dil', 'up_h', 'up_w', 'tag', 'lane', 'signal'):
                assert getattr(got, f) == getattr(ref, f), (i, f)
            assert list(got.wait) == list(ref.wait), (i, 'wait')
            for f in ('in_', 'out', 'stats', 'res1', 'res2', 'up', 'aux'):
                a, b = getattr(got, f), getattr(ref, f)
                assert (a is None) == (b is None), (i, f)
                if a is not None:
                    assert ids_c.setdefault(a, len(ids_c)) == ids_p.setdefault(b, len(ids_p)), (i, f)
            for f in ('weight', 'bias', 'weight_wino', 'weight_split', 'weight2_split', 'bias2', 'norm2'):
                if ref.kind == 25 and f in ('weight', 'weight_wino'):
                    # SBC_OP_CONV_DOWN: calibration-only pointers at the layers' UNPOOLED forms, which the Python host packs for other
                    # array sizes and a C handle (one size, only the forms it runs) does not have (include/sbc_hip.h)
                    assert getattr(got, f) is None
                    continue
                assert (getattr(got, f) is None) == (getattr(ref, f) is None), (i, f)
            if ref.kind == 24:                      # SBC_OP_CHAIN: the same blocks in the same order
                cg, cr = C.cast(got.ext, C.POINTER(_lib.sbc_chain)).contents, C.cast(ref.ext, C.POINTER(_lib.sbc_chain)).contents
                assert cg.n_blocks == cr.n_blocks and list(cg.type)[:cg.n_blocks] == list(cr.type)[:cr.n_blocks]
                assert all(cg.w1[k] and cg.w2[k] and cr.w1[k] and cr.w2[k] for k in range(cg.n_blocks))
            elif ref.kind == 3:                     # (fused records carry the Winograd forms for the calibration only where the host packed them)
                assert (got.weight_wino_split is None) == (ref.weight_wino_split is None), (i, 'weight_wino_split')
        # bit-identical forward
        g = load_golden('forward_64x16.npz')
        x = torch.from_numpy(g['x'][:B]).cuda()
        labels = torch.tensor([0, 1155, 2310], dtype=torch.long, device='cuda')
        want = net(x, labels)
        px, po, pl = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(L.sbc_score_buffers(h, C.byref(px), C.byref(po), C.byref(pl)))
        xin = x.permute(0, 2, 3, 1).contiguous()
        hip = torch.cuda.current_stream().cuda_stream
        out = torch.empty(B, nt, nr, 2, device='cuda')
        lib_rt = C.CDLL('libamdhip64.so')
        lib_rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        torch.cuda.synchronize()
        assert lib_rt.hipMemcpy(px, C.c_void_p(xin.data_ptr()), xin.numel() * 4, 3) == 0            # device to device
        assert lib_rt.hipMemcpy(pl, C.c_void_p(labels.data_ptr()), B * 8, 3) == 0
        _lib.check(L.sbc_score_forward(h, C.c_void_p(hip)))
        torch.cuda.synchronize()
        assert lib_rt.hipMemcpy(C.c_void_p(out.data_ptr()), po, out.numel() * 4, 3) == 0
        assert torch.equal(out.permute(0, 3, 1, 2), want)
    finally:
        L.sbc_score_destroy(h)


@pytest.mark.parametrize('mode,pairs,fold,chain', [('bf16x3', False, False, False), ('f16x2', True, True, False), ('f16x2', True, True, True)])
def test_langevin_plan_composed_from_c_records(weights64, mode, pairs, fold, chain):
    """sbc_score_level_source + sbc_score_ops + SBC_OP_LANGEVIN + SBC_OP_STEP_INC = the plan AldBatch builds: same NMSE log --
    in the exact mode and in the shipped default (conv_mode 3 | SBC_SCORE_FUSE_PAIRS | SBC_SCORE_FOLD_STATS, calibrated scales)."""
    import torch
    from score_based_channels_amd import _lib, plan as P
    from score_based_channels_amd.ald import AldBatch, schedule_tables, snr_to_noise
    from score_based_channels_amd.noise import HostNoise
    from score_based_channels_amd.scorenet import ScoreNet
    cfg, sd = weights64
    L = _lib.lib()
    g = load_golden('ald_plumbing_3levels.npz')
    H, Pm = g['H'], g['P']
    B, nt, nr = H.shape
    npil = Pm.shape[1]
    levels, n_steps = [0, 1, 2], 9
    noise = HostNoise(int(g['seed']))
    ln = float(snr_to_noise(g['snr_db'], nt)[0])
    steps = noise.step_block(0, H.shape, n_steps)
    # reference run through the Python host
    net = ScoreNet(cfg, conv_mode=mode, fold_stats=fold, fuse_pairs=pairs, fuse_res=False, fuse_chain=chain, fuse_down=False, fuse_end=False).cuda().load_state_dict(sd)
    ald = AldBatch(net, H, Pm, np.arange(B), np.arange(B), ln, levels=levels, step_noise=torch.from_numpy(steps))
    ald.set_init(torch.from_numpy(noise.init(H.shape)))
    Y = ald.synthesize_measurements(torch.from_numpy(noise.measurement(0, (B, npil, nr)))).clone()
    ald.run()
    torch.cuda.synchronize()
    want = ald.nmse_log().clone()
    # the same plan from C records
    h = _create(sd, cfg, B, nt, nr, mode, pairs, fold, False, chain)
    try:
        sched, sig = schedule_tables(sd['sigmas'], cfg.model.sigma_end, levels, 3, [3e-11], [0.01], [ln])
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(
            sched=sched, sig=sig, H=H.view(np.float32), P=Pm.view(np.float32), nz=steps.view(np.float32)).items()}
        step = torch.zeros(1, dtype=torch.int32, device='cuda')
        nm = torch.zeros(n_steps, B, device='cuda')
        _lib.check(L.sbc_score_level_source(h, C.c_void_p(dev['sig'].data_ptr()), C.c_void_p(step.data_ptr())))
        ops_p, n = C.POINTER(_lib.sbc_op)(), C.c_int32()
        _lib.check(L.sbc_score_ops(h, C.byref(ops_p), C.byref(n)))
        px, po = C.c_void_p(), C.c_void_p()
        _lib.check(L.sbc_score_buffers(h, C.byref(px), C.byref(po), None))
        ext = _lib.sbc_langevin(X=px, score=po, P=dev['P'].data_ptr(), Y=torch.view_as_real(Y).data_ptr(),
                                Htrue=dev['H'].data_ptr(), sched=dev['sched'].data_ptr(), noise=dev['nz'].data_ptr(),
                                nmse=nm.data_ptr(), step=step.data_ptr(), n_steps=n_steps, Nt=nt, Nr=nr, Np=npil)
        recs = [ops_p[i] for i in range(n.value)]
        recs.append(_lib.sbc_op(kind=P.LANGEVIN, B=B, ext=C.cast(C.pointer(ext), C.c_void_p)))
        recs.append(_lib.sbc_op(kind=P.STEP_INC, B=1, out=step.data_ptr()))
        plan = _lib.Plan(recs)
        x0 = torch.view_as_real(torch.from_numpy(noise.init(H.shape)).cuda()).contiguous()
        lib_rt = C.CDLL('libamdhip64.so')
        lib_rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        torch.cuda.synchronize()
        assert lib_rt.hipMemcpy(px, C.c_void_p(x0.data_ptr()), x0.numel() * 4, 3) == 0
        plan.run(torch.cuda.current_stream().cuda_stream, n_steps)
        torch.cuda.synchronize()
        assert torch.equal(nm, want)
        assert np.max(np.abs(nm.cpu().numpy() / g['nmse_log'][0] - 1)) < 1e-5
        plan.close()
    finally:
        L.sbc_score_destroy(h)


def test_score_create_reports_missing_tensors(weights64):
    from score_based_channels_amd import _lib
    cfg, sd = weights64
    bad = {k: v for k, v in sd.items() if k != 'refine3.msf.convs.1.bias'}
    with pytest.raises(_lib.SbcError, match='refine3.msf.convs.1.bias'):
        _create(bad, cfg, 2, 64, 16, 'bf16x3')


def test_plan_refuses_inconsistent_lanes():
    """sbc_plan_create validates the launch-lane fields of its records (ABI 14): a lane beyond SBC_MAX_LANES, an event id beyond
    SBC_MAX_EVENTS, a wait for an event no EARLIER record signals, lanes mixed with the SBC_OP_SIDE / SBC_OP_JOIN flags -- all refused
    with a message, none of them a hang at run time."""
    import torch
    from score_based_channels_amd import _lib, plan as P
    x = torch.zeros(2, 8, 8, 2, device='cuda')
    y = torch.zeros(1, dtype=torch.int32, device='cuda')

    def inc(**kw):
        return _lib.sbc_op(kind=P.STEP_INC, B=1, out=C.c_void_p(y.data_ptr()), **kw)
    ok = _lib.Plan([inc(signal=1), inc(lane=1, wait=(C.c_int32 * 2)(1, 0), signal=2), inc(wait=(C.c_int32 * 2)(2, 0))])
    ok.run(torch.cuda.current_stream().cuda_stream, 3)
    torch.cuda.synchronize()
    assert int(y.item()) == 9
    ok.close()
    for bad, what in (([inc(lane=4)], 'lane out of range'), ([inc(signal=65)], 'signal id out of range'),
                      ([inc(wait=(C.c_int32 * 2)(1, 0)), inc(signal=1)], 'no earlier record signals'),
                      ([inc(signal=1), inc(lane=1, flags=P.OP_SIDE, wait=(C.c_int32 * 2)(1, 0))], 'do not mix')):
        with pytest.raises(_lib.SbcError, match=what):
            _lib.Plan(bad)
    del x


# ---- the classical baselines (sbc_l1_lifted_run, sbc_ls_regularized) through the raw ABI: descriptors filled by hand from torch
# device pointers, so that the library's own checks are reached (baselines.py refuses bad input on the host first)

OK, INVALID, UNSUPPORTED = 0, -1, -3
SENTINEL = 7.0


class _Case:
    """Device tensors of B problems (QPSK pilots, Gaussian channels: cs_checks.ls_problem) and the two descriptors over them.
    ``spare``: that many extra matrices in front of and behind the nP / nH the descriptor declares (the descriptor's P / Htrue
    point at the first declared one), so that the indices -1 and nP / nH stay inside the allocation."""

    def __init__(self, B, npil, nt=64, nr=16, L=2, steps=5, nP=None, nH=None, spare=0, seed=3):
        import torch
        import cs_checks as K
        nP, nH = nP or B, nH or B
        P, _, H, _, _, noise = K.ls_problem(npil, nt, nr, seed, B=B, nP=nP + 2 * spare, nH=nH + 2 * spare, noises=(0.1, 1.0))
        self.B, self.nP, self.nH, self.nt, self.nr, self.npil, self.L, self.steps, self.spare = B, nP, nH, nt, nr, npil, L, steps, spare
        self.pidx_np, self.hidx_np = np.arange(B) % nP, (np.arange(B) + 1) % nH
        rng = np.random.default_rng(seed)
        z = rng.standard_normal((B, npil, nr)) + 1j * rng.standard_normal((B, npil, nr))
        Y = (P[spare + self.pidx_np] @ H[spare + self.hidx_np] + 0.2 * z).astype(np.complex64)   # of the DECLARED matrices
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.P, self.Y, self.H = dev(P), dev(Y), dev(H)
        self.pidx, self.hidx = dev(self.pidx_np.astype(np.int32)), dev(self.hidx_np.astype(np.int32))
        self.lam, self.lr, self.nv = dev(np.full(B, 0.3, np.float32)), dev(np.full(B, 3e-3, np.float32)), dev(noise.astype(np.float32))
        self.fresh()

    def fresh(self):
        import torch
        full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device='cuda')
        self.log, self.nmse = full(self.steps, self.B), full(self.B)
        self.Hh, self.X = full(self.B, self.nt, self.nr, 2), full(self.B, self.L * self.nt, self.L * self.nr, 2)
        return self

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in (self.log, self.nmse, self.Hh, self.X))

    def _base(self, t):
        return t.data_ptr() + self.spare * t[0].numel() * 8

    def l1(self, **over):
        from score_based_channels_amd import _lib
        f = dict(P=self._base(self.P), p_index=self.pidx.data_ptr(), Y=self.Y.data_ptr(), Htrue=self._base(self.H),
                 h_index=self.hidx.data_ptr(), lmbda=self.lam.data_ptr(), lr=self.lr.data_ptr(), nmse=self.log.data_ptr(),
                 H_hat=self.Hh.data_ptr(), X=self.X.data_ptr(), B=self.B, nP=self.nP, nH=self.nH, Nt=self.nt, Nr=self.nr, Np=self.npil,
                 lifting=self.L, steps=self.steps)
        f.update(over)
        return _lib.sbc_l1_lifted_desc(**f)

    def ls(self, **over):
        from score_based_channels_amd import _lib
        f = dict(P=self._base(self.P), p_index=self.pidx.data_ptr(), Y=self.Y.data_ptr(), noise_var=self.nv.data_ptr(),
                 Htrue=self._base(self.H), h_index=self.hidx.data_ptr(), H_hat=self.Hh.data_ptr(), nmse=self.nmse.data_ptr(), B=self.B,
                 nP=self.nP, nH=self.nH, Nt=self.nt, Nr=self.nr, Np=self.npil)
        f.update(over)
        return _lib.sbc_ls_desc(**f)


def _call(fn, desc, stream=None):
    """(status, sbc_last_error text) of one call on ``stream`` (default: torch's current stream), synchronised"""
    import torch
    from score_based_channels_amd import _lib
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = getattr(_lib.lib(), fn)(C.byref(desc) if desc is not None else None, C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc, _lib.lib().sbc_last_error().decode()


def _bits(*tensors):
    return b''.join(t.cpu().numpy().tobytes() for t in tensors)


L1_REFUSALS = [(dict(Nt=32), UNSUPPORTED, 'Nt=32'), (dict(Nr=8), UNSUPPORTED, 'Nr=8'), (dict(lifting=3), UNSUPPORTED, 'lifting=3'),
               (dict(Np=0), UNSUPPORTED, 'Np=0'), (dict(Np=65), UNSUPPORTED, 'Np=65'), (dict(steps=0), INVALID, 'steps=0'),
               (dict(nP=0), INVALID, 'nP=0'), (dict(nH=0), INVALID, 'nH=0'), (dict(B=-1), INVALID, 'B=-1')] + \
              [({k: None}, INVALID, 'NULL %s' % k) for k in ('P', 'Y', 'Htrue', 'lmbda', 'lr', 'nmse')]
LS_REFUSALS = [(dict(Nr=65), UNSUPPORTED, 'Nr=65'), (dict(Np=65, Nt=65), UNSUPPORTED, 'Np=65'), (dict(Nt=1025), UNSUPPORTED, 'Nt=1025'),
               (dict(Np=1025), UNSUPPORTED, 'Np=1025'), (dict(Nt=0), UNSUPPORTED, 'Nt=0'), (dict(Htrue=None), INVALID, 'nmse needs Htrue'),
               (dict(nP=0), INVALID, 'nP=0'), (dict(nH=0), INVALID, 'nH=0'), (dict(B=-1), INVALID, 'B=-1')] + \
              [({k: None}, INVALID, 'NULL %s' % k) for k in ('P', 'Y', 'noise_var', 'H_hat')]


@pytest.mark.parametrize('fn,table', [('sbc_l1_lifted_run', L1_REFUSALS), ('sbc_ls_regularized', LS_REFUSALS)])
def test_baseline_calls_refuse_what_the_header_excludes(fn, table):
    """Each refusal of the library itself: its status code, a message that names the function and the offending value, and no
    output buffer written (they hold a sentinel)."""
    c = _Case(4, 38)
    make = c.l1 if fn == 'sbc_l1_lifted_run' else c.ls
    for over, status, text in table:
        rc, msg = _call(fn, make(**over))
        assert rc == status and fn in msg and text in msg, (over, rc, msg)
        assert c.untouched(), over
    rc, msg = _call(fn, None)
    assert rc == INVALID and fn in msg and 'NULL descriptor' in msg
    # B = 0: fine, and nothing launched
    rc, _ = _call(fn, make(B=0))
    assert rc == OK and c.untouched()
    # and the same descriptor unmodified runs
    rc, msg = _call(fn, make())
    assert rc == OK, msg
    assert not c.untouched()


@pytest.mark.parametrize('L', [1, 2, 4])
def test_l1_call_optional_outputs_and_index_maps(L):
    """H_hat = NULL, X = NULL, both: the log has the same bits and the output that is given too; p_index / h_index = NULL with
    nP = nH = B is the identity map."""
    c = _Case(5, 25, L=L, steps=6)
    ident = np.arange(5, dtype=np.int32)
    import torch
    c.pidx, c.hidx = torch.from_numpy(ident).cuda(), torch.from_numpy(ident).cuda()
    assert _call('sbc_l1_lifted_run', c.l1())[0] == OK
    log, Hh, X = _bits(c.log), _bits(c.Hh), _bits(c.X)
    assert np.all(np.isfinite(c.log.cpu().numpy()))
    for over in (dict(H_hat=None), dict(X=None), dict(H_hat=None, X=None), dict(p_index=None), dict(h_index=None),
                 dict(p_index=None, h_index=None)):
        c.fresh()
        rc, msg = _call('sbc_l1_lifted_run', c.l1(**over))
        assert rc == OK, msg
        assert _bits(c.log) == log, over
        assert bool((c.Hh == SENTINEL).all()) if 'H_hat' in over else _bits(c.Hh) == Hh, over
        assert bool((c.X == SENTINEL).all()) if 'X' in over else _bits(c.X) == X, over


@pytest.mark.parametrize('npil,nt,nr', [(25, 64, 16), (70, 33, 5)])
def test_ls_call_optional_outputs_and_index_maps(npil, nt, nr):
    """Htrue = nmse = NULL: the same H_hat bits, nmse untouched; NULL index maps with nP = nH = B are the identity."""
    import torch
    c = _Case(6, npil, nt, nr)
    ident = np.arange(6, dtype=np.int32)
    c.pidx, c.hidx = torch.from_numpy(ident).cuda(), torch.from_numpy(ident).cuda()
    assert _call('sbc_ls_regularized', c.ls())[0] == OK
    Hh, nmse = _bits(c.Hh), _bits(c.nmse)
    assert np.all(np.isfinite(c.nmse.cpu().numpy())) and np.all(np.isfinite(c.Hh.cpu().numpy()))
    for over in (dict(Htrue=None, h_index=None, nmse=None, nH=0), dict(nmse=None), dict(p_index=None), dict(h_index=None),
                 dict(p_index=None, h_index=None)):
        c.fresh()
        rc, msg = _call('sbc_ls_regularized', c.ls(**over))
        assert rc == OK, msg
        assert _bits(c.Hh) == Hh, over
        assert bool((c.nmse == SENTINEL).all()) if 'nmse' in over else _bits(c.nmse) == nmse, over


def test_baseline_calls_on_a_callers_stream():
    """A non-default stream: the same bits as on the default stream once that stream is synchronised."""
    import torch
    c = _Case(6, 51, L=4, steps=8)
    assert _call('sbc_l1_lifted_run', c.l1())[0] == OK
    want_l1 = _bits(c.log, c.Hh, c.X)
    c.fresh()
    assert _call('sbc_ls_regularized', c.ls())[0] == OK
    want_ls = _bits(c.Hh, c.nmse)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    c.fresh()
    torch.cuda.synchronize()
    assert _call('sbc_l1_lifted_run', c.l1(), side)[0] == OK
    assert _bits(c.log, c.Hh, c.X) == want_l1
    c.fresh()
    torch.cuda.synchronize()
    assert _call('sbc_ls_regularized', c.ls(), side)[0] == OK
    assert _bits(c.Hh, c.nmse) == want_ls


def test_baseline_calls_mark_out_of_range_indices_with_nan():
    """include/sbc_hip.h: an index outside [0, nP) / [0, nH) gives that problem a NaN log (l1) / nmse (ML) and NaN H_hat / X,
    reads nothing through the bad index and leaves every other problem as it is.  Both kernels test ``idx < 0 || idx >= n``
    before forming any address from it (cs_l1.hip, cs_ls.hip: first statement after the index loads).  The case is safe even
    against a wrong guard: P and H hold one spare matrix in front of and behind the declared ones, and only -1 and nP / nH are
    used.  One launch per solver."""
    import torch
    c = _Case(8, 38, L=2, steps=5, nP=4, nH=4, spare=1)
    assert _call('sbc_l1_lifted_run', c.l1())[0] == OK
    log, Hh, X = c.log.cpu().numpy(), c.Hh.cpu().numpy(), c.X.cpu().numpy()
    c.fresh()
    assert _call('sbc_ls_regularized', c.ls())[0] == OK
    lsH, lsn = c.Hh.cpu().numpy(), c.nmse.cpu().numpy()
    assert np.all(np.isfinite(log)) and np.all(np.isfinite(lsn))
    pb, hb = c.pidx_np.astype(np.int32), c.hidx_np.astype(np.int32)
    pb[1], pb[3], hb[4], hb[6] = -1, c.nP, -1, c.nH
    bad, good = [1, 3, 4, 6], [0, 2, 5, 7]
    c.pidx, c.hidx = torch.from_numpy(pb).cuda(), torch.from_numpy(hb).cuda()
    c.fresh()
    assert _call('sbc_l1_lifted_run', c.l1())[0] == OK
    log1, Hh1, X1 = c.log.cpu().numpy(), c.Hh.cpu().numpy(), c.X.cpu().numpy()
    assert np.all(np.isnan(log1[:, bad])) and np.all(np.isnan(Hh1[bad])) and np.all(np.isnan(X1[bad]))
    assert log1[:, good].tobytes() == log[:, good].tobytes() and Hh1[good].tobytes() == Hh[good].tobytes()
    assert X1[good].tobytes() == X[good].tobytes()
    c.fresh()
    assert _call('sbc_ls_regularized', c.ls())[0] == OK
    lsH1, lsn1 = c.Hh.cpu().numpy(), c.nmse.cpu().numpy()
    assert np.all(np.isnan(lsn1[bad])) and np.all(np.isnan(lsH1[bad]))
    assert lsn1[good].tobytes() == lsn[good].tobytes() and lsH1[good].tobytes() == lsH[good].tobytes()
    # without Htrue the channel map is not looked at: only the bad pilot indices are marked
    c.fresh()
    assert _call('sbc_ls_regularized', c.ls(Htrue=None, nmse=None))[0] == OK
    lsH2 = c.Hh.cpu().numpy()
    assert np.all(np.isnan(lsH2[[1, 3]])) and np.delete(lsH2, [1, 3], axis=0).tobytes() == np.delete(lsH, [1, 3], axis=0).tobytes()
    assert bool((c.nmse == SENTINEL).all())
