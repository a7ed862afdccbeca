"""SBC_OP_MEASURE, SBC_OP_LANGEVIN and SBC_OP_STEP_INC (csrc/ops.hip) on their own -- no network, no weights -- against the
float64 reference of tests/langevin_ref.py, on every path ``launch_langevin`` can pick (the table ``CASES`` there; its coverage is
asserted in tests/test_langevin_cases_cpu.py) and over the whole argument surface: index maps, NULL forms, a step counter above
zero, both in-kernel Philox streams, plans (eager and captured), and every refusal.  ``pytest -m gpu``.

Bounds.  X: norm-wise ``rel_err`` per trajectory; NMSE: relative.  Both against float64, never above the 1e-5 the project holds this
kernel to elsewhere; where a path measured under a quarter of that on the device, the assertion is 4x the worst value measured on the
path (the factor covers a sequential FMA chain against a blocked summation).  With in-kernel noise ``nscale * 4e-6`` is added: the
device's Box-Muller against libm's.  Every test prints what it measured next to the error of the complex64 restatement
(oracle/ald_oracle.py) on the same inputs.

Measured on an MI355X (worst over the tests and cases of a path and their five trajectories; the complex64 restatement's worst
one-step error on the same inputs in brackets), and the bound asserted:
    path                                X                    NMSE                 asserted X / NMSE
    flat, X and P in LDS, 4 col         8.02e-8 (7.40e-8)    1.09e-7 (1.47e-7)    3.21e-7 / 4.36e-7
    flat, X and P in LDS, 1 col         8.56e-8 (8.56e-8)    1.38e-7 (1.43e-7)    3.42e-7 / 5.52e-7
    flat, X in LDS, P global, 4 col     2.28e-7 (9.61e-8)    1.58e-7 (9.85e-8)    9.12e-7 / 6.32e-7    (one step: X 1.44e-7)
    flat, X in LDS, P global, 1 col     8.97e-8 (8.97e-8)    1.56e-7 (1.94e-7)    3.59e-7 / 6.24e-7
    flat, X global, 4 col               1.44e-7 (8.41e-8)    1.71e-7 (1.29e-7)    5.76e-7 / 6.84e-7
    flat, X global, 1 col               9.42e-8 (7.13e-8)    9.41e-8 (9.41e-8)    3.77e-7 / 3.76e-7
    tiled                               1.47e-7 (9.47e-8)    1.98e-7 (1.91e-7)    5.88e-7 / 7.92e-7
    SBC_OP_MEASURE, Y                   2.54e-6 at Nt = 2000 (4.69e-7): a sequential chain of Nt FMAs; asserted 1e-5
The 2.28e-7 is the final X of the three-step plan on 128 x 8 x 77 (each step rounds X to float32; the reference carries float64).
"""
import ctypes as C

import numpy as np
import pytest

import langevin_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

INVALID = -1
SENTINEL = -123456.75                  # exact in float32; around X, Y and nmse, which live inside larger allocations
PAD = 64                               # floats on either side (256 bytes: the payload keeps its 16-byte alignment)
BOUND = 1e-5
# worst (X, NMSE) error measured on the device per path, over every test below that runs it (the table in the docstring); every
# path is under BOUND / 4, so the asserted bound is 4 x the path's own worst
MEASURED = {
    'flat, X and P in LDS, 4 col': (8.02e-8, 1.09e-7), 'flat, X and P in LDS, 1 col': (8.56e-8, 1.38e-7),
    'flat, X in LDS, P global, 4 col': (2.28e-7, 1.58e-7), 'flat, X in LDS, P global, 1 col': (8.97e-8, 1.56e-7),
    'flat, X global, 4 col': (1.44e-7, 1.71e-7), 'flat, X global, 1 col': (9.42e-8, 9.41e-8),
    'tiled': (1.47e-7, 1.98e-7)}
assert set(MEASURED) == {R.path_label(R.dispatch_path(*s)) for s in R.SHAPES}
assert all(v < BOUND / 4 for m in MEASURED.values() for v in m)
X_TOL = {label: min(BOUND, 4 * m[0]) for label, m in MEASURED.items()}
NMSE_TOL = {label: min(BOUND, 4 * m[1]) for label, m in MEASURED.items()}
MEASURE_TOL = BOUND                    # SBC_OP_MEASURE: worst 2.54e-6 (Nt = 2000), not under a quarter of the bound: stays
BOX_MULLER = 4e-6                      # x nscale: device vs libm log / sin / cos in the noise draw (test_gpu_parity.py)
TRAJ_IDS = np.array([11, 2 ** 33 + 1, 5, 0, 7], np.int64)
SEED = 2 ** 63 + 0x5DEECE66D
IDS = dict(ids=lambda s: 'x'.join(map(str, s)))


def _f32(a):
    return np.ascontiguousarray(a).view(np.float32).reshape(-1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(a):
    import torch
    flat = torch.from_numpy(_f32(a).copy())
    buf = torch.full((flat.numel() + 2 * PAD,), SENTINEL, dtype=torch.float32, device='cuda')
    buf[PAD:PAD + flat.numel()] = flat
    return buf


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def _problem(shape, null=(), n_steps=R.N_STEPS, nscale=None):
    """Host side of one batch: the case's seeded inputs, the index maps (or their NULL forms: tables expanded to one entry per
    trajectory, B == nP == nH), the sched table."""
    h = R.make_inputs(shape, n_steps=n_steps)
    h.update(shape=shape, n_steps=n_steps, p_index=R.P_INDEX.copy(), h_index=R.H_INDEX.copy(), group=R.GROUP.copy(),
             sched=R.make_sched(n_steps), traj_id=None, seed=0)
    if 'p_index' in null:
        h['P'], h['p_index'] = h['P'][R.P_INDEX], None
    if 'h_index' in null:
        h['H'], h['h_index'] = h['H'][R.H_INDEX], None
    if 'group' in null:
        h['group'] = None
    if nscale is not None:
        h['sched'][:, :, 2] = nscale
    return h


def _permuted(h, perm):
    g = dict(h)
    for k in ('X', 'S', 'Y', 'mnoise', 'meas_scale', 'p_index', 'h_index', 'group', 'traj_id'):
        if g[k] is not None:
            g[k] = g[k][perm].copy()
    if h['noise'] is not None:
        g['noise'] = h['noise'][:, perm].copy()
    return g


def _per_traj(h, step):
    """P and H of each trajectory and its four sched scalars at ``step``."""
    b = np.arange(R.B)
    P = h['P'][b if h['p_index'] is None else h['p_index']]
    H = h['H'][b if h['h_index'] is None else h['h_index']]
    row = h['sched'][np.zeros(R.B, int) if h['group'] is None else h['group'], step]
    return P, H, row[:, 0], row[:, 1], row[:, 2], row[:, 3]


def _step_noise(h, step):
    """What the kernel adds at ``step``: the replayed slab, or the host-restated Philox stream when ``noise`` is NULL."""
    if h['noise'] is not None:
        return h['noise'][step]
    ids = np.arange(R.B) if h['traj_id'] is None else h['traj_id']
    return R.philox_noise(h['seed'], ids, step, h['shape'][:2])


def _reference(h, step, X=None, Y=None):
    P, H, a, dv, ns, dcb = _per_traj(h, step)
    return R.langevin64(h['X'] if X is None else X, h['S'], P, h['Y'] if Y is None else Y, a, dv, ns, dcb, _step_noise(h, step), H)


def _restatement_errors(h, step, Xref, nref):
    """Error of the complex64 oracle on the same inputs against the float64 reference (printed beside the kernel's)."""
    from oracle import ald_oracle as A
    P, H, a, dv, ns, dcb = _per_traj(h, step)
    nz = _step_noise(h, step)
    ex = en = 0.0
    for b in range(R.B):
        s = slice(b, b + 1)
        Xo = A.langevin_step(h['X'][s], h['S'][s], P[s], h['Y'][s], a[b], dv[b], ns[b], nz[s], dc_boost32=dcb[b] if dcb[b] else None)
        ex, en = max(ex, rel_err(Xo, Xref[s])), max(en, abs(A.nmse(Xo, H[s])[0] / nref[b] - 1))
    return ex, en


class _Device:
    """The batch on the device: X, Y and the NMSE log each inside a larger allocation filled with SENTINEL, the log itself NaN."""

    def __init__(self, h, step=0):
        import torch
        self.h, (self.nt, self.nr, self.np_) = h, h['shape']
        self.X, self.Y = _guarded(h['X']), _guarded(h['Y'])
        self.nmse = _guarded(np.full((h['n_steps'], R.B), np.nan, np.float32))
        self.ro = {k: _dev(_f32(h[k])) for k in ('S', 'P', 'H')}
        self.noise = None if h['noise'] is None else _dev(_f32(h['noise']))
        self.mnoise = _dev(_f32(h['mnoise']))
        self.sched, self.meas_scale = _dev(h['sched']), _dev(h['meas_scale'])
        self.maps = {k: None if h[k] is None else _dev(h[k]) for k in ('p_index', 'h_index', 'group', 'traj_id')}
        self.step = torch.tensor([step], dtype=torch.int32, device='cuda')
        self.before = {k: _bits(v) for k, v in self.ro.items()}
        self.before['Y'] = _bits(self.Y)
        torch.cuda.synchronize()

    @staticmethod
    def _ptr(t, guarded=False):
        return None if t is None else t.data_ptr() + (PAD * 4 if guarded else 0)

    def ext(self, measure=False, **over):
        from score_based_channels_amd import _lib
        p = self._ptr
        f = dict(X=p(self.X, True), score=p(self.ro['S']), P=p(self.ro['P']), p_index=p(self.maps['p_index']), Y=p(self.Y, True),
                 Htrue=p(self.ro['H']), h_index=p(self.maps['h_index']), sched=p(self.sched), group=p(self.maps['group']),
                 noise=p(self.mnoise if measure else self.noise), nmse=p(self.nmse, True), step=p(self.step),
                 traj_id=p(self.maps['traj_id']), meas_scale=p(self.meas_scale) if measure else None, seed=self.h['seed'],
                 n_steps=self.h['n_steps'], Nt=self.nt, Nr=self.nr, Np=self.np_)
        f.update(over)
        return _lib.sbc_langevin(**f)

    def op(self, kind, ext=None, **over):
        from score_based_channels_amd import _lib
        f = dict(kind=kind, B=R.B, ext=None if ext is None else C.cast(C.pointer(ext), C.c_void_p))
        f.update(over)
        o = _lib.sbc_op(**f)
        o._keep = ext
        return o

    def launch(self, kind, **over):
        import torch
        from score_based_channels_amd import _lib, plan as PL
        op = self.op(kind, self.ext(measure=kind == PL.MEASURE, **over))
        _lib.check(_lib.lib().sbc_op_launch(C.byref(op), None))
        torch.cuda.synchronize()

    def x(self):
        return self.X[PAD:-PAD].cpu().numpy().view(np.complex64).reshape(R.B, self.nt, self.nr)

    def y(self):
        return self.Y[PAD:-PAD].cpu().numpy().view(np.complex64).reshape(R.B, self.np_, self.nr)

    def log(self):
        return self.nmse[PAD:-PAD].cpu().numpy().reshape(self.h['n_steps'], R.B)

    def assert_guards_and_inputs(self, y_written=False):
        for name in ('X', 'Y', 'nmse'):
            buf = getattr(self, name)
            assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), 'wrote outside ' + name
        for k, v in self.ro.items():
            assert np.array_equal(_bits(v), self.before[k]), k + ' changed'
        if not y_written:
            assert np.array_equal(_bits(self.Y), self.before['Y']), 'Y changed'


def _check_step(tag, h, dev, step, Xref, nref, extra=0.0, restated=True):
    """X and row ``step`` of the log against the reference, within the bound of the shape's path; prints the figures."""
    label = R.path_label(R.dispatch_path(*h['shape']))
    X, nm = dev.x(), dev.log()[step]
    ex = max(rel_err(X[b], Xref[b]) for b in range(R.B))
    en = float(np.max(np.abs(nm / nref - 1)))
    rx, rn = _restatement_errors(h, step, Xref, nref) if restated else (float('nan'),) * 2
    print('LANGEVIN-ERR %-22s %-16s %-34s X %.2e nmse %.2e | complex64 restatement X %.2e nmse %.2e'
          % (tag, 'x'.join(map(str, h['shape'])), label, ex, en, rx, rn))
    assert np.all(np.isfinite(X)) and ex < X_TOL[label] + extra, (tag, h['shape'], ex)
    assert en < NMSE_TOL[label] + extra, (tag, h['shape'], en)
    return ex, en


# ------------------------------------------------------------------------------------------------ one step, every path
@pytest.mark.parametrize('shape', R.SHAPES, **IDS)
def test_one_step_on_every_path(shape):
    """B = 5 over 3 pilot matrices / 4 channels through p_index / h_index, both sched groups (one with dc_boost = 0), the device
    counter at 1 of n_steps = 3: the sched row, the noise slab (the others are NaN) and the nmse row of step 1, rows 0 and 2
    untouched, the inputs bit-unchanged, and nothing written around X, Y or the log."""
    from score_based_channels_amd import plan as PL
    h = _problem(shape)
    h['noise'][[0, 2]] = np.nan
    dev = _Device(h, step=1)
    dev.launch(PL.LANGEVIN)
    Xref, nref = _reference(h, 1)
    _check_step('one step', h, dev, 1, Xref, nref)
    log = dev.log()
    assert np.all(np.isnan(log[0])) and np.all(np.isnan(log[2]))
    assert int(dev.step.item()) == 1
    dev.assert_guards_and_inputs()


@pytest.mark.parametrize('null', ['group', 'p_index', 'h_index', 'group+p_index+h_index'])
@pytest.mark.parametrize('shape', [(128, 8, 77), (500, 64, 37)], **IDS)
def test_null_group_and_index_maps(shape, null):
    """group = NULL is sched group 0 for everyone; p_index / h_index = NULL is the identity map (B == nP == nH)."""
    from score_based_channels_amd import plan as PL
    h = _problem(shape, null=null.split('+'))
    dev = _Device(h, step=2)
    dev.launch(PL.LANGEVIN)
    _check_step('NULL ' + null, h, dev, 2, *_reference(h, 2))
    assert np.all(np.isnan(dev.log()[:2]))
    dev.assert_guards_and_inputs()


# ------------------------------------------------------------------------------------------------ in-kernel noise
@pytest.mark.parametrize('ids', ['traj_id', 'NULL'])
@pytest.mark.parametrize('shape', [(64, 16, 38), (64, 18, 38), (300, 128, 100), (500, 64, 37)], **IDS)
def test_in_kernel_noise_is_the_restated_stream(shape, ids):
    """noise = NULL: the flat kernel draws per pair (complex_normal_pair(q)), the tiled one per element (complex_normal(e)); both
    must be the stream oracle/ald_oracle.py::device_complex_normal restates, under a seed >= 2^63 and trajectory ids >= 2^32
    (NULL: the batch position).  nscale = 0.3, so a wrong draw is a wrong X by far more than the bound.  A trajectory gets the same
    bits wherever it sits in the batch."""
    from score_based_channels_amd import plan as PL
    h = _problem(shape, nscale=0.3)
    h.update(noise=None, seed=SEED, traj_id=TRAJ_IDS.copy() if ids == 'traj_id' else None)
    dev = _Device(h, step=1)
    dev.launch(PL.LANGEVIN)
    Xref, nref = _reference(h, 1)
    _check_step('philox ' + ids, h, dev, 1, Xref, nref, extra=0.3 * BOX_MULLER)
    dev.assert_guards_and_inputs()
    if ids == 'traj_id':
        perm = np.array([3, 0, 4, 1, 2])
        dev2 = _Device(_permuted(h, perm), step=1)
        dev2.launch(PL.LANGEVIN)
        assert np.array_equal(dev2.x().view(np.int32), dev.x()[perm].view(np.int32))
        assert np.array_equal(dev2.log()[1].view(np.int32), dev.log()[1][perm].view(np.int32))


# ------------------------------------------------------------------------------------------------ measurements
@pytest.mark.parametrize('noise', ['replayed', 'philox'])
@pytest.mark.parametrize('shape', R.SHAPES + R.MEASURE_ONLY_SHAPES, **IDS)
def test_measure(shape, noise):
    """Y = P[p_index] H[h_index] + meas_scale[b] n on its own (odd Nr included), n replayed or drawn in the kernel (step -1 of
    the trajectory's stream); on one flat and one tiled shape that Y then feeds a LANGEVIN record."""
    from score_based_channels_amd import plan as PL
    h = _problem(shape)
    h.update(seed=SEED, traj_id=TRAJ_IDS.copy())
    h['Y'] = np.full_like(h['Y'], np.nan)                        # every element must be written
    dev = _Device(h, step=0)
    over = dict(noise=None) if noise == 'philox' else {}
    dev.launch(PL.MEASURE, **over)
    P, H = _per_traj(h, 0)[:2]
    nz = h['mnoise'] if noise == 'replayed' else R.philox_noise(SEED, TRAJ_IDS, -1, (shape[2], shape[1]))
    Yref = R.measure64(P, H, h['meas_scale'], nz)
    Y = dev.y()
    err = max(rel_err(Y[b], Yref[b]) for b in range(R.B))
    from oracle import ald_oracle as A
    rest = max(rel_err(A.make_measurements(P[b:b + 1], H[b:b + 1], np.float64(h['meas_scale'][b]) ** 2, nz[b:b + 1]), Yref[b:b + 1])
               for b in range(R.B))
    print('MEASURE-ERR %-9s %-16s Y %.2e | complex64 restatement %.2e' % (noise, 'x'.join(map(str, shape)), err, rest))
    assert np.all(np.isfinite(Y)) and err < MEASURE_TOL + (float(h['meas_scale'].max()) * BOX_MULLER if noise == 'philox' else 0.0)
    assert np.all(np.isnan(dev.log())) and np.array_equal(dev.x().view(np.int32), h['X'].view(np.int32))
    dev.assert_guards_and_inputs(y_written=True)
    if noise == 'replayed' and shape in ((128, 8, 77), (500, 64, 37)):
        dev.launch(PL.LANGEVIN)
        g = dict(h, Y=Y.copy())
        _check_step('after MEASURE', g, dev, 0, *_reference(g, 0))
        assert np.array_equal(dev.y().view(np.int32), Y.view(np.int32))
        dev.assert_guards_and_inputs(y_written=True)


# ------------------------------------------------------------------------------------------------ several steps as a plan
@pytest.mark.parametrize('noise', ['replayed', 'philox'])
@pytest.mark.parametrize('shape', [(128, 8, 77), (500, 64, 37)], **IDS)
def test_three_steps_as_a_plan(shape, noise):
    """[LANGEVIN, STEP_INC] x 3 through sbc_plan_create / sbc_plan_run, eager and as a captured graph, the score held fixed: every
    row of the log and the final X against three iterations of the reference; graph == eager bit for bit; the counter reads 3."""
    import torch
    from score_based_channels_amd import _lib, plan as PL
    h = _problem(shape)
    if noise == 'philox':
        h.update(noise=None, seed=SEED, traj_id=TRAJ_IDS.copy())
    X, refs = h['X'], []
    for k in range(3):
        X, nm = _reference(h, k, X=X)
        refs.append(nm)
    stream = torch.cuda.Stream()
    got = []
    for use_graph in (False, True):
        dev = _Device(h, step=0)
        ext = dev.ext()
        plan = _lib.Plan([dev.op(PL.LANGEVIN, ext), dev.op(PL.STEP_INC, out=dev.step.data_ptr())], keepalive=dev)
        plan.run(stream.cuda_stream, 3, use_graph)
        stream.synchronize()
        torch.cuda.synchronize()
        assert int(dev.step.item()) == 3
        extra = float(h['sched'][:, :, 2].max()) * BOX_MULLER if noise == 'philox' else 0.0
        label = R.path_label(R.dispatch_path(*shape))
        log = dev.log()
        for k in range(3):
            en = float(np.max(np.abs(log[k] / refs[k] - 1)))
            print('PLAN-ERR %-8s graph=%d %-12s step %d nmse %.2e' % (noise, use_graph, 'x'.join(map(str, shape)), k, en))
            assert en < NMSE_TOL[label] + extra, (k, en)
        ex = max(rel_err(dev.x()[b], X[b]) for b in range(R.B))
        print('PLAN-ERR %-8s graph=%d %-12s final X %.2e' % (noise, use_graph, 'x'.join(map(str, shape)), ex))
        assert ex < X_TOL[label] + extra
        dev.assert_guards_and_inputs()
        got.append((dev.x().view(np.int32), log.view(np.int32)))
        plan.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


# ------------------------------------------------------------------------------------------------ refusals
def _refusals():
    """(op kind, overrides of the sbc_langevin / of the sbc_op, text the message must hold) -- every refusal of check_langevin and
    of the records around it, in the style of test_gpu_capi.py::L1_REFUSALS."""
    L, M, S = 'LANGEVIN', 'MEASURE', 'STEP_INC'
    t = [(L, dict(Nr=15), {}, 'Nr = 15 must be even')]
    t += [(L, {k: 8}, {}, '%s must be 16-byte aligned' % k) for k in ('X', 'score', 'Y', 'Htrue', 'noise', 'P')]      # (+8 bytes)
    t += [(L, dict(Nr=512, Np=38), {}, 'Nr=512 Np=38 needs')]                                                      # 152 KB > 150 KB
    t += [(L, {k: None}, {}, 'langevin: %s must be set' % k) for k in ('X', 'score', 'P', 'Y', 'Htrue', 'sched', 'nmse', 'step')]
    t += [(M, {k: None}, {}, 'measure: %s must be set' % k) for k in ('P', 'Y', 'Htrue', 'meas_scale')]
    t += [(L, dict(n_steps=0), {}, 'n_steps = 0'), (L, {}, dict(B=0), 'B = 0'), (M, {}, dict(B=0), 'B = 0'),
          (L, {}, dict(ext=None), 'ext'), (M, {}, dict(ext=None), 'ext'), (S, {}, dict(out=None), 'step_inc: out')]
    return t


def test_refusals_name_the_field_and_launch_nothing():
    import torch
    from score_based_channels_amd import _lib, plan as PL
    L = _lib.lib()
    h = _problem((64, 16, 38))
    dev = _Device(h, step=1)
    state = lambda: [_bits(t) for t in (dev.X, dev.Y, dev.nmse, dev.step)]
    before = state()

    def both(op):
        out = []
        handle = C.c_void_p()
        for rc in (L.sbc_op_launch(C.byref(op), None), L.sbc_plan_create(C.byref(op), 1, C.byref(handle))):
            out.append((rc, L.sbc_last_error().decode() if rc else ''))
        if handle:
            L.sbc_plan_destroy(handle)
        return out

    for kind, ext_over, op_over, text in _refusals():
        base = dev.ext(measure=kind == 'MEASURE')
        over = {k: (getattr(base, k) + v if isinstance(v, int) and k not in ('Nr', 'Np', 'n_steps') else v) for k, v in ext_over.items()}
        ext = dev.ext(measure=kind == 'MEASURE', **over) if kind != 'STEP_INC' and 'ext' not in op_over else None
        fields = dict(out=dev.step.data_ptr()) if kind == 'STEP_INC' else {}
        fields.update({k: v for k, v in op_over.items() if k != 'ext'})
        op = dev.op(getattr(PL, kind), ext, **fields)
        for rc, msg in both(op):
            assert rc == INVALID and text in msg, (kind, ext_over, op_over, rc, msg)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, state()))
    # the same records unmodified are accepted by both entry points (sbc_op_launch runs them: step 1, then the counter reads 2)
    for kind in ('MEASURE', 'LANGEVIN', 'STEP_INC'):
        ext = dev.ext(measure=kind == 'MEASURE') if kind != 'STEP_INC' else None
        op = dev.op(getattr(PL, kind), ext, **(dict(out=dev.step.data_ptr()) if kind == 'STEP_INC' else {}))
        assert [rc for rc, _ in both(op)] == [0, 0], (kind, both(op))
    torch.cuda.synchronize()
    assert int(dev.step.item()) == 2 and np.all(np.isfinite(dev.log()[1])) and np.all(np.isnan(dev.log()[[0, 2]]))
