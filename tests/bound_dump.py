"""Canonical dump of what ``ScoreNet.bind`` hands the library -- every field of every ``sbc_op`` and ``sbc_chain`` -- and the matrix
of bindings ``tests/golden/score_bindings.json`` records (shared by ``tests/gen_golden_bindings.py``, which wrote that file at the
last commit whose ``scorenet.py`` bound the records in Python, and ``tests/test_bind_golden_cpu.py``, which holds today's binder to
it).  Scalars as they are; pointers by what they point at: ``slot:<i>``, ``param:<key of ScoreNet._woff>``, ``end`` (the record's
``sbc_endconv``), ``chain:<k>`` (the k-th ``sbc_chain``), ``sigmas``, ``labels`` or ``null``.  Needs no GPU: the nets live on the CPU
device and ``SBC_NO_CALIB`` keeps ``bind`` from launching the calibration pass."""
import ctypes as C
import hashlib
import json
import os

from score_based_channels_amd import _lib
from score_based_channels_amd.config import default_config
from score_based_channels_amd.scorenet import ScoreNet
from score_based_channels_amd.weights import seeded_state_dict

B = 3
MODES = ('bf16x3', 'f32', 'f16w', 'f16x2')
SIZES = ((64, 16), (128, 8), (256, 64), (24, 8))
UNFUSED = dict(fold_stats=False, fuse_pairs=False, fuse_res=False, fuse_chain=False, fuse_down=False, fuse_end=False)
# (fusion name, ScoreNet keyword arguments, the values of bind's ``lanes``: overlap=True never takes launch lanes)
FUSIONS = (('default', {}, (False, True)), ('unfused', UNFUSED, (False, True)), ('overlap', dict(overlap=True), (False,)))
FULL = tuple('%s/64x16/default/seq' % m for m in MODES)       # the cases whose whole dump the golden file holds

_nets = {}


def net(mode, fusion):
    """One CPU ScoreNet per (mode, fusion); the nets of a mode share one packed weight buffer."""
    if (mode, fusion) not in _nets:
        cfg = default_config()
        n = ScoreNet(cfg, device='cpu', conv_mode=mode, **dict((f[0], f[1]) for f in FUSIONS)[fusion])
        first = _nets.get((mode, FUSIONS[0][0]))
        if first is None:
            n.load_state_dict(seeded_state_dict(cfg, 2024))
        else:
            n._wdev, n._woff = first._wdev, first._woff
        _nets[mode, fusion] = n
    return _nets[mode, fusion]


def bind(mode, nt, nr, fusion, lanes):
    old = os.environ.get('SBC_NO_CALIB')
    os.environ['SBC_NO_CALIB'] = '1'
    try:
        n = net(mode, fusion)
        return n, n.bind(B, nt, nr, lanes=lanes)
    finally:
        if old is None:
            del os.environ['SBC_NO_CALIB']
        else:
            os.environ['SBC_NO_CALIB'] = old


def dump(n, bound):
    """``[record, ...]``: every field of the ``sbc_op`` by name; ``ext`` of a CHAIN / END_CONV record followed by the struct's fields."""
    names = {n._wdev.data_ptr() + 4 * off: 'param:' + key for key, off in n._woff.items()}
    assert len(names) == len(n._woff)
    for i, s in enumerate(bound.slots):
        assert s.data_ptr() not in names
        names[s.data_ptr()] = 'slot:%d' % i
    assert len(names) == len(n._woff) + len(bound.slots)
    names[n.sigmas.data_ptr()] = 'sigmas'
    names[bound.labels.data_ptr()] = 'labels'
    sym = lambda p: 'null' if not p else names[p]
    n_chains, out = 0, []
    for o in bound.ops:
        rec = {}
        for f, typ in _lib.sbc_op._fields_:
            if f == 'ext':
                continue
            v = getattr(o, f)
            rec[f] = list(v) if f == 'wait' else v if typ is C.c_int32 else sym(v)
        if o.kind == 24:                    # SBC_OP_CHAIN
            ch = C.cast(o.ext, C.POINTER(_lib.sbc_chain)).contents
            rec['ext'] = 'chain:%d' % n_chains
            n_chains += 1
            rec['chain'] = {f: getattr(ch, f) if f == 'n_blocks' else list(getattr(ch, f)) if f in ('type', 'dil')
                            else [sym(p) for p in getattr(ch, f)] for f, _ in _lib.sbc_chain._fields_}
        elif o.kind == 5:                   # SBC_OP_END_CONV
            e = C.cast(o.ext, C.POINTER(_lib.sbc_endconv)).contents
            rec['ext'] = 'end'
            rec['end'] = {f: sym(getattr(e, f)) for f, _ in _lib.sbc_endconv._fields_}
        else:
            assert not o.ext
            rec['ext'] = 'null'
        out.append(rec)
    return out


def sparse(records):
    """The dump without the fields that say nothing: null pointers, zeros, empty wait lists."""
    return [{k: v for k, v in r.items() if v not in ('null', 0, [0, 0])} for r in records]


def text(records):
    return json.dumps(records, sort_keys=True, separators=(',', ':'))


def sha256(records):
    return hashlib.sha256(text(records).encode()).hexdigest()


def cases():
    """``(case id, mode, nt, nr, fusion, lanes)`` of the whole matrix."""
    for mode in MODES:
        for nt, nr in SIZES:
            for fusion, _, lane_values in FUSIONS:
                for lanes in lane_values:
                    yield '%s/%dx%d/%s/%s' % (mode, nt, nr, fusion, 'lanes' if lanes else 'seq'), mode, nt, nr, fusion, lanes
