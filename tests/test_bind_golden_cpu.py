"""The library's binder (csrc/score_wire.cpp: sbc_score_wiring_bind, called by scorenet.ScoreNet.bind) against the records this
repository's Python binder built before it was removed: tests/golden/score_bindings.json holds, per conv_mode, array size, fusion set
and lane choice, the sha256 of the canonical dump (bound_dump.dump: every field of every sbc_op and sbc_chain, pointers by what they
point at), tests/golden/score_bindings_full.json.gz the whole dump of the four modes at 64x16.  And what the binder refuses.  No GPU:
binding is pointer arithmetic, the nets live on the CPU device."""
import ctypes as C
import gzip
import json
import os

import pytest

import bound_dump
from score_based_channels_amd import _lib

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
with open(os.path.join(_GOLDEN, 'score_bindings.json')) as _f:
    GOLDEN = json.load(_f)
with gzip.open(os.path.join(_GOLDEN, 'score_bindings_full.json.gz')) as _f:
    FULL = json.loads(_f.read().decode())
CASES = list(bound_dump.cases())


def test_golden_matrix_is_the_whole_matrix():
    assert len(CASES) == 4 * 4 * 5 == len(GOLDEN) and {c[0] for c in CASES} == set(GOLDEN)
    assert set(FULL) == set(bound_dump.FULL) <= set(GOLDEN)
    # lanes and side records are different bindings in every mode, and every kind of fused record is in the matrix
    for m in bound_dump.MODES:
        assert len({GOLDEN['%s/64x16/%s' % (m, v)]['sha256'] for v in ('default/seq', 'default/lanes', 'overlap/seq')}) == 3
    assert [GOLDEN[c]['records'] for c in bound_dump.FULL] == [136, 150, 128, 54]
    kinds = {r['kind'] for recs in FULL.values() for r in recs}
    assert kinds == {1, 2, 3, 4, 5, 21, 22, 23, 24, 25}


@pytest.mark.parametrize('cid,mode,nt,nr,fusion,lanes', CASES, ids=[c[0] for c in CASES])
def test_binding_equals_the_python_binder_it_replaced(cid, mode, nt, nr, fusion, lanes):
    n, bound = bound_dump.bind(mode, nt, nr, fusion, lanes)
    records = bound_dump.dump(n, bound)
    if cid in FULL:                         # (first, so that a difference shows as records, not as a digest)
        for i, (got, want) in enumerate(zip(bound_dump.sparse(records), FULL[cid])):
            assert got == want, (cid, i)
    assert len(records) == GOLDEN[cid]['records'] == len(bound.plan.ops)
    assert bound_dump.sha256(records) == GOLDEN[cid]['sha256']
    # the interface bench.py, ald.py and the tools use: a list of sbc_op that can be sliced and concatenated
    assert isinstance(bound.ops, list) and all(isinstance(o, _lib.sbc_op) for o in bound.ops)
    assert bound.x.shape == bound.out.shape == (bound_dump.B, nt, nr, 2) and bound.labels.shape == (bound_dump.B,)


def _bind_raw(n, pl, table):
    """sbc_score_wiring_bind of ``pl`` for batch 1 over fake slot addresses and the parameter ``table`` {name: address}."""
    names = [k.encode() for k in table]
    params = (_lib.sbc_named_ptr * len(names))(*[_lib.sbc_named_ptr(k, v) for k, v in zip(names, table.values())])
    slots = (C.c_void_p * len(pl.slot_elems))(*[0x1000 * (i + 1) for i in range(len(pl.slot_elems))])
    ext = _lib.sbc_endconv()
    ops, chains = (_lib.sbc_op * len(pl.ops))(), (_lib.sbc_chain * pl.wiring.n_chains)()
    desc = _lib.sbc_score_bind_desc(batch=1, conv_mode=_lib.CONV_MODE_IDS[n.conv_mode], slots=slots, n_slots=len(slots), params=params,
                                    n_params=len(params), endconv=C.pointer(ext))
    rc = _lib.lib().sbc_score_wiring_bind(pl.wiring.handle, C.byref(desc), ops, chains)
    return rc, _lib.lib().sbc_last_error().decode(), list(ops), list(chains)


def test_a_table_without_a_form_a_kernel_reads_is_refused():
    """Each kind of form once: the message names the record and the form."""
    n = bound_dump.net('f16x2', 'default')
    pl = n.score_plan(64, 16)
    table = {k: 0x10000000 + 4 * off for k, off in n._woff.items()}
    assert _bind_raw(n, pl, table)[0] == 0
    for key, record in (('res1.0.conv1.weight#split', 'res1.0.block'), ('res2.0.shortcut.conv.weight#pool', 'res2.0.down'),
                        ('res2.1.conv1.weight#winograd_split', 'res2.1.conv1'), ('res5.1.normalize2', 'res5.0.chain.0+'),
                        ('refine1.adapt_convs.0.2_1_conv.weight#split', 'res5.0.chain.0+'), ('res2.0.conv1.bias', 'res2.0.conv1'),
                        ('begin_conv.weight', 'begin_conv'), ('normalizer', 'end_conv'), ('res2.0.normalize1', 'res2.0.normalize1')):
        assert key in table
        rc, msg, _, _ = _bind_raw(n, pl, {k: v for k, v in table.items() if k != key})
        assert rc == -1 and "'%s'" % key in msg and "record '%s" % record in msg, (key, rc, msg)
    f32 = bound_dump.net('f32', 'default')
    rc, msg, _, _ = _bind_raw(f32, f32.score_plan(64, 16), {k: 0x10000000 + 4 * off for k, off in f32._woff.items() if k != 'res1.0.conv1.weight#winograd'})
    assert rc == -1 and "record 'res1.0.conv1' reads 'res1.0.conv1.weight#winograd'" in msg


def test_a_table_without_the_calibration_only_forms_binds_them_null():
    """What a host with one array size packs (sbc_score_create): no Winograd form of a layer that runs fused, no unpooled form of a
    CONV_DOWN layer.  Everything else is the binding of the full table."""
    n = bound_dump.net('f16x2', 'default')
    pl = n.score_plan(64, 16)
    table = {k: 0x10000000 + 4 * off for k, off in n._woff.items()}
    fused, down = set(), set()
    for op in pl.ops:
        if op.kind in (21, 22, 23):
            fused |= {op.weight, op.weight2} - {None}
        elif op.kind == 24:
            fused |= {k for b in op.blocks for k in (b[1], b[2], b[3] and b[3]['w3']) if k}
        elif op.kind == 25:
            down |= {op.weight, op.weight2}
    assert fused and len(down) == 4
    lean = {k: v for k, v in table.items() if not (k.endswith('#winograd_split') and k[:-len('#winograd_split')] in fused | down)
            and not (k.endswith('#split') and k[:-len('#split')] in down)}
    assert len(lean) < len(table)
    rc, msg, full_ops, full_chains = _bind_raw(n, pl, table)
    assert rc == 0, msg
    rc, msg, ops, chains = _bind_raw(n, pl, lean)
    assert rc == 0, msg
    only_calib = {21: ('weight_wino_split', 'weight2_wino_split'), 22: ('weight_wino_split',), 23: ('weight_wino_split', 'weight2_wino_split'),
                  25: ('weight', 'weight_wino_split', 'weight_wino')}
    seen = set()
    for a, b in zip(ops, full_ops):
        for f, _ in _lib.sbc_op._fields_:
            if f in only_calib.get(a.kind, ()):
                assert getattr(a, f) is None and getattr(b, f) is not None, (a.kind, f)
                seen.add((a.kind, f))
            elif f == 'wait':
                assert list(a.wait) == list(b.wait)
            elif f != 'ext':
                assert getattr(a, f) == getattr(b, f), (a.kind, f)
    assert seen == {(k, f) for k, fs in only_calib.items() for f in fs}
    assert len(chains) == len(full_chains) == pl.wiring.n_chains > 0
    dilated = 0
    for a, b in zip(chains, full_chains):
        for f, _ in _lib.sbc_chain._fields_:
            if f in ('w1_wino', 'w2_wino'):
                assert not any(getattr(a, f))
                # the full table: every undilated layer's Winograd form, none of a dilated layer
                assert [bool(p) for p in getattr(b, f)] == [k < b.n_blocks and b.dil[k] <= 1 for k in range(6)]
                dilated += sum(b.dil[k] > 1 for k in range(b.n_blocks))
            else:
                assert list(getattr(a, f)) == list(getattr(b, f)) if f != 'n_blocks' else a.n_blocks == b.n_blocks
    assert dilated
