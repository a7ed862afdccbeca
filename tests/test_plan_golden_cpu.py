"""The library's wiring of the score network (csrc/score_wire.cpp, read by plan.build_score_plan) against the plans this repository's
Python wiring built before it was removed: tests/golden/score_plans.json holds, per geometry and argument set, the sha256 of the
canonical dump (plan_dump.dump: every tensor, record, slot) and four counts.  And everything the wiring refuses, by type and
message.  No GPU: the wiring is host code."""
import ctypes as C
import json
import os

import pytest

import plan_dump
from score_based_channels_amd import _lib, plan as P

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'score_plans.json')) as _f:
    GOLDEN = json.load(_f)
CASES = list(plan_dump.cases())


def test_golden_matrix_is_the_whole_matrix():
    assert len(CASES) == 9 * 13 == len(GOLDEN) and {c[0] for c in CASES} == set(GOLDEN)
    at = lambda key: [GOLDEN['64x16/' + name][key] for name, _ in plan_dump.ARGUMENT_SETS]
    assert at('records') == [150, 136, 143, 129, 125, 65, 54, 54, 136, 124, 150, 150, 54]
    assert at('lane_records') == [0, 0, 0, 0, 0, 0, 0, 6, 20, 0, 0, 0, 4]
    assert at('side_records') == [0, 0, 0, 0, 0, 0, 0, 0, 0, 24, 24, 0, 0]


@pytest.mark.parametrize('cid,nt,nr,kw', CASES, ids=[c[0] for c in CASES])
def test_plan_equals_the_python_wiring_it_replaced(cid, nt, nr, kw):
    got = plan_dump.summary(P.build_score_plan(32, nt, nr, **kw))
    print(cid, got)
    counts = lambda s: {k: v for k, v in s.items() if k != 'sha256'}
    assert counts(got) == counts(GOLDEN[cid])
    assert got['sha256'] == GOLDEN[cid]['sha256']


def test_records_and_tensors_share_objects():
    """``op.src is t`` for a ``t`` of ``plan.tensors``: what plan_interp, train and scorenet key their buffers by."""
    pl = P.build_score_plan(32, 64, 16, fold_stats=True, fuse_pairs=True, fuse_chain=True)
    ids = {id(t) for t in pl.tensors}
    assert all(id(t) in ids for op in pl.ops for t in op.inputs() + op.outputs()) and id(pl.x) in ids and id(pl.out) in ids
    assert pl.ops[0].src is pl.x and pl.ops[-1].dst is pl.out
    assert pl.ops[1].src is pl.ops[0].moments and pl.ops[1].geom is pl.ops[0].dst            # (statistics from the begin convolution's tile moments)


def _wiring_dump(nt, nr, flags, conv_mode):
    """Canonical dump of the wiring the library builds from ``flags`` and ``conv_mode`` alone (its own shape list and skip branches)."""
    desc = _lib.sbc_score_wiring_desc(ngf=32, channels=2, nt=nt, nr=nr, flags=flags, conv_mode=conv_mode)
    h, view = C.c_void_p(), _lib.sbc_score_wiring_view()
    _lib.check(_lib.lib().sbc_score_wiring_create(C.byref(desc), C.byref(h)))
    try:
        _lib.check(_lib.lib().sbc_score_wiring_read(h, C.byref(view)))
        return ([(t.name, t.h, t.w, t.c, t.slot) for t in view.tensors[:view.n_tensors]],
                [(r.kind, r.name, r.src, r.dst, r.tag, r.lane, r.signal, tuple(r.wait)) for r in view.records[:view.n_records]])
    finally:
        _lib.lib().sbc_score_wiring_destroy(h)


def test_the_librarys_default_lists_are_the_python_constants():
    """``fuse_pairs=True`` / ``skip_overlap=True`` (the library's lists, what sbc_score_create uses) against plan.PAIR_SHAPES /
    plan.DEFAULT_SKIP_SPEC passed explicitly, with no conv_mode and in every mode but 'f16w'; conv_mode 2 (sbc_score_create, and
    ScoreNet in 'f16w') against plan.PAIR_SHAPES_F16W, at 64x16 and 256x64, which between them use every shape of that list."""
    kw = dict(fold_stats=True, fuse_res=True, fuse_chain=True, fuse_down=True, fuse_end=True)
    for nt, nr in ((64, 16), (256, 64)):
        for mode in (None, 'bf16x3', 'f16x2'):
            a = P.build_score_plan(32, nt, nr, fuse_pairs=True, skip_overlap=True, conv_mode=mode, **kw)
            b = P.build_score_plan(32, nt, nr, fuse_pairs=P.PAIR_SHAPES, skip_overlap=P.DEFAULT_SKIP_SPEC, **kw)
            assert plan_dump.dump(a) == plan_dump.dump(b)
    seen = set()
    for nt, nr in ((64, 16), (256, 64)):
        wide = P.build_score_plan(32, nt, nr, fuse_pairs=P.PAIR_SHAPES_F16W)
        assert plan_dump.dump(wide) == plan_dump.dump(P.build_score_plan(32, nt, nr, fuse_pairs=True, conv_mode='f16w'))
        seen |= {(o.src.c, o.src.w) for o in wide.ops if o.kind == P.CONV_PAIR}
        tensors, records = _wiring_dump(nt, nr, P.SCORE_FUSE_PAIRS, 2)
        index = {id(t): i for i, t in enumerate(wide.tensors)}
        assert tensors == [(t.name.encode(), t.h, t.w, t.c, t.slot) for t in wide.tensors]
        assert records == [(o.kind, o.name.encode(), index[id(o.src)], index[id(o.dst)], o.tag, o.lane, o.signal, (tuple(o.wait) + (0, 0))[:2])
                           for o in wide.ops]
    assert seen == set(P.PAIR_SHAPES_F16W)
    chains = [o for o in P.build_score_plan(32, 64, 16, fuse_chain=True).ops if o.kind == P.CHAIN]
    chains += [o for o in P.build_score_plan(32, 256, 64, fuse_chain=True).ops if o.kind == P.CHAIN]
    assert chains and all(o.tag == P.TAG_CHAIN + P.CHAIN_KERNELS.index((o.src.c, o.src.w)) for o in chains)
    assert {o.tag - P.TAG_CHAIN for o in chains} == set(range(len(P.CHAIN_KERNELS)))


def test_a_conv_mode_puts_its_gates_in_front_of_the_switches():
    """``conv_mode`` (sbc_score_wiring_desc.conv_mode 0 .. 3): folded statistics are dropped in 'f32' and for Nt or Nr that are no powers
    of two, and nothing else changes; without a mode the switches are taken as they are (the golden matrix; the trainer)."""
    same = lambda a, b: plan_dump.dump(a) == plan_dump.dump(b)
    for nt, nr in ((64, 16), (48, 16), (96, 32), (128, 8)):
        pow2 = not (nt & (nt - 1) or nr & (nr - 1))
        folded, plain = P.build_score_plan(32, nt, nr, fold_stats=True), P.build_score_plan(32, nt, nr)
        assert not same(folded, plain)
        for mode in ('bf16x3', 'f16w', 'f16x2'):
            assert same(P.build_score_plan(32, nt, nr, fold_stats=True, conv_mode=mode), folded if pow2 else plain)
            assert same(P.build_score_plan(32, nt, nr, conv_mode=mode), plain)
        assert same(P.build_score_plan(32, nt, nr, fold_stats=True, conv_mode='f32'), plain)
    with pytest.raises(KeyError):
        P.build_score_plan(32, 64, 16, conv_mode='fp8')
    desc = _lib.sbc_score_wiring_desc(ngf=32, channels=2, nt=64, nr=16, conv_mode=4)
    assert _lib.lib().sbc_score_wiring_create(C.byref(desc), C.byref(C.c_void_p())) == -1 and b'conv_mode' in _lib.lib().sbc_last_error()


def test_the_librarys_tags_are_the_python_constants():
    """Every ``plan.TAG_*`` that bench.py profiles by occurs on the records it names, and no other tag occurs."""
    six = P.build_score_plan(32, 64, 16, **plan_dump.SIX).ops
    plain = P.build_score_plan(32, 64, 16, fold_stats=True).ops
    assert {o.tag for o in six if o.kind == P.RES_BLOCK} == {P.TAG_RES_TOP} and {o.tag for o in six if o.kind == P.CONV_PAIR} == {P.TAG_PAIR_TOP}
    assert {o.tag for o in six if o.kind == P.CONV_POOL} == {P.TAG_POOL_TOP} and [o.tag for o in six if o.kind == P.CONV_DOWN] == [P.TAG_DOWN, P.TAG_DOWN + 1]
    top = {o.name for o in plain if o.tag == P.TAG_CONV_TOP}
    assert top == {o.name for o in plain if o.kind == P.CONV and o.ksize == 3 and o.src.c == o.dst.c == 32 and o.src.h == 64}
    mid = [o for o in plain if o.kind == P.CONV and o.ksize == 3 and o.dil == 1 and o.src.c == o.dst.c == 64 and o.src.h == 32 and not o.flags & P.EPI_POOL]
    direct = [o for o in mid if not o.flags & (P.PRO_NORM | P.EPI_UP | P.EPI_MOMENTS_OUT)]
    assert direct and len(direct) < len(mid)
    assert all(o.tag == (P.TAG_DIRECT_MID if o in direct else P.TAG_CONV_MID) for o in mid)
    known = {0, P.TAG_CONV_TOP, P.TAG_PAIR_TOP, P.TAG_CONV_MID, P.TAG_POOL_TOP, P.TAG_DIRECT_MID, P.TAG_RES_TOP, P.TAG_DOWN, P.TAG_DOWN + 1}
    assert {o.tag for o in six + plain} <= known | {P.TAG_CHAIN + k for k in range(len(P.CHAIN_KERNELS))}


def _too_many_events():
    """33 single-record branches, each behind the record in front of it: two events each."""
    names = [o.name for o in P.build_score_plan(32, 64, 16).ops]
    return [(names[k], names[k - 1], 1) for k in range(2, len(names), 3) if sum(n.startswith(names[k]) for n in names) == 1][:33]


REFUSALS = [
    (dict(nt=12, nr=4), 'Nt and Nr must be multiples of 8 (three 2x mean-pools), got 12x4'),
    (dict(nt=64, nr=20), 'Nt and Nr must be multiples of 8 (three 2x mean-pools), got 64x20'),
    (dict(skip_overlap=True, overlap=True), 'skip_overlap and overlap (SBC_OP_SIDE records) do not mix'),
    (dict(skip_overlap=[('res1.0.conv', 'begin_conv', 1)]), "skip branch 'res1.0.conv' is not one contiguous run of records (or bad lane 1)"),
    (dict(skip_overlap=[('refine5.adapt_convs.0.', 'res3.1.', 4)]),
     "skip branch 'refine5.adapt_convs.0.' is not one contiguous run of records (or bad lane 4)"),
    (dict(skip_overlap=[('refine5.adapt_convs.0.', 'res3.1.', 0)]),
     "skip branch 'refine5.adapt_convs.0.' is not one contiguous run of records (or bad lane 0)"),
    (dict(skip_overlap=[('refine5.adapt_convs.0.', 'nope.', 1)]), "anchor 'nope.' of skip branch 'refine5.adapt_convs.0.' not found in front of it"),
    (dict(skip_overlap=[('res2.0.conv2', 'res2.0.shortcut', 1), ('res2.0.normalize2', 'res2.0.conv1', 2), ('res2.0.shortcut', 'res2.0.normalize2', 3)]),
     "record 'res2.0.conv2' already waits for two events"),
    (dict(skip_overlap=[('refine5.adapt_convs.0.', 'res3.1.', 1), ('refine5.adapt_convs.0.1_1', 'res3.1.', 1)]),
     "skip branch 'refine5.adapt_convs.0.1_1' is already on a lane"),
    (dict(skip_overlap=[('refine4.adapt_convs.1.', 'res3.1.', 1)]),
     "skip branch 'refine4.adapt_convs.1.' reads refine3.output_convs.1_2_conv, which record 'res3.1.conv2' does not have yet"),
    (dict(skip_overlap=_too_many_events), 'more than 64 lane events'),
]


@pytest.mark.parametrize('kw,message', REFUSALS, ids=[m[:28] for _, m in REFUSALS])
def test_refusals_keep_their_type_and_message(kw, message):
    """Each message is the text the Python wiring raised, word for word."""
    kw = dict(dict(nt=64, nr=16), **kw)
    if callable(kw.get('skip_overlap')):
        kw['skip_overlap'] = kw['skip_overlap']()
        assert len(kw['skip_overlap']) == 33
        assert max(o.signal for o in P.build_score_plan(32, 64, 16, skip_overlap=kw['skip_overlap'][:32]).ops) == P.MAX_EVENTS    # (32 of them: accepted)
    with pytest.raises(ValueError) as e:
        P.build_score_plan(32, **kw)
    assert str(e.value) == message
