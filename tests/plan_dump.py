"""Canonical dump of a ``plan.ScorePlan`` and the matrix of plans ``tests/golden/score_plans.json`` records (shared by
``tests/gen_golden_plans.py``, which wrote that file from the wiring this repository had in Python before the library's became the
only one, and ``tests/test_plan_golden_cpu.py``, which holds today's wiring to it)."""
import hashlib
import json

from score_based_channels_amd import plan as P

GEOMETRIES = ((64, 16), (256, 64), (32, 32), (32, 16), (128, 8), (24, 8), (48, 16), (8, 8), (16, 64))
SIX = dict(fold_stats=True, fuse_pairs=True, fuse_res=True, fuse_chain=True, fuse_down=True, fuse_end=True)
THREE_LANES = (('refine5.adapt_convs.0.', 'res3.1.', 1), ('refine4.adapt_convs.0.', 'res3.1.', 2), ('refine3.adapt_convs.0.', 'res3.1.', 3))
ARGUMENT_SETS = (
    ('none', {}),
    ('fold', dict(fold_stats=True)),
    ('pairs', dict(fuse_pairs=True)),
    ('f16w_pairs+fold', dict(fuse_pairs=P.PAIR_SHAPES_F16W, fold_stats=True)),
    ('fold+pairs+res', dict(fold_stats=True, fuse_pairs=True, fuse_res=True)),
    ('pairs+chain', dict(fuse_pairs=True, fuse_chain=True)),
    ('six', SIX),
    ('six+skip', dict(SIX, skip_overlap=True)),
    ('fold+skip', dict(fold_stats=True, skip_overlap=True)),
    ('fold+pairs+res+end+overlap', dict(fold_stats=True, fuse_pairs=True, fuse_res=True, fuse_end=True, overlap=True)),
    ('overlap', dict(overlap=True)),
    ('private_slots', dict(share_slots=False)),
    ('six+three_lanes', dict(SIX, skip_overlap=THREE_LANES)),
)


def dump(plan):
    """Everything a plan says, as JSON-ready lists; tensors are named by their index in ``plan.tensors`` (by identity)."""
    index = {id(t): i for i, t in enumerate(plan.tensors)}
    assert len(index) == len(plan.tensors)

    def ti(t):
        return None if t is None else index[id(t)]

    def block(b):
        return [b[0], b[1], b[2], None if b[3] is None else sorted(b[3].items())]

    return dict(
        tensors=[[t.name, t.h, t.w, t.c, t.slot] for t in plan.tensors],
        ops=[dict(kind=o.kind, name=o.name, src=ti(o.src), dst=ti(o.dst), stats=ti(o.stats), res1=ti(o.res1), res2=ti(o.res2), up=ti(o.up),
                  weight=o.weight, weight2=o.weight2, bias=o.bias, bias2=o.bias2, norm2=o.norm2, flags=o.flags, ksize=o.ksize, dil=o.dil,
                  tag=o.tag, side=bool(o.side), join=bool(o.join), moments=ti(o.moments), geom=ti(o.geom), norm_key=o.norm_key,
                  blocks=None if o.blocks is None else [block(b) for b in o.blocks], lane=o.lane, signal=o.signal, wait=list(o.wait))
             for o in plan.ops],
        slot_elems=[int(n) for n in plan.slot_elems], x=ti(plan.x), out=ti(plan.out))


def summary(plan):
    """What the golden file holds per case."""
    text = json.dumps(dump(plan), sort_keys=True, separators=(',', ':'))
    return dict(sha256=hashlib.sha256(text.encode()).hexdigest(), records=len(plan.ops), slots=len(plan.slot_elems),
                lane_records=sum(1 for o in plan.ops if o.lane), side_records=sum(1 for o in plan.ops if o.side))


def cases():
    """``(case id, nt, nr, keyword arguments of build_score_plan)`` of the whole matrix."""
    for nt, nr in GEOMETRIES:
        for name, kw in ARGUMENT_SETS:
            yield '%dx%d/%s' % (nt, nr, name), nt, nr, kw
