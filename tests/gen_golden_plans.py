"""Writes tests/golden/score_plans.json: per case of ``plan_dump.cases()`` the sha256 of the plan's canonical dump and four counts.
The committed file was written at the last commit whose ``plan.py`` wired the network in Python; run it again only from a commit
whose wiring is known good, never to make ``tests/test_plan_golden_cpu.py`` pass."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import plan_dump  # noqa: E402
from score_based_channels_amd import plan as P  # noqa: E402

if __name__ == '__main__':
    out = {cid: plan_dump.summary(P.build_score_plan(32, nt, nr, **kw)) for cid, nt, nr, kw in plan_dump.cases()}
    with open(os.path.join(HERE, 'golden', 'score_plans.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases' % len(out))
