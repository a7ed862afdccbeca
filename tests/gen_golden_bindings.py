"""Writes tests/golden/score_bindings.json (per case of ``bound_dump.cases()`` the sha256 of the binding's canonical dump and its
record count) and tests/golden/score_bindings_full.json.gz (the whole dump of ``bound_dump.FULL``, fields that are null or zero left
out).  The committed files were written at the last commit whose ``scorenet.py`` bound the records in Python; run it again only from
a commit whose binding is known good, never to make ``tests/test_bind_golden_cpu.py`` pass."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import bound_dump  # noqa: E402


if __name__ == '__main__':
    out, full = {}, {}
    for cid, mode, nt, nr, fusion, lanes in bound_dump.cases():
        records = bound_dump.dump(*bound_dump.bind(mode, nt, nr, fusion, lanes))
        out[cid] = dict(sha256=bound_dump.sha256(records), records=len(records))
        if cid in bound_dump.FULL:
            full[cid] = bound_dump.sparse(records)
    with open(os.path.join(HERE, 'golden', 'score_bindings.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    with open(os.path.join(HERE, 'golden', 'score_bindings_full.json.gz'), 'wb') as raw:
        with gzip.GzipFile(fileobj=raw, mode='wb', mtime=0) as f:
            f.write(json.dumps(full, sort_keys=True, separators=(',', ':')).encode())
    print('%d cases, %d in full' % (len(out), len(full)))
