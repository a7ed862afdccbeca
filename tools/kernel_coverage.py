#!/usr/bin/env python3
"""Which kernels of libsbc_hip.so does the GPU suite launch?  Host only: reads kernel NAMES, never instructions.

    python tools/kernel_coverage.py                         check the built library against profiles/kernel_coverage.txt (exit 1 on a hole)
    python tools/kernel_coverage.py STATS.csv [...]         table + never-launched list for these rocprofv3 kernel-statistics files
    python tools/kernel_coverage.py --write STATS.csv [...] the same, and rewrite the record from them
    python tools/kernel_coverage.py --write --merge STATS.csv [...]   rewrite the record from these files AND its current launched set: for
                                                            a change that leaves the other modules' kernels identical (tools/device_code_diff.py),
                                                            only the modules that launch the new kernels are traced again
    options:  --lib PATH  --record PATH  --parent-lib PATH --parent STATS.csv [...]  (the suite of the parent commit, for the first table;
              without them --write carries the record's current table over as the parent's)  --bench FILE [...]  (benchmark traces to list)

Kernel set: the `.name` entries of the AMDGPU metadata notes of the gfx950 code objects in the library (llvm-readelf --notes, as
tools/kernel_resources.py reads them).  Launched set: the `Name` column of `rocprofv3 --kernel-trace --stats -M -f csv` output, one run per
test module (the commands are kept in the record); -M keeps the names mangled so the two sets compare exactly, and c++filt is for printing only.
A directory given in place of a file stands for every *kernel_stats.csv below it."""
import argparse
import csv
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from check_no_packed import code_objects  # noqa: E402

READELF = '/opt/rocm/lib/llvm/bin/llvm-readelf'
FILT = '/usr/bin/c++filt'
LIB = os.path.join(ROOT, 'score_based_channels_amd', 'libsbc_hip.so')
RECORD = os.path.join(ROOT, 'profiles', 'kernel_coverage.txt')
BENCH_TRACES = ['profiles/r06_kernel_stats_cdlc_steps10.csv', 'profiles/r06_bench_big.json', 'profiles/r02_train_kernel_stats_b32.csv']
COMMANDS = """\
make -C score_based_channels_amd/csrc
# one step per module M in tests/test_gpu_*.py except test_gpu_bench.py (it runs bench.py, not a comparison), each under its own
# `timeout -k 10`, chained with &&; kernel trace and statistics only, no counters:
rocprofv3 --kernel-trace --stats -M -f csv -d <dir>/M -- python -m pytest tests/M.py -m gpu -q \\
    --deselect tests/test_gpu_parity.py::test_cli_two_ranks_equal_one_rank \\
    --deselect tests/test_gpu_parity.py::test_cli_several_test_profiles_are_one_sharded_list \\
    --deselect tests/test_gpu_parity.py::test_cli_rank_failure_ends_every_rank_quickly \\
    --deselect tests/test_gpu_train.py::test_data_parallel_training_is_the_same_optimisation
# (the deselected tests start ranks through torch.distributed.run: the same kernels as the single-process tests, more processes)
python tools/kernel_coverage.py --write <dir>"""


MERGED = """\
# THIS record was written with --write --merge: its launched set is the previous record's set plus the kernels in traces of only the
# modules that launch new kernels, taken with the command above; every kernel both libraries hold was shown to be identical
# (tools/device_code_diff.py).  A kernel whose code changes must be traced again, not carried over.  Traces merged in:"""


def library_kernels(path):
    """Mangled names of every kernel in the gfx950 code objects of `path`."""
    blob = open(path, 'rb').read()
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        for i, (triple, co) in enumerate(code_objects(blob)):
            if 'gfx' not in triple:
                continue
            fn = os.path.join(tmp, 'co%d.o' % i)
            open(fn, 'wb').write(co)
            txt = subprocess.run([READELF, '--notes', fn], capture_output=True, text=True, check=True).stdout
            for blk in txt.split('- .agpr_count:')[1:]:
                m = re.search(r'\.name:\s+(\S+)', blk)
                if m:
                    names.add(m.group(1).strip('\'"'))
    return names


def stats_files(paths):
    for p in paths:
        if os.path.isdir(p):
            for d, _, fs in sorted(os.walk(p)):
                for f in sorted(fs):
                    if f.endswith('kernel_stats.csv'):
                        yield os.path.join(d, f)
        else:
            yield p


def launched_kernels(paths):
    """Mangled names in the Name column of the kernel-statistics files."""
    names = set()
    for fn in stats_files(paths):
        with open(fn, newline='') as f:
            rows = csv.reader(line for line in f if not line.startswith('#'))
            head = next(rows, None)
            if not head or 'Name' not in head:
                continue
            k = head.index('Name')
            for r in rows:
                if len(r) > k:
                    n = r[k].strip()
                    names.add(n[:-3] if n.endswith('.kd') else n)
    return names


def demangle(names):
    names = list(names)
    out = subprocess.run([FILT], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def short(demangled):
    """'void sbc::k<1, 2>(sbc::P)' -> 'k<1, 2>': what the committed benchmark traces can be compared by."""
    s = re.sub(r'^void ', '', demangled).replace('(anonymous namespace)::', '')
    depth = 0
    for i, c in enumerate(s):
        depth += c == '<'
        depth -= c == '>'
        if c == '(' and depth == 0:
            s = s[:i]
            break
    return s.replace('sbc::', '').strip()


def template_of(demangled):
    return short(demangled).split('<')[0]


def table(lib, launched, dem):
    rows = {}
    for n in lib:
        r = rows.setdefault(template_of(dem[n]), [0, 0])
        r[0] += 1
        r[1] += n in launched
    lines = ['%-34s %10s %9s' % ('kernel template', 'in library', 'launched')]
    for t in sorted(rows):
        lines.append('%-34s %10d %9d' % (t, rows[t][0], rows[t][1]))
    lines.append('%-34s %10d %9d' % ('TOTAL', len(lib), len(lib & launched)))
    return lines


def bench_section(files, lib, launched, dem):
    by_short = {short(dem[n]): n for n in lib}
    lines = []
    for fn in files:
        text = open(os.path.join(ROOT, fn) if not os.path.isabs(fn) else fn).read()
        seen = sorted(set(re.sub(r'\s+', ' ', m) for m in re.findall(r'\b\w+_kernel(?:<[^<>()]*>)?', text)))
        here = [s for s in seen if s in by_short]
        missing = [s for s in here if by_short[s] not in launched]
        lines.append('%s: %d kernel names, %d still in the library, %d of those launched by no test' % (fn, len(seen), len(here), len(missing)))
        lines += ['  NOT LAUNCHED BY A TEST  ' + s for s in missing]
        lines += ['  launched  ' + s for s in here if s not in missing]
    return lines


def read_record(path):
    """{section title: [lines]} of the record; sections start with '== '."""
    sec, cur = {}, None
    if not os.path.exists(path):
        return sec
    for line in open(path).read().splitlines():
        if line.startswith('== '):
            cur = line[3:].strip()
            sec[cur] = []
        elif cur is not None:
            sec[cur].append(line)
    return sec


def record_sets(path):
    sec = read_record(path)
    launched = {ln.strip() for ln in sec.get('LAUNCHED', []) if ln.strip()}
    waived = {}
    for ln in sec.get('NOT LAUNCHED', []):
        if ln.strip() and not ln.startswith('#'):
            name, _, reason = ln.partition(' ')
            waived[name] = reason.strip(' :')
    return launched, waived


def check(lib_path, record):
    lib = library_kernels(lib_path)
    launched, waived = record_sets(record)
    dem = demangle(lib)
    print('\n'.join(table(lib, launched, dem)))
    holes = sorted(lib - launched - set(waived), key=lambda n: dem[n])
    noreason = sorted(n for n in waived if not waived[n])
    # the NOT LAUNCHED list is for kernels that are not part of an operator (probes, debug aids): a conv_* kernel is tested or deleted
    operator = sorted(n for n in waived if n in lib and template_of(dem[n]).startswith('conv'))
    if holes or noreason or operator or not lib:
        for n in holes:
            print('NOT IN THE RECORD  %s  %s' % (n, dem[n]))
        for n in noreason:
            print('NO REASON GIVEN    %s' % n)
        for n in operator:
            print('OPERATOR KERNEL ON THE NOT LAUNCHED LIST  %s  %s' % (n, dem[n]))
        print('%d of %d kernels of %s are neither launched by a traced GPU test nor on the NOT LAUNCHED list of %s (%d operator kernels are on '
              'that list).\nAdd a comparison test that launches them, trace the suite and regenerate the record:\n%s'
              % (len(holes), len(lib), lib_path, record, len(operator), COMMANDS))
        return 1
    print('every kernel of %s is launched by a GPU test (%d) or listed with a reason (%d)' % (lib_path, len(lib & launched), len(set(waived) & lib)))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('stats', nargs='*')
    ap.add_argument('--lib', default=LIB)
    ap.add_argument('--record', default=RECORD)
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--merge', action='store_true')
    ap.add_argument('--parent', nargs='*', default=[])
    ap.add_argument('--parent-lib')
    ap.add_argument('--parent-title', default='parent commit')
    ap.add_argument('--bench', nargs='*', default=BENCH_TRACES)
    a = ap.parse_args()
    if not a.stats:
        return check(a.lib, a.record)
    lib = library_kernels(a.lib)
    launched = launched_kernels(a.stats)
    if a.merge:
        launched |= record_sets(a.record)[0]
    dem = demangle(lib)
    tab = table(lib, launched, dem)
    never = sorted(lib - launched, key=lambda n: dem[n])
    print('\n'.join(tab))
    print('%d kernel names in the statistics files are not in the library (framework kernels)' % len(launched - lib))
    print('NEVER LAUNCHED: %d' % len(never))
    for n in never:
        print('  ' + short(dem[n]))
    bench = bench_section(a.bench, lib, launched, dem)
    print('\n'.join(bench))
    if not a.write:
        return 0
    old = read_record(a.record)
    _, waived = record_sets(a.record)
    if a.parent:
        plib = library_kernels(a.parent_lib or a.lib)
        pl = launched_kernels(a.parent)
        ptab = table(plib, pl, demangle(plib))
    else:
        ptab = [ln for ln in old.get('TABLE this suite', []) if ln.strip()]
    out = ['Kernel coverage of the GPU suite: which kernels of libsbc_hip.so a comparison test launches.  Written and checked by',
           'tools/kernel_coverage.py; tests/test_kernel_coverage_cpu.py holds every later build to it.  1x MI355X.', '',
           '== COMMANDS'] + COMMANDS.splitlines() + (MERGED.splitlines() + ['#   ' + (os.path.relpath(f, d) if os.path.isdir(d) else os.path.basename(f)) for d in a.stats for f in stats_files([d])] if a.merge else []) + ['', '== TABLE ' + a.parent_title] + ptab + ['', '== TABLE this suite'] + tab
    out += ['', '== BENCHMARK KERNELS'] + bench
    out += ['', '== NOT LAUNCHED', '# one line per kernel: mangled name, a blank, the reason']
    out += ['%s %s' % (n, waived.get(n, '')) for n in never]
    out += ['', '== LAUNCHED'] + sorted(lib & launched)
    open(a.record, 'w').write('\n'.join(out) + '\n')
    print('wrote %s (%d launched, %d not)' % (a.record, len(lib & launched), len(never)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
