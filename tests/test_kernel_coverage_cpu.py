"""No kernel ships unlaunched by a comparison test: every kernel of the built library is in the launched set of
profiles/kernel_coverage.txt (taken from rocprofv3 kernel traces of the GPU suite) or, if it is not part of an operator, on its
NOT LAUNCHED list with a reason.  Host only: tools/kernel_coverage.py reads the kernel names out of the library's code objects."""
import os
import subprocess
import sys

from conftest import ROOT

TOOL = os.path.join(ROOT, 'tools', 'kernel_coverage.py')
RECORD = os.path.join(ROOT, 'profiles', 'kernel_coverage.txt')
# fp32 Winograd, 32 -> 32, 256-pixel tiles: launched by the W = 128 records of tests/test_gpu_ops.py only
VICTIM = '_ZN3sbc16conv_wino_kernelILi32ELi32ELi2ELb1EEEvNS_10ConvParamsE'


def _check(record):
    return subprocess.run([sys.executable, TOOL, '--record', str(record)], capture_output=True, text=True)


def test_every_kernel_of_the_library_is_launched_by_a_traced_gpu_test():
    """A pull request that adds or re-parameterises a kernel has to launch it from a GPU test and regenerate the record
    (the tool's failure message, repeated here, says how)."""
    p = _check(RECORD)
    assert p.returncode == 0, ('kernels without a traced test (regenerate profiles/kernel_coverage.txt with tools/kernel_coverage.py --write '
                               'after tracing the GPU suite):\n' + p.stdout[-6000:] + p.stderr[-2000:])
    assert 'every kernel of' in p.stdout


def test_a_kernel_missing_from_the_record_is_named(tmp_path):
    """The check is live: with one launched name taken out of a copy of the record the tool fails and names that kernel; putting it on the
    NOT LAUNCHED list fails too, without a reason and -- an operator kernel -- with one."""
    text = open(RECORD).read()
    assert text.count('\n' + VICTIM + '\n') == 1
    cut = text.replace('\n' + VICTIM + '\n', '\n', 1)
    (tmp_path / 'cut.txt').write_text(cut)
    p = _check(tmp_path / 'cut.txt')
    assert p.returncode == 1 and 'NOT IN THE RECORD  ' + VICTIM in p.stdout and 'regenerate the record' in p.stdout
    assert p.stdout.count('NOT IN THE RECORD') == 1
    (tmp_path / 'bare.txt').write_text(cut.replace('== NOT LAUNCHED\n', '== NOT LAUNCHED\n' + VICTIM + '\n', 1))
    p = _check(tmp_path / 'bare.txt')
    assert p.returncode == 1 and 'NO REASON GIVEN    ' + VICTIM in p.stdout
    (tmp_path / 'waived.txt').write_text(cut.replace('== NOT LAUNCHED\n', '== NOT LAUNCHED\n' + VICTIM + ' no test yet\n', 1))
    p = _check(tmp_path / 'waived.txt')
    assert p.returncode == 1 and 'OPERATOR KERNEL ON THE NOT LAUNCHED LIST  ' + VICTIM in p.stdout
