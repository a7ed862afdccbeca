#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libsbc_hip.so, kernel by kernel:  device_code_diff.py OLD.so NEW.so

Every code object of both libraries is disassembled and the instruction text of each kernel symbol (comments stripped) compared.
Prints the symbols only in OLD, only in NEW, and those whose text differs; exit status 0 iff the last two lists are empty --
i.e. NEW is OLD minus removed kernels.  What a refactor of csrc/ shows instead of a timing; needs no GPU."""
import os
import re
import subprocess
import sys
import tempfile

from check_no_packed import OBJDUMP, code_objects


def kernels(lib):
    """{demangled symbol: instruction text} over every gfx950 code object in `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (triple, co) in enumerate(code_objects(open(lib, 'rb').read())):
            if 'gfx950' not in triple:
                continue
            fn = os.path.join(tmp, 'co%d.o' % i)
            open(fn, 'wb').write(co)
            dis = subprocess.run([OBJDUMP, '-d', '--no-show-raw-insn', '--no-leading-addr', '-C', fn],
                                 capture_output=True, text=True, check=True).stdout
            sym = None
            for line in dis.splitlines():
                m = re.match(r'^<(.+)>:$', line)
                if m:
                    sym = m.group(1)
                    assert sym not in out, 'symbol %s in two code objects of %s' % (sym, lib)
                    out[sym] = []
                elif sym and line[:1] in ' \t':
                    out[sym].append(line.split('//')[0].strip())
    return out


def main(old_lib, new_lib):
    old, new = kernels(old_lib), kernels(new_lib)
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differs = sorted(s for s in set(old) & set(new) if old[s] != new[s])
    print('%d symbols in OLD, %d in NEW, %d in both and identical' % (len(old), len(new), len(set(old) & set(new)) - len(differs)))
    for title, names in (('only in OLD', only_old), ('only in NEW', only_new), ('differs', differs)):
        print('%s (%d):' % (title, len(names)))
        for s in names:
            print('  %s' % s + ('  [%d / %d instructions]' % (len(old[s]), len(new[s])) if title == 'differs' else ''))
    return 1 if only_new or differs else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
