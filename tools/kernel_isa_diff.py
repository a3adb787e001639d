#!/usr/bin/env python3
"""Per-kernel instruction streams of two builds, compared: the check for a refactor of kernel text.
usage: tools/kernel_isa_diff.py OLD NEW    two assembly files (hipcc <HIPFLAGS of the Makefile> --cuda-device-only -S) or two built librpt_hip.so
Of every symbol only the instruction lines count: no directives, no comments, a branch label becomes the position it marks.
Prints `same N of M` and, for each symbol whose stream differs, its name and both instruction counts; exit status 1 if any differs."""
import os, re, shutil, subprocess, sys, tempfile

LLVM = '/opt/rocm/lib/llvm/bin/'

def listing(path):
    if not path.endswith('.so'): return open(path).read()
    with tempfile.TemporaryDirectory() as t:         # the gfx950 code objects of the library, disassembled
        shutil.copy(path, os.path.join(t, 'lib.so'))
        subprocess.run([LLVM + 'llvm-objdump', '--offloading', 'lib.so'], cwd=t, check=True, capture_output=True)
        return ''.join(subprocess.run([LLVM + 'llvm-objdump', '-d', os.path.join(t, f)], check=True, capture_output=True, text=True).stdout
                       for f in sorted(os.listdir(t)) if 'gfx950' in f)

def streams(text):
    out, labels, cur = {}, {}, None
    for line in text.split('\n'):
        line = re.split(r';|//', line)[0].rstrip()
        sym = re.match(r'(?:[0-9a-f]+ <)?([^\s<>:]+)>?:$', line)
        if sym and sym[1].startswith('.L'): labels[sym[1]] = str(len(cur)) if cur is not None else '?'
        elif sym: cur = out.setdefault(sym[1], [])
        elif cur is not None and line[:1].isspace() and not line.lstrip().startswith('.'): cur.append(' '.join(line.split()))
    return {k: [re.sub(r'\.L\w+', lambda m: '@' + labels.get(m[0], m[0]), i) for i in v] for k, v in out.items() if v}

def main(old, new):
    a, b = streams(listing(old)), streams(listing(new))
    names = sorted(set(a) | set(b))
    differ = [n for n in names if a.get(n) != b.get(n)]
    print('same %d of %d' % (len(names) - len(differ), len(names)))
    pretty = subprocess.run(['c++filt'], input='\n'.join(differ), capture_output=True, text=True).stdout.split('\n')
    for n, p in zip(differ, pretty):
        print('%6s -> %6s  %s' % (len(a[n]) if n in a else '-', len(b[n]) if n in b else '-', p))
    return 1 if differ else 0

if __name__ == '__main__':
    if len(sys.argv) != 3: sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
