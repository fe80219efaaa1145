#!/usr/bin/env python3
"""tools/compare_device_code.py [--by-symbol] <objdir A> <objdir B>: is the gfx950 device code of two builds the same?

For every *.o of A (ar-vae_amd/csrc/build or build_diag of two trees) the gfx950 code object is taken out of the fat binary and
disassembled with ROCm's LLVM tools; for every kernel symbol the instruction stream and the VGPR, SGPR, LDS, scratch and spill
figures of the two builds are compared.  Prints one line per kernel that differs (the first differing line) and a count; exit
status 1 if anything differs or a kernel or object exists on one side only.

--by-symbol pairs the kernels by symbol across ALL objects of each side instead of object by object (kernels that moved to another
source file still meet their counterpart); a kernel present on one side only is reported by name."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
FIGURES = ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'vgpr_spill_count',
           'sgpr_spill_count')


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels(obj, tmp):
    """{kernel symbol: (figures, [instructions])} of one host object; {} if it carries no device code"""
    fat, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'co')
    run(os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', obj, fat)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return {}
    run(os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET, '--input=' + fat, '--output=' + co)
    figures, rec = {}, {}
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '--notes', co).splitlines():
        m = re.match(r'  (- |  )\.(\w+):\s+(\S+)$', line)  # a key of a kernel's record in amdhsa.kernels (arguments sit deeper)
        if not m:
            continue
        if m.group(1) == '- ':
            rec = {}
        rec[m.group(2)] = m.group(3)
        if m.group(2) == 'name':
            figures[m.group(3)] = rec
    streams, cur = {}, None
    for line in run(os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', co).splitlines():
        m = re.match(r'<(\S+)>:', line)
        if m:
            cur = streams.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != '...':      # ('...': zero padding up to the next symbol)
            cur.append(re.sub(r'\s*//.*', '', line).strip())
    return {k: (tuple((f, r.get(f)) for f in FIGURES), streams.get(k, [])) for k, r in figures.items()}


def differs(where, k, a, b):
    """prints what differs between kernel k's two records (figures, instructions); False if nothing does"""
    if a[0] != b[0]:
        print(f'{where}{k}: ' + ', '.join(f'{f} {x} != {y}' for (f, x), (_, y) in zip(a[0], b[0]) if x != y))
    elif a[1] != b[1]:
        i = next((i for i, (x, y) in enumerate(zip(a[1], b[1])) if x != y), min(len(a[1]), len(b[1])))
        print(f'{where}{k}: instruction {i}: {a[1][i:i + 1]} != {b[1][i:i + 1]}')
    else:
        return False
    return True


def main_by_symbol(dir_a, dir_b):
    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        for d in (dir_a, dir_b):
            side = {}
            for o in sorted(f for f in os.listdir(d) if f.endswith('.o')):
                for k, rec in kernels(os.path.join(d, o), tmp).items():
                    if side.setdefault(k, rec) != rec:
                        sys.exit(f'{d}: {k} is defined differently in two objects')
            sides.append(side)
    a, b = sides
    differing = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f'{k}: only in {dir_a if k in a else dir_b}')
            differing += 1
        else:
            differing += differs('', k, a[k], b[k])
    print(f'{len(set(a) | set(b))} kernels ({len(a)} in {dir_a}, {len(b)} in {dir_b}): {differing} differ')
    return 1 if differing else 0


def main(dir_a, dir_b):
    objs = sorted(set(f for d in (dir_a, dir_b) for f in os.listdir(d) if f.endswith('.o')))
    total = differing = with_kernels = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            pa, pb = os.path.join(dir_a, o), os.path.join(dir_b, o)
            if not (os.path.exists(pa) and os.path.exists(pb)):
                print(f'{o}: only in {dir_a if os.path.exists(pa) else dir_b}')
                differing += 1
                continue
            a, b = kernels(pa, tmp), kernels(pb, tmp)
            with_kernels += bool(a or b)
            for k in sorted(set(a) | set(b)):
                total += 1
                if k not in a or k not in b:
                    print(f'{o}: {k}: only in {dir_a if k in a else dir_b}')
                    differing += 1
                else:
                    differing += differs(f'{o}: ', k, a[k], b[k])
    print(f'{total} kernels in {with_kernels} objects with kernels ({len(objs)} objects): {differing} differ')
    return 1 if differing else 0


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--by-symbol']
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit((main_by_symbol if len(args) < len(sys.argv) - 1 else main)(*args))
