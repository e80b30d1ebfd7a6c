#!/usr/bin/env python
"""Code bytes, registers and scratch of every kernel of one .hip translation unit (no GPU).

usage: python tools/kernel_code_sizes.py graph-detr4d_amd/csrc/gd4d_rowchain.hip [-DNAME=VALUE ...]

Compiles the file device-only with the Makefile's flags (hipcc --offload-arch=gfx950 --cuda-device-only
--no-gpu-bundle-output), reads the symbol table (llvm-readelf -s: a kernel's FUNC symbol size = its instruction bytes) and the
code-object metadata note (VGPRs, AGPRs, SGPRs, spills, private segment = scratch bytes per work-item) and prints one row per
kernel, largest first.  Exit status 1 if a kernel uses scratch or spills vector registers."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
CSRC = os.path.join(ROOT, 'graph-detr4d_amd', 'csrc')
FLAGS = ['--offload-arch=gfx950', '--cuda-device-only', '--no-gpu-bundle-output', '-O3', '-std=c++17', '-I' + os.path.join(ROOT, 'include'),
         '-I' + CSRC, '-fhip-fp32-correctly-rounded-divide-sqrt', '-ffp-contract=off', '-munsafe-fp-atomics', '-Wno-unused-function']


def demangle(names):
    try:
        out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    except (OSError, subprocess.CalledProcessError):
        out = names
    return {n: re.sub(r'\(.*', '', d).replace('gd4d::', '').replace('void ', '') for n, d in zip(names, out)}


def kernel_table(source, extra=()):
    """[(name, bytes, vgprs, agprs, sgprs, vgpr spills, scratch bytes)] of the kernels of `source`."""
    readelf = os.path.join(ROCM, 'llvm', 'bin', 'llvm-readelf')
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, 'unit.co')
        subprocess.check_call([os.path.join(ROCM, 'bin', 'hipcc')] + FLAGS + list(extra) + ['-c', source, '-o', obj])
        syms = subprocess.run([readelf, '-s', '-W', obj], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([readelf, '--notes', obj], capture_output=True, text=True, check=True).stdout
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == 'FUNC':
            size[f[7]] = int(f[2])
    rows = []
    for block in notes.split('  - .agpr_count:')[1:]:
        get = lambda key: re.search(r'\.' + key + r':\s+(\S+)', block)      # noqa: E731
        if not get('name') or not get('vgpr_count'):
            continue
        name = get('name').group(1)
        agpr = int(block.split()[0])
        rows.append((name, size.get(name, 0), int(get('vgpr_count').group(1)), agpr, int(get('sgpr_count').group(1)),
                     int(get('vgpr_spill_count').group(1)), int(get('private_segment_fixed_size').group(1))))
    names = demangle([r[0] for r in rows])
    return sorted(((names[r[0]],) + r[1:] for r in rows), key=lambda r: -r[1])


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rows = kernel_table(sys.argv[1], sys.argv[2:])
    width = max(len(r[0]) for r in rows)
    print(f'{"kernel":{width}s}  {"bytes":>7s} {"VGPR":>5s} {"AGPR":>5s} {"SGPR":>5s} {"spill":>5s} {"scratch":>7s}')
    for r in rows:
        print(f'{r[0]:{width}s}  {r[1]:7d} {r[2]:5d} {r[3]:5d} {r[4]:5d} {r[5]:5d} {r[6]:7d}')
    bad = [r[0] for r in rows if r[5] or r[6]]
    if bad:
        sys.exit('scratch or spilled vector registers in: ' + ', '.join(bad))


if __name__ == '__main__':
    main()
