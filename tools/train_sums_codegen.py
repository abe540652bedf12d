#!/usr/bin/env python3
"""What sharing the ordered sums (csrc/pw_train_sums.hpp) did to the compiler's output, against another build's objects:

    python3 tools/train_sums_codegen.py DIR     # DIR: the csrc/_obj of the parent commit's build at the same flags

Prints tools/code_object.py --compare DIR (every kernel but the three that add the slots must be instruction for instruction the
parent's), then, for those three, registers, spills, scratch instructions, instructions, floating-point additions and subtractions
and global loads and stores, DIR's beside this tree's.  A packed addition counts as two, except the horizontal one
(v_pk_add_f32 X, X, X op_sel_hi:[0,1]: one half adds the pair's two numbers, the other doubles the first and is dropped), which
counts as one and is listed under 'idle halves'.  The rule: no spill, no scratch instruction, vgpr + agpr not above DIR's, and the
same numbers of additions, loads and stores -- with -ffp-contract=off -fno-fast-math the compiler may neither reorder nor fuse the
sums, so equal counts from the same source order are the same arithmetic.  Exit status 0 when the rule holds.
profiles/train_sums_codegen.txt is this tool's output."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import code_object  # noqa: E402

REDUCE = ('pw_front_train_reduce_kernel', 'pw_lstm_train_wgrad_reduce_kernel', 'pw_head_train_reduce_kernel')
COLUMNS = ('vgpr', 'agpr', 'vgpr spill', 'scratch', 'instructions', 'idle halves', 'fp add/sub', 'global loads', 'global stores')
HORIZONTAL = re.compile(r'v_pk_add_f32 (v\[\d+:\d+\]), \1, \1 op_sel_hi:\[0,1\]')


def figures(k):
    asm = [' '.join(line.split()) for line in k['asm'] if line.split()]
    ops = [line.split()[0] for line in asm]
    idle = sum(bool(HORIZONTAL.match(line)) for line in asm)
    adds = sum(2 if op.startswith('v_pk_') else 1 for op in ops if re.match(r'v_(pk_)?(add|sub|subrev)_f32', op)) - idle
    return (k['.vgpr_count'], k['.agpr_count'], k['.vgpr_spill_count'], k['scratch_insts'], len(asm), idle, adds,
            sum(op.startswith('global_load') for op in ops), sum(op.startswith('global_store') for op in ops))


def reduce_kernels(objs):
    found = {}
    for ks in code_object.units(objs).values():
        for mangled, k in ks.items():
            for name in REDUCE:
                if name in mangled:
                    found[name] = figures(k)
    return found


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from multiagent_rl_amd import build_native
    code_object.compare(sys.argv[1])                 # names every kernel that differs: these three and no other
    old, new = reduce_kernels(sorted(glob.glob(os.path.join(sys.argv[1], '*.o')))), reduce_kernels(build_native.objects())
    print('\nthe three kernels that add the slots: parent | this tree')
    print('%-36s' % 'kernel' + ''.join('%15s' % c for c in COLUMNS))
    ok = True
    for name in REDUCE:
        o, n = old[name], new[name]
        print('%-36s' % name + ''.join('%15s' % ('%d | %d' % (a, b)) for a, b in zip(o, n)))
        ok = ok and n[2] == 0 and n[3] == 0 and n[0] + n[1] <= o[0] + o[1] and n[6:] == o[6:]
    print('rule (no spill, no scratch, vgpr + agpr not above the parent, equal additions, loads and stores): %s' % ('holds' if ok else 'BROKEN'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
