#!/usr/bin/env python3
"""What the compiler made of the kernels in libpworld.so, read from the built objects (multiagent_rl_amd/csrc/_obj/*.o): the gfx950
code object of each translation unit is unbundled from the object's .hip_fatbin section, its AMDGPU metadata notes give
registers / spills / private segment per kernel, its disassembly the number of scratch-memory instructions per kernel.

    python3 tools/code_object.py            # table of every kernel that spills, has a private segment or touches scratch
    python3 tools/code_object.py --all
    python3 tools/code_object.py --compare DIR   # DIR: the csrc/_obj of another build at the same flags (e.g. the parent commit's)

tests/test_code_object.py holds the rule: no kernel spills a VGPR and no kernel executes a scratch instruction.  --compare is the
proof a host-side refactor owes: per kernel, matched by mangled name, the metadata FIELDS and the disassembly are those of DIR."""
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
FIELDS = ('.vgpr_count', '.agpr_count', '.vgpr_spill_count', '.sgpr_count', '.sgpr_spill_count', '.private_segment_fixed_size',
          '.group_segment_fixed_size')


def tools_present():
    return all(os.path.exists(os.path.join(LLVM, t)) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf', 'llvm-objdump'))


def _demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def code_object(obj, workdir):
    """-> path of the gfx950 code object embedded in a host object compiled by hipcc."""
    base = os.path.join(workdir, os.path.basename(obj))
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=%s.fatbin' % base, obj, os.devnull])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o',
                           '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=%s.fatbin' % base, '--output=%s.co' % base])
    return base + '.co'


def kernels(co):
    """-> {mangled kernel name: {field: int, 'scratch_insts': int, 'asm': [instruction lines without the // address comments]}}"""
    notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], capture_output=True, text=True, check=True).stdout
    out = {}
    # one block per kernel: from its '.agpr_count' (first key of the sorted map after .args) to the next
    for blk in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
        blk = '\n    .agpr_count:' + blk
        name = re.search(r'\n\s+\.name:\s+(\S+)', blk).group(1)
        out[name] = {f: int(re.search(r'\n\s+%s:\s+(\d+)' % re.escape(f), blk).group(1)) for f in FIELDS}
        out[name]['asm'] = []
    dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], capture_output=True, text=True,
                         check=True).stdout
    cur = None
    for line in dis.splitlines():
        m = re.match(r'^[0-9a-f]+ <(\S+)>:', line)
        if m:
            cur = m.group(1) if m.group(1) in out else None
        elif cur and line.strip() not in ('', '...'):   # '...': objdump's mark for a run of zero padding behind a kernel, no instruction
            out[cur]['asm'].append(line.split('//')[0].rstrip())
    for d in out.values():
        d['scratch_insts'] = sum('scratch_' in line for line in d['asm'])
    return out


def units(objs):
    """-> {translation unit: kernels() of its object}"""
    with tempfile.TemporaryDirectory() as wd:
        return {os.path.basename(o).split('.')[0]: kernels(code_object(o, wd)) for o in objs}


def _plain(names):
    dm = _demangle(list(names))
    return {k: dm[k].replace('(anonymous namespace)::', '') for k in names}


def per_unit_kernels():
    """-> {translation unit: sorted demangled kernel names}: what each unit's code object really carries (all_kernels merges the
    units by name and cannot see a kernel that one unit compiles for nothing)."""
    from multiagent_rl_amd import build_native
    return {u: sorted(_plain(ks).values()) for u, ks in units(build_native.objects()).items()}


def compare(parent_dir):
    """Prints the kernels that sit in other units than in the build under parent_dir and the kernels whose metadata or
    disassembly differ; -> exit status (non-zero: a kernel differs, or one the parent had is in no unit any more)."""
    from multiagent_rl_amd import build_native
    old, new = units(sorted(glob.glob(os.path.join(parent_dir, '*.o')))), units(build_native.objects())
    if not old:
        sys.exit('no objects (*.o) in %s' % parent_dir)
    where = lambda tree, k: sorted(u for u, ks in tree.items() if k in ks)  # noqa: E731
    names = _plain({k for ks in list(old.values()) + list(new.values()) for k in ks})
    differ, gone = [], []
    for k in sorted(names, key=names.get):
        uo, un = where(old, k), where(new, k)
        if uo != un:
            print('%-40s -> %-40s %s' % (' '.join(uo) or '(new)', ' '.join(un) or '(GONE)', names[k].split('(')[0]))
        if uo and not un:
            gone.append(k)
        copies = [tree[u][k] for tree, us in ((old, uo), (new, un)) for u in us]
        if uo and un and any(c != copies[0] for c in copies):
            differ.append(k)
            print('DIFFERS: %s' % names[k])
    print('%d kernels in the parent, %d here; %d differ, %d gone' % (sum(bool(where(old, k)) for k in names),
                                                                      sum(bool(where(new, k)) for k in names), len(differ), len(gone)))
    return 1 if differ or gone else 0


def all_kernels():
    from multiagent_rl_amd import build_native
    res = {}
    for ks in units(build_native.objects()).values():
        res.update(ks)
    names = _plain(res)
    return {names[k]: v for k, v in res.items()}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    if '--compare' in sys.argv:
        sys.exit(compare(sys.argv[sys.argv.index('--compare') + 1]))
    ks = all_kernels()
    print('%-86s %5s %5s %6s %6s %5s %7s' % ('kernel', 'vgpr', 'vspill', 'sspill', 'priv B', 'LDS', 'scratch'))
    for n, d in sorted(ks.items()):
        if '--all' in sys.argv or d['.vgpr_spill_count'] or d['.private_segment_fixed_size'] or d['scratch_insts']:
            print('%-86s %5d %5d %6d %6d %5d %7d' % (n.split('(')[0][:86], d['.vgpr_count'], d['.vgpr_spill_count'], d['.sgpr_spill_count'],
                                                     d['.private_segment_fixed_size'], d['.group_segment_fixed_size'], d['scratch_insts']))
    print('%d kernels' % len(ks))
