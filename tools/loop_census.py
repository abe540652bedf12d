#!/usr/bin/env python3
"""What a wave ISSUES per trip of a kernel's loops, counted from the disassembly of the built object (tools/code_object.py): for every
loop of a kernel -- a back edge to its header -- the instructions by class: VALU / SALU / LDS / VMEM / wait / nop / branch.  A wave
issues at most one instruction per four clocks whatever its kind, so a loop's cost has a floor that the VALU count alone does not show
(profiles/r6_quad_loop_census.txt holds the step loops of pw_spread_quad_kernel).

    python3 tools/loop_census.py 'pw_spread_quad_kernel<true,false,true>'      # the kernel of the built libpworld.so objects
    python3 tools/loop_census.py --co FILE.co 'pw_spread_quad_kernel<true'      # ... of a gfx950 code object given by path
    python3 tools/loop_census.py --dump OB                                      # the common path of one step loop, disassembled

Two counts per loop:
  body    every instruction of the natural loop (the blocks that reach the back edge without passing the header), inner loops included
  common  the shortest path from the header to the back edge that FALLS THROUGH every exec-skip branch (s_cbranch_execz jumps
          over a region only when no lane wants it; the path a step takes when some lane does) -- scalar branches (an episode reset,
          a cold block behind a wave-uniform test) take whichever side is shorter
Loops that hold an s_barrier are a workgroup's step loops; `role` names the quad kernel's by what only that wave does: the physics
waves publish the state ring (ds_write_b128) and store nothing to global memory, wave OA shuffles (ds_bpermute), wave OB stores
16-byte chunks, an idle physics wave only meets."""
import heapq
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import code_object  # noqa: E402

CLASSES = ('VALU', 'SALU', 'LDS', 'VMEM', 'wait', 'nop', 'branch')


def classify(op):
    if op.startswith('s_waitcnt'):
        return 'wait'
    if op == 's_nop':
        return 'nop'
    if op == 's_branch' or op.startswith('s_cbranch'):
        return 'branch'
    if op.startswith('ds_'):
        return 'LDS'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'VMEM'
    if op.startswith('v_'):
        return 'VALU'
    return 'SALU'   # s_* arithmetic, moves, compares, s_barrier, s_setprio, ...


def instructions(co):
    """-> {mangled kernel name: [(address, mnemonic, operands, branch target address or None)]} of a code object."""
    dis = subprocess.run([os.path.join(code_object.LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], capture_output=True, text=True,
                         check=True).stdout
    out, cur, start = {}, None, None
    for line in dis.splitlines():
        m = re.match(r'^([0-9a-f]+) <(\S+)>:', line)
        if m:
            cur, start = out.setdefault(m.group(2), []), int(m.group(1), 16)
            continue
        m = re.match(r'^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$', line)
        if cur is None or not m:
            continue
        op, args, addr, rest = m.group(1), m.group(2), int(m.group(3), 16), m.group(4)
        tgt = None
        if classify(op) == 'branch':
            t = re.search(r'<[^>]*\+0x([0-9a-f]+)>\s*$', rest)
            tgt = start + int(t.group(1), 16) if t else start   # no offset: the kernel's first instruction
        cur.append((addr, op, args, tgt))
    return out


def _blocks(ins):
    """Basic blocks: -> (list of (first index, last index)), successors per block)."""
    index = {a: i for i, (a, _, _, _) in enumerate(ins)}
    leaders = {0}
    for i, (_, op, _, tgt) in enumerate(ins):
        if tgt is not None:
            if tgt in index:
                leaders.add(index[tgt])
            leaders.add(i + 1)
        elif op == 's_endpgm':
            leaders.add(i + 1)
    leaders = sorted(x for x in leaders if x < len(ins))
    blocks = [(b, (leaders[k + 1] if k + 1 < len(leaders) else len(ins)) - 1) for k, b in enumerate(leaders)]
    at = {b: k for k, (b, _) in enumerate(blocks)}
    succ = []
    for k, (_, e) in enumerate(blocks):
        _, op, _, tgt = ins[e]
        s = []   # (successor block, is the taken side of an exec-skip branch)
        if tgt is not None and tgt in index:
            s.append((at[index[tgt]], op == 's_cbranch_execz'))
        if op not in ('s_branch', 's_endpgm') and k + 1 < len(blocks):
            s.append((k + 1, False))
        succ.append(s)
    return blocks, succ


def _count(ins, blocks, which):
    c = dict.fromkeys(CLASSES, 0)
    ops, text = [], []
    for k in which:
        for i in range(blocks[k][0], blocks[k][1] + 1):
            c[classify(ins[i][1])] += 1
            ops.append(ins[i][1])
            text.append('%6x  %s %s' % ins[i][:3])
    return c, ops, text


def loops(ins):
    """-> the loops of one kernel, in address order of their headers: dicts with 'header', 'latch' (addresses), 'body' and 'common'
    (counts by class), 'body_ops' / 'common_ops' (mnemonics), 'common_text' (the common path's disassembly), 'role'."""
    blocks, succ = _blocks(ins)
    pred = [[] for _ in blocks]
    for k, s in enumerate(succ):
        for j, _ in s:
            pred[j].append(k)
    # dominators (iterative; a kernel has a few hundred blocks): a back edge is an edge to a block that dominates its source -- a cold
    # block laid out behind the loop that jumps back INTO it is not one
    every = set(range(len(blocks)))
    dom = [every] * len(blocks)
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for k in range(1, len(blocks)):
            new = set.intersection(*[dom[p] for p in pred[k]]) | {k} if pred[k] else {k}
            if new != dom[k]:
                dom[k], changed = new, True
    found = {}
    for k, s in enumerate(succ):
        for j, _ in s:
            if j in dom[k]:   # header j, latch k
                found.setdefault(j, []).append(k)
    res = []
    for h, latches in sorted(found.items()):
        body, todo = {h}, list(latches)
        while todo:   # the natural loop: everything that reaches a latch without passing the header
            k = todo.pop()
            if k not in body:
                body.add(k)
                todo.extend(pred[k])
        # the common path: Dijkstra by instruction count over the loop's blocks, never along the taken side of an exec-skip branch
        size = lambda k: blocks[k][1] - blocks[k][0] + 1  # noqa: E731
        dist, prev, heap = {h: size(h)}, {}, [(size(h), h)]
        while heap:
            d, k = heapq.heappop(heap)
            if d > dist[k]:
                continue
            for j, skip in succ[k]:
                if j in body and j != h and not skip and d + size(j) < dist.get(j, 1 << 60):
                    dist[j], prev[j] = d + size(j), k
                    heapq.heappush(heap, (dist[j], j))
        ends = [k for k in latches if k in dist]
        path = []
        if ends:
            k = min(ends, key=dist.get)
            while True:
                path.append(k)
                if k == h:
                    break
                k = prev[k]
        bc, bops, _ = _count(ins, blocks, sorted(body))
        cc, cops, ctext = _count(ins, blocks, path[::-1])
        role = ''
        if 's_barrier' in bops:
            role = ('P' if 'ds_write_b128' in bops and not any(o.startswith('global_store') for o in bops) else
                    'OA' if 'ds_bpermute_b32' in bops else 'OB' if 'global_store_dwordx4' in bops else 'idle')
        res.append(dict(header=ins[blocks[h][0]][0], latch=ins[blocks[max(latches)][1]][0], body=bc, common=cc, body_ops=bops,
                        common_ops=cops, common_text=ctext, role=role))
    return res


def kernel_loops(name, co=None):
    """The loops of the kernel whose demangled name (without the anonymous namespace) starts with `name`, from code object `co` or from
    the built objects of libpworld.so."""
    with tempfile.TemporaryDirectory() as wd:
        cos = [co] if co else [code_object.code_object(o, wd) for o in __import__('multiagent_rl_amd.build_native', fromlist=['x']).objects()]
        for c in cos:
            ks = instructions(c)
            plain = {k: re.sub(r'^void ', '', v).replace(', ', ',') for k, v in code_object._plain(ks).items()}
            for k in sorted(ks):
                if plain[k].startswith(name.replace(', ', ',')):
                    return plain[k], loops(ks[k])
    raise SystemExit('no kernel named %s*' % name)


def report(name, co=None, dump=None):
    full, ls = kernel_loops(name, co)
    if dump:
        return '\n'.join(t for lp in ls if lp['role'] == dump for t in lp['common_text'])
    lines = ['%s: %d loops' % (full.split('(')[0], len(ls)),
             '%-6s %-6s %-6s %-7s' % ('header', 'latch', 'role', 'count') + ''.join('%7s' % c for c in CLASSES) + '%7s' % 'total']
    for lp in ls:
        for kind in ('body', 'common'):
            c = lp[kind]
            lines.append('%-6x %-6x %-6s %-7s' % (lp['header'], lp['latch'], lp['role'] or '-', kind) + ''.join('%7d' % c[k] for k in CLASSES) +
                         '%7d' % sum(c.values()))
    return '\n'.join(lines)


if __name__ == '__main__':
    args = sys.argv[1:]
    co = None
    if '--co' in args:
        i = args.index('--co')
        co = args[i + 1]
        del args[i:i + 2]
    dump = None
    if '--dump' in args:   # --dump ROLE: the common path of that step loop, instruction by instruction
        i = args.index('--dump')
        dump = args[i + 1]
        del args[i:i + 2]
    print(report(args[0] if args else 'pw_spread_quad_kernel<true,false,true>', co, dump))
