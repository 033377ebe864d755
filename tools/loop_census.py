#!/usr/bin/env python3
"""Instruction census of a kernel's token loops, from a `hipcc -S` dump.

    python tools/loop_census.py DUMP.s KERNEL [--opcodes]

KERNEL is a substring of the kernel's symbol (mangled, or demangled where c++filt is on the PATH); every kernel that
matches is reported.  The tool builds the kernel's control-flow graph from its labels and branches, finds the natural
loops, keeps the innermost ones that contain a `v_cmpx_ge_u32` (the emit compare of a token step: k_encode_counts.h)
and prints for each the number of instructions per class -- VALU, v_mov among them, LDS, vector-memory loads and
stores, s_load*, s_waitcnt, s_nop, *saveexec*, other scalar -- and, with --opcodes, per opcode.  A block that belongs to
the loop but is laid out behind its latch (the staging buffer's flush) is counted apart: it runs once in a few steps.

Also printed, because they are what the loop is held to (profiles/token_loop_blocks.md):
  - the s_waitcnt operands between the loop header and the first token step;
  - the s_nop that stand outside a v_cmpx -> v_mbcnt pair.
Static facts of the ISA, not timings.  Runs on the CPU."""
import argparse
import collections
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"^([.\w$]+):")
BRANCH = re.compile(r"^s_(?:c?branch\w*)\s+([.\w$]+)")
FAR = re.compile(r"^s_add_u32\s.*\(([.\w$]+)-\.Lpost_getpc\d+\)")  # a branch out of s_cbranch's reach: s_getpc, add, s_setpc
STEP = "v_cmpx_ge_u32"


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def functions(lines):
    """{symbol: (first line, last line)} of every function of the dump."""
    out, cur = {}, None
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.type\s+([.\w$]+),@function", l)
        if m:
            cur = (m.group(1), i)
        elif cur and re.match(r"\s*\.Lfunc_end\d+:", l):
            out[cur[0]] = (cur[1], i)
            cur = None
    return out


class Block:
    def __init__(self, idx, label):
        self.idx, self.label, self.ins, self.succ = idx, label, [], []


def cfg_of(body):
    """Basic blocks of a function body (list of source lines) in layout order."""
    blocks, by_label = [Block(0, None)], {}
    for raw in body:
        l = raw.split(";")[0].strip()
        if not l or l.startswith("//"):
            continue
        m = LABEL.match(l)
        if m and m.group(1).startswith(".Lpost_getpc"):
            continue
        if m:
            if blocks[-1].ins or blocks[-1].label:
                blocks.append(Block(len(blocks), m.group(1)))
            else:
                blocks[-1].label = m.group(1)
            by_label[m.group(1)] = blocks[-1]
            continue
        if l.startswith("."):
            continue
        blocks[-1].ins.append(l)
        if BRANCH.match(l) or l.startswith(("s_endpgm", "s_setpc", "s_trap")):
            blocks.append(Block(len(blocks), None))
    for b in blocks:
        fall = True
        if b.ins:
            last = b.ins[-1]
            m = BRANCH.match(last)
            if last.startswith("s_setpc"):
                far = [FAR.match(l) for l in b.ins]
                m = next((f for f in reversed(far) if f), None)
            if m and m.group(1) in by_label:
                b.succ.append(by_label[m.group(1)].idx)
            if last.startswith(("s_branch", "s_endpgm", "s_setpc")):
                fall = False
        if fall and b.idx + 1 < len(blocks):
            b.succ.append(b.idx + 1)
    return blocks


def natural_loops(blocks):
    """{header: set of blocks} -- the loops of one header merged."""
    n = len(blocks)
    pred = [[] for _ in range(n)]
    for b in blocks:
        for s in b.succ:
            pred[s].append(b.idx)
    # reachable blocks in reverse post-order, then the iterative dominator sets
    seen, order, stack = {0}, [], [(0, iter(blocks[0].succ))]
    while stack:
        node, it = stack[-1]
        for s in it:
            if s not in seen:
                seen.add(s)
                stack.append((s, iter(blocks[s].succ)))
                break
        else:
            order.append(node)
            stack.pop()
    order.reverse()
    dom = {v: set(order) for v in order}
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for v in order[1:]:
            ps = [dom[p] for p in pred[v] if p in dom]
            new = (set.intersection(*ps) if ps else set()) | {v}
            if new != dom[v]:
                dom[v], changed = new, True
    loops = collections.defaultdict(set)
    for v in order:
        for h in blocks[v].succ:
            if h in dom[v]:  # back edge v -> h
                body, work = {h, v}, [v]
                while work:
                    x = work.pop()
                    if x == h:
                        continue
                    for p in pred[x]:
                        if p in dom and p not in body:
                            body.add(p)
                            work.append(p)
                loops[h] |= body
    # a rotated loop keeps the block that prefetches for the next iteration in FRONT of its header, entered from the latch
    # and from outside: no natural-loop member, but it runs once per iteration -- a block entered from the loop and leading
    # nowhere but into it belongs to it
    for body in loops.values():
        grown = True
        while grown:
            grown = False
            for x in order:
                if x not in body and blocks[x].succ and all(t in body for t in blocks[x].succ) \
                        and any(q in body for q in pred[x]):
                    body.add(x)
                    grown = True
    return loops


def classify(op):
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_nop":
        return "s_nop"
    if "saveexec" in op:
        return "saveexec"
    if op.startswith("s_load"):
        return "s_load*"
    if op.startswith("s_"):
        return "other scalar"
    if op.startswith("ds_"):
        return "LDS"
    if re.match(r"(global|buffer|flat|scratch)_load", op):
        return "vector loads"
    if re.match(r"(global|buffer|flat|scratch)_", op):
        return "vector stores / atomics"
    if op.startswith("v_"):
        return "VALU"
    return "other"


ORDER = ["VALU", "  of them v_mov", "LDS", "vector loads", "vector stores / atomics", "s_load*", "s_waitcnt", "s_nop",
         "saveexec", "other scalar", "other"]


def census(ins):
    c, ops = collections.Counter(), collections.Counter()
    for l in ins:
        op = l.split()[0]
        ops[op] += 1
        c[classify(op)] += 1
        if op.startswith("v_mov"):
            c["  of them v_mov"] += 1
    return c, ops


def report(sym, pretty, body, want_ops):
    blocks = cfg_of(body)
    loops = natural_loops(blocks)
    has_step = {h: any(STEP in l for b in bl for l in blocks[b].ins) for h, bl in loops.items()}
    inner = [h for h in loops if has_step[h]
             and not any(o != h and has_step[o] and loops[o] < loops[h] for o in loops)]
    print(f"kernel {pretty}\n  symbol {sym}\n  {len(inner)} innermost loop(s) with {STEP}")
    for k, h in enumerate(sorted(inner)):
        members = sorted(loops[h])
        latch = max(b for b in members if h in blocks[b].succ)
        inline = [l for b in members if b <= latch for l in blocks[b].ins]
        behind = [l for b in members if b > latch for l in blocks[b].ins]
        steps = sum(STEP in l for l in inline)
        c, ops = census(inline)
        cb, opsb = census(behind)
        print(f"\n  loop {k}: header {blocks[h].label}, {steps} token step(s), {len(inline)} instructions in line, "
              f"{len(behind)} behind the latch")
        for name in ORDER:
            if c[name] or cb[name]:
                print(f"    {name:26s}{c[name]:6d}{('   (+' + str(cb[name]) + ' behind the latch)') if cb[name] else ''}")
        first = next(i for i, l in enumerate(inline) if STEP in l)
        waits = [l.split(None, 1)[1] for l in inline[:first] if l.startswith("s_waitcnt")]
        print(f"    s_waitcnt before the first token step: {', '.join(waits) if waits else 'none'}")
        in_pair, outside = False, 0
        for l in inline:
            if STEP in l:
                in_pair = True
            elif l.startswith("v_mbcnt"):
                in_pair = False
            elif l.startswith("s_nop") and not in_pair:
                outside += 1
        print(f"    s_nop outside a v_cmpx -> v_mbcnt pair: {outside}")
        if want_ops:
            for op, nops in sorted(ops.items(), key=lambda kv: (-kv[1], kv[0])):
                print(f"      {op:34s}{nops:5d}{('   (+' + str(opsb[op]) + ')') if opsb[op] else ''}")
            for op, nops in sorted(opsb.items()):
                if op not in ops:
                    print(f"      {op:34s}{0:5d}   (+{nops})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dump")
    ap.add_argument("kernel")
    ap.add_argument("--opcodes", action="store_true", help="per-opcode counts as well")
    args = ap.parse_args()
    lines = open(args.dump).read().splitlines()
    funcs = functions(lines)
    names = demangle(list(funcs))
    hits = [s for s in funcs if args.kernel in s or args.kernel in names[s]]
    if not hits:
        sys.exit(f"no function matching {args.kernel!r} in {args.dump}")
    for s in hits:
        a, b = funcs[s]
        report(s, names[s], lines[a:b], args.opcodes)
        print()


if __name__ == "__main__":
    main()
