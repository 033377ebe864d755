#!/usr/bin/env python
"""Which kernel instances of the library does a run launch?

    python tools/instance_coverage.py lmcache_amd/csrc/kernel_resources.json TRACE [TRACE ...] [--title TEXT]

kernel_resources.json is the instance list of the build (native.build() writes it, names demangled).  A TRACE is a rocpd
sqlite database of a `rocprofv3 --kernel-trace` run, or a directory that is searched for `*.db`: a traced pytest run
writes one database per process, so give them all (or their directory).  The `kernels` view is read, as
tools/rocpd_stats.py reads it.

Output (stdout): a markdown table -- per family the instances of the build and how many of them the traces hold at least
one dispatch of -- and below it every unlaunched instance by its full name.

Names are normalised on both sides (a leading `void `, the argument list, a `.kd` suffix, spacing, the cast in front of
an enumerator).  A traced kernel whose name starts with `k_` and matches NO instance of the build is an error (exit
status 1, the names on stderr): a naming mismatch must not read as "nothing covered", and must not be dropped either.

The trace is a run of its own, never part of a test: kernel tracing alone (no `--pmc`), the program behind `--`, under a
time limit, for example one database directory per test file:

    timeout 600 rocprofv3 --kernel-trace -f rocpd -d traces/test_gpu_instances -- \\
        python -m pytest -m gpu -q tests/test_gpu_instances.py
    python tools/instance_coverage.py lmcache_amd/csrc/kernel_resources.json traces/test_gpu_instances
"""
import glob
import json
import os
import re
import sqlite3
import sys
from collections import Counter, OrderedDict


def normalise(name):
    """`void k_decode<0, 3, 0>(DecodeArgs) [clone .kd]` -> `k_decode<0,3,0>`."""
    s = name.strip()
    s = re.sub(r"\s*\[clone[^\]]*\]\s*$", "", s)
    if s.endswith(".kd"):
        s = s[:-3]
    if s.startswith("void "):
        s = s[5:]
    if s.endswith(")"):  # the argument list: the last parenthesis at depth 0 (angle brackets may hold casts)
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += s[i] == ")"
            depth -= s[i] == "("
            if depth == 0:
                s = s[:i]
                break
    s = re.sub(r"\([A-Za-z_][\w:]*\)(?=-?\d)", "", s)  # (DecSink)0 -> 0
    return re.sub(r"\s+", "", s)


def family(norm):
    return norm.split("<", 1)[0]


def instances(resources_path):
    """normalised name -> the name as the build has it, in the file's order."""
    out = OrderedDict()
    for k in json.load(open(resources_path)):
        n = normalise(k)
        if n in out:
            raise SystemExit(f"{resources_path}: `{k}` and `{out[n]}` normalise to the same name `{n}`")
        out[n] = k
    return out


def databases(paths):
    out = []
    for p in paths:
        if os.path.isdir(p):
            found = sorted(glob.glob(os.path.join(p, "**", "*.db"), recursive=True))
            if not found:
                raise SystemExit(f"{p}: no *.db below it")
            out += found
        else:
            out.append(p)
    return out


def dispatches(db_paths):
    """normalised kernel name -> dispatches, summed over the databases."""
    n = Counter()
    for p in db_paths:
        db = sqlite3.connect(f"file:{p}?mode=ro", uri=True)
        try:
            for name, calls in db.execute("select name, count(*) from kernels group by name"):
                n[normalise(name)] += calls
        finally:
            db.close()
    return n


def coverage(inst, seen):
    """-> (rows [(family, instances, launched)], unlaunched full names, traced k_ names that no instance matches)."""
    unknown = sorted(k for k in seen if k.startswith("k_") and k not in inst)
    fam = OrderedDict()
    for n in inst:
        row = fam.setdefault(family(n), [0, 0])
        row[0] += 1
        row[1] += seen.get(n, 0) > 0
    rows = sorted(((f, a, b) for f, (a, b) in fam.items()), key=lambda r: (-r[1], r[0]))
    return rows, [inst[n] for n in inst if not seen.get(n, 0)], unknown


def render(title, rows, missing, ndb):
    total, hit = sum(r[1] for r in rows), sum(r[2] for r in rows)
    out = [f"## {title}", "", f"{ndb} trace database(s); {hit} of {total} instances launched, {total - hit} never.", "",
           "| family | instances | launched |", "|---|---|---|"]
    out += [f"| `{f}` | {a} | {b} |" for f, a, b in rows]
    out += [f"| **all** | {total} | {hit} |", ""]
    if missing:
        out.append("Not launched:")
        out.append("")
        out += [f"- `{m}`" for m in missing]
    else:
        out.append("Every instance was launched.")
    return "\n".join(out) + "\n"


def main(argv):
    args, title = [], None
    i = 1
    while i < len(argv):
        if argv[i] == "--title" and i + 1 < len(argv):
            title = argv[i + 1]
            i += 2
        elif argv[i].startswith("-"):
            raise SystemExit(__doc__)
        else:
            args.append(argv[i])
            i += 1
    if len(args) < 2:
        raise SystemExit(__doc__)
    inst = instances(args[0])
    dbs = databases(args[1:])
    rows, missing, unknown = coverage(inst, dispatches(dbs))
    if unknown:
        sys.stderr.write("traced kernels that match no instance of the build:\n" + "".join(f"  {u}\n" for u in unknown))
        return 1
    sys.stdout.write(render(title or "Kernel instances launched", rows, missing, len(dbs)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
