"""The instance list of tests/test_gpu_instances.py stays complete, without a GPU: every instance the build holds of the
five families whose instance lmc_api.hip picks from a width, a dtype or a kind (k_quantize, k_encode_fused,
k_fixed_encode, k_decode, k_fixed_decode) has a case in that file's MATRIX or stands in its UNREACHABLE list with the
line of lmc_api.hip that builds it.  An instance added later without a case fails here.  Below that,
tools/instance_coverage.py (which instances a traced run launched) on databases made here: no test runs a profiler."""
import json
import os
import re

import pytest

from tests import test_gpu_instances as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["k_quantize", "k_encode_fused", "k_fixed_encode", "k_decode", "k_fixed_decode"]


def _parse(name):
    """`void k_decode<0, 3, 2>(DecodeArgs)` -> ("k_decode", (0, 3, 2)); None for a kernel without template arguments."""
    m = re.match(r"(?:void )?(\w+)<([^<>]*)>\(", name)
    if not m:
        return None
    args = tuple(a.strip() == "true" if a.strip() in ("true", "false") else int(a) for a in m.group(2).split(","))
    return m.group(1), args


def _built():
    from lmcache_amd import native
    native.build()
    if not os.path.exists(native.RESOURCES_PATH):
        pytest.skip("the library was not compiled here (prebuilt): no kernel_resources.json")
    names = [k for k in json.load(open(native.RESOURCES_PATH)) if any(re.search(r"\b" + f + r"\b", k) for f in FAMILIES)]
    out = [_parse(k) for k in names]
    assert all(i and i[0] in FAMILIES for i in out), "a kernel name of the five families that _parse cannot read"
    return out


def test_parse_reads_the_builds_names():
    assert _parse("void k_quantize<64, 2, 3, true, 4, false>(QuantArgs)") == ("k_quantize", (64, 2, 3, True, 4, False))
    assert _parse("void k_fixed_decode<1, 2>(FixedDecArgs)") == ("k_fixed_decode", (1, 2))
    assert _parse("k_fixed_layers_finish(FixedFinishArgs)") is None


def test_every_instance_of_the_five_families_has_a_case_or_is_declared_unreachable():
    built = _built()
    assert {i[0] for i in built} == set(FAMILIES), "a family the build no longer holds"
    missing = [i for i in built if i not in gi.MATRIX and i not in gi.UNREACHABLE]
    assert not missing, f"instances without a case in tests/test_gpu_instances.py: {missing}"
    both = [i for i in gi.MATRIX if i in gi.UNREACHABLE]
    assert not both, f"declared unreachable AND given a case: {both}"
    for inst, cases in gi.MATRIX.items():
        assert inst[0] in FAMILIES and cases, inst


def test_the_matrix_and_the_unreachable_list_name_only_instances_the_build_holds():
    built = set(_built())
    stale = [i for i in list(gi.MATRIX) + list(gi.UNREACHABLE) if i not in built]
    assert not stale, f"rows for instances the library does not hold: {stale}"


def test_every_case_of_the_matrix_is_a_case_of_the_file():
    ids = set()
    for name in dir(gi):
        fn = getattr(gi, name)
        if not name.startswith("test_") or not callable(fn):
            continue
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        if not marks:
            ids.add(name)
        for m in marks:
            ids.update(p.id for p in m.args[1])
    named = {c for cases in gi.MATRIX.values() for c in cases}
    assert named <= ids, sorted(named - ids)


def test_the_unreachable_list_is_the_eight_wide_quad_instances_and_names_the_lines_that_build_them():
    """launch_quant_dt chooses between SPLIT and NITER 4 / 8 with a plain `if (QUAD)`, so QUAD = true builds the NITER 4 / 8
    arm too (HISTORY.md); the list may only grow by instances shown unreachable the same way: by reading the line."""
    assert sorted(gi.UNREACHABLE) == sorted(("k_quantize", (64, n, dt, True, 1, False)) for n in (4, 8) for dt in range(4))
    src = [" ".join(l.split()) for l in open(os.path.join(ROOT, "lmcache_amd", "csrc", "lmc_api.hip"))]
    for inst, line in gi.UNREACHABLE.items():
        assert any(line in l for l in src), (inst, line)
    # the arm those lines stand in is the one a QUAD launch never takes
    text = "\n".join(src)
    assert re.search(r"\} else if \(QUAD\) \{.*?\} else \{\s*if \(C <= 2048\) launch\(g64, IntTag<4>\{\}, IntTag<1>\{\}\);", text, re.S)


# ------------------------------------------------------------------ tools/instance_coverage.py
def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("instance_coverage", os.path.join(ROOT, "tools", "instance_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trace(path, names):
    """A database with the one thing the tool reads of a rocpd trace: `kernels`, a row per dispatch."""
    import sqlite3
    db = sqlite3.connect(str(path))
    db.execute("create table kernels (name text, duration integer)")
    db.executemany("insert into kernels values (?, 1)", [(n,) for n in names])
    db.commit()
    db.close()
    return str(path)


def test_the_coverage_tool_normalises_names_sums_databases_and_refuses_unknown_kernels(tmp_path, capsys):
    tool = _tool()
    assert tool.normalise("void k_decode<0, 3, 2>(DecodeArgs)") == "k_decode<0,3,2>"
    assert tool.normalise("k_decode<0,3,2>(DecodeArgs).kd") == "k_decode<0,3,2>"
    assert tool.normalise("void k_decode<(DecSink)0, 3, 2>(DecodeArgs) [clone .kd]") == "k_decode<0,3,2>"
    assert tool.normalise("k_set_kv_dtype(unsigned char*, long long, int, unsigned int)") == "k_set_kv_dtype"
    assert tool.normalise("k_offload.kd") == "k_offload"
    res = tmp_path / "kernel_resources.json"
    res.write_text(json.dumps({"void k_decode<0, 3, 2>(DecodeArgs)": {}, "void k_decode<0, 0, 0>(DecodeArgs)": {},
                               "k_offload(OffloadArgs)": {}}))
    # two databases of one run (a process each), a directory of them, spellings that differ from the build's
    a = _trace(tmp_path / "a_results.db", ["void k_decode<0,3,2>(DecodeArgs)", "void at::native::vectorized_elementwise_kernel<4>(int)"])
    sub = tmp_path / "more"
    sub.mkdir()
    _trace(sub / "b_results.db", ["k_offload.kd", "k_offload.kd"])
    assert tool.main(["x", str(res), a, str(sub), "--title", "T"]) == 0
    out = capsys.readouterr().out
    assert "## T" in out and "| `k_decode` | 2 | 1 |" in out and "| `k_offload` | 1 | 1 |" in out and "| **all** | 3 | 2 |" in out
    assert "- `void k_decode<0, 0, 0>(DecodeArgs)`" in out and "k_decode<0, 3, 2>" not in out
    # a k_ kernel that matches no instance of the build is an error, not a zero
    bad = _trace(tmp_path / "c_results.db", ["void k_decode<0, 9, 9>(DecodeArgs)"])
    assert tool.main(["x", str(res), a, bad]) == 1
    cap = capsys.readouterr()
    assert "k_decode<0,9,9>" in cap.err and cap.out == ""
