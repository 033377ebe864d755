"""Builds and loads tests/csrc/arith_harness.hip: test-only kernels that call the product's device helpers one by one
(row_div_short, quant_z2, divmod_est, rne_div_u32, cdf_column_to_lds, transpose64, ...) so that
tests/test_gpu_device_arith.py can hold each of them, over every input it can meet, against a reference that shares no
code with it.

The harness is compiled with native.HIPCC_FLAGS as they are -- the optimisation level, -ffp-contract=off and whatever
else the library is built with -- so the helpers are lowered as they are inside the library.  Only the resource remark
of native.build() is left out (nothing reads it here)."""
import ctypes
import os
import subprocess
import sys

from lmcache_amd import native

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "arith_harness.hip")
SO_PATH = os.path.join(_HERE, "csrc", "_arith_harness.so")

_vp, _i32, _i64, _f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
# name -> argument types in front of the trailing (count, stream); every entry returns the launch's hipError_t
ENTRIES = {
    "ah_row_factor": [_vp, _vp, _i32, _vp, _vp, _vp],
    "ah_quant_pair": [_vp, _vp, _vp, _f32, _vp],
    "ah_quant_single": [_vp, _vp, _vp, _f32, _vp, _vp],
    "ah_quant_special": [_vp, _vp, _vp, _vp, _vp],
    "ah_rans": [_vp, _vp, _vp, _vp, _vp, _vp],
    "ah_rne_div": [_vp, _vp, _vp, _vp],
    "ah_cdf_column": [_vp, _vp, _vp, _vp],
    "ah_cdf_column_wide": [_vp, _vp, _vp, _vp],
    "ah_divmod_small": [_vp, _vp, _vp, _vp, _vp],
    "ah_split_divmod": [_vp, _vp, _vp, _vp, _vp],
    "ah_counts_scale": [_vp, _vp, _vp, _vp],
    "ah_f2bf16": [_vp, _vp],
    "ah_f2fp16": [_vp, _vp],
    "ah_h2f": [_vp, _i32, _vp],
    "ah_transpose64": [_vp, _vp],
}

_lib = None


def _sources():
    srcs = [SRC]
    for d in (native.CSRC, native.INCLUDE):
        srcs += [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hip", ".h"))]
    return srcs


def hipcc() -> str:
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def command(out: str = SO_PATH, extra=()) -> list:
    """The compile line: the library's flags verbatim (extra: more flags behind them, for experiments)."""
    return [hipcc()] + list(native.HIPCC_FLAGS) + list(extra) + [SRC, "-o", out]


def build(force: bool = False) -> str:
    """Compile the harness in-tree when it is missing or older than its source or any of the library's sources."""
    newest = max(os.path.getmtime(s) for s in _sources())
    if force or not os.path.exists(SO_PATH) or os.path.getmtime(SO_PATH) < newest:
        if not os.path.exists(hipcc()):
            if os.path.exists(SO_PATH):
                raise RuntimeError(f"{SO_PATH} is older than the sources it was built from and there is no hipcc ({hipcc()}) to rebuild it")
            raise RuntimeError(f"{SO_PATH} is missing and there is no hipcc ({hipcc()}) to build it: the device arithmetic "
                               "tests cannot run (python -c 'import __graft_entry__ as g; g.build()' on a box with ROCm builds it)")
        cmd = command()
        proc = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr)
            raise subprocess.CalledProcessError(proc.returncode, cmd)
        if "warning:" in proc.stderr:
            sys.stderr.write(proc.stderr)
    return SO_PATH


def lib() -> ctypes.CDLL:
    """The loaded harness (built by build()); raises when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} is missing: call tests.arith_harness.build() first")
        import torch  # noqa: F401  (its libamdhip64 first, as native.py does: one HIP runtime per process)
        L = ctypes.CDLL(SO_PATH)
        for name, args in ENTRIES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ctypes.c_int, args + [_i64, _vp]
        _lib = L
    return _lib


def call(name: str, *args, n: int) -> None:
    """Launch entry `name` on the current torch stream; tensors are passed as their device pointers."""
    import torch
    raw = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(lib(), name)(*raw, int(n), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"{name}: launch failed with hipError_t {rc}")
