"""The Fr NTT of device columns (hsw_gadget_ntt) without a GPU: the model over Python integers that the GPU tests
import (tests/ntt_model.py, a recursive radix-2 transform), proven here against the O(N^2) definition, the public surface (one symbol
with one signature in the header, in _native.py and in hsw-sys, two structs, the ABI numbers unchanged, the new kernels
in libhsw.so), the argument rules of the Python wrapper, and two stand-alone programs under ASan + UBSan:
tests/cpp/ntt_value_check.cpp (the launches of csrc/hsw_ntt_value.hpp run point for point on the CPU against the direct
sum) and, with the stand-in HIP runtime and LeakSanitizer, tests/cpp/ntt_lifecycle.cpp (refusals, launch counts, groups,
scratch, the twiddle cache, overlaps)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from tests.constraint_check import P_INT
from tests.ntt_model import default_launches, dft, ntt_definition, ntt_model, root_of_unity  # noqa: F401
from tests.test_host_sanitizers import CSRC, ROOT, _compile, _hipcc, _link_and_run, host_objects  # noqa: F401 (fixture)


# ---- the model (tests/ntt_model.py) against the definition ----------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 2, 3, 5, 8])
def test_the_model_is_the_definition(log_n):
    import random
    rng = random.Random(1000 + log_n)
    n, w = 1 << log_n, root_of_unity(log_n)
    g, c = rng.randrange(2, P_INT), rng.randrange(2, P_INT)
    for rows in sorted({0, 1, max(0, n - 5), n}):
        a = [rng.randrange(P_INT) for _ in range(rows)]
        for kw in (dict(), dict(shift=g), dict(scale=c), dict(shift=g, scale=c), dict(shift=g, shift_after=True),
                   dict(shift=g, scale=c, shift_after=True)):
            assert ntt_model(a, log_n, w, **kw) == ntt_definition(a, log_n, w, **kw), (rows, kw)
    a = [rng.randrange(P_INT) for _ in range(n)]                          # and back: the inverse root and 1 / N
    coeff = ntt_model(a, log_n, pow(w, -1, P_INT), scale=pow(n, -1, P_INT))
    assert ntt_model(coeff, log_n, w) == a


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_symbol_signature_and_abi_numbers(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_VERSION 3\b", header) and re.search(r"#define HSW_ABI_MINOR 1\b", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    name = "hsw_gadget_ntt"
    assert name in N.SYMBOLS and hasattr(lib, name) and lib.hsw_gadget_ntt.restype is C.c_int
    assert lib.hsw_gadget_ntt.argtypes == [C.c_void_p, C.POINTER(N.Ntt), C.POINTER(N.NttReport)]
    assert (C.sizeof(N.Ntt), C.sizeof(N.NttReport)) == (80, 64)
    assert [f[0] for f in N.Ntt._fields_] == ["flags", "log_n", "pass_log", "reserved_", "n_columns", "d_inputs", "input_rows", "d_outputs",
                                              "omega", "shift", "scale", "status"]
    assert [f[0] for f in N.NttReport._fields_] == ["columns", "written", "refused_columns", "first_refused", "twiddle_bytes", "scratch_bytes",
                                                    "launches", "pass_log", "kernel_ms", "twiddle_ms"]
    assert (N.HSW_NTT_SHIFT_AFTER, N.HSW_NTT_CELL_NOT_BELOW_P) == (1, 4) and N.HSW_NTT_CELL_NOT_BELOW_P == N.HSW_PRODUCT_CELL_NOT_BELOW_P
    assert re.search(r"#define HSW_NTT_SHIFT_AFTER 1u\b", header) and re.search(r"#define HSW_NTT_CELL_NOT_BELOW_P 4u\b", header)
    assert re.search(r"int hsw_gadget_ntt\(hsw_gadget \*g, const hsw_ntt \*args, hsw_ntt_report \*report\);", header)
    assert re.search(r"typedef struct hsw_ntt \{\s*uint32_t flags, log_n;[^}]*uint32_t pass_log, reserved_;[^}]*size_t n_columns;[^}]*"
                     r"const void \*const \*d_inputs;[^}]*const uint64_t \*input_rows;[^}]*void \*const \*d_outputs;[^}]*"
                     r"const void \*omega, \*shift, \*scale;[^}]*uint32_t \*status;[^}]*\} hsw_ntt;", header)
    assert re.search(r"typedef struct hsw_ntt_report \{\s*uint64_t columns, written, refused_columns, first_refused;[^}]*"
                     r"uint64_t twiddle_bytes, scratch_bytes;[^}]*uint32_t launches, pass_log;[^}]*float kernel_ms, twiddle_ms;[^}]*"
                     r"\} hsw_ntt_report;", header)
    assert re.search(r"pub fn hsw_gadget_ntt\(g: \*mut hsw_gadget, args: \*const hsw_ntt, report: \*mut hsw_ntt_report\) -> c_int;", rs)
    assert re.search(r"pub struct hsw_ntt \{\s*pub flags: u32,\s*pub log_n: u32,\s*pub pass_log: u32,\s*pub reserved_: u32,\s*pub n_columns: usize,\s*"
                     r"pub d_inputs: \*const \*const c_void,\s*pub input_rows: \*const u64,\s*pub d_outputs: \*const \*mut c_void,\s*"
                     r"pub omega: \*const c_void,\s*pub shift: \*const c_void,\s*pub scale: \*const c_void,\s*pub status: \*mut u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_ntt_report \{\s*pub columns: u64,\s*pub written: u64,\s*pub refused_columns: u64,\s*pub first_refused: u64,\s*"
                     r"pub twiddle_bytes: u64,\s*pub scratch_bytes: u64,\s*pub launches: u32,\s*pub pass_log: u32,\s*pub kernel_ms: f32,\s*"
                     r"pub twiddle_ms: f32,\s*\}", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "ntt")
    blob = open(N.LIB_PATH, "rb").read()
    for kernel in (b"hsw_ntt_kernel", b"hsw_ntt_twiddle_kernel"):
        assert kernel in blob, kernel                                        # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import numpy as np
    import torch
    N = hsw._native
    rep = N.NttReport()
    assert N.lib().hsw_gadget_ntt(None, C.byref(N.Ntt()), C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    log_n, n = 6, 64
    cols = torch.zeros((3, n, 4), dtype=torch.uint64)
    good = dict(omega=root_of_unity(log_n), columns=cols, out=torch.zeros((3, n, 4), dtype=torch.uint64))

    def but(**kw):
        d = dict(good)
        d.update(kw)
        return d
    for k, kw in ((0, good), (29, good), (log_n, but(pass_log=11)), (log_n, but(pass_log=-1)),
                  (log_n, but(omega=None)),
                  (log_n, but(omega=[1, 2])),                                    # one element
                  (log_n, but(shift=np.zeros((2, 4), dtype=np.uint64))),
                  (log_n, but(scale=[1, 2, 3])),
                  (log_n, but(columns=cols.to(torch.int64))),                    # dtype
                  (log_n, but(columns=torch.zeros((3, n - 1, 4), dtype=torch.uint64))),   # fewer rows than are read
                  (log_n, but(columns=torch.zeros((2, n, 4), dtype=torch.uint64))),       # one output per column
                  (log_n, but(columns=torch.zeros((3 * n, 4), dtype=torch.uint64))),      # (columns, rows, 4)
                  (log_n, but(columns=torch.zeros((0, n, 4), dtype=torch.uint64))),
                  (log_n, but(columns=[])),
                  (log_n, but(out=torch.zeros((3, n - 1, 4), dtype=torch.uint64))),       # an output has N rows
                  (log_n, but(out=torch.zeros((3, n, 8), dtype=torch.uint64)[:, :, ::2])),   # not contiguous
                  (log_n, but(out=cols.to("meta"))),                             # another device
                  (log_n, but(out=[16, 32])),                                    # addresses: one per column
                  (log_n, but(columns=[16, 32, 8])),                             # ... 16-byte aligned
                  (log_n, but(columns=[16, 32, 0])),
                  (log_n, but(input_rows=[n, n])),
                  (log_n, but(input_rows=[n, n, n + 1])),
                  (log_n, but(input_rows=[n, n, -1]))):
        with pytest.raises(ValueError):
            cfg.ntt(k, **kw)
    # a short column tensor must still hold the rows that input_rows declares
    with pytest.raises(ValueError):
        cfg.ntt(log_n, **but(columns=torch.zeros((3, 10, 4), dtype=torch.uint64), input_rows=[10, 10, 11]))


# ---- the stand-alone programs -------------------------------------------------------------------------------------------
def test_ntt_launches_point_for_point_under_asan_ubsan(tmp_path):
    hipcc = _hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    cxx = clang if os.path.exists(clang) else "g++"
    exe = str(tmp_path / "ntt_value_check")
    r = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "ntt_value_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    got = re.search(r"ntt value check ok: (\d+) points, (\d+) transforms", res.stdout)
    # per log_n: its heights x 11 pass_logs (the default and 1 .. 10) x 2 cell forms x 4 kinds of shift and scale
    heights = sum(len({0, 1, max(0, (1 << k) - 5), 1 << k}) for k in range(1, 13))
    # ... and the default plan at log_n 15 and 16 (digits of 8 bits), 2 cell forms x 2 flags, sampled rows
    assert got and int(got.group(2)) == heights * 11 * 2 * 4 + 2 * 2 * 2 and int(got.group(1)) > 2000000


def test_ntt_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, "hsw_ntt.o")]                    # (the entry point refers to these kernels alone)
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_ntt.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "ntt_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "ntt_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "ntt lifecycle ok" in res.stdout
