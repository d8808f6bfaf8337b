"""The commitments of device columns (hsw_gadget_msm) without a GPU: the model over Python integers that the GPU tests
import (tests/msm_model.py: bases with known discrete logs, so that a commitment is ONE multiplication), proven here
against the term-by-term definition, the public surface (one symbol with one signature in the header, in _native.py and
in hsw-sys, two structs, the ABI numbers unchanged, the new kernels in libhsw.so), the argument rules of the Python
wrapper, and three stand-alone programs under ASan + UBSan: tests/cpp/g1_check.cpp (Fq and the complete formulas against
shift-and-add and affine arithmetic), tests/cpp/msm_value_check.cpp (the launches of csrc/hsw_msm_value.hpp run on the
CPU against double-and-add) and, with the stand-in HIP runtime and LeakSanitizer, tests/cpp/msm_lifecycle.cpp (refusals,
the plan, launches, scratch, groups)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from tests.constraint_check import P_INT
from tests.msm_model import G, Q_INT, add, cell_words, chain, commitment, msm_definition, mul, neg, plan, point_words, words_point
from tests.test_host_sanitizers import CSRC, ROOT, _compile, _hipcc, _link_and_run, host_objects  # noqa: F401 (fixture)


# ---- the model (tests/msm_model.py) against the definition ----------------------------------------------------------
def test_the_curve_of_the_model():
    assert mul(P_INT, G) is None and mul(P_INT - 1, G) == neg(G) and add(G, neg(G)) is None   # r G = O: the order is the Fr modulus
    assert add(G, G) == mul(2, G) and add(mul(5, G), mul(7, G)) == mul(12, G)
    for p in (G, mul(123456789, G)):
        assert (p[1] ** 2 - p[0] ** 3 - 3) % Q_INT == 0
        assert words_point(point_words(p)) == p
    assert point_words(None) == [0] * 8 and words_point([0] * 8) is None
    assert cell_words(5, False) == [5, 0, 0, 0] and cell_words(1, True)[0] == ((1 << 256) % P_INT) & (2**64 - 1)


@pytest.mark.parametrize("rows", [0, 1, 2, 17, 64])
def test_the_model_is_the_definition(rows):
    import random
    rng = random.Random(500 + rows)
    pts, logs = [], []
    for n in (rows // 3, rows - rows // 3):                                  # two chains
        p, k = chain(rng.randrange(1, P_INT), rng.randrange(1, P_INT), n)
        pts += p
        logs += k
    assert all(mul(k, G) == p for p, k in list(zip(pts, logs))[:3])
    if rows >= 17:
        pts[3], logs[3] = None, None                                         # an identity base
        pts[5], logs[5] = pts[4], logs[4]                                    # duplicates
        pts[9], logs[9] = neg(pts[8]), (P_INT - logs[8]) % P_INT             # a negated pair
    scalars = [rng.randrange(P_INT) for _ in range(rows)]
    if rows >= 17:
        scalars[0], scalars[1], scalars[2] = 0, 1, P_INT - 1
        scalars[9] = scalars[8]
    assert commitment(scalars, logs) == msm_definition(scalars, pts)
    assert commitment(scalars[:rows // 2], logs) == msm_definition(scalars[:rows // 2], pts)   # input_rows below n_bases


def test_the_plan_of_the_model():
    assert plan(1 << 20) == (8, 32, 4096, 256) and plan(1 << 28) == (8, 32, 1 << 18, 1024) and plan(0, 5, 64) == (5, 51, 64, 1)
    assert plan(300, 1, 64) == (1, 254, 64, 5) and plan(1 << 16) == (8, 32, 4096, 16)


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_symbol_signature_and_abi_numbers(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_VERSION 3\b", header) and re.search(r"#define HSW_ABI_MINOR 1\b", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    name = "hsw_gadget_msm"
    assert name in N.SYMBOLS and N.SYMBOLS.count(name) == 1 and hasattr(lib, name) and lib.hsw_gadget_msm.restype is C.c_int
    assert lib.hsw_gadget_msm.argtypes == [C.c_void_p, C.POINTER(N.Msm), C.POINTER(N.MsmReport)]
    assert len(re.findall(r"\bint hsw_gadget_msm\(", header)) == 1 and len(re.findall(r"pub fn hsw_gadget_msm\(", rs)) == 1
    assert (C.sizeof(N.Msm), C.sizeof(N.MsmReport)) == (72, 80)
    assert [f[0] for f in N.Msm._fields_] == ["flags", "window_bits", "slice_rows", "reserved_", "n_columns", "n_bases", "d_bases", "d_scalars",
                                              "input_rows", "out_points", "status"]
    assert [f[0] for f in N.MsmReport._fields_] == ["columns", "refused_columns", "first_refused", "bad_bases", "first_bad_base", "scratch_bytes",
                                                    "window_bits", "windows", "slice_rows", "slices", "launches", "reserved_", "kernel_ms", "finish_ms"]
    assert (N.HSW_MSM_CELL_NOT_BELOW_P, N.HSW_MSM_BASE_NOT_BELOW_Q) == (4, 8) and N.HSW_MSM_CELL_NOT_BELOW_P == N.HSW_NTT_CELL_NOT_BELOW_P
    assert N.HSW_MSM_MAX_WINDOW_BITS >= 8
    assert re.search(r"#define HSW_MSM_CELL_NOT_BELOW_P 4u\b", header) and re.search(r"#define HSW_MSM_BASE_NOT_BELOW_Q 8u\b", header)
    assert re.search(r"#define HSW_MSM_MAX_WINDOW_BITS %du\b" % N.HSW_MSM_MAX_WINDOW_BITS, header)
    assert re.search(r"int hsw_gadget_msm\(hsw_gadget \*g, const hsw_msm \*args, hsw_msm_report \*report\);", header)
    assert re.search(r"typedef struct hsw_msm \{\s*uint32_t flags, window_bits;[^}]*uint32_t slice_rows, reserved_;[^}]*size_t n_columns;[^}]*"
                     r"uint64_t n_bases;[^}]*const void \*d_bases;[^}]*const void \*const \*d_scalars;[^}]*const uint64_t \*input_rows;[^}]*"
                     r"void \*out_points;[^}]*uint32_t \*status;[^}]*\} hsw_msm;", header)
    assert re.search(r"typedef struct hsw_msm_report \{\s*uint64_t columns, refused_columns, first_refused;[^}]*uint64_t bad_bases, first_bad_base;[^}]*"
                     r"uint64_t scratch_bytes;[^}]*uint32_t window_bits, windows, slice_rows, slices;[^}]*uint32_t launches, reserved_;[^}]*"
                     r"float kernel_ms, finish_ms;[^}]*\} hsw_msm_report;", header)
    assert re.search(r"pub fn hsw_gadget_msm\(g: \*mut hsw_gadget, args: \*const hsw_msm, report: \*mut hsw_msm_report\) -> c_int;", rs)
    assert re.search(r"pub struct hsw_msm \{\s*pub flags: u32,\s*pub window_bits: u32,\s*pub slice_rows: u32,\s*pub reserved_: u32,\s*pub n_columns: usize,\s*"
                     r"pub n_bases: u64,\s*pub d_bases: \*const c_void,\s*pub d_scalars: \*const \*const c_void,\s*pub input_rows: \*const u64,\s*"
                     r"pub out_points: \*mut c_void,\s*pub status: \*mut u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_msm_report \{\s*pub columns: u64,\s*pub refused_columns: u64,\s*pub first_refused: u64,\s*pub bad_bases: u64,\s*"
                     r"pub first_bad_base: u64,\s*pub scratch_bytes: u64,\s*pub window_bits: u32,\s*pub windows: u32,\s*pub slice_rows: u32,\s*"
                     r"pub slices: u32,\s*pub launches: u32,\s*pub reserved_: u32,\s*pub kernel_ms: f32,\s*pub finish_ms: f32,\s*\}", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "msm")
    blob = open(N.LIB_PATH, "rb").read()
    for kernel in (b"hsw_msm_check_kernel", b"hsw_msm_accumulate_kernel", b"hsw_msm_reduce_kernel"):
        assert kernel in blob, kernel                                        # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import torch
    N = hsw._native
    rep = N.MsmReport()
    assert N.lib().hsw_gadget_msm(None, C.byref(N.Msm()), C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    n = 64
    bases = torch.zeros((n, 8), dtype=torch.uint64)
    cols = torch.zeros((3, n, 4), dtype=torch.uint64)
    good = dict(bases=bases, columns=cols)

    def but(**kw):
        d = dict(good)
        d.update(kw)
        return d
    for kw in (but(window_bits=9), but(window_bits=-1), but(slice_rows=32), but(slice_rows=96), but(slice_rows=1 << 29), but(slice_rows=-64),
               but(bases=bases.to(torch.int64)),                                 # dtype
               but(bases=torch.zeros((n, 4), dtype=torch.uint64)),               # (n_bases, 8)
               but(bases=torch.zeros((n * 8,), dtype=torch.uint64)),
               but(bases=torch.zeros((n, 16), dtype=torch.uint64)[:, ::2]),      # not contiguous
               but(bases=torch.zeros((0, 8), dtype=torch.uint64)),               # at least one base
               but(bases=bases.to("meta")),                                      # another device
               but(bases=bases, n_bases=n + 1),                                  # the tensor's own count
               but(bases=4096),                                                  # an address needs n_bases
               but(bases=4096 + 8, n_bases=n),                                   # ... 16-byte aligned
               but(bases=0, n_bases=n),
               but(bases=4096, n_bases=0),
               but(bases=4096, n_bases=(1 << 28) + 1),
               but(bases=(4096, 0)),
               but(columns=cols.to(torch.int64)),
               but(columns=torch.zeros((3, n - 1, 4), dtype=torch.uint64)),      # fewer rows than are read
               but(columns=torch.zeros((3 * n, 4), dtype=torch.uint64)),         # (columns, rows, 4)
               but(columns=torch.zeros((0, n, 4), dtype=torch.uint64)),
               but(columns=torch.zeros((3, n, 8), dtype=torch.uint64)[:, :, ::2]),
               but(columns=cols.to("meta")),
               but(columns=[]),
               but(columns=[16, 32, 8]),                                         # addresses: 16-byte aligned
               but(columns=[16, 32, 0]),
               but(input_rows=[n, n]),
               but(input_rows=[n, n, n + 1]),
               but(input_rows=[n, n, -1])):
        with pytest.raises(ValueError):
            cfg.msm(**kw)
    # a short column tensor must still hold the rows that input_rows declares
    with pytest.raises(ValueError):
        cfg.msm(**but(columns=torch.zeros((3, 10, 4), dtype=torch.uint64), input_rows=[10, 10, 11]))


# ---- the stand-alone programs -------------------------------------------------------------------------------------------
def _standalone(tmp_path, name):
    hipcc = _hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    cxx = clang if os.path.exists(clang) else "g++"
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    return res.stdout


def test_fq_and_the_complete_formulas_under_asan_ubsan(tmp_path):
    got = re.search(r"g1 check ok: (\d+) field checks, (\d+) curve checks", _standalone(tmp_path, "g1_check"))
    assert got and int(got.group(1)) == 200 * 7 + 12 and int(got.group(2)) == 12 * 19


def test_msm_launches_on_the_cpu_under_asan_ubsan(tmp_path):
    got = re.search(r"msm value check ok: (\d+) runs", _standalone(tmp_path, "msm_value_check"))
    # per height and cell form: every window_bits 1 .. 8 at slice_rows 64 and the library's plan; and the lone negated pair
    assert got and int(got.group(1)) == 6 * 2 * (8 + 1) + 1


def test_msm_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, "hsw_msm.o")]                    # (the entry point refers to these kernels alone)
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_msm.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "msm_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "msm_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "msm lifecycle ok" in res.stdout
