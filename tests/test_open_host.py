"""Evaluating and opening device columns (hsw_gadget_evaluate, hsw_gadget_open) without a GPU: the model over Python
integers that the GPU tests import (tests/open_model.py), proven here against the term-by-term definitions and the
identity c(X) - c(z) = (X - z) q(X); the public surface (one symbol each with one signature in the header, in
_native.py and in hsw-sys, four structs, the ABI numbers unchanged, the new kernels in libhsw.so); the argument rules of
the Python wrapper; and two stand-alone programs under ASan + UBSan: tests/cpp/open_value_check.cpp (the launches of
csrc/hsw_open_value.hpp run on the CPU against the plain recurrence) and, with the stand-in HIP runtime and
LeakSanitizer, tests/cpp/open_lifecycle.cpp (refusals, geometry, launches, scratch, batches)."""
import ctypes as C
import os
import random
import re
import subprocess
import types

import pytest

from tests.constraint_check import P_INT
from tests.open_model import evaluate_definition, evaluate_model, fold_model, open_definition, open_model
from tests.test_host_sanitizers import CSRC, ROOT, _compile, _hipcc, _link_and_run, host_objects  # noqa: F401 (fixture)


# ---- the model (tests/open_model.py) against the definition ---------------------------------------------------------
def _columns(rng, rows):
    heights = [rows, rows - 1, min(1, rows), 0, rows]
    cols = [[rng.randrange(P_INT) for _ in range(h)] for h in heights]
    cols[0][0] = P_INT - 1
    if rows >= 3:
        cols[0][1], cols[0][2] = 0, 1
    return cols


@pytest.mark.parametrize("rows", [1, 2, 3, 17, 64])
def test_the_model_is_the_definition(rows):
    rng = random.Random(700 + rows)
    cols = _columns(rng, rows)
    for z in (0, 1, P_INT - 1, rng.randrange(P_INT)):
        for a in cols:
            assert evaluate_model(a, z) == evaluate_definition(a, z, rows)
        for v in (0, 1, rng.randrange(P_INT)):
            for group in (cols[:1], cols[1:2], cols[:3], cols[3:], cols[::-1], [cols[3]]):
                q, ev = open_model(group, z, v, rows)
                dq, dev, dc = open_definition(group, z, v, rows)
                assert q == dq and ev == dev and dc == fold_model(group, v, rows)
                assert len(q) == rows and q[rows - 1] == 0 and ev == (dc[0] + z * q[0]) % P_INT
                if len(group) == 1:
                    assert ev == evaluate_model(group[0], z)


@pytest.mark.parametrize("rows", [1, 2, 3, 17, 64])
def test_the_quotient_identity_at_a_random_point(rows):
    rng = random.Random(800 + rows)
    cols = _columns(rng, rows)
    for z in (0, 1, P_INT - 1, rng.randrange(P_INT)):
        v, x = rng.randrange(P_INT), rng.randrange(P_INT)
        q, ev = open_model(cols, z, v, rows)
        c = fold_model(cols, v, rows)
        assert (evaluate_model(c, x) - ev) % P_INT == (x - z) * evaluate_model(q, x) % P_INT    # c(X) - c(z) = (X - z) q(X)
        # subtracting the evaluation first changes c[0] alone, which the quotient never reads
        q2, ev2 = open_model([[(c[0] - ev) % P_INT] + c[1:]], z, 0, rows)
        assert q2 == q and ev2 == 0


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_symbol_signature_and_abi_numbers(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_VERSION 3\b", header) and re.search(r"#define HSW_ABI_MINOR 1\b", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    for name, arg, rep in (("hsw_gadget_evaluate", N.Evaluate, N.EvaluateReport), ("hsw_gadget_open", N.Open, N.OpenReport)):
        assert name in N.SYMBOLS and N.SYMBOLS.count(name) == 1 and hasattr(lib, name) and getattr(lib, name).restype is C.c_int
        assert getattr(lib, name).argtypes == [C.c_void_p, C.POINTER(arg), C.POINTER(rep)]
        assert len(re.findall(r"\bint %s\(" % name, header)) == 1 and len(re.findall(r"pub fn %s\(" % name, rs)) == 1
    assert (C.sizeof(N.Evaluate), C.sizeof(N.EvaluateReport), C.sizeof(N.Open), C.sizeof(N.OpenReport)) == (96, 72, 104, 72)
    assert [f[0] for f in N.Evaluate._fields_] == ["flags", "tile_rows", "rows", "n_columns", "d_columns", "input_rows", "n_points", "points",
                                                   "n_queries", "query_column", "query_point", "out_evals", "status"]
    assert [f[0] for f in N.EvaluateReport._fields_] == ["columns", "queries", "refused_columns", "refused_queries", "first_refused", "scratch_bytes",
                                                         "tile_rows", "tiles", "thread_rows", "launches", "kernel_ms", "reserved_"]
    assert [f[0] for f in N.Open._fields_] == ["flags", "tile_rows", "rows", "n_columns", "d_columns", "input_rows", "n_groups", "group_first",
                                               "group_columns", "points", "challenges", "d_quotients", "out_evals", "status"]
    assert [f[0] for f in N.OpenReport._fields_] == ["groups", "written", "refused_groups", "first_refused", "scratch_bytes", "tile_rows", "tiles",
                                                     "thread_rows", "launches", "batches", "reserved_", "kernel_ms", "reserved2_"]
    assert N.HSW_OPEN_CELL_NOT_BELOW_P == 4 == N.HSW_NTT_CELL_NOT_BELOW_P and N.HSW_OPEN_MIN_TILE_ROWS <= 256 and N.HSW_OPEN_THREAD_ROWS >= 1
    assert re.search(r"#define HSW_OPEN_CELL_NOT_BELOW_P 4u\b", header)
    assert re.search(r"#define HSW_OPEN_MIN_TILE_ROWS %du\b" % N.HSW_OPEN_MIN_TILE_ROWS, header)
    assert re.search(r"#define HSW_OPEN_THREAD_ROWS %du\b" % N.HSW_OPEN_THREAD_ROWS, header)
    assert re.search(r"pub const HSW_OPEN_MIN_TILE_ROWS: u32 = %d;" % N.HSW_OPEN_MIN_TILE_ROWS, rs)
    assert re.search(r"pub const HSW_OPEN_THREAD_ROWS: u32 = %d;" % N.HSW_OPEN_THREAD_ROWS, rs) and re.search(r"pub const HSW_OPEN_CELL_NOT_BELOW_P: u32 = 4;", rs)
    assert re.search(r"int hsw_gadget_evaluate\(hsw_gadget \*g, const hsw_evaluate \*args, hsw_evaluate_report \*report\);", header)
    assert re.search(r"int hsw_gadget_open\(hsw_gadget \*g, const hsw_open \*args, hsw_open_report \*report\);", header)
    assert re.search(r"typedef struct hsw_evaluate \{\s*uint32_t flags, tile_rows;[^}]*uint64_t rows;[^}]*size_t n_columns;[^}]*const void \*const \*d_columns;[^}]*"
                     r"const uint64_t \*input_rows;[^}]*size_t n_points;[^}]*const void \*points;[^}]*size_t n_queries;[^}]*const uint32_t \*query_column;[^}]*"
                     r"const uint32_t \*query_point;[^}]*void \*out_evals;[^}]*uint32_t \*status;[^}]*\} hsw_evaluate;", header)
    assert re.search(r"typedef struct hsw_evaluate_report \{\s*uint64_t columns, queries, refused_columns, refused_queries, first_refused;[^}]*"
                     r"uint64_t scratch_bytes;[^}]*uint32_t tile_rows, tiles, thread_rows, launches;[^}]*float kernel_ms;[^}]*uint32_t reserved_;[^}]*"
                     r"\} hsw_evaluate_report;", header)
    assert re.search(r"typedef struct hsw_open \{\s*uint32_t flags, tile_rows;[^}]*uint64_t rows;[^}]*size_t n_columns;[^}]*const void \*const \*d_columns;[^}]*"
                     r"const uint64_t \*input_rows;[^}]*size_t n_groups;[^}]*const uint64_t \*group_first;[^}]*const uint32_t \*group_columns;[^}]*"
                     r"const void \*points, \*challenges;[^}]*void \*const \*d_quotients;[^}]*void \*out_evals;[^}]*uint32_t \*status;[^}]*\} hsw_open;", header)
    assert re.search(r"typedef struct hsw_open_report \{\s*uint64_t groups, written, refused_groups, first_refused;[^}]*uint64_t scratch_bytes;[^}]*"
                     r"uint32_t tile_rows, tiles, thread_rows, launches;[^}]*uint32_t batches, reserved_;[^}]*float kernel_ms, reserved2_;[^}]*\} hsw_open_report;", header)
    assert re.search(r"pub fn hsw_gadget_evaluate\(g: \*mut hsw_gadget, args: \*const hsw_evaluate, report: \*mut hsw_evaluate_report\) -> c_int;", rs)
    assert re.search(r"pub fn hsw_gadget_open\(g: \*mut hsw_gadget, args: \*const hsw_open, report: \*mut hsw_open_report\) -> c_int;", rs)
    assert re.search(r"pub struct hsw_evaluate \{\s*pub flags: u32,\s*pub tile_rows: u32,\s*pub rows: u64,\s*pub n_columns: usize,\s*"
                     r"pub d_columns: \*const \*const c_void,\s*pub input_rows: \*const u64,\s*pub n_points: usize,\s*pub points: \*const c_void,\s*"
                     r"pub n_queries: usize,\s*pub query_column: \*const u32,\s*pub query_point: \*const u32,\s*pub out_evals: \*mut c_void,\s*"
                     r"pub status: \*mut u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_evaluate_report \{\s*pub columns: u64,\s*pub queries: u64,\s*pub refused_columns: u64,\s*pub refused_queries: u64,\s*"
                     r"pub first_refused: u64,\s*pub scratch_bytes: u64,\s*pub tile_rows: u32,\s*pub tiles: u32,\s*pub thread_rows: u32,\s*pub launches: u32,\s*"
                     r"pub kernel_ms: f32,\s*pub reserved_: u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_open \{\s*pub flags: u32,\s*pub tile_rows: u32,\s*pub rows: u64,\s*pub n_columns: usize,\s*"
                     r"pub d_columns: \*const \*const c_void,\s*pub input_rows: \*const u64,\s*pub n_groups: usize,\s*pub group_first: \*const u64,\s*"
                     r"pub group_columns: \*const u32,\s*pub points: \*const c_void,\s*pub challenges: \*const c_void,\s*pub d_quotients: \*const \*mut c_void,\s*"
                     r"pub out_evals: \*mut c_void,\s*pub status: \*mut u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_open_report \{\s*pub groups: u64,\s*pub written: u64,\s*pub refused_groups: u64,\s*pub first_refused: u64,\s*"
                     r"pub scratch_bytes: u64,\s*pub tile_rows: u32,\s*pub tiles: u32,\s*pub thread_rows: u32,\s*pub launches: u32,\s*pub batches: u32,\s*"
                     r"pub reserved_: u32,\s*pub kernel_ms: f32,\s*pub reserved2_: f32,\s*\}", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "evaluate") and hasattr(hsw.Sha256DynamicConfig, "open")
    blob = open(N.LIB_PATH, "rb").read()
    for kernel in (b"hsw_open_tiles_kernel", b"hsw_evaluate_tiles_kernel", b"hsw_open_scan_kernel", b"hsw_open_write_kernel"):
        assert kernel in blob, kernel                                        # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import torch
    N = hsw._native
    assert N.lib().hsw_gadget_evaluate(None, C.byref(N.Evaluate()), C.byref(N.EvaluateReport())) == N.HSW_ERR_INVALID_ARG
    assert N.lib().hsw_gadget_open(None, C.byref(N.Open()), C.byref(N.OpenReport())) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    n = 64
    cols = torch.zeros((3, n, 4), dtype=torch.uint64)
    shared = [dict(rows=0), dict(rows=(1 << 28) + 1), dict(tile_rows=128), dict(tile_rows=384), dict(tile_rows=1 << 21), dict(tile_rows=-256),
              dict(columns=cols.to(torch.int64)),
              dict(columns=torch.zeros((3, n - 1, 4), dtype=torch.uint64)),      # fewer rows than are read
              dict(columns=torch.zeros((3 * n, 4), dtype=torch.uint64)),         # (columns, rows, 4)
              dict(columns=torch.zeros((0, n, 4), dtype=torch.uint64)),
              dict(columns=torch.zeros((3, n, 8), dtype=torch.uint64)[:, :, ::2]),
              dict(columns=cols.to("meta")),
              dict(columns=[]),
              dict(columns=[16, 32, 8]),                                         # addresses: 16-byte aligned
              dict(columns=[16, 32, 0]),
              dict(input_rows=[n, n]),
              dict(input_rows=[n, n, n + 1]),
              dict(input_rows=[n, n, -1])]
    good_e = dict(rows=n, columns=cols, points=[5, 7], queries=[(0, 0), (2, 1)])
    good_o = dict(rows=n, columns=cols, groups=[[0, 1], [2]], points=[5, 7], challenges=[9, 11])

    def but(good, **kw):
        d = dict(good)
        d.update(kw)
        return d
    for kw in shared + [dict(points=[]), dict(points=[1 << 256, 2]), dict(points=[-1, 2]), dict(queries=[]), dict(queries=[(3, 0)]), dict(queries=[(0, 2)]),
                        dict(queries=[(-1, 0)]), dict(points=torch.zeros((2, 3), dtype=torch.uint64))]:
        with pytest.raises(ValueError):
            cfg.evaluate(**but(good_e, **kw))
    for kw in shared + [dict(groups=[]), dict(groups=[[0, 1], []]), dict(groups=[[0, 3], [2]]), dict(groups=[[0, -1], [2]]), dict(points=[5]),
                        dict(challenges=[9, 11, 13]), dict(points=None), dict(challenges=[1 << 256, 2]),
                        dict(out=torch.zeros((2, n, 4), dtype=torch.int64)),
                        dict(out=torch.zeros((2, n - 1, 4), dtype=torch.uint64)),    # fewer rows than are written
                        dict(out=torch.zeros((3, n, 4), dtype=torch.uint64)),        # one quotient per group
                        dict(out=torch.zeros((2, n, 8), dtype=torch.uint64)[:, :, ::2]),
                        dict(out=torch.zeros((2, n, 4), dtype=torch.uint64).to("meta")),
                        dict(out=[4096]), dict(out=[4096, 8]), dict(out=[4096, 0])]:
        with pytest.raises(ValueError):
            cfg.open(**but(good_o, **kw))
    # a short column tensor must still hold the rows that input_rows declares
    with pytest.raises(ValueError):
        cfg.open(**but(good_o, columns=torch.zeros((3, 10, 4), dtype=torch.uint64), input_rows=[10, 10, 11]))


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


def test_open_launches_on_the_cpu_under_asan_ubsan(tmp_path):
    got = re.search(r"open value check ok: (\d+) runs, (\d+) rows", _standalone(tmp_path, "open_value_check"))
    assert got and int(got.group(1)) > 5000 and int(got.group(2)) > 10_000_000


def test_open_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, "hsw_open.o")]                   # (the entry points refer to these kernels alone)
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_open.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "open_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "open_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "open lifecycle ok" in res.stdout
