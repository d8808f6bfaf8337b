"""SHPLONK's multi-point opening of device columns (hsw_gadget_shplonk_quotient, hsw_gadget_shplonk_open) without a GPU:
the model over Python integers that the GPU tests import (tests/shplonk_model.py: the quotient by SUCCESSIVE Kate
division), proven here against the partial-fraction sum the device runs and against the identities c - R = Z Q and
(X - u) w = (L - L(u)) / zd_0; the public surface (one symbol each with one signature in the header, in _native.py and
in hsw-sys, two structs, the ABI numbers unchanged, the new kernels in libhsw.so); the argument rules of the Python
wrapper, matched by message; and two stand-alone programs under ASan + UBSan: tests/cpp/shplonk_value_check.cpp (the
launches run thread for thread on the CPU against the plain recurrence) and, with the stand-in HIP runtime and
LeakSanitizer, tests/cpp/shplonk_lifecycle.cpp (refusals, geometry, launches, scratch).
The two model proofs at the top exercise tests/shplonk_model.py and tests/open_model.py alone: they prove the yardstick,
not the library, and pass whether or not the library has the calls.  Every other test here needs the new code."""
import ctypes as C
import os
import random
import re
import subprocess
import types

import pytest

from tests.constraint_check import P_INT
from tests.open_model import evaluate_model, open_model
from tests.shplonk_model import (fold_y, interpolate_eval, linearisation, partial_fraction_quotient, set_quotient, shplonk_open_model,
                                 shplonk_quotient_model, vanish, zd_of)
from tests.test_host_sanitizers import CSRC, ROOT, _compile, _hipcc, _link_and_run, host_objects  # noqa: F401 (fixture)

ROWS = [1, 2, 3, 17, 64]


def _columns(rng, rows, n):
    heights = [[rows, rows - 1, min(1, rows), 0, rows][b % 5] for b in range(n)]
    cols = [[rng.randrange(P_INT) for _ in range(h)] for h in heights]
    cols[0][0] = P_INT - 1
    return cols


def _points(rng, t):
    pts = [rng.randrange(P_INT) for _ in range(t)]
    if t > 1:
        pts[1] = 0                                                            # a point equal to 0
    return pts


# ---- the model (tests/shplonk_model.py) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("t", [1, 2, 3, 4])
def test_successive_division_is_the_partial_fraction_sum_and_the_floor(rows, t):
    rng = random.Random(900 + 10 * rows + t)
    cols = _columns(rng, rows, 5)
    zs = _points(rng, t)
    for y in (0, 1, rng.randrange(P_INT)):
        for group in (cols[:1], cols[1:2], cols[:3], cols[::-1], [cols[3]]):
            c = fold_y(group, y, rows)
            q = set_quotient(c, zs)
            assert q == partial_fraction_quotient(c, zs)                      # cell for cell
            assert q[rows - min(t, rows):] == [0] * min(t, rows)              # the top min(t, rows) cells are 0
            # c(r) - R(r) = Z(r) Q(r), R interpolated from the evaluations of c over the set
            r = rng.randrange(P_INT)
            R_r = interpolate_eval(zs, [evaluate_model(c, z) for z in zs], r)
            assert (evaluate_model(c, r) - R_r) % P_INT == vanish(r, zs) * evaluate_model(q, r) % P_INT
            if t == 1:                                                        # the GWC quotient of the reversed list, challenge y
                assert q == open_model(group[::-1], zs[0], y, rows)[0]


@pytest.mark.parametrize("rows", ROWS)
def test_the_linearisation_vanishes_at_u_and_w_is_its_quotient(rows):
    rng = random.Random(1000 + rows)
    cols = _columns(rng, rows, 7)
    T = _points(rng, 4)
    sets = [([0, 1], [0]), ([2], [0, 1]), ([3, 4, 5], [1, 2, 3]), ([6], [3, 0, 2, 1])]
    for y, v in ((rng.randrange(P_INT), rng.randrange(P_INT)), (0, 1), (1, 0)):
        u, r = rng.randrange(P_INT), rng.randrange(P_INT)
        h = shplonk_quotient_model(cols, sets, T, y, v, rows)
        # h by the device's route: the v-fold of the partial-fraction sums
        folds = [fold_y([cols[b] for b in cs], y, rows) for cs, _ in sets]
        alt = [0] * rows
        for i, (c, (_, ps)) in enumerate(zip(folds, sets)):
            q = partial_fraction_quotient(c, [T[t] for t in ps])
            alt = [(a + pow(v, i, P_INT) * b) % P_INT for a, b in zip(alt, q)]
        assert h == alt
        L = linearisation(cols, sets, T, y, v, u, h, rows)
        w = shplonk_open_model(cols, sets, T, y, v, u, h, rows)
        zd = zd_of(sets, T, u)
        # the constant that halo2 subtracts: sum_i v^i zd_i R_i(u); it changes L[0] alone, which w never reads
        const = sum(pow(v, i, P_INT) * zd[i] * interpolate_eval([T[t] for t in ps], [evaluate_model(c, T[t]) for t in ps], u)
                    for i, (c, (_, ps)) in enumerate(zip(folds, sets))) % P_INT
        assert (evaluate_model(L, u) - const) % P_INT == 0                    # (L - const)(u) = 0
        assert (r - u) * evaluate_model(w, r) % P_INT == (evaluate_model(L, r) - const) * pow(zd[0], -1, P_INT) % P_INT
        assert len(w) == rows and w[rows - 1] == 0
        L2 = [(L[0] - const) % P_INT] + L[1:]
        assert [x * pow(zd[0], -1, P_INT) % P_INT for x in open_model([L2], u, 0, rows)[0]] == w


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_symbol_signature_and_abi_numbers(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_VERSION 3\b", header) and re.search(r"#define HSW_ABI_MINOR 1\b", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    for name in ("hsw_gadget_shplonk_quotient", "hsw_gadget_shplonk_open"):
        assert name in N.SYMBOLS and N.SYMBOLS.count(name) == 1 and hasattr(lib, name) and getattr(lib, name).restype is C.c_int
        assert getattr(lib, name).argtypes == [C.c_void_p, C.POINTER(N.Shplonk), C.POINTER(N.ShplonkReport)]
        assert len(re.findall(r"\bint %s\(" % name, header)) == 1 and len(re.findall(r"pub fn %s\(" % name, rs)) == 1
        assert re.search(r"int %s\(hsw_gadget \*g, const hsw_shplonk \*args, hsw_shplonk_report \*report\);" % name, header)
        assert re.search(r"pub fn %s\(g: \*mut hsw_gadget, args: \*const hsw_shplonk, report: \*mut hsw_shplonk_report\) -> c_int;" % name, rs)
    assert (C.sizeof(N.Shplonk), C.sizeof(N.ShplonkReport)) == (144, 72)
    assert [f[0] for f in N.Shplonk._fields_] == ["flags", "tile_rows", "rows", "n_columns", "d_columns", "input_rows", "n_points", "points", "n_sets",
                                                  "set_first", "set_columns", "set_point_first", "set_points", "y", "v", "u", "d_h", "d_out", "status"]
    assert [f[0] for f in N.ShplonkReport._fields_] == ["sets", "items", "columns", "written", "refused", "scratch_bytes", "tile_rows", "tiles",
                                                        "thread_rows", "launches", "kernel_ms", "reserved_"]
    assert N.HSW_SHPLONK_CELL_NOT_BELOW_P == 4 == N.HSW_NTT_CELL_NOT_BELOW_P and N.HSW_SHPLONK_MAX_SET_POINTS == 16
    assert re.search(r"#define HSW_SHPLONK_CELL_NOT_BELOW_P 4u\b", header) and re.search(r"#define HSW_SHPLONK_MAX_SET_POINTS 16u\b", header)
    assert re.search(r"pub const HSW_SHPLONK_CELL_NOT_BELOW_P: u32 = 4;", rs) and re.search(r"pub const HSW_SHPLONK_MAX_SET_POINTS: u32 = 16;", rs)
    assert re.search(r"typedef struct hsw_shplonk \{\s*uint32_t flags, tile_rows;[^}]*uint64_t rows;[^}]*size_t n_columns;[^}]*const void \*const \*d_columns;[^}]*"
                     r"const uint64_t \*input_rows;[^}]*size_t n_points;[^}]*const void \*points;[^}]*size_t n_sets;[^}]*const uint64_t \*set_first;[^}]*"
                     r"const uint32_t \*set_columns;[^}]*const uint64_t \*set_point_first;[^}]*const uint32_t \*set_points;[^}]*const void \*y, \*v, \*u;[^}]*"
                     r"const void \*d_h;[^}]*void \*d_out;[^}]*uint32_t \*status;[^}]*\} hsw_shplonk;", header)
    assert re.search(r"typedef struct hsw_shplonk_report \{\s*uint64_t sets, items, columns;[^}]*uint64_t written, refused;[^}]*uint64_t scratch_bytes;[^}]*"
                     r"uint32_t tile_rows, tiles, thread_rows, launches;[^}]*float kernel_ms;[^}]*uint32_t reserved_;[^}]*\} hsw_shplonk_report;", header)
    assert re.search(r"pub struct hsw_shplonk \{\s*pub flags: u32,\s*pub tile_rows: u32,\s*pub rows: u64,\s*pub n_columns: usize,\s*"
                     r"pub d_columns: \*const \*const c_void,\s*pub input_rows: \*const u64,\s*pub n_points: usize,\s*pub points: \*const c_void,\s*"
                     r"pub n_sets: usize,\s*pub set_first: \*const u64,\s*pub set_columns: \*const u32,\s*pub set_point_first: \*const u64,\s*"
                     r"pub set_points: \*const u32,\s*pub y: \*const c_void,\s*pub v: \*const c_void,\s*pub u: \*const c_void,\s*pub d_h: \*const c_void,\s*"
                     r"pub d_out: \*mut c_void,\s*pub status: \*mut u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_shplonk_report \{\s*pub sets: u64,\s*pub items: u64,\s*pub columns: u64,\s*pub written: u64,\s*pub refused: u64,\s*"
                     r"pub scratch_bytes: u64,\s*pub tile_rows: u32,\s*pub tiles: u32,\s*pub thread_rows: u32,\s*pub launches: u32,\s*pub kernel_ms: f32,\s*"
                     r"pub reserved_: u32,\s*\}", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "shplonk_quotient") and hasattr(hsw.Sha256DynamicConfig, "shplonk_open")
    blob = open(N.LIB_PATH, "rb").read()
    for kernel in (b"hsw_shplonk_tiles_kernel", b"hsw_shplonk_write_kernel", b"hsw_open_scan_kernel"):
        assert kernel in blob, kernel                                        # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import torch
    N = hsw._native
    assert N.lib().hsw_gadget_shplonk_quotient(None, C.byref(N.Shplonk()), C.byref(N.ShplonkReport())) == N.HSW_ERR_INVALID_ARG
    assert N.lib().hsw_gadget_shplonk_open(None, C.byref(N.Shplonk()), C.byref(N.ShplonkReport())) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    n = 64
    cols = torch.zeros((4, n, 4), dtype=torch.uint64)
    good = dict(rows=n, columns=cols, sets=[([0, 1], [0]), ([2], [0, 1]), ([3], [0, 1, 2])], points=[5, 7, 9], y=11, v=13)
    h = torch.zeros((n, 4), dtype=torch.uint64)
    rules = [(dict(rows=0), "rows must be"), (dict(rows=(1 << 28) + 1), "rows must be"), (dict(tile_rows=384), "tile_rows must be"),
             (dict(columns=cols.to(torch.int64)), "columns must be a uint64 tensor"), (dict(columns=[16, 32, 8, 64]), "columns: 4 device addresses"),
             (dict(input_rows=[n, n, n, n + 1]), "input_rows"),
             (dict(points=[]), "points: at least one"), (dict(points=[5, 7, 1 << 256]), "field elements of 256 bits"),
             (dict(points=[5, 7, 5]), "points: the entries must differ in value"),
             (dict(points=[5, 7, 9, 10]), "points: every entry must be used by a set"),
             (dict(sets=[]), "sets: 1 .. 65535"), (dict(sets=[([0], [0])] * 65536), "sets: 1 .. 65535"),
             (dict(sets=[([], [0]), ([2], [0, 1]), ([3], [0, 1, 2])]), "sets: each lists at least one column index below 4"),
             (dict(sets=[([0, 4], [0]), ([2], [0, 1]), ([3], [0, 1, 2])]), "sets: each lists at least one column index below 4"),
             (dict(sets=[([0, 0], [0]), ([2], [0, 1]), ([3], [0, 1, 2])]), "sets: a column is listed once"),
             (dict(sets=[([0, 1], [0]), ([1], [0, 1]), ([3], [0, 1, 2])]), "sets: a column is listed once"),
             (dict(sets=[([0, 1], []), ([2], [0, 1]), ([3], [0, 1, 2])]), "sets: each lists 1 .. 16 distinct point indices below 3"),
             (dict(sets=[([0, 1], [3]), ([2], [0, 1]), ([3], [0, 1, 2])]), "sets: each lists 1 .. 16 distinct point indices below 3"),
             (dict(sets=[([0, 1], [0]), ([2], [1, 1]), ([3], [0, 1, 2])]), "sets: each lists 1 .. 16 distinct point indices below 3"),
             (dict(sets=[([0], list(range(17)))], points=list(range(1, 18))), "sets: each lists 1 .. 16 distinct point indices below 17"),
             (dict(y=None), "y: 1 field element"), (dict(v=[1, 2]), "v: 1 field element"),
             (dict(out=torch.zeros((n, 4), dtype=torch.int64)), "out must be a contiguous uint64 tensor"),
             (dict(out=torch.zeros((n - 1, 4), dtype=torch.uint64)), "out must be a contiguous uint64 tensor"),
             (dict(out=torch.zeros((1, n, 4), dtype=torch.uint64)), "out must be a contiguous uint64 tensor"),
             (dict(out=4104), "out: a tensor or a device address")]
    for kw, message in rules:
        for call, extra in ((cfg.shplonk_quotient, {}), (cfg.shplonk_open, dict(u=17, h=h))):
            d = dict(good)
            d.update(extra)
            d.update(kw)
            with pytest.raises(ValueError, match=re.escape(message)):
                call(**d)
    for kw, message in [(dict(u=None), "u: 1 field element"), (dict(u=1 << 256), "field elements of 256 bits"), (dict(h=None), "h: a tensor or a device address"),
                        (dict(h=8), "h: a tensor or a device address"), (dict(h=h[: n - 1]), "h must be a contiguous uint64 tensor"),
                        (dict(h=h.to(torch.int64)), "h must be a contiguous uint64 tensor")]:
        d = dict(good, u=17, h=h)
        d.update(kw)
        with pytest.raises(ValueError, match=re.escape(message)):
            cfg.shplonk_open(**d)


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


def test_shplonk_launches_on_the_cpu_under_asan_ubsan(tmp_path):
    got = re.search(r"shplonk value check ok: (\d+) runs, (\d+) rows", _standalone(tmp_path, "shplonk_value_check"))
    assert got and int(got.group(1)) > 4000 and int(got.group(2)) > 3_000_000


def test_shplonk_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, "hsw_open.o"), os.path.join(CSRC, "hsw_shplonk.o")]   # (the entry points refer to these kernels alone)
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_shplonk.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "shplonk_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "shplonk_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "shplonk lifecycle ok" in res.stdout
