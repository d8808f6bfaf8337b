"""The permutation argument's grand products (hsw_gadget_permutation_product) without a GPU: the public surface -- one
symbol with one signature in the header, in _native.py and in hsw-sys, two structs, the ABI numbers unchanged, the new
kernels in libhsw.so --, the argument rules of the Python wrapper, and two stand-alone programs under ASan + UBSan:
tests/cpp/permutation_value_check.cpp (the row rules of csrc/hsw_permutation_value.hpp against a shift-and-add model)
and, with the stand-in HIP runtime and LeakSanitizer, tests/cpp/permutation_product_lifecycle.cpp (refusals, products,
launches, overlaps, scratch)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from tests.test_host_sanitizers import CSRC, ROOT, _compile, _hipcc, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_symbol_signature_and_abi_numbers(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_VERSION 3\b", header) and re.search(r"#define HSW_ABI_MINOR 1\b", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    name = "hsw_gadget_permutation_product"
    assert name in N.SYMBOLS and hasattr(lib, name) and lib.hsw_gadget_permutation_product.restype is C.c_int
    assert lib.hsw_gadget_permutation_product.argtypes == [C.c_void_p, C.POINTER(N.PermutationProduct), C.POINTER(N.PermutationReport)]
    assert (C.sizeof(N.PermutationProduct), C.sizeof(N.PermutationReport)) == (96, 80)
    assert [f[0] for f in N.PermutationProduct._fields_] == ["flags", "chunk_columns", "usable_rows", "n_columns", "d_columns", "column_rows",
                                                             "d_sigmas", "d_products", "betas", "gammas", "omega", "delta", "status"]
    assert [f[0] for f in N.PermutationReport._fields_] == ["proofs", "products", "written", "open_proofs", "first_open", "refused_proofs",
                                                            "first_refused", "tile_rows", "reserved_", "kernel_ms", "tiles_ms", "scan_ms", "write_ms"]
    assert re.search(r"int hsw_gadget_permutation_product\(hsw_gadget \*g, const hsw_permutation_product \*args, hsw_permutation_report \*report\);", header)
    assert re.search(r"typedef struct hsw_permutation_product \{\s*uint32_t flags, chunk_columns;[^}]*uint64_t usable_rows;[^}]*size_t n_columns;[^}]*"
                     r"const void \*const \*d_columns;[^}]*const uint64_t \*column_rows;[^}]*const void \*const \*d_sigmas;[^}]*"
                     r"void \*const \*d_products;[^}]*const void \*betas, \*gammas;[^}]*const void \*omega, \*delta;[^}]*uint32_t \*status;[^}]*"
                     r"\} hsw_permutation_product;", header)
    assert re.search(r"typedef struct hsw_permutation_report \{\s*uint64_t proofs, products, written;[^}]*"
                     r"uint64_t open_proofs, first_open, refused_proofs, first_refused;[^}]*uint32_t tile_rows, reserved_;\s*"
                     r"float kernel_ms, tiles_ms, scan_ms, write_ms;\s*\} hsw_permutation_report;", header)
    assert re.search(r"pub fn hsw_gadget_permutation_product\(g: \*mut hsw_gadget, args: \*const hsw_permutation_product,\s*"
                     r"report: \*mut hsw_permutation_report\) -> c_int;", rs)
    assert re.search(r"pub struct hsw_permutation_product \{\s*pub flags: u32,\s*pub chunk_columns: u32,\s*pub usable_rows: u64,\s*pub n_columns: usize,\s*"
                     r"pub d_columns: \*const \*const c_void,\s*pub column_rows: \*const u64,\s*pub d_sigmas: \*const \*const c_void,\s*"
                     r"pub d_products: \*const \*mut c_void,\s*pub betas: \*const c_void,\s*pub gammas: \*const c_void,\s*pub omega: \*const c_void,\s*"
                     r"pub delta: \*const c_void,\s*pub status: \*mut u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_permutation_report \{\s*pub proofs: u64,\s*pub products: u64,\s*pub written: u64,\s*pub open_proofs: u64,\s*"
                     r"pub first_open: u64,\s*pub refused_proofs: u64,\s*pub first_refused: u64,\s*pub tile_rows: u32,\s*pub reserved_: u32,\s*"
                     r"pub kernel_ms: f32,\s*pub tiles_ms: f32,\s*pub scan_ms: f32,\s*pub write_ms: f32,\s*\}", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "permutation_product")
    blob = open(N.LIB_PATH, "rb").read()
    for kernel in (b"hsw_permutation_tiles_kernel", b"hsw_permutation_scan_kernel", b"hsw_permutation_write_kernel"):
        assert kernel in blob, kernel                                        # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import numpy as np
    import torch
    N = hsw._native
    rep = N.PermutationReport()
    assert N.lib().hsw_gadget_permutation_product(None, C.byref(N.PermutationProduct()), C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.n_contexts, cfg.context_images, cfg.max_variable_byte_sizes = 3, False, [64]
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    ch = [1, 2, 3]
    u, m, L = 300, 5, 2                                      # three proofs, S = 3 chunks
    cols = torch.zeros((3, m, u, 4), dtype=torch.uint64)
    sig = torch.zeros((m, u, 4), dtype=torch.uint64)
    z = torch.zeros((3, 3, u + 1, 4), dtype=torch.uint64)
    good = dict(betas=ch, gammas=ch, omega=7, delta=9, columns=cols, sigmas=sig, out=z)

    def but(**kw):
        d = dict(good)
        d.update(kw)
        return d
    for (rows, chunk), kw in (((0, L), good),                                             # usable_rows
                              (((1 << 31) + 1, L), good),
                              ((u, 0), good),                                             # chunk_columns
                              ((u, L), but(betas=None)),
                              ((u, L), but(betas=[1, 2])),                                # one per proof
                              ((u, L), but(gammas=[1, 2, 3, 4])),
                              ((u, L), but(gammas=np.zeros((3, 3), dtype=np.uint64))),
                              ((u, L), but(omega=None)),
                              ((u, L), but(omega=[1, 2])),                                # one element
                              ((u, L), but(delta=None)),
                              ((u, L), but(delta=np.zeros((2, 4), dtype=np.uint64))),
                              ((u, L), but(columns=cols.to(torch.int64))),                # dtype
                              ((u, L), but(sigmas=sig.to(torch.int32))),
                              ((u, L), but(columns=torch.zeros((3, m - 1, u, 4), dtype=torch.uint64))),   # one column per sigma
                              ((u, L), but(columns=torch.zeros((2, m, u, 4), dtype=torch.uint64))),       # ... and proof
                              ((u, L), but(columns=torch.zeros((3 * m, u, 4), dtype=torch.uint64))),      # (proofs, m, rows, 4)
                              ((u, L), but(columns=torch.zeros((3, m, u - 1, 4), dtype=torch.uint64))),   # fewer rows than usable
                              ((u, L), but(sigmas=torch.zeros((m, u - 1, 4), dtype=torch.uint64))),
                              ((u, L), but(sigmas=torch.zeros((0, u, 4), dtype=torch.uint64))),
                              ((u, L), but(sigmas=[])),
                              ((u, L), but(out=torch.zeros((3, 3, u, 4), dtype=torch.uint64))),           # Z has usable_rows + 1
                              ((u, L), but(out=torch.zeros((3, 2, u + 1, 4), dtype=torch.uint64))),       # S = ceil(5 / 2)
                              ((u, 1), good),                                                             # S = 5 now
                              ((u, L), but(out=torch.zeros((3, 3, u + 1, 8), dtype=torch.uint64)[:, :, :, ::2])),   # not contiguous
                              ((u, L), but(out=z.to("meta"))),                            # another device
                              ((u, L), but(out=[16] * 9)),
                              ((u, L), but(columns=[16 * (i + 1) for i in range(14)])),   # addresses: proofs x m
                              ((u, L), but(columns=[16 * (i + 1) for i in range(14)] + [8])),   # ... 16-byte aligned
                              ((u, L), but(columns=[16 * (i + 1) for i in range(14)] + [0])),
                              ((u, L), but(sigmas=[16, 32, 48, 64, 72])),
                              ((u, L), but(column_rows=[u] * 14)),
                              ((u, L), but(column_rows=[u] * 14 + [u + 1])),
                              ((u, L), but(column_rows=[u] * 14 + [-1]))):
        with pytest.raises(ValueError):
            cfg.permutation_product(rows, chunk, **kw)
    # a short column tensor must still hold the rows that column_rows declares
    with pytest.raises(ValueError):
        cfg.permutation_product(u, L, **but(columns=torch.zeros((3, m, 10, 4), dtype=torch.uint64), column_rows=[10] * 14 + [11]))


def test_permutation_row_rules_under_asan_ubsan(tmp_path):
    hipcc = _hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    cxx = clang if os.path.exists(clang) else "g++"
    exe = str(tmp_path / "permutation_value_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "permutation_value_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    got = re.search(r"permutation value check ok: (\d+) rows, (\d+) permutations", res.stdout)
    # m x L x u x 2 cell forms of random columns, the closing ones for u in {1, 5} and once per cell form at u = 1030
    assert got and int(got.group(2)) == 27 * 2 + 18 * 2 + 2 and int(got.group(1)) > 40000


def test_permutation_product_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, "hsw_permutation_product.o")]    # (the entry point refers to these kernels alone)
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_permutation.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "permutation_product_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "permutation_product_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "permutation product lifecycle ok" in res.stdout
