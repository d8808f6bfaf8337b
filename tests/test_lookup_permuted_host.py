"""The permuted lookup pair (hsw_gadget_lookup_permuted) without a GPU: the public surface -- one symbol with one
signature in the header, in _native.py and in hsw-sys, two structs, two flags, the ABI numbers unchanged, the new
kernels in libhsw.so --, the argument rules of the Python wrapper, and two stand-alone programs under ASan + UBSan:
tests/cpp/permuted_index_check.cpp (the index rules and the row values of csrc/hsw_permuted_index.hpp /
hsw_permuted_value.hpp against brute-force models) and, with the stand-in HIP runtime and LeakSanitizer,
tests/cpp/lookup_permuted_lifecycle.cpp (refusals, argument counts, launches, scratch)."""
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
    name = "hsw_gadget_lookup_permuted"
    assert name in N.SYMBOLS and hasattr(lib, name) and lib.hsw_gadget_lookup_permuted.restype is C.c_int
    assert lib.hsw_gadget_lookup_permuted.argtypes == [C.c_void_p, C.POINTER(N.LookupPermuted), C.POINTER(N.PermutedReport)]
    assert (C.sizeof(N.LookupPermuted), C.sizeof(N.PermutedReport)) == (64, 80)
    assert [f[0] for f in N.LookupPermuted._fields_] == ["table", "flags", "usable_rows", "n_arguments", "d_input_columns", "d_table_columns",
                                                         "thetas", "d_m", "m_pitch"]
    assert [f[0] for f in N.PermutedReport._fields_] == ["arguments", "entries", "written", "not_in_table", "first_context", "first_entry",
                                                         "first_table", "first_column", "overflow_arguments", "kernel_ms", "prepare_ms",
                                                         "write_ms", "reserved_"]
    assert (N.HSW_PERMUTED_GIVEN_M, N.HSW_PERMUTED_THETA_ON_SPREAD) == (1, 2)
    for decl in (r"int hsw_gadget_lookup_permuted\(hsw_gadget \*g, const hsw_lookup_permuted \*args, hsw_permuted_report \*report\);",
                 r"#define HSW_PERMUTED_GIVEN_M 1u\b", r"#define HSW_PERMUTED_THETA_ON_SPREAD 2u\b"):
        assert re.search(decl, header), decl
    assert re.search(r"typedef struct hsw_lookup_permuted \{\s*uint32_t table;[^}]*uint32_t flags;[^}]*uint64_t usable_rows;[^}]*size_t n_arguments;[^}]*"
                     r"void \*const \*d_input_columns;[^}]*void \*const \*d_table_columns;[^}]*const void \*thetas;[^}]*uint32_t \*d_m;[^}]*"
                     r"uint64_t m_pitch;[^}]*\} hsw_lookup_permuted;", header)
    assert re.search(r"typedef struct hsw_permuted_report \{\s*uint64_t arguments;[^}]*uint64_t entries;[^}]*uint64_t written;[^}]*uint64_t not_in_table;[^}]*"
                     r"uint64_t first_context, first_entry;[^}]*uint32_t first_table, first_column;\s*uint64_t overflow_arguments;[^}]*"
                     r"float kernel_ms, prepare_ms, write_ms; uint32_t reserved_;\s*\} hsw_permuted_report;", header)
    for decl in (r"pub fn hsw_gadget_lookup_permuted\(g: \*mut hsw_gadget, args: \*const hsw_lookup_permuted,\s*report: \*mut hsw_permuted_report\) -> c_int;",
                 r"pub const HSW_PERMUTED_GIVEN_M: u32 = 1;", r"pub const HSW_PERMUTED_THETA_ON_SPREAD: u32 = 2;"):
        assert re.search(decl, rs), decl
    assert re.search(r"pub struct hsw_lookup_permuted \{\s*pub table: u32,\s*pub flags: u32,\s*pub usable_rows: u64,\s*pub n_arguments: usize,\s*"
                     r"pub d_input_columns: \*const \*mut c_void,\s*pub d_table_columns: \*const \*mut c_void,\s*pub thetas: \*const c_void,\s*"
                     r"pub d_m: \*mut u32,\s*pub m_pitch: u64,\s*\}", rs)
    assert re.search(r"pub struct hsw_permuted_report \{\s*pub arguments: u64,\s*pub entries: u64,\s*pub written: u64,\s*pub not_in_table: u64,\s*"
                     r"pub first_context: u64,\s*pub first_entry: u64,\s*pub first_table: u32,\s*pub first_column: u32,\s*pub overflow_arguments: u64,\s*"
                     r"pub kernel_ms: f32,\s*pub prepare_ms: f32,\s*pub write_ms: f32,\s*pub reserved_: u32,\s*\}", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "lookup_permuted")
    blob = open(N.LIB_PATH, "rb").read()
    for kernel in (b"hsw_permuted_prepare_kernel", b"hsw_permuted_values_kernel", b"hsw_permuted_write_kernel", b"hsw_permuted_sums_kernel",
                   b"hsw_permuted_zero_kernel"):
        assert kernel in blob, kernel                                        # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import torch
    N = hsw._native
    rep = N.PermutedReport()
    assert N.lib().hsw_gadget_lookup_permuted(None, C.byref(N.LookupPermuted()), C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.n_contexts, cfg.context_images, cfg.max_variable_byte_sizes = 3, False, [64]
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    S, R = N.HSW_LOOKUP_SPREAD, N.HSW_LOOKUP_RANGE
    th = [1, 2, 3]
    col = torch.zeros((6, 300, 4), dtype=torch.uint64)
    for args, kw in (((7, 300), dict(thetas=th)),                                        # no such table
                     ((S, 255), dict(thetas=th)),                                        # usable_rows below the table size
                     ((R, 65535), {}),
                     ((S, 300), {}),                                                     # no thetas
                     ((S, 300), dict(thetas=[1, 2])),                                    # one per proof
                     ((R, 65536), dict(thetas=th)),                                      # thetas for the range argument
                     ((S, 300), dict(thetas=th, out_input=torch.zeros((6, 300, 4), dtype=torch.int64))),    # dtype
                     ((S, 300), dict(thetas=th, out_input=torch.zeros((5, 300, 4), dtype=torch.uint64))),   # one column per argument
                     ((S, 300), dict(thetas=th, out_table=torch.zeros((6, 299, 4), dtype=torch.uint64))),   # fewer rows than usable
                     ((S, 300), dict(thetas=th, out_table=torch.zeros((6, 300, 8), dtype=torch.uint64)[:, :, ::2])),   # not contiguous
                     ((S, 300), dict(thetas=th, out_input=col.to("meta"))),              # another device
                     ((S, 300), dict(thetas=th, m=torch.zeros((6, 256), dtype=torch.int64))),
                     ((S, 300), dict(thetas=th, m=torch.zeros((6, 255), dtype=torch.int32))),
                     ((S, 300), dict(thetas=th, m=torch.zeros((3, 256), dtype=torch.int32)))):
        with pytest.raises(ValueError):
            cfg.lookup_permuted(*args, **kw)


def test_index_rules_and_row_values_under_asan_ubsan(tmp_path):
    hipcc = _hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    cxx = clang if os.path.exists(clang) else "g++"
    exe = str(tmp_path / "permuted_index_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "permuted_index_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    got = re.search(r"permuted index check ok: (\d+) exhaustive cases, (\d+) corner and random cases", res.stdout)
    # T = 2: sum over u in {2, 3, 7} of (u + 1) compositions... counted directly: every m with sum m <= u
    want = sum(sum(_compositions(E, T) for E in range(u + 1)) for T in (2, 4) for u in (T, T + 1, T + 5))
    assert got and int(got.group(1)) == want and int(got.group(2)) >= 4 * 11


def _compositions(E, T):
    """ways to write E as an ordered sum of T non-negative integers"""
    from math import comb
    return comb(E + T - 1, T - 1)


def test_lookup_permuted_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, f) for f in ("hsw_lookup_counts.o", "hsw_lookup_permuted.o")]
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_lookup.cpp"), out),
             _compile(hipcc, os.path.join(CSRC, "hsw_gadget_permuted.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "lookup_permuted_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "lookup_permuted_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "lookup permuted lifecycle ok" in res.stdout
