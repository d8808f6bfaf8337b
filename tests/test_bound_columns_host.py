"""hsw_gadget_bind_columns (a gadget's image columns bound to one device pointer each) without a GPU: the public
surface -- the symbol in the header, in _native.py and in hsw-sys, ABI version 3, hsw_region_binding still 96 bytes --
and, under ASan + UBSan + LeakSanitizer with the stand-in HIP runtime, the argument rules, the lifecycle, the five
refusals and every position of a bound gadget against an unbound twin (tests/cpp/bound_columns_lifecycle.cpp)."""
import ctypes as C
import os
import re

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_symbol_signature_and_abi_version(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    assert C.sizeof(N.RegionBinding) == 96
    assert "hsw_gadget_bind_columns" in N.SYMBOLS
    f = lib.hsw_gadget_bind_columns
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.POINTER(N.RegionBinding), C.POINTER(C.c_void_p), C.c_size_t]
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"int hsw_gadget_bind_columns\(hsw_gadget \*g, const hsw_region_binding \*b,\s*void \*const \*d_column_ptrs, size_t n_ptrs\);", header)
    assert "columns by pointer table" in header
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn hsw_gadget_bind_columns\(\s*g: \*mut hsw_gadget,\s*b: \*const hsw_region_binding,\s*"
                     r"d_column_ptrs: \*const \*mut c_void,\s*n_ptrs: usize,\s*\) -> c_int;", rs)


def test_argument_rules_that_need_no_device(hsw):
    N = hsw._native
    lib = N.lib()
    b = N.RegionBinding()
    ptrs = (C.c_void_p * 1)(0)
    assert lib.hsw_gadget_bind_columns(None, C.byref(b), ptrs, 1) == N.HSW_ERR_INVALID_ARG
    li = N.LaunchInfo()
    li.limbs, li.tile_cells, li.tile_rows, li.repr, li.split = 2, 64, 32, 1, 4
    assert li.kernel_name() == "hsw::hsw_expand_table_kernel<2, 64, 32, 1, true>"
    li.split = 6
    assert li.kernel_name() == "hsw::hsw_small_table_kernel<2, 1, true>"


def test_bound_columns_lifecycle_and_positions_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "bound_columns_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "bound_columns_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "bound columns lifecycle ok" in res.stdout
