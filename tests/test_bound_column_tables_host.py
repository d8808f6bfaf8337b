"""hsw_gadget_bind_column_tables (the lookup-advice column and the chip columns of a bound gadget by pointer table too)
without a GPU: the public surface -- the symbol and its struct in the header, in _native.py and in hsw-sys, ABI version
3 with minor 1, hsw_region_binding still 96 bytes -- and, under ASan + UBSan + LeakSanitizer with the stand-in HIP
runtime, every refusal, the lifecycle, the reports and the download layout of a gadget whose every advice column is an
allocation of its own (tests/cpp/bound_column_tables_lifecycle.cpp)."""
import ctypes as C
import os
import re

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_symbol_signature_struct_and_abi_version(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    assert C.sizeof(N.RegionBinding) == 96 and C.sizeof(N.ColumnTables) == 7 * C.sizeof(C.c_void_p)
    assert [n for n, _ in N.ColumnTables._fields_] == ["d_column_ptrs", "n_column_ptrs", "d_lookup_ptrs", "n_lookup_ptrs",
                                                      "d_chip_dense_ptrs", "d_chip_spread_ptrs", "n_chip_ptrs"]
    assert "hsw_gadget_bind_column_tables" in N.SYMBOLS
    f = lib.hsw_gadget_bind_column_tables
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.POINTER(N.RegionBinding), C.POINTER(N.ColumnTables)]
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_MINOR 1\b", header)
    assert re.search(r"int hsw_gadget_bind_column_tables\(hsw_gadget \*g, const hsw_region_binding \*b,\s*const hsw_column_tables \*t\);", header)
    # hsw_gadget_bind_columns is exactly what it was
    assert re.search(r"int hsw_gadget_bind_columns\(hsw_gadget \*g, const hsw_region_binding \*b,\s*void \*const \*d_column_ptrs, size_t n_ptrs\);", header)
    fields = re.search(r"typedef struct hsw_column_tables \{(.*?)\} hsw_column_tables;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [n for n, _ in N.ColumnTables._fields_]
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn hsw_gadget_bind_column_tables\(\s*g: \*mut hsw_gadget,\s*b: \*const hsw_region_binding,\s*"
                     r"t: \*const hsw_column_tables,\s*\) -> c_int;", rs)
    rs_fields = re.search(r"pub struct hsw_column_tables \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", rs_fields) == [n for n, _ in N.ColumnTables._fields_]


def test_argument_rules_that_need_no_device(hsw):
    N = hsw._native
    lib = N.lib()
    b = N.RegionBinding()
    ptrs = (C.c_void_p * 1)(0)
    t = N.ColumnTables(C.cast(ptrs, C.POINTER(C.c_void_p)), 1, None, 0, None, None, 0)
    assert lib.hsw_gadget_bind_column_tables(None, C.byref(b), C.byref(t)) == N.HSW_ERR_INVALID_ARG


def test_bound_column_tables_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "bound_column_tables_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "bound_column_tables_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "bound column tables lifecycle ok" in res.stdout
