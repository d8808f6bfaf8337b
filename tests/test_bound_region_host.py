"""hsw_gadget_bind_region (a gadget's region bound to caller-owned device columns with pitches) without a GPU: the
public surface -- symbols, argtypes, the struct's size and field order in the header, in _native.py and in hsw-sys,
ABI version 3 -- and, under ASan + UBSan + LeakSanitizer with the stand-in HIP runtime, the argument rules, the
lifecycle and every position of a bound gadget against an unbound twin (tests/cpp/bound_region_lifecycle.cpp)."""
import ctypes as C
import os
import re

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)

FIELDS = ["d_columns", "column_pitch", "columns_capacity", "context_pitch", "d_lookup", "lookup_capacity", "lookup_pitch",
          "d_chip_dense", "d_chip_spread", "chip_col_stride", "chip_rows_capacity", "chip_context_pitch"]
POINTERS = {"d_columns", "d_lookup", "d_chip_dense", "d_chip_spread"}


def test_symbols_signatures_and_abi_version(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    for name in ("hsw_gadget_bind_region", "hsw_gadget_region_binding"):
        assert name in N.SYMBOLS
        f = getattr(lib, name)
        assert f.restype is C.c_int and len(f.argtypes) == 2
        assert f.argtypes[0] is C.c_void_p and f.argtypes[1] is C.POINTER(N.RegionBinding)
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"int hsw_gadget_bind_region\(hsw_gadget \*g, const hsw_region_binding \*b\);", header)
    assert re.search(r"int hsw_gadget_region_binding\(const hsw_gadget \*g, hsw_region_binding \*out\);", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn hsw_gadget_bind_region\(g: \*mut hsw_gadget, b: \*const hsw_region_binding\) -> c_int;", rs)
    assert re.search(r"pub fn hsw_gadget_region_binding\(g: \*const hsw_gadget, out: \*mut hsw_region_binding\) -> c_int;", rs)


def test_struct_is_the_same_in_the_header_the_ctypes_binding_and_hsw_sys(hsw):
    N = hsw._native
    assert C.sizeof(N.RegionBinding) == 12 * 8
    assert [n for n, _ in N.RegionBinding._fields_] == FIELDS
    for n, t in N.RegionBinding._fields_:
        assert t is (C.c_void_p if n in POINTERS else C.c_uint64), n
        assert getattr(N.RegionBinding, n).offset == 8 * FIELDS.index(n)
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    body = re.search(r"typedef struct hsw_region_binding \{(.*?)\} hsw_region_binding;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        kind = "ptr" if stmt.startswith("void") else "u64"
        assert stmt.startswith("void") or stmt.startswith("uint64_t"), stmt
        decls += [(n.strip().lstrip("*").strip(), kind) for n in re.sub(r"^(void|uint64_t)\s*", "", stmt).split(",")]
    assert [n for n, _ in decls] == FIELDS
    assert {n for n, k in decls if k == "ptr"} == POINTERS
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    rbody = re.search(r"#\[repr\(C\)\]\s*pub struct hsw_region_binding \{(.*?)\}", rs, re.S).group(1)
    rfields = re.findall(r"pub (\w+): ([^,]+),", rbody)
    assert [n for n, _ in rfields] == FIELDS
    for n, t in rfields:
        assert t.strip() == ("*mut c_void" if n in POINTERS else "u64"), (n, t)


def test_argument_rules_that_need_no_device(hsw):
    N = hsw._native
    lib = N.lib()
    b = N.RegionBinding()
    assert lib.hsw_gadget_bind_region(None, C.byref(b)) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_bind_region(None, None) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_region_binding(None, C.byref(b)) == N.HSW_ERR_INVALID_ARG


def test_bound_region_lifecycle_and_positions_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "bound_region_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "bound_region_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "bound region lifecycle ok" in res.stdout
