"""HSW_GADGET_SHARED_CONTEXT without a GPU: the public surface (flag values, symbol lists of the Python binding and
hsw-sys) and the host-side lifecycle under ASan + UBSan + LeakSanitizer with the stand-in HIP runtime."""
import os
import re

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_flag_and_symbol_lists(hsw):
    N = hsw._native
    assert N.lib().hsw_abi_version() == 3
    assert N.HSW_GADGET_SHARED_CONTEXT == 8 and N.HSW_GADGET_MAX_COLUMNS >= 1024
    assert "hsw_gadget_set_digest_origin" in N.SYMBOLS
    assert N.lib().hsw_gadget_set_digest_origin.argtypes is not None
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_GADGET_SHARED_CONTEXT 8u", header)
    assert re.search(r"#define HSW_GADGET_MAX_COLUMNS %du" % N.HSW_GADGET_MAX_COLUMNS, header)
    assert re.search(r"int hsw_gadget_set_digest_origin\(hsw_gadget \*g, size_t h, uint64_t column, uint64_t row, "
                     r"uint64_t lookups_queued\);", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    assert "pub fn hsw_gadget_set_digest_origin(" in rs and "pub const HSW_GADGET_SHARED_CONTEXT: u32 = 8;" in rs


def test_shared_context_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "shared_context_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "shared_context_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "shared context lifecycle ok" in res.stdout
