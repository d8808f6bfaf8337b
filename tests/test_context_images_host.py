"""HSW_GADGET_CONTEXT_IMAGES without a GPU: the public surface (ABI version, symbol lists of the Python binding and
hsw-sys) and the host-side lifecycle under ASan + UBSan + LeakSanitizer with the stand-in HIP runtime."""
import os
import re

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_abi_version_and_symbol_lists(hsw):
    N = hsw._native
    assert N.lib().hsw_abi_version() == 3
    assert "hsw_gadget_context_region" in N.SYMBOLS and N.HSW_GADGET_CONTEXT_IMAGES == 4
    assert N.lib().hsw_gadget_context_region.argtypes is not None
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_GADGET_CONTEXT_IMAGES 4u", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    assert "pub fn hsw_gadget_context_region(" in rs and "pub const HSW_GADGET_CONTEXT_IMAGES: u32 = 4;" in rs
    assert "pub struct hsw_context_region" in rs


def test_context_region_struct_layout_matches_the_header(hsw):
    """14 x 8-byte fields after the four pointers and a final pair of u32: 128 bytes on LP64."""
    import ctypes as C
    assert C.sizeof(hsw._native.ContextRegion) == 4 * 8 + 11 * 8 + 8


def test_context_images_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "context_images_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "context_images_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "context images lifecycle ok" in res.stdout
