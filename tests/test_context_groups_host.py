"""hsw_gadget_create_contexts (K Contexts of M digests each) without a GPU: the public surface -- symbol, argtypes,
hsw-sys declaration, ABI version -- and, under ASan + UBSan + LeakSanitizer with the stand-in HIP runtime, the
creation rules, the lifecycle and every position of a group against a single shared-context gadget
(tests/cpp/context_groups_lifecycle.cpp)."""
import ctypes as C
import os
import re

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_symbol_signature_and_declarations(hsw):
    N = hsw._native
    assert N.lib().hsw_abi_version() == 3
    assert "hsw_gadget_create_contexts" in N.SYMBOLS
    f = N.lib().hsw_gadget_create_contexts
    assert f.restype is C.c_int and len(f.argtypes) == 7
    assert f.argtypes[2] is C.c_size_t and f.argtypes[3] is C.c_size_t and f.argtypes[5] is C.c_uint32
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"int hsw_gadget_create_contexts\(hsw_engine \*e, const size_t \*max_variable_byte_sizes, "
                     r"size_t digests_per_context,\s+size_t n_contexts, int is_input_range_check, uint32_t flags, "
                     r"hsw_gadget \*\*out\);", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn hsw_gadget_create_contexts\(e: \*mut hsw_engine, max_variable_byte_sizes: \*const usize, "
                     r"digests_per_context: usize,\s+n_contexts: usize, is_input_range_check: c_int, flags: u32,\s+"
                     r"out: \*mut \*mut hsw_gadget\) -> c_int;", rs)


def test_argument_rules_that_need_no_device(hsw):
    """Null handles and empty groups are refused before anything is created."""
    N = hsw._native
    lib = N.lib()
    sizes = (C.c_size_t * 2)(128, 64)
    out = C.c_void_p()
    for args in ((None, sizes, 2, 3), (C.c_void_p(1), None, 2, 3), (C.c_void_p(1), sizes, 0, 3), (C.c_void_p(1), sizes, 2, 0)):
        e, s, m, k = args
        assert lib.hsw_gadget_create_contexts(e, s, m, k, 1, N.HSW_GADGET_WHOLE_DIGEST, C.byref(out)) == N.HSW_ERR_INVALID_ARG
        assert not out.value


def test_launch_record_counts_expansion_launches(hsw):
    """hsw_launch_info.seq sits where the reserved word was: the struct keeps its size and field offsets."""
    N = hsw._native
    assert C.sizeof(N.LaunchInfo) == 48 and N.LaunchInfo.seq.offset == 28 and N.LaunchInfo.n_blocks.offset == 32
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    body = re.search(r"typedef struct hsw_launch_info \{(.*?)\} hsw_launch_info;", header, re.S).group(1)
    fields = re.findall(r"uint(?:32|64)_t (\w+);", body)
    assert fields == [n for n, _ in N.LaunchInfo._fields_]


def test_context_groups_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "context_groups_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "context_groups_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "context groups lifecycle ok" in res.stdout
