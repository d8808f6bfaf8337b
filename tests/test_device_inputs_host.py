"""hsw_gadget_digest_batch_device (messages that already live in device memory) without a GPU: the public surface --
the symbol in the header, in _native.py and in hsw-sys with one signature, HSW_ABI_MINOR still 1,
hsw_gadget_digest_batch's declaration untouched -- the refusals that need no device, and, under ASan + UBSan +
LeakSanitizer with the stand-in HIP runtime, the refusals, the lifecycle and the proof that the host never reads a
message byte (tests/cpp/device_inputs_lifecycle.cpp)."""
import ctypes as C
import os
import re

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_symbol_signature_and_abi_version(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    assert "hsw_gadget_digest_batch_device" in N.SYMBOLS
    f = lib.hsw_gadget_digest_batch_device
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                          C.POINTER(N.HashResult)]
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_MINOR 1\b", header)
    assert re.search(r"int hsw_gadget_digest_batch_device\(hsw_gadget \*g, size_t n, const void \*const \*d_inputs,\s*"
                     r"const size_t \*input_lens, const size_t \*precomputed_input_lens,\s*hsw_hash_result \*results\);", header)
    # hsw_gadget_digest_batch is exactly what it was
    assert ("int hsw_gadget_digest_batch(hsw_gadget *g, size_t n, const uint8_t *const *inputs,\n"
            "                            const size_t *input_lens, const size_t *precomputed_input_lens,\n"
            "                            hsw_hash_result *results);") in header
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn hsw_gadget_digest_batch_device\(\s*g: \*mut hsw_gadget,\s*n: usize,\s*d_inputs: \*const \*const c_void,\s*"
                     r"input_lens: \*const usize,\s*precomputed_input_lens: \*const usize,\s*results: \*mut hsw_hash_result,?\s*\) -> c_int;", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "digest_batch_device")


def test_argument_rules_that_need_no_device(hsw):
    N = hsw._native
    lib = N.lib()
    ptrs = (C.c_void_p * 1)(64)
    lens = (C.c_size_t * 1)(5)
    res = (N.HashResult * 1)()
    assert lib.hsw_gadget_digest_batch_device(None, 1, ptrs, lens, None, res) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_digest_batch_device(None, 1, ptrs, lens, None, None) == N.HSW_ERR_INVALID_ARG


def test_device_inputs_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "device_inputs_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "device_inputs_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "device inputs lifecycle ok" in res.stdout
