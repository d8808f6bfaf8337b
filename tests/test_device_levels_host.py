"""hsw_gadget_digest_levels_device (dependent digests -- Merkle trees, hash chains -- in one call) without a GPU: the
public surface -- the symbol in the header, in _native.py and in hsw-sys with one signature, HSW_ABI_MINOR still 1,
the declarations of hsw_gadget_digest_batch and hsw_gadget_digest_batch_device untouched -- the refusals that need
no device, the Python-side validation, and, under ASan + UBSan + LeakSanitizer with the stand-in HIP runtime, the
overlap refusals, the launch count per level, shuffled levels, a Context group and the proof that the host neither
reads an input nor touches an output (tests/cpp/device_levels_lifecycle.cpp)."""
import ctypes as C
import os
import re

import pytest

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_symbol_signature_and_abi_version(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    assert "hsw_gadget_digest_levels_device" in N.SYMBOLS
    f = lib.hsw_gadget_digest_levels_device
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                          C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(N.HashResult)]
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_MINOR 1\b", header)
    assert re.search(r"int hsw_gadget_digest_levels_device\(hsw_gadget \*g, size_t n, const void \*const \*d_inputs,\s*"
                     r"const size_t \*input_lens, const size_t \*precomputed_input_lens,\s*const uint32_t \*levels,\s*"
                     r"void \*const \*d_outputs,\s*hsw_hash_result \*results\);", header)
    # the two earlier calls are exactly what they were
    assert ("int hsw_gadget_digest_batch(hsw_gadget *g, size_t n, const uint8_t *const *inputs,\n"
            "                            const size_t *input_lens, const size_t *precomputed_input_lens,\n"
            "                            hsw_hash_result *results);") in header
    assert ("int hsw_gadget_digest_batch_device(hsw_gadget *g, size_t n, const void *const *d_inputs,\n"
            "                                   const size_t *input_lens, const size_t *precomputed_input_lens,\n"
            "                                   hsw_hash_result *results);") in header
    # the header says what is not checked
    comment = header[header.index("hsw_gadget_digest_batch_device for messages that DEPEND"):header.index("int hsw_gadget_digest_levels_device(")]
    assert "bound columns included" in comment and "NOT checked" in comment
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn hsw_gadget_digest_levels_device\(\s*g: \*mut hsw_gadget,\s*n: usize,\s*d_inputs: \*const \*const c_void,\s*"
                     r"input_lens: \*const usize,\s*precomputed_input_lens: \*const usize,\s*levels: \*const u32,\s*"
                     r"d_outputs: \*const \*mut c_void,\s*results: \*mut hsw_hash_result,?\s*\) -> c_int;", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "digest_levels_device") and hasattr(hsw.Sha256DynamicConfig, "merkle_tree_device")


def test_argument_rules_that_need_no_device(hsw):
    N = hsw._native
    lib = N.lib()
    ptrs = (C.c_void_p * 1)(64)
    lens = (C.c_size_t * 1)(5)
    outs = (C.c_void_p * 1)(128)
    lv = (C.c_uint32 * 1)(0)
    res = (N.HashResult * 1)()
    assert lib.hsw_gadget_digest_levels_device(None, 1, ptrs, lens, None, lv, outs, res) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_digest_levels_device(None, 1, ptrs, lens, None, None, None, res) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_digest_levels_device(None, 1, ptrs, lens, None, None, None, None) == N.HSW_ERR_INVALID_ARG


class _NoLibrary:
    """Stands where the library handle would: any call into it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were validated" % name)


def test_python_validates_everything_before_the_library_is_called(hsw):
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.lib, cfg.h, cfg._n, cfg._pending = _NoLibrary(), None, 0, []
    ok = [(4096, 5), (8192, 7)]
    for kw, exc in ((dict(levels=[0]), ValueError), (dict(levels=[0, -1]), ValueError), (dict(levels=[0, 1 << 32]), ValueError),
                    (dict(outputs=[4096 + 64]), ValueError), (dict(outputs=[0, None]), ValueError),
                    (dict(outputs=[b"x" * 32, None]), TypeError), (dict(outputs=[True, None]), TypeError),
                    (dict(precomputed_input_lens=[64]), ValueError)):
        with pytest.raises(exc):
            cfg.digest_levels_device(ok, **kw)
    with pytest.raises(ValueError):
        cfg.digest_levels_device([(0, 5)])                      # the device-fed call's own input rule
    import torch
    nodes = torch.zeros(32 * 5, dtype=torch.uint8)
    for leaves in ([], [(4096, 1)] * 3, [(4096, 1)] * 6):
        with pytest.raises(ValueError):
            cfg.merkle_tree_device(leaves, nodes)
    with pytest.raises(TypeError):
        cfg.merkle_tree_device([(4096, 1)] * 2, torch.zeros(96, dtype=torch.int32))
    with pytest.raises(ValueError):
        cfg.merkle_tree_device([(4096, 1)] * 2, torch.zeros(96, dtype=torch.uint8))     # not on the device
    cfg.h = None                                                # (nothing for __del__ to destroy)


def test_device_levels_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "device_levels_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "device_levels_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "device levels lifecycle ok" in res.stdout
