"""The lookup argument's grand product (hsw_gadget_lookup_product) without a GPU: the public surface -- one symbol with
one signature in the header, in _native.py and in hsw-sys, two structs, three status bits, the ABI numbers unchanged, the
new kernels in libhsw.so --, the argument rules of the Python wrapper, and two stand-alone programs under ASan + UBSan:
tests/cpp/fr_mul_check.cpp (the device's Fr arithmetic of csrc/hsw_fr_mul.hpp and the row rules of
csrc/hsw_product_value.hpp against a shift-and-add model) and, with the stand-in HIP runtime and LeakSanitizer,
tests/cpp/lookup_product_lifecycle.cpp (refusals, argument counts, launches, scratch)."""
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
    name = "hsw_gadget_lookup_product"
    assert name in N.SYMBOLS and hasattr(lib, name) and lib.hsw_gadget_lookup_product.restype is C.c_int
    assert lib.hsw_gadget_lookup_product.argtypes == [C.c_void_p, C.POINTER(N.LookupProduct), C.POINTER(N.ProductReport)]
    assert (C.sizeof(N.LookupProduct), C.sizeof(N.ProductReport)) == (104, 72)
    assert [f[0] for f in N.LookupProduct._fields_] == ["table", "flags", "usable_rows", "n_arguments", "d_inputs", "d_inputs_spread", "input_rows",
                                                        "d_permuted_inputs", "d_permuted_tables", "d_products", "thetas", "betas", "gammas", "status"]
    assert [f[0] for f in N.ProductReport._fields_] == ["arguments", "written", "open_arguments", "first_open", "refused_arguments", "first_refused",
                                                        "tile_rows", "reserved_", "kernel_ms", "tiles_ms", "scan_ms", "write_ms"]
    assert (N.HSW_PRODUCT_OPEN, N.HSW_PRODUCT_ZERO_DENOM, N.HSW_PRODUCT_CELL_NOT_BELOW_P) == (1, 2, 4)
    for decl in (r"int hsw_gadget_lookup_product\(hsw_gadget \*g, const hsw_lookup_product \*args, hsw_product_report \*report\);",
                 r"#define HSW_PRODUCT_OPEN\s+1u\b", r"#define HSW_PRODUCT_ZERO_DENOM\s+2u\b", r"#define HSW_PRODUCT_CELL_NOT_BELOW_P 4u"):
        assert re.search(decl, header), decl
    assert re.search(r"typedef struct hsw_lookup_product \{\s*uint32_t table, flags;[^}]*uint64_t usable_rows;[^}]*size_t n_arguments;[^}]*"
                     r"const void \*const \*d_inputs;[^}]*const void \*const \*d_inputs_spread;[^}]*const uint64_t \*input_rows;[^}]*"
                     r"const void \*const \*d_permuted_inputs;[^}]*const void \*const \*d_permuted_tables;[^}]*void \*const \*d_products;[^}]*"
                     r"const void \*thetas, \*betas, \*gammas;[^}]*uint32_t \*status;[^}]*\} hsw_lookup_product;", header)
    assert re.search(r"typedef struct hsw_product_report \{\s*uint64_t arguments, written;[^}]*uint64_t open_arguments, first_open;\s*"
                     r"uint64_t refused_arguments, first_refused;[^}]*uint32_t tile_rows, reserved_;\s*"
                     r"float kernel_ms, tiles_ms, scan_ms, write_ms;\s*\} hsw_product_report;", header)
    for decl in (r"pub fn hsw_gadget_lookup_product\(g: \*mut hsw_gadget, args: \*const hsw_lookup_product,\s*report: \*mut hsw_product_report\) -> c_int;",
                 r"pub const HSW_PRODUCT_OPEN: u32 = 1;", r"pub const HSW_PRODUCT_ZERO_DENOM: u32 = 2;", r"pub const HSW_PRODUCT_CELL_NOT_BELOW_P: u32 = 4;"):
        assert re.search(decl, rs), decl
    assert re.search(r"pub struct hsw_lookup_product \{\s*pub table: u32,\s*pub flags: u32,\s*pub usable_rows: u64,\s*pub n_arguments: usize,\s*"
                     r"pub d_inputs: \*const \*const c_void,\s*pub d_inputs_spread: \*const \*const c_void,\s*pub input_rows: \*const u64,\s*"
                     r"pub d_permuted_inputs: \*const \*const c_void,\s*pub d_permuted_tables: \*const \*const c_void,\s*"
                     r"pub d_products: \*const \*mut c_void,\s*pub thetas: \*const c_void,\s*pub betas: \*const c_void,\s*pub gammas: \*const c_void,\s*"
                     r"pub status: \*mut u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_product_report \{\s*pub arguments: u64,\s*pub written: u64,\s*pub open_arguments: u64,\s*pub first_open: u64,\s*"
                     r"pub refused_arguments: u64,\s*pub first_refused: u64,\s*pub tile_rows: u32,\s*pub reserved_: u32,\s*"
                     r"pub kernel_ms: f32,\s*pub tiles_ms: f32,\s*pub scan_ms: f32,\s*pub write_ms: f32,\s*\}", rs)
    assert hasattr(hsw.Sha256DynamicConfig, "lookup_product")
    blob = open(N.LIB_PATH, "rb").read()
    for kernel in (b"hsw_product_tiles_kernel", b"hsw_product_scan_kernel", b"hsw_product_write_kernel"):
        assert kernel in blob, kernel                                        # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import torch
    N = hsw._native
    rep = N.ProductReport()
    assert N.lib().hsw_gadget_lookup_product(None, C.byref(N.LookupProduct()), C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.n_contexts, cfg.context_images, cfg.max_variable_byte_sizes = 3, False, [64]
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    S, R = N.HSW_LOOKUP_SPREAD, N.HSW_LOOKUP_RANGE
    ch = [1, 2, 3]
    col = torch.zeros((6, 300, 4), dtype=torch.uint64)
    z = torch.zeros((6, 301, 4), dtype=torch.uint64)
    rng = torch.zeros((3, 65536, 4), dtype=torch.uint64)
    good = dict(betas=ch, gammas=ch, inputs=col, permuted_input=col, permuted_table=col, thetas=ch, inputs_spread=col, out=z)

    def but(**kw):
        d = dict(good)
        d.update(kw)
        return d
    for args, kw in (((7, 300), good),                                                   # no such table
                     ((S, 255), good),                                                   # usable_rows below the table size
                     ((R, 65535), dict(betas=ch, gammas=ch, inputs=rng, permuted_input=rng, permuted_table=rng)),
                     ((S, (1 << 31) + 1), good),
                     ((S, 300), but(thetas=None)),
                     ((S, 300), but(thetas=[1, 2])),                                     # one per proof
                     ((S, 300), but(betas=[1, 2, 3, 4])),
                     ((S, 300), but(gammas=None)),
                     ((S, 300), but(inputs_spread=None)),                                # the spread argument reads two columns
                     ((R, 65536), dict(betas=ch, gammas=ch, inputs=rng, permuted_input=rng, permuted_table=rng, inputs_spread=rng)),
                     ((R, 65536), dict(betas=ch, gammas=ch, inputs=rng, permuted_input=rng, permuted_table=rng, thetas=ch)),
                     ((S, 300), but(inputs=col.to(torch.int64))),                        # dtype
                     ((S, 300), but(permuted_input=torch.zeros((5, 300, 4), dtype=torch.uint64))),     # one column per argument
                     ((S, 300), but(permuted_table=torch.zeros((6, 299, 4), dtype=torch.uint64))),     # fewer rows than usable
                     ((S, 300), but(out=torch.zeros((6, 300, 4), dtype=torch.uint64))),                # Z has usable_rows + 1
                     ((S, 300), but(out=torch.zeros((6, 301, 8), dtype=torch.uint64)[:, :, ::2])),     # not contiguous
                     ((S, 300), but(out=z.to("meta"))),                                  # another device
                     ((S, 300), but(out=[1, 2, 3])),
                     ((S, 300), but(inputs=[16, 32, 48, 64, 80])),                       # addresses: one per argument
                     ((S, 300), but(inputs=[16, 32, 48, 64, 80, 8])),                    # ... 16-byte aligned
                     ((S, 300), but(inputs=[16, 32, 48, 64, 80, 0])),
                     ((S, 300), but(input_rows=[300] * 5)),
                     ((S, 300), but(input_rows=[300] * 5 + [301]))):
        with pytest.raises(ValueError):
            cfg.lookup_product(*args, **kw)
    # a short input tensor must still hold the rows that input_rows declares
    with pytest.raises(ValueError):
        cfg.lookup_product(S, 300, **but(inputs=torch.zeros((6, 10, 4), dtype=torch.uint64), input_rows=[11, 0, 3, 10, 9, 1]))


def test_fr_arithmetic_and_product_rows_under_asan_ubsan(tmp_path):
    hipcc = _hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    cxx = clang if os.path.exists(clang) else "g++"
    exe = str(tmp_path / "fr_mul_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "fr_mul_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    got = re.search(r"fr mul check ok: (\d+) operand pairs, (\d+) columns", res.stdout)
    # 6 x 6 corner pairs, 300 random pairs, 12 x 6 x 2 mixed ones; u in {1, 2, 5} x 3 kinds and u = 64 x 1 kind, x 2 cell forms x 2
    assert got and int(got.group(1)) == 36 + 300 + 144 and int(got.group(2)) == (3 * 3 + 1) * 4


def test_lookup_product_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, "hsw_lookup_product.o")]         # (the entry point refers to these kernels alone)
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_product.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "lookup_product_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "lookup_product_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "lookup product lifecycle ok" in res.stdout
