"""The quotient h(X) of device columns (hsw_gadget_quotient) without a GPU: the model over Python integers that the GPU
tests import (tests/quotient_model.py), proven here on a SATISFIED toy circuit -- its h has the degree halo2 expects
and the identity sum of the folded expressions = h(X) (X^n - 1) holds at a random point, and with one witness cell
flipped it does not; the public surface (one symbol with one signature in the header, in _native.py and in hsw-sys, the
struct sizes and field offsets, the ABI numbers unchanged, the new kernels in libhsw.so); the argument rules of the
Python wrapper; and two stand-alone programs under ASan + UBSan: tests/cpp/quotient_value_check.cpp (the kernels'
thread bodies of csrc/hsw_quotient_value.hpp run on the CPU against the plain definition) and, with the stand-in HIP
runtime and LeakSanitizer, tests/cpp/quotient_lifecycle.cpp (refusals, launches, scratch, batches, destroy)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from tests.constraint_check import P_INT
from tests.ntt_model import root_of_unity
from tests.quotient_model import evaluate, from_extended, numerator_model, quotient_model, toy_at_point, toy_circuit, toy_extended
from tests.test_host_sanitizers import CSRC, ROOT, _compile, _hipcc, _link_and_run, host_objects  # noqa: F401 (fixture)
from tests.test_open_host import _standalone

E, ZETA, DEGREE = 2, 5, 4        # the extension; the coset; the highest degree among the expressions: l_active Z (..)(..)


def _h_coefficients(flip):
    t = toy_circuit(flip=flip)
    lr, ln = t["log_rows"], t["log_rows"] + E
    assert (lr, t["u"], t["L"], len(t["perm_z"])) == (4, 10, 2, 2)
    ext = toy_extended(t, E, ZETA)
    h, count = quotient_model(lr, ln, t["u"], ext["columns"], ext["fixed"], t["gates"], t["y"], root_of_unity(ln), ZETA, **ext["kw"])
    assert count == 2 + (2 + 1 + 2) + 2 * 5
    return t, from_extended(h, ln, ZETA)


def test_the_model_proves_a_satisfied_circuit():
    t, hc = _h_coefficients(False)
    lr, n = t["log_rows"], 1 << t["log_rows"]
    bound = (DEGREE - 1) * n
    assert any(hc[:bound]) and not any(hc[bound:])                           # every coefficient at and beyond (d - 1) n is 0
    for x in (3, 0x123456789ABCDEF0123456789ABCDEF0123456789 % P_INT):
        pt = toy_at_point(t, x)
        V, _ = numerator_model(lr, lr + E, t["u"], pt["columns"], pt["fixed"], t["gates"], t["y"], root_of_unity(lr + E), ZETA, at_x=x, **pt["kw"])
        assert V[0] == evaluate(hc, x) * (pow(x, n, P_INT) - 1) % P_INT      # sum of the folded expressions at x = h(x) (x^n - 1)


def test_one_flipped_witness_cell_breaks_the_degree_bound():
    t, hc = _h_coefficients(True)
    assert any(hc[(DEGREE - 1) * (1 << t["log_rows"]):])                     # the numerator no longer vanishes on the domain


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_symbol_signature_and_abi_numbers(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_VERSION 3\b", header) and re.search(r"#define HSW_ABI_MINOR 1\b", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    name = "hsw_gadget_quotient"
    assert name in N.SYMBOLS and N.SYMBOLS.count(name) == 1 and hasattr(lib, name) and getattr(lib, name).restype is C.c_int
    assert getattr(lib, name).argtypes == [C.c_void_p, C.POINTER(N.Quotient), C.POINTER(N.QuotientReport)]
    assert len(re.findall(r"\bint %s\(" % name, header)) == 1 and len(re.findall(r"pub fn %s\(" % name, rs)) == 1
    assert re.search(r"int hsw_gadget_quotient\(hsw_gadget \*g, const hsw_quotient \*args, hsw_quotient_report \*report\);", header)
    assert re.search(r"pub fn hsw_gadget_quotient\(g: \*mut hsw_gadget, args: \*const hsw_quotient, report: \*mut hsw_quotient_report\) -> c_int;", rs)
    assert (C.sizeof(N.QuotientGates), C.sizeof(N.QuotientLookups), C.sizeof(N.Quotient), C.sizeof(N.QuotientReport)) == (64, 72, 320, 80)
    # every field of the header's structs, in order, is the ctypes field of that name and the Rust field of that name
    for struct, cls in (("hsw_quotient_gates", N.QuotientGates), ("hsw_quotient_lookups", N.QuotientLookups), ("hsw_quotient", N.Quotient),
                        ("hsw_quotient_report", N.QuotientReport)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"^[\s\*]*(const\s+)?\**\s*", "", part).strip().split()[-1].lstrip("*") for part in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], (struct, names)
        rust = re.search(r"pub struct %s \{(.*?)\n\}" % struct, rs, re.S).group(1)
        assert re.findall(r"pub (\w+):", rust) == names, struct
    offsets = {f: getattr(N.Quotient, f).offset for f in ("usable_rows", "n_proofs", "d_columns", "d_l0", "gates", "n_perm_columns", "lookups", "betas", "omega_ext", "d_h", "status")}
    assert offsets == dict(usable_rows=16, n_proofs=24, d_columns=48, d_l0=64, gates=88, n_perm_columns=152, lookups=184, betas=256, omega_ext=280, d_h=304, status=312)
    assert (N.QuotientReport.launches.offset, N.QuotientReport.kernel_ms.offset, N.QuotientReport.finish_ms.offset) == (48, 56, 72)
    assert (N.HSW_QUOTIENT_CELL_NOT_BELOW_P, N.HSW_QUOTIENT_MAX_FACTORS, N.HSW_QUOTIENT_MAX_EXTENSION) == (4, 8, 8) and N.HSW_NTT_CELL_NOT_BELOW_P == 4
    for macro, value in (("HSW_QUOTIENT_CELL_NOT_BELOW_P", 4), ("HSW_QUOTIENT_MAX_FACTORS", 8), ("HSW_QUOTIENT_MAX_EXTENSION", 8)):
        assert re.search(r"#define %s %du\b" % (macro, value), header) and re.search(r"pub const %s: u32 = %d;" % (macro, value), rs)
    assert hasattr(hsw.Sha256DynamicConfig, "quotient")
    blob = open(N.LIB_PATH, "rb").read()
    for kernel in (b"hsw_quotient_gates_kernel", b"hsw_quotient_permutation_kernel", b"hsw_quotient_lookups_kernel", b"hsw_quotient_finish_kernel"):
        assert kernel in blob, kernel                                        # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import torch
    N = hsw._native
    assert N.lib().hsw_gadget_quotient(None, C.byref(N.Quotient()), C.byref(N.QuotientReport())) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    rows = 64
    cols = torch.zeros((2, 3, rows, 4), dtype=torch.uint64)
    col = torch.zeros((rows, 4), dtype=torch.uint64)
    good = dict(log_rows=4, log_n=6, usable_rows=10, columns=cols, ys=[2, 3], omega_ext=5, zeta=7, fixed=torch.zeros((2, rows, 4), dtype=torch.uint64),
                gates=[[(1, [(3, 0), (0, 0)]), (P_INT - 1, [(3, 0), (0, 3)])]], l0=col, l_last=col, l_active=col, perm_columns=[0, 4, 2], chunk_columns=2,
                sigmas=torch.zeros((3, rows, 4), dtype=torch.uint64), perm_products=torch.zeros((2, 2, rows, 4), dtype=torch.uint64), delta=7,
                betas=[1, 2], gammas=[3, 4], lookups=[([2], [3]), ([0, 4], [4, 1])], permuted_inputs=torch.zeros((2, 2, rows, 4), dtype=torch.uint64),
                permuted_tables=torch.zeros((2, 2, rows, 4), dtype=torch.uint64), lookup_products=torch.zeros((2, 2, rows, 4), dtype=torch.uint64),
                thetas=[5, 6])
    z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get("dtype", torch.uint64))        # noqa: E731
    bad = [(dict(log_n=29, log_rows=27), "log_n at most 28"), (dict(log_n=4), "log_n - log_rows 1 .. 8"), (dict(log_n=13), "log_n - log_rows 1 .. 8"),
           (dict(usable_rows=0), "usable_rows must be 1 .. 2^log_rows - 1"), (dict(usable_rows=16), "usable_rows must be 1 .. 2^log_rows - 1"),
           (dict(columns=cols.to(torch.int64)), "columns must be a uint64 tensor on cpu"),
           (dict(columns=z(2, 3, rows - 1, 4)), "columns must be contiguous, of shape (2, 3) + (rows >= 64, 4)"),    # fewer rows than are read
           (dict(columns=z(2, 3, rows, 8)[:, :, :, ::2]), "columns must be contiguous"),
           (dict(columns=cols.to("meta")), "columns must be a uint64 tensor on cpu"), (dict(columns=[]), "columns: at least one proof"),
           (dict(columns=[[16, 32, 0], [64, 80, 96]]), "columns: 6 device addresses"), (dict(columns=[[16, 32], [64, 80, 96]]), "columns: 4 device addresses"),
           (dict(fixed=z(2, rows - 1, 4)), "fixed must be contiguous, of shape (2,) + (rows >= 64, 4)"),
           (dict(gates=[[(1, [(5, 0)])]]), "gates: a column index is not below 5"), (dict(gates=[[(1, [(0, 16)])]]), "gates: a rotation is not below"),
           (dict(gates=[[(1, [(0, -16)])]]), "gates: a rotation is not below"), (dict(gates=[[(1, [(0, 0)] * 9)]]), "gates: a monomial has at most 8 factors"),
           (dict(gates=[[(1 << 256, [(0, 0)])]]), "gates: coefficients: field elements of 256 bits"),
           (dict(gates=[[(-1, [])]]), "gates: coefficients: field elements of 256 bits"),
           (dict(gates=[], perm_columns=[], lookups=[]), "nothing to fold"),
           (dict(perm_columns=[0, 5, 2]), "perm_columns: a column index is not below 5"), (dict(chunk_columns=0), "chunk_columns is at least 1"),
           (dict(sigmas=z(2, rows, 4)), "sigmas must be contiguous, of shape (3,)"),
           (dict(perm_products=z(2, 1, rows, 4)), "perm_products must be contiguous, of shape (2, 2)"), (dict(delta=None), "delta: 1 field element(s)"),
           (dict(betas=[1]), "betas: 2 field element(s)"), (dict(gammas=None), "gammas: 2 field element(s)"),
           (dict(l0=None), "l0: 1 column(s)"), (dict(l_active=z(rows - 1, 4)), "l_active must be contiguous"),
           (dict(lookups=[([], [3])]), "lookups: at least one input and one table column each"),
           (dict(lookups=[([2], [])]), "lookups: at least one input and one table column each"),
           (dict(lookups=[([2], [5]), ([0], [1])]), "lookups: a column index is not below 5"), (dict(thetas=[1, 2, 3]), "thetas: 2 field element(s)"),
           (dict(lookup_products=z(2, 1, rows, 4)), "lookup_products must be contiguous, of shape (2, 2)"),
           (dict(ys=[1]), "ys: 2 field element(s)"), (dict(ys=[1 << 256, 2]), "ys: field elements of 256 bits"), (dict(zeta=None), "zeta: 1 field element(s)"),
           (dict(omega_ext=[1, 2]), "omega_ext: 1 field element(s)"),
           (dict(out=z(2, rows, 4, dtype=torch.int64)), "out must be a uint64 tensor on cpu"), (dict(out=z(2, rows - 1, 4)), "out must be contiguous"),
           (dict(out=z(3, rows, 4)), "out must be contiguous, of shape (2,)"), (dict(out=[4096]), "out: 2 device addresses"),
           (dict(out=[4096, 0]), "out: 2 device addresses")]
    for kw, text in bad:                                     # each case trips the rule it names, and no other
        d = dict(good)
        d.update(kw)
        with pytest.raises(ValueError, match=re.escape(text)):
            cfg.quotient(**d)


# ---- the stand-alone programs -------------------------------------------------------------------------------------------
def test_quotient_thread_bodies_on_the_cpu_under_asan_ubsan(tmp_path):
    got = re.search(r"quotient value check ok: (\d+) runs, (\d+) rows", _standalone(tmp_path, "quotient_value_check"))
    assert got and int(got.group(1)) >= 30 and int(got.group(2)) > 5000


def test_quotient_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, "hsw_quotient.o")]               # (the entry point refers to these kernels alone)
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_quotient.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "quotient_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "quotient_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "quotient lifecycle ok" in res.stdout
