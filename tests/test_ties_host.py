"""Digest-to-digest copy constraints (hsw_gadget_ties, hsw_gadget_cell_address, hsw_gadget_verify_ties,
hsw_gadget_verify_equal) without a GPU: the public surface -- four symbols with one signature in the header, in
_native.py and in hsw-sys, the ABI numbers unchanged -- the refusals that need no device, and, under ASan + UBSan +
LeakSanitizer with the stand-in HIP runtime, tests/cpp/ties_lifecycle.cpp: the derivation of the ties (replayed here
through a model of a dozen lines from what the program handed to the library), the cap / NULL rules, cell addresses
against position arithmetic and against the caller's own column pointers, no launch for a refused or empty check."""
import ctypes as C
import os
import re

import pytest

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)

NEW = ("hsw_gadget_ties", "hsw_gadget_cell_address", "hsw_gadget_verify_ties", "hsw_gadget_verify_equal")


def test_symbols_signatures_and_abi_numbers(hsw):
    N = hsw._native
    lib = N.lib()
    assert lib.hsw_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "hsw.h")).read()
    assert re.search(r"#define HSW_ABI_VERSION 3\b", header) and re.search(r"#define HSW_ABI_MINOR 1\b", header)
    rs = open(os.path.join(ROOT, "rust", "hsw-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert name in N.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    u64p = C.POINTER(C.c_uint64)
    assert lib.hsw_gadget_ties.argtypes == [C.c_void_p, C.POINTER(N.CellTie), C.c_size_t, C.POINTER(C.c_size_t), u64p]
    assert lib.hsw_gadget_cell_address.argtypes == [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    assert lib.hsw_gadget_verify_ties.argtypes == [C.c_void_p, C.POINTER(N.TieReport)]
    assert lib.hsw_gadget_verify_equal.argtypes == [C.c_void_p, u64p, u64p, C.c_size_t, C.POINTER(N.TieReport)]
    assert C.sizeof(N.CellTie) == 40 and C.sizeof(N.TieReport) == 32
    assert [f[0] for f in N.CellTie._fields_] == ["src_hash", "dst_hash", "src_byte", "dst_byte", "src_cell", "dst_cell"]
    assert [f[0] for f in N.TieReport._fields_] == ["violations", "checks", "first", "kernel_ms"]
    for decl in (r"int hsw_gadget_ties\(const hsw_gadget \*g, hsw_cell_tie \*out, size_t cap, size_t \*n, uint64_t \*prefix_bytes_untied\);",
                 r"int hsw_gadget_cell_address\(const hsw_gadget \*g, uint64_t cell, void \*\*d_cell\);",
                 r"int hsw_gadget_verify_ties\(hsw_gadget \*g, hsw_tie_report \*report\);",
                 r"int hsw_gadget_verify_equal\(hsw_gadget \*g, const uint64_t \*cells_a, const uint64_t \*cells_b, size_t n, hsw_tie_report \*report\);"):
        assert re.search(decl, header), decl
    assert re.search(r"typedef struct hsw_cell_tie \{\s*uint64_t src_hash, dst_hash;[^}]*uint32_t src_byte, dst_byte;[^}]*uint64_t src_cell, dst_cell;[^}]*\} hsw_cell_tie;", header)
    assert re.search(r"typedef struct hsw_tie_report \{\s*uint64_t violations, checks, first;[^}]*float kernel_ms;\s*\} hsw_tie_report;", header)
    for decl in (r"pub fn hsw_gadget_ties\(g: \*const hsw_gadget, out: \*mut hsw_cell_tie, cap: usize, n: \*mut usize,\s*prefix_bytes_untied: \*mut u64\) -> c_int;",
                 r"pub fn hsw_gadget_cell_address\(g: \*const hsw_gadget, cell: u64, d_cell: \*mut \*mut c_void\) -> c_int;",
                 r"pub fn hsw_gadget_verify_ties\(g: \*mut hsw_gadget, report: \*mut hsw_tie_report\) -> c_int;",
                 r"pub fn hsw_gadget_verify_equal\(g: \*mut hsw_gadget, cells_a: \*const u64, cells_b: \*const u64, n: usize,\s*report: \*mut hsw_tie_report\) -> c_int;"):
        assert re.search(decl, rs), decl
    assert re.search(r"pub struct hsw_cell_tie \{\s*pub src_hash: u64,\s*pub dst_hash: u64,\s*pub src_byte: u32,\s*pub dst_byte: u32,\s*"
                     r"pub src_cell: u64,\s*pub dst_cell: u64,\s*\}", rs)
    assert re.search(r"pub struct hsw_tie_report \{\s*pub violations: u64,\s*pub checks: u64,\s*pub first: u64,\s*pub kernel_ms: f32,\s*\}", rs)
    for name in ("ties", "cell_address", "verify_ties", "verify_equal", "merkle_tree_device"):
        assert hasattr(hsw.Sha256DynamicConfig, name)


def test_argument_rules_that_need_no_device(hsw):
    N = hsw._native
    lib = N.lib()
    n, rep, p = C.c_size_t(7), N.TieReport(), C.c_void_p()
    cells = (C.c_uint64 * 1)(0)
    assert lib.hsw_gadget_ties(None, None, 0, C.byref(n), None) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_cell_address(None, 0, C.byref(p)) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_verify_ties(None, C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_verify_equal(None, cells, cells, 1, C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    with pytest.raises(ValueError):
        cfg.verify_equal([1, 2], [1])                        # before the library is called


def _model(msgs):
    """The ties of a pass, from the issue's words: calls in order; inside a call the levels in ascending order, a
    level's messages first READ (every byte some earlier write of the pass owns is a tie, or a counted prefix byte)
    and then WRITE their 32 destination bytes, each byte taking its new owner."""
    owner, ties, prefix = {}, [], 0
    for call in sorted({m["call"] for m in msgs}):
        mine = [m for m in msgs if m["call"] == call]
        for level in sorted({m["level"] for m in mine}):
            now = [m for m in mine if m["level"] == level]
            for m in now:
                for off in range(m["len"] if m["device"] else 0):
                    if m["src"] + off in owner and off < m["pre"]:
                        prefix += 1
                    elif m["src"] + off in owner:
                        ties.append(owner[m["src"] + off][:1] + (m["hash"],) + owner[m["src"] + off][1:] + (off - m["pre"],))
            for m in now:
                owner.update({m["dst"] + j: (m["hash"], j) for j in range(32 if m["dst"] else 0)})
    return sorted(ties, key=lambda t: (t[1], t[3])), prefix


def test_ties_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "ties_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "ties_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "ties lifecycle ok" in res.stdout
    cases, msgs, ties = {}, [], []
    for line in res.stdout.splitlines():
        w = line.split()
        if w[0] == "MSG":
            msgs.append(dict(zip(("hash", "call", "level", "device", "src", "len", "pre", "dst"), map(int, w[1:]))))
        elif w[0] == "TIE":
            ties.append(tuple(map(int, w[1:])))
        elif w[0] == "CASE":
            cases[w[1]] = (msgs, ties, int(w[2]), int(w[3]))
            msgs, ties = [], []
    want = dict(tree2=(64, 0), after_reset=(0, 0), tree4=(192, 0), shuffled=(192, 0), partial=(37, 0), prefix=(32, 64),
                unwritten_slot=(0, 0), two_calls=(64, 0), rewritten=(64, 0), context_group=(128, 0), pointer_table=(64, 0),
                block_stream=(0, 0))
    assert set(cases) == set(want)
    for name, (m, t, n, prefix) in cases.items():
        assert (n, prefix) == want[name] and len(t) == n, name
        if name == "block_stream":                           # no byte cells: nothing is recorded, every call refuses
            continue
        assert (t, prefix) == _model(m), name
    # what the cases are about, said once more on the printed lists
    group = cases["context_group"][1]
    assert all(s // 3 == d // 3 for s, d, _, _ in group) and {d for _, d, _, _ in group} == {2, 5}
    assert cases["unwritten_slot"][0][2]["len"] == 64 and not cases["unwritten_slot"][1]
    assert [t[0] for t in cases["rewritten"][1]] == [0] * 16 + [2] * 32 + [1] * 16
    assert cases["prefix"][1][0][3] == 0 and cases["two_calls"][0][2]["device"] == 0
