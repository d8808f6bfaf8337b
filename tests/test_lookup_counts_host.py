"""Lookup-table multiplicities (hsw_gadget_lookup_runs, hsw_gadget_lookup_multiplicities) without a GPU: the public
surface -- two symbols with one signature in the header, in _native.py and in hsw-sys, three structs, the ABI numbers
unchanged --, the refusals that need no device, and, under ASan + UBSan + LeakSanitizer with the stand-in HIP runtime,
tests/cpp/lookup_counts_lifecycle.cpp: the run list of seven kinds of pass, checked here against a model of a dozen
lines (counts from the closed forms, addresses from the geometry the program printed, no caller entry inside a run)."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from tests.test_host_sanitizers import CSRC, ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)

NEW = ("hsw_gadget_lookup_runs", "hsw_gadget_lookup_multiplicities")


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
    assert lib.hsw_gadget_lookup_runs.argtypes == [C.c_void_p, C.POINTER(N.LookupRun), C.c_size_t, C.POINTER(C.c_size_t)]
    assert lib.hsw_gadget_lookup_multiplicities.argtypes == [C.c_void_p, C.POINTER(N.LookupCounts), C.POINTER(N.LookupReport)]
    assert (C.sizeof(N.LookupRun), C.sizeof(N.LookupCounts), C.sizeof(N.LookupReport)) == (48, 40, 56)
    assert [f[0] for f in N.LookupRun._fields_] == ["context", "table", "column", "first", "n", "d_cells", "d_spread"]
    assert [f[0] for f in N.LookupCounts._fields_] == ["d_range", "d_spread", "range_pitch", "spread_pitch", "flags", "reserved_"]
    assert [f[0] for f in N.LookupReport._fields_] == ["range_entries", "spread_entries", "not_in_table", "first_context", "first_entry",
                                                       "first_table", "first_column", "kernel_ms", "reserved_"]
    assert (N.HSW_LOOKUP_RANGE, N.HSW_LOOKUP_SPREAD, N.HSW_LOOKUP_ACCUMULATE) == (0, 1, 1)
    for decl in (r"int hsw_gadget_lookup_runs\(const hsw_gadget \*g, hsw_lookup_run \*out, size_t cap, size_t \*n\);",
                 r"int hsw_gadget_lookup_multiplicities\(hsw_gadget \*g, const hsw_lookup_counts \*out, hsw_lookup_report \*report\);",
                 r"#define HSW_LOOKUP_RANGE 0u\b", r"#define HSW_LOOKUP_SPREAD 1u\b", r"#define HSW_LOOKUP_ACCUMULATE 1u\b"):
        assert re.search(decl, header), decl
    assert re.search(r"typedef struct hsw_lookup_run \{\s*uint64_t context;[^}]*uint32_t table;[^}]*uint32_t column;[^}]*uint64_t first;[^}]*"
                     r"uint64_t n;[^}]*void \*d_cells;[^}]*void \*d_spread;[^}]*\} hsw_lookup_run;", header)
    assert re.search(r"typedef struct hsw_lookup_counts \{\s*uint32_t \*d_range;[^}]*uint32_t \*d_spread;[^}]*uint64_t range_pitch;[^}]*"
                     r"uint64_t spread_pitch;[^}]*uint32_t flags, reserved_;\s*\} hsw_lookup_counts;", header)
    assert re.search(r"typedef struct hsw_lookup_report \{\s*uint64_t range_entries, spread_entries;[^}]*uint64_t not_in_table;[^}]*"
                     r"uint64_t first_context, first_entry;[^}]*uint32_t first_table, first_column;\s*float kernel_ms; uint32_t reserved_;\s*"
                     r"\} hsw_lookup_report;", header)
    for decl in (r"pub fn hsw_gadget_lookup_runs\(g: \*const hsw_gadget, out: \*mut hsw_lookup_run, cap: usize, n: \*mut usize\) -> c_int;",
                 r"pub fn hsw_gadget_lookup_multiplicities\(g: \*mut hsw_gadget, out: \*const hsw_lookup_counts,\s*report: \*mut hsw_lookup_report\) -> c_int;",
                 r"pub const HSW_LOOKUP_RANGE: u32 = 0;", r"pub const HSW_LOOKUP_SPREAD: u32 = 1;", r"pub const HSW_LOOKUP_ACCUMULATE: u32 = 1;"):
        assert re.search(decl, rs), decl
    assert re.search(r"pub struct hsw_lookup_run \{\s*pub context: u64,\s*pub table: u32,\s*pub column: u32,\s*pub first: u64,\s*pub n: u64,\s*"
                     r"pub d_cells: \*mut c_void,\s*pub d_spread: \*mut c_void,\s*\}", rs)
    assert re.search(r"pub struct hsw_lookup_counts \{\s*pub d_range: \*mut u32,\s*pub d_spread: \*mut u32,\s*pub range_pitch: u64,\s*"
                     r"pub spread_pitch: u64,\s*pub flags: u32,\s*pub reserved_: u32,\s*\}", rs)
    assert re.search(r"pub struct hsw_lookup_report \{\s*pub range_entries: u64,\s*pub spread_entries: u64,\s*pub not_in_table: u64,\s*"
                     r"pub first_context: u64,\s*pub first_entry: u64,\s*pub first_table: u32,\s*pub first_column: u32,\s*pub kernel_ms: f32,\s*"
                     r"pub reserved_: u32,\s*\}", rs)
    for name in ("lookup_runs", "lookup_multiplicities"):
        assert hasattr(hsw.Sha256DynamicConfig, name)
    blob = open(N.LIB_PATH, "rb").read()
    assert b"hsw_lookup_counts_kernel" in blob and b"hsw_lookup_zero_kernel" in blob       # the library's own gfx950 code


def test_argument_rules_that_need_no_device(hsw):
    import torch
    N = hsw._native
    lib = N.lib()
    n, rep = C.c_size_t(7), N.LookupReport()
    table = (C.c_uint32 * 65536)()
    args = N.LookupCounts(C.addressof(table), C.addressof(table), 0, 0, 0, 0)
    assert lib.hsw_gadget_lookup_runs(None, None, 0, C.byref(n)) == N.HSW_ERR_INVALID_ARG
    assert lib.hsw_gadget_lookup_multiplicities(None, C.byref(args), C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    # (both table pointers NULL, a short pitch, a misaligned pointer: refused on a live gadget before any launch, which
    #  the stand-alone program below checks against the stub's launch counter -- a gadget needs an engine, an engine a device)
    cfg = object.__new__(hsw.Sha256DynamicConfig)
    cfg.h = None
    cfg.n_contexts, cfg.context_images, cfg.max_variable_byte_sizes = 3, False, [64]
    cfg.engine = types.SimpleNamespace(device=torch.device("cpu"), shape=hsw.shape_query(8, 2))
    cfg.lib = types.SimpleNamespace()                        # any call into the library would be an AttributeError
    good = torch.zeros((3, 65536), dtype=torch.int32)
    for kw in (dict(range=False, spread=False),
               dict(out_range=torch.zeros((3, 65536), dtype=torch.int64)),           # dtype
               dict(out_range=torch.zeros((2, 65536), dtype=torch.int32)),           # one row per Context
               dict(out_range=torch.zeros((3, 65535), dtype=torch.int32)),           # a pitch below the table size
               dict(out_range=torch.zeros((3 * 65536,), dtype=torch.int32)),         # not 2-D
               dict(out_range=torch.zeros((3, 2 * 65536), dtype=torch.int32)[:, ::2]),   # not contiguous
               dict(out_range=good, out_spread=torch.zeros((3, 255), dtype=torch.int32)),
               dict(out_range=good, out_spread=[0] * 256),                           # not a tensor
               dict(range=False, out_range=good),                                    # a tensor for a table not asked for
               dict(accumulate=True),                                                # nothing to accumulate into
               dict(out_range=good.to("meta"))):                                     # another device
        with pytest.raises(ValueError):
            cfg.lookup_multiplicities(**kw)


def _model(dig, caller, limbs):
    """The run list from the issue's words.  RANGE: one run per committed digest -- 3 + 2 * max * rc + n_blocks * 3184 + 64
    entries from where its own entries start -- neighbours of one Context merged where they touch; SPREAD: per
    (Context, chip column k) the committed limb calls n = k (mod ncols), ceil((N - k) / ncols) rows from row 0.
    In (context, table, column, first) order."""
    runs = []
    for cx, first, n_blocks, size, rc in dig:
        n = 3 + 2 * size * rc + n_blocks * 3184 + 64
        if runs and runs[-1][0] == cx and runs[-1][3] + runs[-1][4] == first:
            runs[-1][4] += n
        else:
            runs.append([cx, 0, 0, first, n])
    for cx, total, ncols in limbs:
        runs += [[cx, 1, k, 0, -(-(total - k) // ncols)] for k in range(ncols) if total > k]
    return sorted(runs)


def test_lookup_counts_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    kernel = os.path.join(CSRC, "hsw_lookup_counts.o")
    if not os.path.exists(kernel):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_lookup.cpp"), out),
             _compile(hipcc, os.path.join(ROOT, "tests", "cpp", "lookup_counts_lifecycle.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels + [kernel], "lookup_counts_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "lookup counts lifecycle ok" in res.stdout
    cases, cur = {}, dict(DIG=[], CALLER=[], CTX=[], LIMBS=[], RUN=[])
    for line in res.stdout.splitlines():
        w = line.split()
        if w[0] in cur:
            cur[w[0]].append(tuple(map(int, w[1:])))
        elif w[0] == "CASE":
            cases[w[1]] = (cur, int(w[2]))
            cur = dict(DIG=[], CALLER=[], CTX=[], LIMBS=[], RUN=[])
    want = dict(fresh=0, block_stream=3, origin=3, after_reset=0, shared_interlude=4, images_2_of_3=6, group_pitch=8, group_tables=8)
    assert {k: v[1] for k, v in cases.items()} == want
    for name, (c, n) in cases.items():
        runs = c["RUN"]
        assert len(runs) == n
        assert [list(r[:5]) for r in runs] == _model(c["DIG"], c["CALLER"], c["LIMBS"]), name
        ctx = {x[0]: x[1:] for x in c["CTX"]}
        for cx, table, col, first, cnt, d_cells, d_spread in runs:
            ncols = (len(ctx[cx]) - 1) // 2
            if table == 0:                                   # the Context's lookup column + the entry
                assert d_cells == ctx[cx][0] + 32 * first and d_spread == 0, name
                for ccx, lo, hi in c["CALLER"]:              # no caller entry inside a run
                    assert ccx != cx or hi <= first or lo >= first + cnt, name
            else:                                            # the Context's chip column k of either family + the row
                assert d_cells == ctx[cx][1 + col] + 32 * first and d_spread == ctx[cx][1 + ncols + col] + 32 * first, name
    # what the cases are about, said once more on the printed lists
    assert [r[4] for r in cases["block_stream"][0]["RUN"]] == [2747, 2747, 2746]          # 8,240 limb calls over 3 columns
    assert cases["origin"][0]["RUN"][0][3] == 5
    sh = [r for r in cases["shared_interlude"][0]["RUN"] if r[1] == 0]
    assert len(sh) == 2 and sh[1][3] == sh[0][3] + sh[0][4] + 11
    assert {r[0] for r in cases["images_2_of_3"][0]["RUN"]} == {0, 1}
    for name in ("group_pitch", "group_tables"):
        assert [(r[0], r[1]) for r in cases[name][0]["RUN"]] == [(0, 0), (0, 0), (0, 1), (0, 1), (1, 0), (1, 0), (1, 1), (1, 1)]
    lk = [x[1] for x in cases["group_tables"][0]["CTX"]]
    assert lk[1] < lk[0]                                     # the tables' address order is not the Contexts'
