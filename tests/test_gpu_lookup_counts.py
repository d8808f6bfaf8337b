"""hsw_gadget_lookup_multiplicities on the MI355X: per-proof multiplicity tables of the range lookup (2^16 rows) and of
the spread lookup (2^num_bits_lookup rows), counted by hsw_lookup_counts_kernel from the cells where they lie.

The yardstick is the CPU oracle: its lookup stream and chip cells for the same messages (oracle.digest_cells, one call
per Context, as tests/test_gpu_origin.py / test_gpu_context_groups.py obtain them), binned with numpy.bincount.  Tables
must be EQUAL counter for counter, the totals equal to the run list's, not_in_table 0 -- also where every cell of the
caller's (queued lookup entries, interlude entries, rows past a column's used ones, everything between columns) holds a
sentinel that is no table row, so a run that reached one cell too far would be seen."""
import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.test_gpu_bound_column_tables import CarvedAll, geometry
from tests.test_gpu_bound_columns import interleaved
from tests.test_gpu_bound_region import MAX_ROWS, REPR, Slabs, interlude_after_digest0, make

pytestmark = pytest.mark.gpu
ORIGIN = (2, 131000, False, 5)              # column 2, row 131000, no zero cell yet, 5 lookups queued by the caller
PATTERN = 0x55AA1234                        # what a pre-filled counter holds
_REF = {}


def _msg(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def spread_of(t):
    return sum(((t >> b) & 1) << (2 * b) for b in range(16))


def oracle_tables(oracle, msgs, sizes, bits=8, ncols=2):
    """(range table, spread table, ref) of ONE Context that digests msgs: bincount over the oracle's own cells."""
    key = (tuple(msgs), tuple(sizes), bits, ncols)
    if key not in _REF:
        ref = oracle.digest_cells(list(msgs), list(sizes), None, True, num_bits_lookup=bits, num_advice_columns=ncols)
        lk = ref["lookup"]
        assert not lk[:, 1:].any() and int(lk[:, 0].max()) < 65536
        n = ref["LC"] * (sum(sizes) // 64)
        dense = np.concatenate([ref["dense"][k, : -(-(n - k) // ncols)] for k in range(ncols)])
        spread = np.concatenate([ref["spread"][k, : -(-(n - k) // ncols)] for k in range(ncols)])
        assert len(dense) == n and not dense[:, 1:].any() and not spread[:, 1:].any()
        assert all(int(s) == spread_of(int(d)) for d, s in zip(dense[:64, 0], spread[:64, 0]))
        _REF[key] = (np.bincount(lk[:, 0].astype(np.int64), minlength=65536), np.bincount(dense[:, 0].astype(np.int64), minlength=1 << bits), ref)
    return _REF[key]


def check(cfg, exp, bits=8, **kw):
    """One count of both tables against the per-Context oracle tables `exp`; returns (range, spread, report, runs)."""
    runs = cfg.lookup_runs()
    assert runs == sorted(runs, key=lambda r: (r["context"], r["table"], r["column"], r["first"]))
    r, s, rep = cfg.lookup_multiplicities(**kw)
    print("lookup counts: %d + %d entries, not_in_table %d, kernel %.3f ms" % (rep["range_entries"], rep["spread_entries"],
                                                                               rep["not_in_table"], rep["kernel_ms"]))
    assert rep["range_entries"] == sum(x["n"] for x in runs if x["table"] == 0)
    assert rep["spread_entries"] == sum(x["n"] for x in runs if x["table"] == 1)
    assert rep["not_in_table"] == 0, rep
    rh, sh = r.cpu().numpy(), s.cpu().numpy()
    for c, (er, es, _) in enumerate(exp):
        assert np.array_equal(rh[c, :65536], er), "range table of proof %d" % c
        assert np.array_equal(sh[c, : 1 << bits], es), "spread table of proof %d" % c
    assert rep["range_entries"] == sum(int(e[0].sum()) for e in exp) and rep["spread_entries"] == sum(int(e[1].sum()) for e in exp)
    return r, s, rep, runs


# ---- 1. a linear whole-digest stream: every table width, 2 and 3 chip columns, both cell forms, both kernels ----------
@REPR
@pytest.mark.parametrize("bits,ncols", [(8, 2), (8, 3), (16, 2), (1, 2)], ids=["8bit_lds", "8bit_3_columns", "16bit_large_table", "1bit_two_bins"])
def test_linear_stream(hsw, oracle, kernel_choice, bits, ncols, mont):
    N = hsw._native
    sizes = [128, 64] if bits > 1 else [64]                 # 3 blocks; 1 block of the 1-bit table (8 x the limb calls)
    msgs = [_msg(7, 100), _msg(8, 20)] if bits > 1 else [_msg(9, 40)]
    exp = [oracle_tables(oracle, msgs, sizes, bits, ncols)]
    eng = hsw.WitnessEngine(0, bits, ncols, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        eng.set_option("split", -1 if kernel_choice == "default" else 0)
        cfg = hsw.Sha256DynamicConfig(eng, sizes, is_input_range_check=True, whole_digest=True)
        if mont:
            cfg.set_repr(N.HSW_REPR_MONTGOMERY)
        assert cfg.lookup_runs() == []
        cfg.digest_batch(msgs)
        before = cfg.streams()
        r, s, rep, runs = check(cfg, exp, bits)
        assert [(x["table"], x["column"]) for x in runs] == [(0, 0)] + [(1, k) for k in range(ncols)]     # the two digests' entries: one run
        n = exp[0][2]["LC"] * (sum(sizes) // 64)
        assert [x["n"] for x in runs[1:]] == [-(-(n - k) // ncols) for k in range(ncols)]
        assert r.shape == (1, 65536) and s.shape == (1, 1 << bits) and r.dtype == s.dtype
        # the count wrote nothing but counters: the verifier still passes, the region is bit-identical
        assert cfg.verify()["violations"] == 0
        after = cfg.streams()
        for name in ("gate", "lookup", "dense", "spread"):
            assert np.array_equal(before[name], after[name]), name
        cfg.reset()
        assert cfg.lookup_runs() == []
        cfg.close()
    finally:
        eng.close()


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


# ---- 2. accumulate, pitches above the table size, one table only ------------------------------------------------------
def test_accumulate_and_pitches(hsw, oracle, eng_int):
    import torch
    sizes, msgs = [128, 64], [_msg(7, 100), _msg(8, 20)]
    er, es, _ = oracle_tables(oracle, msgs, sizes)
    cfg = make(hsw, eng_int, "single", sizes, 1, ORIGIN, True)          # a column image at (2, 131000), 5 lookups queued, Montgomery
    cfg.digest_batch(msgs)
    runs = cfg.lookup_runs()
    assert runs[0]["table"] == 0 and runs[0]["first"] == 5
    # (4 bytes past a 16-byte line: the tables are aligned for 4-byte stores only)
    r = torch.full((1, 65536 + 25), PATTERN, dtype=torch.int32, device="cuda")[:, 1:]
    s = torch.full((1, 256 + 4), PATTERN, dtype=torch.int32, device="cuda")[:, 1:]
    assert r.is_contiguous() and r.data_ptr() % 16 == 4 and s.data_ptr() % 16 == 4
    for accumulate, times in ((False, 1), (True, 2), (True, 3), (False, 1)):
        r2, s2, rep = cfg.lookup_multiplicities(out_range=r, out_spread=s, accumulate=accumulate)
        assert r2 is r and s2 is s and rep["not_in_table"] == 0
        rh, sh = r.cpu().numpy(), s.cpu().numpy()
        assert np.array_equal(rh[0, :65536], times * er) and np.array_equal(sh[0, :256], times * es), (accumulate, times)
        assert (rh[0, 65536:] == PATTERN).all() and (sh[0, 256:] == PATTERN).all()      # between tables: the caller's
    # one table only: the other tensor is not touched, its entries are not looked at
    s.fill_(PATTERN)
    r2, s2, rep = cfg.lookup_multiplicities(spread=False, out_range=r)
    assert s2 is None and rep["spread_entries"] == 0 and rep["range_entries"] == int(er.sum()) and (s.cpu().numpy() == PATTERN).all()
    r2, s2, rep = cfg.lookup_multiplicities(range=False)
    assert r2 is None and np.array_equal(s2.cpu().numpy()[0], es) and rep["range_entries"] == 0
    with pytest.raises(hsw.HswError) as ei:                              # a misaligned table: refused by the library itself
        N = hsw._native
        args = N.LookupCounts(r.data_ptr() + 2, None, 0, 0, 0, 0)
        cfg._ok(cfg.lib.hsw_gadget_lookup_multiplicities(cfg.h, args, N.LookupReport()))
    assert ei.value.status == hsw._native.HSW_ERR_INVALID_ARG
    assert cfg.verify()["violations"] == 0
    cfg.close()
    # a gadget without a lookup column: the spread table alone
    plain = hsw.WitnessEngine(0, 8, 2)
    try:
        g = hsw.Sha256DynamicConfig(plain, sizes, is_input_range_check=False)
        g.digest_batch(msgs)
        assert [x["table"] for x in g.lookup_runs()] == [1, 1]
        with pytest.raises(hsw.HswError) as ei:
            g.lookup_multiplicities()
        assert ei.value.status == hsw._native.HSW_ERR_UNSUPPORTED
        _, s3, rep = g.lookup_multiplicities(range=False)
        assert np.array_equal(s3.cpu().numpy()[0], es) and rep["not_in_table"] == 0
        g.close()
    finally:
        plain.close()


# ---- 3. a shared context with an interlude; K = 3 context images, all and 2 of 3 digested -----------------------------
@REPR
def test_shared_context_with_an_interlude(hsw, oracle, eng_int, mont):
    sizes, msgs = [64, 128], [_msg(21, 30), _msg(22, 101)]
    decl = interlude_after_digest0(hsw, eng_int, sizes, ORIGIN)
    cfg = make(hsw, eng_int, "shared", sizes, 1, ORIGIN, mont, decl)
    sl = Slabs(cfg, 1, MAX_ROWS + 12)                       # every cell of the caller's a sentinel: no table row
    cfg.bind_region(**sl.kw)
    cfg.digest_batch(msgs)
    _, _, _, runs = check(cfg, [oracle_tables(oracle, msgs, sizes)])
    rng = [x for x in runs if x["table"] == 0]
    assert len(rng) == 2 and rng[0]["first"] == 5 and rng[1]["first"] == rng[0]["first"] + rng[0]["n"] + 11
    assert cfg.verify()["violations"] == 0
    cfg.close()


@REPR
@pytest.mark.parametrize("digested", [3, 2])
def test_context_images(hsw, oracle, eng_int, mont, digested):
    import torch
    sizes, K = [64], 3
    msgs = [_msg(30 + c, 10 + 20 * c) for c in range(K)]
    cfg = make(hsw, eng_int, "images", sizes, K, ORIGIN, mont)
    cfg.digest_batch(msgs[:digested])
    exp = [oracle_tables(oracle, [m], sizes) for m in msgs[:digested]]
    r = torch.full((K, 65536 + 8), PATTERN, dtype=torch.int32, device="cuda")        # pitches above the table sizes
    s = torch.full((K, 256 + 4), PATTERN, dtype=torch.int32, device="cuda")
    _, _, _, runs = check(cfg, exp, out_range=r, out_spread=s)
    assert {x["context"] for x in runs} == set(range(digested)) and len(runs) == 3 * digested
    assert (r[:, 65536:].cpu().numpy() == PATTERN).all() and (s[:, 256:].cpu().numpy() == PATTERN).all()   # between tables: the caller's
    for c in range(digested, K):                            # a proof without runs: its tables are the caller's
        assert (r[c].cpu().numpy() == PATTERN).all() and (s[c].cpu().numpy() == PATTERN).all()
    assert cfg.verify()["violations"] == 0
    cfg.close()


# ---- 4. a Context group M = 2, K = 2: unbound, bound by pitch, bound by pointer tables in shuffled order --------------
G_SIZES, G_K = [128, 64], 2


def group_msgs():
    return [[_msg(40 + 2 * c, 90 + c), _msg(41 + 2 * c, 33 + c)] for c in range(G_K)]


def group_decl(hsw, eng):
    return interlude_after_digest0(hsw, eng, G_SIZES, ORIGIN)


@REPR
@pytest.mark.parametrize("binding", ["unbound", "pitch", "tables"])
def test_context_group(hsw, oracle, eng_int, mont, binding):
    msgs, decl = group_msgs(), group_decl(hsw, eng_int)
    cfg = make(hsw, eng_int, "group", G_SIZES, G_K, ORIGIN, mont, decl)
    keep = None
    if binding == "pitch":                                  # lookup_pitch and chip_context_pitch = a whole slab: larger than needed
        keep = Slabs(cfg, G_K, MAX_ROWS + 12)
        cfg.bind_region(**keep.kw)
    elif binding == "tables":
        columns, lp, rows = geometry(hsw, eng_int, "group", G_SIZES, G_K, ORIGIN, mont, decl)
        keep = CarvedAll(G_K, columns, interleaved(G_K, columns, list(range(columns))[::-1]), lp, rows)
        cfg.bind_columns(**keep.kw)
    cfg.digest_batch([m for ctx in msgs for m in ctx])
    exp = [oracle_tables(oracle, m, G_SIZES) for m in msgs]
    _, _, _, runs = check(cfg, exp)
    assert [(x["context"], x["table"], x["column"]) for x in runs] == [(c, t, k) for c in range(G_K) for t, k in ((0, 0), (0, 0), (1, 0), (1, 1))]
    if binding == "tables":                                 # the addresses are the caller's own pointers
        for x in runs:
            if x["table"] == 0:
                assert x["d_cells"] == keep.kw["lookup_ptrs"][x["context"]] + 32 * x["first"]
            else:
                i = x["context"] * 2 + x["column"]
                assert (x["d_cells"], x["d_spread"]) == (keep.kw["chip_dense_ptrs"][i], keep.kw["chip_spread_ptrs"][i])
    assert cfg.verify()["violations"] == 0
    cfg.close()


# ---- 5. entries that are no table row --------------------------------------------------------------------------------
@REPR
def test_non_members_are_counted_apart(hsw, oracle, eng_int, mont):
    import torch
    msgs, decl = group_msgs(), group_decl(hsw, eng_int)
    cfg = make(hsw, eng_int, "group", G_SIZES, G_K, ORIGIN, mont, decl)
    sl = Slabs(cfg, G_K, MAX_ROWS + 12)
    cfg.bind_region(**sl.kw)
    cfg.digest_batch([m for ctx in msgs for m in ctx])
    exp = [oracle_tables(oracle, m, G_SIZES) for m in msgs]
    _, _, _, runs = check(cfg, exp)
    base = sl.t.data_ptr()

    def poke(addr, value, plus_p=False):
        """the whole cell at a device address := value, in the gadget's representation; plus_p: stored as m + p"""
        cell = np.array([[(value >> (64 * i)) & (2**64 - 1) for i in range(4)]], dtype=np.uint64)
        if mont:
            cell = oracle.to_montgomery(cell)
        if plus_p:
            m = sum(int(x) << (64 * i) for i, x in enumerate(cell[0])) + P_INT
            assert mont and m < 1 << 256
            cell = np.array([[(m >> (64 * i)) & (2**64 - 1) for i in range(4)]], dtype=np.uint64)
        assert (addr - base) % 32 == 0
        sl.t[(addr - base) // 32] = torch.from_numpy(cell.view(np.int64)[0]).cuda()
        torch.cuda.synchronize()
    want = [(e[0].copy(), e[1].copy()) for e in exp]
    # proof 1, second range run, entry 7 := 2^16; proof 1, first range run, entry 100 := 2^64 + 5 (its low limb alone would pass)
    r1 = [x for x in runs if x["context"] == 1 and x["table"] == 0]
    lk1 = exp[1][2]["lookup"][:, 0].astype(np.int64)        # proof 1's own entries in order: first run, then second
    poke(r1[1]["d_cells"] + 32 * 7, 1 << 16)
    want[1][0][lk1[r1[0]["n"] + 7]] -= 1
    poke(r1[0]["d_cells"] + 32 * 100, (1 << 64) + 5)
    want[1][0][lk1[100]] -= 1
    # proof 1, chip column 1, row 9: the spread cell := spread(dense) + 1
    c1 = [x for x in runs if x["context"] == 1 and x["table"] == 1 and x["column"] == 1][0]
    d = int(exp[1][2]["dense"][1, 9, 0])
    poke(c1["d_spread"] + 32 * 9, spread_of(d) + 1)
    want[1][1][d] -= 1
    bad = 3
    if mont:
        # A Montgomery cell is an encoding m < p.  Stored as m + p it reduces to the same value, but the whole 32-byte
        # value is then no table row: proof 1, first range run, entry 200 and chip column 0, row 11, the spread cell.
        poke(r1[0]["d_cells"] + 32 * 200, int(lk1[200]), plus_p=True)
        want[1][0][lk1[200]] -= 1
        c0 = [x for x in runs if x["context"] == 1 and x["table"] == 1 and x["column"] == 0][0]
        d0 = int(exp[1][2]["dense"][0, 11, 0])
        poke(c0["d_spread"] + 32 * 11, spread_of(d0), plus_p=True)
        want[1][1][d0] -= 1
        bad = 5
    r, s, rep = cfg.lookup_multiplicities()
    assert rep["not_in_table"] == bad, rep
    # the lowest in (context, table, column, entry) order: proof 1's range entry 100 of its first run
    assert (rep["first_context"], rep["first_table"], rep["first_column"], rep["first_entry"]) == (1, 0, 0, r1[0]["first"] + 100), rep
    rh, sh = r.cpu().numpy(), s.cpu().numpy()
    for c in range(G_K):
        assert np.array_equal(rh[c], want[c][0]) and np.array_equal(sh[c], want[c][1]), c
        assert int(rh[c].sum() + sh[c].sum()) == int(exp[c][0].sum() + exp[c][1].sum()) - (bad if c == 1 else 0)
    cfg.close()
