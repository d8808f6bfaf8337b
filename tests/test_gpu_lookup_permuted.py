"""hsw_gadget_lookup_permuted on the MI355X: halo2's permuted lookup columns A' and S' of every argument of a table,
written by the kernels of hsw_lookup_permuted.hip.

The yardstick is a numpy / Python-int model of the contract in include/hsw.h: multiplicities m (counted mode: numpy.bincount
over the CPU oracle's own cells, obtained as tests/test_gpu_lookup_counts.py obtains them; given mode: the test's own),
m'[0] = m[0] + (u - E), A' = row t repeated m'[t] times, S' = the first position of every run holds the run's row and the
other positions the leftover rows (row 0 (u - T) + [m'[0] = 0] times, then every unused t > 0) in ascending order.  The
value of a row is a Python int (t, t * theta + spread(t) or t + spread(t) * theta mod p; Montgomery cells: times 2^256
mod p).  Comparison is exact equality.  Every column lies between sentinel cells -- before row 0 and from row u on --
which must be unchanged after every call."""
import ctypes as C

import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.test_gpu_bound_column_tables import CarvedAll, geometry
from tests.test_gpu_bound_columns import interleaved
from tests.test_gpu_bound_region import MAX_ROWS, REPR, Slabs, make
from tests.test_gpu_lookup_counts import G_K, G_SIZES, ORIGIN, _msg, group_decl, group_msgs, oracle_tables, spread_of

pytestmark = pytest.mark.gpu
PAD = 3                                     # sentinel cells before row 0 and after row u - 1 of every column
SENT = 0x5A5A5A5A5A5A5A5A
R_INT = (1 << 256) % P_INT
_VAL = {}


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


def limbs(values):
    """Python ints below 2^256 -> (n, 4) uint64"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4)


def stored(theta, mont):
    return theta * R_INT % P_INT if mont else theta


def value_table(kind, T, theta, mont):
    """(T, 4) uint64: the cell of every table row.  kind: 'range', 'spread' (t * theta + spread(t)), 'on_spread'"""
    key = (kind, T, theta, mont)
    if key not in _VAL:
        if kind == "range":
            vals = list(range(T))
        elif kind == "spread":
            vals = [(t * theta + spread_of(t)) % P_INT for t in range(T)]
        else:
            vals = [(t + spread_of(t) * theta) % P_INT for t in range(T)]
        _VAL[key] = limbs([v * R_INT % P_INT for v in vals] if mont else vals)
    return _VAL[key]


def model_rows(m, u):
    """The table rows of A' and S' for multiplicities m (sum <= u), from the words of the contract."""
    m = np.asarray(m, dtype=np.int64)
    T = len(m)
    mp = m.copy()
    mp[0] += u - int(m.sum())
    off = np.concatenate([[0], np.cumsum(mp)[:-1]])
    a = np.repeat(np.arange(T), mp)
    assert len(a) == u
    s = np.full(u, -1, dtype=np.int64)
    used = mp > 0
    s[off[used]] = np.arange(T)[used]
    unused = np.arange(1, T)[~used[1:]]
    left = np.concatenate([np.zeros((u - T) + (0 if used[0] else 1), dtype=np.int64), unused])
    assert len(left) == u - int(used.sum())
    s[s < 0] = left
    # the two permuted-pair constraints, on the model itself
    assert a[0] == s[0] and np.all((a[1:] == s[1:]) | (a[1:] == a[:-1]))
    return a, s


def call(cfg, hsw, table, u, n_args, thetas=None, m=None, flags=0, order="ascending", want_m=True):
    """One call through the C ABI with the columns carved out of one sentinel-filled buffer, in the slot order `order`.
    Returns (A, S, m, report): A, S (n_args, u, 4) uint64; the sentinels are checked here."""
    import torch
    N = hsw._native
    stride = u + 2 * PAD
    slots = list(range(2 * n_args))
    if order == "reversed":
        slots = slots[::-1]
    elif order == "interleaved":
        slots = slots[1::2] + slots[0::2]
    buf = torch.full((2 * n_args * stride, 4), SENT, dtype=torch.int64, device="cuda")
    base = buf.data_ptr()
    ptr = [base + (s * stride + PAD) * 32 for s in slots]
    T = 1 << int(cfg.engine.shape.num_bits_lookup) if table == N.HSW_LOOKUP_SPREAD else 65536
    if m is not None:
        d_m = torch.from_numpy(np.ascontiguousarray(m, dtype=np.int64).astype(np.uint32).view(np.int32)).cuda()
        flags |= N.HSW_PERMUTED_GIVEN_M
    else:
        d_m = torch.full((n_args, T + 5), 0x55AA1234, dtype=torch.int32, device="cuda") if want_m else None
    th = np.ascontiguousarray(limbs(thetas)) if thetas is not None else None
    args = N.LookupPermuted(table, flags, u, n_args, (C.c_void_p * n_args)(*ptr[:n_args]), (C.c_void_p * n_args)(*ptr[n_args:]),
                            th.ctypes.data if th is not None else None, d_m.data_ptr() if d_m is not None else None,
                            d_m.shape[1] if d_m is not None else 0)
    rep = N.PermutedReport()
    torch.cuda.synchronize()
    cfg._ok(cfg.lib.hsw_gadget_lookup_permuted(cfg.h, C.byref(args), C.byref(rep)))
    host = buf.cpu().numpy().view(np.uint64).reshape(2 * n_args, stride, 4)
    assert (host[:, :PAD] == SENT).all() and (host[:, PAD + u:] == SENT).all(), "a cell outside rows [0, u) was written"
    cols = host[:, PAD: PAD + u]
    A = np.stack([cols[slots[a]] for a in range(n_args)])
    S = np.stack([cols[slots[n_args + a]] for a in range(n_args)])
    mh = d_m.cpu().numpy().view(np.uint32) if d_m is not None else None
    if mh is not None and m is None:
        assert (mh[:, T:] == 0x55AA1234).all()                    # between the tables: the caller's
    report = {f[0]: getattr(rep, f[0]) for f in N.PermutedReport._fields_}
    print("permuted: %d arguments, u %d, written %d, prepare %.3f ms, write %.3f ms" % (n_args, u, report["written"], report["prepare_ms"], report["write_ms"]))
    return A, S, mh, report


def expect(A, S, ms, u, tables):
    """Every argument's columns against the model: ms[a] its multiplicities, tables[a] its value table"""
    for a, m in enumerate(ms):
        ra, rs = model_rows(m, u)
        assert np.array_equal(A[a], tables[a][ra]), "A' of argument %d" % a
        assert np.array_equal(S[a], tables[a][rs]), "S' of argument %d" % a


def column_counts(ref, sizes, bits, ncols):
    """per chip column k: (rows, bincount of its dense cells) of ONE Context from the oracle's cells"""
    n = ref["LC"] * (sum(sizes) // 64)
    out = []
    for k in range(ncols):
        rows = -(-(n - k) // ncols)
        out.append((rows, np.bincount(ref["dense"][k, :rows, 0].astype(np.int64), minlength=1 << bits)))
    return out


def theta_of(seed):
    return int.from_bytes(np.random.default_rng(seed).bytes(40), "little") % P_INT


# ---- 1. counted mode, a linear whole-digest stream: every table width, 2 and 3 chip columns, both cell forms ----------
@REPR
@pytest.mark.parametrize("bits,ncols", [(8, 2), (8, 3), (16, 2), (1, 2)], ids=["8bit", "8bit_3_columns", "16bit_large_table", "1bit_two_rows"])
def test_counted_linear_stream(hsw, oracle, bits, ncols, mont):
    N = hsw._native
    sizes = [128, 64] if bits > 1 else [64]
    msgs = [_msg(7, 100), _msg(8, 20)] if bits > 1 else [_msg(9, 40)]
    er, es, ref = oracle_tables(oracle, msgs, sizes, bits, ncols)
    eng = hsw.WitnessEngine(0, bits, ncols, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        cfg = hsw.Sha256DynamicConfig(eng, sizes, is_input_range_check=True, whole_digest=True)
        if mont:
            cfg.set_repr(N.HSW_REPR_MONTGOMERY)
        cfg.digest_batch(msgs)
        before = cfg.streams()
        # RANGE: one argument, the proof's own entries
        u = 65536 + 3
        A, S, m, rep = call(cfg, hsw, N.HSW_LOOKUP_RANGE, u, 1)
        assert rep["written"] == 2 * u and rep["not_in_table"] == 0 and rep["entries"] == int(er.sum()) and rep["arguments"] == 1
        assert np.array_equal(m[0, :65536], er)
        expect(A, S, [er], u, [value_table("range", 65536, 0, mont)])
        # SPREAD: one argument per chip column, the column's own rows
        cc = column_counts(ref, sizes, bits, ncols)
        u = cc[0][0] + 1 if bits <= 8 else 65536 + 3
        theta = theta_of(100 + bits + ncols)
        A, S, m, rep = call(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, ncols, thetas=[stored(theta, mont)], order="reversed")
        assert rep["written"] == 2 * u * ncols and rep["not_in_table"] == 0 and rep["entries"] == sum(r for r, _ in cc)
        T = 1 << bits
        for k in range(ncols):
            assert np.array_equal(m[k, :T], cc[k][1]), k
        expect(A, S, [c for _, c in cc], u, [value_table("spread", T, theta, mont)] * ncols)
        # the per-argument tables sum to the per-proof table of hsw_gadget_lookup_multiplicities
        _, s_proof, _ = cfg.lookup_multiplicities(range=False)
        assert np.array_equal(m[:, :T].astype(np.int64).sum(axis=0), s_proof.cpu().numpy()[0].astype(np.int64))
        assert np.array_equal(s_proof.cpu().numpy()[0], es)
        # without d_m: the same columns
        A2, S2, m2, _ = call(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, ncols, thetas=[stored(theta, mont)], want_m=False)
        assert m2 is None and np.array_equal(A2, A) and np.array_equal(S2, S)
        # nothing of the region was written: the verifier still passes, the streams are bit-identical
        assert cfg.verify()["violations"] == 0
        after = cfg.streams()
        for name in ("gate", "lookup", "dense", "spread"):
            assert np.array_equal(before[name], after[name]), name
        cfg.close()
    finally:
        eng.close()


# ---- 2. theta = 0, HSW_PERMUTED_THETA_ON_SPREAD, E = u exactly, an empty pass, the Python wrapper --------------------
@REPR
def test_theta_variants_and_exact_fill(hsw, oracle, eng_int, mont):
    N = hsw._native
    sizes, msgs = [64], [_msg(9, 40)]
    _, _, ref = oracle_tables(oracle, msgs, sizes)
    cc = column_counts(ref, sizes, 8, 2)
    assert cc[0][0] == cc[1][0] == 2060
    cfg = hsw.Sha256DynamicConfig(eng_int, sizes, is_input_range_check=True, whole_digest=True)
    if mont:
        cfg.set_repr(N.HSW_REPR_MONTGOMERY)
    # nothing digested yet: an empty run list, every row unassigned
    theta = theta_of(5)
    A, S, m, rep = call(cfg, hsw, N.HSW_LOOKUP_SPREAD, 300, 2, thetas=[stored(theta, mont)])
    assert rep["entries"] == 0 and rep["written"] == 2 * 300 * 2 and not m[:, :256].any()
    tab = value_table("spread", 256, theta, mont)
    expect(A, S, [np.zeros(256, dtype=np.int64)] * 2, 300, [tab, tab])
    # A' is u x val(0); S' is the table and its padding: row 0 and its 44 copies first, as the leftover rule orders them
    assert (A == tab[0]).all() and (S[0, :45] == tab[0]).all() and np.array_equal(S[0, 45:], tab[1:])
    cfg.digest_batch(msgs)
    u = 2060                                                    # E = u exactly: no unassigned row
    for kind, th, flags in (("spread", 0, 0), ("on_spread", theta, N.HSW_PERMUTED_THETA_ON_SPREAD), ("spread", P_INT - 1, 0)):
        A, S, m, rep = call(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, 2, thetas=[stored(th, mont)], flags=flags, order="interleaved")
        assert rep["written"] == 4 * u and rep["entries"] == 2 * u
        expect(A, S, [c for _, c in cc], u, [value_table(kind, 256, th, mont)] * 2)
    # refusals of the library itself: one entry too many for u, a theta that is not below p
    for kw, u2 in ((dict(thetas=[stored(theta, mont)]), u - 1), (dict(thetas=[P_INT]), u)):
        with pytest.raises(hsw.HswError) as ei:
            call(cfg, hsw, N.HSW_LOOKUP_SPREAD, u2, 2, **kw)
        assert ei.value.status == N.HSW_ERR_INVALID_ARG
        assert ("argument 0" in str(ei.value)) == (u2 == u - 1)        # the text names the argument with too many entries
    # the Python wrapper: its own tensors, rows from u on are the caller's
    a, s, counts, rep = cfg.lookup_permuted(N.HSW_LOOKUP_SPREAD, u + 7, thetas=[stored(theta, mont)])
    assert a.shape == s.shape == (2, u + 7, 4) and counts.shape == (2, 256) and rep["written"] == 4 * (u + 7)
    expect(a.cpu().numpy(), s.cpu().numpy(), [c for _, c in cc], u + 7, [tab, tab])
    a2, s2, _, rep = cfg.lookup_permuted(N.HSW_LOOKUP_RANGE, 65536)
    assert a2.shape == (1, 65536, 4) and rep["written"] == 2 * 65536
    cfg.close()


# ---- 3. given multiplicities: the corner multisets, both table sizes, groups of one proof, overflow -------------------
def corner_ms(T, u, rng):
    one = np.ones(T, dtype=np.int64)
    last = np.zeros(T, dtype=np.int64); last[T - 1] = u                       # all of u on row T - 1: m'[0] = 0
    full = one.copy(); full[0] = 0; full[1] = u - (T - 2)                    # E = u with m'[0] = 0
    sparse = np.zeros(T, dtype=np.int64)
    np.add.at(sparse, rng.integers(0, T, size=u // 2) // 7 * 7 % T, 1)      # E = u / 2 on every 7th row
    dense = np.bincount(rng.integers(0, T, size=u), minlength=T)             # E = u, random
    return [np.zeros(T, dtype=np.int64), last, full, one, sparse, dense]     # (one: no repeated position where u = T)


@REPR
@pytest.mark.parametrize("table,u", [("spread", 256), ("spread", 257), ("spread", 4099), ("range", 65536), ("range", 65536 + 2060)])
def test_given_multiplicities(hsw, eng_int, table, u, mont):
    N = hsw._native
    K = 3
    cfg = make(hsw, eng_int, "images", [64], K, ORIGIN, mont)                  # 3 proofs: 3 range, 6 spread arguments; nothing digested
    T, n_args = (256, 6) if table == "spread" else (65536, 3)
    ms = corner_ms(T, u, np.random.default_rng(u))
    thetas = [theta_of(60 + c) for c in range(K)]
    tabs = [value_table("spread", T, thetas[a // 2], mont) for a in range(n_args)] if table == "spread" else [value_table("range", T, 0, mont)] * n_args
    tid = N.HSW_LOOKUP_SPREAD if table == "spread" else N.HSW_LOOKUP_RANGE
    kw = dict(thetas=[stored(t, mont) for t in thetas]) if table == "spread" else {}
    try:
        for lo in range(0, len(ms), n_args):
            part = (ms[lo: lo + n_args] * 2)[:n_args]
            A, S, _, rep = call(cfg, hsw, tid, u, n_args, m=np.stack(part), order="reversed", **kw)
            assert rep["written"] == 2 * u * n_args and rep["overflow_arguments"] == 0 and rep["entries"] == 0
            expect(A, S, part, u, tabs)
        eng_int.set_option("permuted_scratch", 1)                          # groups of one proof each: the same bytes
        A2, S2, _, rep = call(cfg, hsw, tid, u, n_args, m=np.stack(part), order="interleaved", **kw)
        assert rep["written"] == 2 * u * n_args and np.array_equal(A2, A) and np.array_equal(S2, S)
        # sum m = u + 1 in ONE argument (of the last group): nothing at all is written
        bad = [m.copy() for m in (ms * 2)[:n_args]]
        bad[n_args - 1] = np.zeros(T, dtype=np.int64); bad[n_args - 1][5] = u + 1
        A, S, _, rep = call(cfg, hsw, tid, u, n_args, m=np.stack(bad), **kw)
        assert rep["written"] == 0 and rep["overflow_arguments"] == 1 and rep["not_in_table"] == 0
        assert (A == SENT).all() and (S == SENT).all()
    finally:
        eng_int.set_option("permuted_scratch", 256 << 20)
    cfg.close()


# ---- 4. an entry that is no table row: reported, nothing written -----------------------------------------------------
@REPR
def test_offender_writes_nothing(hsw, oracle, eng_int, mont):
    import torch
    N = hsw._native
    sizes, msgs = [128, 64], [_msg(7, 100), _msg(8, 20)]
    cfg = make(hsw, eng_int, "single", sizes, 1, ORIGIN, mont)
    sl = Slabs(cfg, 1, MAX_ROWS + 12)
    cfg.bind_region(**sl.kw)
    cfg.digest_batch(msgs)
    run = [x for x in cfg.lookup_runs() if x["table"] == 1 and x["column"] == 1][0]
    cell = np.array([[5, 1, 0, 0]], dtype=np.uint64)                        # 2^64 + 5: the low limb alone would be a row
    if mont:
        cell = oracle.to_montgomery(cell)
    idx = (run["d_cells"] + 32 * 9 - sl.t.data_ptr()) // 32
    sl.t[idx] = torch.from_numpy(cell.view(np.int64)[0]).cuda()
    torch.cuda.synchronize()
    u = run["n"] + 1
    A, S, _, rep = call(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, 2, thetas=[stored(theta_of(3), mont)])
    assert rep["written"] == 0 and rep["not_in_table"] == 1 and rep["overflow_arguments"] == 0
    assert (rep["first_context"], rep["first_table"], rep["first_column"], rep["first_entry"]) == (0, 1, 1, 9), rep
    assert (A == SENT).all() and (S == SENT).all()
    # the range argument of the same pass is untouched by that cell
    A, S, _, rep = call(cfg, hsw, N.HSW_LOOKUP_RANGE, 65536, 1)
    assert rep["written"] == 2 * 65536 and rep["not_in_table"] == 0
    cfg.close()


# ---- 5. a Context group, K = 2, bound by pointer tables; Montgomery cells, a theta per proof -------------------------
def test_context_group_bound_by_pointer_tables(hsw, oracle, eng_int):
    N = hsw._native
    mont = True
    msgs, decl = group_msgs(), group_decl(hsw, eng_int)
    cfg = make(hsw, eng_int, "group", G_SIZES, G_K, ORIGIN, mont, decl)
    columns, lp, rows = geometry(hsw, eng_int, "group", G_SIZES, G_K, ORIGIN, mont, decl)
    keep = CarvedAll(G_K, columns, interleaved(G_K, columns, list(range(columns))[::-1]), lp, rows)
    cfg.bind_columns(**keep.kw)
    cfg.digest_batch([m for ctx in msgs for m in ctx])
    exp = [oracle_tables(oracle, m, G_SIZES) for m in msgs]
    u = 65536 + 3
    A, S, m, rep = call(cfg, hsw, N.HSW_LOOKUP_RANGE, u, G_K, order="reversed")
    assert rep["written"] == 2 * u * G_K and rep["not_in_table"] == 0
    expect(A, S, [e[0] for e in exp], u, [value_table("range", 65536, 0, mont)] * G_K)
    thetas = [theta_of(70 + c) for c in range(G_K)]
    cc = [column_counts(e[2], G_SIZES, 8, 2) for e in exp]
    u = max(r for c in cc for r, _ in c) + 1
    A, S, m, rep = call(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, 2 * G_K, thetas=[stored(t, mont) for t in thetas], order="reversed")
    assert rep["written"] == 2 * u * 2 * G_K and rep["not_in_table"] == 0
    expect(A, S, [cnt for c in cc for _, cnt in c], u, [value_table("spread", 256, thetas[a // 2], mont) for a in range(2 * G_K)])
    assert cfg.verify()["violations"] == 0
    cfg.close()
