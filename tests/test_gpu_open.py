"""hsw_gadget_evaluate and hsw_gadget_open on the MI355X: device columns evaluated at points and opened, by the kernels
of hsw_open.hip.

The yardstick is Python integers: tests/open_model.py, proven in tests/test_open_host.py against the term-by-term
definitions.  Every cell of every quotient and every evaluation is compared with it, exactly, in both cell forms.  All
columns and quotients are carved out of one buffer with sentinel cells around each; after a call every byte of it
outside rows [0, rows) of the quotients that were to be written must be what it was.  Rows of a column at and beyond its
input_rows hold limbs far above p: a read of them shows as a refusal or as a wrong value.  out_evals and status are
pre-filled, so an entry that must not be written is seen to be untouched."""
import ctypes as C

import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.msm_model import chain, commitment, point_words
from tests.ntt_model import ntt_model, root_of_unity
from tests.open_model import evaluate_model, fold_model, open_model
from tests.test_gpu_bound_region import REPR, make
from tests.test_gpu_lookup_counts import ORIGIN
from tests.test_gpu_lookup_permuted import SENT, limbs, stored

pytestmark = pytest.mark.gpu
PAD = 3                                     # sentinel cells before and after every column and quotient
GARBAGE = (1 << 64) - 2                     # every limb of a cell that must not be read: far above p, and not 0
EVAL_FILL = 0xA5A5A5A5A5A5A5A5              # what out_evals holds before a call
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


def gadget(hsw, eng, mont):
    return make(hsw, eng, "images", [64], 1, ORIGIN, mont)                   # nothing digested: the columns are synthetic


def random_column(rng, h):
    return [int.from_bytes(rng.bytes(40), "little") % P_INT for _ in range(h)]


class Case:
    """Columns of `rows` cells (values[b]: the input_rows[b] values of column b) and n_quotients quotient slots."""

    def __init__(self, cfg, hsw, rows, mont, values, n_quotients=0):
        import torch
        self.cfg, self.N, self.rows, self.mont, self.values = cfg, hsw._native, rows, mont, [list(v) for v in values]
        self.n, self.heights = len(values), [len(v) for v in values]
        self.col_at, self.q_at, at = [], [], 0
        for _ in range(self.n):
            self.col_at.append(at + PAD)
            at += 2 * PAD + rows
        for _ in range(n_quotients):
            self.q_at.append(at + PAD)
            at += 2 * PAD + rows
        host = np.full((at, 4), np.uint64(SENT), dtype=np.uint64)
        for b, vals in enumerate(self.values):
            s = self.col_at[b]
            host[s: s + rows] = np.uint64(GARBAGE)
            if vals:
                host[s: s + len(vals)] = limbs([stored(x, mont) for x in vals])
        self.buf = torch.from_numpy(host.view(np.int64)).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 16 == 0

    def poke(self, b, row, x):
        """store the 256-bit integer x as cell `row` of column b"""
        import torch
        self.buf[self.col_at[b] + row] = torch.from_numpy(limbs([x]).copy().view(np.int64)[0]).cuda()
        torch.cuda.synchronize()

    def _common(self):
        import torch
        cols = (C.c_void_p * self.n)(*[self.base + 32 * a for a in self.col_at])
        hs = (C.c_uint64 * self.n)(*self.heights) if self.heights != [self.rows] * self.n else None
        torch.cuda.synchronize()
        return cols, hs, self.buf.cpu().numpy().view(np.uint64).copy()

    def enc(self, xs):
        return np.array(limbs([stored(x, self.mont) for x in xs]))            # (a writable copy)

    def evaluate(self, points, queries, tile_rows=0, refused=(), batches=1):
        """the call, then every check: returns (evals (queries, 4), status, report).  batches: the batches of columns the
        call is to take"""
        N, n = self.N, self.n
        cols, hs, before = self._common()
        nq = len(queries)
        z = self.enc(points)
        evals = np.full((nq, 4), np.uint64(EVAL_FILL), dtype=np.uint64)
        status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        args = N.Evaluate(0, tile_rows, self.rows, n, cols, hs, len(points), z.ctypes.data, nq, (C.c_uint32 * nq)(*[b for b, _ in queries]),
                          (C.c_uint32 * nq)(*[t for _, t in queries]), evals.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.EvaluateReport()
        rc = N.lib().hsw_gadget_evaluate(self.cfg.h, C.byref(args), C.byref(rep))
        assert rc == N.HSW_OK, rc
        print("evaluate: rows %d, columns %d, queries %d, tile_rows %d (%d tiles), launches %d, kernel %.3f ms, scratch %d bytes, status %s"
              % (self.rows, n, nq, rep.tile_rows, rep.tiles, rep.launches, rep.kernel_ms, rep.scratch_bytes, status.tolist()))
        assert np.array_equal(self.buf.cpu().numpy().view(np.uint64), before), "evaluate wrote device memory of the caller"
        refused = sorted(set(refused))
        assert [b for b in range(n) if status[b]] == refused and all(status[b] == N.HSW_OPEN_CELL_NOT_BELOW_P for b in refused)
        assert (rep.columns, rep.queries, rep.refused_columns, rep.first_refused) == (n, nq, len(refused), refused[0] if refused else NONE)
        assert rep.refused_queries == sum(1 for b, _ in queries if b in refused) and rep.thread_rows == N.HSW_OPEN_THREAD_ROWS
        assert rep.tile_rows == (tile_rows or 2048) and rep.tiles == -(-self.rows // rep.tile_rows) and rep.launches == 2 * batches
        for i, (b, t) in enumerate(queries):
            if b in refused:
                assert (evals[i] == np.uint64(EVAL_FILL)).all(), "query %d of a refused column was written" % i
            else:
                assert evals[i].tolist() == self.enc([evaluate_model(self.values[b], points[t])])[0].tolist(), "query %d: a wrong value" % i
        return evals, status, rep

    def open(self, groups, points, challenges, tile_rows=0, refused=(), expect=None, batches=1):
        """the call, then every check: returns (quotient cells per group or None, evals, status, report).  expect: the
        (q, eval) of every group, if the caller has them already; batches: the batches of groups the call is to take"""
        N, n, rows = self.N, self.n, self.rows
        ng = len(groups)
        assert ng <= len(self.q_at)
        cols, hs, before = self._common()
        first = [0]
        for grp in groups:
            first.append(first[-1] + len(grp))
        flat = [b for grp in groups for b in grp]
        z, v = self.enc(points), self.enc(challenges)
        evals = np.full((ng, 4), np.uint64(EVAL_FILL), dtype=np.uint64)
        status = np.full(ng, 0xFFFFFFFF, dtype=np.uint32)
        qs = (C.c_void_p * ng)(*[self.base + 32 * self.q_at[k] for k in range(ng)])
        args = N.Open(0, tile_rows, rows, n, cols, hs, ng, (C.c_uint64 * (ng + 1))(*first), (C.c_uint32 * len(flat))(*flat), z.ctypes.data,
                      v.ctypes.data, qs, evals.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.OpenReport()
        rc = N.lib().hsw_gadget_open(self.cfg.h, C.byref(args), C.byref(rep))
        assert rc == N.HSW_OK, rc
        print("open: rows %d, groups %d, tile_rows %d (%d tiles), batches %d, launches %d, kernel %.3f ms, scratch %d bytes, status %s"
              % (rows, ng, rep.tile_rows, rep.tiles, rep.batches, rep.launches, rep.kernel_ms, rep.scratch_bytes, status.tolist()))
        after = self.buf.cpu().numpy().view(np.uint64)
        refused = sorted(set(refused))
        assert [k for k in range(ng) if status[k]] == refused and all(status[k] == N.HSW_OPEN_CELL_NOT_BELOW_P for k in refused)
        assert (rep.groups, rep.refused_groups, rep.first_refused, rep.written) == (ng, len(refused), refused[0] if refused else NONE, rows * (ng - len(refused)))
        assert rep.tile_rows == (tile_rows or 2048) and rep.tiles == -(-rows // rep.tile_rows) and rep.launches == 3 * rep.batches and rep.batches == batches
        assert rep.thread_rows == N.HSW_OPEN_THREAD_ROWS
        mask = np.ones(len(before), dtype=bool)                               # the guard: everything but the quotients that were to be written
        out = []
        for k in range(ng):
            s = self.q_at[k]
            if k in refused:
                assert (evals[k] == np.uint64(EVAL_FILL)).all(), "out_evals of refused group %d was written" % k
                out.append(None)
                continue
            mask[s: s + rows] = False
            cells = after[s: s + rows]
            q, ev = expect[k] if expect is not None else open_model([self.values[b] for b in groups[k]], points[k], challenges[k], rows)
            want = self.enc(q)
            if not np.array_equal(cells, want):
                bad = int(np.nonzero((cells != want).any(axis=1))[0][0])
                raise AssertionError("group %d: quotient row %d differs" % (k, bad))
            assert evals[k].tolist() == self.enc([ev])[0].tolist(), "group %d: a wrong evaluation" % k
            assert not cells[rows - 1].any()                                  # q[rows-1] = 0: n_bases = rows commits it as it lies
            # the cross-check from the DEVICE quotient: eval = c[0] + z q[0]
            c0 = fold_model([self.values[b][:1] for b in groups[k]], challenges[k], 1)[0]
            q0 = int.from_bytes(cells[0].tobytes(), "little")
            q0 = q0 * pow(1 << 256, -1, P_INT) % P_INT if self.mont else q0
            assert ev == (c0 + points[k] * q0) % P_INT
            out.append(cells.copy())
        assert np.array_equal(after[mask], before[mask]), "something outside the quotients was written"
        return out, evals, status, rep


def heights_for(rows):
    return [rows, rows - 1, min(1, rows), 0, rows, rows - 1]


def edge_values(rng, rows):
    values = [random_column(rng, h) for h in heights_for(rows)]
    values[0][0] = P_INT - 1
    if rows >= 3:
        values[0][1], values[0][2] = 0, 1
        values[4][rows - 1] = 0
    return values


# ---- 1. rows at every boundary of a thread, a tile and the scan; the output does not depend on tile_rows -------------------
def _row_sizes(N):
    T, R = N.HSW_OPEN_MIN_TILE_ROWS, N.HSW_OPEN_THREAD_ROWS
    return [1, 2, 3, R - 1, R, R + 1, T - 1, T, T + 1, 2 * T + 3, 257 * T + 5]


@REPR
@pytest.mark.parametrize("which", range(11))
def test_rows_at_every_boundary_and_any_tile_rows(hsw, eng_int, mont, which):
    N = hsw._native
    T = N.HSW_OPEN_MIN_TILE_ROWS
    rows = _row_sizes(N)[which]
    assert rows >= 1
    rng = np.random.default_rng(1000 + which)
    values = edge_values(rng, rows)[:3]                                       # heights rows, rows - 1, 1 (or 0)
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values, n_quotients=2)
    groups, points, challenges = [[0], [1, 0, 2]], [random_column(rng, 1)[0], random_column(rng, 1)[0]], [0, random_column(rng, 1)[0]]
    expect = [open_model([values[b] for b in grp], z, v, rows) for grp, z, v in zip(groups, points, challenges)]
    out, evals, _, rep = case.open(groups, points, challenges, tile_rows=T, expect=expect)
    assert rep.tiles == -(-rows // T)
    if which == 10:
        assert rep.tiles > 256                                                # more tiles than the scan workgroup has threads
    queries = [(0, 0), (1, 1), (0, 1), (2, 0), (0, 0)]
    ev, _, _ = case.evaluate(points, queries, tile_rows=T)
    assert ev[0].tolist() == evals[0].tolist()                                # evaluate is open's out_evals for m = 1
    for other in (0, 2 * T, 4096):                                            # 4096: two sweeps per tile
        out2, evals2, _, _ = case.open(groups, points, challenges, tile_rows=other, expect=expect)
        assert all(np.array_equal(a, b) for a, b in zip(out, out2)) and np.array_equal(evals, evals2)
        ev2, _, _ = case.evaluate(points, queries, tile_rows=other)
        assert np.array_equal(ev, ev2)
    cfg.close()


# ---- 2. groups ------------------------------------------------------------------------------------------------------------------
@REPR
def test_groups_of_every_shape_and_edge_points(hsw, eng_int, mont):
    N = hsw._native
    T = N.HSW_OPEN_MIN_TILE_ROWS
    rows = 2 * T + 3
    rng = np.random.default_rng(2000)
    values = edge_values(rng, rows)                                           # heights rows, rows - 1, 1, 0, rows, rows - 1
    zr, vr = random_column(rng, 2), random_column(rng, 3)
    spec = [([0], zr[0], 0),                  # m = 1
            ([0, 1], 0, vr[0]),               # m = 2, z = 0: q[j] = c[j+1]
            ([0, 1, 2, 3, 4], 1, vr[1]),      # m = 5, the longest column first (and last), heights rows, rows - 1, 1, 0, rows
            ([3, 2, 1, 0], zr[1], vr[2]),     # the longest column last
            ([0, 2, 3], P_INT - 1, 1),        # the longest first; v = 1: the plain sum
            ([1, 4], zr[0], 0),               # the point of group 0 again; v = 0: the last column alone
            ([5], P_INT - 1, vr[0]),
            ([3], zr[1], vr[0]),              # input_rows 0: a zero quotient
            ([4, 4, 0], 1, P_INT - 1)]        # a column twice in one group
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values, n_quotients=len(spec))
    groups, points, challenges = [s[0] for s in spec], [s[1] for s in spec], [s[2] for s in spec]
    out, evals, _, _ = case.open(groups, points, challenges, tile_rows=T)
    assert not out[7].any() and not evals[7].any()
    out0, evals0, _, _ = case.open(groups, points, challenges)                # the library's own tile
    assert all(np.array_equal(a, b) for a, b in zip(out, out0)) and np.array_equal(evals, evals0)
    cfg.close()


# ---- 3. evaluate ----------------------------------------------------------------------------------------------------------------
@REPR
def test_evaluate_many_points_duplicates_and_a_column_without_a_query(hsw, eng_int, mont):
    N = hsw._native
    T = N.HSW_OPEN_MIN_TILE_ROWS
    rows = 3 * T + 1
    rng = np.random.default_rng(3000)
    values = edge_values(rng, rows)
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values, n_quotients=3)
    case.poke(4, 0, P_INT)                                                    # column 4 has no query: it is not read, hence not refused
    points = [random_column(rng, 1)[0], 0, 1, P_INT - 1, random_column(rng, 1)[0]]
    queries = [(0, 0), (0, 4), (0, 1), (0, 2), (0, 3), (1, 0), (0, 0), (2, 4), (3, 2), (5, 3), (1, 0), (5, 0), (0, 4)]
    for tile_rows in (T, 0):
        ev, status, rep = case.evaluate(points, queries, tile_rows=tile_rows)
        assert ev[0].tolist() == ev[6].tolist() and ev[5].tolist() == ev[10].tolist() and not ev[8].any()
        assert rep.scratch_bytes == 10 * rep.tiles * 32                       # ten distinct (column, point) pairs
    _, evals, _, _ = case.open([[0], [1], [5]], [points[4], points[0], points[3]], [7, 7, 7], tile_rows=T)
    assert evals[0].tolist() == ev[1].tolist() and evals[1].tolist() == ev[5].tolist() and evals[2].tolist() == ev[9].tolist()
    cfg.close()


# ---- 4. refusals decided on the device ------------------------------------------------------------------------------------------
@REPR
@pytest.mark.parametrize("where", ["first", "last", "unread"])
def test_a_cell_not_below_p_refuses_its_groups_and_queries_alone(hsw, eng_int, mont, where):
    N = hsw._native
    T = N.HSW_OPEN_MIN_TILE_ROWS
    rows = 2 * T + 3
    rng = np.random.default_rng(4000)
    values = [random_column(rng, h) for h in (rows, rows - 5, rows, rows - 5)]
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values, n_quotients=4)
    case.poke(1, {"first": 0, "last": rows - 6, "unread": rows - 5}[where], P_INT)     # p itself: the least encoding not below p
    case.poke(3, rows - 5, P_INT + 1)                                         # always at input_rows: never read
    groups, points, challenges = [[0], [0, 1, 2], [2, 3], [1]], random_column(rng, 4), random_column(rng, 4)
    bad_groups, bad_cols = ([], []) if where == "unread" else ([1, 3], [1])
    for tile_rows in (T, 0):
        out, _, _, _ = case.open(groups, points, challenges, tile_rows=tile_rows, refused=bad_groups)
        assert out[0] is not None and out[2] is not None
        case.evaluate(points, [(1, 0), (0, 1), (1, 2), (3, 3), (2, 0)], tile_rows=tile_rows, refused=bad_cols)
    cfg.close()


# ---- 4b. batches: the engine option "round_scratch" lowers the 1 GiB a batch's scratch may take ------------------------------
@REPR
def test_evaluate_in_batches_of_columns_under_a_scratch_budget(hsw, eng_int, mont):
    """773 rows in tiles of 256: 4 tiles, 128 bytes of scratch an item.  Five columns of 1, 3, 0, 2 and 1 items (a
    duplicate query besides), the queries listed in an order that interleaves the columns; a batch's items lie from 0 in
    the scratch whatever their place in the call."""
    T = hsw._native.HSW_OPEN_MIN_TILE_ROWS
    assert T == 256
    rows = 3 * T + 5
    rng = np.random.default_rng(4500)
    values = [random_column(rng, h) for h in (rows, rows - 1, rows, 1, rows)]
    points = random_column(rng, 3) + [P_INT - 1]
    queries = [(1, 0), (0, 1), (3, 2), (1, 3), (4, 0), (3, 0), (1, 1), (1, 0)]
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values)
    case.poke(2, 0, P_INT)                                                    # column 2 has no query: not read, not refused
    whole, _, rep = case.evaluate(points, queries, tile_rows=T)
    assert rep.scratch_bytes == 7 * 128
    try:
        # four items: columns {0, 1} and {3, 4}; a byte short: {0}, {1}, {3, 4}; 1: every column alone, the three items of column 1 together
        for budget, batches, held in ((4 * 128, 2, 4), (4 * 128 - 1, 3, 3), (1, 4, 3)):
            eng_int.set_option("round_scratch", budget)
            ev, _, rep = case.evaluate(points, queries, tile_rows=T, batches=batches)
            assert np.array_equal(ev, whole) and rep.scratch_bytes == held * 128
        case.poke(4, rows - 1, P_INT)                                         # a column of the last batch: its one query alone is refused
        for budget, batches in ((4 * 128, 2), (1, 4)):
            eng_int.set_option("round_scratch", budget)
            ev, status, rep = case.evaluate(points, queries, tile_rows=T, refused=(4,), batches=batches)
            assert status.tolist() == [0, 0, 0, 0, 4] and rep.refused_queries == 1
            assert np.array_equal(np.delete(ev, 4, 0), np.delete(whole, 4, 0))
    finally:
        eng_int.set_option("round_scratch", 1 << 30)
    cfg.close()


FOLDED, SINGLE = 128 + 3328 + 24832, 128 + 3328   # 773 rows, 4 tiles: the tiles' sums, a cell per thread (97, to 256 bytes), c (to 256 bytes)


@REPR
@pytest.mark.parametrize("first", ["folded_first", "single_first"])
def test_open_in_batches_of_groups_under_a_scratch_budget(hsw, eng_int, mont, first):
    """773 rows in tiles of 256.  Six groups, folded ones (2, 3, 2 columns) and single columns in turn.  A batch's scratch
    is all its tiles' sums first, then per group its seeds and, if it is folded, c: a batch of a folded and a single
    group runs tiles, seeds, c, seeds; one of a single and a folded group tiles, seeds, seeds, c."""
    T = hsw._native.HSW_OPEN_MIN_TILE_ROWS
    assert T == 256
    rows = 3 * T + 5
    rng = np.random.default_rng(4600)
    values = [random_column(rng, h) for h in (rows, rows - 5, rows, 1, rows - 1, rows)]
    groups = [[0, 1], [2], [1, 3, 0], [4], [4, 0], [5]]
    if first == "single_first":
        groups = groups[1:] + groups[:1]                                      # ... and [0, 1] last
    points, challenges = random_column(rng, 6), random_column(rng, 6)
    expect = [open_model([values[b] for b in grp], z, v, rows) for grp, z, v in zip(groups, points, challenges)]
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values, n_quotients=6)
    whole, whole_evals, _, rep = case.open(groups, points, challenges, tile_rows=T, expect=expect)
    assert rep.scratch_bytes == 3 * FOLDED + 3 * SINGLE == 95232
    last = 5 if first == "folded_first" else 4                                # the group that is column 5 alone
    try:
        # a folded and a single group together: three batches of two; a byte short: every group alone; 1: the same
        for budget, batches, held in ((FOLDED + SINGLE, 3, 31744), (FOLDED + SINGLE - 1, 6, 28416), (1, 6, 28416)):
            eng_int.set_option("round_scratch", budget)
            out, evals, _, rep = case.open(groups, points, challenges, tile_rows=T, expect=expect, batches=batches)
            assert rep.scratch_bytes == held and np.array_equal(evals, whole_evals)
            assert all(np.array_equal(a, b) for a, b in zip(out, whole))
        case.poke(5, 300, P_INT)                                              # column 5: one group of the last batch is refused
        for budget, batches in ((FOLDED + SINGLE, 3), (1, 6)):
            eng_int.set_option("round_scratch", budget)
            out, evals, status, rep = case.open(groups, points, challenges, tile_rows=T, expect=expect, refused=(last,), batches=batches)
            assert [int(s) for s in status] == [4 if k == last else 0 for k in range(6)] and out[last] is None
            assert all(np.array_equal(out[k], whole[k]) for k in range(6) if k != last)
    finally:
        eng_int.set_option("round_scratch", 1 << 30)
    cfg.close()


# ---- 4c. the other limit of a batch: 65,535 columns or groups in a grid dimension ------------------------------------------------
def eight_cells(mont, seed):
    """eight one-row columns side by side with sentinels around them: (device buffer, its host image, the eight stored cells)"""
    import torch
    rng = np.random.default_rng(seed)
    cells = np.array(limbs([stored(x, mont) for x in random_column(rng, 8)]))
    host = np.full((8 + 2 * PAD, 4), np.uint64(SENT), dtype=np.uint64)
    host[PAD: PAD + 8] = cells
    buf = torch.from_numpy(host.view(np.int64)).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, host, cells


@REPR
def test_evaluate_more_columns_than_a_grid_dimension_holds(hsw, eng_int, mont):
    """65,537 columns of one row, a query each: batches of 65,535 and 2.  The columns are eight cells read over and
    over; the evaluation of a one-row column is its cell, at any point."""
    N, n = hsw._native, 65537
    cfg = gadget(hsw, eng_int, mont)
    buf, host, cells = eight_cells(mont, 4700)
    z = np.array(limbs([stored(x, mont) for x in random_column(np.random.default_rng(4701), 2)]))
    cols = (C.c_void_p * n)(*[buf.data_ptr() + 32 * (PAD + b % 8) for b in range(n)])
    evals = np.full((n + 2, 4), np.uint64(EVAL_FILL), dtype=np.uint64)         # a row before and a row behind: untouched
    status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    qc = np.arange(n, dtype=np.uint32)
    qp = (qc & 1).astype(np.uint32)
    args = N.Evaluate(0, 0, 1, n, cols, None, 2, z.ctypes.data, n, qc.ctypes.data_as(C.POINTER(C.c_uint32)), qp.ctypes.data_as(C.POINTER(C.c_uint32)),
                      evals[1:].ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
    rep = N.EvaluateReport()
    rc = N.lib().hsw_gadget_evaluate(cfg.h, C.byref(args), C.byref(rep))
    assert rc == N.HSW_OK, rc
    print("evaluate: rows 1, columns %d (batches of 65535 and 2), launches %d, kernel %.3f ms, scratch %d bytes, refused %d"
          % (rep.columns, rep.launches, rep.kernel_ms, rep.scratch_bytes, rep.refused_columns))
    assert (rep.columns, rep.queries, rep.refused_columns, rep.refused_queries, rep.launches, rep.tiles) == (n, n, 0, 0, 4, 1)
    assert rep.scratch_bytes == 65535 * 32 and not status.any()
    assert (evals[0] == np.uint64(EVAL_FILL)).all() and (evals[n + 1] == np.uint64(EVAL_FILL)).all()
    assert np.array_equal(evals[n - 1: n + 1], cells[[(n - 2) % 8, (n - 1) % 8]])   # the second batch's
    assert np.array_equal(evals[1: n + 1], np.tile(cells, (n // 8 + 1, 1))[:n])
    assert np.array_equal(buf.cpu().numpy().view(np.uint64), host)
    cfg.close()


@REPR
def test_open_more_groups_than_a_grid_dimension_holds(hsw, eng_int, mont):
    """65,537 groups of one column of one row: batches of 65,535 and 2.  Every quotient is one zero cell at an address of
    its own, every evaluation the column's cell."""
    import torch
    N, ng = hsw._native, 65537
    cfg = gadget(hsw, eng_int, mont)
    buf, host, cells = eight_cells(mont, 4800)
    quot = torch.from_numpy(np.full((ng + 2 * PAD, 4), np.uint64(SENT), dtype=np.uint64).view(np.int64)).cuda()
    assert quot.data_ptr() % 16 == 0
    zv = np.array(limbs([stored(x, mont) for x in random_column(np.random.default_rng(4801), 2)]))
    z, v = np.tile(zv[0], (ng, 1)), np.tile(zv[1], (ng, 1))
    cols = (C.c_void_p * 8)(*[buf.data_ptr() + 32 * (PAD + b) for b in range(8)])
    qs = (C.c_void_p * ng)(*[quot.data_ptr() + 32 * (PAD + k) for k in range(ng)])
    first = np.arange(ng + 1, dtype=np.uint64)
    flat = (np.arange(ng, dtype=np.uint32) % 8).astype(np.uint32)
    evals = np.full((ng + 2, 4), np.uint64(EVAL_FILL), dtype=np.uint64)        # a row before and a row behind: untouched
    status = np.full(ng, 0xFFFFFFFF, dtype=np.uint32)
    args = N.Open(0, 0, 1, 8, cols, None, ng, first.ctypes.data_as(C.POINTER(C.c_uint64)), flat.ctypes.data_as(C.POINTER(C.c_uint32)), z.ctypes.data,
                  v.ctypes.data, qs, evals[1:].ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
    rep = N.OpenReport()
    torch.cuda.synchronize()
    rc = N.lib().hsw_gadget_open(cfg.h, C.byref(args), C.byref(rep))
    assert rc == N.HSW_OK, rc
    print("open: rows 1, groups %d, batches %d, launches %d, kernel %.3f ms, scratch %d bytes, refused %d"
          % (rep.groups, rep.batches, rep.launches, rep.kernel_ms, rep.scratch_bytes, rep.refused_groups))
    assert (rep.groups, rep.refused_groups, rep.written, rep.batches, rep.launches, rep.tiles) == (ng, 0, ng, 2, 6, 1)
    assert rep.scratch_bytes == 18874112 and not status.any()                 # 65,535 x (a tile's sum, and one seed to 256 bytes), to 256 bytes
    got = quot.cpu().numpy().view(np.uint64)
    assert (got[:PAD] == np.uint64(SENT)).all() and (got[PAD + ng:] == np.uint64(SENT)).all()
    assert not got[PAD + ng - 2: PAD + ng].any() and not got[PAD: PAD + ng].any()   # the second batch's two, then all: q = 0
    assert (evals[0] == np.uint64(EVAL_FILL)).all() and (evals[ng + 1] == np.uint64(EVAL_FILL)).all()
    assert np.array_equal(evals[ng - 1: ng + 1], cells[[(ng - 2) % 8, (ng - 1) % 8]])
    assert np.array_equal(evals[1: ng + 1], np.tile(cells, (ng // 8 + 1, 1))[:ng])
    assert np.array_equal(buf.cpu().numpy().view(np.uint64), host)
    cfg.close()


# ---- 5. the wrapper, and the whole path: lagrange_to_coeff, open, commit ----------------------------------------------------------
@REPR
def test_ntt_then_open_then_msm_of_the_quotient(hsw, eng_int, mont):
    import random

    import torch
    N = hsw._native
    log_n, n = 8, 256
    rng = np.random.default_rng(5000)
    lagrange = [random_column(rng, n), random_column(rng, n)]
    omega = root_of_unity(log_n)
    w_inv, n_inv = pow(omega, -1, P_INT), pow(n, -1, P_INT)
    coeff_model = [ntt_model(a, log_n, w_inv, scale=n_inv) for a in lagrange]
    prng = random.Random(5001)
    pts, logs = chain(prng.randrange(1, P_INT), prng.randrange(1, P_INT), n)
    cfg = gadget(hsw, eng_int, mont)
    enc = lambda xs: np.array(limbs([stored(x, mont) for x in xs]))           # noqa: E731
    cols = torch.from_numpy(np.stack([enc(a) for a in lagrange]).view(np.int64)).cuda().view(torch.uint64)
    bases = torch.from_numpy(np.array([point_words(p) for p in pts], dtype=np.uint64).view(np.int64)).cuda().view(torch.uint64)
    coeff, st, _ = cfg.ntt(log_n, enc([w_inv])[0], cols, scale=enc([n_inv])[0])
    assert not st.any()
    x = random_column(rng, 1)[0]
    z = [x, x * omega % P_INT]
    v = random_column(rng, 2)
    evals, st, rep = cfg.evaluate(n, coeff, [int(stored(t, mont)) for t in z], [(0, 0), (1, 0), (0, 1)])
    assert not st.any() and rep["queries"] == 3
    assert evals.tolist() == enc([evaluate_model(coeff_model[0], z[0]), evaluate_model(coeff_model[1], z[0]), evaluate_model(coeff_model[0], z[1])]).tolist()
    quotients, oevals, st, rep = cfg.open(n, coeff, [[0, 1], [0]], [int(stored(t, mont)) for t in z], [int(stored(t, mont)) for t in v])
    assert not st.any() and rep["launches"] == 3 and quotients.shape == (2, n, 4)
    want = [open_model(coeff_model, z[0], v[0], n), open_model(coeff_model[:1], z[1], v[1], n)]
    assert quotients.view(torch.int64).cpu().numpy().view(np.uint64).tolist() == [enc(q).tolist() for q, _ in want] and oevals.tolist() == enc([e for _, e in want]).tolist()
    points, st, _ = cfg.msm(bases, quotients)                                 # n_bases = rows: the quotient as it lies
    assert not st.any()
    assert points.tolist() == [point_words(commitment(q, logs)) for q, _ in want]
    cfg.close()
