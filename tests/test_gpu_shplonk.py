"""hsw_gadget_shplonk_quotient and hsw_gadget_shplonk_open on the MI355X: SHPLONK's multi-point opening of device
columns, by the kernels of hsw_shplonk.hip around the scan of hsw_open.hip.

The yardstick is Python integers: tests/shplonk_model.py -- the quotient by SUCCESSIVE Kate division, not the partial
fractions the device runs -- proven in tests/test_shplonk_host.py.  Every cell of h and of w is compared with it,
exactly, in both cell forms.  The columns, h and the output are carved out of one buffer with sentinel cells around
each; after a call every byte of it outside rows [0, rows) of the output must be what it was.  Rows of a column at and
beyond its input_rows hold limbs far above p: a read of them shows as a refusal or as a wrong value.  The status word
is pre-filled."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.msm_model import G, R_INT, add, commitment, mul, neg, point_words, words_point
from tests.ntt_model import ntt_model, root_of_unity
from tests.open_model import evaluate_model, open_model
from tests.shplonk_model import interpolate_eval, shplonk_open_model, shplonk_quotient_model, vanish, zd_of
from tests.test_gpu_bound_region import REPR
from tests.test_gpu_lookup_permuted import SENT, limbs, stored
from tests.test_gpu_open import GARBAGE, PAD, eng_int, gadget, random_column  # noqa: F401 (eng_int: a fixture)

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 3), (3, 2), (5, 4), (2, 16)]       # (m, t) of the rotation sets


def sets_of(shapes):
    """the sets of the given (m, t): consecutive columns; set i takes the points i, i + 1, .. (mod 16) of a T of 16,
    re-indexed to the points that are used"""
    sets, col, remap = [], 0, {}
    for i, (m, t) in enumerate(shapes):
        pts = [remap.setdefault((i + k) % 16, len(remap)) for k in range(t)]
        sets.append((list(range(col, col + m)), pts))
        col += m
    return sets, col, len(remap)


def heights_for(rows, n):
    return [[rows, rows - 1, min(1, rows), 0, rows][b % 5] for b in range(n)]


class Case:
    """Columns of `rows` cells (values[b]: the input_rows[b] values of column b), a slot for h and one for the output."""

    def __init__(self, cfg, hsw, rows, mont, values):
        import torch
        self.cfg, self.N, self.rows, self.mont, self.values = cfg, hsw._native, rows, mont, [list(v) for v in values]
        self.n, self.heights = len(values), [len(v) for v in values]
        self.col_at, at = [], 0
        for _ in range(self.n + 2):
            self.col_at.append(at + PAD)
            at += 2 * PAD + rows
        self.h_at, self.out_at = self.col_at[self.n], self.col_at[self.n + 1]
        host = np.full((at, 4), np.uint64(SENT), dtype=np.uint64)
        for b, vals in enumerate(self.values):
            s = self.col_at[b]
            host[s: s + rows] = np.uint64(GARBAGE)
            if vals:
                host[s: s + len(vals)] = limbs([stored(x, mont) for x in vals])
        self.buf = torch.from_numpy(host.view(np.int64)).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 16 == 0

    def put(self, at, cells):
        """store encoded cells (an (k, 4) uint64 array) from buffer row `at` on"""
        import torch
        self.buf[at: at + len(cells)] = torch.from_numpy(np.ascontiguousarray(cells).view(np.int64)).cuda()
        torch.cuda.synchronize()

    def enc(self, xs):
        return np.array(limbs([stored(x, self.mont) for x in xs]))            # (a writable copy)

    def call(self, which, sets, points, y, v, u=None, h=None, tile_rows=0, refused=False, expect=None):
        """one call and every check; returns (the output cells or None, report).  h: the values of h (open)"""
        import torch
        N, n, rows = self.N, self.n, self.rows
        if which == "open":
            self.put(self.h_at, self.enc(h) if not isinstance(h, np.ndarray) else h)
        cols = (C.c_void_p * n)(*[self.base + 32 * a for a in self.col_at[:n]])
        hs = (C.c_uint64 * n)(*self.heights) if self.heights != [rows] * n else None
        torch.cuda.synchronize()
        before = self.buf.cpu().numpy().view(np.uint64).copy()
        first, pfirst = [0], [0]
        for cs, ps in sets:
            first.append(first[-1] + len(cs))
            pfirst.append(pfirst[-1] + len(ps))
        flat_c, flat_p = [b for cs, _ in sets for b in cs], [t for _, ps in sets for t in ps]
        z, ch = self.enc(points), self.enc([y, v, u or 0])
        status = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
        ns = len(sets)
        args = N.Shplonk(0, tile_rows, rows, n, cols, hs, len(points), z.ctypes.data, ns, (C.c_uint64 * (ns + 1))(*first),
                         (C.c_uint32 * len(flat_c))(*flat_c), (C.c_uint64 * (ns + 1))(*pfirst), (C.c_uint32 * len(flat_p))(*flat_p),
                         ch[0].ctypes.data, ch[1].ctypes.data, ch[2].ctypes.data if which == "open" else None,
                         self.base + 32 * self.h_at if which == "open" else None, self.base + 32 * self.out_at,
                         status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.ShplonkReport()
        fn = N.lib().hsw_gadget_shplonk_open if which == "open" else N.lib().hsw_gadget_shplonk_quotient
        rc = fn(self.cfg.h, C.byref(args), C.byref(rep))
        assert rc == N.HSW_OK, rc
        after = self.buf.cpu().numpy().view(np.uint64)
        assert status[0] == (N.HSW_SHPLONK_CELL_NOT_BELOW_P if refused else 0)
        assert (rep.sets, rep.items, rep.refused, rep.written) == (ns, len(flat_p), int(refused), 0 if refused else rows)
        assert rep.columns == len(flat_c) + (which == "open") and rep.launches == 3 and rep.thread_rows == N.HSW_OPEN_THREAD_ROWS
        assert rep.tile_rows == (tile_rows or 2048) and rep.tiles == -(-rows // rep.tile_rows) and rep.scratch_bytes > 0
        if refused:
            assert np.array_equal(after, before), "a refused call wrote device memory of the caller"
            return None, rep
        mask = np.ones(len(before), dtype=bool)
        mask[self.out_at: self.out_at + rows] = False
        assert np.array_equal(after[mask], before[mask]), "something outside the output was written"
        cells = after[self.out_at: self.out_at + rows].copy()
        if expect is None:
            cols_v = self.values
            expect = (shplonk_open_model(cols_v, sets, points, y, v, u, h, rows) if which == "open"
                      else shplonk_quotient_model(cols_v, sets, points, y, v, rows))
        want = self.enc(expect)
        if not np.array_equal(cells, want):
            bad = int(np.nonzero((cells != want).any(axis=1))[0][0])
            raise AssertionError("%s: output row %d differs" % (which, bad))
        assert not cells[rows - 1].any()                                      # the top cell is 0: n_bases = rows commits it as it lies
        return cells, rep

    def both(self, sets, points, y, v, u, tile_rows=0, expect=None):
        """the quotient, then the open fed with the DEVICE's h; expect: (h, w) if the caller has them already"""
        h_cells, _ = self.call("quotient", sets, points, y, v, tile_rows=tile_rows, expect=expect and expect[0])
        h = expect[0] if expect else shplonk_quotient_model(self.values, sets, points, y, v, self.rows)
        w_cells, rep = self.call("open", sets, points, y, v, u=u, h=h_cells, tile_rows=tile_rows,
                                 expect=expect[1] if expect else shplonk_open_model(self.values, sets, points, y, v, u, h, self.rows))
        return h_cells, w_cells, rep


def problem(seed, rows, shapes):
    """(values, sets, points, y, v, u): columns of heights rows, rows - 1, 1, 0, rows, ..; a point equal to 0"""
    rng = np.random.default_rng(seed)
    sets, n, n_points = sets_of(shapes)
    values = [random_column(rng, h) for h in heights_for(rows, n)]
    values[0][0] = P_INT - 1
    points = random_column(rng, n_points)
    points[min(1, n_points - 1)] = 0                                          # a point equal to 0
    y, v, u = random_column(rng, 3)
    return values, sets, points, y, v, u


@functools.lru_cache(maxsize=None)
def reference(seed, rows, shapes):
    """the problem and its (h, w), computed once and shared by both cell forms"""
    values, sets, points, y, v, u = problem(seed, rows, shapes)
    h = shplonk_quotient_model(values, sets, points, y, v, rows)
    return values, sets, points, y, v, u, h, shplonk_open_model(values, sets, points, y, v, u, h, rows)


# ---- 1. rows at every boundary of a thread, a workgroup and a tile; all five shapes of set in one call ---------------------
@REPR
@pytest.mark.parametrize("rows", [1, 2, 7, 8, 9, 255, 257, 2053])
def test_rows_at_every_boundary_default_tile(hsw, eng_int, mont, rows):  # noqa: F811
    values, sets, points, y, v, u, h, w = reference(100 + rows, rows, tuple(SHAPES))
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values)
    _, _, rep = case.both(sets, points, y, v, u, expect=(h, w))
    assert rep.tiles == -(-rows // 2048)
    cfg.close()


# ---- 2. several tiles; two sweeps per tile, the carry through scratch -------------------------------------------------------
@REPR
@pytest.mark.parametrize("tile_rows,rows", [(256, 3 * 256 + 5), (4096, 4096 + 9)])
def test_several_tiles_and_two_sweeps(hsw, eng_int, mont, tile_rows, rows):  # noqa: F811
    values, sets, points, y, v, u, h, w = reference(200 + tile_rows, rows, tuple(SHAPES))
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values)
    _, _, rep = case.both(sets, points, y, v, u, tile_rows=tile_rows, expect=(h, w))
    assert rep.tiles == -(-rows // tile_rows) and rep.tiles >= 2
    cfg.close()


@REPR
def test_more_tiles_than_the_scan_has_threads(hsw, eng_int, mont):  # noqa: F811
    rows = 256 * 257 + 3
    values, sets, points, y, v, u, h, w = reference(300, rows, ((1, 3),))
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values)
    _, _, rep = case.both(sets, points, y, v, u, tile_rows=256, expect=(h, w))
    assert rep.tiles == 258 and rep.items == 3
    cfg.close()


# ---- 3. every shape of set alone, and y, v among 0, 1 and random ----------------------------------------------------------
@REPR
@pytest.mark.parametrize("which", range(6))
def test_each_shape_alone_and_edge_challenges(hsw, eng_int, mont, which):  # noqa: F811
    rows = 257
    shapes = tuple(SHAPES) if which == 5 else (SHAPES[which],)
    values, sets, points, y, v, u = problem(400 + which, rows, shapes)
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values)
    for yy, vv in ((y, v), (0, v), (1, 0), (y, 1), (0, 0), (1, 1)) if which >= 3 else ((y, v), (0, 1), (1, 0)):
        case.both(sets, points, yy, vv, u, tile_rows=256)
    cfg.close()


# ---- 4. a cell not below p: decided on the device, nothing written -------------------------------------------------------------
@REPR
@pytest.mark.parametrize("where", ["column", "h", "unread"])
def test_a_cell_not_below_p_refuses_the_call(hsw, eng_int, mont, where):  # noqa: F811
    rows = 2 * 256 + 3
    values, sets, points, y, v, u, h, w = reference(500, rows, ((1, 1), (3, 2), (1, 3)))
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values)
    p_cell = np.array(limbs([P_INT]))                                         # p itself: the least encoding not below p
    if where == "column":                                                      # column 2 (height 1) sits in the second set
        case.put(case.col_at[2], p_cell)
        for tile_rows in (256, 0):
            case.call("quotient", sets, points, y, v, tile_rows=tile_rows, refused=True)
            case.call("open", sets, points, y, v, u=u, h=h, tile_rows=tile_rows, refused=True)
    elif where == "h":
        bad = case.enc(h)
        bad[rows - 2] = p_cell[0]
        for tile_rows in (256, 0):
            case.call("open", sets, points, y, v, u=u, h=bad, tile_rows=tile_rows, refused=True)
        case.call("quotient", sets, points, y, v, expect=h)                   # the first call does not read h
    else:                                                                      # at input_rows of column 2: never read
        case.put(case.col_at[2] + 1, p_cell)
        case.both(sets, points, y, v, u, tile_rows=256, expect=(h, w))
    cfg.close()


# ---- 5. a single set with one point is the GWC quotient of the reversed list with challenge y --------------------------------
@REPR
def test_one_set_one_point_is_hsw_gadget_open_of_the_reversed_list(hsw, eng_int, mont):  # noqa: F811
    import torch
    rows = 2 * 256 + 3
    values, sets, points, y, v, u = problem(600, rows, ((4, 1),))
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, rows, mont, values)
    want, _ = open_model([values[b] for b in reversed(sets[0][0])], points[0], y, rows)
    cells, _ = case.call("quotient", sets, points, y, v, tile_rows=256, expect=want)
    enc1 = lambda x: [int(t) for t in case.enc([x])[0]]                       # noqa: E731
    addr = [case.base + 32 * a for a in case.col_at[:case.n]]
    q = torch.zeros((1, rows, 4), dtype=torch.uint64, device="cuda")
    _, _, st, _ = cfg.open(rows, addr, [list(reversed(sets[0][0]))], np.array([enc1(points[0])], dtype=np.uint64),
                           np.array([enc1(y)], dtype=np.uint64), out=q, input_rows=case.heights, tile_rows=256)
    assert not st.any()
    assert np.array_equal(q[0].view(torch.int64).cpu().numpy().view(np.uint64), cells)
    cfg.close()


# ---- 6. the whole path: ntt, evaluate, both calls, msm -- and the verifier's equation in G1 ------------------------------------
@REPR
def test_chain_ntt_evaluate_shplonk_msm_and_the_verifier_equation(hsw, eng_int, mont):  # noqa: F811
    import random

    import torch
    log_n, n = 6, 64
    rng = np.random.default_rng(7000)
    lagrange = [random_column(rng, n) for _ in range(4)]
    omega = root_of_unity(log_n)
    w_inv, n_inv = pow(omega, -1, P_INT), pow(n, -1, P_INT)
    coeff_model = [ntt_model(a, log_n, w_inv, scale=n_inv) for a in lagrange]
    prng = random.Random(7001)
    s = prng.randrange(1, P_INT)                                              # the test's own trapdoor: bases s^j G
    logs = [pow(s, j, R_INT) for j in range(n)]
    pts = [mul(k, G) for k in logs]
    cfg = gadget(hsw, eng_int, mont)
    enc = lambda xs: np.array(limbs([stored(x, mont) for x in xs]))           # noqa: E731
    one = lambda x: [int(t) for t in enc([x])[0]]                             # noqa: E731
    cols = torch.from_numpy(np.stack([enc(a) for a in lagrange]).view(np.int64)).cuda().view(torch.uint64)
    bases = torch.from_numpy(np.array([point_words(p) for p in pts], dtype=np.uint64).view(np.int64)).cuda().view(torch.uint64)
    coeff, st, _ = cfg.ntt(log_n, enc([w_inv])[0], cols, scale=enc([n_inv])[0])
    assert not st.any()
    x = random_column(rng, 1)[0]
    T = [x, x * omega % P_INT, x * w_inv % P_INT]                             # {x, x omega, x omega^-1}
    sets = [([0, 1], [0]), ([2], [0, 1]), ([3], [0, 1, 2])]
    y, v, u = random_column(rng, 3)
    queries = [(b, t) for cs, ps in sets for b in cs for t in ps]
    evals, st, _ = cfg.evaluate(n, coeff, np.array([one(t) for t in T], dtype=np.uint64), queries)
    assert not st.any()
    dec = lambda row: (sum(int(row[i]) << (64 * i) for i in range(4)) * (pow(1 << 256, -1, P_INT) if mont else 1)) % P_INT   # noqa: E731
    ev = {q: dec(evals[i]) for i, q in enumerate(queries)}
    assert all(ev[(b, t)] == evaluate_model(coeff_model[b], T[t]) for b, t in queries)
    zs, ye, ve, ue = (np.array([one(t) for t in xs], dtype=np.uint64) for xs in (T, [y], [v], [u]))
    h, status, rep = cfg.shplonk_quotient(n, coeff, sets, zs, ye, ve)
    assert status == 0 and rep["launches"] == 3 and h.shape == (n, 4)
    w, status, rep = cfg.shplonk_open(n, coeff, sets, zs, ye, ve, ue, h)
    assert status == 0 and rep["launches"] == 3 and rep["columns"] == 5
    h_model = shplonk_quotient_model(coeff_model, sets, T, y, v, n)
    assert h.view(torch.int64).cpu().numpy().view(np.uint64).tolist() == enc(h_model).tolist()
    assert w.view(torch.int64).cpu().numpy().view(np.uint64).tolist() == enc(shplonk_open_model(coeff_model, sets, T, y, v, u, h_model, n)).tolist()
    commits, st, _ = cfg.msm(bases, torch.cat([t.view(torch.int64) for t in (coeff, h.unsqueeze(0), w.unsqueeze(0))]).view(torch.uint64))   # the four columns, H and W
    assert not st.any()
    Cs = [words_point(r) for r in commits]
    H, W = Cs[4], Cs[5]
    assert H == commitment(h_model, logs)
    # the verifier: sum_i v^i (zd_i / zd_0) (sum_k y^k C_{i,k} - R_i(u) G) - (zt / zd_0) H == (s - u) W, with R_i
    # interpolated from the DEVICE's evaluations
    zd, zt = zd_of(sets, T, u), vanish(u, T)
    inv0 = pow(zd[0], -1, P_INT)
    lhs = None
    for i, (cs, ps) in enumerate(sets):
        acc = None
        for k, b in enumerate(cs):
            acc = add(acc, mul(pow(y, k, P_INT), Cs[b]))
        folded = [sum(pow(y, k, P_INT) * ev[(b, t)] for k, b in enumerate(cs)) % P_INT for t in ps]
        r_u = interpolate_eval([T[t] for t in ps], folded, u)
        acc = add(acc, neg(mul(r_u, G)))
        lhs = add(lhs, mul(pow(v, i, P_INT) * zd[i] * inv0, acc))
    lhs = add(lhs, neg(mul(zt * inv0, H)))
    assert lhs == mul(s - u, W)
    cfg.close()
