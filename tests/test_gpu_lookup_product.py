"""hsw_gadget_lookup_product on the MI355X: the grand-product column Z of halo2's lookup argument, written by the kernels
of hsw_lookup_product.hip.

The yardstick is Python integers.  A Z column is correct iff Z[0] encodes 1 and Z[i+1] den[i] = Z[i] num[i] (mod p) for
every i < u -- the argument's own constraint, which determines Z where no den is zero and needs no inversion --, with
  num[i] = (A[i] + beta)(S[i] + gamma),   den[i] = (A'[i] + beta)(S'[i] + gamma)
A[i] the compressed input (0 from input_rows on), S[i] = val(i) for i < T and val(0) on the padding rows, val the value
model of tests/test_gpu_lookup_permuted.py, and A', S' the cells the device holds.  Every row of every argument is
checked, exactly.  All columns -- inputs, A', S', Z -- are carved out of one buffer with sentinel cells around each;
after the call every byte of it outside rows [0, u] of the Z columns that were to be written must be what it was."""
import ctypes as C

import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.test_gpu_bound_column_tables import CarvedAll, geometry
from tests.test_gpu_bound_columns import interleaved
from tests.test_gpu_bound_region import REPR, make
from tests.test_gpu_lookup_counts import ORIGIN, spread_of
from tests.test_gpu_lookup_permuted import R_INT, SENT, limbs, stored, theta_of, value_table

pytestmark = pytest.mark.gpu
PAD = 3                                     # sentinel cells before and after every column
R_INV = pow(R_INT, -1, P_INT)
GARBAGE = (1 << 64) - 2                     # every limb of an input cell that must not be read: far above p, and not 0
T_SPREAD = 256
_TILE = {}


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


def ints(cells):
    """(n, 4) uint64 -> Python ints"""
    b = np.ascontiguousarray(cells, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i: i + 32], "little") for i in range(0, len(b), 32)]


def value(x, mont):
    """the field element a stored cell stands for (reduced: an encoding m + p stands for what m stands for)"""
    return x * R_INV % P_INT if mont else x % P_INT


def val(kind, t, theta):
    return t if kind == "range" else (t * theta + spread_of(t)) % P_INT if kind == "spread" else (t + spread_of(t) * theta) % P_INT


class Case:
    """One call's columns: per argument in, (sp,) pin, ptab of u cells and z of u + 1, carved in the slot order `order`."""

    def __init__(self, cfg, hsw, table, u, K, mont, seed, order="ascending", on_spread=False, input_rows=None):
        import torch
        N = hsw._native
        self.cfg, self.N, self.table, self.u, self.K, self.mont = cfg, N, table, u, K, mont
        self.spread_arg = table == N.HSW_LOOKUP_SPREAD
        self.T = T_SPREAD if self.spread_arg else 65536
        self.n_args = 2 * K if self.spread_arg else K
        self.kind = "range" if not self.spread_arg else "on_spread" if on_spread else "spread"
        self.on_spread = on_spread
        self.rows = list(input_rows) if input_rows is not None else [u] * self.n_args
        rng = np.random.default_rng(seed)
        self.theta = [theta_of(seed * 31 + 3 * c) if self.spread_arg else 0 for c in range(K)]
        self.beta = [theta_of(seed * 31 + 3 * c + 1) for c in range(K)]
        self.gamma = [theta_of(seed * 31 + 3 * c + 2) for c in range(K)]
        self.t_rows = [rng.integers(0, self.T, size=self.rows[a]) for a in range(self.n_args)]
        fams = ["in", "sp", "pin", "ptab", "z"] if self.spread_arg else ["in", "pin", "ptab", "z"]
        slots = [(f, a) for a in range(self.n_args) for f in fams]
        if order == "reversed":
            slots = slots[::-1]
        elif order == "interleaved":
            slots = slots[1::2] + slots[0::2]
        self.at, at = {}, 0
        for f, a in slots:
            self.at[(f, a)] = at + PAD
            at += 2 * PAD + u + (1 if f == "z" else 0)
        host = np.full((at, 4), np.uint64(SENT), dtype=np.uint64)
        dense_cells = value_table("range", self.T, 0, mont)
        spread_cells = limbs([stored(spread_of(t), mont) for t in range(T_SPREAD)])
        for a in range(self.n_args):
            for f, cells in (("in", dense_cells), ("sp", spread_cells)):
                if (f, a) in self.at:
                    s = self.at[(f, a)]
                    host[s: s + u] = np.uint64(GARBAGE)
                    host[s: s + self.rows[a]] = cells[self.t_rows[a]]
        self.buf = torch.from_numpy(host.view(np.int64)).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 16 == 0
        # A' and S' from the library itself, given m = bincount
        m = np.stack([np.bincount(t, minlength=self.T) for t in self.t_rows]).astype(np.uint32)
        d_m = torch.from_numpy(m.view(np.int32)).cuda()
        th = np.ascontiguousarray(limbs([stored(t, mont) for t in self.theta])) if self.spread_arg else None
        args = N.LookupPermuted(table, N.HSW_PERMUTED_GIVEN_M | (N.HSW_PERMUTED_THETA_ON_SPREAD if on_spread else 0), u, self.n_args,
                                self.ptrs("pin"), self.ptrs("ptab"), th.ctypes.data if th is not None else None, d_m.data_ptr(), self.T)
        rep = N.PermutedReport()
        torch.cuda.synchronize()
        cfg._ok(cfg.lib.hsw_gadget_lookup_permuted(cfg.h, C.byref(args), C.byref(rep)))
        assert rep.written == 2 * u * self.n_args

    def addr(self, fam, a, row=0):
        return self.base + 32 * (self.at[(fam, a)] + row)

    def ptrs(self, fam):
        return (C.c_void_p * self.n_args)(*[self.addr(fam, a) for a in range(self.n_args)])

    def poke(self, fam, a, row, x):
        """store the 256-bit integer x as the cell"""
        import torch
        self.buf[self.at[(fam, a)] + row] = torch.from_numpy(limbs([x]).copy().view(np.int64)[0]).cuda()
        torch.cuda.synchronize()

    def peek(self, fam, a, row):
        return ints(self.buf[self.at[(fam, a)] + row].cpu().numpy().view(np.uint64).reshape(1, 4))[0]

    def run(self, betas=None):
        """the call, then every check that holds for any outcome; returns (Z per argument or None, status, report)"""
        import torch
        N, u, mont = self.N, self.u, self.mont
        betas = betas if betas is not None else self.beta
        before = self.buf.cpu().numpy().view(np.uint64).copy()
        enc = lambda vs: np.ascontiguousarray(limbs([stored(v, mont) for v in vs]))      # noqa: E731
        th, be, ga = enc(self.theta), enc(betas), enc(self.gamma)
        status = np.full(self.n_args, 0xFFFFFFFF, dtype=np.uint32)
        rows = (C.c_uint64 * self.n_args)(*self.rows)
        args = N.LookupProduct(self.table, N.HSW_PERMUTED_THETA_ON_SPREAD if self.on_spread else 0, u, self.n_args, self.ptrs("in"),
                               self.ptrs("sp") if self.spread_arg else None, rows if self.rows != [u] * self.n_args else None,
                               self.ptrs("pin"), self.ptrs("ptab"), self.ptrs("z"), th.ctypes.data if self.spread_arg else None,
                               be.ctypes.data, ga.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.ProductReport()
        torch.cuda.synchronize()
        self.cfg._ok(self.cfg.lib.hsw_gadget_lookup_product(self.cfg.h, C.byref(args), C.byref(rep)))
        after = self.buf.cpu().numpy().view(np.uint64)
        report = {f[0]: getattr(rep, f[0]) for f in N.ProductReport._fields_}
        print("product: %d arguments, u %d, written %d, tiles %.3f ms, scan %.3f ms, write %.3f ms, status %s"
              % (self.n_args, u, report["written"], report["tiles_ms"], report["scan_ms"], report["write_ms"], status.tolist()))
        # the model: what each argument's status and Z must be
        changed = np.zeros(len(after), dtype=bool)
        zs, n_written, n_open, n_refused = [], 0, 0, 0
        for a in range(self.n_args):
            c = a // 2 if self.spread_arg else a
            s = lambda f: self.at[(f, a)]                                                # noqa: E731
            pin, ptab = ints(before[s("pin"): s("pin") + u]), ints(before[s("ptab"): s("ptab") + u])
            read = pin + ptab + ints(before[s("in"): s("in") + self.rows[a]])
            if self.spread_arg:
                read += ints(before[s("sp"): s("sp") + self.rows[a]])
            beta, gamma, theta = betas[c], self.gamma[c], self.theta[c]
            A = [val(self.kind, int(t), theta) for t in self.t_rows[a]] + [0] * (u - self.rows[a])
            table_vals = [val(self.kind, t, theta) for t in range(self.T)]
            num = [(A[i] + beta) * ((table_vals[i] if i < self.T else table_vals[0]) + gamma) % P_INT for i in range(u)]
            den = [(value(pin[i], mont) + beta) * (value(ptab[i], mont) + gamma) % P_INT for i in range(u)]
            want = 0
            if any(x >= P_INT for x in read):
                want |= N.HSW_PRODUCT_CELL_NOT_BELOW_P
            if 0 in den:
                want |= N.HSW_PRODUCT_ZERO_DENOM
            got = after[s("z"): s("z") + u + 1]
            if want:
                assert status[a] == want, (a, status[a], want)
                assert (got == np.uint64(SENT)).all(), "a refused argument was written"
                n_refused += 1
                zs.append(None)
                continue
            changed[s("z"): s("z") + u + 1] = True
            n_written += 1
            z = ints(got)
            assert all(x < P_INT for x in z), "a Z cell that is not below p"
            z = [value(x, mont) for x in z]
            assert z[0] == 1
            bad = [i for i in range(u) if z[i + 1] * den[i] % P_INT != z[i] * num[i] % P_INT]
            assert not bad, "argument %d: the recurrence fails at rows %s" % (a, bad[:5])
            is_open = z[u] != 1
            assert status[a] == (N.HSW_PRODUCT_OPEN if is_open else 0), (a, status[a])
            n_open += is_open
            zs.append(got.copy())
        assert np.array_equal(before[~changed], after[~changed]), "a cell outside rows [0, u] of a written Z column changed"
        assert report["arguments"] == self.n_args and report["written"] == (u + 1) * n_written
        assert report["open_arguments"] == n_open and report["refused_arguments"] == n_refused
        opened = [a for a in range(self.n_args) if zs[a] is not None and status[a] & N.HSW_PRODUCT_OPEN]
        refused = [a for a in range(self.n_args) if zs[a] is None]
        none = (1 << 64) - 1
        assert report["first_open"] == (opened[0] if opened else none) and report["first_refused"] == (refused[0] if refused else none)
        assert abs(report["kernel_ms"] - (report["tiles_ms"] + report["scan_ms"] + report["write_ms"])) < 1e-3
        return zs, status, report


def spread_cfg(hsw, eng, mont, K=3):
    return make(hsw, eng, "images", [64], K, ORIGIN, mont)                  # K proofs, nothing digested: the columns are synthetic


def tile_rows(hsw, eng):
    """report.tile_rows, from one small call"""
    if "r" not in _TILE:
        cfg = spread_cfg(hsw, eng, False)
        _, _, rep = Case(cfg, hsw, hsw._native.HSW_LOOKUP_SPREAD, 256, 3, False, 1).run()
        cfg.close()
        _TILE["r"] = int(rep["tile_rows"])
        assert 64 <= _TILE["r"] <= 1 << 16
    return _TILE["r"]


U_SPREAD = ["256", "257", "300", "r-1", "r", "r+1", "3r+7"]


# ---- 1. the spread argument closes: table-sized columns, the tile boundaries, both cell forms, three proofs -----------
@REPR
@pytest.mark.parametrize("which", range(len(U_SPREAD)), ids=U_SPREAD)
def test_spread_argument_closes(hsw, eng_int, which, mont):
    N = hsw._native
    r = tile_rows(hsw, eng_int)
    u = max(T_SPREAD, [256, 257, 300, r - 1, r, r + 1, 3 * r + 7][which])
    cfg = spread_cfg(hsw, eng_int, mont)
    case = Case(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, 3, mont, 100 + which, order=["ascending", "reversed", "interleaved"][which % 3],
                on_spread=bool(which % 2))
    zs, status, rep = case.run()
    assert rep["open_arguments"] == 0 and rep["refused_arguments"] == 0 and not status.any() and rep["written"] == 6 * (u + 1)
    one = limbs([stored(1, mont)])[0]
    assert all(np.array_equal(z[u], one) for z in zs)
    cfg.close()


# ---- 2. every address order with either theta order; input_rows below u with garbage beyond ---------------------------
@REPR
def test_address_orders_theta_orders_and_short_inputs(hsw, eng_int, mont):
    N = hsw._native
    cfg = spread_cfg(hsw, eng_int, mont)
    u = 300
    for n, (order, on_spread) in enumerate((o, t) for o in ("ascending", "reversed", "interleaved") for t in (False, True)):
        rows = [300, 0, 17, 299, 256, 1] if n % 2 == 0 else None
        case = Case(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, 3, mont, 200 + n, order=order, on_spread=on_spread, input_rows=rows)
        zs, status, rep = case.run()
        assert rep["open_arguments"] == 0 and rep["refused_arguments"] == 0 and rep["written"] == 6 * (u + 1), (order, on_spread)
        zs2, _, _ = case.run()                                                # again: the same bytes
        assert all(np.array_equal(x, y) for x, y in zip(zs, zs2))
    cfg.close()


# ---- 3. the range argument: 65,536 table rows, two proofs --------------------------------------------------------------
@REPR
@pytest.mark.parametrize("u", [65536, 65536 + 37])
def test_range_argument_closes(hsw, eng_int, u, mont):
    N = hsw._native
    cfg = make(hsw, eng_int, "images", [64], 2, ORIGIN, mont)
    case = Case(cfg, hsw, N.HSW_LOOKUP_RANGE, u, 2, mont, u, order="reversed", input_rows=[u, u - 4321])
    zs, status, rep = case.run()
    assert rep["open_arguments"] == 0 and rep["refused_arguments"] == 0 and not status.any() and rep["written"] == 2 * (u + 1)
    cfg.close()


# ---- 4. outcomes: an open argument is written, a refused one is not, the others do not notice -------------------------
@REPR
def test_one_wrong_cell_of_the_permuted_input_leaves_that_argument_open(hsw, eng_int, mont):
    N = hsw._native
    cfg = spread_cfg(hsw, eng_int, mont)
    r = tile_rows(hsw, eng_int)
    u, a, j = r + 300, 3, r + 5                                               # (the cell lies in the second tile)
    case = Case(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, 3, mont, 300, order="interleaved")
    clean, _, _ = case.run()
    tab = ints(value_table("spread", T_SPREAD, case.theta[1], mont))
    now = case.peek("pin", a, j)
    case.poke("pin", a, j, tab[(tab.index(now) + 1) % T_SPREAD])              # another table row
    zs, status, rep = case.run()
    assert status.tolist() == [0, 0, 0, N.HSW_PRODUCT_OPEN, 0, 0] and rep["open_arguments"] == 1 and rep["first_open"] == a
    assert rep["written"] == 6 * (u + 1)
    for b in range(6):
        assert np.array_equal(zs[b], clean[b]) == (b != a)
    assert np.array_equal(zs[a][: j + 1], clean[a][: j + 1]) and not np.array_equal(zs[a][j + 1], clean[a][j + 1])
    cfg.close()


@REPR
def test_beta_that_cancels_a_permuted_cell_refuses_that_argument(hsw, eng_int, mont):
    N = hsw._native
    cfg = spread_cfg(hsw, eng_int, mont)
    u, a, j = 300, 2, 123
    case = Case(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, 3, mont, 400, order="reversed")
    betas = list(case.beta)
    betas[a // 2] = (P_INT - value(case.peek("pin", a, j), mont)) % P_INT     # beta = -A'[j]: den[j] = 0
    zs, status, rep = case.run(betas)
    assert status[a] == N.HSW_PRODUCT_ZERO_DENOM and zs[a] is None
    assert [zs[b] is not None and status[b] == 0 for b in (0, 1, 4, 5)] == [True] * 4   # the other proofs' arguments are written
    assert rep["first_refused"] == a and rep["refused_arguments"] in (1, 2)   # (argument 3 shares beta: the model decided)
    cfg.close()


@REPR
@pytest.mark.parametrize("family", ["pin", "ptab", "in", "sp"])
def test_a_cell_stored_as_m_plus_p_refuses_that_argument(hsw, eng_int, family, mont):
    N = hsw._native
    cfg = spread_cfg(hsw, eng_int, mont)
    r = tile_rows(hsw, eng_int)
    u, a, j = r + 40, 4, r + 2
    case = Case(cfg, hsw, N.HSW_LOOKUP_SPREAD, u, 3, mont, 500)
    case.poke(family, a, j, case.peek(family, a, j) + P_INT)                  # the same value, not an encoding below p
    zs, status, rep = case.run()
    assert status.tolist() == [0, 0, 0, 0, N.HSW_PRODUCT_CELL_NOT_BELOW_P, 0] and zs[a] is None
    assert rep["refused_arguments"] == 1 and rep["first_refused"] == a and rep["written"] == 5 * (u + 1)
    cfg.close()


# ---- 5. end to end: K = 2 bench proofs bound by column tables, counted permuted pair, then Z --------------------------
@REPR
def test_bench_proofs_bound_by_column_tables_end_to_end(hsw, eng_int, mont):
    import torch
    N = hsw._native
    K, origin = 2, (0, 0, False, 0)
    msgs = [bytes([h + 1] * 56) for h in range(K)]
    cfg = make(hsw, eng_int, "images", [1024], K, origin, mont)
    columns, lp, rows = geometry(hsw, eng_int, "images", [1024], K, origin, mont, None)
    keep = CarvedAll(K, columns, interleaved(K, columns, list(range(columns))[::-1]), lp, rows)
    cfg.bind_columns(**keep.kw)
    cfg.digest_batch(msgs)
    runs = cfg.lookup_runs()
    theta = [theta_of(900 + c) for c in range(K)]
    beta = [theta_of(910 + c) for c in range(K)]
    gamma = [theta_of(920 + c) for c in range(K)]
    enc = lambda vs: [stored(v, mont) for v in vs]                            # noqa: E731
    for table, u in ((N.HSW_LOOKUP_RANGE, 65536 + 3), (N.HSW_LOOKUP_SPREAD, 16 * 4120 // 2 + 1)):
        spread = table == N.HSW_LOOKUP_SPREAD
        mine = [x for x in runs if x["table"] == table]
        n_args = 2 * K if spread else K
        assert [(x["context"], x["column"]) for x in mine] == [(a // 2, a % 2) if spread else (a, 0) for a in range(n_args)]   # one run each
        pin, ptab, _, prep = cfg.lookup_permuted(table, u, thetas=enc(theta) if spread else None)
        assert prep["written"] == 2 * u * n_args and prep["not_in_table"] == 0
        kw = dict(thetas=enc(theta), inputs_spread=[x["d_spread"] for x in mine]) if spread else {}
        out = torch.full((n_args, u + 1 + PAD, 4), SENT, dtype=torch.int64, device="cuda").view(torch.uint64)
        z, status, rep = cfg.lookup_product(table, u, enc(beta), enc(gamma), [x["d_cells"] for x in mine], pin, ptab,
                                            input_rows=[x["n"] for x in mine], out=out, **kw)
        print("end to end: table %d, %d arguments, u %d: %s" % (table, n_args, u, rep))
        assert z is out and not status.any() and rep["open_arguments"] == 0 and rep["refused_arguments"] == 0 and rep["written"] == n_args * (u + 1)
        zh = z.cpu().numpy()
        assert (zh[:, u + 1:] == np.uint64(SENT)).all()
        ph, th = pin.cpu().numpy(), ptab.cpu().numpy()
        host = keep.host()
        for a, x in enumerate(mine):
            c = a // 2 if spread else a
            kind = "spread" if spread else "range"
            cell = (x["d_cells"] - keep.base) // 32
            A = [value(v, mont) for v in ints(host[cell: cell + x["n"]])]
            if spread:
                cell = (x["d_spread"] - keep.base) // 32
                sp = [value(v, mont) for v in ints(host[cell: cell + x["n"]])]
                A = [(d * theta[c] + s) % P_INT for d, s in zip(A, sp)]
            A += [0] * (u - x["n"])
            T = T_SPREAD if spread else 65536
            tv = [val(kind, t, theta[c]) for t in range(T)]
            zv = [value(v, mont) for v in ints(zh[a, : u + 1])]
            pa, ps = [value(v, mont) for v in ints(ph[a])], [value(v, mont) for v in ints(th[a])]
            assert zv[0] == 1 and zv[u] == 1
            bad = [i for i in range(u) if zv[i + 1] * ((pa[i] + beta[c]) * (ps[i] + gamma[c]) % P_INT) % P_INT
                   != zv[i] * ((A[i] + beta[c]) * ((tv[i] if i < T else tv[0]) + gamma[c]) % P_INT) % P_INT]
            assert not bad, (table, a, bad[:5])
        z2, _, _ = cfg.lookup_product(table, u, enc(beta), enc(gamma), [x["d_cells"] for x in mine], pin, ptab,
                                      input_rows=[x["n"] for x in mine], **kw)
        assert np.array_equal(z2.cpu().numpy(), zh[:, : u + 1])               # twice: identical bytes
    assert cfg.verify()["violations"] == 0                                    # nothing of the region was written
    cfg.close()
