"""hsw_gadget_quotient on the MI355X: h(X) on the extended coset, written by the kernels of hsw_quotient.hip.

The yardstick is Python integers: tests/quotient_model.py, which tests/test_quotient_host.py proves on a satisfied
circuit.  Every cell of every h is compared with it, exactly, in both cell forms, on RANDOM columns that satisfy
nothing.  All columns -- inputs and outputs -- are carved out of one buffer with sentinel cells around each; after the
call every byte of it outside rows [0, N) of the h of the proofs that were to be written must be what it was, so no
input byte and no sentinel is ever written.  The calls go through cfg.quotient with device addresses.

The last test runs the chain on the device for the satisfied toy circuit of the host test: hsw_gadget_ntt
(lagrange_to_coeff, coeff_to_extended), hsw_gadget_quotient, hsw_gadget_ntt (extended_to_coeff), hsw_gadget_evaluate.
The permutation's Z comes from the device: hsw_gadget_permutation_product takes the caller's own value and sigma columns,
omega, delta and chunks of L, which is the toy circuit's recurrence; it writes rows 0 .. u, and the blinding rows above
keep random cells, as in the model.  The lookups' Z and permuted pairs come from the model's recurrences:
hsw_gadget_lookup_product derives its table from the pass's RANGE / SPREAD kinds and reads no table column, so the toy
circuit's own table columns have no way into it."""
import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.ntt_model import root_of_unity
from tests.quotient_model import (DELTA, FLEX_GATE, evaluate, inv, numerator_model, quotient_model, toy_at_point, toy_circuit)
from tests.test_gpu_bound_region import REPR, make
from tests.test_gpu_lookup_counts import ORIGIN
from tests.test_gpu_lookup_permuted import R_INT, SENT, limbs, stored

pytestmark = pytest.mark.gpu
PAD = 3                                     # sentinel cells before and after every column
R_INV = pow(R_INT, -1, P_INT)
NONE = (1 << 64) - 1
ZETA = 5


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


def ints(cells):
    b = np.ascontiguousarray(cells, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i: i + 32], "little") for i in range(0, len(b), 32)]


class Case:
    """One call: K proofs of m own columns and F shared ones, random values everywhere."""

    def __init__(self, hsw, cfg, mont, log_rows, e, seed, K=1, m=3, F=2, gates=(), perm=(), L=0, lookups=(), u=None):
        import torch
        self.cfg, self.N, self.mont = cfg, hsw._native, mont
        self.log_rows, self.log_n, self.K, self.m, self.F = log_rows, log_rows + e, K, m, F
        self.rows, self.n = 1 << self.log_n, 1 << log_rows
        self.u = self.n - 6 if u is None else u
        self.gates, self.perm, self.L, self.lookups = list(gates), list(perm), L, list(lookups)
        self.S = -(-len(self.perm) // min(L, len(self.perm))) if self.perm else 0
        rng = np.random.default_rng(seed)
        self.rnd = lambda: int.from_bytes(rng.bytes(40), "little") % P_INT
        col = lambda: [self.rnd() for _ in range(self.rows)]
        nl = len(self.lookups)
        self.v = dict(cols=[[col() for _ in range(m)] for _ in range(K)], fixed=[col() for _ in range(F)], l0=col(), l_last=col(), l_active=col(),
                      sigmas=[col() for _ in self.perm], pz=[[col() for _ in range(self.S)] for _ in range(K)],
                      la=[[col() for _ in range(nl)] for _ in range(K)], ls=[[col() for _ in range(nl)] for _ in range(K)],
                      lz=[[col() for _ in range(nl)] for _ in range(K)])
        self.ch = dict(y=[self.rnd() for _ in range(K)], beta=[self.rnd() for _ in range(K)], gamma=[self.rnd() for _ in range(K)],
                       theta=[self.rnd() for _ in range(K)])
        slots = [("h", c) for c in range(K)]
        for c in range(K):
            slots += [("cols", c, j) for j in range(m)] + [("pz", c, s) for s in range(self.S)]
            slots += [(k, c, l) for l in range(nl) for k in ("la", "ls", "lz")]
        slots += [("fixed", j) for j in range(F)] + [("sigmas", j) for j in range(len(self.perm))] + [("l0",), ("l_last",), ("l_active",)]
        self.at, at = {}, 0
        for slot in slots[::-1] if seed % 2 else slots:                      # (address order both ways)
            self.at[slot] = at + PAD
            at += 2 * PAD + self.rows
        host = np.full((at, 4), np.uint64(SENT), dtype=np.uint64)
        for slot, s in self.at.items():
            if slot[0] == "h":
                continue
            vals = self.v[slot[0]]
            for k in slot[1:]:
                vals = vals[k]
            host[s: s + self.rows] = limbs([stored(x, mont) for x in vals])
        self.buf = torch.from_numpy(host.view(np.int64)).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 16 == 0

    def addr(self, *slot):
        return self.base + 32 * self.at[slot]

    def poke(self, slot, row, x):
        import torch
        self.buf[self.at[slot] + row] = torch.from_numpy(limbs([x]).copy().view(np.int64)[0]).cuda()
        torch.cuda.synchronize()

    def want(self, c):
        v, ch = self.v, self.ch
        h, count = quotient_model(self.log_rows, self.log_n, self.u, v["cols"][c], v["fixed"], self.gates, ch["y"][c], root_of_unity(self.log_n), ZETA,
                                  l0=v["l0"], l_last=v["l_last"], l_active=v["l_active"], perm_columns=self.perm, L=min(self.L, len(self.perm)) or 1,
                                  sigmas=v["sigmas"], perm_z=v["pz"][c], delta=DELTA, beta=ch["beta"][c], gamma=ch["gamma"][c], lookups=self.lookups,
                                  perm_inputs=v["la"][c], perm_tables=v["ls"][c], lookup_z=v["lz"][c], theta=ch["theta"][c])
        return limbs([stored(x, self.mont) for x in h]), count

    def call(self, **over):
        K, m, nl, mont = self.K, self.m, len(self.lookups), self.mont
        enc = lambda xs: limbs([stored(x, mont) for x in xs]).copy()         # noqa: E731
        kw = dict(log_rows=self.log_rows, log_n=self.log_n, usable_rows=self.u,
                  columns=[[self.addr("cols", c, j) for j in range(m)] for c in range(K)], ys=enc(self.ch["y"]),
                  omega_ext=enc([root_of_unity(self.log_n)]), zeta=enc([ZETA]), fixed=[self.addr("fixed", j) for j in range(self.F)],
                  gates=[[(stored(coeff, mont), factors) for coeff, factors in g] for g in self.gates],
                  out=[self.addr("h", c) for c in range(K)])
        if self.perm or self.lookups:
            kw.update(l0=self.addr("l0"), l_last=self.addr("l_last"), l_active=self.addr("l_active"), betas=enc(self.ch["beta"]), gammas=enc(self.ch["gamma"]))
        if self.perm:
            kw.update(perm_columns=self.perm, chunk_columns=self.L, sigmas=[self.addr("sigmas", j) for j in range(len(self.perm))],
                      perm_products=[[self.addr("pz", c, s) for s in range(self.S)] for c in range(K)], delta=enc([DELTA]))
        if self.lookups:
            kw.update(lookups=self.lookups, thetas=enc(self.ch["theta"]),
                      permuted_inputs=[[self.addr("la", c, l) for l in range(nl)] for c in range(K)],
                      permuted_tables=[[self.addr("ls", c, l) for l in range(nl)] for c in range(K)],
                      lookup_products=[[self.addr("lz", c, l) for l in range(nl)] for c in range(K)])
        kw.update(over)
        return self.cfg.quotient(**kw)

    def run(self, refused=(), launches=None):
        """the call, then every check; returns (h cells per proof or None, report)"""
        N, K, rows = self.N, self.K, self.rows
        before = self.buf.cpu().numpy().view(np.uint64).copy()
        _, status, report = self.call()
        after = self.buf.cpu().numpy().view(np.uint64)
        print("quotient: log_rows %d, log_n %d, K %d, %d expressions, %d launches, %d rows per thread, scratch %d bytes, kernel %.3f ms "
              "(gates %.3f, permutation %.3f, lookups %.3f, finish %.3f), status %s"
              % (self.log_rows, self.log_n, K, report["expressions"], report["launches"], report["rows_per_thread"], report["scratch_bytes"],
                 report["kernel_ms"], report["gates_ms"], report["permutation_ms"], report["lookups_ms"], report["finish_ms"], status.tolist()))
        changed = np.zeros(len(after), dtype=bool)
        outs = []
        for c in range(K):
            s = self.at[("h", c)]
            if c in refused:
                assert status[c] == N.HSW_QUOTIENT_CELL_NOT_BELOW_P, (c, status[c])
                outs.append(None)
                continue
            assert status[c] == 0, (c, status[c])
            changed[s: s + rows] = True
            want, count = self.want(c)
            got = after[s: s + rows]
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert not len(bad), "proof %d: %d rows differ, the first ones %s" % (c, len(bad), bad[:8].tolist())
            assert report["expressions"] == count
            outs.append(got.copy())
        assert np.array_equal(before[~changed], after[~changed]), "a cell outside rows [0, N) of a written h changed"
        refused = sorted(refused)
        assert report["proofs"] == K and report["written"] == rows * (K - len(refused)) and report["refused_proofs"] == len(refused)
        assert report["first_refused"] == (refused[0] if refused else NONE)
        families = bool(self.gates) + bool(self.perm) + bool(self.lookups) + 1
        batches = -(-K * rows * 32 // report["scratch_bytes"])
        assert report["launches"] == families * batches and report["rows_per_thread"] >= 1
        if launches is not None:
            assert report["launches"] == launches
        return outs, report


def toy_gates(n, m, F):
    """gates over columns 0 .. m + F - 1 with rotations -(n-1), -1, 0, +3, +(n-1)"""
    w = m + F
    far = n - 1
    return [FLEX_GATE(m, 0),
            [(7, [(1 % w, -far)]), (P_INT - 3, [(2 % w, far), (0, -1)])],
            [(1, [(0, 3), (1 % w, -1), (w - 1, 0)]), (P_INT - 1, [(w - 1, far)])]]


# ---- 1. gates only ---------------------------------------------------------------------------------------------------
@REPR
@pytest.mark.parametrize("log_rows,e", [(4, 2), (6, 1), (10, 2), (9, 3)])
def test_gates_only(hsw, eng_int, log_rows, e, mont):
    cfg = gadget(hsw, eng_int, mont)
    n = 1 << log_rows
    gates = toy_gates(n, 3, 2)
    if (log_rows, e) == (4, 2):
        gates.append([(12345, [])])                                          # a gate that is a bare constant
    if (log_rows, e) == (6, 1):                                              # a monomial of HSW_QUOTIENT_MAX_FACTORS factors, and a constant term
        gates.append([(P_INT - 2, [(j % 5, r) for j, r in zip(range(8), (-(n - 1), -1, 0, 3, n - 1, 0, 1, -2))]), (9, [])])
        assert len(gates[-1][0][1]) == hsw._native.HSW_QUOTIENT_MAX_FACTORS
    Case(hsw, cfg, mont, log_rows, e, 100 + log_rows + e, gates=gates).run(launches=2)
    cfg.close()


# ---- 2. permutation only ---------------------------------------------------------------------------------------------
@REPR
@pytest.mark.parametrize("log_rows,e", [(4, 2), (10, 2)])
@pytest.mark.parametrize("n_perm,L", [(1, 4), (4, 2), (5, 2)])
def test_permutation_only(hsw, eng_int, n_perm, L, log_rows, e, mont):
    cfg = gadget(hsw, eng_int, mont)
    perm = [4, 0, 3, 1, 2][:n_perm]                                          # (column 4 and 3: shared fixed columns among the permuted ones)
    case = Case(hsw, cfg, mont, log_rows, e, 200 + n_perm + log_rows, perm=perm, L=L)
    assert case.u == (1 << log_rows) - 6
    case.run(launches=2)
    cfg.close()


# ---- 3. lookups only -------------------------------------------------------------------------------------------------
@REPR
@pytest.mark.parametrize("log_rows,e", [(4, 2), (10, 2)])
def test_lookups_only(hsw, eng_int, log_rows, e, mont):
    cfg = gadget(hsw, eng_int, mont)
    Case(hsw, cfg, mont, log_rows, e, 300 + log_rows, lookups=[([2], [3]), ([0, 4], [4, 1])]).run(launches=2)
    cfg.close()


# ---- 4. everything together, K = 3, refusals -------------------------------------------------------------------------
def everything(hsw, cfg, mont, seed, K=3, log_rows=8):
    n = 1 << log_rows
    return Case(hsw, cfg, mont, log_rows, 2, seed, K=K, gates=toy_gates(n, 3, 2), perm=[0, 3, 1, 2, 4], L=2, lookups=[([2], [3]), ([0, 4], [4, 1])])


@REPR
def test_everything_and_a_bad_cell_of_one_proof(hsw, eng_int, mont):
    cfg = gadget(hsw, eng_int, mont)
    case = everything(hsw, cfg, mont, 400)
    case.run(launches=4)
    case.poke(("cols", 1, 2), 777, P_INT)                                    # p itself, in a column proof 1 alone reads
    case.run(refused={1}, launches=4)
    cfg.close()


@REPR
def test_a_bad_cell_of_a_shared_column_refuses_every_proof(hsw, eng_int, mont):
    cfg = gadget(hsw, eng_int, mont)
    case = everything(hsw, cfg, mont, 401)
    case.poke(("fixed", 1), 5, P_INT + 1)
    _, report = case.run(refused={0, 1, 2})
    assert report["written"] == 0
    cfg.close()


# ---- 5. scratch batches ----------------------------------------------------------------------------------------------
@REPR
def test_two_batches_give_the_single_batch_result(hsw, eng_int, mont):
    cfg = gadget(hsw, eng_int, mont)
    case = everything(hsw, cfg, mont, 500, K=3, log_rows=6)
    one, rep1 = case.run(launches=4)
    eng_int.set_option("quotient_scratch", 2 * case.rows * 32)               # two proofs at a time: batches of 2 and 1
    try:
        two, rep2 = case.run(launches=8)
    finally:
        eng_int.set_option("quotient_scratch", 1 << 30)
    assert rep1["scratch_bytes"] == 3 * case.rows * 32 and rep2["scratch_bytes"] == 2 * case.rows * 32
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    cfg.close()


# ---- 6. refusals that need a device pointer --------------------------------------------------------------------------
@REPR
def test_overlaps_and_alignment_are_refused_before_any_launch(hsw, eng_int, mont):
    N = hsw._native
    cfg = gadget(hsw, eng_int, mont)
    case = everything(hsw, cfg, mont, 600, K=2, log_rows=4)
    before = case.buf.cpu().numpy().copy()
    h0, h1 = case.addr("h", 0), case.addr("h", 1)
    bad = [(dict(out=[h0, h0 + 32 * (case.rows - 1)]), "its d_h overlaps the d_h of proof"),
           (dict(out=[case.addr("cols", 1, 0) + 32, h1]), "its d_h overlaps column 3"),
           (dict(out=[h0, case.addr("fixed", 1) - 32 * (case.rows - 1)]), "proof 1: its d_h overlaps fixed column"),
           (dict(out=[case.addr("l_active"), h1]), "overlaps l_active"),
           (dict(out=[h0, case.addr("lz", 1, 1)]), "overlaps lookup product 3"),
           (dict(l0=case.addr("l0") + 8), "l0 0: a pointer that is NULL or not 16-byte aligned"),
           (dict(out=[h0, h1 + 4]), "proof 1: a d_h pointer that is NULL or not 16-byte aligned"),
           (dict(sigmas=[case.addr("sigmas", j) + (8 if j == 2 else 0) for j in range(5)]), "sigma 2: a pointer that is NULL or not 16-byte aligned")]
    for over, text in bad:
        with pytest.raises(RuntimeError) as err:
            case.call(**over)
        assert err.value.status == N.HSW_ERR_INVALID_ARG and text in str(err.value), str(err.value)
    assert np.array_equal(before, case.buf.cpu().numpy())                    # nothing was launched: nothing changed
    case.run()
    cfg.close()


# ---- 7. the chain on the device, on the satisfied toy circuit --------------------------------------------------------
@REPR
def test_the_chain_on_the_device_proves_the_toy_circuit(hsw, eng_int, mont):
    import torch
    cfg = gadget(hsw, eng_int, mont)
    t = toy_circuit()
    lr, e, u = t["log_rows"], 2, t["u"]
    ln, n = lr + e, 1 << lr
    rows = 1 << ln
    omega, w = root_of_unity(lr), root_of_unity(ln)
    names = [("advice", j) for j in range(3)] + [("fixed", j) for j in range(7)] + [("sigma", j) for j in range(3)] + [("perm_z", j) for j in range(2)]
    base = [t[k][j] for k, j in names] + [t["lookups"][l][k] for l in range(2) for k in range(3)] + [t["l0"], t["l_last"], t["l_active"]]
    dev = lambda cols: torch.from_numpy(np.stack([limbs([stored(x, mont) for x in c]) for c in cols]).view(np.int64).copy()).cuda().view(torch.uint64)
    enc = lambda x: limbs([stored(x, mont)]).copy()                          # noqa: E731
    lagrange = dev(base)
    # the permutation's Z by hsw_gadget_permutation_product, from the advice and sigma columns as they lie in `lagrange`;
    # it writes rows 0 .. u, the blinding rows above keep the model's random cells
    S = len(t["perm_z"])
    l64 = lagrange.view(torch.int64)                                         # (names: advice 0 .. 2, sigma 10 .. 12, perm_z 13, 14)
    z, st, prep = cfg.permutation_product(u, t["L"], enc(t["beta"]), enc(t["gamma"]), enc(omega), enc(DELTA),
                                          l64[0:3].unsqueeze(0).view(torch.uint64), l64[10:13].view(torch.uint64))
    assert not st.any() and prep["refused_proofs"] == 0 and tuple(z.shape) == (1, S, u + 1, 4)        # status 0: the last Z closes at 1
    for s in range(S):
        assert ints(z[0, s].view(torch.int64).cpu().numpy().view(np.uint64)) == [stored(x, mont) for x in t["perm_z"][s][:u + 1]]
        assert any(t["perm_z"][s][u + 1:])
    l64[13:13 + S, :u + 1] = z.view(torch.int64)[0]                           # the quotient below reads the device's Z
    torch.cuda.synchronize()
    coeff, st, _ = cfg.ntt(lr, enc(inv(omega)), lagrange, scale=enc(inv(n)))                              # lagrange_to_coeff
    assert not st.any()
    wide = torch.zeros((len(base), rows, 4), dtype=torch.int64, device=lagrange.device)
    wide[:, :n] = coeff.view(torch.int64)
    wide = wide.view(torch.uint64)
    ext, st, _ = cfg.ntt(ln, enc(w), wide, input_rows=[n] * len(base), shift=enc(ZETA))                   # coeff_to_extended
    assert not st.any()
    col = lambda i: ext.data_ptr() + i * rows * 32
    gates = [[(stored(c, mont), f) for c, f in g] for g in t["gates"]]
    h, st, rep = cfg.quotient(lr, ln, u, [[col(0), col(1), col(2)]], enc(t["y"]), enc(w), enc(ZETA), fixed=[col(3 + j) for j in range(7)], gates=gates,
                              l0=col(21), l_last=col(22), l_active=col(23), perm_columns=t["perm_columns"], chunk_columns=t["L"],
                              sigmas=[col(10 + j) for j in range(3)], perm_products=[[col(13), col(14)]], delta=enc(DELTA), betas=enc(t["beta"]),
                              gammas=enc(t["gamma"]), lookups=t["lookup_columns"], permuted_inputs=[[col(15), col(18)]],
                              permuted_tables=[[col(16), col(19)]], lookup_products=[[col(17), col(20)]], thetas=enc(t["theta"]))
    assert not st.any() and rep["expressions"] == 17 and rep["launches"] == 4
    hc, st, _ = cfg.ntt(ln, enc(inv(w)), h, shift=enc(inv(ZETA)), scale=enc(inv(rows)), shift_after=True)   # extended_to_coeff
    assert not st.any()
    got = [x * R_INV % P_INT if mont else x for x in ints(hc[0].view(torch.int64).cpu().numpy().view(np.uint64))]
    assert any(got[:3 * n]) and not any(got[3 * n:])                         # degree below (d - 1) n, d = 4: three pieces of n rows
    # the identity at a random x, every evaluation by hsw_gadget_evaluate
    x = 0x1234567890ABCDEF1234567890ABCDEF % P_INT
    rots = (0, 1, 2, 3, -1, u)
    points = [x * pow(omega, r % n, P_INT) % P_INT for r in rots]
    queries = [(b, k) for b in range(len(base)) for k in range(len(rots))]
    ev, st, _ = cfg.evaluate(n, coeff, limbs([stored(z, mont) for z in points]).copy(), queries)
    assert not st.any()
    ev = [v * R_INV % P_INT if mont else v for v in ints(ev)]
    index = {id(c): b for b, c in enumerate(base)}
    pt = toy_at_point(t, x, evaluator=lambda c, z: ev[index[id(c)] * len(rots) + points.index(z)])
    V, _ = numerator_model(lr, ln, u, pt["columns"], pt["fixed"], t["gates"], t["y"], w, ZETA, at_x=x, **pt["kw"])
    hx, st, _ = cfg.evaluate(3 * n, hc, enc(x), [(0, 0)])
    assert not st.any()
    hx = ints(hx)[0] * R_INV % P_INT if mont else ints(hx)[0]
    assert hx == evaluate(got, x) and V[0] == hx * (pow(x, n, P_INT) - 1) % P_INT
    cfg.close()
