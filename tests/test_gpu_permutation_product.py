"""hsw_gadget_permutation_product on the MI355X: the grand products Z of halo2's permutation argument, written by the
kernels of hsw_permutation_product.hip.

The yardstick is Python integers.  A result is correct iff for every proof c, chunk s and row i < u
  Z_{c,0}[0] encodes 1,   Z_{c,s}[0] = Z_{c,s-1}[u],   Z_{c,s}[i+1] den_s[i] = Z_{c,s}[i] num_s[i]  (mod p)
-- the argument's own constraint, which determines Z where no den is zero and needs no inversion -- with
  num_s[i] = prod_j (v_j[i] + beta delta^j omega^i + gamma),   den_s[i] = prod_j (v_j[i] + beta sigma_j[i] + gamma)
over the columns j of chunk s, v_j[i] = 0 from column_rows on.  Every row of every Z column is checked, exactly.  All
columns -- values, sigmas, Z -- are carved out of one buffer with sentinel cells around each; after the call every byte of
it outside rows [0, u] of the Z columns that were to be written must be what it was.

omega = 7^((p-1)/2^k) with 2^k > u and delta = 7^(2^28) are the test's: the library pins neither."""
import ctypes as C

import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.test_gpu_bound_region import REPR, make
from tests.test_gpu_lookup_counts import ORIGIN
from tests.test_gpu_lookup_permuted import R_INT, SENT, limbs, stored, theta_of

pytestmark = pytest.mark.gpu
PAD = 3                                     # sentinel cells before and after every column
R_INV = pow(R_INT, -1, P_INT)
GARBAGE = (1 << 64) - 2                     # every limb of a value cell that must not be read: far above p, and not 0
DELTA = pow(7, 1 << 28, P_INT)
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


def omega_for(u):
    k = max(1, u.bit_length())              # 2^k > u
    return pow(7, (P_INT - 1) >> k, P_INT)


def ints(cells):
    """(n, 4) uint64 -> Python ints"""
    b = np.ascontiguousarray(cells, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i: i + 32], "little") for i in range(0, len(b), 32)]


def value(x, mont):
    """the field element a stored cell stands for (reduced: an encoding m + p stands for what m stands for)"""
    return x * R_INV % P_INT if mont else x % P_INT


def labels(m, u, omega):
    """delta^j omega^i, [j][i]"""
    row = [1] * u
    for i in range(1, u):
        row[i] = row[i - 1] * omega % P_INT
    out, dj = [], 1
    for _ in range(m):
        out.append([dj * w % P_INT for w in row])
        dj = dj * DELTA % P_INT
    return out


def model(values, sigma, heights, beta, gamma, lab, L, u):
    """(num, den) per chunk and row of one proof, from VALUES (not encodings); values[j] holds heights[j] entries"""
    m = len(sigma)
    num, den = [], []
    for j0 in range(0, m, L):
        n, d = [1] * u, [1] * u
        for j in range(j0, min(m, j0 + L)):
            v, sg, lb, h = values[j], sigma[j], lab[j], heights[j]
            for i in range(u):
                x = (v[i] if i < h else 0) + gamma
                n[i] = n[i] * (x + beta * lb[i]) % P_INT
                d[i] = d[i] * (x + beta * sg[i]) % P_INT
        num.append(n)
        den.append(d)
    return num, den


def check_z(z, num, den, u):
    """z[s]: the VALUES of Z_s[0 .. u]; returns Z_{S-1}[u]"""
    last = 1
    for s in range(len(z)):
        assert z[s][0] == last, "chunk %d does not start where chunk %d ended" % (s, s - 1)
        zs, n, d = z[s], num[s], den[s]
        bad = [i for i in range(u) if zs[i + 1] * d[i] % P_INT != zs[i] * n[i] % P_INT]
        assert not bad, "chunk %d: the recurrence fails at rows %s" % (s, bad[:5])
        last = zs[u]
    return last


class Case:
    """One call's columns: per proof m value columns of u cells and S Z columns of u + 1, and m sigma columns of u,
    carved in the slot order `order`.  sigma is a true permutation of the labels -- cycles of 1 to 4 cells drawn across
    rows, columns and chunks -- and every proof's values are equal along each cycle, so every proof closes.  Cells at or
    beyond a column's height in ANY proof are cycles of their own (they count as 0 there)."""

    def __init__(self, cfg, hsw, K, m, L, u, mont, seed, order="ascending", heights=None):
        import torch
        N = hsw._native
        self.cfg, self.N, self.K, self.m, self.L, self.u, self.mont = cfg, N, K, m, L, u, mont
        self.S = (m + L - 1) // L
        self.heights = [list(h) for h in heights] if heights is not None else [[u] * m for _ in range(K)]
        rng = np.random.default_rng(seed)
        self.omega = omega_for(u)
        self.lab = labels(m, u, self.omega)
        self.beta = [theta_of(seed * 31 + 2 * c) for c in range(K)]
        self.gamma = [theta_of(seed * 31 + 2 * c + 1) for c in range(K)]
        low = [min(self.heights[c][j] for c in range(K)) for j in range(m)]
        cells = [(j, i) for j in range(m) for i in range(low[j])]
        cells = [cells[k] for k in rng.permutation(len(cells))]
        self.cycles, at = [], 0
        while at < len(cells):
            n = int(rng.integers(1, 5))
            self.cycles.append(cells[at: at + n])
            at += n
        sigma = [list(self.lab[j]) for j in range(m)]                          # identity wherever no cycle says otherwise
        rand_value = lambda: int.from_bytes(rng.bytes(40), "little") % P_INT   # noqa: E731
        vals = [[[rand_value() if i < self.heights[c][j] else None for i in range(u)] for j in range(m)] for c in range(K)]
        for cyc in self.cycles:
            for t, (j, i) in enumerate(cyc):
                nj, ni = cyc[(t + 1) % len(cyc)]
                sigma[j][i] = self.lab[nj][ni]
            for c in range(K):
                x = rand_value()
                for j, i in cyc:
                    vals[c][j][i] = x
        slots = [("s", 0, j) for j in range(m)]
        for c in range(K):
            slots += [("v", c, j) for j in range(m)] + [("z", c, s) for s in range(self.S)]
        if order == "reversed":
            slots = slots[::-1]
        elif order == "interleaved":
            slots = slots[1::2] + slots[0::2]
        self.at, at = {}, 0
        for slot in slots:
            self.at[slot] = at + PAD
            at += 2 * PAD + u + (1 if slot[0] == "z" else 0)
        host = np.full((at, 4), np.uint64(SENT), dtype=np.uint64)
        for j in range(m):
            s = self.at[("s", 0, j)]
            host[s: s + u] = limbs([stored(x, mont) for x in sigma[j]])
            for c in range(K):
                s, h = self.at[("v", c, j)], self.heights[c][j]
                host[s: s + u] = np.uint64(GARBAGE)
                if h:
                    host[s: s + h] = limbs([stored(x, mont) for x in vals[c][j][:h]])
        self.buf = torch.from_numpy(host.view(np.int64)).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 16 == 0

    def addr(self, slot, row=0):
        return self.base + 32 * (self.at[slot] + row)

    def poke(self, slot, row, x):
        """store the 256-bit integer x as the cell"""
        import torch
        self.buf[self.at[slot] + row] = torch.from_numpy(limbs([x]).copy().view(np.int64)[0]).cuda()
        torch.cuda.synchronize()

    def peek(self, slot, row):
        return ints(self.buf[self.at[slot] + row].cpu().numpy().view(np.uint64).reshape(1, 4))[0]

    def arguments(self, betas=None, z_slots=None):
        """(args, what must stay alive)"""
        N, K, m, S, mont = self.N, self.K, self.m, self.S, self.mont
        enc = lambda vs: np.array(limbs([stored(v, mont) for v in vs]))      # noqa: E731 (a writable copy)
        be, ga = enc(betas if betas is not None else self.beta), enc(self.gamma)
        om, de = enc([self.omega]), enc([DELTA])
        status = np.full(K, 0xFFFFFFFF, dtype=np.uint32)
        cols = (C.c_void_p * (K * m))(*[self.addr(("v", c, j)) for c in range(K) for j in range(m)])
        flat = [h for hs in self.heights for h in hs]
        rows = (C.c_uint64 * (K * m))(*flat) if flat != [self.u] * (K * m) else None
        sig = (C.c_void_p * m)(*[self.addr(("s", 0, j)) for j in range(m)])
        zs = (C.c_void_p * (K * S))(*(z_slots or [self.addr(("z", c, s)) for c in range(K) for s in range(S)]))
        args = N.PermutationProduct(0, self.L, self.u, m, cols, rows, sig, zs, be.ctypes.data, ga.ctypes.data, om.ctypes.data, de.ctypes.data,
                                    status.ctypes.data_as(C.POINTER(C.c_uint32)))
        return args, (be, ga, om, de, status, cols, rows, sig, zs)

    def run(self, betas=None):
        """the call, then every check that holds for any outcome; returns (Z cells per proof or None, status, report)"""
        import torch
        N, K, m, S, u, mont = self.N, self.K, self.m, self.S, self.u, self.mont
        betas = betas if betas is not None else self.beta
        before = self.buf.cpu().numpy().view(np.uint64).copy()
        args, keep = self.arguments(betas)
        status = keep[4]
        rep = N.PermutationReport()
        torch.cuda.synchronize()
        self.cfg._ok(self.cfg.lib.hsw_gadget_permutation_product(self.cfg.h, C.byref(args), C.byref(rep)))
        after = self.buf.cpu().numpy().view(np.uint64)
        report = {f[0]: getattr(rep, f[0]) for f in N.PermutationReport._fields_}
        print("permutation product: K %d, m %d, L %d, u %d, written %d, tiles %.3f ms, scan %.3f ms, write %.3f ms, status %s"
              % (K, m, self.L, u, report["written"], report["tiles_ms"], report["scan_ms"], report["write_ms"], status.tolist()))
        sig_cells = [ints(before[self.at[("s", 0, j)]: self.at[("s", 0, j)] + u]) for j in range(m)]
        sigma = [[value(x, mont) for x in col] for col in sig_cells]
        changed = np.zeros(len(after), dtype=bool)
        zs, n_written, opened, refused = [], 0, [], []
        for c in range(K):
            hs = self.heights[c]
            v_cells = [ints(before[self.at[("v", c, j)]: self.at[("v", c, j)] + hs[j]]) for j in range(m)]
            num, den = model([[value(x, mont) for x in col] for col in v_cells], sigma, hs, betas[c], self.gamma[c], self.lab, self.L, u)
            want = 0
            if any(x >= P_INT for col in v_cells + sig_cells for x in col):
                want |= N.HSW_PRODUCT_CELL_NOT_BELOW_P
            if any(0 in d for d in den):
                want |= N.HSW_PRODUCT_ZERO_DENOM
            got = [after[self.at[("z", c, s)]: self.at[("z", c, s)] + u + 1] for s in range(S)]
            if want:
                assert status[c] == want, (c, status[c], want)
                assert all((g == np.uint64(SENT)).all() for g in got), "a refused proof was written"
                refused.append(c)
                zs.append(None)
                continue
            for s in range(S):
                changed[self.at[("z", c, s)]: self.at[("z", c, s)] + u + 1] = True
            n_written += 1
            z = [ints(g) for g in got]
            assert all(x < P_INT for col in z for x in col), "a Z cell that is not below p"
            last = check_z([[value(x, mont) for x in col] for col in z], num, den, u)
            assert status[c] == (N.HSW_PRODUCT_OPEN if last != 1 else 0), (c, status[c], last != 1)
            if last != 1:
                opened.append(c)
            zs.append([g.copy() for g in got])
        assert np.array_equal(before[~changed], after[~changed]), "a cell outside rows [0, u] of a written Z column changed"
        assert report["proofs"] == K and report["products"] == K * S and report["written"] == (u + 1) * S * n_written
        assert report["open_proofs"] == len(opened) and report["refused_proofs"] == len(refused)
        assert report["first_open"] == (opened[0] if opened else NONE) and report["first_refused"] == (refused[0] if refused else NONE)
        assert report["tile_rows"] == 1024 and abs(report["kernel_ms"] - (report["tiles_ms"] + report["scan_ms"] + report["write_ms"])) < 1e-3
        return zs, status, report


def proofs(hsw, eng, mont, K):
    return make(hsw, eng, "images", [64], K, ORIGIN, mont)                  # K proofs, nothing digested: the columns are synthetic


# ---- 1. closes: one row, a thread's partial group, u + 1 = one tile, one tile + 1, three tiles -------------------------
# every u with two (m, L), every (m, L) twice, K = 1 and 3; each with both cell forms
GRID = [(1, 1, 1, 1), (1, 3, 2, 3), (5, 5, 2, 3), (5, 2, 5, 1), (1023, 4, 4, 1), (1023, 1, 1, 3), (1024, 3, 2, 3), (1024, 2, 5, 1),
        (2500, 5, 2, 3), (2500, 4, 4, 1)]


@REPR
@pytest.mark.parametrize("which", range(len(GRID)), ids=["u%d_m%d_L%d_K%d" % g for g in GRID])
def test_true_permutations_close(hsw, eng_int, which, mont):
    u, m, L, K = GRID[which]
    cfg = proofs(hsw, eng_int, mont, K)
    case = Case(cfg, hsw, K, m, L, u, mont, 100 + which, order=["ascending", "reversed", "interleaved"][which % 3])
    if u >= 1023 and m > L:
        assert any(len({j // L for j, _ in cyc}) > 1 for cyc in case.cycles)  # cycles span chunks
    zs, status, rep = case.run()
    assert rep["open_proofs"] == 0 and rep["refused_proofs"] == 0 and not status.any() and rep["written"] == K * case.S * (u + 1)
    one = limbs([stored(1, mont)])[0]
    assert all(np.array_equal(z[-1][u], one) and np.array_equal(z[0][0], one) for z in zs)
    if which % 4 == 0:
        zs2, _, _ = case.run()                                                # again: the same bytes
        assert all(np.array_equal(x, y) for a, b in zip(zs, zs2) for x, y in zip(a, b))
    cfg.close()


# ---- 2. column_rows: heights below u, garbage beyond them that must not be read ----------------------------------------
@REPR
def test_short_columns_count_as_zero_and_are_not_read(hsw, eng_int, mont):
    K, m, L, u = 2, 5, 2, 1300
    cfg = proofs(hsw, eng_int, mont, K)
    heights = [[1300, 0, 17, 1299, 1024], [1, 1300, 1025, 700, 1023]]
    case = Case(cfg, hsw, K, m, L, u, mont, 200, order="interleaved", heights=heights)
    assert case.peek(("v", 0, 2), 17) == int.from_bytes(GARBAGE.to_bytes(8, "little") * 4, "little")
    zs, status, rep = case.run()
    assert rep["open_proofs"] == 0 and rep["refused_proofs"] == 0 and not status.any() and rep["written"] == K * 3 * (u + 1)
    cfg.close()


# ---- 3. open: one cell of one cycle changed in proof 1 of 3 -------------------------------------------------------------
@REPR
def test_one_changed_cell_of_a_cycle_leaves_that_proof_open(hsw, eng_int, mont):
    N = hsw._native
    K, m, L, u = 3, 3, 2, 1024 + 300
    cfg = proofs(hsw, eng_int, mont, K)
    case = Case(cfg, hsw, K, m, L, u, mont, 300, order="interleaved")
    clean, _, _ = case.run()
    j, i = next(cyc for cyc in case.cycles if len(cyc) > 1 and cyc[0][1] > 1024 and cyc[0][0] == 0)[0]   # in the second tile of chunk 0
    case.poke(("v", 1, j), i, stored((value(case.peek(("v", 1, j), i), mont) + 1) % P_INT, mont))
    zs, status, rep = case.run()                                              # (OPEN exactly when the model's last value is not 1)
    assert status.tolist() == [0, N.HSW_PRODUCT_OPEN, 0] and rep["open_proofs"] == 1 and rep["first_open"] == 1
    assert rep["written"] == K * 2 * (u + 1)
    for c in range(K):
        assert all(np.array_equal(x, y) for x, y in zip(zs[c], clean[c])) == (c != 1)
    assert np.array_equal(zs[1][0][: i + 1], clean[1][0][: i + 1]) and not np.array_equal(zs[1][0][i + 1], clean[1][0][i + 1])
    cfg.close()


# ---- 4. refused: a zero denominator, an encoding that is not below p -----------------------------------------------------
@REPR
def test_a_value_that_cancels_its_sigma_term_refuses_that_proof(hsw, eng_int, mont):
    N = hsw._native
    K, m, L, u = 3, 4, 4, 1024 + 40
    cfg = proofs(hsw, eng_int, mont, K)
    case = Case(cfg, hsw, K, m, L, u, mont, 400, order="reversed")
    c, j, i = 1, 2, 1024 + 2
    sg = value(case.peek(("s", 0, j), i), mont)
    case.poke(("v", c, j), i, stored(-(case.beta[c] * sg + case.gamma[c]) % P_INT, mont))       # v = -(beta sigma + gamma)
    zs, status, rep = case.run()
    assert status.tolist() == [0, N.HSW_PRODUCT_ZERO_DENOM, 0] and zs[1] is None and zs[0] is not None and zs[2] is not None
    assert rep["refused_proofs"] == 1 and rep["first_refused"] == 1 and rep["open_proofs"] == 0 and rep["written"] == 2 * (u + 1)
    cfg.close()


@REPR
@pytest.mark.parametrize("family", ["value", "sigma"])
def test_a_cell_stored_as_m_plus_p_refuses_every_proof_that_reads_it(hsw, eng_int, family, mont):
    N = hsw._native
    K, m, L, u = 3, 3, 2, 1024 + 40
    cfg = proofs(hsw, eng_int, mont, K)
    case = Case(cfg, hsw, K, m, L, u, mont, 500)
    slot, i = (("v", 1, 2) if family == "value" else ("s", 0, 2)), 1024 + 2
    case.poke(slot, i, case.peek(slot, i) + P_INT)                            # the same value, not an encoding below p
    zs, status, rep = case.run()
    bit = N.HSW_PRODUCT_CELL_NOT_BELOW_P
    if family == "value":                                                     # proof 1's own column
        assert status.tolist() == [0, bit, 0] and zs[1] is None and rep["refused_proofs"] == 1 and rep["first_refused"] == 1
        assert rep["written"] == 2 * 2 * (u + 1)
    else:                                                                     # the key's column: every proof reads it
        assert status.tolist() == [bit] * 3 and zs == [None] * 3 and rep["refused_proofs"] == 3 and rep["first_refused"] == 0
        assert rep["written"] == 0
    cfg.close()


# ---- 5. refusals before any launch, on the real runtime ------------------------------------------------------------------
@REPR
def test_an_overlap_and_a_challenge_above_p_are_refused_before_anything_is_written(hsw, eng_int, mont):
    import torch
    N = hsw._native
    K, m, L, u = 2, 3, 2, 300
    cfg = proofs(hsw, eng_int, mont, K)
    case = Case(cfg, hsw, K, m, L, u, mont, 600)
    before = case.buf.cpu().numpy().copy()
    rep = N.PermutationReport()
    z_slots = [case.addr(("z", c, s)) for c in range(K) for s in range(case.S)]
    z_slots[3] = case.addr(("s", 0, 1), u - 1) - 32 * u                       # row u of proof 1's Z_1 is the last cell of sigma_1
    args, keep = case.arguments(z_slots=z_slots)
    torch.cuda.synchronize()
    assert cfg.lib.hsw_gadget_permutation_product(cfg.h, C.byref(args), C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    assert "proof 1" in cfg.lib.hsw_last_error(cfg.engine.h).decode() and "overlaps" in cfg.lib.hsw_last_error(cfg.engine.h).decode()
    assert keep[4].tolist() == [0xFFFFFFFF] * K and rep.written == 0
    args, keep = case.arguments(betas=[case.beta[0], P_INT] if not mont else None)
    if mont:
        keep[0][1] = limbs([P_INT])[0]                                        # (stored() would reduce it)
    assert cfg.lib.hsw_gadget_permutation_product(cfg.h, C.byref(args), C.byref(rep)) == N.HSW_ERR_INVALID_ARG
    assert "below p" in cfg.lib.hsw_last_error(cfg.engine.h).decode() and rep.written == 0
    torch.cuda.synchronize()
    assert np.array_equal(before, case.buf.cpu().numpy())
    zs, status, _ = case.run()                                                # and the same columns, called properly, close
    assert not status.any() and all(z is not None for z in zs)
    cfg.close()


# ---- 6. end to end: the copy constraints of a tree pass on caller-bound columns -----------------------------------------
@REPR
def test_the_ties_of_a_tree_pass_as_a_permutation_close_and_a_broken_tie_opens(hsw, eng_int, mont):
    import torch
    from tests.test_gpu_device_inputs import device_messages, rand
    from tests.test_gpu_device_levels import filled, host, sha
    from tests.test_gpu_origin import MAX_ROWS
    from tests.test_gpu_ties import PITCH, Columns
    N = hsw._native
    a, b = rand(4000, 10), rand(4001, 119)
    probe = hsw.Sha256DynamicConfig(eng_int, [128] * 3, True, whole_digest=True)
    m = probe.set_columns(MAX_ROWS)
    rb = probe.region_binding()
    Lp, chip_rows = int(rb.lookup_capacity), int(rb.chip_rows_capacity)
    probe.close()
    cfg = hsw.Sha256DynamicConfig(eng_int, [128] * 3, True, whole_digest=True)
    if mont:
        cfg.set_repr(N.HSW_REPR_MONTGOMERY)
    assert cfg.set_columns(MAX_ROWS) == m
    cv = Columns(1, m, Lp, chip_rows, reverse=True)
    ptrs = [cv.addr(cv.col_cell[j]) for j in range(m)]
    cfg.bind_columns(ptrs, PITCH, m, **cv.areas)
    _t, slices = device_messages([a, b])
    nodes = filled(128)
    base = nodes.data_ptr()
    cfg.digest_levels_device(slices + [(base, 64)], [0, 0, 1], [base, base + 32, None])          # two leaves, one parent
    assert host(nodes)[:64] == sha(a) + sha(b)
    ties, prefix = cfg.ties()
    assert len(ties) == 64 and prefix == 0 and cfg.verify_ties()["violations"] == 0
    # sigma: the identity, except the cycles the ties form (a source tied to several destinations is one longer cycle)
    u, L = MAX_ROWS, 2
    omega = omega_for(u)
    lab = labels(m, u, omega)
    sigma = [list(col) for col in lab]
    groups = {}
    for t in ties:
        src, dst = cfg.cell_position(int(t["src_cell"])), cfg.cell_position(int(t["dst_cell"]))
        assert cfg.cell_address(int(t["dst_cell"])) == ptrs[dst[0]] + 32 * dst[1] and dst[1] < MAX_ROWS
        groups.setdefault(src, [src]).append(dst)
    for cyc in groups.values():
        for k, (j, i) in enumerate(cyc):
            nj, ni = cyc[(k + 1) % len(cyc)]
            sigma[j][i] = lab[nj][ni]
    d_sigma = torch.from_numpy(np.stack([limbs([stored(x, mont) for x in col]) for col in sigma]).view(np.int64).copy()).cuda().view(torch.uint64)
    beta, gamma = theta_of(700), theta_of(701)
    S = (m + L - 1) // L
    out = torch.full((1, S, u + 1 + PAD, 4), SENT, dtype=torch.int64, device="cuda").view(torch.uint64)
    enc = lambda v: [stored(v, mont)]                                         # noqa: E731

    def call_and_check():
        words = cv.words()
        z, status, rep = cfg.permutation_product(u, L, enc(beta), enc(gamma), enc(omega)[0], enc(DELTA)[0], ptrs, d_sigma,
                                                 column_rows=[MAX_ROWS] * m, out=out)
        assert z is out and rep["refused_proofs"] == 0 and rep["written"] == S * (u + 1) and rep["products"] == S
        zh = z.cpu().numpy()
        assert (zh[:, :, u + 1:] == np.uint64(SENT)).all()
        assert np.array_equal(words, cv.words())                              # nothing of the caller's columns was written
        vals = [[value(x, mont) for x in ints(words[cv.col_cell[j]: cv.col_cell[j] + MAX_ROWS])] for j in range(m)]
        num, den = model(vals, sigma, [MAX_ROWS] * m, beta, gamma, lab, L, u)
        last = check_z([[value(x, mont) for x in ints(zh[0, s, : u + 1])] for s in range(S)], num, den, u)
        print("end to end: m %d, u %d: %s" % (m, u, rep))
        assert status[0] == (N.HSW_PRODUCT_OPEN if last != 1 else 0)
        return last

    assert call_and_check() == 1                                              # the pass satisfies its copy constraints
    # one tied input-byte cell of the parent overwritten with another byte value: the same permutation no longer closes
    j, i = cfg.cell_position(int(ties[5]["dst_cell"]))
    byte = value(ints(cv.words()[cv.col_cell[j] + i].reshape(1, 4))[0], mont)
    assert byte == (sha(a) + sha(b))[5]
    cv.t[cv.col_cell[j] + i] = torch.from_numpy(limbs([stored(byte ^ 0x55, mont)]).copy().view(np.int64)[0]).cuda()
    torch.cuda.synchronize()
    assert cfg.verify_ties()["violations"] == 1
    assert call_and_check() != 1
    cfg.close()
