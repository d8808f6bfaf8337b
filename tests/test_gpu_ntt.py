"""hsw_gadget_ntt on the MI355X: the Fr NTT of device columns, written by the kernels of hsw_ntt.hip.

The yardstick is Python integers: the recursive model of tests/ntt_model.py, proven in tests/test_ntt_host.py against the O(N^2)
definition.  Every output cell of every column is compared with it, exactly, in both cell forms.  All columns -- inputs
and outputs -- are carved out of one buffer with sentinel cells around each; after the call every byte of it outside
rows [0, N) of the outputs that were to be written must be what it was.  Rows of an input at and beyond input_rows hold
limbs far above p: a read of them shows as a refusal or as a wrong value.

omega = 7^((p-1)/2^log_n) is the test's: the library pins no constant, it only checks omega^(N/2) = p - 1."""
import ctypes as C

import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.test_gpu_bound_region import REPR, make
from tests.test_gpu_lookup_counts import ORIGIN
from tests.test_gpu_lookup_permuted import R_INT, SENT, limbs, stored
from tests.ntt_model import default_launches, ntt_model, root_of_unity

pytestmark = pytest.mark.gpu
PAD = 3                                     # sentinel cells before and after every column
R_INV = pow(R_INT, -1, P_INT)
GARBAGE = (1 << 64) - 2                     # every limb of a cell that must not be read: far above p, and not 0
NONE = (1 << 64) - 1
SHIFT, SCALE = 5, pow(12345, -1, P_INT)


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
    """(n, 4) uint64 -> Python ints"""
    b = np.ascontiguousarray(cells, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i: i + 32], "little") for i in range(0, len(b), 32)]


def value(x, mont):
    return x * R_INV % P_INT if mont else x % P_INT


class Case:
    """One call's columns.  heights[b]: input_rows of column b.  reads[b]: the column whose input column b reads (b
    itself by default); in_place: the columns whose output IS their input."""

    def __init__(self, cfg, hsw, log_n, mont, heights, seed, order="ascending", in_place=(), reads=None, values=None):
        import torch
        self.cfg, self.N, self.log_n, self.mont, self.heights = cfg, hsw._native, log_n, mont, list(heights)
        self.n, self.rows = len(heights), 1 << log_n
        self.in_place = set(in_place)
        self.reads = list(reads) if reads is not None else list(range(self.n))
        rng = np.random.default_rng(seed)
        slots = []
        for b in range(self.n):
            if self.reads[b] == b:
                slots.append(("in", b))
            if b not in self.in_place:
                slots.append(("out", b))
        if order == "reversed":
            slots = slots[::-1]
        elif order == "interleaved":
            slots = slots[1::2] + slots[0::2]
        self.at, at = {}, 0
        for slot in slots:
            self.at[slot] = at + PAD
            at += 2 * PAD + self.rows
        host = np.full((at, 4), np.uint64(SENT), dtype=np.uint64)
        for b in range(self.n):
            if self.reads[b] != b:
                continue
            s, h = self.at[("in", b)], self.heights[b]
            host[s: s + self.rows] = np.uint64(GARBAGE)
            if h:
                vals = values[b] if values is not None else [int.from_bytes(rng.bytes(40), "little") % P_INT for _ in range(h)]
                host[s: s + h] = limbs([stored(x, mont) for x in vals])
        self.buf = torch.from_numpy(host.view(np.int64)).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 16 == 0

    def slot_in(self, b):
        return self.at[("in", self.reads[b])]

    def slot_out(self, b):
        return self.at[("in", b)] if b in self.in_place else self.at[("out", b)]

    def poke(self, b, row, x):
        """store the 256-bit integer x as cell `row` of the input of column b"""
        import torch
        self.buf[self.slot_in(b) + row] = torch.from_numpy(limbs([x]).copy().view(np.int64)[0]).cuda()
        torch.cuda.synchronize()

    def run(self, omega=None, shift=None, scale=None, shift_after=False, pass_log=0, launches=None, held=None):
        """the call, then every check that holds for any outcome; returns (output cells per column or None, status, report).
        held: the columns whose points the scratch is to hold between launches (all of them by default)"""
        import torch
        N, n, rows, mont = self.N, self.n, self.rows, self.mont
        omega = root_of_unity(self.log_n) if omega is None else omega
        assert pow(omega, rows // 2, P_INT) == P_INT - 1
        enc = lambda v: np.array(limbs([stored(v, mont)]))                   # noqa: E731 (a writable copy)
        om, sh, sc = enc(omega), enc(shift) if shift is not None else None, enc(scale) if scale is not None else None
        before = self.buf.cpu().numpy().view(np.uint64).copy()
        status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        ins = (C.c_void_p * n)(*[self.base + 32 * self.slot_in(b) for b in range(n)])
        outs = (C.c_void_p * n)(*[self.base + 32 * self.slot_out(b) for b in range(n)])
        hs = (C.c_uint64 * n)(*self.heights) if self.heights != [rows] * n else None
        args = N.Ntt(N.HSW_NTT_SHIFT_AFTER if shift_after else 0, self.log_n, pass_log, 0, n, ins, hs, outs, om.ctypes.data,
                     sh.ctypes.data if sh is not None else None, sc.ctypes.data if sc is not None else None,
                     status.ctypes.data_as(C.POINTER(C.c_uint32)))
        rep = N.NttReport()
        torch.cuda.synchronize()
        self.cfg._ok(self.cfg.lib.hsw_gadget_ntt(self.cfg.h, C.byref(args), C.byref(rep)))
        after = self.buf.cpu().numpy().view(np.uint64)
        report = {f[0]: getattr(rep, f[0]) for f in N.NttReport._fields_}
        print("ntt: log_n %d, columns %d, pass_log %d, launches %d, kernel %.3f ms, twiddles %.3f ms (%d bytes), scratch %d bytes, status %s"
              % (self.log_n, n, report["pass_log"], report["launches"], report["kernel_ms"], report["twiddle_ms"], report["twiddle_bytes"],
                 report["scratch_bytes"], status.tolist()))
        changed = np.zeros(len(after), dtype=bool)
        outputs, refused = [], []
        for b in range(n):
            cells = ints(before[self.slot_in(b): self.slot_in(b) + self.heights[b]])
            got = after[self.slot_out(b): self.slot_out(b) + rows]
            if any(x >= P_INT for x in cells):
                assert status[b] == N.HSW_NTT_CELL_NOT_BELOW_P, (b, status[b])
                refused.append(b)
                outputs.append(None)                                          # (unchanged: checked below with everything else)
                continue
            assert status[b] == 0, (b, status[b])
            changed[self.slot_out(b): self.slot_out(b) + rows] = True
            want = ntt_model([value(x, mont) for x in cells], self.log_n, omega, shift, scale, shift_after)
            want = limbs([stored(x, mont) for x in want])
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert not len(bad), "column %d: %d rows differ, the first ones %s" % (b, len(bad), bad[:8].tolist())
            outputs.append(got.copy())
        assert np.array_equal(before[~changed], after[~changed]), "a cell outside rows [0, N) of a written output changed"
        assert report["columns"] == n and report["written"] == rows * (n - len(refused)) and report["refused_columns"] == len(refused)
        assert report["first_refused"] == (refused[0] if refused else NONE)
        assert report["pass_log"] == (pass_log or 10) and report["launches"] == default_launches(self.log_n, pass_log)
        if launches is not None:
            assert report["launches"] == launches
        assert report["twiddle_bytes"] == 32 * max(1, rows // 2)
        assert report["scratch_bytes"] == (0 if report["launches"] == 1 else 32 * rows * (n if held is None else held))
        return outputs, status, report


# ---- 1. dense random cells, the default geometry: one launch up to 2^10, two from there -----------------------------------
@REPR
@pytest.mark.parametrize("log_n", [1, 2, 3, 5, 8, 10, 11, 12])
def test_dense_columns_of_three_heights(hsw, eng_int, log_n, mont):
    n = 1 << log_n
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, log_n, mont, [n, n - 5 if n > 5 else 1, 0], 100 + log_n, order=["ascending", "reversed", "interleaved"][log_n % 3])
    outs, status, rep = case.run(launches=1 if log_n <= 10 else 2)
    assert not status.any() and not outs[2].any()                              # input_rows 0: N zero cells
    outs2, _, rep2 = case.run(shift=SHIFT, scale=SCALE)
    assert rep2["twiddle_ms"] == 0 and rep2["twiddle_bytes"] == rep["twiddle_bytes"]   # the same root: the cached table
    case.run(shift=SHIFT, shift_after=True)
    cfg.close()


# ---- 2. forced launch counts: three launches and more, log_n a multiple of the digits and not -----------------------------
@REPR
@pytest.mark.parametrize("log_n", [7, 9, 10])
@pytest.mark.parametrize("pass_log", [1, 2, 3, 4])
def test_forced_launch_counts(hsw, eng_int, pass_log, log_n, mont):
    n = 1 << log_n
    digit = pass_log - 2 if pass_log > 3 else 1
    launches = -(-log_n // digit)
    assert launches >= 3
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, log_n, mont, [n, n - 5, 0], 200 + 16 * log_n + pass_log, order="interleaved")
    case.run(pass_log=pass_log, launches=launches)
    case.run(shift=SHIFT, scale=SCALE, pass_log=pass_log, launches=launches)
    case.run(shift=SHIFT, scale=SCALE, shift_after=True, pass_log=pass_log, launches=launches)
    cfg.close()


# ---- 3. the three calls of halo2, chained ---------------------------------------------------------------------------------
@REPR
@pytest.mark.parametrize("k,e", [(6, 2), (10, 3)])
def test_lagrange_to_coeff_to_extended_and_back(hsw, eng_int, k, e, mont):
    import torch
    n, big = 1 << k, 1 << (k + e)
    w, w_ext, zeta = root_of_unity(k), root_of_unity(k + e), 7
    cfg = gadget(hsw, eng_int, mont)
    rng = np.random.default_rng(300 + k)
    column = [int.from_bytes(rng.bytes(40), "little") % P_INT for _ in range(n)]
    lagrange = torch.from_numpy(limbs([stored(x, mont) for x in column]).copy().view(np.int64)).cuda().view(torch.uint64).reshape(1, n, 4)
    one = stored(1, mont)

    def cells(t):
        return [value(x, mont) for x in ints(t.cpu().numpy().reshape(-1, 4))]

    coeff, status, _ = cfg.ntt(k, stored(pow(w, -1, P_INT), mont), lagrange, scale=stored(pow(n, -1, P_INT), mont))
    assert not status.any()
    c = cells(coeff)
    assert ntt_model(c, k, w) == column                                        # the coefficients evaluate back to the column
    ext, status, rep = cfg.ntt(k + e, stored(w_ext, mont), coeff, input_rows=[n], shift=stored(zeta, mont))
    assert not status.any() and rep["launches"] == default_launches(k + e)
    x, got = zeta, cells(ext)
    for i in range(big):                                                       # the polynomial at zeta w_ext^i, by Horner
        acc = 0
        if i < 64 or i % 37 == 0 or i >= big - 2:
            for a in reversed(c):
                acc = (acc * x + a) % P_INT
            assert got[i] == acc, i
        x = x * w_ext % P_INT
    assert got == ntt_model(c, k + e, w_ext, shift=zeta)                       # ... and every row against the model
    back, status, _ = cfg.ntt(k + e, stored(pow(w_ext, -1, P_INT), mont), ext, shift=stored(pow(zeta, -1, P_INT), mont),
                              scale=stored(pow(big, -1, P_INT), mont), shift_after=True)
    assert not status.any() and cells(back) == c + [0] * (big - n)             # the coefficients, and zeros above them
    # shift and scale NULL against an explicit 1: the same bytes
    a, _, _ = cfg.ntt(k + e, stored(w_ext, mont), coeff, input_rows=[n])
    for kw in (dict(shift=one), dict(scale=one), dict(shift=one, scale=one), dict(shift=one, shift_after=True)):
        b, _, _ = cfg.ntt(k + e, stored(w_ext, mont), coeff, input_rows=[n], **kw)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), kw
    cfg.close()


# ---- 4. addressing: in place, pointer orders, two outputs from one input --------------------------------------------------
@REPR
@pytest.mark.parametrize("log_n,pass_log", [(9, 0), (12, 0), (9, 3)], ids=["one_launch", "two_launches", "nine_launches"])
def test_in_place_pointer_orders_and_a_shared_input(hsw, eng_int, log_n, pass_log, mont):
    n = 1 << log_n
    cfg = gadget(hsw, eng_int, mont)
    for which, order in enumerate(("ascending", "reversed", "interleaved")):
        # column 0 in place, column 1 out of place, column 2 reads column 1's input, column 3 in place and short
        case = Case(cfg, hsw, log_n, mont, [n, n - 5, n - 5, 1], 400 + log_n + which, order=order, in_place=(0, 3), reads=[0, 1, 1, 3])
        outs, status, _ = case.run(shift=SHIFT, scale=SCALE, shift_after=bool(which & 1), pass_log=pass_log)
        assert not status.any() and np.array_equal(outs[1], outs[2])
    cfg.close()


# ---- 5. refusal: a stored cell m + p that is read ---------------------------------------------------------------------------
@REPR
@pytest.mark.parametrize("log_n,pass_log", [(9, 0), (12, 0), (8, 4)], ids=["one_launch", "two_launches", "four_launches"])
def test_a_cell_not_below_p_refuses_its_column_alone(hsw, eng_int, log_n, pass_log, mont):
    n = 1 << log_n
    cfg = gadget(hsw, eng_int, mont)
    rows = n - 5
    m = 2 ** 250 // 3                                                          # m + p < 2^256: an encoding that is not below p
    for which, (row, in_place) in enumerate(((0, False), (rows - 1, False), (rows // 2 + 1, False), (rows // 3, True))):
        case = Case(cfg, hsw, log_n, mont, [n, rows, n], 500 + log_n + which, in_place=(1,) if in_place else ())
        case.poke(1, row, m + P_INT)
        outs, status, rep = case.run(scale=SCALE, pass_log=pass_log)
        assert status.tolist() == [0, 4, 0] and rep["refused_columns"] == 1 and rep["first_refused"] == 1 and outs[1] is None
    case = Case(cfg, hsw, log_n, mont, [n, rows, n], 590 + log_n)              # beyond input_rows: not read, not refused
    case.poke(1, rows, m + P_INT)
    _, status, rep = case.run(scale=SCALE, pass_log=pass_log)
    assert not status.any() and rep["refused_columns"] == 0
    cfg.close()


# ---- 5b. groups of columns: the engine option "round_scratch" lowers the 1 GiB a group's points may take --------------------
def grouped_case(cfg, hsw, log_n, mont, seed):
    """column 0 in place, columns 1 and 2 read one input, column 3 is short, column 4 plain"""
    n = 1 << log_n
    return Case(cfg, hsw, log_n, mont, [n, n - 5, n - 5, 7, n], seed, order="interleaved", in_place=(0,), reads=[0, 1, 1, 3, 4])


@REPR
@pytest.mark.parametrize("log_n,pass_log", [(9, 3), (12, 0)], ids=["nine_launches", "two_launches"])
def test_groups_of_columns_under_a_scratch_budget(hsw, eng_int, log_n, pass_log, mont):
    """Five columns in groups of 2, 2, 1 and in five groups of one: column b keeps its points in slot b modulo the group,
    and every group's launches start at its own column and status word."""
    n = 1 << log_n
    cfg = gadget(hsw, eng_int, mont)
    whole, _, _ = grouped_case(cfg, hsw, log_n, mont, 700 + log_n).run(shift=SHIFT, scale=SCALE, pass_log=pass_log)
    try:
        for budget, held in ((2 * n * 32, 2), (2 * n * 32 - 1, 1), (1, 1)):    # groups 2, 2, 1; five of one; five of one
            eng_int.set_option("round_scratch", budget)
            case = grouped_case(cfg, hsw, log_n, mont, 700 + log_n)          # (column 0 is in place: a fresh buffer per call)
            outs, status, _ = case.run(shift=SHIFT, scale=SCALE, pass_log=pass_log, held=held)
            assert not status.any() and all(np.array_equal(a, b) for a, b in zip(outs, whole))
        # a cell not below p in column 3, the second column of the second group: it alone is refused
        for budget, held in ((2 * n * 32, 2), (1, 1)):
            eng_int.set_option("round_scratch", budget)
            case = grouped_case(cfg, hsw, log_n, mont, 700 + log_n)
            case.poke(3, 6, 2 ** 250 // 3 + P_INT)
            outs, status, rep = case.run(shift=SHIFT, scale=SCALE, pass_log=pass_log, held=held)
            assert status.tolist() == [0, 0, 0, 4, 0] and rep["refused_columns"] == 1 and rep["first_refused"] == 3 and outs[3] is None
            assert all(np.array_equal(outs[b], whole[b]) for b in (0, 1, 2, 4))
    finally:
        eng_int.set_option("round_scratch", 1 << 30)
    cfg.close()


@REPR
def test_one_launch_holds_no_scratch_whatever_the_budget(hsw, eng_int, mont):
    """log_n 8 with the default pass_log is one launch: no points lie in the scratch, so the budget cuts nothing"""
    cfg = gadget(hsw, eng_int, mont)
    whole, _, rep = grouped_case(cfg, hsw, 8, mont, 708).run(shift=SHIFT, scale=SCALE, launches=1)
    assert rep["scratch_bytes"] == 0
    try:
        eng_int.set_option("round_scratch", 1)
        outs, status, rep = grouped_case(cfg, hsw, 8, mont, 708).run(shift=SHIFT, scale=SCALE, launches=1)
        assert rep["scratch_bytes"] == 0 and not status.any() and all(np.array_equal(a, b) for a, b in zip(outs, whole))
    finally:
        eng_int.set_option("round_scratch", 1 << 30)
    cfg.close()


# ---- 5c. the other limit of a group: 65,535 columns in a grid dimension ------------------------------------------------------
@REPR
def test_more_columns_than_a_grid_dimension_holds(hsw, eng_int, mont):
    """65,537 columns of two cells (log_n 1, one launch): groups of 65,535 and 2.  The inputs are eight columns read over
    and over -- a shared input is allowed --, the outputs 65,537 columns of 64 bytes side by side in one buffer."""
    import torch
    N, n, K = hsw._native, 65537, 8
    cfg = gadget(hsw, eng_int, mont)
    rng = np.random.default_rng(750)
    vals = [[int.from_bytes(rng.bytes(40), "little") % P_INT for _ in range(2)] for _ in range(K)]
    omega = root_of_unity(1)
    want = np.concatenate([limbs([stored(x, mont) for x in ntt_model(v, 1, omega, SHIFT, SCALE, False)]) for v in vals])   # (2 K, 4)
    src_host = np.full((2 * K + 2 * PAD, 4), np.uint64(SENT), dtype=np.uint64)
    src_host[PAD: PAD + 2 * K] = np.concatenate([limbs([stored(x, mont) for x in v]) for v in vals])
    src = torch.from_numpy(src_host.view(np.int64)).cuda()
    dst = torch.from_numpy(np.full((2 * n + 2 * PAD, 4), np.uint64(SENT), dtype=np.uint64).view(np.int64)).cuda()
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ins = (C.c_void_p * n)(*[src.data_ptr() + 32 * (PAD + 2 * (b % K)) for b in range(n)])
    outs = (C.c_void_p * n)(*[dst.data_ptr() + 32 * (PAD + 2 * b) for b in range(n)])
    enc = lambda v: np.array(limbs([stored(v, mont)]))                       # noqa: E731 (a writable copy)
    om, sh, sc = enc(omega), enc(SHIFT), enc(SCALE)
    status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    args = N.Ntt(0, 1, 0, 0, n, ins, None, outs, om.ctypes.data, sh.ctypes.data, sc.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
    rep = N.NttReport()
    torch.cuda.synchronize()
    cfg._ok(cfg.lib.hsw_gadget_ntt(cfg.h, C.byref(args), C.byref(rep)))
    print("ntt: log_n 1, columns %d (groups of 65535 and 2), launches %d, kernel %.3f ms, scratch %d bytes, refused %d"
          % (rep.columns, rep.launches, rep.kernel_ms, rep.scratch_bytes, rep.refused_columns))
    assert not status.any() and (rep.columns, rep.written, rep.refused_columns, rep.launches, rep.scratch_bytes) == (n, 2 * n, 0, 1, 0)
    got = dst.cpu().numpy().view(np.uint64)
    assert (got[:PAD] == np.uint64(SENT)).all() and (got[PAD + 2 * n:] == np.uint64(SENT)).all()
    assert np.array_equal(got[PAD + 2 * (n - 2): PAD + 2 * n], np.concatenate([want[2 * ((n - 2) % K): 2 * ((n - 2) % K) + 2], want[2 * ((n - 1) % K): 2 * ((n - 1) % K) + 2]]))
    tiled = np.tile(want, (n // K + 1, 1))[:2 * n]
    assert np.array_equal(got[PAD: PAD + 2 * n], tiled), "column %d differs" % (int(np.nonzero((got[PAD: PAD + 2 * n] != tiled).any(axis=1))[0][0]) // 2)
    assert np.array_equal(src.cpu().numpy().view(np.uint64), src_host)
    cfg.close()


# ---- 6. digits of 8 bits: tiles of 2^8 strided x 4 adjacent cells, every cell against the model ---------------------------------
@REPR
@pytest.mark.parametrize("log_n", [15, 16])
def test_digits_of_eight_bits_every_cell(hsw, eng_int, log_n, mont):
    """The default plan at log_n 15 (digits 8, 7) and 16 (8, 8): the first shapes whose strided launches hold runs of
    exactly four cells, the tile the default also takes at 2^22 .. 2^24 and 2^28."""
    n = 1 << log_n
    cfg = gadget(hsw, eng_int, mont)
    case = Case(cfg, hsw, log_n, mont, [n, n - 5], 600 + log_n, order="reversed")
    case.run(shift=SHIFT, scale=SCALE, launches=2)
    case.run(shift=SHIFT, scale=SCALE, shift_after=True, launches=2)
    cfg.close()


# ---- 7. the default geometry at three launches and at its greatest launch count ------------------------------------------------
GREATEST = min(k for k in range(1, 29) if default_launches(k) == max(default_launches(j) for j in range(1, 29)))


@REPR
@pytest.mark.parametrize("log_n", [17, GREATEST], ids=["three_launches", "the_most_launches"])
def test_default_geometry_at_its_launch_counts(hsw, eng_int, log_n, mont):
    """The smallest log_n at which the default takes the most launches it ever takes -- 4, from log_n = 25, read from
    report.launches -- and the smallest with 3.  A column of 2^25 cells is not built from Python integers: the input is
    PERIODIC, a block alpha^r of B = 2^16 rows made once on the host and repeated on the device, cut at N - 5 rows with
    limbs far above p behind them.  With shift g and scale c, z = g w^i and t = alpha z:
      out[i] (t - 1)(z^B - 1) = c ((t^B - 1)(z^N - 1) - (t - 1)(z^B - 1) sum_{k<5} alpha^(B-5+k) z^(N-5+k))
    (the block's geometric sum times the sum over the repeats, less the five rows cut off), which checks a row in
    O(log N) without the model.  Rows 0, 1, N/2, N - 1 and a seeded sample of 2^16 rows are gathered on the device.
    Tests 1, 2 and 6 check every cell of every code path; this one guards the real geometry's sizes."""
    import torch
    assert GREATEST == 25 and default_launches(GREATEST) == 4 and default_launches(17) == 3 and default_launches(16) == 2
    n, w = 1 << log_n, root_of_unity(log_n)
    rows, B = n - 5, 1 << 16
    alpha, g, c = pow(3, 1 << 30, P_INT), pow(11, 1 << 29, P_INT), SCALE
    cfg = gadget(hsw, eng_int, mont)
    a, block = 1, []
    for _ in range(B):
        block.append(stored(a, mont))
        a = a * alpha % P_INT
    d_block = torch.from_numpy(limbs(block).copy().view(np.int64)).cuda()
    src = torch.empty((n + 2 * PAD, 4), dtype=torch.int64, device="cuda")
    src[PAD: PAD + n] = d_block.repeat(n // B, 1)
    garbage = torch.from_numpy(np.array([GARBAGE], dtype=np.uint64).view(np.int64)).cuda()
    src[:PAD] = garbage
    src[PAD + rows:] = garbage                                                # the five rows cut off, and the pad
    before = src.clone()
    sent = torch.from_numpy(np.array([SENT], dtype=np.uint64).view(np.int64)).cuda()
    dst = torch.empty((n + 2 * PAD, 4), dtype=torch.int64, device="cuda")
    dst[:] = sent
    call = lambda: cfg.ntt(log_n, stored(w, mont), [src.data_ptr() + 32 * PAD], out=[dst.data_ptr() + 32 * PAD], input_rows=[rows],   # noqa: E731
                           shift=stored(g, mont), scale=stored(c, mont))
    _, status, rep = call()
    print("ntt: log_n %d, launches %d, kernel %.3f ms, twiddles %.3f ms" % (log_n, rep["launches"], rep["kernel_ms"], rep["twiddle_ms"]))
    assert not status.any() and rep["launches"] == default_launches(log_n) and rep["written"] == n and rep["twiddle_ms"] > 0
    assert bool((dst[:PAD] == sent).all()) and bool((dst[PAD + n:] == sent).all()) and torch.equal(src, before)
    sample = sorted({0, 1, n // 2, n - 1} | set(np.random.default_rng(600 + log_n).choice(n, 1 << 16, replace=False).tolist()))
    picked = dst[PAD: PAD + n][torch.tensor(sample, dtype=torch.int64, device="cuda")]
    cells = ints(picked.cpu().numpy().view(np.uint64))
    tail = [pow(alpha, B - 5 + k, P_INT) for k in range(5)]
    for i, x in zip(sample, cells):
        assert x < P_INT
        z = g * pow(w, i, P_INT) % P_INT
        t = alpha * z % P_INT
        zb = pow(z, B, P_INT)
        zn = pow(zb, n // B, P_INT)
        den = (t - 1) * (zb - 1) % P_INT
        cut, zk = 0, zn                                                        # both sides times z^5: no inverse per row
        for k in range(5):
            cut = (cut + tail[k] * zk) % P_INT
            zk = zk * z % P_INT
        assert den != 0 and value(x, mont) * den * pow(z, 5, P_INT) % P_INT == c * ((pow(t, B, P_INT) - 1) * (zn - 1) * pow(z, 5, P_INT) - den * cut) % P_INT, i
    first = dst.clone()
    _, status, rep2 = call()                                                   # the same root again: the cached table, the same bytes
    assert rep2["twiddle_ms"] == 0 and rep2["twiddle_bytes"] == rep["twiddle_bytes"] == 32 * (n // 2)
    assert torch.equal(dst, first)
    cfg.close()
