"""hsw_gadget_msm on the MI355X: the commitments of device columns, the BN254 G1 MSM of hsw_msm.hip.

The yardstick is Python integers: tests/msm_model.py, affine chord-and-tangent arithmetic over bases with known discrete
logs, proven in tests/test_msm_host.py against the term-by-term definition.  Every output point is compared with it byte
for byte, in both cell forms.  The bases and all columns are carved out of ONE device buffer with sentinel cells around
each; after the call the WHOLE buffer must be what it was.  out_points is pre-filled with a sentinel.  Rows of a column
at and beyond input_rows hold limbs far above r and bases at and beyond max input_rows coordinates far above q: a read of
either shows as a refusal or as a wrong point."""
import ctypes as C

import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.msm_model import Q_INT, add, cell_words, chain, commitment, neg, plan, point_words, words_point
from tests.test_gpu_bound_region import REPR, make
from tests.test_gpu_lookup_counts import ORIGIN
from tests.test_gpu_lookup_permuted import SENT

pytestmark = pytest.mark.gpu
PAD = 3                                     # sentinel cells before and after the bases and every column
GARBAGE = (1 << 64) - 2                     # every limb of a cell or base that must not be read: far above r and q
NONE = (1 << 64) - 1
OUT_SENT = 0xA5A5A5A5A5A5A5A5               # what out_points holds before the call
_CHAINS = {}


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


def chains(n):
    """n bases in several chains of known logs, computed once and shared: ([point], [log])"""
    size = 1024 if n <= 1024 else 1 << 16
    if size not in _CHAINS:
        import random
        rng = random.Random(77)
        cuts = [0, 200, 700, 1024] if size == 1024 else [0, 200, 1024, 20000, size]
        pts, logs = [], []
        for lo, hi in zip(cuts, cuts[1:]):
            p, k = chain(rng.randrange(1, P_INT), rng.randrange(1, P_INT), hi - lo)
            pts += p
            logs += k
        _CHAINS[size] = (pts, logs)
    pts, logs = _CHAINS[size]
    return list(pts[:n]), list(logs[:n])


class Case:
    """One call's bases and columns in one device buffer.  heights[b]: input_rows of column b; scalars[b]: its values
    (integers below r) -- None for a column that reads the input of column reads[b]."""

    def __init__(self, cfg, hsw, mont, points, logs, heights, scalars, reads=None):
        import torch
        self.cfg, self.N, self.mont = cfg, hsw._native, mont
        self.points, self.logs, self.heights, self.scalars = points, logs, list(heights), scalars
        self.n, self.n_bases = len(heights), len(points)
        self.reads = list(reads) if reads is not None else list(range(self.n))
        self.checked = max(self.heights)
        self.at, at = {}, PAD
        self.at["bases"] = at
        at += 2 * self.n_bases + 2 * PAD
        for b in range(self.n):
            if self.reads[b] == b:
                self.at[b] = at
                at += self.n_bases + 2 * PAD
        host = np.full((at, 4), np.uint64(SENT), dtype=np.uint64)
        s = self.at["bases"]
        host[s: s + 2 * self.n_bases] = np.uint64(GARBAGE)
        if self.checked:
            host[s: s + 2 * self.checked] = np.array([point_words(p) for p in points[:self.checked]], dtype=np.uint64).reshape(-1, 4)
        for b in range(self.n):
            if self.reads[b] != b:
                continue
            s, h = self.at[b], max(self.heights[c] for c in range(self.n) if self.reads[c] == b)
            host[s: s + self.n_bases] = np.uint64(GARBAGE)
            if h:
                host[s: s + h] = np.array([cell_words(x, mont) for x in scalars[b][:h]], dtype=np.uint64)
        self.buf = torch.from_numpy(host.view(np.int64)).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 16 == 0

    def poke(self, cell, words):
        """store 4 uint64 words at cell `cell` of the buffer"""
        import torch
        self.buf[cell] = torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).cuda()
        torch.cuda.synchronize()

    def expected(self, b):
        return commitment(self.scalars[self.reads[b]][:self.heights[b]], self.logs)

    def call(self, window_bits=0, slice_rows=0, **over):
        """the raw call: (rc, out bytes (n, 8) uint64, status, report); the buffer must be unchanged whatever it returns"""
        import torch
        N, n = self.N, self.n
        before = self.buf.cpu().numpy().view(np.uint64).copy()
        out = np.full((n, 8), np.uint64(OUT_SENT), dtype=np.uint64)
        status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        ptrs = (C.c_void_p * n)(*[self.base + 32 * self.at[self.reads[b]] for b in range(n)])
        hs = (C.c_uint64 * n)(*self.heights) if self.heights != [self.n_bases] * n else None
        kw = dict(flags=0, window_bits=window_bits, slice_rows=slice_rows, reserved_=0, n_columns=n, n_bases=self.n_bases,
                  d_bases=self.base + 32 * self.at["bases"], d_scalars=ptrs, input_rows=hs, out_points=out.ctypes.data,
                  status=status.ctypes.data_as(C.POINTER(C.c_uint32)))
        kw.update(over)
        args = N.Msm(**kw)
        rep = N.MsmReport()
        torch.cuda.synchronize()
        rc = self.cfg.lib.hsw_gadget_msm(self.cfg.h, C.byref(args), C.byref(rep))
        after = self.buf.cpu().numpy().view(np.uint64)
        assert np.array_equal(before, after), "device memory of the caller was written"
        return rc, out, status, {f[0]: getattr(rep, f[0]) for f in N.MsmReport._fields_}

    def run(self, window_bits=0, slice_rows=0, refused=(), bad_bases=0, groups=1, held=None):
        """the call, then every check that holds for any outcome.  groups: the groups of columns the call is to take;
        held: the columns whose partial buckets the scratch is to hold (under the default budget: as many as fit 1 GiB)"""
        N = self.N
        rc, out, status, report = self.call(window_bits, slice_rows)
        assert rc == N.HSW_OK, self.cfg.lib.hsw_last_error(self.cfg.engine.h)
        print("msm: bases %d, columns %d, window_bits %d (%d windows), slice_rows %d (%d slices), launches %d, kernel %.3f ms, finish %.3f ms, "
              "scratch %d bytes, status %s" % (self.n_bases, self.n, report["window_bits"], report["windows"], report["slice_rows"], report["slices"],
                                             report["launches"], report["kernel_ms"], report["finish_ms"], report["scratch_bytes"], status.tolist()))
        c, W, s, slices = plan(self.checked, window_bits, slice_rows)
        assert (report["window_bits"], report["windows"], report["slice_rows"], report["slices"]) == (c, W, s, slices)
        assert report["launches"] == (1 if self.checked else 0) + 2 * groups and report["columns"] == self.n
        if held is None:
            held = min(self.n, max(1, (1 << 30) // (W * slices * ((1 << c) - 1) * 96)))
        assert report["scratch_bytes"] == held * W * slices * ((1 << c) - 1) * 96
        if bad_bases:
            assert report["bad_bases"] == bad_bases[0] and report["first_bad_base"] == bad_bases[1]
            assert (status == N.HSW_MSM_BASE_NOT_BELOW_Q).all() and (out == np.uint64(OUT_SENT)).all()
            assert report["refused_columns"] == self.n and report["first_refused"] == 0
            return out, status, report
        assert report["bad_bases"] == 0 and report["first_bad_base"] == NONE
        for b in range(self.n):
            if b in refused:
                assert status[b] == N.HSW_MSM_CELL_NOT_BELOW_P and (out[b] == np.uint64(OUT_SENT)).all(), (b, status[b])
            else:
                assert status[b] == 0, (b, status[b])
                assert out[b].tolist() == point_words(self.expected(b)), "column %d: a wrong point" % b
        assert report["refused_columns"] == len(refused) and report["first_refused"] == (min(refused) if refused else NONE)
        return out, status, report


def random_scalars(seed, n):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % P_INT for _ in range(n)]


# ---- 1. every window width ------------------------------------------------------------------------------------------------
@REPR
@pytest.mark.parametrize("window_bits", [1, 3, 5, 8, 0])                      # (8 is the maximum; 5: a short top window)
def test_every_window_width(hsw, eng_int, window_bits, mont):
    cfg = gadget(hsw, eng_int, mont)
    pts, logs = chains(300)
    case = Case(cfg, hsw, mont, pts, logs, [300, 299, 1], [random_scalars(10 + b, 300) for b in range(3)])
    assert hsw._native.HSW_MSM_MAX_WINDOW_BITS == 8
    case.run(window_bits, 64)                                                # 5 slices, the last one short
    cfg.close()


# ---- 2. boundaries --------------------------------------------------------------------------------------------------------
@REPR
def test_heights_at_the_slice_boundaries_and_a_shared_input(hsw, eng_int, mont):
    cfg = gadget(hsw, eng_int, mont)
    pts, logs = chains(1024)
    heights = [0, 1, 63, 64, 65, 1000, 700]
    scal = [random_scalars(20 + b, 1024) for b in range(6)] + [None]
    case = Case(cfg, hsw, mont, pts, logs, heights, scal, reads=[0, 1, 2, 3, 4, 5, 5])   # the last two read one input
    out, _, _ = case.run(8, 64)
    assert not out[0].any()                                                  # no rows: the identity, 64 zero bytes
    case.run(4, 128)
    cfg.close()


# ---- 3. edge values -------------------------------------------------------------------------------------------------------
@REPR
def test_edge_scalars_and_bases(hsw, eng_int, mont):
    cfg = gadget(hsw, eng_int, mont)
    pts, logs = chains(300)
    pts[7], logs[7] = None, None                                             # (0, 0) bases under non-zero scalars
    pts[130], logs[130] = None, None
    pts[21], logs[21] = pts[20], logs[20]                                    # duplicates under different scalars: a bucket doubles
    pts[90], logs[90] = pts[20], logs[20]
    pts[41], logs[41] = neg(pts[40]), (P_INT - logs[40]) % P_INT             # a negated pair
    edge = [0, 1, P_INT - 1, 2, 1 << 64, 1 << 128, 1 << 253, int("01" * 32, 16) % P_INT, int("11" * 31, 16), 255, 256]
    col0 = random_scalars(30, 300)
    col0[:len(edge)] = edge
    col0[20], col0[21], col0[90] = 5, 5 + 256, 5 + 65536                     # one bucket of window 0, thrice the same point
    col0[40] = col0[41]
    col1 = [0x37] * 300                                                      # one value throughout: every row in one bucket
    col2 = [0] * 300                                                         # the negated pair under equal scalars, alone
    col2[40] = col2[41] = 0xABCDEF0123456789ABCDEF
    col3 = [0] * 300                                                         # nothing at all
    col4 = [0] * 300
    col4[7] = col4[130] = 12345                                              # identity bases only
    case = Case(cfg, hsw, mont, pts, logs, [300] * 5, [col0, col1, col2, col3, col4])
    for window_bits, slice_rows in ((8, 64), (0, 0), (2, 256)):
        out, _, _ = case.run(window_bits, slice_rows)
        assert not out[2].any() and not out[3].any() and not out[4].any()    # the identity: 64 zero bytes
    cfg.close()


# ---- 4. refusals on the device ----------------------------------------------------------------------------------------------
@REPR
def test_a_cell_not_below_r_refuses_its_column_alone(hsw, eng_int, mont):
    cfg = gadget(hsw, eng_int, mont)
    pts, logs = chains(300)
    case = Case(cfg, hsw, mont, pts, logs, [300, 300, 200], [random_scalars(40 + b, 300) for b in range(3)])
    case.poke(case.at[1] + 17, cell_words(P_INT, False))                     # a cell equal to r
    case.poke(case.at[1] + 299, [5, 0, 0, 1 << 63])                          # ... and one with a high limb set
    case.run(8, 64, refused=(1,))
    case.run(0, 0, refused=(1,))
    cfg.close()


@REPR
def test_a_base_not_below_q_refuses_everything_inside_the_checked_rows_only(hsw, eng_int, mont):
    cfg = gadget(hsw, eng_int, mont)
    pts, logs = chains(300)
    q_words = [(Q_INT >> (64 * i)) & NONE for i in range(4)]
    good = point_words(pts[150])
    case = Case(cfg, hsw, mont, pts, logs, [200, 100, 3], [random_scalars(50 + b, 300) for b in range(3)])
    base = case.at["bases"]
    case.poke(base + 2 * 150 + 1, q_words)                                   # y of base 150 equal to q: inside rows [0, 200)
    case.run(8, 64, bad_bases=(1, 150))
    case.poke(base + 2 * 40, q_words)                                        # x of base 40 too: two, the first one is 40
    case.run(0, 0, bad_bases=(2, 40))
    case.poke(base + 2 * 150 + 1, good[4:])
    case.poke(base + 2 * 40, point_words(pts[40])[:4])
    case.run(8, 64)
    # the same base beyond the checked rows: not read (those rows hold coordinates far above q anyway)
    case.poke(base + 2 * 250 + 1, q_words)
    case.run(8, 64)
    cfg.close()


# ---- 4b. groups of columns: the engine option "round_scratch" lowers the 1 GiB a group's partial buckets may take ------------
# (the other limit of a group, 65,535 columns in a grid dimension, cannot be the one that cuts: at one bucket per window a
# column still takes 254 x 96 = 24 KB of partial buckets, and 65,535 of them are above 1 GiB)
@REPR
def test_groups_of_columns_under_a_scratch_budget(hsw, eng_int, mont):
    """300 bases, window_bits 8, slice_rows 64: 5 slices x 32 windows x 255 buckets x 96 bytes a column.  Six columns of
    heights 300, 65, 300, 0, 1, 299 -- in groups of two, the one-row column takes the slot the second 300-row column left
    full of slices, and the 299-row one the slot of the empty column.  Every group has its own offset into the columns,
    the status words and the window points."""
    cfg = gadget(hsw, eng_int, mont)
    pts, logs = chains(300)
    column = 5 * 32 * 255 * 96
    scal = [random_scalars(45 + b, 300) for b in range(5)] + [None]
    case = Case(cfg, hsw, mont, pts, logs, [300, 65, 300, 0, 1, 299], scal, reads=[0, 1, 2, 3, 4, 0])   # the last reads column 0's input
    whole, _, _ = case.run(8, 64)                                            # one group
    try:
        for budget, groups, held in ((2 * column, 3, 2), (2 * column - 1, 6, 1), (1, 6, 1)):
            eng_int.set_option("round_scratch", budget)
            out, status, _ = case.run(8, 64, groups=groups, held=held)
            assert np.array_equal(out, whole) and not status.any()
        assert words_point(out[4]) == commitment(scal[4][:1], logs)          # the one-row column: its scalar times base 0
        # a cell equal to r in column 2, the first column of the second group (the third of six)
        case.poke(case.at[2] + 17, cell_words(P_INT, False))
        for budget, groups, held in ((2 * column, 3, 2), (1, 6, 1)):
            eng_int.set_option("round_scratch", budget)
            out, status, report = case.run(8, 64, refused=(2,), groups=groups, held=held)
            assert status.tolist() == [0, 0, 4, 0, 0, 0] and report["first_refused"] == 2 and report["refused_columns"] == 1
            assert (out[2] == np.uint64(OUT_SENT)).all() and np.array_equal(np.delete(out, 2, 0), np.delete(whole, 2, 0))
    finally:
        eng_int.set_option("round_scratch", 1 << 30)
    out, _, _ = case.run(8, 64, refused=(2,))                                # the option is back: one group again
    assert np.array_equal(np.delete(out, 2, 0), np.delete(whole, 2, 0))
    cfg.close()


# ---- 5. refusals on the host ------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(hsw, eng_int):
    N = hsw._native
    cfg = gadget(hsw, eng_int, False)
    pts, logs = chains(300)
    case = Case(cfg, hsw, False, pts, logs, [300, 100], [random_scalars(60 + b, 300) for b in range(2)])
    base = case.base + 32 * case.at["bases"]
    cols = [case.base + 32 * case.at[b] for b in range(2)]
    ptr = lambda *a: (C.c_void_p * len(a))(*a)                               # noqa: E731
    rows = lambda *a: (C.c_uint64 * len(a))(*a)                              # noqa: E731
    invalid = [dict(n_columns=0), dict(n_bases=0), dict(n_bases=(1 << 28) + 1), dict(flags=1), dict(d_bases=None), dict(d_bases=base + 8),
               dict(d_scalars=None), dict(d_scalars=ptr(cols[0], None)), dict(d_scalars=ptr(cols[0], cols[1] + 8)), dict(out_points=None),
               dict(input_rows=rows(300, 301)), dict(window_bits=9), dict(slice_rows=32), dict(slice_rows=96), dict(slice_rows=1 << 29)]
    for over in invalid:
        rc, out, status, report = case.call(**dict(dict(window_bits=8, slice_rows=64), **over))
        assert rc == N.HSW_ERR_INVALID_ARG, over
        assert (out == np.uint64(OUT_SENT)).all() and (status == 0xFFFFFFFF).all() and report["launches"] == 0, over
    rc, _, _, _ = case.call(8, 64, d_scalars=ptr(cols[0], cols[1] + 8))
    assert rc == N.HSW_ERR_INVALID_ARG and b"column 1" in cfg.lib.hsw_last_error(eng_int.h)
    case.run(8, 64)                                                          # and the gadget is as good as before
    cfg.close()
    # a pass whose batches differ in representation
    cfg = make(hsw, eng_int, "images", [64], 2, ORIGIN, False)
    case = Case(cfg, hsw, False, pts, logs, [300], [random_scalars(70, 300)])
    cfg.digest(b"abc")
    case.run(8, 64)                                                          # one batch so far: canonical
    cfg.set_repr(N.HSW_REPR_MONTGOMERY)
    cfg.digest(b"def")
    rc, out, status, _ = case.call(8, 64)
    assert rc == N.HSW_ERR_UNSUPPORTED and b"differ in representation" in cfg.lib.hsw_last_error(eng_int.h)
    assert (out == np.uint64(OUT_SENT)).all() and (status == 0xFFFFFFFF).all()
    cfg.close()
    # 8-byte cells
    plain = hsw.WitnessEngine(0, 8, 2)
    try:
        g = hsw.Sha256DynamicConfig(plain, [128], is_input_range_check=False)
        g.set_repr(N.HSW_REPR_COMPACT64)
        case = Case(g, hsw, False, pts, logs, [300], [random_scalars(71, 300)])
        rc, out, status, _ = case.call(8, 64)
        assert rc == N.HSW_ERR_UNSUPPORTED and b"32-byte" in g.lib.hsw_last_error(plain.h)
        assert (out == np.uint64(OUT_SENT)).all() and (status == 0xFFFFFFFF).all()
        g.close()
    finally:
        plain.close()


# ---- 6. the library's own plan ------------------------------------------------------------------------------------------------
@REPR
def test_the_librarys_own_plan_and_linearity(hsw, eng_int, mont):
    import torch
    cfg = gadget(hsw, eng_int, mont)
    n = 1 << 16
    pts, logs = chains(n)
    rng = np.random.default_rng(99)
    uniform = random_scalars(80, n)
    kinds = rng.integers(0, 4, n)                                            # witness-like: bits, bytes, zero runs, a few full values
    witness = [int(rng.integers(0, 2)) if k == 0 else int(rng.integers(0, 256)) if k == 1 else 0 for k in kinds]
    witness[1000:9000] = [0] * 8000
    witness[30000:30064] = uniform[:64]
    both = [(a + b) % P_INT for a, b in zip(uniform, witness)]
    case = Case(cfg, hsw, mont, pts, logs, [n, n, n], [uniform, witness, both])
    out, _, report = case.run()                                              # all knobs 0
    assert (report["window_bits"], report["windows"], report["slice_rows"], report["slices"], report["launches"]) == (8, 32, 4096, 16, 3)
    assert words_point(out[2]) == add(words_point(out[0]), words_point(out[1]))
    # the wrapper, over the same memory: tensors carved out of the buffer
    cells = case.buf.view(torch.uint64)
    bases = cells[case.at["bases"]: case.at["bases"] + 2 * n].view(n, 8)
    columns = [case.base + 32 * case.at[b] for b in range(3)]
    points, status, rep = cfg.msm(bases, columns)
    assert np.array_equal(points, out) and not status.any() and rep["slices"] == 16
    cfg.close()
