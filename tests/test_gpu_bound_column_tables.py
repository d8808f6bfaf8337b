"""hsw_gadget_bind_column_tables on the MI355X: EVERY advice column of a region -- the FlexGate image columns, the
lookup-advice column and the dense / spread chip columns of every proof -- given one device pointer each.

The method is that of tests/test_gpu_bound_columns.py: all columns are carved out of one sentinel-filled tensor, the pass
runs over two different sentinels and a cell was written exactly if both passes agree on it, the expected mask and the
values come from an UNBOUND twin (itself checked against the oracle for single proofs), and the comparison is exact over
the whole tensor.

The lookup and chip columns are carved in an order no pitch can express: proof K-1's lookup column lowest and proof 0's
highest; then, the proofs interleaved, dense column 1 below spread column 0 below dense column 0 below spread column 1.
Neighbours are separated by pads of odd multiples of 4 cells (every column starts on a 128-byte line, the runs differ in
length), and every column holds the cells it needs + 12, so an overrun lands on a sentinel."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.test_gpu_bound_columns import PITCH, image_mask, interleaved, positions
from tests.test_gpu_bound_region import (HOST, MAX_ROWS, REPR, S1, S2, eng_int, interlude_after_digest0, make,  # noqa: F401
                                         oracle_single, run_twice, up4)

pytestmark = pytest.mark.gpu
PADS = [4, 28, 12, 52, 20, 36, 44]                            # odd multiples of 4 cells
CHIP_ORDER = [("dense", 1), ("spread", 0), ("dense", 0), ("spread", 1)]
SLACK = 12


class CarvedAll:
    """K x cols image columns of PITCH cells in the address order `order`, then K lookup columns of Lp + 12 cells (proof
    K-1 first) and 2 x K x 2 chip columns of rows + 12 cells in CHIP_ORDER with the proofs interleaved -- or, for a family
    that keeps the pitch model (lk_table / chip_table False), one area per proof as tests/test_gpu_bound_columns.py carves
    them.  .t stands in for Slabs.t (run_twice)."""

    def __init__(self, K, cols, order, Lp, rows, lk_table=True, chip_table=True):
        import torch
        self.K, self.cols, self.Lp, self.rows = K, cols, Lp, rows
        self.lk_table, self.chip_table = lk_table, chip_table
        self.start, self.lk, self.chip = {}, {}, {}
        at, i = 8, 0

        def carve(cells):
            nonlocal at, i
            at = up4(at + PADS[i % len(PADS)])
            i += 1
            s, at = at, at + cells
            return s
        for ck in order:
            self.start[ck] = carve(PITCH)
        self.lk_cap, self.chip_cap = Lp + SLACK, rows + SLACK
        self.lk_pitch = up4(self.lk_cap + 4)
        self.chip_stride = up4(self.chip_cap + 4)
        self.chip_ctx = 2 * self.chip_stride + 8
        if lk_table:
            for c in range(K - 1, -1, -1):
                self.lk[c] = carve(self.lk_cap)
        else:
            s = carve(K * self.lk_pitch)
            self.lk = {c: s + c * self.lk_pitch for c in range(K)}
        if chip_table:
            for fam, k in CHIP_ORDER:
                for c in range(K):
                    self.chip[(fam, c, k)] = carve(self.chip_cap)
        else:
            for fam in ("dense", "spread"):
                s = carve(K * self.chip_ctx)
                for c in range(K):
                    for k in range(2):
                        self.chip[(fam, c, k)] = s + c * self.chip_ctx + k * self.chip_stride
        self.total = at + 8
        self.t = torch.empty((self.total, 4), dtype=torch.int64, device="cuda")
        self.fill(S1)
        p = self.t.data_ptr()
        assert p % 128 == 0
        self.base = p
        self.ptrs = [p + 32 * self.start[(c, k)] for c in range(K) for k in range(cols)]
        self.kw = dict(column_ptrs=self.ptrs, column_pitch=PITCH, columns_capacity=cols, lookup_capacity=self.lk_cap,
                       chip_rows_capacity=self.chip_cap)
        if lk_table:
            self.kw.update(lookup_ptrs=[self.addr(self.lk[c]) for c in range(K)])
        else:
            self.kw.update(lookup=self.addr(self.lk[0]), lookup_pitch=self.lk_pitch)
        if chip_table:
            self.kw.update(chip_dense_ptrs=[self.addr(self.chip[("dense", c, k)]) for c in range(K) for k in range(2)],
                           chip_spread_ptrs=[self.addr(self.chip[("spread", c, k)]) for c in range(K) for k in range(2)])
        else:
            self.kw.update(chip_dense=self.addr(self.chip[("dense", 0, 0)]), chip_spread=self.addr(self.chip[("spread", 0, 0)]),
                           chip_col_stride=self.chip_stride, chip_context_pitch=self.chip_ctx)

    def addr(self, cell):
        return self.base + 32 * cell

    def fill(self, v):
        import torch
        self.t.fill_(v)
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(np.uint64)

    def poke(self, cell, value):
        import torch
        self.t[cell, 0] = value - (1 << 64) if value >= (1 << 63) else value
        torch.cuda.synchronize()

    def peek(self, cell):
        return int(self.t[cell, 0].item()) & ((1 << 64) - 1)


def test_the_carving_is_one_no_pitch_can_express():
    """The address order on paper (CarvedAll carves in exactly this order; check_pass asserts the reported pointers)."""
    order = [(fam, c, k) for fam, k in CHIP_ORDER for c in range(2)]
    at = {x: i for i, x in enumerate(order)}
    for c in range(2):
        assert at[("dense", c, 1)] < at[("spread", c, 0)] < at[("dense", c, 0)] < at[("spread", c, 1)]
    assert at[("dense", 1, 1)] < at[("spread", 0, 0)]        # proofs interleaved
    assert all((p // 4) % 2 == 1 and p % 4 == 0 for p in PADS)


def twin_lookup_mask(hsw, twin, K):
    """(K, Lp) mask of the lookup cells the unbound twin's own delivery touches."""
    N = hsw._native
    v = twin.view()
    Lp = int(twin.region_binding().lookup_capacity) if K > 1 else int(v.lookup_cells)
    look = np.full((K * Lp, 4), np.uint64(HOST), dtype=np.uint64)
    dst = N.RegionHost(None, look.ctypes.data, None, None)
    twin._ok(twin.lib.hsw_gadget_download_region(twin.h, C.byref(dst)))
    return (look[:, 0] != np.uint64(HOST)).reshape(K, Lp), Lp


def geometry(hsw, eng, kind, sizes, K, origin, mont, decl):
    """Lp and one proof's chip rows, from a fresh gadget of the kind."""
    probe = make(hsw, eng, kind, sizes, K, origin, mont, decl)
    b = probe.region_binding()
    out = int(probe.view().columns), int(b.lookup_capacity), int(b.chip_rows_capacity)
    probe.close()
    return out


def check_pass(hsw, eng, kind, sizes, K, origin, mont, msgs, perm, decl=None, split=None, oracle_ref=None, lk_table=True,
               chip_table=True):
    N = hsw._native
    columns, lp_need, rows_need = geometry(hsw, eng, kind, sizes, K, origin, mont, decl)
    twin = make(hsw, eng, kind, sizes, K, origin, mont, decl)
    cfg = make(hsw, eng, kind, sizes, K, origin, mont, decl)
    cv = CarvedAll(K, columns, interleaved(K, columns, perm), lp_need, rows_need, lk_table, chip_table)
    cfg.bind_columns(**cv.kw)
    # the reports: proof 0's pointers, pitches 0 for a family bound by table; proof c's through context_region
    b, v = cfg.region_binding(), cfg.view()
    assert int(b.d_columns) == cv.ptrs[0] and int(b.context_pitch) == 0 and int(b.column_pitch) == PITCH
    assert int(b.d_lookup) == cv.addr(cv.lk[0]) == int(v.d_lookup) and int(b.lookup_pitch) == (0 if lk_table else cv.lk_pitch)
    assert int(b.d_chip_dense) == cv.addr(cv.chip[("dense", 0, 0)]) == int(v.d_chip_dense)
    assert int(b.d_chip_spread) == cv.addr(cv.chip[("spread", 0, 0)]) == int(v.d_chip_spread)
    assert (int(b.chip_col_stride), int(b.chip_context_pitch)) == ((0, 0) if chip_table else (cv.chip_stride, cv.chip_ctx))
    if K > 1:
        for c in (0, K - 1):
            r = cfg.context_region(c)
            assert int(r.d_image) == cv.ptrs[c * columns] and int(r.d_lookup) == cv.addr(cv.lk[c])
            assert int(r.d_chip_dense) == cv.addr(cv.chip[("dense", c, 0)]) and int(r.d_chip_spread) == cv.addr(cv.chip[("spread", c, 0)])
    tres = twin.digest_batch(msgs)
    a, bb, res = run_twice(cfg, cv, msgs, split)
    assert [r.output_bytes for r in res] == [hashlib.sha256(m).digest() for m in msgs]
    for r, t in zip(res, tres):                              # positions, lookup cells included: an unbound twin's
        for cell in (r.prologue_cell, r.block_cell, r.block_cell + eng.G - 1, r.epilogue_cell, r.end_cell - 1):
            assert cfg.cell_position(cell) == twin.cell_position(cell)
        assert (r.prologue_cell, r.block_cell, r.end_cell, r.first_block) == (t.prologue_cell, t.block_cell, t.end_cell, t.first_block)
        if lk_table:
            assert (r.prologue_lookup, r.block_lookup, r.epilogue_lookup) == (t.prologue_lookup, t.block_lookup, t.epilogue_lookup)
    # the expected mask, from the twin
    tv = twin.view()
    C1 = int(tv.gate_cells) // K
    pos = positions(twin, (kind, tuple(sizes), K > 1, origin, tuple(decl or [])), C1)
    oc = int(tv.origin_column)
    assert pos[:, 1].max() < MAX_ROWS and (pos[:, 0] - oc).max() < columns
    lk, Lp = twin_lookup_mask(hsw, twin, K)
    rows = int(tv.num_limb_sum) // 2 // K
    assert Lp <= lp_need and rows == rows_need
    gate = np.zeros(cv.total, dtype=bool)
    exp = np.zeros(cv.total, dtype=bool)
    for c in range(K):
        starts = np.array([cv.start[(c, k)] for k in range(columns)], dtype=np.int64)
        gate[starts[pos[:, 0] - oc] + pos[:, 1]] = True
        exp[cv.lk[c]: cv.lk[c] + Lp] = lk[c]
        for fam in ("dense", "spread"):
            for k in range(2):
                exp[cv.chip[(fam, c, k)]: cv.chip[(fam, c, k)] + rows] = True
    assert int(gate.sum()) == C1 * K
    exp |= gate
    written = (a == bb).all(axis=1)
    print("written %d, expected %d (gate %d, lookup %d, chip %d)" % (int(written.sum()), int(exp.sum()), int(gate.sum()), int(lk.sum()), 4 * K * rows))
    diff = np.nonzero(written != exp)[0]
    assert len(diff) == 0, "cells written but not assigned, or assigned but not written: %s" % diff[:8].tolist()
    assert (bb[~written] == np.uint64(S2)).all()
    # the values: gathered through the caller's own pointers, equal to the twin's streams
    st, ts = cfg.streams(), twin.streams()
    gm = np.stack([image_mask(cv, gate, c, columns) for c in range(K)])
    gm = gm if K > 1 else gm[0]
    assert st["gate"].shape == ts["gate"].shape
    assert np.array_equal(st["gate"][gm], ts["gate"][gm]) and (st["gate"][~gm] == np.uint64(S2)).all() and not ts["gate"][~gm].any()
    assert np.array_equal(st["dense"], ts["dense"]) and np.array_equal(st["spread"], ts["spread"])
    lm = lk.reshape(-1)
    assert len(ts["lookup"]) == K * Lp and np.array_equal(st["lookup"][lm], ts["lookup"][lm]) and (st["lookup"][~lm][:, 0] == np.uint64(S2)).all()
    if oracle_ref is not None:
        img, mask, lookup, dense, spread = oracle_ref
        assert np.array_equal(mask, gm) and np.array_equal(st["gate"][mask], img[mask])
        assert np.array_equal(st["lookup"][origin[3]:], lookup)
        assert np.array_equal(st["dense"], dense[:, : st["rows"]]) and np.array_equal(st["spread"], spread[:, : st["rows"]])
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    # download_region: every host buffer of a table-bound family laid out as the unbound twin's, used rows only
    stride = int(tv.chip_col_stride)
    assert stride == K * rows
    hg = np.full((K * columns * MAX_ROWS, 4), np.uint64(HOST), dtype=np.uint64)
    hl = np.full((K * Lp, 4), np.uint64(HOST), dtype=np.uint64)
    hd = np.full((2 * stride, 4), np.uint64(HOST), dtype=np.uint64)
    hs = np.full((2 * stride, 4), np.uint64(HOST), dtype=np.uint64)
    dst = N.RegionHost(hg.ctypes.data, hl.ctypes.data if lk_table else None, hd.ctypes.data if chip_table else None,
                       hs.ctypes.data if chip_table else None)
    cfg._ok(cfg.lib.hsw_gadget_download_region(cfg.h, C.byref(dst)))
    hg = hg.reshape(ts["gate"].shape)
    assert np.array_equal(hg[gm], ts["gate"][gm]) and (hg[~gm] == np.uint64(HOST)).all()
    if lk_table:
        assert np.array_equal(hl[lm], ts["lookup"][lm]) and (hl[~lm] == np.uint64(HOST)).all()
    if chip_table:
        assert np.array_equal(hd.reshape(2, stride, 4), ts["dense"]) and np.array_equal(hs.reshape(2, stride, 4), ts["spread"])
    tape = N.RegionTape()
    cfg._ok(cfg.lib.hsw_gadget_region_tape(cfg.h, C.byref(tape)))
    n = C.c_size_t()
    one = np.zeros((1, 4), dtype=np.uint64)
    for rc in (cfg.lib.hsw_gadget_download_region_distinct(cfg.h, one.ctypes.data, 1, C.byref(n)),
               cfg.lib.hsw_gadget_replay_region(cfg.h, one.ctypes.data, C.byref(dst), 1)):
        assert rc == N.HSW_ERR_UNSUPPORTED
    for call in (lambda: cfg.seek(0), lambda: cfg.download_region_compact()):
        with pytest.raises(hsw.HswError) as ei:
            call()
        assert ei.value.status == N.HSW_ERR_UNSUPPORTED
    return cfg, twin, cv, bb, res


def reset_and_unbind(cfg, twin, cv, last, msgs):
    """9: after a reset the same bytes are written again; unbound, the gadget equals the twin and the caller's tensor is
    untouched."""
    cfg.reset()
    cfg.digest_batch(msgs)
    assert np.array_equal(cv.host(), last)
    cfg.reset()
    cfg.bind_region(None)
    v = cfg.view()
    assert int(v.d_gate) not in cv.ptrs and int(v.d_lookup) != cv.addr(cv.lk[0]) and int(v.d_chip_dense) != cv.addr(cv.chip[("dense", 0, 0)])
    cfg.digest_batch(msgs)
    st, ts = cfg.streams(), twin.streams()
    for k in ("gate", "lookup", "dense", "spread"):
        assert np.array_equal(st[k], ts[k]), k
    assert cfg.verify()["violations"] == 0
    assert np.array_equal(cv.host(), last)


def proof_parity(hsw, oracle, eng, cfg, msgs, K, origin, mont):
    """The first and last proof, read through their own pointers, equal a single-proof gadget's and the oracle's lookup,
    dense and spread columns (and image)."""
    st = cfg.streams()
    rows = st["rows"] // K
    Lp = len(st["lookup"]) // K
    for c in (0, K - 1):
        img, mask, lookup, dense, spread = oracle_single(oracle, [msgs[c]], [1024], origin, mont)
        one = make(hsw, eng, "single", [1024], 1, origin, mont)
        one.digest(msgs[c])
        so = one.streams()
        assert np.array_equal(st["gate"][c][mask], img[mask]) and np.array_equal(st["gate"][c][mask], so["gate"][mask])
        assert np.array_equal(st["lookup"][c * Lp + origin[3]: (c + 1) * Lp], lookup) and np.array_equal(so["lookup"][origin[3]:], lookup)
        for fam, ref in (("dense", dense), ("spread", spread)):
            assert np.array_equal(st[fam][:, c * rows: (c + 1) * rows], ref[:, :rows])
            assert np.array_equal(so[fam][:, :rows], ref[:, :rows])
        one.close()


def poke_chip_and_lookup(cfg, cv, res, K):
    """8: one dense chip cell and one lookup cell of the LAST proof flipped at their table addresses: verify() reports
    them; restored, it is clean again."""
    per = len(res) // K
    r = res[(K - 1) * per]
    chip_row = 1000
    at = cv.chip[("dense", K - 1, 1)] + chip_row               # limb call 2 * chip_row + 1 of the proof
    old = cv.peek(at)
    cv.poke(at, old ^ 1)
    rep = cfg.verify()
    print("chip poke:", rep)
    assert rep["violations"] > 0 and rep["first_class"] == "chip" and rep["first_block"] == r.first_block + (2 * chip_row + 1) // 4120, rep
    cv.poke(at, old)
    assert cfg.verify()["violations"] == 0
    at = cv.lk[K - 1] + (r.block_lookup - (K - 1) * (cv.Lp if K > 1 else 0)) + 7   # entry 7 of the proof's first block
    old = cv.peek(at)
    cv.poke(at, old ^ 1)
    rep = cfg.verify()
    print("lookup poke:", rep)
    assert rep["violations"] > 0 and rep["first_class"] == "lookup" and rep["first_block"] == r.first_block, rep
    cv.poke(at, old)
    assert cfg.verify()["violations"] == 0


@REPR
def test_single_proof_test_circuit_every_column_by_pointer(hsw, oracle, eng_int, mont):
    """1: sizes [128, 128], b"abc" and b"", origin (0, 17): the small-batch wide kernel, against the oracle; 9: round trips."""
    msgs, sizes, origin = [b"abc", b""], [128, 128], (0, 17, False, 0)
    ref = oracle_single(oracle, msgs, sizes, origin, mont)
    cfg, twin, cv, last, res = check_pass(hsw, eng_int, "single", sizes, 1, origin, mont, msgs, [2, 0, 1], oracle_ref=ref)
    assert eng_int.last_launch()["kernel"] == "hsw::hsw_small_table_kernel<2, %d, true>" % (1 if mont else 0)
    poke_chip_and_lookup(cfg, cv, res, 1)
    reset_and_unbind(cfg, twin, cv, last, msgs)
    cfg.close()
    twin.close()


@REPR
@pytest.mark.parametrize("K", [2, 9], ids=["K2_small_batch_kernel_scatter_chip", "K9_streaming_kernel_flush_chip"])
def test_k_bench_circuits_every_column_by_pointer(hsw, oracle, eng_int, K, mont):
    """2 + 3 (+ 8, 9): K bench circuits as context images: 32 blocks on hsw_small_table_kernel<.., true> (scatter_chip), 144
    on hsw_expand_table_kernel<.., true> (flush_chip)."""
    origin = (0, 0, False, 3)
    msgs = [bytes([h + 1] * 56) for h in range(K)]
    cfg, twin, cv, last, res = check_pass(hsw, eng_int, "images", [1024], K, origin, mont, msgs, list(range(8, -1, -1)))
    kernel = eng_int.last_launch()["kernel"]
    assert kernel.startswith("hsw::hsw_small_table_kernel<" if K == 2 else "hsw::hsw_expand_table_kernel<") and kernel.endswith(", true>"), kernel
    proof_parity(hsw, oracle, eng_int, cfg, msgs, K, origin, mont)
    poke_chip_and_lookup(cfg, cv, res, K)
    reset_and_unbind(cfg, twin, cv, last, msgs)
    cfg.close()
    twin.close()


@REPR
def test_context_group_split_inside_a_context_every_column_by_pointer(hsw, eng_int, mont):
    """4: K = 3 x [192, 64] with an interlude: one batch and a batch split inside Context 1 write identical bytes -- a launch
    whose first block is not its Context's first still finds the Context's chip rows and lookup offset."""
    K, sizes, origin = 3, [192, 64], (1, 777, False, 5)
    decl = interlude_after_digest0(hsw, eng_int, sizes, origin)
    msgs = [bytes([7 + i] * (20 + 5 * i)) for i in range(2 * K)]
    cols = geometry(hsw, eng_int, "group", sizes, K, origin, mont, decl)[0]
    perm = list(range(cols - 1, -1, -1))
    cfg, twin, cv, one_batch, res = check_pass(hsw, eng_int, "group", sizes, K, origin, mont, msgs, perm, decl=decl)
    poke_chip_and_lookup(cfg, cv, res, K)
    cfg2, twin2, cv2, split_batch, _ = check_pass(hsw, eng_int, "group", sizes, K, origin, mont, msgs, perm, decl=decl, split=3)
    assert cv2.start == cv.start and cv2.lk == cv.lk and cv2.chip == cv.chip and np.array_equal(split_batch, one_batch)
    for x in (cfg, twin, cfg2, twin2):
        x.close()


@REPR
def test_shared_context_beyond_17_columns_every_column_by_pointer(hsw, eng_int, mont):
    """5: ONE Context with two digests and an interlude that spans columns (more than 17 columns): the chip rows of digest 1
    follow digest 0's in the same allocations."""
    sizes, origin = [1024, 1024], (1, 777, False, 5)
    decl = interlude_after_digest0(hsw, eng_int, sizes, origin)
    msgs = [b"a" * 700, b"b" * 100]
    cols = geometry(hsw, eng_int, "shared", sizes, 1, origin, mont, decl)[0]
    assert cols > 17
    cfg, twin, cv, last, _ = check_pass(hsw, eng_int, "shared", sizes, 1, origin, mont, msgs, list(range(cols - 1, -1, -1)), decl=decl)
    reset_and_unbind(cfg, twin, cv, last, msgs)
    cfg.close()
    twin.close()


def test_three_chip_columns_context_images_are_refused_at_creation(hsw):
    """6: 4,120 limb calls per block is no multiple of 3, so the chip columns of one proof of [128] would end on different
    rows and the next proof would not start on a row of its own: the whole-digest gadget refuses K context images with 3
    chip columns when it is created (HSW_ERR_UNSUPPORTED), today as before -- there is nothing to bind."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    N = hsw._native
    eng3 = hsw.WitnessEngine(0, 8, 3, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        assert (2 * 4120) % 3 != 0
        with pytest.raises(hsw.HswError) as ei:
            hsw.Sha256DynamicConfig(eng3, [128] * 2, True, whole_digest=True, independent=True, context_images=True)
        assert ei.value.status == N.HSW_ERR_UNSUPPORTED
    finally:
        eng3.close()


@REPR
@pytest.mark.parametrize("family", ["lookup_by_table_chips_by_pitch", "chips_by_table_lookup_by_pitch"])
def test_mixed_families(hsw, eng_int, family, mont):
    """7: K = 2 x [128]: one family by pointer table, the other at the pitches of hsw_region_binding."""
    K, origin = 2, (0, 5, False, 2)
    msgs = [b"abc", b"x" * 100]
    lk_table = family.startswith("lookup")
    cols = geometry(hsw, eng_int, "images", [128], K, origin, mont, None)[0]
    cfg, twin, cv, last, _ = check_pass(hsw, eng_int, "images", [128], K, origin, mont, msgs, list(range(cols - 1, -1, -1)),
                                        lk_table=lk_table, chip_table=not lk_table)
    reset_and_unbind(cfg, twin, cv, last, msgs)
    cfg.close()
    twin.close()
