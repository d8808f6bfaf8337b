"""hsw_gadget_bind_columns on the MI355X: the FlexGate image columns of a region given ONE device pointer each.

The columns are carved out of one sentinel-filled tensor, so that the test sees every byte around them: each column
holds MAX_ROWS + 12 cells, columns are separated by odd-looking pads (multiples of 4 cells, the next column then starts
on the next 128-byte line, which the entry point requires), the address order is a fixed permutation of the column
order with a descending neighbour pair inside every proof (the case a 32-bit gap gets wrong), and proofs are
interleaved.  The lookup and chip areas keep the pitch model, one set per proof behind the columns.

"Written" is decided as in tests/test_gpu_bound_region.py: the pass runs over two different sentinels, and a cell was
written exactly if both passes agree on it.  Where cells should be follows from an UNBOUND twin's positions."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.test_gpu_bound_region import (HOST, MAX_ROWS, REPR, S1, S2, eng_int, interlude_after_digest0, make,  # noqa: F401
                                         oracle_single, run_twice, up4)

pytestmark = pytest.mark.gpu
PITCH = MAX_ROWS + 12
PADS = [4, 28, 12, 52, 8, 36, 20]                             # cells between two carved columns, before aligning up


class Carved:
    """K x cols columns of PITCH cells in one tensor, in the address order `order` (a list of (proof, column)), then per
    proof [lookup | 2 dense | 2 spread] of PITCH cells each; every cell a sentinel.  .t stands in for Slabs.t (run_twice)."""

    def __init__(self, K, cols, order):
        import torch
        assert sorted(order) == [(c, k) for c in range(K) for k in range(cols)]
        self.K, self.cols, self.pitch = K, cols, PITCH
        self.start, at = {}, 8
        for i, ck in enumerate(order):
            at = up4(at + PADS[i % len(PADS)])
            self.start[ck] = at
            at += PITCH
        self.o_lk = up4(at + 4)
        self.area = up4(PITCH)
        self.per_proof = 5 * self.area
        self.total = self.o_lk + K * self.per_proof + 8
        self.t = torch.empty((self.total, 4), dtype=torch.int64, device="cuda")
        self.fill(S1)
        p = self.t.data_ptr()
        assert p % 128 == 0
        self.ptrs = [p + 32 * self.start[(c, k)] for c in range(K) for k in range(cols)]
        self.kw = dict(column_ptrs=self.ptrs, column_pitch=PITCH, columns_capacity=cols,
                       lookup=p + 32 * self.o_lk, lookup_capacity=PITCH, lookup_pitch=self.per_proof,
                       chip_dense=p + 32 * (self.o_lk + self.area), chip_spread=p + 32 * (self.o_lk + 3 * self.area),
                       chip_col_stride=self.area, chip_rows_capacity=PITCH, chip_context_pitch=self.per_proof)

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


def interleaved(K, cols, perm):
    """Address order: columns in the order `perm`, the proofs interleaved column by column."""
    return [(c, k) for k in perm for c in range(K)]


_POS = {}


def positions(twin, key, n):
    if key not in _POS:
        _POS[key] = np.array([twin.cell_position(i) for i in range(n)], dtype=np.int64)
    return _POS[key]


def expected_mask(hsw, twin, cv, key):
    """The cells of the carved tensor the layout assigns, from the UNBOUND twin after its pass."""
    N = hsw._native
    v, K = twin.view(), cv.K
    exp = np.zeros(cv.total, dtype=bool)
    C1 = int(v.gate_cells) // K
    pos = positions(twin, key, C1)
    oc = int(v.origin_column)
    assert pos[:, 1].max() < MAX_ROWS and (pos[:, 0] - oc).max() < cv.cols
    Lp = int(twin.region_binding().lookup_capacity) if K > 1 else int(v.lookup_cells)
    look = np.full((K * Lp, 4), np.uint64(HOST), dtype=np.uint64)
    dst = N.RegionHost(None, look.ctypes.data, None, None)
    twin._ok(twin.lib.hsw_gadget_download_region(twin.h, C.byref(dst)))
    lk = (look[:, 0] != np.uint64(HOST)).reshape(K, Lp)
    rows = int(v.num_limb_sum) // 2 // K
    gate = np.zeros(cv.total, dtype=bool)
    for c in range(K):
        starts = np.array([cv.start[(c, k)] for k in range(cv.cols)], dtype=np.int64)
        gate[starts[pos[:, 0] - oc] + pos[:, 1]] = True
        base = cv.o_lk + c * cv.per_proof
        exp[base: base + Lp] = lk[c]
        for o in (1, 3):
            for k in range(2):
                exp[base + (o + k) * cv.area: base + (o + k) * cv.area + rows] = True
    assert int(gate.sum()) == C1 * K
    return exp | gate, gate


def image_mask(cv, gate, c, columns):
    """(columns, MAX_ROWS) mask of proof c's assigned image cells."""
    return np.stack([gate[cv.start[(c, k)]: cv.start[(c, k)] + MAX_ROWS] for k in range(columns)])


def check_pass(hsw, eng, kind, sizes, K, origin, mont, msgs, perm, decl=None, split=None, oracle_ref=None, cols=None):
    N = hsw._native
    twin = make(hsw, eng, kind, sizes, K, origin, mont, decl)
    cfg = make(hsw, eng, kind, sizes, K, origin, mont, decl)
    columns = int(cfg.view().columns)
    cols = cols or columns
    cv = Carved(K, cols, interleaved(K, cols, perm))
    cfg.bind_columns(**cv.kw)
    b = cfg.region_binding()
    assert int(b.d_columns) == cv.ptrs[0] and int(b.context_pitch) == 0 and int(b.column_pitch) == PITCH
    assert int(cfg.view().d_gate) == cv.ptrs[0]
    if K > 1:
        for c in (0, K - 1):
            assert int(cfg.context_region(c).d_image) == cv.ptrs[c * cols]
    tres = twin.digest_batch(msgs)
    a, bb, res = run_twice(cfg, cv, msgs, split)
    assert [r.output_bytes for r in res] == [hashlib.sha256(m).digest() for m in msgs]
    for r, t in zip(res, tres):                              # positions: an unbound twin's
        for cell in (r.prologue_cell, r.block_cell, r.block_cell + eng.G - 1, r.epilogue_cell, r.end_cell - 1):
            assert cfg.cell_position(cell) == twin.cell_position(cell)
        assert (r.prologue_cell, r.block_cell, r.end_cell, r.first_block) == (t.prologue_cell, t.block_cell, t.end_cell, t.first_block)
    written = (a == bb).all(axis=1)
    exp, gate = expected_mask(hsw, twin, cv, (kind, tuple(sizes), K > 1, origin, tuple(decl or [])))
    print("written %d, expected %d (gate %d)" % (int(written.sum()), int(exp.sum()), int(gate.sum())))
    diff = np.nonzero(written != exp)[0]
    assert len(diff) == 0, "cells written but not assigned, or assigned but not written: %s" % diff[:8].tolist()
    assert (bb[~written] == np.uint64(S2)).all()               # rows >= MAX_ROWS of every column, pads, everything else
    st, ts = cfg.streams(), twin.streams()
    gm = np.stack([image_mask(cv, gate, c, columns) for c in range(K)])
    gm = gm if K > 1 else gm[0]
    assert st["gate"].shape == ts["gate"].shape
    assert np.array_equal(st["gate"][gm], ts["gate"][gm]) and (st["gate"][~gm] == np.uint64(S2)).all() and not ts["gate"][~gm].any()
    assert np.array_equal(st["dense"], ts["dense"]) and np.array_equal(st["spread"], ts["spread"])
    Lp = len(ts["lookup"]) // K
    lm = np.concatenate([exp[cv.o_lk + c * cv.per_proof: cv.o_lk + c * cv.per_proof + Lp] for c in range(K)])
    assert np.array_equal(st["lookup"][lm], ts["lookup"][lm])
    if oracle_ref is not None:
        img, mask, lookup, dense, spread = oracle_ref
        assert np.array_equal(mask, gm) and np.array_equal(st["gate"][mask], img[mask])
        assert np.array_equal(st["lookup"][origin[3]:], lookup)
        assert np.array_equal(st["dense"], dense[:, : st["rows"]]) and np.array_equal(st["spread"], spread[:, : st["rows"]])
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    # download_region: the gate buffer laid out as the unbound twin's, lookup and chip buffers as the bound pitches
    hg = np.full((K * columns * MAX_ROWS, 4), np.uint64(HOST), dtype=np.uint64)
    rest = np.full((K * cv.per_proof, 4), np.uint64(HOST), dtype=np.uint64)
    p = rest.ctypes.data
    dst = N.RegionHost(hg.ctypes.data, p, p + 32 * cv.area, p + 32 * 3 * cv.area)
    cfg._ok(cfg.lib.hsw_gadget_download_region(cfg.h, C.byref(dst)))
    hg = hg.reshape(ts["gate"].shape)
    assert np.array_equal(hg[gm], ts["gate"][gm]) and (hg[~gm] == np.uint64(HOST)).all()
    area = exp[cv.o_lk: cv.o_lk + K * cv.per_proof]
    assert np.array_equal(rest[area], bb[cv.o_lk: cv.o_lk + K * cv.per_proof][area]) and (rest[~area] == np.uint64(HOST)).all()
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
    """After a reset the same bytes are written again; unbound, the gadget behaves like the twin and the caller's tensor is
    untouched."""
    cfg.reset()
    cfg.digest_batch(msgs)
    assert np.array_equal(cv.host(), last)
    cfg.reset()
    cfg.bind_region(None)
    assert int(cfg.view().d_gate) not in cv.ptrs
    cfg.digest_batch(msgs)
    st, ts = cfg.streams(), twin.streams()
    for k in ("gate", "lookup", "dense", "spread"):
        assert np.array_equal(st[k], ts[k]), k
    assert cfg.verify()["violations"] == 0
    assert np.array_equal(cv.host(), last)


SINGLE = [("test_circuit", [b"abc", b""], [128, 128], (0, 17, False, 0), [2, 0, 1]),
          ("bench_circuit", [bytes([1] * 56)], [1024], (2, 131000, False, 5), None)]   # None: reversed address order


@REPR
@pytest.mark.parametrize("shape", SINGLE, ids=[s[0] for s in SINGLE])
def test_single_proof_columns_by_pointer(hsw, oracle, eng_int, shape, mont):
    """1 + 2: 3 columns in address order 2, 0, 1 and the bench circuit's columns in reversed address order (9 columns from
    row 0; from origin row 131000 the first column holds 63 cells only and the layout takes 10)."""
    _, msgs, sizes, origin, perm = shape
    ref = oracle_single(oracle, msgs, sizes, origin, mont)
    if perm is None:
        perm = list(range(ref[0].shape[0] - 1, -1, -1))     # (the oracle's image, placed by the FlexGate model: its columns)
        assert len(perm) >= 9
    cfg, twin, cv, last, _ = check_pass(hsw, eng_int, "single", sizes, 1, origin, mont, msgs, perm, oracle_ref=ref)
    assert int(cfg.view().columns) == len(perm)
    assert "hsw_small_table_kernel" in eng_int.last_launch()["kernel"]
    reset_and_unbind(cfg, twin, cv, last, msgs)
    cfg.close()
    twin.close()


@REPR
@pytest.mark.parametrize("K", [2, 9], ids=["K2_small_batch_kernel", "K9_streaming_kernel"])
def test_k_proofs_context_images_columns_by_pointer(hsw, oracle, eng_int, K, mont):
    """3: K bench circuits as context images, 9 columns each by pointer; the first and last proof gathered through their own
    pointers equal a single-proof gadget's and the oracle's; a poked gate cell is reported."""
    origin = (0, 0, False, 3)
    msgs = [bytes([h + 1] * 56) for h in range(K)]
    cfg, twin, cv, last, res = check_pass(hsw, eng_int, "images", [1024], K, origin, mont, msgs, list(range(8, -1, -1)))
    kernel = eng_int.last_launch()["kernel"]
    assert ("hsw_small_table_kernel" if K == 2 else "hsw_expand_table_kernel") in kernel, kernel
    st = cfg.streams()
    rows = st["rows"] // K
    for c in (0, K - 1):
        img, mask, lookup, dense, spread = oracle_single(oracle, [msgs[c]], [1024], origin, mont)
        one = make(hsw, eng_int, "single", [1024], 1, origin, mont)
        one.digest(msgs[c])
        so = one.streams()
        assert np.array_equal(st["gate"][c][mask], img[mask]) and np.array_equal(st["gate"][c][mask], so["gate"][mask])
        Lp = len(st["lookup"]) // K
        assert np.array_equal(st["lookup"][c * Lp + 3: (c + 1) * Lp], lookup)
        assert np.array_equal(st["dense"][:, c * rows: (c + 1) * rows], dense[:, :rows])
        assert np.array_equal(st["spread"][:, c * rows: (c + 1) * rows], spread[:, :rows])
        one.close()
    # one gate cell of the last proof, in a column >= 1: the verifier reports its block, within 3 cells before it
    r = res[K - 1]
    cell = r.block_cell + (r.n_blocks - 1) * eng_int.G + 1000
    col, row = cfg.cell_position(cell)
    assert col >= 1
    at = cv.start[(K - 1, col)] + row
    old = cv.peek(at)
    cv.poke(at, 12345 if old != 12345 else 54321)
    rep = cfg.verify()
    assert rep["violations"] > 0 and rep["first_block"] == r.first_block + r.n_blocks - 1 and 1000 - 3 <= rep["first_cell"] <= 1000, rep
    cv.poke(at, old)
    assert cfg.verify()["violations"] == 0
    cfg.close()
    twin.close()


@REPR
def test_context_group_with_an_interlude_columns_by_pointer(hsw, eng_int, mont):
    """4: K = 3 proofs x [192, 64] with an interlude; one batch and a batch split inside Context 1 write the same bytes."""
    K, sizes, origin = 3, [192, 64], (1, 777, False, 5)
    decl = interlude_after_digest0(hsw, eng_int, sizes, origin)
    msgs = [bytes([7 + i] * (20 + 5 * i)) for i in range(2 * K)]
    probe = make(hsw, eng_int, "group", sizes, K, origin, mont, decl)
    cols = int(probe.view().columns)
    probe.close()
    perm = list(range(cols - 1, -1, -1))
    cfg, twin, cv, one_batch, _ = check_pass(hsw, eng_int, "group", sizes, K, origin, mont, msgs, perm, decl=decl)
    _, _, cv2, split_batch, _ = check_pass(hsw, eng_int, "group", sizes, K, origin, mont, msgs, perm, decl=decl, split=3)
    assert cv2.start == cv.start and np.array_equal(split_batch, one_batch)
    cfg.close()
    twin.close()


@REPR
def test_shared_context_beyond_17_columns_columns_by_pointer(hsw, eng_int, mont):
    """5: a shared context whose interlude spans columns (more than 17 columns); a declaration past columns_capacity is
    HSW_ERR_TOO_LARGE and changes nothing."""
    sizes, origin = [1024, 1024], (1, 777, False, 5)
    decl = interlude_after_digest0(hsw, eng_int, sizes, origin)
    msgs = [b"a" * 700, b"b" * 100]
    probe = make(hsw, eng_int, "shared", sizes, 1, origin, mont, decl)
    cols = int(probe.view().columns)
    probe.close()
    assert cols > 17
    cfg, twin, cv, last, _ = check_pass(hsw, eng_int, "shared", sizes, 1, origin, mont, msgs, list(range(cols - 1, -1, -1)), decl=decl)
    cfg.reset()
    with pytest.raises(hsw.HswError) as ei:
        cfg.set_digest_origin(1, decl[0][1] + 5, 41, decl[0][3])
    assert ei.value.status == hsw._native.HSW_ERR_TOO_LARGE
    assert int(cfg.view().d_gate) == cv.ptrs[0] and int(cfg.view().columns) == int(twin.view().columns)
    assert np.array_equal(cv.host(), last)
    reset_and_unbind(cfg, twin, cv, last, msgs)
    cfg.close()
    twin.close()


@REPR
def test_bench_circuit_every_column_an_allocation_of_its_own(hsw, oracle, eng_int, mont):
    """6: the bench circuit with every column a torch.empty of its own, wherever the allocator puts them: values,
    verify() and the twin's positions."""
    import torch
    msgs, sizes, origin = [bytes([1] * 56)], [1024], (2, 131000, False, 5)
    img, mask, lookup, dense, spread = oracle_single(oracle, msgs, sizes, origin, mont)
    twin = make(hsw, eng_int, "single", sizes, 1, origin, mont)
    cfg = make(hsw, eng_int, "single", sizes, 1, origin, mont)
    ncols = img.shape[0]
    assert ncols >= 9 and int(cfg.view().columns) == ncols
    columns = [torch.zeros((PITCH, 4), dtype=torch.int64, device="cuda") for _ in range(ncols)]
    rest = torch.zeros((5 * up4(PITCH), 4), dtype=torch.int64, device="cuda")
    p, area = rest.data_ptr(), up4(PITCH)
    cfg.bind_columns(columns, PITCH, ncols, lookup=p, lookup_capacity=PITCH, chip_dense=p + 32 * area, chip_spread=p + 32 * 3 * area,
                     chip_col_stride=area, chip_rows_capacity=PITCH)
    res, tres = cfg.digest_batch(msgs), twin.digest_batch(msgs)
    assert res[0].output_bytes == hashlib.sha256(msgs[0]).digest()
    for cell in (res[0].prologue_cell, res[0].block_cell, res[0].epilogue_cell, res[0].end_cell - 1):
        assert cfg.cell_position(cell) == twin.cell_position(cell)
    assert res[0].end_cell == tres[0].end_cell
    torch.cuda.synchronize()
    got = np.stack([c.cpu().numpy().view(np.uint64)[:MAX_ROWS] for c in columns])
    assert np.array_equal(got[mask], img[mask]) and not got[~mask].any()
    st = cfg.streams()
    assert np.array_equal(st["lookup"][origin[3]:], lookup)
    assert np.array_equal(st["dense"], dense[:, : st["rows"]]) and np.array_equal(st["spread"], spread[:, : st["rows"]])
    assert cfg.verify()["violations"] == 0
    cfg.close()
    twin.close()
