"""hsw_gadget_bind_region on the MI355X: a gadget's region written straight into caller-owned device memory at the
caller's pitches.  Every case runs in canonical and Montgomery form, the caller's memory pre-filled with a non-zero
sentinel in every cell.

What was written is found without the layout code of the gadget under test: the pass runs twice over two different
sentinels, and a cell is written exactly if both runs agree on it.  Where the cells should be follows from an UNBOUND
twin gadget (its positions, its deliveries) and, for the single-proof shapes, from the oracle's streams placed by the
FlexGate model of tests/test_gpu_origin.py."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.test_gpu_origin import model_columns

pytestmark = pytest.mark.gpu
MAX_ROWS = (1 << 17) - 9
N17 = 1 << 17
S1, S2, HOST = 0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C3C3C3C3C, 0x7EADBEEFCAFEF00D
REPR = pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


def up4(x):
    return (x + 3) & ~3


class Slabs:
    """One slab per proof in ONE allocation: [cols image columns | lookup | 2 dense | 2 spread] "polynomials" of
    `pitch` cells each, every area on a 128-byte line, every cell a sentinel."""

    def __init__(self, cfg, K, pitch, cols=9):
        import torch
        need = cfg.region_binding()
        self.K, self.pitch = K, pitch
        self.cols = max(cols, int(cfg.view().columns))
        assert int(need.lookup_capacity) <= pitch and int(need.chip_rows_capacity) <= pitch
        self.o_lk = up4(self.cols * pitch)
        self.o_cd = self.o_lk + up4(pitch)
        self.o_cs = self.o_cd + up4(2 * pitch)
        self.slab = self.o_cs + up4(2 * pitch)
        if pitch == N17:
            assert self.slab == (self.cols + 5) * N17            # 14 * 2^17 for the 9-column bench circuit
        self.t = torch.empty((K * self.slab, 4), dtype=torch.int64, device="cuda")
        self.fill(S1)
        p = self.t.data_ptr()
        self.kw = dict(columns=p, column_pitch=pitch, columns_capacity=self.cols, context_pitch=self.slab,
                       lookup=p + 32 * self.o_lk, lookup_capacity=pitch, lookup_pitch=self.slab,
                       chip_dense=p + 32 * self.o_cd, chip_spread=p + 32 * self.o_cs, chip_col_stride=pitch,
                       chip_rows_capacity=pitch, chip_context_pitch=self.slab)

    def fill(self, v):
        import torch
        self.t.fill_(v)
        torch.cuda.synchronize()

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(np.uint64)

    def peek(self, cell):
        return int(self.t[cell, 0].item()) & ((1 << 64) - 1)

    def poke(self, cell, value):
        """limb 0 of one cell := value (a uint64)"""
        import torch
        self.t[cell, 0] = value - (1 << 64) if value >= (1 << 63) else value
        torch.cuda.synchronize()


def make(hsw, eng, kind, sizes, K, origin, mont, decl=None):
    N = hsw._native
    col, row, zero, lq = origin
    if kind == "single":
        cfg = hsw.Sha256DynamicConfig(eng, sizes, True, whole_digest=True)
    elif kind == "shared":
        cfg = hsw.Sha256DynamicConfig(eng, sizes, True, whole_digest=True, shared_context=True)
    elif kind == "images":
        cfg = hsw.Sha256DynamicConfig(eng, sizes * K, True, whole_digest=True, independent=True, context_images=True)
    else:
        cfg = hsw.Sha256DynamicConfig(eng, sizes, True, n_contexts=K)
    if mont:
        cfg.set_repr(N.HSW_REPR_MONTGOMERY)
    cfg.set_origin(col, row, zero, lq)
    cfg.set_columns(MAX_ROWS)
    for d in decl or []:
        cfg.set_digest_origin(*d)
    return cfg


def interlude_after_digest0(hsw, eng, sizes, origin):
    """A declaration for digest 1: three columns past digest 0's last cell, row 41, 11 caller lookups in between."""
    probe = make(hsw, eng, "shared", sizes, 1, origin, False)
    r = probe.digest(b"x")
    c, _ = probe.cell_position(r.end_cell - 1)
    lk = int(probe.view().lookup_cells)
    probe.close()
    return [(1, c + 3, 41, lk + 11)]


_POSITIONS = {}                                               # (layout key) -> one Context's positions: they do not depend on pitch or form


def expected_mask(hsw, twin, sl, K, key):
    """The cells of the slabs the layout assigns, from the UNBOUND twin after its pass: its gate positions (one Context's,
    repeated per proof), the lookup cells its own delivery touches, the chip rows of one proof."""
    N = hsw._native
    v = twin.view()
    exp = np.zeros(K * sl.slab, dtype=bool)
    C1 = int(v.gate_cells) // K
    oc = int(v.origin_column)
    if key not in _POSITIONS:
        _POSITIONS[key] = np.array([twin.cell_position(i) for i in range(C1)], dtype=np.int64)
    pos = _POSITIONS[key]
    assert len(pos) == C1
    img = (pos[:, 0] - oc) * sl.pitch + pos[:, 1]
    assert pos[:, 1].max() < MAX_ROWS and len(np.unique(img)) == C1
    Lp = int(twin.region_binding().lookup_capacity) if K > 1 else int(v.lookup_cells)
    look = np.full((K * Lp if K > 1 else Lp, 4), np.uint64(HOST), dtype=np.uint64)
    dst = N.RegionHost(None, look.ctypes.data, None, None)
    twin._ok(twin.lib.hsw_gadget_download_region(twin.h, C.byref(dst)))
    lk = (look[:, 0] != np.uint64(HOST)).reshape(K, Lp)
    rows = int(v.num_limb_sum) // 2 // K
    for c in range(K):
        base = c * sl.slab
        exp[base + img] = True
        exp[base + sl.o_lk: base + sl.o_lk + Lp] = lk[c]
        for o in (sl.o_cd, sl.o_cs):
            for k in range(2):
                exp[base + o + k * sl.pitch: base + o + k * sl.pitch + rows] = True
    return exp, int(lk.sum())


def run_twice(cfg, sl, msgs, split=None):
    """The pass over sentinel S1, then -- after a reset -- over S2: the slabs after each."""
    snaps = []
    for s in (S1, S2):
        cfg.reset()
        sl.fill(s)
        if split:
            res = cfg.digest_batch(msgs[:split]) + cfg.digest_batch(msgs[split:])
        else:
            res = cfg.digest_batch(msgs)
        snaps.append(sl.host())
    return snaps[0], snaps[1], res


def check_bound_pass(hsw, eng, kind, sizes, K, origin, mont, pitch, msgs, decl=None, split=None, oracle_ref=None):
    """Checks 1, 2, 5, 6 (and the per-proof half of 3) for one layout; returns the slab bytes of the last pass."""
    N = hsw._native
    twin = make(hsw, eng, kind, sizes, K, origin, mont, decl)
    cfg = make(hsw, eng, kind, sizes, K, origin, mont, decl)
    sl = Slabs(cfg, K, pitch)
    cfg.bind_region(**sl.kw)
    b = cfg.region_binding()
    assert int(b.d_columns) == sl.t.data_ptr() and int(b.column_pitch) == pitch and int(b.context_pitch) == sl.slab
    tres = twin.digest_batch(msgs)
    a, bb, res = run_twice(cfg, sl, msgs, split)
    v = cfg.view()
    assert int(v.d_gate) == sl.t.data_ptr() and int(v.d_lookup) == sl.t.data_ptr() + 32 * sl.o_lk
    assert int(v.chip_col_stride) == pitch
    assert [r.output_bytes for r in res] == [hashlib.sha256(m).digest() for m in msgs]
    # positions: the same as the unbound twin's
    for r, t in zip(res, tres):
        for cell in (r.prologue_cell, r.block_cell, r.block_cell + eng.G - 1, r.epilogue_cell, r.end_cell - 1):
            assert cfg.cell_position(cell) == twin.cell_position(cell)
        assert (r.prologue_cell, r.block_cell, r.end_cell, r.first_block) == (t.prologue_cell, t.block_cell, t.end_cell, t.first_block)
    # 2. nothing else is written: a cell is written exactly if both runs agree on it
    written = (a == bb).all(axis=1)
    exp, n_lookup = expected_mask(hsw, twin, sl, K, (kind, tuple(sizes), K > 1, origin, tuple(decl or [])))
    gate_area = np.zeros_like(exp)
    for c in range(K):
        gate_area[c * sl.slab: c * sl.slab + sl.o_lk] = True
    print("written cells: gate %d (gate_cells %d), all %d, expected %d" % (int((written & gate_area).sum()), int(v.gate_cells),
                                                                       int(written.sum()), int(exp.sum())))
    assert int((written & gate_area).sum()) == int(v.gate_cells)
    diff = np.nonzero(written != exp)[0]
    assert len(diff) == 0, "cells written but not assigned, or assigned but not written (proof, slab cell): %s" % [
        (int(i) // sl.slab, int(i) % sl.slab) for i in diff[:8]]
    assert (bb[~written] == np.uint64(S2)).all()
    # 1 / 3. the values: the bound gadget's cells, gathered at the pitches, equal the unbound twin's streams
    st, ts = cfg.streams(), twin.streams()
    tg = ts["gate"]
    assert st["gate"].shape == tg.shape
    # (the twin's unassigned cells are zero, the caller's hold the sentinel: compare where the layout assigns)
    gm = np.stack([exp[c * sl.slab: c * sl.slab + sl.cols * sl.pitch].reshape(sl.cols, sl.pitch)[: tg.shape[-3], :MAX_ROWS] for c in range(K)])
    gm = gm if K > 1 else gm[0]
    assert np.array_equal(st["gate"][gm], tg[gm]) and (st["gate"][~gm] == np.uint64(S2)).all() and not tg[~gm].any()
    assert np.array_equal(st["dense"], ts["dense"]) and np.array_equal(st["spread"], ts["spread"])
    lm = np.concatenate([exp[c * sl.slab + sl.o_lk: c * sl.slab + sl.o_lk + len(ts["lookup"]) // K] for c in range(K)])
    assert np.array_equal(st["lookup"][lm], ts["lookup"][lm]) and (st["lookup"][~lm] == np.uint64(S2)).all()
    if oracle_ref is not None:                                # single proof: the oracle's streams, placed by the FlexGate model
        img, mask, lookup, dense, spread = oracle_ref
        assert np.array_equal(st["gate"][mask], img[mask]) and np.array_equal(mask, gm)
        lq = origin[3]
        assert np.array_equal(st["lookup"][lq:], lookup)
        assert np.array_equal(st["dense"], dense[:, : st["rows"]]) and np.array_equal(st["spread"], spread[:, : st["rows"]])
    # 5. the verifier follows the binding
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    # 6. deliveries into host buffers laid out like the slabs
    host = np.full((K * sl.slab, 4), np.uint64(HOST), dtype=np.uint64)
    p = host.ctypes.data
    dst = N.RegionHost(p, p + 32 * sl.o_lk, p + 32 * sl.o_cd, p + 32 * sl.o_cs)
    cfg._ok(cfg.lib.hsw_gadget_download_region(cfg.h, C.byref(dst)))
    assert np.array_equal(host[exp], bb[exp]) and (host[~exp] == np.uint64(HOST)).all()
    tape = N.RegionTape()
    cfg._ok(cfg.lib.hsw_gadget_region_tape(cfg.h, C.byref(tape)))
    distinct = np.zeros((int(tape.n_distinct) + 1, 4), dtype=np.uint64)
    n = C.c_size_t()
    cfg._ok(cfg.lib.hsw_gadget_download_region_distinct(cfg.h, distinct.ctypes.data, int(tape.n_distinct), C.byref(n)))
    host2 = np.full((K * sl.slab, 4), np.uint64(HOST), dtype=np.uint64)
    p = host2.ctypes.data
    dst = N.RegionHost(p, p + 32 * sl.o_lk, p + 32 * sl.o_cd, p + 32 * sl.o_cs)
    cfg._ok(cfg.lib.hsw_gadget_replay_region(cfg.h, distinct.ctypes.data, C.byref(dst), 8))
    assert np.array_equal(host2, host)
    # the refusals of a bound gadget
    for call in (lambda: cfg.seek(0), lambda: cfg.download_region_compact()):
        with pytest.raises(hsw.HswError) as ei:
            call()
        assert ei.value.status == N.HSW_ERR_UNSUPPORTED
    return cfg, twin, sl, bb, res


def oracle_single(oracle, msgs, sizes, origin, mont):
    conv = oracle.to_montgomery if mont else (lambda x: x)
    ref = oracle.digest_cells(msgs, sizes, None, True, zero_cell_loaded=origin[2])
    img, mask, _ = model_columns(ref["call_lens"], conv(ref["gate"]), MAX_ROWS, origin[1])
    return img, mask, conv(ref["lookup"]), conv(ref["dense"]), conv(ref["spread"])


SINGLE = [("test_circuit", [b"abc", b""], [128, 128], (0, 17, False, 0)),
          ("bench_circuit", [bytes([1] * 56)], [1024], (2, 131000, False, 5))]


@REPR
@pytest.mark.parametrize("pitch", [MAX_ROWS + 3, N17], ids=["pitch_max_rows_plus_3", "pitch_2_17"])
@pytest.mark.parametrize("shape", SINGLE, ids=[s[0] for s in SINGLE])
def test_single_proof_oracle_parity_and_nothing_else_written(hsw, oracle, eng_int, shape, pitch, mont):
    """1 + 2 (+ 5, 6, 7): the gadget's cells at column * pitch + row equal the oracle's, placed as tests/test_gpu_origin.py
    places them; every other cell of the caller's memory keeps the sentinel; unbinding gives a library-owned gadget."""
    _, msgs, sizes, origin = shape
    ref = oracle_single(oracle, msgs, sizes, origin, mont)
    cfg, twin, sl, last, _ = check_bound_pass(hsw, eng_int, "single", sizes, 1, origin, mont, pitch, msgs, oracle_ref=ref)
    # 7. after a reset the bound gadget writes the same bytes again; unbound, it behaves like a fresh library-owned one
    cfg.reset()
    cfg.digest_batch(msgs)
    assert np.array_equal(sl.host(), last)
    cfg.reset()
    cfg.bind_region(None)
    assert int(cfg.view().d_gate) != sl.t.data_ptr()
    cfg.digest_batch(msgs)
    st, ts = cfg.streams(), twin.streams()
    for k in ("gate", "lookup", "dense", "spread"):
        assert np.array_equal(st[k], ts[k]), k
    assert cfg.verify()["violations"] == 0
    assert np.array_equal(sl.host(), last)                    # the caller's memory: untouched since
    cfg.close()
    twin.close()


def poke_and_verify(cfg, sl, res, proof, chip_row):
    """5. one cell of the caller's slab overwritten: the verifier reports that cell -- a gate cell in a column other than
    column 0 of a proof other than proof 0, and a chip cell likewise."""
    G, LC = cfg.engine.G, 4120                                 # gate cells of a block in internals mode; limb calls
    v = cfg.view()
    per = len(res) // sl.K
    r = res[proof * per]
    cell = r.block_cell + (r.n_blocks - 1) * G + 1000          # in the digest's last block
    col, row = cfg.cell_position(cell)
    assert col - int(v.origin_column) >= 1
    at = proof * sl.slab + (col - int(v.origin_column)) * sl.pitch + row
    old = sl.peek(at)
    sl.poke(at, 12345 if old != 12345 else 54321)
    rep = cfg.verify()
    print("gate poke:", rep)
    # (the earliest failure of the block: the poked cell's own checks or its gate row, which starts <= 3 cells before it)
    assert rep["violations"] > 0 and rep["first_block"] == r.first_block + r.n_blocks - 1 and 1000 - 3 <= rep["first_cell"] <= 1000, rep
    sl.poke(at, old)
    assert cfg.verify()["violations"] == 0
    # chip column 1 of the proof, row chip_row: limb call 2 * chip_row + 1 of the proof, in its block (2 * chip_row + 1) // 4120
    at = proof * sl.slab + sl.o_cd + sl.pitch + chip_row
    old = sl.peek(at)
    sl.poke(at, old ^ 1)
    rep = cfg.verify()
    print("chip poke:", rep)
    first_block = res[proof * per].first_block + (2 * chip_row + 1) // LC
    assert rep["violations"] > 0 and rep["first_class"] == "chip" and rep["first_block"] == first_block, rep
    sl.poke(at, old)
    assert cfg.verify()["violations"] == 0


@REPR
@pytest.mark.parametrize("K", [8, 9], ids=["K8_small_batch_kernel", "K9_streaming_kernel"])
def test_k_proofs_context_images_one_slab_per_proof(hsw, oracle, eng_int, K, mont):
    """3 (+ 1, 2, 5, 6 per proof): K bench circuits, one slab of 14 x 2^17 cells per proof, all pointers in one
    allocation; proof c's image, lookup column and chip rows, read from its slab alone, equal a single-proof gadget's
    and the oracle's."""
    origin = (0, 0, False, 3)
    msgs = [bytes([h + 1] * 56) for h in range(K)]
    cfg, twin, sl, last, res = check_bound_pass(hsw, eng_int, "images", [1024], K, origin, mont, N17, msgs)
    assert sl.slab == 14 * N17
    kernel = eng_int.last_launch()["kernel"]
    assert ("hsw_small_kernel" in kernel) == (K == 8), kernel      # K = 8 x 16 blocks: the small-batch kernel takes it
    # proof c from its slab alone against a single-proof gadget and the oracle
    st = cfg.streams()
    rows = st["rows"] // K
    for c in (0, K - 1):
        img, mask, lookup, dense, spread = oracle_single(oracle, [msgs[c]], [1024], origin, mont)
        one = make(hsw, eng_int, "single", [1024], 1, origin, mont)
        one.digest(msgs[c])
        so = one.streams()
        assert np.array_equal(st["gate"][c][mask], img[mask]) and np.array_equal(st["gate"][c][mask], so["gate"][mask])
        Lp = len(st["lookup"]) // K
        assert np.array_equal(st["lookup"][c * Lp + 3: (c + 1) * Lp], lookup) and np.array_equal(so["lookup"][3:], lookup)
        assert np.array_equal(st["dense"][:, c * rows: (c + 1) * rows], dense[:, :rows])
        assert np.array_equal(st["spread"][:, c * rows: (c + 1) * rows], spread[:, :rows])
        one.close()
    poke_and_verify(cfg, sl, res, K - 1, 5000)
    cfg.close()
    twin.close()


@REPR
def test_context_group_with_an_interlude_and_a_split_batch(hsw, eng_int, mont):
    """3: K = 4 proofs x 2 digests with an interlude, one slab per proof; a batch split in the middle of a Context
    writes the same bytes as one batch."""
    K, sizes, origin = 4, [192, 64], (1, 777, False, 5)
    decl = interlude_after_digest0(hsw, eng_int, sizes, origin)
    msgs = [bytes([7 + i] * (20 + 5 * i)) for i in range(2 * K)]
    cfg, twin, sl, one_batch, res = check_bound_pass(hsw, eng_int, "group", sizes, K, origin, mont, N17, msgs, decl=decl)
    assert sl.slab == 14 * N17
    # (the pass as ONE batch: digest 0 of every Context is one launch from block 0, so the report's blocks are the pass's)
    poke_and_verify(cfg, sl, res, 2, 1000)
    cfg.reset()
    sl.fill(S2)
    cfg.digest_batch(msgs[:3])                                 # ends in the middle of Context 1
    cfg.digest_batch(msgs[3:])
    assert np.array_equal(sl.host(), one_batch)
    assert cfg.verify()["violations"] == 0
    cfg.close()
    twin.close()


@REPR
def test_shared_context_beyond_17_columns_with_an_interlude(hsw, eng_int, mont):
    """4: a shared context of more than 17 columns with a declared interlude that spans columns, bound."""
    sizes, origin = [1024, 1024], (1, 777, False, 5)
    decl = interlude_after_digest0(hsw, eng_int, sizes, origin)
    msgs = [b"a" * 700, b"b" * 100]
    cfg, twin, sl, _, _ = check_bound_pass(hsw, eng_int, "shared", sizes, 1, origin, mont, N17, msgs, decl=decl)
    assert int(cfg.view().columns) > 17
    # a declaration that would grow the image past the caller's columns: refused, nothing changed
    cfg.reset()
    with pytest.raises(hsw.HswError) as ei:
        cfg.set_digest_origin(1, decl[0][1] + 5, 41, decl[0][3])
    assert ei.value.status == hsw._native.HSW_ERR_TOO_LARGE
    assert int(cfg.view().d_gate) == sl.t.data_ptr() and int(cfg.view().columns) == int(twin.view().columns)
    cfg.close()
    twin.close()
