"""hsw_gadget_create_contexts: K proofs (Contexts) of a circuit with M digests each, every Context laid out like one
HSW_GADGET_SHARED_CONTEXT gadget of the M sizes, the K layouts repeating like context images.

For every Context c the expected region is the oracle's streams of that Context's M digests as ONE Context
(oracle.digest_cells), placed by the host model of tests/test_gpu_shared_context.py (model_shared).  Image, used /
unused mask, lookup column and chip rows of EVERY Context are compared bit for bit, every digest against hashlib.
The caller's cells -- rows above the origin, interlude cells, queued lookup entries -- are never written on the
device and never touched in host buffers."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.test_gpu_context_images import ORIGINS
from tests.test_gpu_origin import MAX_ROWS
from tests.test_gpu_shared_context import SENTINEL, model_shared, write_device_cells

pytestmark = pytest.mark.gpu
LC = 4120                                   # limb calls per block at the 8-bit table


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


def _msg(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def messages(sizes, k, lengths, seed):
    """msgs[c][j], pres[c][j]: `lengths` is a list of (context, digest, length, precomputed_input_len) that must be
    covered; every other digest gets a random length.  All messages differ."""
    rng = np.random.default_rng(seed)
    msgs = [[None] * len(sizes) for _ in range(k)]
    pres = [[0] * len(sizes) for _ in range(k)]
    for c, j, n, pre in lengths:
        assert msgs[c][j] is None
        msgs[c][j], pres[c][j] = _msg(seed * 1000 + c * 10 + j, n), pre
    for c in range(k):
        for j, mx in enumerate(sizes):
            if msgs[c][j] is None:
                msgs[c][j] = _msg(seed * 1000 + c * 10 + j, int(rng.integers(1, mx - 9)))
    return msgs, pres


def make_group(hsw, eng, sizes, k, origin, decl, mont, rc=True):
    col0, row0, zero, lq = origin
    cfg = hsw.Sha256DynamicConfig(eng, sizes, is_input_range_check=rc, n_contexts=k)
    if mont:
        cfg.set_repr(hsw._native.HSW_REPR_MONTGOMERY)
    cfg.set_origin(col0, row0, zero, lq)
    cfg.set_columns(MAX_ROWS)
    for j, (c, r, lk) in sorted(decl.items()):
        cfg.set_digest_origin(j, c, r, lk)
    return cfg


def issue(cfg, msgs, pres, how):
    """The pass as one batch, digest by digest, or as two batches split in the middle of Context 1."""
    flat = [m for ctx in msgs for m in ctx]
    fpre = [p for ctx in pres for p in ctx]
    m = len(msgs[0])
    if how == "batch":
        return cfg.digest_batch(flat, fpre)
    if how == "each":
        return [cfg.digest(a, b) for a, b in zip(flat, fpre)]
    cut = m + (m + 1) // 2                                       # inside Context 1
    return cfg.digest_batch(flat[:cut], fpre[:cut]) + cfg.digest_batch(flat[cut:], fpre[cut:])


def expected(oracle, sizes, msgs, pres, origin, decl, mont, rc=True):
    """Per Context: (image, mask, lookup, lmask, dense, spread) from the oracle and the host model."""
    col0, row0, zero, lq = origin
    conv = oracle.to_montgomery if mont else (lambda x: x)
    out = []
    for mc, pc in zip(msgs, pres):
        ref = oracle.digest_cells(mc, sizes, pc, rc, zero_cell_loaded=zero)
        image, mask, lookup, lmask = model_shared(ref, conv, (col0, row0), {j: (c, r) for j, (c, r, _) in decl.items()}, lq,
                                                  {j: lk for j, (_, _, lk) in decl.items()})
        out.append((image, mask, lookup, lmask, conv(ref["dense"]), conv(ref["spread"])))
    return out


def check_group(cfg, res, exp, sizes, msgs, origin, sentinels=None):
    """Image, used / unused mask, lookup column and chip rows of EVERY Context; every digest against hashlib.
    sentinels: (image offsets, lookup cells) per Context that hold SENTINEL instead of 0."""
    k, m = len(msgs), len(sizes)
    lq = origin[3]
    flat = [x for ctx in msgs for x in ctx]
    assert [r.output_bytes for r in res] == [hashlib.sha256(x).digest() for x in flat]
    st = cfg.streams()
    reg0 = cfg.context_region(0)
    ncols, Lp, cstream = int(reg0.columns), int(reg0.lookup_cells), int(reg0.stream_cells)
    assert st["gate"].shape == (k, ncols, MAX_ROWS, 4)
    assert st["lookup"].shape[0] == k * Lp
    look = st["lookup"].reshape(k, Lp, 4)
    rows_ctx = sum(sizes) // 64 * LC // 2
    assert st["rows"] == k * rows_ctx
    blocks_ctx = sum(sizes) // 64
    s_cells, l_cells = sentinels if sentinels else ([], [])
    for c in range(k):
        image, mask, lookup, lmask, dense, spread = exp[c]
        assert image.shape[0] <= ncols and len(lookup) == Lp
        g = st["gate"][c]
        bad = np.nonzero((g[: image.shape[0]][mask] != image[mask]).any(axis=1))[0]
        assert len(bad) == 0, "Context %d: %d used cells differ (first at used index %d)" % (c, len(bad), bad[0])
        unused = g.reshape(-1, 4).copy()
        unused[: image.shape[0] * MAX_ROWS][mask.reshape(-1)] = 0
        for s in s_cells:
            assert (unused[s] == SENTINEL).all(), "Context %d: the caller's cell %d was written" % (c, s)
            unused[s] = 0
        assert not unused.any(), "Context %d: a cell outside the used mask was written" % c
        assert np.array_equal(look[c][lmask], lookup[lmask]), "Context %d: lookup column" % c
        rest = look[c].copy()
        rest[lmask] = 0
        for s in l_cells:
            assert (rest[s] == SENTINEL).all(), "Context %d: the caller's lookup entry %d was written" % (c, s)
            rest[s] = 0
        assert not rest.any()
        assert np.array_equal(st["dense"][:, c * rows_ctx:(c + 1) * rows_ctx], dense), "Context %d: chip dense" % c
        assert np.array_equal(st["spread"][:, c * rows_ctx:(c + 1) * rows_ctx], spread), "Context %d: chip spread" % c
        reg = cfg.context_region(c)
        assert int(reg.assigned) == 1 and int(reg.first_stream_cell) == c * cstream == res[c * m].prologue_cell
        assert int(reg.d_image) == int(cfg.view().d_gate) + c * ncols * MAX_ROWS * 32
        assert int(reg.d_lookup) == int(cfg.view().d_lookup) + c * Lp * 32
        assert int(reg.chip_rows) == rows_ctx and res[c * m].first_block == c * blocks_ctx
        assert res[c * m + m - 1].end_cell == (c + 1) * cstream
        assert res[c * m].prologue_lookup == c * Lp + lq
    return st


# ---- 1. the small-batch size class: 9 blocks, issued three ways ---------------------------------------------------
LEN_1 = [(0, 0, 0, 0), (1, 0, 55, 0), (2, 0, 119, 0),            # 128-byte digest: empty, one block full, max - 9
         (0, 1, 55, 0), (1, 1, 64 + 20, 64), (2, 1, 0, 0)]       # 64-byte digest: max - 9, a precomputed prefix of 64, empty


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
def test_small_group_three_ways(hsw, oracle, eng_int, mont):
    sizes, k, origin = [128, 64], 3, ORIGINS[0]
    msgs, pres = messages(sizes, k, LEN_1, 11)
    exp = expected(oracle, sizes, msgs, pres, origin, {}, mont)
    got = []
    for how in ("batch", "each", "split"):
        cfg = make_group(hsw, eng_int, sizes, k, origin, {}, mont)
        seq0 = eng_int.last_launch()["seq"] if got else None
        res = issue(cfg, msgs, pres, how)
        li = eng_int.last_launch()
        assert li["split"] == 0 and "hsw_expand_kernel<2, " in li["kernel"]     # what ran: the streaming (table) kernel
        if how == "each":
            assert li["seq"] - seq0 == k * len(sizes) and li["n_blocks"] == 1
        if how == "split":
            assert li["seq"] - seq0 == 2 * len(sizes)
        st = check_group(cfg, res, exp, sizes, msgs, origin)
        rep = cfg.verify()
        assert rep["violations"] == 0 and rep["checks"] > 0, rep
        got.append((st, [(r.prologue_cell, r.block_cell, r.end_cell, r.prologue_lookup, r.first_block) for r in res]))
        cfg.close()
    for st, pos in got[1:]:
        assert pos == got[0][1]
        for name in ("gate", "lookup", "dense", "spread"):
            assert np.array_equal(st[name], got[0][0][name]), name


# ---- 2. two bench-circuit digests per proof: more than 17 columns per Context, expansion + frame launches ---------
LEN_2 = [(0, 0, 56, 0), (0, 1, 1015, 0), (1, 0, 0, 0), (1, 1, 119, 0), (2, 0, 120, 0), (2, 1, 64 * 3 + 700, 192),
         (3, 0, 55, 0), (4, 1, 1015 + 128, 128)]


@pytest.mark.parametrize("origin", [ORIGINS[0], ORIGINS[2]], ids=["origin_0_0", "shifted_zero_loaded_lookups_queued"])
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
def test_wide_group_expansion_and_frames(hsw, oracle, eng_int, mont, origin):
    sizes, k = [1024, 1024], 5
    msgs, pres = messages(sizes, k, LEN_2, 22)
    exp = expected(oracle, sizes, msgs, pres, origin, {}, mont)
    cfg = make_group(hsw, eng_int, sizes, k, origin, {}, mont)
    assert int(cfg.view().columns) > 17                                           # needs the table
    probe = hsw.Sha256DynamicConfig(eng_int, [64], is_input_range_check=True, whole_digest=True)
    probe.digest(b"x")                                                            # a launch on record before the batch
    probe.close()
    seq0 = eng_int.last_launch()["seq"]
    res = issue(cfg, msgs, pres, "batch")
    li = eng_int.last_launch()
    # 160 blocks: M expansion launches of K x 16 blocks each, not K x M of 16
    assert li["seq"] - seq0 == len(sizes) and li["n_blocks"] == k * 16 and li["split"] == 0
    check_group(cfg, res, exp, sizes, msgs, origin)
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    # positions: FlexGate columns inside the owning Context's image
    st = cfg.streams()
    for d in (1, 2 * k - 1):
        rc = hsw._native.ResultCells()
        cfg._ok(cfg.lib.hsw_gadget_result_cells(cfg.h, d, C.byref(rc)))
        col, row = int(rc.output_byte_pos[0][0]), int(rc.output_byte_pos[0][1])
        flat = [x for ctx in msgs for x in ctx]
        byte0 = np.array([[hashlib.sha256(flat[d]).digest()[0], 0, 0, 0]], dtype=np.uint64)
        byte0 = (oracle.to_montgomery(byte0) if mont else byte0)[0]
        assert np.array_equal(st["gate"][d // 2, col - origin[0], row], byte0)
    cfg.close()


# ---- 3-5. interludes, sentinels, the verifier, deliveries, a second pass -------------------------------------------
LEN_3 = [(0, 0, 183, 0), (0, 1, 55, 0), (0, 2, 56, 0), (1, 0, 120, 0), (1, 1, 0, 0), (1, 2, 119, 0),
         (2, 0, 56, 0), (2, 2, 64 + 56, 64), (3, 0, 119, 0), (3, 1, 64 * 2 + 30, 128), (3, 2, 0, 0)]


def _interlude_layout(hsw, eng, sizes, origin):
    """Declarations: an interlude before digest 1 that crosses a column break, one before digest 2 that adds only
    lookup entries -- found with single shared-context gadgets (the layout follows from the sizes alone)."""
    col0, row0, zero, lq = origin

    def probe(n, decl):
        p = hsw.Sha256DynamicConfig(eng, sizes, is_input_range_check=True, whole_digest=True, shared_context=True)
        p.set_origin(col0, row0, zero, lq)
        p.set_columns(MAX_ROWS)
        for j, (c, r, lk) in sorted(decl.items()):
            p.set_digest_origin(j, c, r, lk)
        res = p.digest_batch([b"a"] * n)
        c, r = p.cell_position(res[-1].end_cell - 1)
        out = (c, r + 1, int(p.view().lookup_cells))
        p.close()
        return out
    fc, fr, lk = probe(1, {})
    decl = {1: (fc + 1, 100, lk + 9)}                                       # from (fc, fr) over the column break to (fc + 1, 100)
    free1 = (fc - col0) * MAX_ROWS + fr
    land1 = (fc + 1 - col0) * MAX_ROWS + 100
    fc2, fr2, lk2 = probe(2, decl)
    decl[2] = (fc2, fr2, lk2 + 7)                                           # the next free cell itself: lookup entries only
    gate_cells = sorted({free1, (free1 + land1) // 2, (fc + 1 - col0) * MAX_ROWS, land1 - 1})
    look_cells = list(range(lq)) + list(range(lk, lk + 9)) + list(range(lk2, lk2 + 7))
    return decl, gate_cells, look_cells


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
def test_interludes_sentinels_verifier_deliveries_and_second_pass(hsw, oracle, eng_int, mont):
    N = hsw._native
    sizes, k, origin = [192, 64, 128], 4, (1, 777, False, 5)
    decl, s_gate, s_look = _interlude_layout(hsw, eng_int, sizes, origin)
    msgs, pres = messages(sizes, k, LEN_3, 33)
    exp = expected(oracle, sizes, msgs, pres, origin, decl, mont)
    cfg = make_group(hsw, eng_int, sizes, k, origin, decl, mont)
    v = cfg.view()
    ncols, Lp = int(v.columns), int(cfg.context_region(0).lookup_cells)
    S = ncols * MAX_ROWS
    # the caller's cells of EVERY Context, on the device, before the pass
    write_device_cells(int(v.d_gate), [c * S + s for c in range(k) for s in s_gate], SENTINEL)
    write_device_cells(int(v.d_lookup), [c * Lp + s for c in range(k) for s in s_look], SENTINEL)
    res = issue(cfg, msgs, pres, "batch")
    st = check_group(cfg, res, exp, sizes, msgs, origin, sentinels=(s_gate, s_look))
    for c in range(k):
        assert cfg.cell_position(res[c * 3 + 1].prologue_cell) == decl[1][:2]
        assert res[c * 3 + 1].prologue_lookup == c * Lp + decl[1][2] and res[c * 3 + 2].prologue_lookup == c * Lp + decl[2][2]
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep

    # ---- 4. deliveries into sentinel-filled host buffers: device bytes on used cells, the caller's cells untouched
    used = np.zeros((k, ncols, MAX_ROWS), dtype=bool)
    lused = np.zeros((k, Lp), dtype=bool)
    for c in range(k):
        used[c, : exp[c][1].shape[0]] = exp[c][1]
        lused[c] = exp[c][3]
    gate_h = np.full((k, ncols, MAX_ROWS, 4), SENTINEL, dtype=np.uint64)
    look_h = np.full((k, Lp, 4), SENTINEL, dtype=np.uint64)
    stride = int(v.chip_col_stride)
    dense_h = np.full((2 * stride, 4), SENTINEL, dtype=np.uint64)
    spread_h = np.full((2 * stride, 4), SENTINEL, dtype=np.uint64)
    dst = N.RegionHost(gate_h.ctypes.data, look_h.ctypes.data, dense_h.ctypes.data, spread_h.ctypes.data)
    cfg._ok(cfg.lib.hsw_gadget_download_region(cfg.h, C.byref(dst)))
    assert np.array_equal(gate_h[used], st["gate"][used]) and (gate_h[~used] == SENTINEL).all()
    assert np.array_equal(look_h[lused], st["lookup"].reshape(k, Lp, 4)[lused]) and (look_h[~lused] == SENTINEL).all()
    assert np.array_equal(dense_h.reshape(2, stride, 4)[:, : st["rows"]], st["dense"])
    assert np.array_equal(spread_h.reshape(2, stride, 4)[:, : st["rows"]], st["spread"])
    full = (gate_h.copy(), look_h.copy(), dense_h.copy(), spread_h.copy())
    # the distinct delivery + replay: bit-equal to download_region, the caller's cells untouched again
    tape = N.RegionTape()
    cfg._ok(cfg.lib.hsw_gadget_region_tape(cfg.h, C.byref(tape)))
    tape_codes = int(C.cast(tape.gate_code, C.c_void_p).value)
    assert int(tape.gate_cells) == res[-1].end_cell
    distinct = eng_int.host_empty((int(tape.distinct_capacity), 4))
    n = C.c_size_t()
    cfg._ok(cfg.lib.hsw_gadget_download_region_distinct(cfg.h, distinct.ctypes.data, distinct.shape[0], C.byref(n)))
    assert n.value == int(tape.n_distinct)
    for a in (gate_h, look_h, dense_h, spread_h):
        a[:] = SENTINEL
    cfg._ok(cfg.lib.hsw_gadget_replay_region(cfg.h, distinct.ctypes.data, C.byref(dst), 4))
    for a, b in zip((gate_h, look_h), full):
        assert np.array_equal(a, b)
    assert np.array_equal(dense_h.reshape(2, stride, 4)[:, : st["rows"]], st["dense"])
    assert np.array_equal(spread_h.reshape(2, stride, 4)[:, : st["rows"]], st["spread"])
    d = cfg.download_region_distinct(threads=3)
    assert np.array_equal(d["gate"][used], st["gate"][used]) and np.array_equal(d["dense"], st["dense"])
    # the device still holds the caller's cells after every delivery
    st_after = cfg.streams()
    assert np.array_equal(st_after["gate"], st["gate"]) and np.array_equal(st_after["lookup"], st["lookup"])
    for call in (lambda: cfg.seek(1), lambda: cfg.place(2)) + (() if mont else (cfg.download_region_compact,)):
        with pytest.raises(hsw.HswError) as ei:
            call()
        assert ei.value.status == N.HSW_ERR_UNSUPPORTED

    # ---- 5. reset, the same declarations again, a second pass with other messages: layout, buffers and tape kept
    ptrs = (int(v.d_gate), int(v.d_lookup))
    cfg.reset()
    for j, (c, r, lk) in sorted(decl.items()):
        cfg.set_digest_origin(j, c, r, lk)
    v2 = cfg.view()
    assert (int(v2.d_gate), int(v2.d_lookup)) == ptrs and int(v2.columns) == ncols
    msgs2, pres2 = messages(sizes, k, [(c, j, n, p) for c, j, n, p in LEN_3 if p == 0][::-1][:5], 44)
    exp2 = expected(oracle, sizes, msgs2, pres2, origin, decl, mont)
    res2 = issue(cfg, msgs2, pres2, "split")
    check_group(cfg, res2, exp2, sizes, msgs2, origin, sentinels=(s_gate, s_look))
    cfg._ok(cfg.lib.hsw_gadget_region_tape(cfg.h, C.byref(tape)))
    assert int(C.cast(tape.gate_code, C.c_void_p).value) == tape_codes
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep

    # ---- 3 (end). one cell of Context K - 1 behind the interlude flipped: the verifier must see it
    r = res2[(k - 1) * 3 + 1]
    col, row = cfg.cell_position(r.block_cell + 1234)
    write_device_cells(int(v2.d_gate), [(k - 1) * S + (col - origin[0]) * MAX_ROWS + row], np.uint64(12345))
    rep = cfg.verify()
    assert rep["violations"] >= 1, rep
    cfg.close()


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
def test_zero_loaded_origin_without_input_range_check_deliveries(hsw, oracle, eng_int, mont):
    """Contexts that come with their zero cell (no Context of the group assigns one: every stream is a cell shorter,
    the region tape leaves K cells of the capacity unused) and queued lookups, input range checks off: the pass, the
    verifier, the full delivery and the distinct delivery + replay, into sentinel-filled host buffers."""
    N = hsw._native
    sizes, k, origin = [128, 64], 3, ORIGINS[2]
    assert origin[2] and origin[3] > 0
    msgs, pres = messages(sizes, k, LEN_1, 55)
    exp = expected(oracle, sizes, msgs, pres, origin, {}, mont, rc=False)
    cfg = make_group(hsw, eng_int, sizes, k, origin, {}, mont, rc=False)
    res = issue(cfg, msgs, pres, "split")
    st = check_group(cfg, res, exp, sizes, msgs, origin)
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    v = cfg.view()
    ncols, Lp, stride = int(v.columns), int(cfg.context_region(0).lookup_cells), int(v.chip_col_stride)
    used = np.zeros((k, ncols, MAX_ROWS), dtype=bool)
    lused = np.zeros((k, Lp), dtype=bool)
    for c in range(k):
        used[c, : exp[c][1].shape[0]] = exp[c][1]
        lused[c] = exp[c][3]
    assert not lused[:, : origin[3]].any() and not used[:, 0, : origin[1]].any()       # the caller's
    gate_h = np.full((k, ncols, MAX_ROWS, 4), SENTINEL, dtype=np.uint64)
    look_h = np.full((k, Lp, 4), SENTINEL, dtype=np.uint64)
    dense_h = np.full((2 * stride, 4), SENTINEL, dtype=np.uint64)
    spread_h = np.full((2 * stride, 4), SENTINEL, dtype=np.uint64)
    dst = N.RegionHost(gate_h.ctypes.data, look_h.ctypes.data, dense_h.ctypes.data, spread_h.ctypes.data)
    cfg._ok(cfg.lib.hsw_gadget_download_region(cfg.h, C.byref(dst)))
    assert np.array_equal(gate_h[used], st["gate"][used]) and (gate_h[~used] == SENTINEL).all()
    assert np.array_equal(look_h[lused], st["lookup"].reshape(k, Lp, 4)[lused]) and (look_h[~lused] == SENTINEL).all()
    full = (gate_h.copy(), look_h.copy())
    tape = N.RegionTape()
    cfg._ok(cfg.lib.hsw_gadget_region_tape(cfg.h, C.byref(tape)))
    assert int(tape.gate_cells) == res[-1].end_cell == k * int(cfg.context_region(0).stream_cells)
    distinct = eng_int.host_empty((int(tape.distinct_capacity), 4))
    n = C.c_size_t()
    cfg._ok(cfg.lib.hsw_gadget_download_region_distinct(cfg.h, distinct.ctypes.data, distinct.shape[0], C.byref(n)))
    for a in (gate_h, look_h, dense_h, spread_h):
        a[:] = SENTINEL
    cfg._ok(cfg.lib.hsw_gadget_replay_region(cfg.h, distinct.ctypes.data, C.byref(dst), 4))
    assert np.array_equal(gate_h, full[0]) and np.array_equal(look_h, full[1])
    assert np.array_equal(dense_h.reshape(2, stride, 4)[:, : st["rows"]], st["dense"])
    assert np.array_equal(spread_h.reshape(2, stride, 4)[:, : st["rows"]], st["spread"])
    cfg.close()


def test_refusals_and_rules_on_the_device(hsw, eng_int):
    N = hsw._native
    for sizes, k, status in (([128, 64], 0, N.HSW_ERR_INVALID_ARG), ([], 3, N.HSW_ERR_INVALID_ARG), ([100], 2, N.HSW_ERR_SHAPE)):
        with pytest.raises(hsw.HswError) as ei:
            hsw.Sha256DynamicConfig(eng_int, sizes, n_contexts=k)
        assert ei.value.status == status
    cfg = hsw.Sha256DynamicConfig(eng_int, [128, 64], n_contexts=2)
    with pytest.raises(hsw.HswError) as ei:
        cfg.digest(b"no column image yet")
    assert ei.value.status == N.HSW_ERR_UNSUPPORTED
    assert cfg.set_columns(MAX_ROWS) >= 2
    with pytest.raises(hsw.HswError) as ei:
        cfg.set_digest_origin(2, 5, 0, 100000)                                    # j < M: ONE Context's digests
    assert ei.value.status == N.HSW_ERR_INVALID_ARG
    with pytest.raises(hsw.HswError) as ei:
        cfg.context_region(2)
    assert ei.value.status == N.HSW_ERR_INVALID_ARG
    assert int(cfg.context_region(1).assigned) == 0
    cfg.digest_batch([b"a", b"b", b"c"])
    assert int(cfg.context_region(0).assigned) == 1 and int(cfg.context_region(1).assigned) == 0
    cfg.close()
