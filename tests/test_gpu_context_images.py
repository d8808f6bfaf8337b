"""HSW_GADGET_CONTEXT_IMAGES: K independent proofs of one circuit, each a FlexGate column image of its own at the
same Context origin, written by one launch.

Every proof's image, lookup column and chip rows must equal, bit for bit, both a fresh single-context gadget given
the same origin and column height, and the oracle's cells laid out by the FlexGate model of test_gpu_origin.  The
caller's cells (rows above the origin, queued lookups) are never written, on the device or in the host buffers the
deliveries fill."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.test_gpu_origin import MAX_ROWS, model_columns

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)
ROWS_PER_PROOF = 16 * 4120 // 2          # chip rows of one 16-block digest (2 columns)


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


ORIGINS = [  # (column, row, zero cell loaded, lookups queued)
    (0, 0, False, 0),
    (2, 131000, False, 5),           # the first column break falls inside the prologue
    (1, 40000, True, 1234),          # a Context that has already loaded its zero cell and queued lookups
    (0, MAX_ROWS - 1, False, 0),     # not even one cell fits: every proof starts on its next column
]


def _messages(k):
    rng = np.random.default_rng(0xC1 + k)
    return [bytes([1] * 56)] + [rng.integers(0, 256, int(rng.integers(0, 1016)), dtype=np.uint8).tobytes() for _ in range(k - 1)]


@pytest.mark.parametrize("origin", ORIGINS, ids=lambda o: "c%d_r%d_z%d_l%d" % (o[0], o[1], int(o[2]), o[3]))
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("k", [8, 9], ids=["k8_small_kernel", "k9_expand_frame"])
def test_k_proofs_as_context_images(hsw, oracle, eng_int, k, mont, origin):
    N = hsw._native
    col0, row0, zero, lq = origin
    conv = oracle.to_montgomery if mont else (lambda x: x)
    msgs = _messages(k)
    cfg = hsw.Sha256DynamicConfig(eng_int, [1024] * k, is_input_range_check=True, whole_digest=True, independent=True,
                                  context_images=True)
    one = hsw.Sha256DynamicConfig(eng_int, [1024], is_input_range_check=True, whole_digest=True)
    for g in (cfg, one):
        if mont:
            g.set_repr(N.HSW_REPR_MONTGOMERY)
        g.set_origin(col0, row0, zero, lq)
    ncols = cfg.set_columns(MAX_ROWS)
    assert one.set_columns(MAX_ROWS) == ncols

    res = cfg.digest_batch(msgs)
    assert eng_int.last_launch()["split"] == (2 if k * 16 <= 128 else 0)      # K = 8: ONE small-batch launch
    assert [r.output_bytes for r in res] == [hashlib.sha256(m).digest() for m in msgs]
    rep = cfg.verify()
    assert rep["violations"] == 0, rep
    st = cfg.streams()
    assert st["gate"].shape == (k, ncols, MAX_ROWS, 4)
    reg0 = cfg.context_region(0)
    C_, Lp = int(reg0.stream_cells), int(reg0.lookup_cells)
    assert int(reg0.columns) == ncols and int(reg0.max_rows) == MAX_ROWS and st["lookup"].shape[0] == k * Lp
    assert C_ == 1116315 - (1 if zero else 0)
    look = st["lookup"].reshape(k, Lp, 4)

    for h in (0, 1, k - 1):
        ref = oracle.digest_cells([msgs[h]], [1024], None, True, zero_cell_loaded=zero)
        img, mask, (last_col, end_row) = model_columns(ref["call_lens"], conv(ref["gate"]), MAX_ROWS, row0)
        assert img.shape[0] == ncols
        r = res[h]
        reg = cfg.context_region(h)
        assert int(reg.first_stream_cell) == h * C_ == r.prologue_cell and r.end_cell == (h + 1) * C_
        assert int(reg.assigned) == 1 and int(reg.last_column_rows) == end_row
        assert (int(reg.origin_column), int(reg.origin_row), int(reg.origin_lookups)) == (col0, row0, lq)
        assert int(reg.d_image) == int(cfg.view().d_gate) + h * ncols * MAX_ROWS * 32
        # (b) the oracle, laid out by the FlexGate model
        bad = np.nonzero((st["gate"][h] != img).any(axis=2))
        assert len(bad[0]) == 0, "proof %d, first differing (image column, row): %s" % (h, [(int(c), int(w)) for c, w in zip(*bad)][:6])
        assert not st["gate"][h, 0, :row0].any()                             # rows above the origin: the caller's
        assert np.array_equal(look[h, lq:], conv(ref["lookup"])) and not look[h, :lq].any()
        c0 = r.first_block * 4120 // 2
        assert np.array_equal(st["dense"][:, c0: c0 + ROWS_PER_PROOF], conv(ref["dense"]))
        assert np.array_equal(st["spread"][:, c0: c0 + ROWS_PER_PROOF], conv(ref["spread"]))
        # positions: FlexGate columns inside the proof's own image
        assert cfg.cell_position(r.end_cell - 1) == (col0 + last_col, end_row - 1)
        rc = N.ResultCells()
        cfg._ok(cfg.lib.hsw_gadget_result_cells(cfg.h, h, C.byref(rc)))
        c, w = int(rc.output_byte_pos[0][0]), int(rc.output_byte_pos[0][1])
        byte0 = conv(np.array([[hashlib.sha256(msgs[h]).digest()[0], 0, 0, 0]], dtype=np.uint64))[0]
        assert np.array_equal(st["gate"][h, c - col0, w], byte0)
        # (a) a fresh single-context gadget at the same origin
        one.reset()
        assert one.digest(msgs[h]).output_bytes == r.output_bytes
        s1 = one.streams()
        assert np.array_equal(s1["gate"], st["gate"][h])
        assert np.array_equal(s1["lookup"], look[h])
        assert np.array_equal(s1["dense"], st["dense"][:, c0: c0 + ROWS_PER_PROOF])
        assert np.array_equal(s1["spread"], st["spread"][:, c0: c0 + ROWS_PER_PROOF])
    one.close()

    # deliveries: sentinel-filled host buffers -- only the proofs' cells arrive, the caller's cells stay as they were
    _, mask, _ = model_columns(oracle.digest_cells([msgs[0]], [1024], None, True, zero_cell_loaded=zero)["call_lens"],
                               np.zeros((C_, 4), dtype=np.uint64), MAX_ROWS, row0)
    gate_h = np.full(st["gate"].shape, SENTINEL, dtype=np.uint64)
    look_h = np.full(st["lookup"].shape, SENTINEL, dtype=np.uint64)
    dense_h = np.full((2 * int(cfg.view().chip_col_stride), 4), SENTINEL, dtype=np.uint64)
    dst = N.RegionHost(gate_h.ctypes.data, look_h.ctypes.data, dense_h.ctypes.data, None)
    cfg._ok(cfg.lib.hsw_gadget_download_region(cfg.h, C.byref(dst)))
    assert np.array_equal(gate_h[:, mask], st["gate"][:, mask]) and (gate_h[:, ~mask] == SENTINEL).all()
    lh = look_h.reshape(k, Lp, 4)
    assert np.array_equal(lh[:, lq:], look[:, lq:]) and (lh[:, :lq] == SENTINEL).all()
    assert np.array_equal(dense_h.reshape(2, -1, 4)[:, : st["rows"]], st["dense"])
    d = cfg.download_region_distinct(threads=4)
    assert np.array_equal(d["gate"], st["gate"]) and np.array_equal(d["lookup"], st["lookup"])
    assert np.array_equal(d["dense"], st["dense"]) and np.array_equal(d["spread"], st["spread"])
    if not mont:
        with pytest.raises(hsw.HswError):
            cfg.download_region_compact()                                     # documented: not in this mode
    with pytest.raises(hsw.HswError):
        cfg.seek(1)

    # the next round of proofs on the same buffers and layout
    cfg.reset()
    res2 = cfg.digest_batch(msgs[::-1])
    assert [r.output_bytes for r in res2] == [hashlib.sha256(m).digest() for m in msgs[::-1]]
    assert cfg.verify()["violations"] == 0
    st2 = cfg.streams()
    assert np.array_equal(st2["gate"][0], st["gate"][k - 1]) and np.array_equal(st2["gate"][k - 1], st["gate"][0])
    assert np.array_equal(st2["lookup"].reshape(k, Lp, 4)[0], look[k - 1])
    cfg.close()


def test_flag_rules_on_the_device(hsw, eng_int):
    """The flag needs whole-digest + independent and K proofs of one size; without it an independent gadget still
    refuses columns and origins; context_region is for context-image gadgets only."""
    N = hsw._native
    with pytest.raises(hsw.HswError) as ei:
        hsw.Sha256DynamicConfig(eng_int, [1024] * 2, whole_digest=True, context_images=True)
    assert ei.value.status == N.HSW_ERR_INVALID_ARG
    with pytest.raises(hsw.HswError) as ei:
        hsw.Sha256DynamicConfig(eng_int, [1024, 512], whole_digest=True, independent=True, context_images=True)
    assert ei.value.status == N.HSW_ERR_UNSUPPORTED
    plain = hsw.Sha256DynamicConfig(eng_int, [1024] * 2, whole_digest=True, independent=True)
    for call in (lambda: plain.set_columns(MAX_ROWS), lambda: plain.set_origin(1, 5), lambda: plain.context_region(0)):
        with pytest.raises(hsw.HswError):
            call()
    plain.close()
    cfg = hsw.Sha256DynamicConfig(eng_int, [1024] * 2, whole_digest=True, independent=True, context_images=True)
    assert cfg.set_columns(MAX_ROWS) == 9
    with pytest.raises(hsw.HswError) as ei:
        cfg.context_region(2)
    assert ei.value.status == N.HSW_ERR_INVALID_ARG
    cfg.close()
