"""HSW_GADGET_SHARED_CONTEXT: one halo2-base Context for the whole pass, the circuit's own cells between two digests.

The expected region is the oracle's streams of the pass as ONE Context (oracle.digest_cells), laid out by the
FlexGate model of tests/test_gpu_origin.py extended with a jump at every declared digest start and a matching shift
of the lookup queue.  Cell values do not depend on position (A1-A4) and the cached zero cell is 0 wherever it sits,
so the model is exact.  The interlude cells are the caller's: never written on the device, never touched in the
caller's host buffers."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests.test_gpu_origin import MAX_ROWS, model_columns

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


def model_shared(ref, conv, origin, landings, lq0, lk_landings):
    """The pass laid out from origin (column, row) with digest h starting at landings[h] = (column, row) (FlexGate
    columns) and its lookup entries at lk_landings[h].  Returns image, mask (both from origin column), lookup."""
    col0, row0 = origin
    starts = {lay["gate0"]: h for h, lay in enumerate(ref["layouts"])}
    gate = conv(ref["gate"])
    cols, masks, col, row, pos = {}, {}, 0, row0, 0

    def column(c):
        if c not in cols:
            cols[c] = np.zeros((MAX_ROWS, 4), dtype=np.uint64)
            masks[c] = np.zeros(MAX_ROWS, dtype=bool)
        return cols[c], masks[c]
    for ln in ref["call_lens"].tolist():
        h = starts.get(pos)
        if h is not None and h in landings:
            col, row = landings[h][0] - col0, landings[h][1]
        if row + ln >= MAX_ROWS:
            col, row = col + 1, 0
        img, m = column(col)
        img[row:row + ln] = gate[pos:pos + ln]
        m[row:row + ln] = True
        row += ln
        pos += ln
    assert pos == len(gate)
    n = max(cols) + 1
    image = np.stack([cols[c] if c in cols else np.zeros((MAX_ROWS, 4), dtype=np.uint64) for c in range(n)])
    mask = np.stack([masks[c] if c in masks else np.zeros(MAX_ROWS, dtype=bool) for c in range(n)])
    # lookup queue: digest h's entries at lk_landings.get(h, right after digest h-1's)
    lk_src = conv(ref["lookup"])
    bounds = [lay["lookup0"] for lay in ref["layouts"]] + [len(lk_src)]
    at, spans = lq0, []
    for h in range(len(ref["layouts"])):
        at = lk_landings.get(h, at)
        spans.append((at, bounds[h], bounds[h + 1]))
        at += bounds[h + 1] - bounds[h]
    lookup = np.zeros((at, 4), dtype=np.uint64)
    lmask = np.zeros(at, dtype=bool)
    for dst, a, b in spans:
        lookup[dst:dst + b - a] = lk_src[a:b]
        lmask[dst:dst + b - a] = True
    return image, mask, lookup, lmask


def write_device_cells(ptr, cells, value):
    """Write `value` into 32-byte cells `cells` of device buffer ptr (the caller's interlude cells)."""
    import torch
    t = torch.tensor(np.full(4, value, dtype=np.uint64).view(np.int64), dtype=torch.int64, device="cuda")
    hip = C.CDLL("libamdhip64.so")           # (the HIP runtime torch already loaded: 32-byte device-to-device copies)
    for c in cells:
        assert hip.hipMemcpy(C.c_void_p(ptr + 32 * c), C.c_void_p(t.data_ptr()), C.c_size_t(32), 3) == 0
    torch.cuda.synchronize()


def run_pass(hsw, eng, sizes, msgs, origin, lq0, decl, batch, mont=False, shared=True, sentinel_cells=None):
    N = hsw._native
    cfg = hsw.Sha256DynamicConfig(eng, sizes, is_input_range_check=True, whole_digest=True, shared_context=shared)
    if mont:
        cfg.set_repr(N.HSW_REPR_MONTGOMERY)
    cfg.set_origin(origin[0], origin[1], False, lq0)
    cfg.set_columns(MAX_ROWS)
    if batch:
        for h, (c, r, lk) in sorted(decl.items()):
            cfg.set_digest_origin(h, c, r, lk)
        res = cfg.digest_batch(msgs)
    else:
        res = []
        for h, m in enumerate(msgs):
            if h in decl:
                c, r, lk = decl[h]
                cfg.set_digest_origin(h, c, r, lk)
                if sentinel_cells is not None:
                    v = cfg.view()
                    write_device_cells(int(v.d_gate), sentinel_cells(h), SENTINEL)
            res.append(cfg.digest(m))
    return cfg, res


def check_region(cfg, res, ref, conv, msgs, image, mask, lookup, lmask, lq0):
    assert [r.output_bytes for r in res] == [hashlib.sha256(m).digest() for m in msgs]
    st = cfg.streams()
    assert st["gate"].shape[0] >= image.shape[0]
    g = st["gate"][: image.shape[0]]
    bad = np.nonzero((g[mask] != image[mask]).any(axis=1))[0]
    assert len(bad) == 0, "%d cells differ" % len(bad)
    assert not st["gate"][image.shape[0]:].any()
    assert np.array_equal(st["lookup"][: len(lookup)][lmask], lookup[lmask])
    assert np.array_equal(st["dense"], conv(ref["dense"])[:, : st["rows"]])
    for r, lay in zip(res, ref["layouts"]):
        assert r.prologue_cell == lay["gate0"]
    return st


CASES_1 = [("testcircuit", [128, 128], [b"abc", b""]),
           ("bench", [1024], [bytes(range(256)) * 3])]


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("case", CASES_1, ids=lambda c: c[0])
def test_flag_without_interludes_is_bit_identical(hsw, oracle, eng_int, case, mont):
    """The table path places exactly what the kernel-argument path places."""
    _, sizes, msgs = case
    out = []
    for shared in (False, True):
        cfg, res = run_pass(hsw, eng_int, sizes, msgs, (0, 0), 0, {}, batch=False, mont=mont, shared=shared)
        st = cfg.streams()
        pos = [cfg.cell_position(c) for r in res for c in (r.prologue_cell, r.block_cell, r.end_cell - 1)]
        out.append((st, pos, [r.output_bytes for r in res]))
        cfg.close()
    (a, pa, da), (b, pb, db) = out
    assert np.array_equal(a["gate"], b["gate"]) and np.array_equal(a["lookup"], b["lookup"])
    assert np.array_equal(a["dense"], b["dense"]) and np.array_equal(a["spread"], b["spread"])
    assert pa == pb and da == db
    ref = oracle.digest_cells(msgs, sizes, None, True)
    conv = oracle.to_montgomery if mont else (lambda x: x)
    img, _, _ = model_columns(ref["call_lens"], conv(ref["gate"]), MAX_ROWS)
    assert np.array_equal(b["gate"], img)


def next_free(cfg, res):
    c, r = cfg.cell_position(res.end_cell - 1)
    return c, r + 1


LANDINGS = [  # digest 1 relative to the next free cell after digest 0: (columns further, row or rows further)
    ("rows_down", 0, 7),
    ("other_column", 2, 1000),
    ("last_row", 1, MAX_ROWS - 1),
]


@pytest.mark.parametrize("batch", [False, True], ids=["per_digest", "one_batch"])
@pytest.mark.parametrize("landing", LANDINGS, ids=lambda l: l[0])
def test_interludes(hsw, oracle, eng_int, landing, batch):
    _, dcol, drow = landing
    sizes, msgs = [1024, 1024], [b"x" * 300, b"hello world"]
    origin, lq0, lk_gap = (2, 131000), 5, 9
    # where digest 0 ends: a probe pass without interludes (the layout depends on the sizes only)
    probe, pr = run_pass(hsw, eng_int, sizes, msgs[:1], origin, lq0, {}, batch=False)
    fc, fr = next_free(probe, pr[0])
    lk_free = int(probe.view().lookup_cells)
    probe.close()
    land = (fc + dcol, fr + drow if dcol == 0 else drow)
    decl = {1: (land[0], land[1], lk_free + lk_gap)}
    ref = oracle.digest_cells(msgs, sizes, None, True)
    image, mask, lookup, lmask = model_shared(ref, lambda x: x, origin, {1: land}, lq0, {1: lk_free + lk_gap})
    # the interlude's cells: image offsets from the next free cell up to the landing
    free_at, land_at = (fc - origin[0]) * MAX_ROWS + fr, (land[0] - origin[0]) * MAX_ROWS + land[1]
    probe_cells = sorted({free_at, (free_at + land_at) // 2, land_at - 1}) if land_at > free_at else []
    cfg, res = run_pass(hsw, eng_int, sizes, msgs, origin, lq0, decl, batch,
                        sentinel_cells=(lambda h: probe_cells) if not batch else None)
    st = check_region(cfg, res, ref, lambda x: x, msgs, image, mask, lookup, lmask, lq0)
    assert res[1].prologue_lookup == lk_free + lk_gap
    start = cfg.cell_position(res[1].prologue_cell)
    assert start == land if land[1] + 1 < MAX_ROWS else start[0] == land[0] + 1
    flat = st["gate"].reshape(-1, 4)
    for c in probe_cells:                                    # never written by the gadget
        assert (flat[c] == (SENTINEL if not batch else 0)).all()
    assert not st["lookup"][lk_free:lk_free + lk_gap].any()
    # deliveries: full and distinct + replay equal the model, and leave the caller's cells alone
    full = cfg.download_region()
    dist = cfg.download_region_distinct()
    for d in (full, dist):
        g = d["gate"][: image.shape[0]]
        assert np.array_equal(g[mask], image[mask])
        assert np.array_equal(d["lookup"][: len(lookup)][lmask], lookup[lmask])
    N = hsw._native
    v = cfg.view()
    gate_h = np.full((int(v.columns), MAX_ROWS, 4), SENTINEL, dtype=np.uint64)
    look_h = np.full((int(v.lookup_cells), 4), SENTINEL, dtype=np.uint64)
    dst = N.RegionHost(gate_h.ctypes.data, look_h.ctypes.data, None, None)
    cfg._ok(cfg.lib.hsw_gadget_download_region(cfg.h, C.byref(dst)))
    assert np.array_equal(gate_h[: image.shape[0]][mask], image[mask])
    assert (gate_h[: image.shape[0]][~mask] == SENTINEL).all()
    assert (look_h[lk_free:lk_free + lk_gap] == SENTINEL).all() and (look_h[:lq0] == SENTINEL).all()
    # the distinct values replayed into the caller's own (sentinel-filled) buffers: the same rule
    gate_h[:] = SENTINEL
    look_h[:] = SENTINEL
    cfg._ok(cfg.lib.hsw_gadget_replay_region(cfg.h, dist["distinct"].ctypes.data, C.byref(dst), 4))
    assert np.array_equal(gate_h[: image.shape[0]][mask], image[mask])
    assert (gate_h[: image.shape[0]][~mask] == SENTINEL).all()
    assert np.array_equal(look_h[: len(lookup)][lmask], lookup[lmask])
    assert (look_h[lk_free:lk_free + lk_gap] == SENTINEL).all() and (look_h[:lq0] == SENTINEL).all()
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    cfg.close()


@pytest.mark.parametrize("interlude", [False, True], ids=["back_to_back", "interlude"])
@pytest.mark.parametrize("k", [4, 9])
def test_wide_layouts(hsw, oracle, eng_int, k, interlude):
    """4 digests (64 blocks: the small kernel with its frame waves) and 9 (144 blocks: the streaming kernel plus
    hsw_frame_kernel), about 35 and 77 columns, as one batch."""
    sizes = [1024] * k
    rng = np.random.default_rng(k)
    msgs = [bytes(rng.integers(0, 256, int(rng.integers(0, 1015)), dtype=np.uint8)) for _ in range(k)]
    decl, land, lkl = {}, {}, {}
    if interlude:
        probe, pr = run_pass(hsw, eng_int, sizes, msgs[:k // 2], (0, 0), 0, {}, batch=True)
        fc, fr = next_free(probe, pr[-1])
        lk_free = int(probe.view().lookup_cells)
        probe.close()
        land = {k // 2: (fc + 3, 500)}
        lkl = {k // 2: lk_free + 100}
        decl = {k // 2: (fc + 3, 500, lk_free + 100)}
    ref = oracle.digest_cells(msgs, sizes, None, True)
    image, mask, lookup, lmask = model_shared(ref, lambda x: x, (0, 0), land, 0, lkl)
    cfg, res = run_pass(hsw, eng_int, sizes, msgs, (0, 0), 0, decl, batch=True)
    assert int(cfg.view().columns) >= image.shape[0] > 17
    check_region(cfg, res, ref, lambda x: x, msgs, image, mask, lookup, lmask, 0)
    rep = cfg.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    if interlude:
        # one cell of a block in a column numbered 17 or higher, behind the interlude: the verifier must see it
        r = res[k - 1]
        cell = next(c for c in range(r.block_cell, r.epilogue_cell, 997) if cfg.cell_position(c)[0] >= 17)
        col, row = cfg.cell_position(cell)
        write_device_cells(int(cfg.view().d_gate), [col * MAX_ROWS + row], np.uint64(12345))
        rep = cfg.verify()
        assert rep["violations"] >= 1, rep
    cfg.close()


def test_layout_change_between_passes(hsw, oracle, eng_int):
    """A pass with an interlude, then a pass at the same origin without one: the image, the distinct delivery (its
    witness positions follow the new layout) and the verifier all see the new layout, and nothing the first pass
    wrote past the second pass's end is left on the device."""
    sizes, msgs = [1024, 1024], [b"first pass " * 20, b"second"]
    origin, lq0 = (1, 4000), 3
    ref = oracle.digest_cells(msgs, sizes, None, True)
    cfg, res = run_pass(hsw, eng_int, sizes, msgs[:1], origin, lq0, {}, batch=False)
    fc, fr = next_free(cfg, res[0])
    lk_free = int(cfg.view().lookup_cells)
    cfg.set_digest_origin(1, fc + 2, 10, lk_free + 4)
    res.append(cfg.digest(msgs[1]))
    d1 = cfg.download_region_distinct()                       # positions of the interlude layout
    cfg.reset()
    cfg.set_origin(origin[0], origin[1], False, lq0)          # same origin: every declaration dropped
    res2 = [cfg.digest(m) for m in msgs]
    image, mask, lookup, lmask = model_shared(ref, lambda x: x, origin, {}, lq0, {})
    st = check_region(cfg, res2, ref, lambda x: x, msgs, image, mask, lookup, lmask, lq0)
    assert not st["gate"][: image.shape[0]][~mask].any()      # (the first pass's digest 1 sat further on)
    assert not st["gate"][image.shape[0]:].any()
    d2 = cfg.download_region_distinct()
    assert np.array_equal(d2["gate"][: image.shape[0]][mask], image[mask])
    assert d1["gate"].shape[0] >= image.shape[0]
    rep = cfg.verify()
    assert rep["violations"] == 0, rep
    cfg.close()
