"""Completeness of hsw_gadget_verify on the layouts that have a verifier instantiation and address arithmetic of their
own: a seeded sample of single-cell corruptions (tests/flip_sweep.py: select_cells, sweep_layout) of every Context and
every digest of

  a  a whole-digest Context at a FlexGate origin in columns          the pack-plan path, a break inside a frame
  b  a shared context with an interlude before digest 1               the TABLE verifier, per-digest lookup offsets
  c  b with the interlude pushed past 17 columns                      a long jump table
  d  K = 3 context images at an origin with queued lookups            the period, Lp steps
  e  a Context group, K = 3 x [128, 64] with an interlude             ctx_blocks, frame_every
  f  e bound with bind_region, pitch 2^17, one slab per proof         Layout::pitch, chip_ctx_extra
  g  e bound with bind_columns, columns in permuted address order     WIDE gate reads through cum rows
  h  e bound with bind_column_tables, every column by pointer         WIDE with lk_row, chip_row

each in canonical and Montgomery form.  Per section (prologue, every block, epilogue) the sample holds the first and the
last cell, both neighbours of every jump, seeded random cells, the zero cell and the free witnesses; per lookup run and
per block's chip cells the first, the last and random ones.

Every corruption must be reported, inside the owning digest's blocks and -- chip and lookup cells -- under its own
class, except the two witnesses per digest that tests/test_gpu_flip_sweep.py documents as free in the reference's own
circuit: the inverse witness of the prologue's is_zero(limb1) (lib.rs:142-143, prologue cell 27) and of the epilogue's
is_equal of the selected round (lib.rs:296-310, epilogue cell 76 * target_round + 6).  The miss list of every case is
exactly those.  No other cell is excluded.

The shapes are the smallest that reach each path: 8-bit table, 2 chip columns, digests of [128, 64] bytes (2 + 1 blocks of
69,348 cells), columns of 70,001 rows -- a block fits a column with 652 rows to spare, so a Context of three blocks spans
four columns and every block that does not start in the first 653 rows of its column breaks.  The interlude follows the
recipe of interlude_after_digest0 of tests/test_gpu_bound_region.py (that function itself lays its probe out in columns
of 2^17 - 9 rows): `push` columns past digest 0's last cell, row 41, 11 caller lookups in between."""
import sys
import time

import pytest

from tests.flip_sweep import CallerMemory, OwnedMemory, add_p, free_witnesses, layout_facts, select_cells, sweep_layout
from tests.test_gpu_bound_column_tables import CarvedAll
from tests.test_gpu_bound_columns import Carved, interleaved
from tests.test_gpu_bound_region import N17, Slabs, eng_int  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
MAX_ROWS = 70001
SIZES, K = [128, 64], 3
LENGTHS = [(60, 3), (100, 20), (119, 55)]                     # per Context: 2 of 2 rounds selected, then 1 of 1 ("abc"-like)

# The origin rows, chosen so that jumps fall strictly inside every kind of section (asserted from cell_position):
#   69700  the prologue of digest 0 (686 cells) runs over the end of its column, and so does every block after it
#   100    block 0 runs 136 cells over its column; block 1 then ends on row 69484 and the epilogue of digest 0 (516 cells)
#          ends on the column's last row: the break falls at the edge, before digest 1's first cell
#   200    (one digest per Context) the same with block 1 ending on row 69584: the break falls inside the epilogue
#   41     the interlude's row: digest 1's epilogue starts on row 69755 and breaks after 244 cells
# `inside`: the kinds of section that hold a jump strictly inside, as the layout walk gives them for these rows.
ALL = {"prologue", "block", "epilogue"}
CASES = {
    "a": dict(kind="whole", origin=(2, 69700, False, 5), inside={"prologue", "block"}),
    "b": dict(kind="shared", origin=(1, 100, False, 5), push=3, inside={"block", "epilogue"}),
    "c": dict(kind="shared", origin=(1, 69700, False, 5), push=16, inside=ALL),
    "d": dict(kind="images", origin=(1, 200, False, 3), inside={"block", "epilogue"}),
    "e": dict(kind="group", origin=(1, 100, False, 5), push=3, inside={"block", "epilogue"}),
    "f": dict(kind="group", origin=(1, 69700, False, 5), push=3, bind="region", inside=ALL),
    "g": dict(kind="group", origin=(1, 100, False, 5), push=3, bind="columns", inside={"block", "epilogue"}),
    "h": dict(kind="group", origin=(1, 69700, False, 5), push=3, bind="tables", inside=ALL),
}
assert set.union(*[c["inside"] for c in CASES.values()]) == ALL


def message(c, d, n):
    return bytes((31 * c + 7 * d + i) % 251 for i in range(n))


def messages(kind):
    """One list per Context.  Context images hold one digest of 128 bytes per proof: Context 1's selects round 1 of 2."""
    if kind == "images":
        return [[message(c, 0, n)] for c, n in enumerate((60, 3, 119))]
    return [[message(c, d, n) for d, n in enumerate(LENGTHS[c])] for c in range(K if kind == "group" else 1)]


def create(hsw, eng, kind, origin, mont, decl=None):
    if kind == "whole":
        cfg = hsw.Sha256DynamicConfig(eng, SIZES, True, whole_digest=True)
    elif kind == "shared":
        cfg = hsw.Sha256DynamicConfig(eng, SIZES, True, whole_digest=True, shared_context=True)
    elif kind == "images":
        cfg = hsw.Sha256DynamicConfig(eng, SIZES[:1] * K, True, whole_digest=True, independent=True, context_images=True)
    else:
        cfg = hsw.Sha256DynamicConfig(eng, SIZES, True, n_contexts=K)
    if mont:
        cfg.set_repr(hsw._native.HSW_REPR_MONTGOMERY)
    cfg.set_origin(*origin)
    cfg.set_columns(MAX_ROWS)
    if decl:
        cfg.set_digest_origin(*decl)
    return cfg


def interlude_before_digest1(hsw, eng, origin, push):
    """The declaration for digest 1: `push` columns past digest 0's last cell, row 41, 11 caller lookups in between."""
    probe = create(hsw, eng, "shared", origin, False)
    r = probe.digest(b"x")
    c, _ = probe.cell_position(r.end_cell - 1)
    lk = int(probe.view().lookup_cells)
    probe.close()
    return (1, c + push, 41, lk + 11)


_LINEAR = {}


def linear_checks(hsw, eng, sizes, msgs):
    """rep["checks"] of a plain linear whole-digest gadget fed msgs: the same constraint system, no placement."""
    key = (tuple(sizes), tuple(msgs))
    if key not in _LINEAR:
        ref = hsw.Sha256DynamicConfig(eng, list(sizes), True, whole_digest=True)
        ref.digest_batch(list(msgs))
        rep = ref.verify()
        ref.close()
        assert rep["violations"] == 0 and rep["checks"] > 0, rep
        _LINEAR[key] = rep["checks"]
    return _LINEAR[key]


def permuted(cols):
    """Address order of the image columns: the odd ones descending, then the even ones ascending (8 columns: 7 5 3 1 0 2
    4 6) -- column 1 lies below column 0, column 3 above column 2."""
    return list(range(cols - 1 - cols % 2, 0, -2)) + list(range(0, cols, 2))


def build(hsw, eng, case, mont):
    """The finished pass of one case: (cfg, results, memory, Contexts, what the binding keeps alive)."""
    spec = CASES[case]
    kind, origin = spec["kind"], spec["origin"]
    contexts = K if kind in ("images", "group") else 1
    decl = interlude_before_digest1(hsw, eng, origin, spec["push"]) if "push" in spec else None
    cfg = create(hsw, eng, kind, origin, mont, decl)
    cols = int(cfg.view().columns)
    bind, keep, mem = spec.get("bind"), None, None
    if bind == "region":
        keep = sl = Slabs(cfg, K, N17)
        cfg.bind_region(**sl.kw)
        mem = CallerMemory(sl.t, lambda c, k, row: c * sl.slab + k * sl.pitch + row, lambda c, j: c * sl.slab + sl.o_lk + j,
                           lambda fam, c, k, row: c * sl.slab + (sl.o_cd if fam == "dense" else sl.o_cs) + k * sl.pitch + row)
    elif bind == "columns":
        keep = cv = Carved(K, cols, interleaved(K, cols, permuted(cols)))
        assert any(cv.start[(1, k + 1)] < cv.start[(1, k)] for k in range(cols - 1)) and any(cv.start[(1, k + 1)] > cv.start[(1, k)] for k in range(cols - 1))
        cfg.bind_columns(**cv.kw)
        mem = CallerMemory(cv.t, lambda c, k, row: cv.start[(c, k)] + row, lambda c, j: cv.o_lk + c * cv.per_proof + j,
                           lambda fam, c, k, row: cv.o_lk + c * cv.per_proof + ((1 if fam == "dense" else 3) + k) * cv.area + row)
    elif bind == "tables":
        b = cfg.region_binding()
        keep = cv = CarvedAll(K, cols, interleaved(K, cols, permuted(cols)), int(b.lookup_capacity), int(b.chip_rows_capacity))
        cfg.bind_columns(**cv.kw)
        mem = CallerMemory(cv.t, lambda c, k, row: cv.start[(c, k)] + row, lambda c, j: cv.lk[c] + j,
                           lambda fam, c, k, row: cv.chip[(fam, c, k)] + row)
    msgs = messages(kind)
    res = cfg.digest_batch([m for ctx in msgs for m in ctx])
    if mem is None:
        mem = OwnedMemory(cfg, contexts)
    return cfg, res, mem, contexts, msgs, keep


def run_case(hsw, eng, case, mont, log=None, mutate=None):
    """One case, with what it asserts about itself; returns sweep_layout's counts (+ "expected": the free witnesses).
    mutate: sweep_layout's, instead of the limb flip."""
    spec = CASES[case]
    cfg, res, mem, contexts, msgs, keep = build(hsw, eng, case, mont)
    try:
        li = eng.last_launch()
        # g, h: the pass went through the wide instantiations.  hsw_last_launch records the expansion launch; the verifier
        # takes its PlaceTable from the same launch builder and picks its wide kernels on the same cum_stride.
        assert bool(li["split"] & 4) == (spec.get("bind") in ("columns", "tables")), li
        cols = int(cfg.view().columns)
        assert (cols > 17) == (case == "c"), cols
        # the clean pass: as many checks as the same digests on a plain linear stream, Context by Context
        rep = cfg.verify()
        sizes = SIZES[:1] if spec["kind"] == "images" else SIZES
        want = sum(linear_checks(hsw, eng, sizes, ctx) for ctx in msgs)
        print("case %s: columns %d, checks %d, linear %d" % (case, cols, rep["checks"], want))
        assert rep["violations"] == 0 and rep["checks"] == want, (rep, want)
        # the sample and where its jumps fall
        facts = layout_facts(cfg, res, contexts)
        inside = {s["name"].rstrip("0123456789") for ctx in facts for dg in ctx for s in dg if any(0 < j < s["cells"] for j in s["jumps"])}
        jumps = sorted({(d, s["name"], j) for ctx in facts for d, dg in enumerate(ctx) for s in dg for j in s["jumps"]})
        print("case %s: jumps (digest, section, offset) %s" % (case, jumps))
        assert inside == spec["inside"], (inside, jumps)
        cells = select_cells(facts, seed=5, n_random=2 if mont else 8)
        free = free_witnesses(res, contexts)
        assert len(free) == 2 * len(res) and set(free) <= set(cells) and len(set(cells)) == len(cells)
        assert {c[0] for c in cells} == set(range(contexts))
        for c, ctx in enumerate(facts):                       # every Context assigns its zero cell here: it is in the sample
            assert ctx[0][0]["zero"] is not None and (c, 0, "prologue", ctx[0][0]["zero"]) in cells
        out = sweep_layout(cfg, res, cells, mem, contexts, mont=mont, log=log, name="%s %s" % (case, "mont" if mont else "canon"), mutate=mutate)
        out["expected"] = free
        print("case %s %s: %d cells tried, %d missed, %.2f s" % (case, "montgomery" if mont else "canonical", out["tested"], len(out["missed"]), out["seconds"]))
        return out
    finally:
        cfg.close()
        del keep


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_sampled_corruptions_leave_only_the_free_witnesses(hsw, eng_int, case, mont):
    out = run_case(hsw, eng_int, case, mont)
    assert out["misattributed"] == []
    assert sorted(out["missed"]) == sorted(out["expected"]), "missed, not free: %s; free, but reported: %s" % (
        sorted(set(out["missed"]) - set(out["expected"])), sorted(set(out["expected"]) - set(out["missed"])))


@pytest.mark.parametrize("case", ["b", "h"])
def test_non_canonical_montgomery_encodings_are_never_free(hsw, eng_int, case):
    """The same sample with every cell stored as m + p instead of flipped: the value does not change, so no equality
    sees it -- only the rule that a Montgomery cell is an encoding m < p.  b: the TABLE frame kernel, h: the WIDE one.
    An encoding is never free: the free witnesses are reported too."""
    out = run_case(hsw, eng_int, case, True, mutate=add_p)
    assert out["misattributed"] == []
    assert out["missed"] == [], "stored as m + p and accepted: %s" % out["missed"]


def run_all(log=sys.stdout):
    """python tests/flip_sweep.py layouts: every case in both forms, one line each."""
    import importlib
    hsw = importlib.import_module("halo2-dynamic-sha256_amd")
    eng = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    bad = 0
    try:
        for case in sorted(CASES):
            for mont in (False, True):
                t0 = time.time()
                out = run_case(hsw, eng, case, mont, log=log)
                extra = sorted(set(out["missed"]) ^ set(out["expected"]))
                bad += len(extra) + len(out["misattributed"])
                if extra or out["misattributed"]:
                    print("  not as expected: %s %s  (%.0f s)" % (extra[:20], out["misattributed"][:20], time.time() - t0), file=log, flush=True)
    finally:
        eng.close()
    return bad
