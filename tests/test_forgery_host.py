"""tests/forgery.py on the host: the evaluator that judges the on-device verifier in tests/test_gpu_forgery.py agrees with
the existing checkers (tests/constraint_check.py), and the census of the compensated forgeries R1, R2, R3 -- which of
them only a range bound, only the lookup column's 16-bit bound or only the spread table rejects -- is pinned for the
fixed inputs."""
import numpy as np
import pytest

from tests import forgery as F
from tests.constraint_check import check_block_batch, check_whole_stream

MSGS, SIZES = [b"abc", bytes(range(70))], [64, 128]
TABLE8 = ([d for d in range(256)], [F.spread_of(d, 8) for d in range(256)])
_CACHE = {}


def whole(oracle, msgs=MSGS, sizes=SIZES):
    key = (tuple(msgs), tuple(sizes))
    if key not in _CACHE:
        ref = oracle.digest_cells(list(msgs), list(sizes), None, True, record=True)
        _CACHE[key] = (ref, F.ConstraintGraph.from_stream(ref))
    return _CACHE[key]


def block_inputs(seed=5, n=2):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 64), dtype=np.uint8), rng.integers(0, 2**32, (n, 8), dtype=np.uint64).astype(np.uint32)


def block(oracle, internals=False, next_state=True, blk=1):
    key = ("block", internals, next_state, blk)
    if key not in _CACHE:
        cs = oracle.constraint_system(8, 2, internals)
        blocks, pre = block_inputs()
        wit = oracle.Oracle(8, 2, check=True, internals=internals).witness_blocks(blocks, pre)
        _CACHE[key] = (cs, wit, blocks, pre, F.ConstraintGraph.from_block(cs, wit, blk, blocks, pre, next_state=next_state))
    return _CACHE[key]


def free_witnesses(ref):
    """Prologue cell 27 and epilogue cell 76 * target_round + 6 of every digest (tests/test_gpu_flip_sweep.py)."""
    out = []
    for lay in ref["layouts"]:
        epi = lay["gate0"] + lay["prologue_cells"] + lay["zero_cells"] + lay["block_cells"]
        out += [lay["gate0"] + 27, epi + 76 * lay["target_round"] + 6]
    return out


def stream_arrays(ref, g, changes):
    gate, lookup, dense, spread = ref["gate"].copy(), ref["lookup"].copy(), ref["dense"].copy(), ref["spread"].copy()
    for n, x in changes.items():
        kind, i = g.kind(n)
        cell = np.array(F.int_to_cell(x), dtype=np.uint64)
        if kind == "gate":
            gate[i] = cell
        elif kind == "lookup":
            lookup[i] = cell
        else:
            (dense if kind == "dense" else spread)[i % g.ncols, i // g.ncols] = cell
    return gate, lookup, dense, spread


def test_clean_streams_violate_nothing(oracle):
    for msgs, sizes in ((MSGS, SIZES), ([b"abc"], [64])):
        ref, g = whole(oracle, msgs, sizes)
        assert g.violated(g.values, range(g.n_nodes)) == set()
        assert g.n_gate == len(ref["gate"]) and g.n_lookup == len(ref["lookup"]) and g.n_chip == len(ref["cs"]["chip"])
    ref, g = whole(oracle)
    assert (g.n_gate, g.n_lookup, g.n_chip) == (210053, 10070, 12360)
    for internals in (False, True):
        for next_state in (False, True):
            g = block(oracle, internals, next_state)[4]
            assert g.violated(g.values, range(g.n_nodes)) == set()
            assert len(g.fixed) <= 73


def samples(g, seed, frees=()):
    """A few forgeries of every generator, accepted ones (the free witnesses) among them."""
    rng = np.random.default_rng(seed)
    nodes = list(frees)[:2] + rng.choice(g.n_free, 6, replace=False).tolist()
    roots = g.copy_classes()
    out = F.sample_by_signature(g.gen_S(nodes), 2, seed)
    out += F.sample_by_signature(g.gen_C([roots[i] for i in rng.choice(len(roots), 6, replace=False)]), 2, seed)
    for gen in (g.gen_R1, g.gen_R2, g.gen_R3):
        out += F.sample_by_signature(gen(), 1, seed)
    return out


def test_evaluator_agrees_with_check_whole_stream(oracle):
    ref, g = whole(oracle, [b"abc"], [64])
    fs = samples(g, 11, free_witnesses(ref))
    assert {f.gen for f in fs} == {"S", "C", "R1", "R2", "R3"}
    verdicts = set()
    for f in fs:
        try:
            check_whole_stream(ref, *stream_arrays(ref, g, f.changes), TABLE8)
            ok = True
        except (AssertionError, KeyError):                     # KeyError: a dense cell that is no row of the table
            ok = False
        assert ok == (not f.sig), f
        assert g.accepts(f.changes) == (not f.sig)
        verdicts.add(ok)
    assert verdicts == {True, False}


@pytest.mark.parametrize("internals", [False, True], ids=["default", "internals"])
def test_evaluator_agrees_with_check_block_batch(oracle, internals):
    cs, wit, blocks, pre, g = block(oracle, internals)
    G, LC, LK = cs["G"], cs["LC"], cs["LK"]
    # check_block_batch takes the chip cells as int64 low limbs: forgeries whose chip cells do not fit are not comparable
    fs = [f for f in samples(g, 12) if all(x < 1 << 63 for n, x in f.changes.items() if n >= g.d0)]
    assert {f.gen for f in fs} >= {"S", "C", "R1"} and len(fs) >= 12
    base_gate = wit["gate"].reshape(2, G, 4)
    chip = lambda a: np.array([[a[n % 2, n // 2, 0] for n in range(b * LC, (b + 1) * LC)] for b in range(2)]).astype(np.int64)
    base_d, base_s = chip(wit["dense"]), chip(wit["spread"])
    base_lk = wit["lookup"][:, 0].reshape(2, LK).astype(np.int64) if internals else None

    def run(changes):
        gate, d, s = base_gate.copy(), base_d.copy(), base_s.copy()
        lk = base_lk.copy() if internals else None
        for n, x in changes.items():
            kind, i = g.kind(n)
            if kind == "gate":
                gate[1, i] = np.array(F.int_to_cell(x), dtype=np.uint64)
            elif kind == "lookup":
                if x >= 1 << 63:
                    return False                               # no 16-bit entry
                lk[1, i] = x
            else:
                (d if kind == "dense" else s)[1, i] = x
        try:
            check_block_batch(np, cs, gate.view(np.int64), blocks.astype(np.int64), pre.astype(np.int64), d, s,
                              wit["next_states"].astype(np.int64), lk, TABLE8[1], 8)
            return True
        except AssertionError:
            return False
    assert run({})
    for f in fs:
        assert run(f.changes) == (not f.sig), f


def test_census_of_the_compensated_forgeries(oracle):
    """Which constraint classes reject R1, R2, R3 on the fixed inputs.  The forgeries that ONE class alone rejects are what
    the equalities of the flip sweeps never reach: 2,280 of R1 violate nothing but the 16-bit bound of the lookup-advice
    column (the limbs of range_check), every R2 and every R3 limb pair ends, after the forward repair, with nothing but the
    spread-table relation violated, and on a default-mode block whose next-state words are not given 8 of R1 (one per
    word of the final addition: word += 2^32, carry -= 1) violate nothing but a range bound."""
    ref, g = whole(oracle)
    r1 = F.census(g.gen_R1())
    assert r1 == {("const",): 2, ("const", "lookup", "range", "row"): 144, ("const", "row"): 758, ("const", "row", "table"): 12360,
                  ("lookup",): 2280, ("lookup", "range", "row"): 957, ("lookup", "row"): 2, ("range", "row"): 1608, ("row",): 7489,
                  ("row", "table"): 12360}
    assert sum(r1.values()) == 37960
    assert F.census(g.gen_R2()) == {("table",): 6180}
    assert F.census(g.gen_R3()) == {("table",): 6180}
    gb = block(oracle, False, next_state=False)[4]
    assert F.census(gb.gen_R1()) == {("row",): 2441, ("row", "table"): 4120, ("range", "row"): 821, ("const", "row"): 192, ("range",): 8}
    # with the next-state words given, those eight break the copy to the word they no longer equal
    gn = block(oracle, False, next_state=True)[4]
    assert F.census(gn.gen_R1()) == {("row",): 2441, ("row", "table"): 4120, ("range", "row"): 821, ("const", "row"): 192, ("copy", "range"): 8}


def test_whole_classes_and_single_nodes_are_rejected_by_equalities(oracle):
    """C accepts no rewrite of a copy class; S accepts exactly the rewrites of the witnesses the reference's circuit leaves
    free -- every node of the stream, every value class."""
    ref, g = whole(oracle)
    rng = np.random.default_rng(1)
    roots = g.copy_classes()
    assert len(roots) == 71003
    tried = 0
    for r in roots:
        for name, x in F.value_classes(g.values[r], rng):
            assert not g.accepts(g.class_changes([(r, x)])), (r, name)
            tried += 1
    accepted = {}
    for n in range(g.n_free):
        for name, x in F.value_classes(g.values[n], rng):
            tried += 1
            if g.accepts({n: x}):
                accepted.setdefault(n, []).append(name)
    free = free_witnesses(ref)
    assert free == [27, 69797, 70182, 209695]
    assert sorted(accepted) == free and all(len(v) == 8 for v in accepted.values()), accepted
    assert tried > 8 * 7 * (g.n_free + len(roots)) // 8


def test_value_classes_and_encodings():
    rng = np.random.default_rng(0)
    assert [n for n, _ in F.value_classes(0, rng)] == ["v+1", "p-1", "v+2^16", "v+2^64", "2^64-1", "random"]     # 0 and p - 0 are v
    assert all(0 <= x < F.P and x != 5 for _, x in F.value_classes(5, rng))
    for v in (0, 1, F.P - 1):
        m = F.to_montgomery_int(v)
        assert [x % F.P for _, x in F.encodings(v, True)] == [m, m] and all(F.P <= x < 1 << 256 for _, x in F.encodings(v, True))
        assert [n for n, _ in F.encodings(v, False)] == ["v+p", "all-ones"] and F.encodings(v, False)[0][1] == v + F.P
