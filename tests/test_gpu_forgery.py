"""Soundness of the on-device verifier (hsw_gadget_verify, hsw_verify_blocks) against forged witnesses whose VALUES are
adversarial, not one bit away from valid: tests/forgery.py rewrites single nodes, whole copy classes and compensated
groups of classes (R1, R2, R3: every equality still holds, only a range bound, the lookup column's 16-bit bound or the
spread-table relation is left to object) and stores cells under non-canonical encodings (E).

The yardstick is the evaluator of tests/forgery.py -- Python integers mod p over the constraint structure the oracle
records, checked against tests/constraint_check.py in tests/test_forgery_host.py: the verifier reports a violation
exactly when the evaluator's signature is non-empty, and a forgery that one class alone rejects is reported under that
class ({"lookup"}: "lookup", {"table"}: "chip", {"range"}: "range").  Encodings are always rejected, free witnesses
included; the free witnesses themselves (tests/test_gpu_flip_sweep.py) accept any value.

Every forgery is written in place, verified, and restored; afterwards the region verifies and every tensor equals its
snapshot.  Samples: up to PER forgeries of every (generator, signature) pair, every signature kept, plus up to PER_FRAME of
every pair among the forgeries seeded in a prologue or an epilogue (the frame verifier has range and lookup code of its
own).  R2 and R3 are seeded at chip cells, which only blocks have: none falls in a frame, and the test asserts that."""
import numpy as np
import pytest

from tests import forgery as F
from tests.flip_sweep import OwnedMemory
from tests.test_forgery_host import MSGS, SIZES, block, block_inputs, free_witnesses, whole

pytestmark = pytest.mark.gpu
PER, PER_FRAME = 40, 8
ATTRIBUTED = {frozenset({"lookup"}): "lookup", frozenset({"table"}): "chip", frozenset({"range"}): "range"}
FORMS = pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
_SAMPLES = {}


class Cells:
    """Where the nodes of a graph lie in device memory, and a forgery written there and taken back.
    gate, lookup: (tensor, first index); dense, spread: per chip column (tensor, first row); call0: the absolute limb call
    of the graph's chip node 0."""

    def __init__(self, g, oracle, mont, gate, lookup, dense, spread, call0=0):
        self.g, self.oracle, self.mont, self.call0 = g, oracle, mont, call0
        self.gate, self.lookup, self.dense, self.spread = gate, lookup, dense, spread

    def _groups(self, nodes):
        """[(tensor, indices, positions in nodes)]"""
        g, n = self.g, np.asarray(nodes, dtype=np.int64)
        assert len(n) and n.min() >= 0 and n.max() < g.n_free
        out = []
        m = n < g.lk0
        if m.any():
            out.append((self.gate[0], self.gate[1] + n[m], np.nonzero(m)[0]))
        m = (n >= g.lk0) & (n < g.d0)
        if m.any():
            out.append((self.lookup[0], self.lookup[1] + n[m] - g.lk0, np.nonzero(m)[0]))
        for lo, hi, cols in ((g.d0, g.s0, self.dense), (g.s0, g.x0, self.spread)):
            call = self.call0 + n - lo
            for k, (t, row0) in enumerate(cols):
                m = (n >= lo) & (n < hi) & (call % g.ncols == k)
                if m.any():
                    out.append((t, row0 + call[m] // g.ncols, np.nonzero(m)[0]))
        assert sum(len(x[2]) for x in out) == len(n)
        return out

    def write(self, nodes, cells, raw=False):
        """cells: (n, 4) uint64 -- field values (stored in the form in force), or raw: the stored limbs themselves.
        Returns what restore() takes."""
        import torch
        cells = np.ascontiguousarray(cells, dtype=np.uint64)
        if self.mont and not raw:
            cells = self.oracle.to_montgomery(cells)
        saved = []
        for t, idx, pos in self._groups(nodes):
            assert idx.min() >= 0 and idx.max() < t.shape[0]
            ti = torch.from_numpy(np.ascontiguousarray(idx)).to(t.device)
            saved.append((t, ti, t[ti].clone()))
            t[ti] = torch.from_numpy(cells[pos].view(np.int64)).to(t.device)
        return saved

    @staticmethod
    def restore(saved):
        for t, ti, old in saved:
            t[ti] = old

    def forge(self, f):
        nodes = sorted(f.changes)
        cell_of = {}
        for x in set(f.changes.values()):
            cell_of[x] = F.int_to_cell(x)
        return self.write(nodes, np.array([cell_of[f.changes[n]] for n in nodes], dtype=np.uint64).reshape(len(nodes), 4))


def judge(cells, verify, forgeries, first_block=None):
    """Every forgery written, verified and restored: the verdicts and attributions that differ from the evaluator's."""
    wrong = []
    for f in forgeries:
        saved = cells.forge(f)
        rep = verify()
        cells.restore(saved)
        if (rep["violations"] >= 1) != bool(f.sig):
            wrong.append(("accepted" if f.sig else "rejected", f, rep))
        elif f.sig in ATTRIBUTED and rep["first_class"] != ATTRIBUTED[f.sig]:
            wrong.append(("attributed to " + str(rep["first_class"]), f, rep))
        elif f.sig and first_block is not None and rep["first_block"] != first_block:
            wrong.append(("in block %d" % rep["first_block"], f, rep))
    return wrong


def judge_encodings(cells, verify, g, nodes, mont):
    """E: every node of `nodes` under every non-canonical encoding of its own value -- the ones that were accepted."""
    accepted, tried = [], 0
    for n in nodes:
        for name, raw in F.encodings(g.values[n], mont):
            saved = cells.write([n], np.array([F.int_to_cell(raw)], dtype=np.uint64), raw=True)
            rep = verify()
            cells.restore(saved)
            tried += 1
            if rep["violations"] == 0:
                accepted.append((g.kind(n), name))
    assert tried >= len(nodes)
    return accepted


# ---- whole digests ----------------------------------------------------------------------------------------------------
def sections(ref):
    """[(name, first gate cell, end, first lookup entry, end)] of the stream, in order."""
    out = []
    for lay in ref["layouts"]:
        c, k = lay["gate0"], lay["lookup0"]
        for name, cells, lks in (("prologue", lay["prologue_cells"], lay["prologue_lookups"]), ("zero", lay["zero_cells"], 0),
                                 ("block", lay["block_cells"], lay["block_lookups"]), ("epilogue", lay["epilogue_cells"], lay["epilogue_lookups"])):
            out.append((name, c, c + cells, k, k + lks))
            c, k = c + cells, k + lks
    return out


def whole_sample(oracle):
    if "whole" in _SAMPLES:
        return _SAMPLES["whole"]
    ref, g = whole(oracle)
    secs = sections(ref)
    assert secs[-1][2] == g.n_gate and secs[-1][4] == g.n_lookup

    def section_of(n):
        kind, i = g.kind(n)
        if kind in ("dense", "spread"):
            return "block"
        return [s[0] for s in secs if (s[1] <= i < s[2] if kind == "gate" else s[3] <= i < s[4])][0]
    rng = np.random.default_rng(21)
    frame_gate = [c for s in secs if s[0] in ("prologue", "epilogue") for c in range(s[1], s[2])]
    frame_lk = [g.lk0 + k for s in secs if s[0] in ("prologue", "epilogue") for k in range(s[3], s[4])]
    zero = [s[1] for s in secs if s[0] == "zero" and s[2] > s[1]]
    free = free_witnesses(ref)
    pick = lambda xs, k: [xs[i] for i in sorted(rng.choice(len(xs), min(k, len(xs)), replace=False).tolist())]
    nodes = free + zero + pick(frame_gate, 150) + pick(frame_lk, 40) + pick(range(g.n_free), 300)
    out = {}
    s_all = list(g.gen_S(nodes, seed=2))
    out["S"] = F.sample_by_signature(s_all, PER, 3)
    roots = g.copy_classes()
    in_frames = [r for r in roots if section_of(r) != "block"]
    out["C"] = F.sample_by_signature(g.gen_C(pick(roots, 150) + pick(in_frames, 60), seed=2), PER, 3)
    for name, gen in (("R1", g.gen_R1), ("R2", g.gen_R2), ("R3", g.gen_R3)):
        fs = list(gen())
        seeded = {"R1": lambda f: section_of(f.where), "R2": lambda f: section_of(g.d0 + f.where), "R3": lambda f: section_of(g.s0 + f.where)}[name]
        framed = [f for f in fs if seeded(f) != "block"]
        if name == "R1":
            assert {seeded(f) for f in framed} == {"prologue", "epilogue"}
        else:
            assert framed == []                                 # chip cells belong to blocks
        out[name] = F.sample_by_signature(fs, PER, 3)
        chosen = set(map(id, out[name]))
        for sec in ("prologue", "epilogue"):
            out[name] += [f for f in F.sample_by_signature([f for f in framed if seeded(f) == sec], PER_FRAME, 4) if id(f) not in chosen]
    # every single-class signature the generators reach is in the sample
    for name, fs in (("S", s_all),):
        assert {f.sig for f in fs} == {f.sig for f in out[name]}
    sigs = {f.sig for fs in out.values() for f in fs}
    # (in internals mode a range bound never stands alone: range_check's limbs, tied by rows, are lookup entries too --
    # {"range"} alone is reached on default-mode blocks, below)
    assert frozenset({"lookup"}) in sigs and frozenset({"table"}) in sigs and frozenset({"range"}) not in sigs, sigs
    assert any(f.sig == frozenset({"lookup"}) and f.gen == "R1" for f in out["R1"])
    assert any(f.sig == frozenset({"table"}) for f in out["R2"]) and any(f.sig == frozenset({"table"}) for f in out["R3"])
    assert any(not f.sig for f in out["S"])                     # the free witnesses: accepted
    enc = free + zero + pick(frame_gate, 24) + pick(frame_lk, 8) + pick(range(g.n_gate), 12) + pick(range(g.lk0, g.d0), 4) + \
        pick(range(g.d0, g.s0), 4) + pick(range(g.s0, g.x0), 4)
    _SAMPLES["whole"] = (ref, g, out, free, enc)
    return _SAMPLES["whole"]


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


@FORMS
def test_whole_digest_forgeries(hsw, oracle, eng_int, mont):
    import torch
    ref, g, sample, free, enc = whole_sample(oracle)
    cfg = hsw.Sha256DynamicConfig(eng_int, SIZES, is_input_range_check=True, whole_digest=True)
    try:
        if mont:
            cfg.set_repr(hsw._native.HSW_REPR_MONTGOMERY)
        cfg.digest_batch(MSGS)
        v = cfg.view()
        assert int(v.gate_cells) == g.n_gate and int(v.lookup_cells) == g.n_lookup and int(v.num_limb_sum) == g.n_chip
        mem = OwnedMemory(cfg)
        cells = Cells(g, oracle, mont, (mem.image[0], 0), (mem.look[0], 0), [(t, 0) for t in mem.dense[0]], [(t, 0) for t in mem.spread[0]])
        assert cfg.verify()["violations"] == 0
        torch.cuda.synchronize()
        snaps = [t.clone() for t in mem.tensors()]
        # the region holds the oracle's cells: a node is where the graph says it is
        got = mem.image[0].cpu().numpy().view(np.uint64)
        assert np.array_equal(got, oracle.to_montgomery(ref["gate"]) if mont else ref["gate"])
        for name, fs in sorted(sample.items()):
            wrong = judge(cells, cfg.verify, fs)
            print("%s: %d forgeries, %d signatures, %d wrong" % (name, len(fs), len({f.sig for f in fs}), len(wrong)))
            assert wrong == [], (name, wrong[:5])
        # free witnesses: any value is accepted (z + 0 * inv = 1 holds for every inv); no encoding is
        rnd = int.from_bytes(np.random.default_rng(9).bytes(32), "little") % F.P
        for n in free:
            for x in (0, 1, F.P - 1, rnd):
                saved = cells.write([n], np.array([F.int_to_cell(x)], dtype=np.uint64))
                rep = cfg.verify()
                cells.restore(saved)
                assert rep["violations"] == 0, (n, hex(x), rep)
        accepted = judge_encodings(cells, cfg.verify, g, enc, mont)
        assert accepted == [], "stored under a non-canonical encoding and accepted: %s" % accepted
        rep = cfg.verify()
        assert rep["violations"] == 0, rep
        torch.cuda.synchronize()
        for t, s in zip(mem.tensors(), snaps):
            assert torch.equal(t, s), "a forgery was left in place"
    finally:
        cfg.close()


# ---- block streams ----------------------------------------------------------------------------------------------------
def block_sample(oracle):
    if "block" in _SAMPLES:
        return _SAMPLES["block"]
    g = block(oracle, False, True)[4]
    gn = block(oracle, False, False)[4]                         # the same block, its next-state words not given
    assert len(g.fixed) <= 73 and g.fixed == gn.fixed
    rng = np.random.default_rng(22)
    pick = lambda xs, k: [xs[i] for i in sorted(rng.choice(len(xs), min(k, len(xs)), replace=False).tolist())]
    no_row = np.nonzero(~g.in_row)[0].tolist()
    assert len(no_row) == 12268
    out = {}
    r1 = list(gn.gen_R1())
    out["R1 range only, no next state"] = [f for f in r1 if f.sig == frozenset({"range"})]
    assert len(out["R1 range only, no next state"]) == 8
    out["R1"] = F.sample_by_signature(g.gen_R1(), PER, 3)
    out["C"] = F.sample_by_signature(g.gen_C(pick(g.copy_classes(), 150), seed=2), PER, 3)
    out["S"] = F.sample_by_signature(g.gen_S(pick(range(g.n_free), 300), seed=2), PER, 3)
    s_no_row = list(g.gen_S(no_row, seed=2))                   # every cell in no gate row, every value class: sampled by signature
    out["S, cells in no gate row"] = F.sample_by_signature(s_no_row, PER, 3)
    assert {f.sig for f in s_no_row} == {f.sig for f in out["S, cells in no gate row"]}
    _SAMPLES["block"] = (g, gn, out, [no_row[0], no_row[-1]] + pick(no_row, 40) + pick(range(g.n_free), 20))
    return _SAMPLES["block"]


@FORMS
def test_block_stream_forgeries(hsw, oracle, engine_factory, kernel_choice, mont):
    import torch
    g, gn, sample, enc = block_sample(oracle)
    eng = engine_factory(8, 2)
    blocks, pre = block_inputs()
    tb, tp = torch.from_numpy(blocks).cuda(), torch.from_numpy(pre.view(np.int32)).cuda()
    flags = hsw._native.HSW_REPR_MONTGOMERY if mont else 0
    out = eng.witness_blocks(tb, tp, cursor0=0, flags=flags)
    eng.synchronize()
    G, LC, blk = eng.G, eng.limb_calls, 1
    assert (G, LC) == (g.n_gate, g.n_chip) and g.n_lookup == 0
    cells = Cells(g, oracle, mont, (out["gate"], blk * G), None, [(out["dense"][k], 0) for k in range(2)],
                  [(out["spread"][k], 0) for k in range(2)], call0=blk * LC)
    tensors = [out["gate"], out["dense"], out["spread"], out["next_states"]]
    verify = lambda **kw: eng.verify_blocks(tb, tp, out, cursor0=0, flags=flags, **kw)
    assert verify()["violations"] == 0
    torch.cuda.synchronize()
    snaps = [t.clone() for t in tensors]
    for name, fs in sorted(sample.items()):
        if name.endswith("no next state"):
            wrong = judge(cells, lambda: verify(check_next=False), fs, first_block=blk)
            # with the next-state words given the same rewrites also break the copy to their word
            for f in fs:
                saved = cells.forge(f)
                rep = verify()
                cells.restore(saved)
                if rep["violations"] == 0:
                    wrong.append(("accepted with next states", f, rep))
        else:
            wrong = judge(cells, verify, fs, first_block=blk)
        print("%s: %d forgeries, %d signatures, %d wrong" % (name, len(fs), len({f.sig for f in fs}), len(wrong)))
        assert wrong == [], (name, wrong[:5])
    accepted = judge_encodings(cells, verify, g, enc, mont)
    assert accepted == [], "stored under a non-canonical encoding and accepted: %s" % accepted
    assert verify()["violations"] == 0
    torch.cuda.synchronize()
    for t, s in zip(tensors, snaps):
        assert torch.equal(t, s), "a forgery was left in place"
