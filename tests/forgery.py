"""Forged witnesses for the on-device verifier, and the yardstick that says which of them must be rejected.

The flip sweeps (tests/flip_sweep.py) change one limb of one cell; an equality -- a gate row, a copy, a constant -- always
catches that.  Here a forgery rewrites a node, a whole copy class or several classes at once, to values that are adversarial
to the arithmetic (p - 1, p - v, v + 2^64, ...), so that every equality can stay satisfied and only a range bound, the
16-bit bound of the lookup-advice column or the spread-table relation is left to decide.

ConstraintGraph holds the constraint STRUCTURE the oracle records from the reference's source -- of a whole-digest
stream (oracle.digest_cells(..., record=True)) or of one block (oracle.constraint_system) -- with one node per gate
cell, lookup entry, dense chip cell and spread chip cell; a block graph also holds the cells outside the block's stream
(input bytes, pre-state words, the zero cell, the next-state words) as nodes that are never rewritten.  violated()
evaluates the constraints incident to the rewritten nodes in Python integers mod p and names the classes that fail:

  row     a gate row x0 + x1*x2 = x3 (mod p)
  const   a fixed constant
  copy    a copy constraint between two gate cells, or to a cell outside the block's stream
  range   a range_check bound
  lookup  a lookup-advice entry: the copy of its source cell, below 2^16
  table   a chip cell pair: tied to its gate cells, (dense, spread) a row of the spread table

("lookup" and "table" include the ties of their cells, as the verifier reports them under VERIFY_LOOKUP and VERIFY_CHIP.)
The structure comes from the oracle only, never from the product's own hsw_block_structure / hsw_frame_structure.

Generators, all seeded, each yielding Forgery(gen, name, changes {node: value}, sig):
  S    one node takes a value of value_classes()
  C    every member of a copy class (two members or more, none outside the stream) takes the same such value
  R1   a gate row [x0, x1, c, x3] whose x2 is a non-zero constant c: class(x0) += c, class(x1) -= 1 -- the row still holds
  R2   the dense limbs of chip calls j, j + 1 of one spread call: class(dense_j) += 2^bits, class(dense_j+1) -= 1 -- their
       recomposition still holds -- then every row this breaks is repaired through the class of its output x3, 4 rounds
  R3   the same on the spread side: class(spread_j) += 2^(2 bits), class(spread_j+1) -= 1
  E    (encodings(): stored bytes, not field values) canonical v + p and all-ones; Montgomery m + p and m + 2p

Test infrastructure: pure Python and numpy."""
import numpy as np

from tests.constraint_check import P_INT, cells_to_int

P = P_INT
LABELS = ("row", "const", "copy", "range", "lookup", "table")
ROW, CONST, COPY, RANGE, LOOKUP, CHIP = range(6)
_LABEL_OF = {ROW: "row", CONST: "const", COPY: "copy", RANGE: "range", LOOKUP: "lookup", CHIP: "table"}
N_EXTERNAL = 81                     # 64 input bytes, 8 pre-state words, the zero cell, 8 next-state words
N_HARD_EXTERNAL = 73                # ... of which the next-state words are outputs: their classes are still rewritten


def spread_of(t, bits=16):
    return sum(((t >> b) & 1) << (2 * b) for b in range(bits))


class Forgery:
    """changes {node: value} (built on first use where a generator knows its signature without them), sig, where"""
    __slots__ = ("gen", "name", "_changes", "_make", "sig", "where")

    def __init__(self, gen, name, changes, sig, where=None, make=None):
        self.gen, self.name, self._changes, self._make, self.sig, self.where = gen, name, changes, make, frozenset(sig), where

    @property
    def changes(self):
        if self._changes is None:
            self._changes = self._make()
        return self._changes

    def __repr__(self):
        return "Forgery(%s %s at %s: %s)" % (self.gen, self.name, self.where, sorted(self.sig))


class _Patched:
    """values with a forgery's changes laid over them"""
    __slots__ = ("base", "ch")

    def __init__(self, base, ch):
        self.base, self.ch = base, ch

    def __getitem__(self, i):
        ch = self.ch
        return ch[i] if i in ch else self.base[i]


def value_classes(v, rng):
    """The values a rewritten node or class takes, by name; those equal to v are left out."""
    out = [("v+1", (v + 1) % P), ("0", 0), ("p-1", P - 1), ("p-v", (P - v) % P), ("v+2^16", (v + (1 << 16)) % P),
           ("v+2^64", (v + (1 << 64)) % P), ("2^64-1", (1 << 64) - 1), ("random", int.from_bytes(rng.bytes(32), "little") % P)]
    return [(n, x) for n, x in out if x != v]


def to_montgomery_int(v):
    return (v << 256) % P


def encodings(v, mont):
    """E: what a cell of value v may be stored as although it is no canonical encoding -- [(name, raw 256-bit integer)]."""
    if mont:
        m = to_montgomery_int(v)
        out = [("m+p", m + P), ("m+2p", m + 2 * P)]
    else:
        out = [("v+p", v + P), ("all-ones", (1 << 256) - 1)]
    return [(n, x) for n, x in out if x < (1 << 256)]


def int_to_cell(x):
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


class ConstraintGraph:
    def __init__(self, n_gate, n_lookup, n_chip, rows, eq, const, rng_, chip, lookup_src, values, bits, ncols, externals=False,
                 next_state_cells=()):
        self.n_gate, self.n_lookup, self.n_chip, self.bits, self.ncols = n_gate, n_lookup, n_chip, bits, ncols
        self.lk0 = n_gate
        self.d0 = self.lk0 + n_lookup
        self.s0 = self.d0 + n_chip
        self.x0 = self.s0 + n_chip
        self.n_nodes = self.x0 + (N_EXTERNAL if externals else 0)
        self.n_free = self.x0                                   # nodes [0, n_free) may be rewritten
        self.values = list(values)
        assert len(self.values) == self.n_nodes
        self.table = {d: spread_of(d, bits) for d in range(1 << bits)}
        self.rows = [int(r) for r in rows]
        self.in_row = np.zeros(n_gate, dtype=bool)
        inc = [[] for _ in range(self.n_nodes)]
        parent = list(range(self.n_nodes))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        def union(a, b):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)

        for r in self.rows:
            c = (ROW, r)
            for k in range(4):
                inc[r + k].append(c)
            self.in_row[r: r + 4] = True
        self.const = {}
        for cell, k in const:
            n = self.node(int(cell))
            if n is None:
                continue
            c = (CONST, n, int(k) % P)
            self.const[n] = int(k) % P
            inc[n].append(c)
        self.n_copy = 0
        for a, b in eq:
            na, nb = self.node(int(a)), self.node(int(b))
            if na is None or nb is None:                        # a halo2-base witness outside the stream
                continue
            c = (COPY, na, nb)
            inc[na].append(c)
            inc[nb].append(c)
            union(na, nb)
            self.n_copy += 1
        for w, cell in enumerate(next_state_cells):
            na, nb = self.node(int(cell)), self.x0 + N_HARD_EXTERNAL + w
            c = (COPY, na, nb)
            inc[na].append(c)
            inc[nb].append(c)
            union(na, nb)
        self.n_range = 0
        for cell, nbits in rng_:
            n = self.node(int(cell))
            if n is None:
                continue
            inc[n].append((RANGE, n, int(nbits)))
            self.n_range += 1
        self.lookup_src = []
        for j in range(n_lookup):
            src = self.node(int(lookup_src[j]))
            assert src is not None
            self.lookup_src.append(src)
            c = (LOOKUP, j)
            inc[self.lk0 + j].append(c)
            inc[src].append(c)
            union(self.lk0 + j, src)
        self.chip = []
        for j in range(n_chip):
            dc, sc = self.node(int(chip[j][0])), self.node(int(chip[j][1]))
            self.chip.append((dc, sc))
            c = (CHIP, j)
            inc[self.d0 + j].append(c)
            inc[self.s0 + j].append(c)
            if dc is not None:
                inc[dc].append(c)
                union(self.d0 + j, dc)
            if sc is not None:
                inc[sc].append(c)
                union(self.s0 + j, sc)
        self.inc = inc
        self._class_cache = {}
        self.cls = [find(a) for a in range(self.n_nodes)]
        self.members = {}
        for a, r in enumerate(self.cls):
            self.members.setdefault(r, []).append(a)
        # classes that hold an input byte, a pre-state word or the zero cell: never rewritten
        self.fixed = {self.cls[self.x0 + e] for e in range(N_HARD_EXTERNAL)} if externals else set()
        for r, ms in self.members.items():                       # a copy class holds one value
            assert len({self.values[m] for m in ms}) == 1, "the clean witness breaks a copy class"

    # ---- constructors -------------------------------------------------------------------------------------------
    @classmethod
    def from_stream(cls, ref, bits=8):
        """The whole-digest stream of oracle.digest_cells(..., record=True)."""
        cs = ref["cs"]
        ncols = ref["dense"].shape[0]
        n_chip = len(cs["chip"])
        g = cells_to_int(ref["gate"])
        lk = cells_to_int(ref["lookup"])
        dense = [_cell_int(ref["dense"][j % ncols, j // ncols]) for j in range(n_chip)]
        spread = [_cell_int(ref["spread"][j % ncols, j // ncols]) for j in range(n_chip)]
        assert (cs["eq"] >= 0).all() and (cs["lookup_src"] >= 0).all() and (cs["chip"] >= 0).all()
        return cls(len(g), len(lk), n_chip, ref["gate_rows"], cs["eq"].tolist(), cs["const"].tolist(), cs["range"].tolist(),
                   cs["chip"].tolist(), cs["lookup_src"].tolist(), g + lk + dense + spread, bits, ncols)

    @classmethod
    def from_block(cls, cs, wit, blk, blocks, pre, bits=8, ncols=2, next_state=True):
        """Block `blk` of Oracle.witness_blocks(blocks, pre, cursor0=0) under oracle.constraint_system's structure.
        next_state=False: the block's next-state words are not given (hsw_verify_blocks without d_next_states), so the
        cells that hold them are tied to nothing outside the stream."""
        G, LC, LK = cs["G"], cs["LC"], cs["LK"]
        has_lookup = bool((cs["lookup_src"] != -2000).all()) and wit.get("lookup") is not None
        g = cells_to_int(wit["gate"][blk * G: (blk + 1) * G])
        lk = cells_to_int(wit["lookup"][blk * LK: (blk + 1) * LK]) if has_lookup else []
        calls = [blk * LC + j for j in range(LC)]
        dense = [_cell_int(wit["dense"][n % ncols, n // ncols]) for n in calls]
        spread = [_cell_int(wit["spread"][n % ncols, n // ncols]) for n in calls]
        ext = [int(b) for b in blocks[blk]] + [int(w) for w in pre[blk]] + [0] + [int(w) for w in wit["next_states"][blk]]
        return cls(G, len(lk), LC, cs["gate_starts"], cs["eq"].tolist(), cs["const"].tolist(), cs["range"].tolist(), cs["chip"].tolist(),
                   cs["lookup_src"].tolist() if has_lookup else [], g + lk + dense + spread + ext, bits, ncols, externals=True,
                   next_state_cells=cs["next_state_cells"].tolist() if next_state else ())

    def node(self, cid):
        """The node of a structure cell id: a stream cell, or a cell outside the block's stream; None for -2000 (a
        halo2-base witness that is in no stream), as tests/constraint_check.py skips them."""
        if cid >= 0:
            return cid
        if -64 <= cid <= -1:
            return self.x0 + (-1 - cid)
        if -107 <= cid <= -100:
            return self.x0 + 64 + (-100 - cid)
        if cid == -1000:
            return self.x0 + 72
        assert cid == -2000, cid
        return None

    def kind(self, n):
        """("gate" | "lookup" | "dense" | "spread" | "external", index)"""
        for name, lo in (("external", self.x0), ("spread", self.s0), ("dense", self.d0), ("lookup", self.lk0)):
            if n >= lo:
                return name, n - lo
        return "gate", n

    # ---- the evaluator ------------------------------------------------------------------------------------------
    def _holds(self, c, v):
        t = c[0]
        if t == ROW:
            r = c[1]
            return (v[r] + v[r + 1] * v[r + 2] - v[r + 3]) % P == 0
        if t == CONST:
            return v[c[1]] == c[2]
        if t == COPY:
            return v[c[1]] == v[c[2]]
        if t == RANGE:
            return v[c[1]] < (1 << c[2])
        if t == LOOKUP:
            x = v[self.lk0 + c[1]]
            return x < 65536 and x == v[self.lookup_src[c[1]]]
        j = c[1]
        d, s = v[self.d0 + j], v[self.s0 + j]
        dc, sc = self.chip[j]
        return (dc is None or v[dc] == d) and (sc is None or v[sc] == s) and self.table.get(d, -1) == s

    def broken(self, values, touched):
        """The constraints incident to the nodes `touched` that `values` (indexable by node) violates."""
        seen, out = set(), []
        for n in touched:
            for c in self.inc[n]:
                if c not in seen:
                    seen.add(c)
                    if not self._holds(c, values):
                        out.append(c)
        return out

    def violated(self, values, touched_nodes):
        return {_LABEL_OF[c[0]] for c in self.broken(values, touched_nodes)}

    def accepts(self, changes):
        """signature(changes) is empty -- stopping at the first constraint that fails"""
        v = _Patched(self.values, changes)
        return all(self._holds(c, v) for n in changes for c in self.inc[n])

    def signature(self, changes):
        return frozenset(self.violated(_Patched(self.values, changes), changes))

    def nodes_of(self, c):
        t = c[0]
        if t == ROW:
            return (c[1], c[1] + 1, c[1] + 2, c[1] + 3)
        if t == COPY:
            return (c[1], c[2])
        if t == LOOKUP:
            return (self.lk0 + c[1], self.lookup_src[c[1]])
        if t == CHIP:
            return (self.d0 + c[1], self.s0 + c[1]) + tuple(x for x in self.chip[c[1]] if x is not None)
        return (c[1],)

    def _class_alone(self, root, x):
        """The class `root` rewritten to x and nothing else: (changes, how many constraints of every label that breaks,
        the broken constraints by node) -- kept: the zero cell's class has thousands of members and takes a handful of values."""
        key = (root, x)
        if key not in self._class_cache:
            ch = self.class_changes([key])
            count, by_node = {}, {}
            for c in self.broken(_Patched(self.values, ch), ch):
                count[c[0]] = count.get(c[0], 0) + 1
                for n in self.nodes_of(c):
                    by_node.setdefault(n, []).append(c)
            self._class_cache[key] = (ch, count, by_node)
        return self._class_cache[key]

    def class_changes(self, parts):
        ch = {}
        for root, x in parts:
            self._set_class(ch, root, x)
        return ch

    def signature_of_classes(self, parts):
        """signature(class_changes(parts)) for parts = [(root, value)]: the same set, with the largest class evaluated
        once per value where it is large.  Its constraints that touch another rewritten node are evaluated afresh."""
        big = max(parts, key=lambda rx: len(self.members[rx[0]]))
        if len(self.members[big[0]]) <= 64:
            return self.signature(self.class_changes(parts))
        small = self.class_changes([rx for rx in parts if rx is not big])
        ch, count, by_node = self._class_alone(*big)
        out = self.violated(_Patched(_Patched(self.values, ch), small), small)
        again = {c for n in small for c in by_node.get(n, ())}        # evaluated just now, with the other classes rewritten
        left = dict(count)
        for c in again:
            left[c[0]] -= 1
        return frozenset(out | {_LABEL_OF[t] for t, k in left.items() if k > 0})

    def _forgery(self, gen, name, changes, where):
        assert all(0 <= n < self.n_free and 0 <= x < P for n, x in changes.items())
        return Forgery(gen, name, changes, self.signature(changes), where)

    # ---- generators ---------------------------------------------------------------------------------------------
    def gen_S(self, nodes, seed=1):
        rng = np.random.default_rng([seed, 0])
        for n in nodes:
            for name, x in value_classes(self.values[n], rng):
                yield self._forgery("S", name, {n: x}, n)

    def copy_classes(self):
        """The roots of the classes C rewrites: two members or more, none of them outside the stream."""
        return [r for r, ms in self.members.items() if len(ms) >= 2 and r not in self.fixed and ms[0] < self.n_free]

    def _set_class(self, changes, root, x):
        for m in self.members[root]:
            if m < self.n_free:                                 # (a next-state word stays: its class is then broken)
                changes[m] = x

    def gen_C(self, roots, seed=1):
        rng = np.random.default_rng([seed, 1])
        for r in roots:
            assert r not in self.fixed
            for name, x in value_classes(self.values[r], rng):
                ch = {}
                self._set_class(ch, r, x)
                yield self._forgery("C", name, ch, r)

    def gen_R1(self):
        for r in self.rows:
            c = self.const.get(r + 2)
            if not c:
                continue
            a, b = self.cls[r], self.cls[r + 1]
            if a == b or a in self.fixed or b in self.fixed:
                continue
            parts = [(a, (self.values[r] + c) % P), (b, (self.values[r + 1] - 1) % P)]
            yield Forgery("R1", "x0+=c,x1-=1", None, self.signature_of_classes(parts), r, make=lambda parts=parts: self.class_changes(parts))

    def _gen_limbs(self, gen, base, step):
        per = 16 // self.bits                                    # limb calls of one spread call
        for j in range(self.n_chip - 1):
            if j % per == per - 1:
                continue
            a, b = self.cls[base + j], self.cls[base + j + 1]
            if a == b or a in self.fixed or b in self.fixed:
                continue
            ch = {}
            self._set_class(ch, a, (self.values[base + j] + step) % P)
            self._set_class(ch, b, (self.values[base + j + 1] - 1) % P)
            v = _Patched(self.values, ch)
            for _ in range(4):                                   # forward repair: the output of every broken row
                rows = [c[1] for c in self.broken(v, list(ch)) if c[0] == ROW]
                if not rows:
                    break
                for r in rows:
                    want = (v[r] + v[r + 1] * v[r + 2]) % P
                    if v[r + 3] != want and self.cls[r + 3] not in self.fixed:
                        self._set_class(ch, self.cls[r + 3], want)
            yield self._forgery(gen, "limb pair", ch, j)

    def gen_R2(self):
        return self._gen_limbs("R2", self.d0, 1 << self.bits)

    def gen_R3(self):
        return self._gen_limbs("R3", self.s0, 1 << (2 * self.bits))

    # ---- a forgery as arrays ------------------------------------------------------------------------------------
    def cells(self, changes):
        """(nodes, (n, 4) uint64 canonical cells) of a forgery, in node order."""
        nodes = sorted(changes)
        return nodes, np.array([int_to_cell(changes[n]) for n in nodes], dtype=np.uint64).reshape(len(nodes), 4)


def _cell_int(c):
    return int(c[0]) | (int(c[1]) << 64) | (int(c[2]) << 128) | (int(c[3]) << 192)


def census(forgeries):
    """{signature (sorted tuple): count}"""
    out = {}
    for f in forgeries:
        k = tuple(sorted(f.sig))
        out[k] = out.get(k, 0) + 1
    return out


def sample_by_signature(forgeries, per_signature, seed=3, must=()):
    """Up to per_signature forgeries of every signature that occurs (every signature is kept), seeded; `must`: predicates
    on a forgery of which one match each is added where the list holds one."""
    by = {}
    forgeries = list(forgeries)
    for f in forgeries:
        by.setdefault(tuple(sorted(f.sig)), []).append(f)
    out = []
    for k in sorted(by):
        fs = by[k]
        rng = np.random.default_rng([seed, len(fs)])
        pick = sorted(rng.choice(len(fs), size=min(per_signature, len(fs)), replace=False).tolist())
        out += [fs[i] for i in pick]
    for pred in must:
        if not any(pred(f) for f in out):
            out += [f for f in forgeries if pred(f)][:1]
    return out
