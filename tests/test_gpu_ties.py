"""Digest-to-digest copy constraints on the device: hsw_gadget_ties lists them, hsw_gadget_cell_address resolves a
cell in every layout and binding, hsw_verify_pairs_kernel (hsw_gadget_verify_ties / hsw_gadget_verify_equal) compares
the cells.

The yardstick is exact: the tie list against the tree's shape, every tied cell -- read back through its own address --
against the digest byte hashlib gives (canonical, or its Montgomery form computed here), addresses against the
position arithmetic of the binding in force, and violation counts that follow from what the test itself overwrote in
its OWN nodes tensor.  Nothing here writes outside the test's tensors."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_device_inputs import device_messages, int_engines, rand  # noqa: F401 (fixture)
from tests.test_gpu_device_levels import filled, host, merkle, sha
from tests.test_gpu_origin import MAX_ROWS

pytestmark = pytest.mark.gpu
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # BN254 scalar field
LEAF_LENS = (0, 1, 55, 56, 63, 64, 100, 119)
PITCH = MAX_ROWS + 12
STEP = (PITCH + 7) & ~3                 # cells from one caller column to the next: 128-byte aligned starts
_TREES = {}


def tree(seed):
    """(leaves, messages, nodes bytes) of the 8-leaf tree with this seed: hashed on the host once, then shared."""
    if seed not in _TREES:
        leaves = [rand(seed + n, n) for n in LEAF_LENS]
        _TREES[seed] = (leaves,) + merkle(leaves)
    return _TREES[seed]


def tree_ties(first=0):
    """The ties of an 8-leaf tree whose 15 digests start at digest `first`, in (dst_hash, dst_byte) order."""
    out, parent, below, width = [], 8, 0, 8
    while width > 1:
        for j in range(width // 2):
            out += [(first + below + 2 * j + k // 32, first + parent, k % 32, k) for k in range(64)]
            parent += 1
        below, width = below + width, width // 2
    return out


def tree_call(base, slices):
    """merkle_tree_device's arguments for one tree whose nodes start at device address `base`."""
    inputs, levels, below, width, level = list(slices), [0] * 8, 0, 8, 0
    while width > 1:
        level += 1
        inputs += [(base + 32 * (below + 2 * j), 64) for j in range(width // 2)]
        levels += [level] * (width // 2)
        below, width = below + width, width // 2
    return inputs, levels, [base + 32 * k for k in range(15)]


def cell_words(byte, mont):
    v = (byte << 256) % P if mont else byte
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


def peek(cfg, cell):
    a = np.zeros(4, dtype=np.uint64)
    cfg._ok(cfg.lib.hsw_download(cfg.engine.h, a.ctypes.data, cfg.cell_address(int(cell)), 32))
    return [int(x) for x in a]


def result_cells(hsw, cfg, idx):
    rc = hsw._native.ResultCells()
    cfg._ok(cfg.lib.hsw_gadget_result_cells(cfg.h, idx, C.byref(rc)))
    return rc


def as_tuples(ties):
    return [(int(t["src_hash"]), int(t["dst_hash"]), int(t["src_byte"]), int(t["dst_byte"])) for t in ties]


def break_inside_parent8(hsw):
    """Column height that puts the first FlexGate break in the middle of digest 8's input bytes: they are single-cell
    calls, so with R rows stream cell R - 1 is the first of column 1 (row + 1 >= R) and nothing before it breaks."""
    N = hsw._native
    fs = N.frame_query(N.shape_query(8, 2, N.HSW_MODE_HALO2_INTERNALS), 128, True)
    cell0 = 8 * int(fs.digest_cells) + 1 + 46            # 8 digests, the Context's zero cell, the prologue's 46 cells
    return cell0 + 33, cell0


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
def test_ties_of_an_8_leaf_tree_across_a_column_break(int_engines, kernel_choice, hsw, mont):  # noqa: F811
    eng = int_engines(kernel_choice)
    leaves, msgs, want_nodes = tree(2000)
    rows, cell0 = break_inside_parent8(hsw)
    cfg = hsw.Sha256DynamicConfig(eng, [128] * 15, True, whole_digest=True)
    if mont:
        cfg.set_repr(hsw._native.HSW_REPR_MONTGOMERY)
    assert cfg.set_columns(rows) == 2
    _t, slices = device_messages(leaves)
    nodes = filled(32 * 15)
    cfg.merkle_tree_device(slices, nodes)
    assert host(nodes) == want_nodes
    # the first parent's 64 input-byte cells span the column break
    rc8 = result_cells(hsw, cfg, 8)
    assert int(rc8.input_bytes_cell0) == cell0
    assert cfg.cell_position(cell0 + 31) == (0, rows - 2) and cfg.cell_position(cell0 + 32) == (1, 0)
    ties, prefix = cfg.ties()
    assert len(ties) == 448 and prefix == 0
    assert as_tuples(ties) == tree_ties()
    outs = {h: result_cells(hsw, cfg, h) for h in range(15)}
    for t in ties:
        s, d, j, k = (int(t[f]) for f in ("src_hash", "dst_hash", "src_byte", "dst_byte"))
        assert int(t["src_cell"]) == int(outs[s].output_byte_cells[j]) and int(t["dst_cell"]) == int(outs[d].input_bytes_cell0) + k
        a, b = peek(cfg, t["src_cell"]), peek(cfg, t["dst_cell"])
        assert a == b == cell_words(want_nodes[32 * s + j], mont), (s, d, j, k)
    rep = cfg.verify_ties()
    print("verify_ties: %d checks, %.4f ms" % (rep["checks"], rep["kernel_ms"]))
    assert rep["violations"] == 0 and rep["checks"] == 448 and rep["kernel_ms"] > 0
    assert cfg.verify()["violations"] == 0
    cfg.close()


class Columns:
    """The caller's advice columns for K proofs in ONE int64 tensor of 32-byte cells: K x cols image columns of PITCH
    cells -- `reverse`: in descending address order, each an allocation of its own as far as the library knows --
    then the lookup and chip areas at pitches of their own."""

    def __init__(self, K, cols, Lp, chip_rows, reverse):
        import torch
        self.K, self.cols = K, cols
        step = STEP
        order = range(K * cols - 1, -1, -1) if reverse else range(K * cols)
        self.col_cell = {i: 4 + slot * step for slot, i in enumerate(order)}
        at = 4 + K * cols * step
        self.lk_pitch = (Lp + 7) & ~3
        self.chip_stride = (chip_rows + 7) & ~3
        self.chip_ctx = 2 * self.chip_stride + 8
        self.lk0, at = at, at + K * self.lk_pitch
        self.cd0, at = at, at + K * self.chip_ctx
        self.cs0, at = at, at + K * self.chip_ctx
        self.t = torch.zeros((at + 4, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self.base = self.t.data_ptr()
        assert self.base % 128 == 0
        self.cells = at + 4
        self.areas = dict(lookup=self.addr(self.lk0), lookup_capacity=Lp, lookup_pitch=self.lk_pitch, chip_dense=self.addr(self.cd0),
                          chip_spread=self.addr(self.cs0), chip_col_stride=self.chip_stride, chip_rows_capacity=chip_rows,
                          chip_context_pitch=self.chip_ctx)

    def addr(self, cell):
        return self.base + 32 * cell

    def words(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("binding", ["pitch", "pointer-tables-reversed"])
def test_ties_of_two_proofs_in_a_context_group_bound_to_caller_columns(int_engines, hsw, binding):  # noqa: F811
    eng = int_engines("default")
    K = 2
    trees = [tree(2000), tree(3000)]
    probe = hsw.Sha256DynamicConfig(eng, [128] * 15, True, n_contexts=K)
    cols = probe.set_columns(MAX_ROWS)
    b = probe.region_binding()
    Lp, chip_rows = int(b.lookup_capacity), int(b.chip_rows_capacity)
    probe.close()
    cfg = hsw.Sha256DynamicConfig(eng, [128] * 15, True, n_contexts=K)
    assert cfg.set_columns(MAX_ROWS) == cols
    cv = Columns(K, cols, Lp, chip_rows, reverse=binding != "pitch")
    if binding == "pitch":
        assert all(cv.col_cell[i] == 4 + i * STEP for i in range(K * cols))
        cfg.bind_region(cv.addr(cv.col_cell[0]), column_pitch=STEP, columns_capacity=cols, context_pitch=cols * STEP,
                        **cv.areas)
    else:
        ptrs = [cv.addr(cv.col_cell[i]) for i in range(K * cols)]
        assert all(ptrs[i + 1] < ptrs[i] for i in range(K * cols - 1))
        cfg.bind_columns(ptrs, PITCH, cols, **cv.areas)
    inputs, levels, outputs, keep = [], [], [], []
    nodes = filled(32 * 15 * K)
    for c in range(K):
        t, slices = device_messages(trees[c][0])
        keep.append(t)
        i, lv, o = tree_call(nodes.data_ptr() + 480 * c, slices)
        inputs, levels, outputs = inputs + i, levels + lv, outputs + o
    cfg.digest_levels_device(inputs, levels, outputs)
    assert host(nodes) == trees[0][2] + trees[1][2]
    ties, prefix = cfg.ties()
    assert prefix == 0 and as_tuples(ties) == tree_ties(0) + tree_ties(15)          # no tie crosses proofs
    stream = int(cfg.context_region(0).stream_cells)
    words = cv.words()
    for t in ties[::7]:
        for side, byte in (("src_cell", int(t["src_byte"])), ("dst_cell", int(t["src_byte"]))):
            cell = int(t[side])
            c, (col, row) = cell // stream, cfg.cell_position(cell)
            assert c == int(t["dst_hash"]) // 15 and row < MAX_ROWS
            at = cv.col_cell[c * cols + col] + row                      # the caller's own column, its own row
            assert cfg.cell_address(cell) == cv.addr(at)
            assert 0 <= at < cv.cells
            want = trees[c][2][32 * (int(t["src_hash"]) % 15) + byte]
            assert [int(x) for x in words[at]] == cell_words(want, False)
    rep = cfg.verify_ties()
    assert rep["violations"] == 0 and rep["checks"] == 896 and rep["kernel_ms"] > 0
    assert cfg.verify()["violations"] == 0
    cfg.close()


def test_a_parent_that_hashed_other_bytes_passes_verify_and_fails_verify_ties(int_engines, kernel_choice, hsw):  # noqa: F811
    import torch
    eng = int_engines(kernel_choice)
    a, b = rand(4000, 10), rand(4001, 119)
    cfg = hsw.Sha256DynamicConfig(eng, [128] * 3, True, whole_digest=True)
    cfg.set_columns(MAX_ROWS)
    _t, slices = device_messages([a, b])
    nodes = filled(128)
    base = nodes.data_ptr()
    # call 1 hashes two leaves into nodes; the test overwrites the second digest in ITS tensor; call 2 hashes the parent
    cfg.digest_levels_device(slices, None, [base, base + 32])
    assert host(nodes)[:64] == sha(a) + sha(b)
    junk = bytes(x ^ 0xFF for x in sha(b))                             # every byte differs from the digest's
    nodes[32:64] = torch.from_numpy(np.frombuffer(junk, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    rd = cfg.digest_batch_device([(base, 64)])
    assert rd[0].output_bytes == sha(sha(a) + junk)
    ties, _ = cfg.ties()
    assert as_tuples(ties) == [(k // 32, 2, k % 32, k) for k in range(64)]
    assert cfg.verify()["violations"] == 0                             # every digest is consistent with its own inputs
    rep = cfg.verify_ties()
    assert rep["violations"] == 32 and rep["checks"] == 64 and rep["first"] == 32      # tie (parent, byte 32)
    # a parent aimed at a slot nobody writes: no tie where a tree has 64
    cfg.reset()
    assert len(cfg.ties()[0]) == 0
    cfg.digest_levels_device(slices + [(base + 64, 64)], [0, 0, 1], [base, base + 32, None])
    ties, prefix = cfg.ties()
    assert len(ties) == 0 and prefix == 0
    rep = cfg.verify_ties()
    assert rep["checks"] == 0 and rep["violations"] == 0
    cfg.close()


def test_verify_equal_finds_the_one_pair_that_differs(int_engines, kernel_choice, hsw):  # noqa: F811
    eng = int_engines(kernel_choice)
    a, b = rand(5000, 56), rand(5001, 64)
    cfg = hsw.Sha256DynamicConfig(eng, [128] * 3, True, whole_digest=True)
    cfg.set_columns(MAX_ROWS)
    _t, slices = device_messages([a, b])
    nodes = filled(96)
    base = nodes.data_ptr()
    cfg.digest_levels_device(slices + [(base, 64)], [0, 0, 1], [base, base + 32, base + 64])
    ties, _ = cfg.ties()
    assert len(ties) == 64
    leaf0 = result_cells(hsw, cfg, 0)
    j = next(k for k in range(1, 32) if sha(a)[k] != sha(a)[0])        # two bytes of leaf 0's digest that differ
    x, y = int(leaf0.output_byte_cells[0]), int(leaf0.output_byte_cells[j])
    assert peek(cfg, x) == cell_words(sha(a)[0], False) != cell_words(sha(a)[j], False) == peek(cfg, y)
    # 70 pairs: the recorded ties, five cells against themselves, and -- at index 66 -- the pair that differs
    ca = [int(t["src_cell"]) for t in ties] + [x, y, x, y, 0, int(cfg.view().gate_cells) - 1]
    cb = [int(t["dst_cell"]) for t in ties] + [x, y, y, y, 0, int(cfg.view().gate_cells) - 1]
    assert len(ca) == 70 and (ca[66], cb[66]) == (x, y)
    rep = cfg.verify_equal(ca, cb)
    assert rep["violations"] == 1 and rep["first"] == 66 and rep["checks"] == 70 and rep["kernel_ms"] > 0
    cb[66] = x
    rep = cfg.verify_equal(ca, cb)
    assert rep["violations"] == 0 and rep["checks"] == 70
    assert cfg.verify_equal([], [])["checks"] == 0
    with pytest.raises(hsw.HswError) as ei:
        cfg.verify_equal([x, int(cfg.view().gate_cells)], [x, x])      # a cell past the last assigned one
    assert ei.value.status == hsw._native.HSW_ERR_INVALID_ARG
    cfg.close()
