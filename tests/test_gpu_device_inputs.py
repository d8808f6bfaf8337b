"""hsw_gadget_digest_batch_device / Sha256DynamicConfig.digest_batch_device: messages that already live in device
memory, padded, prefix-hashed, staged and chained by ONE hsw_ingest_kernel launch.

The yardstick is exact equality: every digest against hashlib.sha256; streams, images, lookup columns, chip rows
and input_bytes against a second gadget on the same engine fed the same messages from host memory (and case 1
against the oracle as well).  The messages are slices of one uint8 device tensor at byte offsets 1, 2, 3, 5, 7, ...
so that every source is misaligned differently, and one message ends exactly at the tensor's last byte: a kernel
that reads a 16-byte granule past a message's end reads past the allocation there."""
import hashlib

import numpy as np
import pytest

from tests.test_gpu_origin import MAX_ROWS

pytestmark = pytest.mark.gpu
OFFSETS = (1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31)


@pytest.fixture(scope="module")
def int_engines(hsw):
    """Internals-mode engines by kernel choice (whole-digest gadgets need one)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    engines = {}

    def get(choice):
        if choice not in engines:
            e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
            e.set_option("split", -1 if choice == "default" else 0)
            engines[choice] = e
        return engines[choice]

    yield get
    for e in engines.values():
        e.close()


def device_messages(msgs):
    """One uint8 device tensor holding every message at its own misalignment, the last one ending with the tensor;
    returns (tensor, slices).  A zero-length message is the pair (0, 0): a NULL pointer."""
    import torch
    at, pos = [], 0
    for i, m in enumerate(msgs):
        off = OFFSETS[i % len(OFFSETS)]
        pos = (pos + 15) // 16 * 16 + off            # every start at byte `off` of a 16-byte granule
        at.append(pos)
        pos += len(m)
    host = np.full(pos, 0xEE, dtype=np.uint8)        # filler bytes no message contains by construction of the checks
    for a, m in zip(at, msgs):
        host[a:a + len(m)] = np.frombuffer(m, dtype=np.uint8)
    t = torch.from_numpy(host).cuda()
    assert t.numel() == at[-1] + len(msgs[-1])       # the last message ends exactly at the tensor's last byte
    torch.cuda.synchronize()
    return t, [t[a:a + len(m)] if len(m) else (0, 0) for a, m in zip(at, msgs)]


def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def same_results(dev, host, msgs):
    for m, x, y in zip(msgs, dev, host):
        assert x.output_bytes == y.output_bytes == hashlib.sha256(m).digest()
        assert x.input_bytes == y.input_bytes and len(x.input_bytes) == 64 * x.n_blocks
        for k in ("input_len", "first_block", "n_blocks", "spread_cursor0", "num_round", "target_round", "prologue_cell",
                  "block_cell", "epilogue_cell", "end_cell", "prologue_lookup", "block_lookup", "epilogue_lookup"):
            assert getattr(x, k) == getattr(y, k), k


def same_streams(a, b):
    sa, sb = a.streams(), b.streams()
    assert sa.keys() == sb.keys() and sa["rows"] == sb["rows"]
    for k in sa:
        if k != "rows":
            assert np.array_equal(sa[k], sb[k]), k
    va, vb = a.view(), b.view()
    for k in ("blocks_done", "num_limb_sum", "cur_hash_idx", "gate_cells", "lookup_cells", "columns"):
        assert getattr(va, k) == getattr(vb, k), k
    return sa


def both(hsw, eng, maxes, msgs, pres=None, **kw):
    """The same pass on two gadgets of one engine: device-fed and host-fed."""
    dev = hsw.Sha256DynamicConfig(eng, maxes, **kw)
    host = hsw.Sha256DynamicConfig(eng, maxes, **kw)
    t, slices = device_messages(msgs)
    rd = dev.digest_batch_device(slices, pres)
    rh = host.digest_batch(msgs, pres)
    same_results(rd, rh, msgs)
    return dev, host, rd, t


def test_plain_gadget_ragged_sizes_null_pointer_and_oracle(engine_factory, kernel_choice, hsw, oracle):
    eng = engine_factory(8, 2)
    maxes = [64, 256, 128, 192]
    msgs = [rand(100 + i, n) for i, n in enumerate((10, 200, 0, 100))]
    dev, host, rd, _ = both(hsw, eng, maxes, msgs, is_input_range_check=False)
    st = same_streams(dev, host)
    o = oracle.Oracle(8, 2, check=True)
    ref = [o.digest(m, mx, 0, want_streams=True) for m, mx in zip(msgs, maxes)]
    assert np.array_equal(st["gate"], np.concatenate([r["gate"] for r in ref]))
    assert np.array_equal(st["dense"], np.concatenate([r["dense"] for r in ref], axis=1))
    assert np.array_equal(st["spread"], np.concatenate([r["spread"] for r in ref], axis=1))
    assert [r.input_bytes for r in rd] == [r["blocks"].tobytes() for r in ref]
    assert dev.verify()["violations"] == 0
    dev.close()
    host.close()


def test_padding_edges_in_one_batch_then_too_large(engine_factory, kernel_choice, hsw):
    eng = engine_factory(8, 2)
    lens = (0, 1, 55, 56, 63, 64, 119)
    msgs = [rand(200 + n, n) for n in lens]
    dev, host, rd, _ = both(hsw, eng, [128] * (len(lens) + 1), msgs, is_input_range_check=False)
    assert [r.num_round for r in rd] == [1, 1, 1, 2, 2, 2, 2]
    same_streams(dev, host)
    before = dev.view()
    _, big = device_messages([rand(9, 120)])
    with pytest.raises(hsw.HswError) as ei:
        dev.digest_batch_device(big)                                  # lib.rs:90
    assert ei.value.status == hsw._native.HSW_ERR_TOO_LARGE
    after = dev.view()
    assert (after.cur_hash_idx, after.blocks_done, after.num_limb_sum) == (before.cur_hash_idx, before.blocks_done, before.num_limb_sum) == (7, 14, 14 * 4120)
    m = rand(10, 77)                                                  # the gadget goes on where it was
    _, s = device_messages([m])
    assert dev.digest_batch_device(s)[0].output_bytes == host.digest(m).output_bytes == hashlib.sha256(m).digest()
    same_streams(dev, host)
    dev.close()
    host.close()


def test_precomputed_prefix(engine_factory, kernel_choice, hsw):
    """lib.rs:587-611: two random 192-byte messages, the first 128 bytes hashed outside the circuit."""
    eng = engine_factory(8, 2)
    msgs = [rand(300, 192), rand(301, 192)]
    dev, host, rd, _ = both(hsw, eng, [128, 128], msgs, [128, 128], is_input_range_check=True)
    assert [(r.num_round, r.target_round) for r in rd] == [(4, 2), (4, 2)]
    same_streams(dev, host)
    dev.close()
    host.close()


def test_prefix_that_swallows_the_padding(engine_factory, kernel_choice, hsw):
    """100 bytes with a 128-byte prefix: 0x80 and the bit length lie inside the prefix, target_round is 0 and the
    digest is the state after the prefix (d_init_states)."""
    eng = engine_factory(8, 2)
    msgs = [rand(400, 100)]
    dev, host, rd, _ = both(hsw, eng, [64], msgs, [128], is_input_range_check=False)
    assert (rd[0].num_round, rd[0].target_round) == (2, 0) and rd[0].input_bytes == bytes(64)
    same_streams(dev, host)
    dev.close()
    host.close()


@pytest.mark.parametrize("length,prefix,mx,rounds", [(2058, None, 2112, 33), (2100, 1984, 192, 33)])
def test_chunk_boundary_of_the_32_round_loop(engine_factory, kernel_choice, hsw, length, prefix, mx, rounds):
    """(a) 33 rounds with the padding in round 32, the second chunk's only round; (b) a 31-round prefix, so the
    variable part's rounds 31, 32, 33 straddle the chunk."""
    eng = engine_factory(8, 2)
    msgs = [rand(500 + length, length)]
    dev, host, rd, _ = both(hsw, eng, [mx], msgs, [prefix], is_input_range_check=False)
    assert rd[0].num_round == rounds and rd[0].target_round == rounds - (prefix or 0) // 64
    assert length // 64 == 32                                         # 0x80 and the bit length in round 32
    same_streams(dev, host)
    dev.close()
    host.close()


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
def test_bench_circuit_whole_digest_image(int_engines, kernel_choice, hsw, mont):
    """benches/digest.rs as one whole region with a column image: 16 blocks are a small-batch launch, which reads
    its inputs from the device staging here (the host-fed twin reads the pinned staging)."""
    eng = int_engines(kernel_choice)
    m = b"\x01" * 56
    gadgets = []
    for _ in range(2):
        cfg = hsw.Sha256DynamicConfig(eng, [1024], True, whole_digest=True)
        if mont:
            cfg.set_repr(hsw._native.HSW_REPR_MONTGOMERY)
        cfg.set_columns(MAX_ROWS)
        gadgets.append(cfg)
    dev, host = gadgets
    _, s = device_messages([m])
    rd, rh = dev.digest_batch_device(s), host.digest_batch([m])
    same_results(rd, rh, [m])
    assert rd[0].n_blocks == 16 and rd[0].target_round == 2
    st = same_streams(dev, host)
    assert st["gate"].shape[1:] == (MAX_ROWS, 4) and st["gate"].any()
    rep = dev.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0
    dev.close()
    host.close()


def test_context_group_table_path_and_frame_launch(int_engines, kernel_choice, hsw):
    eng = int_engines(kernel_choice)
    sizes, k = [128, 64], 2
    msgs = [rand(600, 119), rand(601, 30), rand(602, 64), rand(603, 0)]
    gadgets = []
    for _ in range(2):
        cfg = hsw.Sha256DynamicConfig(eng, sizes, True, n_contexts=k)
        cfg.set_columns(MAX_ROWS)
        gadgets.append(cfg)
    dev, host = gadgets
    _, s = device_messages(msgs)
    rd, rh = dev.digest_batch_device(s), host.digest_batch(msgs)
    same_results(rd, rh, msgs)
    st = same_streams(dev, host)
    assert st["gate"].shape[0] == k
    for c in range(k):
        a, b = dev.context_region(c), host.context_region(c)
        assert int(a.assigned) == 1
        for f, _ in a._fields_:
            if not f.startswith("d_"):
                assert getattr(a, f) == getattr(b, f), f
        assert int(a.d_image) - int(dev.view().d_gate) == int(b.d_image) - int(host.view().d_gate)
        assert st["gate"][c].any()
    rep = dev.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0
    dev.close()
    host.close()


def test_python_surface(engine_factory, kernel_choice, hsw):
    import torch
    eng = engine_factory(8, 2)
    msgs = [rand(700, 40), rand(701, 100)]
    t, slices = device_messages(msgs)
    a = hsw.Sha256DynamicConfig(eng, [64, 128], False)
    b = hsw.Sha256DynamicConfig(eng, [64, 128], False)
    ra = a.digest_batch_device(slices)
    rb = b.digest_batch_device([(x.data_ptr(), x.numel()) for x in slices])
    same_results(ra, rb, msgs)
    same_streams(a, b)
    c = hsw.Sha256DynamicConfig(eng, [64, 128], False)
    lib_calls = c.view().cur_hash_idx
    wide = torch.zeros(256, dtype=torch.uint8, device="cuda")
    for bad, exc in ((wide[::2], ValueError), (wide.view(torch.int32), TypeError), (wide.reshape(16, 16), TypeError),
                     (wide.cpu(), ValueError), ((0, 5), ValueError)):
        with pytest.raises(exc):
            c.digest_batch_device([slices[0], bad])
    assert c.view().cur_hash_idx == lib_calls == 0 and c.view().blocks_done == 0
    for g in (a, b, c):
        g.close()
