"""hsw_gadget_digest_levels_device / Sha256DynamicConfig.digest_levels_device / merkle_tree_device: messages that read
other messages' digests in device memory -- one hsw_ingest_kernel launch per dependency level, the digest written by
the wave that computed it, the expansion once over the whole batch, no host read in between.

The yardstick is exact equality: every digest, in the results AND where the kernel wrote it, against hashlib.sha256;
streams, images, lookup columns, chip rows and input_bytes against a twin gadget on the same engine that is host-fed
the messages computed with hashlib.  Destinations sit in tensors pre-filled with 0xEE at every byte alignment, one of
them ending with its tensor: a store outside a destination's 32 bytes changes a filler byte, a sibling digest or
memory past the allocation."""
import hashlib

import numpy as np
import pytest

from tests.test_gpu_device_inputs import (device_messages, int_engines, rand, same_results,  # noqa: F401 (fixture)
                                          same_streams)
from tests.test_gpu_origin import MAX_ROWS

pytestmark = pytest.mark.gpu
FILL = 0xEE


def sha(m):
    return hashlib.sha256(m).digest()


def filled(n):
    import torch
    t = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy().tobytes()


def launches(eng):
    """Expansion launches of the engine so far (hsw_last_launch refuses while there has been none)."""
    import ctypes as C
    from importlib import import_module
    N = import_module("halo2-dynamic-sha256_amd")._native
    li = N.LaunchInfo()
    return int(li.seq) if eng.lib.hsw_last_launch(eng.h, C.byref(li)) == N.HSW_OK else 0


def merkle(leaves):
    """The hashlib tree in merkle_tree_device's order: (messages, nodes bytes)."""
    msgs, level = list(leaves), [sha(m) for m in leaves]
    nodes = b"".join(level)
    while len(level) > 1:
        inner = [level[2 * j] + level[2 * j + 1] for j in range(len(level) // 2)]
        msgs += inner
        level = [sha(m) for m in inner]
        nodes += b"".join(level)
    return msgs, nodes


def test_one_level_is_the_device_fed_call_and_stores_stay_inside_their_32_bytes(engine_factory, kernel_choice, hsw):
    eng = engine_factory(8, 2)
    lens = (0, 1, 55, 56, 63, 64, 119)
    msgs = [rand(900 + n, n) for n in lens]
    maxes = [128] * 7
    dev = hsw.Sha256DynamicConfig(eng, maxes, is_input_range_check=False)
    twin = hsw.Sha256DynamicConfig(eng, maxes, is_input_range_check=False)
    _t, slices = device_messages(msgs)
    offs = (0, 1, 3, 13, 17, 31)
    at = [64 * k + o for k, o in enumerate(offs)]                    # one window per 64 bytes, each misaligned differently
    out = filled(at[-1] + 32)                                         # the last destination ends with the tensor
    assert out.data_ptr() % 16 == 0
    windows = [out[a:a + 32] for a in at]
    outputs = windows[:3] + [None] + windows[3:]                      # message 3 has no destination
    rd = dev.digest_levels_device(slices, None, outputs)
    rt = twin.digest_batch_device(slices)
    same_results(rd, rt, msgs)
    same_streams(dev, twin)
    want = bytearray([FILL] * out.numel())
    for m, o in zip(msgs, outputs):
        if o is not None:
            a = o.data_ptr() - out.data_ptr()
            want[a:a + 32] = sha(m)
    assert host(out) == bytes(want)                                   # every window the digest, every other byte untouched
    assert dev.verify()["violations"] == 0
    dev.close()
    twin.close()


def test_merkle_tree_of_8_leaves_on_a_whole_digest_image(int_engines, kernel_choice, hsw):  # noqa: F811
    eng = int_engines(kernel_choice)
    leaves = [rand(1000 + n, n) for n in (0, 1, 55, 56, 63, 64, 100, 119)]
    msgs, want_nodes = merkle(leaves)
    assert len(msgs) == 15 and len(want_nodes) == 32 * 15
    gadgets = []
    for _ in range(2):
        cfg = hsw.Sha256DynamicConfig(eng, [128] * 15, True, whole_digest=True)
        cfg.set_columns(MAX_ROWS)
        gadgets.append(cfg)
    dev, twin = gadgets
    _t, slices = device_messages(leaves)
    nodes = filled(32 * 15)
    s0 = launches(eng)
    rd = dev.merkle_tree_device(slices, nodes)
    s1 = launches(eng)
    rt = twin.digest_batch(msgs)
    s2 = launches(eng)
    assert host(nodes) == want_nodes and rd[-1].output_bytes == want_nodes[-32:]
    same_results(rd, rt, msgs)
    st = same_streams(dev, twin)
    assert st["gate"].shape[1:] == (MAX_ROWS, 4) and st["gate"].any()
    rep = dev.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0
    assert (s1 - s0) % (1 << 32) == (s2 - s1) % (1 << 32) >= 1       # the tree's expansion launches are one batch's
    with pytest.raises(ValueError):
        dev.merkle_tree_device(slices[:3], nodes)
    dev.close()
    twin.close()


def test_interleaved_levels_in_a_context_group(int_engines, kernel_choice, hsw):  # noqa: F811
    eng = int_engines(kernel_choice)
    k = 2
    leaves = [rand(1100, 10), rand(1101, 119), rand(1102, 64), rand(1103, 0)]
    msgs, roots = [], []
    for c in range(k):
        a, b = leaves[2 * c], leaves[2 * c + 1]
        msgs += [a, b, sha(a) + sha(b)]
        roots.append(sha(sha(a) + sha(b)))
    gadgets = []
    for _ in range(2):
        cfg = hsw.Sha256DynamicConfig(eng, [128] * 3, True, n_contexts=k)
        cfg.set_columns(MAX_ROWS)
        gadgets.append(cfg)
    dev, twin = gadgets
    _t, sl = device_messages(leaves)
    nodes = filled(96 * k)
    base = nodes.data_ptr()
    inputs, outputs = [], []
    for c in range(k):
        inputs += [sl[2 * c], sl[2 * c + 1], (base + 96 * c, 64)]
        outputs += [nodes[96 * c:96 * c + 32], base + 96 * c + 32, nodes[96 * c + 64:96 * c + 96]]
    rd = dev.digest_levels_device(inputs, [0, 0, 1, 0, 0, 1], outputs)
    rt = twin.digest_batch(msgs)
    same_results(rd, rt, msgs)
    got = host(nodes)
    assert [got[96 * c + 64:96 * c + 96] for c in range(k)] == roots == [rd[2].output_bytes, rd[5].output_bytes]
    st = same_streams(dev, twin)
    assert st["gate"].shape[0] == k
    for c in range(k):
        a, b = dev.context_region(c), twin.context_region(c)
        assert int(a.assigned) == 1
        for f, _ in a._fields_:
            if not f.startswith("d_"):
                assert getattr(a, f) == getattr(b, f), f
        assert st["gate"][c].any()
    rep = dev.verify()
    assert rep["violations"] == 0 and rep["checks"] > 0
    dev.close()
    twin.close()


def test_hash_chain_read_in_place_at_odd_offsets(engine_factory, kernel_choice, hsw):
    eng = engine_factory(8, 2)
    x = rand(1200, 37)
    msgs = [x]
    for _ in range(3):
        msgs.append(sha(msgs[-1]))
    dev = hsw.Sha256DynamicConfig(eng, [64] * 4, is_input_range_check=False)
    twin = hsw.Sha256DynamicConfig(eng, [64] * 4, is_input_range_check=False)
    _t, sl = device_messages([x])
    at = (1, 35, 71, 109)                                             # odd offsets; 1 and 35 leave two bytes between siblings
    buf = filled(at[-1] + 32)
    base = buf.data_ptr()
    inputs = [sl[0]] + [(base + a, 32) for a in at[:3]]
    rd = dev.digest_levels_device(inputs, [0, 1, 2, 3], [base + a for a in at])
    rt = twin.digest_batch(msgs)
    same_results(rd, rt, msgs)
    same_streams(dev, twin)
    want = bytearray([FILL] * buf.numel())
    for a, m in zip(at, msgs):
        want[a:a + 32] = sha(m)
    assert host(buf) == bytes(want)
    dev.close()
    twin.close()


def test_prefix_rounds_produce_digests_that_a_later_level_reads(engine_factory, kernel_choice, hsw):
    """A 100-byte message with a 128-byte prefix (target_round == 0: its digest is the state after a prefix round)
    and a 200-byte message with a 64-byte prefix feed a level-1 message, the 64 bytes of their digests."""
    eng = engine_factory(8, 2)
    a, b = rand(1300, 100), rand(1301, 200)
    msgs = [a, b, sha(a) + sha(b)]
    maxes, pres = [64, 192, 128], [128, 64, None]
    dev = hsw.Sha256DynamicConfig(eng, maxes, is_input_range_check=False)
    twin = hsw.Sha256DynamicConfig(eng, maxes, is_input_range_check=False)
    _t, sl = device_messages([a, b])
    buf = filled(3 + 96)
    base = buf.data_ptr() + 3
    rd = dev.digest_levels_device(sl + [(base, 64)], [0, 0, 1], [base, base + 32, base + 64], pres)
    rt = twin.digest_batch(msgs, pres)
    assert [(r.num_round, r.target_round) for r in rd] == [(2, 0), (4, 3), (2, 2)]
    same_results(rd, rt, msgs)
    same_streams(dev, twin)
    assert host(buf) == bytes([FILL] * 3) + sha(a) + sha(b) + sha(msgs[2])
    dev.close()
    twin.close()


def test_digest_is_written_at_num_round_not_at_the_end_of_the_loop(engine_factory, kernel_choice, hsw):
    """40 staged rounds per message, beyond one 32-round chunk: num_round 32 (the last round of chunk 0), 33 (the
    first of chunk 1), 1, and 33 of the 56 rounds a message with a 16-round prefix runs."""
    eng = engine_factory(8, 2)
    lens, pres = (2039, 2040, 10, 2100), [None, None, None, 1024]
    msgs = [rand(1400 + n, n) for n in lens]
    maxes = [2560] * 4
    dev = hsw.Sha256DynamicConfig(eng, maxes, is_input_range_check=False)
    twin = hsw.Sha256DynamicConfig(eng, maxes, is_input_range_check=False)
    _t, sl = device_messages(msgs)
    buf = filled(5 + 4 * 32)
    outs = [buf[5 + 32 * i:5 + 32 * i + 32] for i in range(4)]
    rd = dev.digest_levels_device(sl, None, outs, pres)
    assert [r.num_round for r in rd] == [(n + 9 + 63) // 64 for n in lens] == [32, 33, 1, 33]
    assert [r.n_blocks for r in rd] == [40] * 4
    assert host(buf) == bytes([FILL] * 5) + b"".join(sha(m) for m in msgs)
    rt = twin.digest_batch(msgs, pres)
    same_results(rd, rt, msgs)
    same_streams(dev, twin)
    dev.close()
    twin.close()


def test_refusals_leave_gadget_and_destinations_alone(engine_factory, kernel_choice, hsw):
    eng = engine_factory(8, 2)
    msgs = [rand(1500, 40), rand(1501, 64)]
    dev = hsw.Sha256DynamicConfig(eng, [64, 128, 128], is_input_range_check=False)
    twin = hsw.Sha256DynamicConfig(eng, [64, 128, 128], is_input_range_check=False)
    _t, sl = device_messages(msgs)
    buf = filled(160)
    base = buf.data_ptr()
    before = dev.view()
    for inputs, levels, outputs in (
            (sl, [0, 0], [base, base + 31]),                          # two outputs sharing one byte
            ([sl[0], (base + 31, 64)], [0, 0], [base, None]),         # an input over a same-level output
            ([(base + 95, 40), sl[1]], [0, 1], [None, base + 64])):   # an input over a higher-level output
        with pytest.raises(hsw.HswError) as ei:
            dev.digest_levels_device(inputs, levels, outputs)
        assert ei.value.status == hsw._native.HSW_ERR_INVALID_ARG and "message" in str(ei.value)
        after = dev.view()
        assert (after.cur_hash_idx, after.blocks_done, after.num_limb_sum) == (before.cur_hash_idx, before.blocks_done, before.num_limb_sum) == (0, 0, 0)
        assert host(buf) == bytes([FILL] * 160)
    third = sha(msgs[0]) + sha(msgs[1])
    rd = dev.digest_levels_device(sl + [(base, 64)], [0, 0, 1], [base, base + 32, base + 64])
    rt = twin.digest_batch(msgs + [third])
    same_results(rd, rt, msgs + [third])
    same_streams(dev, twin)
    assert host(buf) == sha(msgs[0]) + sha(msgs[1]) + sha(third) + bytes([FILL] * 64)
    dev.close()
    twin.close()
