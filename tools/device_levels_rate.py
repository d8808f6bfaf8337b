#!/usr/bin/env python3
"""A Merkle tree whose every node is hashed in circuit: 256 leaves of 64 bytes, 511 digests of
max_variable_byte_size 128 (1,022 blocks) on a whole-digest gadget, Montgomery cells.  Two ways, both gadgets in ONE
process, their timed calls alternated, 3 warm-ups and the median of 9:
  levels     (a) one Sha256DynamicConfig.merkle_tree_device call (hsw_gadget_digest_levels_device): nine ingest
                 launches back to back, one expansion over all 511 digests, no host read of a digest
  per_level  (b) what a caller had to do before: nine digest_batch calls, one per level, each building its messages
                 on the host from the previous call's output_bytes
with the expansion launches of each (hsw_last_launch.seq differences).  No threshold.  Prints one JSON line and writes
it to profiles/device_levels_rate.json.
usage: device_levels_rate.py [--only=levels|per_level]   (one way alone, for a profiler run that must not mix them)"""
import ctypes as C
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hsw = importlib.import_module("halo2-dynamic-sha256_amd")
N = hsw._native
LEAVES, LEAF_BYTES = 256, 64


def main():
    assert torch.cuda.is_available(), "no HIP device"
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    names = ("levels", "per_level")
    ways = tuple(only) if only else names
    assert all(x in names for x in ways), ways
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    n_digests = 2 * LEAVES - 1
    gadgets = {}
    for w in ways:
        g = hsw.Sha256DynamicConfig(eng, [128] * n_digests, True, whole_digest=True)
        g.set_repr(N.HSW_REPR_MONTGOMERY)
        gadgets[w] = g
    rng = np.random.default_rng(11)
    host = rng.integers(0, 256, LEAVES * LEAF_BYTES, dtype=np.uint8)
    leaves = [host[i * LEAF_BYTES:(i + 1) * LEAF_BYTES].tobytes() for i in range(LEAVES)]
    dev = torch.from_numpy(host).cuda()
    tensors = [dev[i * LEAF_BYTES:(i + 1) * LEAF_BYTES] for i in range(LEAVES)]
    nodes = torch.zeros(32 * n_digests, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    level = [hashlib.sha256(m).digest() for m in leaves]
    while len(level) > 1:
        level = [hashlib.sha256(level[2 * j] + level[2 * j + 1]).digest() for j in range(len(level) // 2)]
    root = level[0]

    def seq():                      # expansion launches so far (hsw_last_launch refuses while there has been none)
        li = N.LaunchInfo()
        return int(li.seq) if eng.lib.hsw_last_launch(eng.h, C.byref(li)) == N.HSW_OK else 0

    t = {w: [] for w in ways}
    launches, calls = {}, {}
    for i in range(3 + 9):
        for w in ways if i % 2 == 0 else ways[::-1]:
            g = gadgets[w]
            g.reset()
            s0, t0 = seq(), time.perf_counter()
            if w == "levels":
                res = g.merkle_tree_device(tensors, nodes)
                calls[w] = 1
            else:
                msgs, calls[w] = leaves, 0
                while True:
                    res = g.digest_batch(msgs)
                    calls[w] += 1
                    if len(res) == 1:
                        break
                    msgs = [res[2 * j].output_bytes + res[2 * j + 1].output_bytes for j in range(len(res) // 2)]
            t[w].append(time.perf_counter() - t0)
            launches[w] = (seq() - s0) % (1 << 32)
            assert res[-1].output_bytes == root
    if "levels" in ways:
        assert nodes[-32:].cpu().numpy().tobytes() == root
    out = {}
    for w in ways:
        g = gadgets[w]
        vk = g.verify()
        out[w] = {"ms": float(np.median(t[w][3:])) * 1e3, "all_ms": [x * 1e3 for x in t[w][3:]], "calls": calls[w],
                  "expansion_launches": launches[w], "blocks": int(g.view().blocks_done),
                  "verify": {"violations": vk["violations"], "checks": vk["checks"]}}
        g.close()
    if len(ways) == 2:
        out["levels_over_per_level"] = out["levels"]["ms"] / out["per_level"]["ms"]
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    line = json.dumps({"tool": "device_levels_rate", "commit": commit or None, "leaves": LEAVES, "leaf_bytes": LEAF_BYTES,
                       "digests": n_digests, "max_variable_byte_size": 128, "form": "montgomery", **out})
    eng.close()
    if not only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "device_levels_rate.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
