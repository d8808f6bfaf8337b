#!/usr/bin/env python3
"""The digest-to-digest copy constraints of a pass, checked on the device: kernel time of hsw_gadget_verify_ties
(hsw_verify_pairs_kernel, one lane per tie) next to hsw_gadget_verify's for the same region.  Two cases in ONE process:
  tree     an 8-leaf Merkle tree on a whole-digest image: 15 digests, 30 blocks, 448 ties
  trees    K = 256 such trees as a Context group: 3,840 digests, 7,680 blocks, 114,688 ties
3 warm-ups and the median of 9 for each call; the wall time of verify_ties (host address resolution, upload, launch,
read-back) is reported next to the kernel's.  No threshold.  Prints one JSON line and writes it to
profiles/ties_rate.json.
usage: ties_rate.py [--only=tree|trees]"""
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
MAX_ROWS = (1 << 17) - 9
LEAF_LENS = (0, 1, 55, 56, 63, 64, 100, 119)


def tree_call(base, leaves):
    inputs, levels, below, width, level = list(leaves), [0] * 8, 0, 8, 0
    while width > 1:
        level += 1
        inputs += [(base + 32 * (below + 2 * j), 64) for j in range(width // 2)]
        levels += [level] * (width // 2)
        below, width = below + width, width // 2
    return inputs, levels, [base + 32 * k for k in range(15)]


def main():
    assert torch.cuda.is_available(), "no HIP device"
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    cases = tuple(only) if only else ("tree", "trees")
    assert all(x in ("tree", "trees") for x in cases), cases
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    arena = torch.randint(0, 256, (1024,), dtype=torch.uint8, device="cuda")
    leaves = [(arena.data_ptr() + 120 * i + 2 * i + 1, n) for i, n in enumerate(LEAF_LENS)]
    torch.cuda.synchronize()
    out = {}
    for name in cases:
        K = 1 if name == "tree" else 256
        g = hsw.Sha256DynamicConfig(eng, [128] * 15, True, whole_digest=True) if K == 1 else \
            hsw.Sha256DynamicConfig(eng, [128] * 15, True, n_contexts=K)
        columns = g.set_columns(MAX_ROWS)
        nodes = torch.zeros(480 * K, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        inputs, levels, outputs = [], [], []
        for c in range(K):
            i, lv, o = tree_call(nodes.data_ptr() + 480 * c, leaves)
            inputs, levels, outputs = inputs + i, levels + lv, outputs + o
        g.digest_levels_device(inputs, levels, outputs)
        ties, untied = g.ties()
        assert len(ties) == 448 * K and untied == 0
        t = {"ties_kernel": [], "ties_wall": [], "verify_kernel": []}
        for _ in range(3 + 9):
            t0 = time.perf_counter()
            rep = g.verify_ties()
            t["ties_wall"].append((time.perf_counter() - t0) * 1e3)
            assert rep["violations"] == 0 and rep["checks"] == 448 * K
            t["ties_kernel"].append(rep["kernel_ms"])
            rep = g.verify()
            assert rep["violations"] == 0
            t["verify_kernel"].append(rep["kernel_ms"])
        med = {k: float(np.median(v[3:])) for k, v in t.items()}
        out[name] = {"proofs": K, "digests": 15 * K, "blocks": int(g.view().blocks_done), "columns_per_proof": columns, "ties": 448 * K,
                     "verify_ties_kernel_ms": med["ties_kernel"], "verify_ties_wall_ms": med["ties_wall"],
                     "verify_kernel_ms": med["verify_kernel"], "all_ms": {k: v[3:] for k, v in t.items()}}
        g.close()
        del nodes
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    line = json.dumps({"tool": "ties_rate", "commit": commit or None, "cases": out})
    eng.close()
    if not only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "ties_rate.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
