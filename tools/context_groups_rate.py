#!/usr/bin/env python3
"""K proofs of a circuit that makes TWO 1024-byte digests per proof, Montgomery cells, k = 17 columns, three ways in
the SAME process with their timed calls alternated:

  (a) groups   one Context group (hsw_gadget_create_contexts): K = 128 Contexts of two digests, 4,096 blocks, two
               expansion launches + one frame launch per batch
  (b) images   K = 256 one-digest context images (HSW_GADGET_CONTEXT_IMAGES): the same 4,096 blocks, one expansion
               launch + one frame launch -- the yardstick
  (c) singles  the 128 proofs as 128 separate HSW_GADGET_SHARED_CONTEXT gadgets, a batch of two each: what a caller
               had to do before there were groups; recorded for the ratio only

Message, warm-up and timing loop as in tools/context_images_rate.py.  Kernel times are hsw_last_kernel_ms: the LAST
expansion launch of the call (for (a): digest index 1 of all Contexts, half the blocks).  Writes
profiles/context_groups_rate.json and prints it.  usage: context_groups_rate.py [--only=groups|images|singles] [K]
(K = proofs of (a); --only runs one way, for a profiler run that must not mix them)"""
import ctypes as C
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hsw = importlib.import_module("halo2-dynamic-sha256_amd")
N = hsw._native

HBM_PEAK = 8e12                  # bytes/s, MI355X HBM3E spec (as bench.py)
ALGO_BYTES_PER_BLOCK = 2385664
MAX_ROWS = (1 << 17) - 9
TARGET = 1.10                    # (a) within 10 % of (b): the run-to-run placement swing of such batches


def _args(n):
    m56 = bytes([1] * 56)
    bufs = [(C.c_uint8 * 56).from_buffer_copy(m56) for _ in range(n)]
    return (bufs, (C.c_void_p * n)(*[C.addressof(b) for b in bufs]), (C.c_size_t * n)(*([56] * n)),
            (C.c_size_t * n)(*([0] * n)), (N.HashResult * n)())


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    ways = tuple(only) if only else ("groups", "images", "singles")
    assert all(w in ("groups", "images", "singles") for w in ways), ways
    ks = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    K = ks[0] if ks else 128
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    eng.set_timing(True)
    L = eng.lib
    run = {}
    if "groups" in ways:
        g = hsw.Sha256DynamicConfig(eng, [1024, 1024], True, n_contexts=K)
        g.set_repr(N.HSW_REPR_MONTGOMERY)
        run["groups"] = dict(gadgets=[g], n=2 * K, columns=g.set_columns(MAX_ROWS), args=_args(2 * K))
    if "images" in ways:
        g = hsw.Sha256DynamicConfig(eng, [1024] * (2 * K), True, whole_digest=True, independent=True, context_images=True)
        g.set_repr(N.HSW_REPR_MONTGOMERY)
        run["images"] = dict(gadgets=[g], n=2 * K, columns=g.set_columns(MAX_ROWS), args=_args(2 * K))
    if "singles" in ways:
        gs = []
        for _ in range(K):
            g = hsw.Sha256DynamicConfig(eng, [1024, 1024], True, whole_digest=True, shared_context=True)
            g.set_repr(N.HSW_REPR_MONTGOMERY)
            cols = g.set_columns(MAX_ROWS)
            gs.append(g)
        run["singles"] = dict(gadgets=gs, n=2, columns=cols, args=_args(2))
    for d in run.values():
        d["t"], d["kernel_ms"], d["launches"] = [], [], None
    order = [w for w in ways]
    for i in range(3 + 9):       # 3 warm-up rounds, then the median of 9; alternated, so every way sees the same device state
        for name in order if i % 2 == 0 else order[::-1]:
            d = run[name]
            _, ptrs, lens, pres, res = d["args"]
            for g in d["gadgets"]:
                assert L.hsw_gadget_reset(g.h) == 0
            seq0 = eng.last_launch()["seq"] if i else 0
            t1 = time.perf_counter()
            for g in d["gadgets"]:                      # (c): 128 calls, each synchronous, as a caller would issue them
                rc = L.hsw_gadget_digest_batch(g.h, d["n"], ptrs, lens, pres, res)
                assert rc == 0
            d["t"].append(time.perf_counter() - t1)
            try:
                d["kernel_ms"].append(eng.last_kernel_ms())
            except hsw.HswError:                        # (the small-batch launches of (c) carry no event pair)
                d["kernel_ms"].append(float("nan"))
            d["launch"] = eng.last_launch()
            d["launches"] = d["launch"]["seq"] - seq0 if i else None
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    blocks = 32 * K
    out = {"tool": "context_groups_rate", "commit": commit or None, "proofs": K, "blocks": blocks, "message_bytes": 56,
           "max_rows": MAX_ROWS, "repr": "montgomery", "target_groups_over_images": TARGET, "ways": {}}
    want = hashlib.sha256(bytes([1] * 56)).digest()
    for name, d in run.items():
        assert bytes(d["args"][4][d["n"] - 1].output_bytes) == want
        t = float(np.median(d["t"][3:]))
        vk = d["gadgets"][-1].verify()
        out["ways"][name] = {"ms": t * 1e3, "ms_all": [x * 1e3 for x in d["t"][3:]],
                             "last_expansion_kernel_ms": float(np.median(d["kernel_ms"][3:])),
                             "last_expansion_blocks": d["launch"]["n_blocks"], "expansion_launches_per_round": d["launches"],
                             "frac_algorithmic": blocks * ALGO_BYTES_PER_BLOCK / t / HBM_PEAK, "kernel": d["launch"]["kernel"],
                             "columns_per_proof": d["columns"],
                             "verify_last_gadget": {"violations": vk["violations"], "checks": vk["checks"]}}
        assert vk["violations"] == 0
    w = out["ways"]
    if "groups" in w and "images" in w:
        out["groups_over_images"] = w["groups"]["ms"] / w["images"]["ms"]
        out["target_met"] = out["groups_over_images"] <= TARGET
    if "groups" in w and "singles" in w:
        out["singles_over_groups"] = w["singles"]["ms"] / w["groups"]["ms"]
    for d in run.values():
        for g in d["gadgets"]:
            g.close()
    eng.close()
    text = json.dumps(out)
    if not only and K == 128:
        with open(os.path.join(ROOT, "profiles", "context_groups_rate.json"), "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
