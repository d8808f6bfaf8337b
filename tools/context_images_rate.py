#!/usr/bin/env python3
"""K proofs of the bench circuit in one launch: linear region streams (HSW_GADGET_INDEPENDENT) against one column
image per proof (HSW_GADGET_CONTEXT_IMAGES, origin (0, 0), 9 x 131,063 rows each), both gadgets in the SAME process,
their timed calls alternated.  Message, warm-up and timing loop as in bench.py's "batched" section.  Prints one JSON
line.  usage: context_images_rate.py [--only=linear|images] [K[,form] ...]   (default: 8 64 256 512 Montgomery,
256 canonical; --only runs one layout, for a profiler run that must not mix the two)"""
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
ALGO_BYTES_PER_BLOCK = 2385664   # 16 blocks per proof
MAX_ROWS = (1 << 17) - 9


def case(eng, K, form, layouts=("linear", "images")):
    m56 = bytes([1] * 56)
    bufs = [(C.c_uint8 * 56).from_buffer_copy(m56) for _ in range(K)]
    ptrs = (C.c_void_p * K)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * K)(*([56] * K))
    pres = (C.c_size_t * K)(*([0] * K))
    L = eng.lib
    gadgets = {}
    for name in layouts:
        images = name == "images"
        g = hsw.Sha256DynamicConfig(eng, [1024] * K, True, whole_digest=True, independent=True, context_images=images)
        if form == "montgomery":
            g.set_repr(N.HSW_REPR_MONTGOMERY)
        cols = g.set_columns(MAX_ROWS) if images else None
        placed = g.place(3)[0] if K >= 64 else None
        gadgets[name] = dict(g=g, cols=cols, placed=placed, t=[], res=(N.HashResult * K)())
    for i in range(3 + 9):    # 3 warm-up calls, then the median of 9; alternated, so both layouts see the same device state
        for name in layouts if i % 2 == 0 else layouts[::-1]:
            d = gadgets[name]
            assert L.hsw_gadget_reset(d["g"].h) == 0
            t1 = time.perf_counter()
            rc = L.hsw_gadget_digest_batch(d["g"].h, K, ptrs, lens, pres, d["res"])
            d["t"].append(time.perf_counter() - t1)
            assert rc == 0
            d["launch"] = eng.last_launch()
    out = {}
    for name, d in gadgets.items():
        g = d["g"]
        assert bytes(d["res"][K - 1].output_bytes) == hashlib.sha256(m56).digest()
        v = g.view()
        region_bytes = (int(v.gate_cells) + int(v.lookup_cells) + 2 * int(v.num_limb_sum)) * 32      # as bench.py counts a region
        t = float(np.median(d["t"][3:]))
        vk = g.verify()
        out[name] = {"ms": t * 1e3, "frac_algorithmic": 16 * K * ALGO_BYTES_PER_BLOCK / t / HBM_PEAK,
                     "frac_region": region_bytes / t / HBM_PEAK, "region_bytes": region_bytes,
                     "kernel": d["launch"]["kernel"],
                     "verify": {"violations": vk["violations"], "checks": vk["checks"]},
                     "placement_candidates_batch_ms": d["placed"]}
        if d["cols"]:
            out[name]["columns_per_proof"] = d["cols"]
        g.close()
    if len(layouts) == 2:
        out["images_over_linear"] = out["images"]["ms"] / out["linear"]["ms"]
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    layouts = tuple(only) if only else ("linear", "images")
    assert all(x in ("linear", "images") for x in layouts), layouts
    specs = [a for a in sys.argv[1:] if not a.startswith("--")] or ["8", "64", "256", "512", "256,canonical"]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "context_images_rate", "commit": commit or None, "message_bytes": 56, "max_rows": MAX_ROWS, "cases": {}}
    for spec in specs:
        k, form = (spec.split(",") + ["montgomery"])[:2]
        key = k if form == "montgomery" else "%s_%s" % (k, form)
        try:
            res["cases"][key] = case(eng, int(k), form, layouts)
        except Exception as ex:          # one case failing (memory) does not hide the others
            res["cases"][key] = {"error": repr(ex)}
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
