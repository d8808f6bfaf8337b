#!/usr/bin/env python3
"""hsw_gadget_permutation_product at one prover-sized shape, next to its neighbour: K = 1 proof, m = 17 columns in
chunks of L = 4 (S = 5 Z columns), usable_rows = 2^20 - 6.  The columns are synthetic -- random encodings below p for
the values and the sigmas, so the proof comes out OPEN and is written all the same: the kernels take no data-dependent
path short of a refusal -- and the comparison is hsw_gadget_lookup_product with one range argument over columns of the
same height, equally synthetic, in the same process.
Per cell form, alternated, 2 warm-ups and the median of 7:
  the call            kernel_ms and its three stages (tiles_ms, scan_ms, write_ms), and ns per (row, column);
  the lookup product  kernel_ms and its stages for ONE argument of usable_rows rows, and ns per row.
Nothing is promised: no threshold.  Writes one JSON document (default profiles/permutation_product_rate.json) and
prints it.
usage: permutation_product_rate.py [--out=PATH] [m [L [usable_rows]]]"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hsw = importlib.import_module("halo2-dynamic-sha256_amd")
N = hsw._native


def cells(shape):
    """random encodings below p: every 64-bit limb below 2^60"""
    import torch
    return torch.randint(0, 1 << 60, shape + (4,), dtype=torch.int64, device="cuda").view(torch.uint64)


def case(eng, form, m, L, u):
    import torch
    torch.manual_seed(1)
    g = hsw.Sha256DynamicConfig(eng, [64], True, whole_digest=True, independent=True, context_images=True)
    if form == "montgomery":
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    g.set_columns((1 << 17) - 9)
    S = (m + L - 1) // L
    cols, sig = cells((1, m, u)), cells((m, u))
    z = torch.zeros((1, S, u + 1, 4), dtype=torch.uint64, device="cuda")
    lk = [cells((1, u)) for _ in range(3)]
    lz = torch.zeros((1, u + 1, 4), dtype=torch.uint64, device="cuda")
    ch = np.array([[3, 5, 7, 11]], dtype=np.uint64)                         # any element below p, as stored
    t = {k: [] for k in ("kernel", "tiles", "scan", "write", "lookup_kernel", "lookup_tiles", "lookup_scan", "lookup_write")}
    for i in range(2 + 7):
        for what in (("call", "lookup") if i % 2 == 0 else ("lookup", "call")):
            if what == "call":
                _, status, rep = g.permutation_product(u, L, ch, ch + 1, ch + 2, ch + 3, cols, sig, out=z)
                assert not (status[0] & 6) and rep["written"] == S * (u + 1), (status, rep)
                for k in ("kernel", "tiles", "scan", "write"):
                    t[k].append(rep[k + "_ms"])
            else:
                _, status, rep = g.lookup_product(N.HSW_LOOKUP_RANGE, u, ch, ch + 1, lk[0], lk[1], lk[2], out=lz)
                assert not (status[0] & 6) and rep["written"] == u + 1, (status, rep)
                for k in ("kernel", "tiles", "scan", "write"):
                    t["lookup_" + k].append(rep[k + "_ms"])
    g.close()
    med = {k + "_ms": float(np.median(v[2:])) for k, v in t.items()}
    med.update({"kernel_ms_min": float(min(t["kernel"][2:])), "kernel_ms_max": float(max(t["kernel"][2:])),
                "ns_per_row_and_column": med["kernel_ms"] * 1e6 / (u * m), "lookup_ns_per_row": med["lookup_kernel_ms"] * 1e6 / u,
                "bytes_read_per_stage": 2 * 32 * m * u, "bytes_written": 32 * S * (u + 1)})
    med["row_and_column_over_lookup_row"] = med["ns_per_row_and_column"] / med["lookup_ns_per_row"]
    return med


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "permutation_product_rate.json")
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    m, L, u = (nums + [17, 4, (1 << 20) - 6][len(nums):])[:3]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "permutation_product_rate", "commit": commit or None, "proofs": 1, "columns": m, "chunk_columns": L, "usable_rows": u,
           "runs": "2 warm-ups, median of 7, alternated with the lookup product", "cases": {}}
    for form in ("montgomery", "canonical"):
        res["cases"][form] = case(eng, form, m, L, u)
    eng.close()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
