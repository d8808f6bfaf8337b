#!/usr/bin/env python3
"""hsw_gadget_lookup_multiplicities against a plain read of the same bytes and against hsw_gadget_verify: K = 256 proofs of
the bench circuit (one 1,024-byte digest each: 53,059 range entries + 2 x 65,920 chip cells per proof, 32 bytes a cell,
about 1.5 GB for K = 256) as context images bound (hsw_gadget_bind_region) to ONE torch tensor, so that the yardstick can
read exactly the runs' bytes without any code under test:
  (a) counts        hsw_gadget_lookup_multiplicities, both tables, into the caller's tensors;
  (b) plain_read    torch .sum() over views of the bound tensor that cover exactly the listed runs;
  (c) verify        hsw_gadget_verify of the same region.
One process, the three timed calls alternated in rotating order, 3 warm-ups, the median of 9.  Reported per cell form and
per privatisation variant (engine option "lookup_lds"): lds = the spread table in an LDS histogram per workgroup, the
range entries by one global atomic each (the default); global_atomics = the spread rows by global atomics too.
counts_over_plain_read = (a)/(b), counts_over_verify = (a)/(c); target_met: (a)/(b) <= 2 for Montgomery cells with the
default variant.  Writes one JSON document (default profiles/lookup_counts_rate.json) and prints it.
usage: lookup_counts_rate.py [--out=PATH] [K]"""
import ctypes as C
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

PITCH = 1 << 17
MAX_ROWS = PITCH - 9
COLS = 9
RANGE_PER_PROOF, CHIP_PER_PROOF = 3 + 2 * 1024 + 16 * 3184 + 64, 16 * 4120
MARGIN = 2.0
VARIANTS = (("lds", 1), ("global_atomics", 0))


def case(eng, K, form, variants):
    import torch
    L = eng.lib
    g = hsw.Sha256DynamicConfig(eng, [1024] * K, True, whole_digest=True, independent=True, context_images=True)
    if form == "montgomery":
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    assert g.set_columns(MAX_ROWS) == COLS
    # one slab per proof: [9 image columns | lookup | 2 dense | 2 spread] polynomials of 2^17 cells
    slab, o_lk, o_cd, o_cs = (COLS + 5) * PITCH, COLS * PITCH, (COLS + 1) * PITCH, (COLS + 3) * PITCH
    T = torch.zeros((K, slab, 4), dtype=torch.int64, device="cuda")
    p = T.data_ptr()
    g.bind_region(columns=p, column_pitch=PITCH, columns_capacity=COLS, context_pitch=slab, lookup=p + 32 * o_lk,
                  lookup_capacity=PITCH, lookup_pitch=slab, chip_dense=p + 32 * o_cd, chip_spread=p + 32 * o_cs,
                  chip_col_stride=PITCH, chip_rows_capacity=PITCH, chip_context_pitch=slab)
    m56 = bytes([1] * 56)
    g.digest_batch([m56] * K)
    runs = g.lookup_runs()
    assert len(runs) == 3 * K
    # (b): views of T over exactly the runs -- the same (first, n) in every proof, checked against the list
    views = []
    for r in runs[:3]:
        o = o_lk if r["table"] == 0 else o_cd + r["column"] * PITCH
        same = [x for x in runs if (x["table"], x["column"]) == (r["table"], r["column"])]
        assert all((x["first"], x["n"], x["d_cells"]) == (r["first"], r["n"], p + 32 * (x["context"] * slab + o + r["first"])) for x in same)
        views.append(T[:, o + r["first"]: o + r["first"] + r["n"]])
        if r["table"] == 1:
            assert all(x["d_spread"] == x["d_cells"] + 32 * 2 * PITCH for x in same)
            views.append(T[:, o + 2 * PITCH + r["first"]: o + 2 * PITCH + r["first"] + r["n"]])
    read_bytes = sum(v.numel() * 8 for v in views)
    assert read_bytes == K * (RANGE_PER_PROOF + 2 * CHIP_PER_PROOF) * 32
    rt = torch.zeros((K, 65536), dtype=torch.int32, device="cuda")
    st = torch.zeros((K, 256), dtype=torch.int32, device="cuda")
    args = N.LookupCounts(rt.data_ptr(), st.data_ptr(), 0, 0, 0, 0)
    rep, vrep = N.LookupReport(), N.VerifyReport()
    torch.cuda.synchronize()

    def counts():
        t1 = time.perf_counter()
        rc = L.hsw_gadget_lookup_multiplicities(g.h, C.byref(args), C.byref(rep))
        dt = time.perf_counter() - t1
        assert rc == 0 and rep.not_in_table == 0
        return dt, float(rep.kernel_ms)

    def plain_read():
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        acc = [v.sum() for v in views]
        torch.cuda.synchronize()
        return time.perf_counter() - t1, acc

    def verify():
        t1 = time.perf_counter()
        rc = L.hsw_gadget_verify(g.h, C.byref(vrep))
        dt = time.perf_counter() - t1
        assert rc == 0 and vrep.violations == 0
        return dt

    out = {"read_bytes": read_bytes, "variants": {}}
    for variant, lds in variants:
        eng.set_option("lookup_lds", lds)
        t = {"counts": [], "kernel": [], "plain_read": [], "verify": []}
        order = ["counts", "plain_read", "verify"]
        for i in range(3 + 9):
            for name in order[i % 3:] + order[: i % 3]:
                if name == "counts":
                    dt, k = counts()
                    t["counts"].append(dt)
                    t["kernel"].append(k)
                elif name == "plain_read":
                    t["plain_read"].append(plain_read()[0])
                else:
                    t["verify"].append(verify())
        assert rep.range_entries == K * RANGE_PER_PROOF and rep.spread_entries == K * CHIP_PER_PROOF
        assert int(rt.sum().item()) == K * RANGE_PER_PROOF and int(st.sum().item()) == K * CHIP_PER_PROOF
        med = {k: float(np.median(v[3:])) * (1.0 if k == "kernel" else 1e3) for k, v in t.items()}
        out["variants"][variant] = {
            "counts_ms": med["counts"], "counts_kernel_ms": med["kernel"], "plain_read_ms": med["plain_read"], "verify_ms": med["verify"],
            "counts_over_plain_read": med["counts"] / med["plain_read"], "counts_over_verify": med["counts"] / med["verify"],
            "counts_read_TBps": read_bytes / med["counts"] / 1e9, "plain_read_TBps": read_bytes / med["plain_read"] / 1e9}
    eng.set_option("lookup_lds", 1)
    g.close()
    del T
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "lookup_counts_rate.json")
    ks = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [256]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "lookup_counts_rate", "commit": commit or None, "margin": MARGIN, "cases": {}}
    for K in ks:
        for form in ("montgomery", "canonical"):
            res["cases"]["%d_%s" % (K, form)] = case(eng, K, form, VARIANTS)
    eng.close()
    first = res["cases"]["%d_montgomery" % ks[0]]["variants"]["lds"]
    res["counts_over_plain_read"] = first["counts_over_plain_read"]
    res["counts_over_verify"] = first["counts_over_verify"]
    res["target_met"] = bool(first["counts_over_plain_read"] <= MARGIN)
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
