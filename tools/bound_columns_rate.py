#!/usr/bin/env python3
"""K proofs of the bench circuit written into a prover that keeps ONE allocation per advice column per proof
(hsw_gadget_bind_columns), next to the pitch binding and the library-owned images.  The protocol of
tools/bound_region_rate.py: all gadgets in the SAME process, their timed calls alternated, 3 warm-ups and the median of
9, Montgomery cells, K = 256 bench circuits of 9 columns:
  owned     (a) the library-owned context images: the yardstick
  bound     (b) hsw_gadget_bind_region to one plain slab per proof (pitches)
  carved    (c) K x 9 columns by pointer table, carved from one plain allocation in shuffled order (fixed seed)
  separate  (d) the same columns as K x 9 separate allocations, wherever the allocator puts them
  tables    (e) every advice column a separate allocation: the K x 9 image columns AND, by pointer table too
                (hsw_gadget_bind_column_tables), the K lookup columns and the K x 2 x 2 chip columns
Lookup and chip columns keep the pitch model in (b)-(d) (5 polynomials per proof in one allocation).
Writes profiles/bound_columns_rate.json -- (c)/(a), (d)/(a), (c)/(b), (e)/(a) -- and prints the same JSON line.
usage: bound_columns_rate.py [--only=owned|bound|carved|separate|tables] [K]   (default K = 256)"""
import ctypes as C
import hashlib
import importlib
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hsw = importlib.import_module("halo2-dynamic-sha256_amd")
N = hsw._native

MAX_ROWS, N17, POLYS, COLS = (1 << 17) - 9, 1 << 17, 14, 9


def main():
    assert torch.cuda.is_available(), "no HIP device"
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    names = ("owned", "bound", "carved", "separate", "tables")
    layouts = tuple(only) if only else names
    assert all(x in names for x in layouts), layouts
    ks = [a for a in sys.argv[1:] if not a.startswith("--")]
    K = int(ks[0]) if ks else 256
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    L = eng.lib
    m56 = bytes([1] * 56)
    bufs = [(C.c_uint8 * 56).from_buffer_copy(m56) for _ in range(K)]
    ptrs = (C.c_void_p * K)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * K)(*([56] * K))
    pres = (C.c_size_t * K)(*([0] * K))
    slab = POLYS * N17

    def gadget():
        g = hsw.Sha256DynamicConfig(eng, [1024] * K, True, whole_digest=True, independent=True, context_images=True)
        g.set_repr(N.HSW_REPR_MONTGOMERY)
        assert g.set_columns(MAX_ROWS) == COLS
        return g

    def rest_areas():
        rest = torch.zeros((K * 5 * N17, 4), dtype=torch.int64, device="cuda")
        q = rest.data_ptr()
        return rest, dict(lookup=q, lookup_capacity=N17, chip_dense=q + 32 * N17, chip_spread=q + 32 * 3 * N17, chip_col_stride=N17,
                          chip_rows_capacity=N17, lookup_pitch=5 * N17, chip_context_pitch=5 * N17)

    G, keep = {}, []
    for name in layouts:
        g = gadget()
        d = dict(g=g, t=[], res=(N.HashResult * K)())
        if name == "bound":
            t = torch.zeros((K * slab, 4), dtype=torch.int64, device="cuda")
            keep.append(t)
            p = t.data_ptr()
            g.bind_region(p, N17, COLS, p + 32 * 9 * N17, N17, p + 32 * 10 * N17, p + 32 * 12 * N17, N17, N17,
                          context_pitch=slab, lookup_pitch=slab, chip_context_pitch=slab)
        if name == "carved":
            t = torch.zeros((K * COLS * N17, 4), dtype=torch.int64, device="cuda")
            slots = list(range(K * COLS))
            random.Random(20240229).shuffle(slots)
            rest, kw = rest_areas()
            keep += [t, rest]
            g.bind_columns([t.data_ptr() + 32 * N17 * s for s in slots], N17, COLS, **kw)
        if name == "separate":
            cols = [torch.zeros((N17, 4), dtype=torch.int64, device="cuda") for _ in range(K * COLS)]
            rest, kw = rest_areas()
            keep += [cols, rest]
            g.bind_columns(cols, N17, COLS, **kw)
        if name == "tables":
            def polys(n):
                return [torch.zeros((N17, 4), dtype=torch.int64, device="cuda") for _ in range(n)]
            cols, lks, cds, css = polys(K * COLS), polys(K), polys(K * 2), polys(K * 2)
            keep += [cols, lks, cds, css]
            g.bind_columns(cols, N17, COLS, lookup_capacity=N17, chip_rows_capacity=N17, lookup_ptrs=lks, chip_dense_ptrs=cds,
                           chip_spread_ptrs=css)
        G[name] = d
    torch.cuda.synchronize()

    for i in range(3 + 9):
        for name in layouts if i % 2 == 0 else layouts[::-1]:
            d = G[name]
            assert L.hsw_gadget_reset(d["g"].h) == 0
            t1 = time.perf_counter()
            rc = L.hsw_gadget_digest_batch(d["g"].h, K, ptrs, lens, pres, d["res"])
            d["t"].append(time.perf_counter() - t1)
            assert rc == 0
            d["launch"] = eng.last_launch()
    out = {}
    for name, d in G.items():
        assert bytes(d["res"][K - 1].output_bytes) == hashlib.sha256(m56).digest()
        vk = d["g"].verify()
        out[name] = {"ms": float(np.median(d["t"][3:])) * 1e3, "all_ms": [x * 1e3 for x in d["t"][3:]], "kernel": d["launch"]["kernel"],
                     "verify": {"violations": vk["violations"], "checks": vk["checks"]}}
        d["g"].close()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "bound_columns_rate", "commit": commit or None, "K": K, "form": "montgomery", "message_bytes": 56, "layouts": out}

    def ratio(a, b):
        return out[a]["ms"] / out[b]["ms"] if a in out and b in out else None
    res["carved_over_owned"], res["separate_over_owned"], res["carved_over_bound"] = ratio("carved", "owned"), ratio("separate", "owned"), ratio("carved", "bound")
    res["tables_over_owned"] = ratio("tables", "owned")
    got = [x for x in (res["carved_over_owned"], res["separate_over_owned"], res["tables_over_owned"]) if x is not None]
    if len(got) == 3:
        res["target_met"] = bool(max(got) <= 1.10)            # within the 10 % run-to-run placement swing
    eng.close()
    line = json.dumps(res)
    if not only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "bound_columns_rate.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
