#!/usr/bin/env python3
"""K proofs of the bench circuit written where a prover that keeps its witness in HBM wants them: one slab of 14
polynomials of 2^17 cells per proof ([9 FlexGate | 1 lookup | 2 dense | 2 spread]).  Four ways, all gadgets in the
SAME process, their timed calls alternated, 3 warm-ups and the median of 9, Montgomery cells:
  owned        the library-owned context images (HSW_GADGET_CONTEXT_IMAGES as it was): the yardstick
  copy         owned + the strided device-to-device copy of every proof into its slab: what a prover had to do
  bound        hsw_gadget_bind_region to one plain slab per proof (all slabs one allocation)
  bound_range  bound, the FlexGate columns in an hsw_device_alloc range (allocated once, never freed during the run),
               lookup and chip columns in a separate plain allocation
Writes profiles/bound_region_rate.json and prints the same JSON line.
usage: bound_region_rate.py [--only=owned|copy|bound|bound_range] [K]   (default K = 256)"""
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

MAX_ROWS, N17, POLYS, COLS = (1 << 17) - 9, 1 << 17, 14, 9
D2D = 3                          # hipMemcpyDeviceToDevice


def main():
    assert torch.cuda.is_available(), "no HIP device"
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    names = ("owned", "copy", "bound", "bound_range")
    layouts = tuple(only) if only else names
    assert all(x in names for x in layouts), layouts
    ks = [a for a in sys.argv[1:] if not a.startswith("--")]
    K = int(ks[0]) if ks else 256
    hip = C.CDLL("libamdhip64.so")           # the runtime torch has loaded
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
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

    G = {}
    keep = []
    for name in layouts:
        g = gadget()
        d = dict(g=g, t=[], res=(N.HashResult * K)())
        if name in ("copy", "bound"):
            t = torch.zeros((K * slab, 4), dtype=torch.int64, device="cuda")
            keep.append(t)
            d["slab"] = t.data_ptr()
        if name == "bound":
            p = d["slab"]
            g.bind_region(p, N17, COLS, p + 32 * 9 * N17, N17, p + 32 * 10 * N17, p + 32 * 12 * N17, N17, N17,
                          context_pitch=slab, lookup_pitch=slab, chip_context_pitch=slab)
        if name == "bound_range":
            rng = C.c_void_p()
            assert L.hsw_device_alloc(0, K * COLS * N17 * 32, 0, C.byref(rng)) == 0
            d["range"] = rng
            rest = torch.zeros((K * 5 * N17, 4), dtype=torch.int64, device="cuda")
            keep.append(rest)
            q = rest.data_ptr()
            g.bind_region(rng.value, N17, COLS, q, N17, q + 32 * N17, q + 32 * 3 * N17, N17, N17,
                          context_pitch=COLS * N17, lookup_pitch=5 * N17, chip_context_pitch=5 * N17)
        G[name] = d
    torch.cuda.synchronize()

    def copy_out(d):
        """every proof of the owned gadget into its slab: 9 columns, the lookup column, 2 + 2 chip columns"""
        g = d["g"]
        b = g.region_binding()
        rows = int(b.chip_rows_capacity)
        for c in range(K):
            dst = d["slab"] + 32 * c * slab
            hip.hipMemcpy2DAsync(dst, 32 * N17, int(b.d_columns) + 32 * c * int(b.context_pitch), 32 * MAX_ROWS, 32 * MAX_ROWS, COLS, D2D, None)
            hip.hipMemcpyAsync(dst + 32 * 9 * N17, int(b.d_lookup) + 32 * c * int(b.lookup_pitch), 32 * int(b.lookup_capacity), D2D, None)
            for k in range(2):
                off = 32 * (k * int(b.chip_col_stride) + c * rows)
                hip.hipMemcpyAsync(dst + 32 * (10 + k) * N17, int(b.d_chip_dense) + off, 32 * rows, D2D, None)
                hip.hipMemcpyAsync(dst + 32 * (12 + k) * N17, int(b.d_chip_spread) + off, 32 * rows, D2D, None)
        torch.cuda.synchronize()

    for i in range(3 + 9):
        for name in layouts if i % 2 == 0 else layouts[::-1]:
            d = G[name]
            assert L.hsw_gadget_reset(d["g"].h) == 0
            t1 = time.perf_counter()
            rc = L.hsw_gadget_digest_batch(d["g"].h, K, ptrs, lens, pres, d["res"])
            if name == "copy":
                copy_out(d)
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
    res = {"tool": "bound_region_rate", "commit": commit or None, "K": K, "form": "montgomery", "message_bytes": 56,
           "slab_cells": slab, "copy_bytes_per_batch": None, "layouts": out}
    if "owned" in out:
        over = {n: out[n]["ms"] / out["owned"]["ms"] for n in ("bound", "bound_range") if n in out}
        res["bound_over_owned"] = over
        if over:
            res["target_met"] = bool(min(over.values()) <= 1.10)      # within the 10 % run-to-run placement swing
    if "copy" in out and "bound" in out:
        res["copy_path_over_bound"] = out["copy"]["ms"] / out["bound"]["ms"]
    eng.close()
    line = json.dumps(res)
    if not only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "bound_region_rate.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
