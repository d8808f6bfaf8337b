#!/usr/bin/env python3
"""hsw_gadget_lookup_product against its memory floor and its neighbour: K = 256 proofs of the bench circuit (one
1,024-byte digest each) as context images, usable_rows = 2^17 - 9, all three lookup arguments per proof -- the range
argument (K arguments) and the spread arguments (2 K arguments).  The unpermuted inputs are the pass's own cells
(hsw_gadget_lookup_runs), A' / S' come from hsw_gadget_lookup_permuted in counted mode, Z is usable_rows + 1 cells per
argument.
Per cell form and per table, in one process, alternated, 2 warm-ups and the median of 7:
  the call               kernel_ms and its three stages (tiles_ms, scan_ms, write_ms);
  a plain device copy    that reads and writes as many bytes as the call moves (inputs, A' and S' are read by two stages,
                         Z is written once): the memory floor;
  the permuted step      hsw_gadget_lookup_permuted's kernel_ms on the same columns: what a caller already pays.
Every argument must close (open_arguments == 0, refused_arguments == 0).  Nothing is promised: no threshold.
Writes one JSON document (default profiles/lookup_product_rate.json) and prints it.
usage: lookup_product_rate.py [--out=PATH] [K]"""
import ctypes as C
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

PITCH = 1 << 17
USABLE = PITCH - 9
P_INT = 0x30644e72e131a029b85045b68181585d2833e84879b97091_43e1f593f0000001
R_INT = (1 << 256) % P_INT


def challenges(rng, K, mont):
    vals = [int.from_bytes(rng.bytes(40), "little") % P_INT for _ in range(K)]
    return np.array([[((v * R_INT % P_INT if mont else v) >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in vals], dtype=np.uint64)


def case(eng, K, form):
    import torch
    L = eng.lib
    mont = form == "montgomery"
    g = hsw.Sha256DynamicConfig(eng, [1024] * K, True, whole_digest=True, independent=True, context_images=True)
    if mont:
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    g.set_columns(USABLE)
    g.digest_batch([bytes([1] * 56)] * K)
    runs = g.lookup_runs()
    rng = np.random.default_rng(1)
    thetas, betas, gammas = (challenges(rng, K, mont) for _ in range(3))
    out = {}
    for name, table, n_args in (("range", N.HSW_LOOKUP_RANGE, K), ("spread", N.HSW_LOOKUP_SPREAD, 2 * K)):
        spread = table == N.HSW_LOOKUP_SPREAD
        mine = [r for r in runs if r["table"] == table]
        assert len(mine) == n_args, (len(mine), n_args)                      # one run per argument for this circuit
        pair = torch.empty((2 * n_args, USABLE, 4), dtype=torch.int64, device="cuda")
        z = torch.empty((n_args, USABLE + 1, 4), dtype=torch.int64, device="cuda")
        ptr = [pair.data_ptr() + a * USABLE * 32 for a in range(2 * n_args)]
        arr = lambda v: (C.c_void_p * n_args)(*v)                             # noqa: E731
        pargs = N.LookupPermuted(table, 0, USABLE, n_args, arr(ptr[:n_args]), arr(ptr[n_args:]), thetas.ctypes.data if spread else None, None, 0)
        status = np.zeros(n_args, dtype=np.uint32)
        args = N.LookupProduct(table, 0, USABLE, n_args, arr([r["d_cells"] for r in mine]), arr([r["d_spread"] for r in mine]) if spread else None,
                               (C.c_uint64 * n_args)(*[r["n"] for r in mine]), arr(ptr[:n_args]), arr(ptr[n_args:]),
                               arr([z.data_ptr() + a * (USABLE + 1) * 32 for a in range(n_args)]), thetas.ctypes.data if spread else None,
                               betas.ctypes.data, gammas.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_uint32)))
        read = 32 * (sum(r["n"] for r in mine) * (2 if spread else 1) + 2 * USABLE * n_args)
        moved = 2 * read + 32 * (USABLE + 1) * n_args
        src = torch.empty(moved // 2 // 8, dtype=torch.int64, device="cuda")
        dst = torch.empty_like(src)
        prep, rep = N.PermutedReport(), N.ProductReport()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = {"kernel": [], "tiles": [], "scan": [], "write": [], "copy": [], "permuted": []}
        for i in range(2 + 7):
            rc = L.hsw_gadget_lookup_permuted(g.h, C.byref(pargs), C.byref(prep))
            assert rc == 0 and prep.written == 2 * USABLE * n_args, (rc, prep.written)
            t["permuted"].append(prep.kernel_ms)
            for what in (("call", "copy") if i % 2 == 0 else ("copy", "call")):
                if what == "copy":
                    ev0.record()
                    dst.copy_(src)
                    ev1.record()
                    torch.cuda.synchronize()
                    t["copy"].append(ev0.elapsed_time(ev1))
                else:
                    rc = L.hsw_gadget_lookup_product(g.h, C.byref(args), C.byref(rep))
                    assert rc == 0 and rep.open_arguments == 0 and rep.refused_arguments == 0 and rep.written == (USABLE + 1) * n_args, (rc, rep.written)
                    t["kernel"].append(rep.kernel_ms); t["tiles"].append(rep.tiles_ms); t["scan"].append(rep.scan_ms); t["write"].append(rep.write_ms)
        assert not status.any()
        med = {k: float(np.median(v[2:])) for k, v in t.items()}
        out[name] = {"arguments": n_args, "tile_rows": int(rep.tile_rows), "bytes_moved": moved, "kernel_ms": med["kernel"], "tiles_ms": med["tiles"],
                     "scan_ms": med["scan"], "write_ms": med["write"], "copy_ms": med["copy"], "permuted_kernel_ms": med["permuted"],
                     "kernel_over_copy": med["kernel"] / med["copy"], "kernel_over_permuted": med["kernel"] / med["permuted"],
                     "rows_per_us": USABLE * n_args / med["kernel"] / 1e3}
        del pair, z, src, dst
    g.close()
    tot = {k: out["range"][k] + out["spread"][k] for k in ("bytes_moved", "kernel_ms", "tiles_ms", "scan_ms", "write_ms", "copy_ms", "permuted_kernel_ms")}
    tot["kernel_over_copy"] = tot["kernel_ms"] / tot["copy_ms"]
    tot["kernel_over_permuted"] = tot["kernel_ms"] / tot["permuted_kernel_ms"]
    out["all_arguments"] = tot
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "lookup_product_rate.json")
    ks = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [256]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "lookup_product_rate", "commit": commit or None, "usable_rows": USABLE, "cases": {}}
    for K in ks:
        for form in ("montgomery", "canonical"):
            res["cases"]["%d_%s" % (K, form)] = case(eng, K, form)
    eng.close()
    first = res["cases"]["%d_montgomery" % ks[0]]["all_arguments"]
    res["kernel_over_copy"] = first["kernel_over_copy"]
    res["kernel_over_permuted"] = first["kernel_over_permuted"]
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
