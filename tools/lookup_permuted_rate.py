#!/usr/bin/env python3
"""hsw_gadget_lookup_permuted against a plain fill of the same bytes: K = 256 proofs of the bench circuit (one 1,024-byte
digest each) as context images, usable_rows = 2^17 - 9, all three lookup arguments per proof -- the range argument
(K arguments, 2^16-row table) and the spread arguments (2 K arguments, 2^8-row table) -- an A' and an S' column of
usable_rows 32-byte cells each: 25 MB per proof, 6.4 GB for K = 256.
Per cell form and per table, in one process: the call (counted mode, the multiplicities into scratch) and
hsw_fill_calibrate over the very buffer the call writes, alternated, 2 warm-ups, the median of 7.  Reported: bytes
written, kernel_ms split into prepare_ms (count, index arrays, value tables) and write_ms (the stores), the fill's ms,
and the ratios write_over_fill and kernel_over_fill.  The plain fill is the yardstick; nothing is promised.
Writes one JSON document (default profiles/lookup_permuted_rate.json) and prints it.
usage: lookup_permuted_rate.py [--out=PATH] [K]"""
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
RANGE_PER_PROOF, CHIP_PER_PROOF = 3 + 2 * 1024 + 16 * 3184 + 64, 16 * 4120
P_INT = 0x30644e72e131a029b85045b68181585d2833e84879b97091_43e1f593f0000001


def case(eng, K, form):
    import torch
    L = eng.lib
    g = hsw.Sha256DynamicConfig(eng, [1024] * K, True, whole_digest=True, independent=True, context_images=True)
    if form == "montgomery":
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    g.set_columns(USABLE)
    g.digest_batch([bytes([1] * 56)] * K)
    rng = np.random.default_rng(1)
    thetas = np.array([[(v >> (64 * i)) & (2**64 - 1) for i in range(4)]
                       for v in (int.from_bytes(rng.bytes(40), "little") % P_INT for _ in range(K))], dtype=np.uint64)
    out = {}
    for name, table, n_args, entries in (("range", N.HSW_LOOKUP_RANGE, K, K * RANGE_PER_PROOF), ("spread", N.HSW_LOOKUP_SPREAD, 2 * K, K * CHIP_PER_PROOF)):
        buf = torch.empty((2 * n_args, USABLE, 4), dtype=torch.int64, device="cuda")
        ptr = [buf.data_ptr() + a * USABLE * 32 for a in range(2 * n_args)]
        args = N.LookupPermuted(table, 0, USABLE, n_args, (C.c_void_p * n_args)(*ptr[:n_args]), (C.c_void_p * n_args)(*ptr[n_args:]),
                                thetas.ctypes.data if table == N.HSW_LOOKUP_SPREAD else None, None, 0)
        rep = N.PermutedReport()
        torch.cuda.synchronize()
        t = {"kernel": [], "prepare": [], "write": [], "fill": []}
        for i in range(2 + 7):
            for what in (("call", "fill") if i % 2 == 0 else ("fill", "call")):
                if what == "fill":
                    t["fill"].append(eng.fill_calibrate(buf))
                else:
                    rc = L.hsw_gadget_lookup_permuted(g.h, C.byref(args), C.byref(rep))
                    assert rc == 0 and rep.not_in_table == 0 and rep.entries == entries and rep.written == 2 * USABLE * n_args, (rc, rep.written)
                    t["kernel"].append(rep.kernel_ms); t["prepare"].append(rep.prepare_ms); t["write"].append(rep.write_ms)
        # the pair of the first argument, on the host: the two constraints of a permuted pair
        a, s = buf[0].cpu().numpy(), buf[n_args].cpu().numpy()
        same = (a[1:] == a[:-1]).all(axis=1)
        assert (a[0] == s[0]).all() and (same | (a[1:] == s[1:]).all(axis=1)).all()
        med = {k: float(np.median(v[2:])) for k, v in t.items()}
        nbytes = buf.numel() * 8
        out[name] = {"arguments": n_args, "bytes_written": nbytes, "kernel_ms": med["kernel"], "prepare_ms": med["prepare"], "write_ms": med["write"],
                     "fill_ms": med["fill"], "write_over_fill": med["write"] / med["fill"], "kernel_over_fill": med["kernel"] / med["fill"],
                     "write_TBps": nbytes / med["write"] / 1e9, "fill_TBps": nbytes / med["fill"] / 1e9}
        del buf
    g.close()
    tot = {k: out["range"][k] + out["spread"][k] for k in ("bytes_written", "kernel_ms", "prepare_ms", "write_ms", "fill_ms")}
    tot["write_over_fill"] = tot["write_ms"] / tot["fill_ms"]
    tot["kernel_over_fill"] = tot["kernel_ms"] / tot["fill_ms"]
    out["all_arguments"] = tot
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "lookup_permuted_rate.json")
    ks = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [256]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "lookup_permuted_rate", "commit": commit or None, "usable_rows": USABLE, "cases": {}}
    for K in ks:
        for form in ("montgomery", "canonical"):
            res["cases"]["%d_%s" % (K, form)] = case(eng, K, form)
    eng.close()
    first = res["cases"]["%d_montgomery" % ks[0]]["all_arguments"]
    res["write_over_fill"] = first["write_over_fill"]
    res["kernel_over_fill"] = first["kernel_over_fill"]
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
