#!/usr/bin/env python3
"""hsw_gadget_ntt at one prover-sized shape, next to its neighbour and to a copy: 8 columns of 2^20 cells as halo2's
lagrange_to_coeff (omega^-1, scale 1 / n), and the same 8 as coeff_to_extended to 2^22 (omega_ext, shift zeta,
input_rows 2^20).  The columns are random encodings below p: the kernels take no data-dependent path short of a refusal.
Alternated in one process, per cell form, 2 warm-ups and the median of 7:
  the two calls            kernel_ms, per launch, and ns per butterfly (columns x N / 2 x log_n of them);
  the permutation product  hsw_gadget_permutation_product at the shape of its own rate tool (m = 17, L = 4, u = 2^20 - 6):
                           ns per (row, column), which is about 8 field multiplies -- the price of a multiply next door;
  a copy                   a device-to-device copy of the bytes ONE launch of each call reads (and writes as many).
From these: the multiplies per butterfly that the neighbour's price implies, and the ratio of a launch to the copy.
After the timed runs the values are checked too: extended_to_coeff returns the coefficients and zeros above them, and
the forward transform of the coefficients returns the columns, cell for cell.
Nothing is promised: no threshold.  Writes one JSON document (default profiles/ntt_rate.json) and prints it.
usage: ntt_rate.py [--out=PATH] [--commit=TEXT (where there is no git to ask)] [columns [log_n [extension_bits]]]"""
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
P = 0x30644e72e131a029b85045b68181585d2833e84879b97091_43e1f593f0000001
R = (1 << 256) % P
MULTIPLIES_PER_ROW_AND_COLUMN = 8           # of the permutation product


def cells(shape):
    """random encodings below p: every 64-bit limb below 2^60"""
    import torch
    return torch.randint(0, 1 << 60, shape + (4,), dtype=torch.int64, device="cuda").view(torch.uint64)


def copy_ms(dst, src):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    dst.view(torch.int64).copy_(src.view(torch.int64))
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def case(eng, form, n_cols, k, e):
    import torch
    torch.manual_seed(1)
    g = hsw.Sha256DynamicConfig(eng, [64], True, whole_digest=True, independent=True, context_images=True)
    mont = form == "montgomery"
    if mont:
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    g.set_columns((1 << 17) - 9)
    st = lambda x: x * R % P if mont else x                                  # noqa: E731
    n, big = 1 << k, 1 << (k + e)
    w, w_ext = pow(7, (P - 1) >> k, P), pow(7, (P - 1) >> (k + e), P)
    cols = cells((n_cols, n))
    coeff = torch.zeros((n_cols, n, 4), dtype=torch.uint64, device="cuda")
    ext = torch.zeros((n_cols, big, 4), dtype=torch.uint64, device="cuda")
    spare = torch.zeros((n_cols, big, 4), dtype=torch.uint64, device="cuda")
    spare_n = torch.zeros((n_cols, n, 4), dtype=torch.uint64, device="cuda")
    m, L, u = 17, 4, (1 << 20) - 6
    S = (m + L - 1) // L
    pc, sig = cells((1, m, u)), cells((m, u))
    z = torch.zeros((1, S, u + 1, 4), dtype=torch.uint64, device="cuda")
    ch = np.array([[3, 5, 7, 11]], dtype=np.uint64)                         # any element below p, as stored
    t = {key: [] for key in ("coeff", "extended", "permutation", "copy_n", "copy_extended")}
    launches = {}
    for i in range(2 + 7):
        order = ("coeff", "permutation", "extended", "copy") if i % 2 == 0 else ("copy", "extended", "permutation", "coeff")
        for what in order:
            if what == "coeff":
                _, status, rep = g.ntt(k, st(pow(w, -1, P)), cols, out=coeff, scale=st(pow(n, -1, P)))
            elif what == "extended":
                _, status, rep = g.ntt(k + e, st(w_ext), coeff, out=ext, input_rows=[n] * n_cols, shift=st(7))
            elif what == "permutation":
                _, status, rep = g.permutation_product(u, L, ch, ch + 1, ch + 2, ch + 3, pc, sig, out=z)
                assert not (status[0] & 6), status
                t[what].append(rep["kernel_ms"])
                continue
            else:
                t["copy_n"].append(copy_ms(spare_n, cols))
                t["copy_extended"].append(copy_ms(spare, ext))
                continue
            assert not status.any() and rep["refused_columns"] == 0, (status, rep)
            t[what].append(rep["kernel_ms"])
            launches[what] = (rep["launches"], rep["twiddle_bytes"], rep["scratch_bytes"])
    # what was timed is also right: extended_to_coeff of the extended columns gives the coefficients back, cell for cell
    back, status, _ = g.ntt(k + e, st(pow(w_ext, -1, P)), ext, out=spare, shift=st(pow(7, -1, P)), scale=st(pow(big, -1, P)), shift_after=True)
    assert not status.any() and torch.equal(back[:, :n].view(torch.int64), coeff.view(torch.int64)) and not back[:, n:].view(torch.int64).any()
    again, status, _ = g.ntt(k, st(w), coeff, out=spare_n)                   # ... and coeff_to_lagrange gives the columns back
    assert not status.any() and torch.equal(again.view(torch.int64), cols.view(torch.int64))
    g.close()
    med = {key + "_ms": float(np.median(v[2:])) for key, v in t.items()}
    price = med["permutation_ms"] * 1e6 / (u * m) / MULTIPLIES_PER_ROW_AND_COLUMN
    med["permutation_ns_per_row_and_column"] = med["permutation_ms"] * 1e6 / (u * m)
    med["permutation_ns_per_multiply"] = price
    for what, log_n, copy in (("coeff", k, "copy_n"), ("extended", k + e, "copy_extended")):
        butterflies = n_cols * (1 << (log_n - 1)) * log_n
        ns = med[what + "_ms"] * 1e6 / butterflies
        med[what] = {"log_n": log_n, "launches": launches[what][0], "twiddle_bytes": launches[what][1], "scratch_bytes": launches[what][2],
                     "ms_min": float(min(t[what][2:])), "ms_max": float(max(t[what][2:])),
                     "ms_per_launch": med[what + "_ms"] / launches[what][0], "ns_per_butterfly": ns,
                     "butterfly_over_neighbour_multiply": ns / price,
                     "bytes_read_per_launch": 32 * n_cols * (1 << log_n), "launch_over_copy": med[what + "_ms"] / launches[what][0] / med[copy + "_ms"]}
    return med


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "ntt_rate.json")
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    n_cols, k, e = (nums + [8, 20, 2][len(nums):])[:3]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    commits = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--commit=")]
    try:
        commit = commits[0] if commits else subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "ntt_rate", "commit": commit or None, "columns": n_cols, "log_n": k, "extension_bits": e,
           "runs": "2 warm-ups, median of 7, alternated with the permutation product and a copy", "cases": {}}
    for form in ("montgomery", "canonical"):
        res["cases"][form] = case(eng, form, n_cols, k, e)
    eng.close()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
