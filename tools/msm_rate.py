#!/usr/bin/env python3
"""hsw_gadget_msm at one prover-sized shape, next to its neighbour: 8 columns of 2^20 cells committed against 2^20 bases,
per cell form, 2 warm-ups and the median of 7, alternated in one process with hsw_gadget_ntt (lagrange_to_coeff of the
same columns).  Two sets of columns:
  uniform        random encodings below r: every bucket of every window fills alike;
  witness-like   bits, bytes, zero runs and a few full values, as an advice column holds them: in window 0 most rows of a
                 slice fall into a few buckets, and the windows above are nearly empty.
The bases are multiples of (1, 2) made on the HOST for a few hundred rows and repeated: the kernels take no path that
depends on a base short of (0, 0), and the result of the timed call is not looked at here (tests/test_gpu_msm.py compares
every point with the model).  From the medians:
  ms per column for both sets, and the witness-like set's time over the uniform set's;
  ns per mixed addition (windows x rows of them per column, uniform set);
  the NTT's price of a multiply in the same run (a butterfly is one multiply: columns x N / 2 x log_n of them), and the
  ratio of the addition to 11 such multiplies -- the arithmetic floor of the method, so how far the kernel is from it.
The alternatives to the defaults (window_bits x slice_rows) are timed on the uniform and the witness-like set with
Montgomery cells, one warm-up and the median of 3.  Nothing is promised: no threshold.  Writes one JSON document
(default profiles/msm_rate.json) and prints it.
usage: msm_rate.py [--out=PATH] [--commit=TEXT (where there is no git to ask)] [--no-alternatives] [columns [log_n]]"""
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
Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = (1 << 256) % P
MULTIPLIES_PER_MIXED_ADDITION = 11
ALTERNATIVES = ((8, 1024), (8, 2048), (8, 4096), (8, 8192), (8, 16384), (7, 4096), (6, 4096))


def host_bases(n, distinct=256):
    """(n, 8) uint64: k * (1, 2) for k = 1 .. distinct in Montgomery form mod q, repeated"""
    def add(p, q):
        (x1, y1), (x2, y2) = p, q
        lam = (3 * x1 * x1 * pow(2 * y1, -1, Q) if p == q else (y2 - y1) * pow(x2 - x1, -1, Q)) % Q
        x3 = (lam * lam - x1 - x2) % Q
        return x3, (lam * (x1 - x3) - y1) % Q
    pts, p = [], (1, 2)
    for _ in range(distinct):
        pts.append(p)
        p = add(p, (1, 2))
    words = [[((v << 256) % Q >> (64 * i)) & (2**64 - 1) for v in pt for i in range(4)] for pt in pts]
    return np.tile(np.array(words, dtype=np.uint64), (n // distinct + 1, 1))[:n]


def uniform_cells(shape):
    """random encodings below r with every digit of every window spread out: three limbs of 64 random bits, the top one
    below r's (limbs below 2^60 would leave the windows on bits 60 .. 63 of a canonical cell a sixteenth of their buckets)"""
    import torch
    t = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device="cuda")
    t[..., 3] = torch.randint(0, P >> 192, shape, dtype=torch.int64, device="cuda")
    return t.view(torch.uint64)


def witness_cells(shape, mont):
    """bits, bytes, zeros and one full value in 16, in runs of 64 rows of one kind"""
    import torch
    n_cols, n = shape
    kind = torch.randint(0, 16, (n_cols, n // 64, 1), device="cuda").expand(-1, -1, 64).reshape(n_cols, n)
    small = torch.where(kind < 6, torch.randint(0, 2, (n_cols, n), device="cuda"),
                        torch.where(kind < 11, torch.randint(0, 256, (n_cols, n), device="cuda"), torch.zeros((n_cols, n), dtype=torch.int64, device="cuda")))
    out = torch.zeros((n_cols, n, 4), dtype=torch.int64, device="cuda")
    if mont:                                                                 # x R mod r for x < 256: a table
        table = torch.from_numpy(np.array([[(x * R % P >> (64 * i)) & (2**64 - 1) for i in range(4)] for x in range(256)], dtype=np.uint64).view(np.int64)).cuda()
        out = table[small]
    else:
        out[:, :, 0] = small
    full = uniform_cells((n_cols, n)).view(torch.int64)
    return torch.where((kind == 15).unsqueeze(-1), full, out).contiguous().view(torch.uint64)


def case(eng, form, n_cols, k, alternatives):
    import torch
    torch.manual_seed(1)
    g = hsw.Sha256DynamicConfig(eng, [64], True, whole_digest=True, independent=True, context_images=True)
    mont = form == "montgomery"
    if mont:
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    g.set_columns((1 << 17) - 9)
    st = lambda x: x * R % P if mont else x                                  # noqa: E731
    n = 1 << k
    bases = torch.from_numpy(host_bases(n).view(np.int64)).cuda().view(torch.uint64)
    sets = {"uniform": uniform_cells((n_cols, n)), "witness": witness_cells((n_cols, n), mont)}
    coeff = torch.zeros((n_cols, n, 4), dtype=torch.uint64, device="cuda")
    w = pow(7, (P - 1) >> k, P)
    t = {key: [] for key in ("uniform", "witness", "ntt")}
    reports = {}
    for i in range(2 + 7):
        order = ("uniform", "ntt", "witness") if i % 2 == 0 else ("witness", "ntt", "uniform")
        for what in order:
            if what == "ntt":
                _, status, rep = g.ntt(k, st(pow(w, -1, P)), sets["uniform"], out=coeff, scale=st(pow(n, -1, P)))
            else:
                _, status, rep = g.msm(bases, sets[what])
                reports[what] = rep
            assert not status.any() and rep["refused_columns"] == 0, (status, rep)
            t[what].append(rep["kernel_ms"])
    med = {key + "_ms": float(np.median(v[2:])) for key, v in t.items()}
    rep = reports["uniform"]
    additions = rep["windows"] * n
    ntt_multiply_ns = med["ntt_ms"] * 1e6 / (n_cols * (n // 2) * k)
    add_ns = med["uniform_ms"] * 1e6 / (n_cols * additions)
    res = {"window_bits": rep["window_bits"], "windows": rep["windows"], "slice_rows": rep["slice_rows"], "slices": rep["slices"],
           "launches": rep["launches"], "scratch_bytes": rep["scratch_bytes"], "finish_ms": rep["finish_ms"],
           "uniform_ms_per_column": med["uniform_ms"] / n_cols, "witness_ms_per_column": med["witness_ms"] / n_cols,
           "uniform_ms_min_max": [float(min(t["uniform"][2:])), float(max(t["uniform"][2:]))],
           "witness_ms_min_max": [float(min(t["witness"][2:])), float(max(t["witness"][2:]))],
           "witness_over_uniform": med["witness_ms"] / med["uniform_ms"],
           "ns_per_mixed_addition": add_ns, "ntt_ms": med["ntt_ms"], "ntt_ns_per_multiply": ntt_multiply_ns,
           "addition_over_11_ntt_multiplies": add_ns / (MULTIPLIES_PER_MIXED_ADDITION * ntt_multiply_ns)}
    if alternatives:
        res["alternatives"] = []
        for c, s in ALTERNATIVES:
            row = {"window_bits": c, "slice_rows": s}
            for what in ("uniform", "witness"):
                ms = []
                for _ in range(1 + 3):
                    _, status, rep = g.msm(bases, sets[what], window_bits=c, slice_rows=s)
                    assert not status.any()
                    ms.append(rep["kernel_ms"])
                row[what + "_ms_per_column"] = float(np.median(ms[1:])) / n_cols
            res["alternatives"].append(row)
    g.close()
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "msm_rate.json")
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    n_cols, k = (nums + [8, 20][len(nums):])[:2]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    commits = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--commit=")]
    try:
        commit = commits[0] if commits else subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "msm_rate", "commit": commit or None, "columns": n_cols, "log_n": k,
           "runs": "2 warm-ups, median of 7, alternated with hsw_gadget_ntt (lagrange_to_coeff of the uniform columns); alternatives: 1 warm-up, median of 3",
           "cases": {}}
    for form in ("montgomery", "canonical"):
        res["cases"][form] = case(eng, form, n_cols, k, "--no-alternatives" not in sys.argv and form == "montgomery")
    eng.close()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
