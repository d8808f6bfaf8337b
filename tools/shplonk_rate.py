#!/usr/bin/env python3
"""hsw_gadget_shplonk_quotient and hsw_gadget_shplonk_open at one prover-sized shape, next to their neighbours: 18
columns of 2^20 Montgomery cells in coefficient form, 2 warm-ups and the median of 7, every call alternated in one
process with hsw_gadget_open over the same columns grouped by point (what GWC opens) and with hsw_gadget_ntt
(lagrange_to_coeff of the same columns).  The shape is this tool's choice, one wide rotation set and two narrow ones as
the bench circuit's queries have: a set of 14 columns at {x}, a set of 3 at {x, x omega}, and a set of 1 column at {x,
x omega, x omega^-1}; T has three points, there are six (set, point) items.  GWC opens the same columns in three groups:
18 at x, 4 at x omega, 1 at x omega^-1.  The columns are random encodings below p; the result of a timed call is not
looked at here (tests/test_gpu_shplonk.py compares every cell with the model).  From the medians:
  ms per call, for the whole shape and for the wide set alone (and the GWC group of the same 14 columns at x);
  multiplies per row BUDGETED -- sum m_i + 3 sum t_i for the quotient (the fold, and per item Horner, the recurrence and
  the weight), M + 2 for the open (the fold of M columns and h, Horner, the recurrence) -- and SPENT: one more per (set,
  point) for the workgroup scan, as DESIGN 5.5d explains for the GWC opening (budget m + 1, spent m + 2 per group);
  ns per row and budgeted multiply, and that price over the NTT's in the same run (a butterfly is one multiply);
  for the alternative this replaces, the time to move the same columns to pinned host memory at the 55 GB/s the README
  measures -- arithmetic, not a measurement.
Nothing is promised: no threshold.  Writes one JSON document (default profiles/shplonk_rate.json) and prints it.
usage: shplonk_rate.py [--out=PATH] [--commit=TEXT (where there is no git to ask)] [log_n]"""
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
COLUMNS = 18
SETS = [(list(range(14)), [0]), ([14, 15, 16], [0, 1]), ([17], [0, 1, 2])]      # (columns, indices into T = {x, x omega, x omega^-1})
WIDE = [(list(range(14)), [0])]
GWC_GROUPS = [list(range(18)), [14, 15, 16, 17], [17]]                        # the same queries grouped by point
PCIE_GB_S = 55.0                            # README: the measured device-to-pinned-host rate


def uniform_cells(shape):
    """random encodings below p: three limbs of 64 random bits, the top one below p's"""
    import torch
    t = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device="cuda")
    t[..., 3] = torch.randint(0, P >> 192, shape, dtype=torch.int64, device="cuda")
    return t.view(torch.uint64)


def budget(sets):
    """(quotient budgeted, quotient spent, open budgeted, open spent) multiplies per row"""
    m, t = sum(len(c) for c, _ in sets), sum(len(p) for _, p in sets)
    return m + 3 * t, m + 4 * t, m + 2, m + 3


def case(eng, k):
    import torch
    torch.manual_seed(1)
    g = hsw.Sha256DynamicConfig(eng, [64], True, whole_digest=True, independent=True, context_images=True)
    g.set_repr(N.HSW_REPR_MONTGOMERY)
    g.set_columns((1 << 17) - 9)
    st = lambda x: x * R % P                                                  # noqa: E731
    n = 1 << k
    cols = uniform_cells((COLUMNS, n))
    coeff = torch.zeros((COLUMNS, n, 4), dtype=torch.uint64, device="cuda")
    quot = torch.zeros((3, n, 4), dtype=torch.uint64, device="cuda")
    h = torch.zeros((n, 4), dtype=torch.uint64, device="cuda")
    h_wide = torch.zeros((n, 4), dtype=torch.uint64, device="cuda")
    w_out = torch.zeros((n, 4), dtype=torch.uint64, device="cuda")
    w = pow(7, (P - 1) >> k, P)
    x, y, v, u = pow(5, 123456789, P), pow(11, 987654321, P), pow(13, 192837465, P), pow(17, 564738291, P)
    T = [st(x), st(x * w % P), st(x * pow(w, -1, P) % P)]
    keys = ("ntt", "quotient", "gwc", "open", "quotient_wide", "gwc_wide", "open_wide")
    t = {key: [] for key in keys}
    reports = {}
    for i in range(2 + 7):
        for what in keys if i % 2 == 0 else keys[::-1]:
            if what == "ntt":
                _, status, rep = g.ntt(k, st(pow(w, -1, P)), cols, out=coeff, scale=st(pow(n, -1, P)))
                status = int(status.any())
            elif what == "quotient":
                _, status, rep = g.shplonk_quotient(n, coeff, SETS, T, st(y), st(v), out=h)
            elif what == "open":                                              # (h is of this iteration or the one before: the same cells)
                _, status, rep = g.shplonk_open(n, coeff, SETS, T, st(y), st(v), st(u), h, out=w_out)
            elif what == "quotient_wide":
                _, status, rep = g.shplonk_quotient(n, coeff, WIDE, T[:1], st(y), st(v), out=h_wide)
            elif what == "open_wide":
                _, status, rep = g.shplonk_open(n, coeff, WIDE, T[:1], st(y), st(v), st(u), h_wide, out=w_out)
            elif what == "gwc":
                _, _, status, rep = g.open(n, coeff, GWC_GROUPS, T, [st(v)] * 3, out=quot)
                status = int(status.any())
            else:
                _, _, status, rep = g.open(n, coeff, [WIDE[0][0]], T[:1], [st(v)], out=quot[:1])
                status = int(status.any())
            assert not status, (what, status, rep)
            reports[what] = rep
            t[what].append(rep["kernel_ms"])
    med = {key: float(np.median(vals[2:])) for key, vals in t.items()}
    ntt_multiply_ns = med["ntt"] * 1e6 / (COLUMNS * (n // 2) * k)

    def row(key, budgeted, spent):
        ms = med[key]
        return {"ms": ms, "ms_min_max": [float(min(t[key][2:])), float(max(t[key][2:]))], "budgeted_multiplies_per_row": budgeted,
                "spent_multiplies_per_row": spent, "ns_per_row": ms * 1e6 / n, "ns_per_row_and_multiply": ms * 1e6 / (n * budgeted),
                "over_ntt_multiply": ms * 1e6 / (n * budgeted) / ntt_multiply_ns,
                "spent_over_ntt_multiply": ms * 1e6 / (n * spent) / ntt_multiply_ns}
    qb, qs, ob, os_ = budget(SETS)
    wqb, wqs, wob, wos = budget(WIDE)
    gwc_b = sum(len(grp) + 1 for grp in GWC_GROUPS)
    rep = reports["quotient"]
    res = {"tile_rows": rep["tile_rows"], "tiles": rep["tiles"], "thread_rows": rep["thread_rows"], "launches": rep["launches"],
           "scratch_bytes": {"quotient": rep["scratch_bytes"], "open": reports["open"]["scratch_bytes"], "gwc": reports["gwc"]["scratch_bytes"]},
           "shplonk": {"quotient": row("quotient", qb, qs), "open": row("open", ob, os_), "both_ms": med["quotient"] + med["open"]},
           "shplonk_wide_set_alone": {"quotient": row("quotient_wide", wqb, wqs), "open": row("open_wide", wob, wos)},
           "gwc": {"three_groups_by_point": row("gwc", gwc_b, gwc_b + len(GWC_GROUPS)),
                   "wide_group_alone": row("gwc_wide", len(WIDE[0][0]) + 1, len(WIDE[0][0]) + 2)},
           "ntt_ms": med["ntt"], "ntt_ns_per_multiply": ntt_multiply_ns,
           "columns_to_pinned_host_ms_at_55_GB_s": COLUMNS * n * 32 / (PCIE_GB_S * 1e9) * 1e3}
    g.close()
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "shplonk_rate.json")
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    k = (nums + [20])[0]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    commits = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--commit=")]
    try:
        commit = commits[0] if commits else subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "shplonk_rate", "commit": commit or None, "columns": COLUMNS, "log_n": k, "cells": "montgomery",
           "sets": [{"columns": c, "points": p} for c, p in SETS], "points": ["x", "x omega", "x omega^-1"], "gwc_groups": GWC_GROUPS,
           "runs": "2 warm-ups, median of 7, every call alternated with hsw_gadget_open (the same columns grouped by point) and "
                   "hsw_gadget_ntt (lagrange_to_coeff of the same columns)"}
    res.update(case(eng, k))
    eng.close()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
