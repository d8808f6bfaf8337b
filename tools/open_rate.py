#!/usr/bin/env python3
"""hsw_gadget_open and hsw_gadget_evaluate at one prover-sized shape, next to their neighbour: columns of 2^20 cells in
coefficient form, per cell form, 2 warm-ups and the median of 7, alternated in one process with hsw_gadget_ntt
(lagrange_to_coeff of the same columns).  The shapes are modelled on the openings of the bench circuit under GWC: of 16
columns, ONE group of 14 at x and ONE group of 3 at x omega (a column opened at both is in both), and the same 17
(column, point) pairs as the queries of evaluate.  The counts are this tool's choice: the bench circuit's own depend on
its configuration, and what matters here is one wide group and one narrow one.  The columns are random encodings below
p; the result of a timed call is not looked at here (tests/test_gpu_open.py compares every cell with the model).  From
the medians:
  ms per group, each group timed in a call of its own, and both in one call;
  ns per row, and ns per row and multiply with the BUDGETED multiplies in the denominator: m + 1 for a group of m columns
  (m - 1 for the fold, one for the sums, one for the quotient), P for a column evaluated at P points;
  the NTT's price of a multiply in the same run (a butterfly is one multiply: columns x N / 2 x log_n of them), and the
  ratio of the two;
  for the alternative this replaces, the time to move the same columns to pinned host memory at the 55 GB/s the README
  measures -- arithmetic, not a measurement.
Nothing is promised: no threshold.  Writes one JSON document (default profiles/open_rate.json) and prints it.
usage: open_rate.py [--out=PATH] [--commit=TEXT (where there is no git to ask)] [log_n]"""
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
COLUMNS = 16
GROUP_X = list(range(14))                   # at x
GROUP_XW = [0, 14, 15]                      # at x omega: a rotation of column 0, and two columns opened there alone
PCIE_GB_S = 55.0                            # README: the measured device-to-pinned-host rate


def uniform_cells(shape):
    """random encodings below p: three limbs of 64 random bits, the top one below p's"""
    import torch
    t = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device="cuda")
    t[..., 3] = torch.randint(0, P >> 192, shape, dtype=torch.int64, device="cuda")
    return t.view(torch.uint64)


def case(eng, form, k):
    import torch
    torch.manual_seed(1)
    g = hsw.Sha256DynamicConfig(eng, [64], True, whole_digest=True, independent=True, context_images=True)
    mont = form == "montgomery"
    if mont:
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    g.set_columns((1 << 17) - 9)
    st = lambda x: x * R % P if mont else x                                  # noqa: E731
    n = 1 << k
    cols = uniform_cells((COLUMNS, n))
    coeff = torch.zeros((COLUMNS, n, 4), dtype=torch.uint64, device="cuda")
    quot = torch.zeros((2, n, 4), dtype=torch.uint64, device="cuda")
    w = pow(7, (P - 1) >> k, P)
    x, v = pow(5, 123456789, P), pow(11, 987654321, P)
    points, challenges = [st(x), st(x * w % P)], [st(v), st(v)]
    queries = [(b, 0) for b in GROUP_X] + [(b, 1) for b in GROUP_XW]
    t = {key: [] for key in ("ntt", "open_x", "open_xw", "open_both", "evaluate")}
    reports = {}
    for i in range(2 + 7):
        order = ("ntt", "open_x", "evaluate", "open_xw", "open_both")
        for what in order if i % 2 == 0 else order[::-1]:
            if what == "ntt":
                _, status, rep = g.ntt(k, st(pow(w, -1, P)), cols, out=coeff, scale=st(pow(n, -1, P)))
            elif what == "evaluate":
                _, status, rep = g.evaluate(n, coeff, points, queries)
            elif what == "open_x":
                _, _, status, rep = g.open(n, coeff, [GROUP_X], points[:1], challenges[:1], out=quot[:1])
            elif what == "open_xw":
                _, _, status, rep = g.open(n, coeff, [GROUP_XW], points[1:], challenges[1:], out=quot[1:])
            else:
                _, _, status, rep = g.open(n, coeff, [GROUP_X, GROUP_XW], points, challenges, out=quot)
            assert not status.any(), (what, status, rep)
            reports[what] = rep
            t[what].append(rep["kernel_ms"])
    med = {key: float(np.median(vals[2:])) for key, vals in t.items()}
    ntt_multiply_ns = med["ntt"] * 1e6 / (COLUMNS * (n // 2) * k)

    def group(key, m):
        ms = med[key]
        return {"columns": m, "budgeted_multiplies_per_row": m + 1, "ms": ms, "ms_min_max": [float(min(t[key][2:])), float(max(t[key][2:]))],
                "ns_per_row": ms * 1e6 / n, "ns_per_row_and_multiply": ms * 1e6 / (n * (m + 1)),
                "over_ntt_multiply": ms * 1e6 / (n * (m + 1)) / ntt_multiply_ns}
    rep = reports["open_both"]
    res = {"tile_rows": rep["tile_rows"], "tiles": rep["tiles"], "thread_rows": rep["thread_rows"], "launches": rep["launches"],
           "scratch_bytes": rep["scratch_bytes"],
           "open": {"group_at_x": group("open_x", len(GROUP_X)), "group_at_x_omega": group("open_xw", len(GROUP_XW)),
                    "both_in_one_call_ms": med["open_both"], "both_ms_per_group": med["open_both"] / 2},
           "evaluate": {"queries": len(queries), "columns_read": COLUMNS, "budgeted_multiplies_per_row": len(queries), "ms": med["evaluate"],
                        "ms_min_max": [float(min(t["evaluate"][2:])), float(max(t["evaluate"][2:]))],
                        "ns_per_row": med["evaluate"] * 1e6 / n, "ns_per_row_and_multiply": med["evaluate"] * 1e6 / (n * len(queries)),
                        "over_ntt_multiply": med["evaluate"] * 1e6 / (n * len(queries)) / ntt_multiply_ns,
                        "scratch_bytes": reports["evaluate"]["scratch_bytes"]},
           "ntt_ms": med["ntt"], "ntt_ns_per_multiply": ntt_multiply_ns,
           "columns_to_pinned_host_ms_at_55_GB_s": COLUMNS * n * 32 / (PCIE_GB_S * 1e9) * 1e3}
    g.close()
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "open_rate.json")
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    k = (nums + [20])[0]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    commits = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--commit=")]
    try:
        commit = commits[0] if commits else subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "open_rate", "commit": commit or None, "columns": COLUMNS, "log_n": k, "group_at_x": GROUP_X, "group_at_x_omega": GROUP_XW,
           "runs": "2 warm-ups, median of 7, alternated with hsw_gadget_ntt (lagrange_to_coeff of the same columns)", "cases": {}}
    for form in ("montgomery", "canonical"):
        res["cases"][form] = case(eng, form, k)
    eng.close()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
