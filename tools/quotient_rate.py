#!/usr/bin/env python3
"""hsw_gadget_quotient at one prover-sized shape, next to its neighbours: ONE proof of a circuit shaped like the
reference's region -- 17 gate columns that carry the FlexGate gate q (a + b c - d) under a selector each, a permutation
of those 17 columns in sets of L = 4 (S = 5), the range lookup (1 + 1 columns) and the spread lookup (2 + 2) -- at
log_rows = 18, e = 2: 69 columns of 2^20 cells, about 2.2 GiB.  Per cell form, 2 warm-ups and the median of 7,
alternated in one process with hsw_gadget_ntt (17 columns of the same size) and a device-to-device copy of the bytes a
call reads.  The whole call, and each family alone (which then pays its own finish).  The columns are random encodings
below p; the result of a timed call is not looked at here (tests/test_gpu_quotient.py compares every cell with the
model).  From the medians, per family:
  ms (the family's own kernel from the report), ns per row;
  the multiplies per row BUDGETED -- what the expressions need with every constant free: one per factor of a monomial
  and per product, one per fold with y, theta folds for the columns beyond the first; l_active (L - R) counts ONE multiply
  by l_active -- and SPENT by the kernel in that cell form (it multiplies l_active into L and into R, one more per set and
  lookup, and theta into the 0 a fold starts from; canonical cells pay the R factors: one scaled l0, l_last, l_active per
  row and product);
  ns per row and budgeted multiply against the NTT's multiply of the same run (a butterfly is one multiply);
  the ratio to the device copy of the columns the family reads;
  for the alternative this replaces, the time to move those columns over PCIe at the 55 GB/s the README measures --
  arithmetic, not a measurement.
Nothing is promised: no threshold.  Writes one JSON document (default profiles/quotient_rate.json) and prints it.
usage: quotient_rate.py [--out=PATH] [--commit=TEXT (where there is no git to ask)] [log_rows]"""
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
M, L, E = 17, 4, 2
S = -(-M // L)
PCIE_GB_S = 55.0                            # README: the measured device-to-pinned-host rate
# the shared index space: 0 .. 16 the gate columns, 17 .. 33 their selectors, 34 the range table, 35 / 36 the spread table
GATES = [[(1, [(M + j, 0), (j, 0)]), (1, [(M + j, 0), (j, 1), (j, 2)]), (P - 1, [(M + j, 0), (j, 3)])] for j in range(M)]
LOOKUPS = [([0], [2 * M]), ([1, 2], [2 * M + 1, 2 * M + 2])]
FAMILIES = ("gates", "permutation", "lookups")


def uniform_cells(shape):
    """random encodings below p: three limbs of 64 random bits, the top one below p's"""
    import torch
    t = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device="cuda")
    t[..., 3] = torch.randint(0, P >> 192, shape, dtype=torch.int64, device="cuda")
    return t.view(torch.uint64)


def multiplies(mont):
    """per row and family: (budgeted, spent in this cell form)"""
    factors = sum(len(f) for g in GATES for _, f in g)
    gates = factors + len(GATES)
    # budgeted, from the expressions: l0 (1 - Z) 1 + its fold, l_last (Z^2 - Z) 2 + 1, a link 1 + 1, a set l_active (L - R) 1 + 1 and 4
    # per column (beta sigma, beta delta^j X, and the two running products); the last 1: w^i from row to row
    perm = 2 + 3 + 2 * (S - 1) + 2 * S + 4 * M + 1
    # a lookup: 2 + 3, the product expression 2 + 2 + 1 + 1, l0 (A' - S') 1 + 1, the last 2 + 1: 16, and theta for the columns beyond the first
    folds = sum(len(i) + len(t) for i, t in LOOKUPS)
    lookups = 16 * len(LOOKUPS) + folds - 2 * len(LOOKUPS)
    # spent: the kernels multiply l_active into both products of a set and of a lookup (1 more each), and theta into the 0 a fold starts from
    spent = {"gates": gates, "permutation": perm + S + (0 if mont else 2 + S), "lookups": 17 * len(LOOKUPS) + folds + (0 if mont else 2 + 2 * len(LOOKUPS)),
             "finish": 1}
    return {"gates": gates, "permutation": perm, "lookups": lookups, "finish": 1}, spent


def case(eng, form, k):
    import torch
    torch.manual_seed(1)
    g = hsw.Sha256DynamicConfig(eng, [64], True, whole_digest=True, independent=True, context_images=True)
    mont = form == "montgomery"
    if mont:
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    g.set_columns((1 << 17) - 9)
    st = lambda x: x * R % P if mont else x                                  # noqa: E731
    n_ext, ln = 1 << (k + E), k + E
    cols = uniform_cells((1, M, n_ext))
    fixed = uniform_cells((M + 3, n_ext))
    sigmas, pz = uniform_cells((M, n_ext)), uniform_cells((1, S, n_ext))
    la, ls, lz = (uniform_cells((1, len(LOOKUPS), n_ext)) for _ in range(3))
    l3 = uniform_cells((3, n_ext))
    h = torch.zeros((1, n_ext, 4), dtype=torch.uint64, device="cuda")
    ntt_out = torch.zeros((M, n_ext, 4), dtype=torch.uint64, device="cuda")
    w = pow(7, (P - 1) >> ln, P)
    ch = [st(pow(c, 123456789, P)) for c in (3, 5, 11, 13)]                  # y, beta, gamma, theta
    reads = {"gates": 2 * M, "permutation": 2 * M + S + 3, "lookups": 6 + 3 * len(LOOKUPS) + 3}   # columns a family reads
    reads["all"] = M + (M + 3) + M + S + 3 * len(LOOKUPS) + 3
    src = torch.zeros((reads["all"] * n_ext * 4,), dtype=torch.int64, device="cuda")
    dst = torch.zeros_like(src)
    common = dict(log_rows=k, log_n=ln, usable_rows=(1 << k) - 6, columns=cols, ys=[ch[0]], omega_ext=st(w), zeta=st(5), fixed=fixed, out=h)
    fam = {"gates": dict(gates=[[(st(c), f) for c, f in gate] for gate in GATES]),
           "permutation": dict(l0=l3[0], l_last=l3[1], l_active=l3[2], betas=[ch[1]], gammas=[ch[2]], perm_columns=list(range(M)), chunk_columns=L,
                               sigmas=sigmas, perm_products=pz, delta=st(7)),
           "lookups": dict(l0=l3[0], l_last=l3[1], l_active=l3[2], betas=[ch[1]], gammas=[ch[2]], lookups=LOOKUPS, permuted_inputs=la, permuted_tables=ls,
                           lookup_products=lz, thetas=[ch[3]])}
    every = dict(common)
    for f in FAMILIES:
        every.update(fam[f])
    t = {key: [] for key in ("ntt", "all") + FAMILIES + tuple("copy_" + f for f in ("all",) + FAMILIES)}
    reports = {}
    order = ("ntt", "all", "copy_all", "gates", "copy_gates", "permutation", "copy_permutation", "lookups", "copy_lookups")
    for i in range(2 + 7):
        for what in order if i % 2 == 0 else order[::-1]:
            if what == "ntt":
                _, status, rep = g.ntt(ln, st(w), cols[0], out=ntt_out)
                t[what].append(rep["kernel_ms"])
            elif what.startswith("copy_"):
                words = reads[what[5:]] * n_ext * 4
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                dst[:words].copy_(src[:words])
                b.record()
                torch.cuda.synchronize()
                t[what].append(a.elapsed_time(b))
                continue
            else:
                kw = every if what == "all" else dict(common, **fam[what])
                _, status, rep = g.quotient(**kw)
                t[what].append(rep)
                reports[what] = rep
            assert not status.any(), (what, status, rep)
    ms = lambda vals: float(np.median(vals[2:]))                             # noqa: E731
    ntt_ms = ms(t["ntt"])
    ntt_multiply_ns = ntt_ms * 1e6 / (M * (n_ext // 2) * ln)
    budget, spent = multiplies(mont)
    res = {"rows_per_thread": reports["all"]["rows_per_thread"], "launches": reports["all"]["launches"], "expressions": reports["all"]["expressions"],
           "scratch_bytes": reports["all"]["scratch_bytes"], "ntt_ms": ntt_ms, "ntt_ns_per_multiply": ntt_multiply_ns, "families": {}}

    def entry(kernel_ms, spread, b, s, columns, copy_key):
        copy_ms = ms(t[copy_key])
        return {"ms": kernel_ms, "ms_min_max": spread, "ns_per_row": kernel_ms * 1e6 / n_ext, "budgeted_multiplies_per_row": b, "spent_multiplies_per_row": s,
                "ns_per_row_and_budgeted_multiply": kernel_ms * 1e6 / (n_ext * b), "over_ntt_multiply": kernel_ms * 1e6 / (n_ext * b) / ntt_multiply_ns,
                "columns_read": columns, "bytes_read_per_row": 32 * columns, "device_copy_ms": copy_ms, "over_device_copy": kernel_ms / copy_ms,
                "columns_over_pcie_ms_at_55_GB_s": columns * n_ext * 32 / (PCIE_GB_S * 1e9) * 1e3}
    for f in FAMILIES:
        own = [r[f + "_ms"] for r in t[f]][2:]                               # the family's kernel in the call that runs it alone
        res["families"][f] = entry(float(np.median(own)), [float(min(own)), float(max(own))], budget[f], spent[f], reads[f], "copy_" + f)
        res["families"][f]["ms_in_the_whole_call"] = ms([r[f + "_ms"] for r in t["all"]])
    fin = [r["finish_ms"] for r in t["all"]][2:]
    res["finish_ms"] = float(np.median(fin))
    whole = [r["kernel_ms"] for r in t["all"]][2:]
    total_b, total_s = sum(budget.values()), sum(spent.values())
    res["whole_call"] = entry(float(np.median(whole)), [float(min(whole)), float(max(whole))], total_b, total_s, reads["all"], "copy_all")
    g.close()
    return res


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    outs = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
    path = outs[0] if outs else os.path.join(ROOT, "profiles", "quotient_rate.json")
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    k = (nums + [18])[0]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    commits = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--commit=")]
    try:
        commit = commits[0] if commits else subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    res = {"tool": "quotient_rate", "commit": commit or None, "log_rows": k, "extension": E, "gate_columns": M, "permutation": {"columns": M, "L": L, "sets": S},
           "lookups": LOOKUPS, "columns": 69, "runs": "2 warm-ups, median of 7, alternated with hsw_gadget_ntt (17 columns of 2^log_n) and device copies",
           "cases": {}}
    for form in ("montgomery", "canonical"):
        res["cases"][form] = case(eng, form, k)
    eng.close()
    text = json.dumps(res)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
