#!/usr/bin/env python3
"""HSW_GADGET_SHARED_CONTEXT cost, through the C ABI, gadgets of each layout in the SAME process with their timed
passes alternated (as tools/context_images_rate.py).  Two comparisons, Montgomery and canonical cells:
  one_digest  the bench circuit (one 1024-byte digest, 9 columns at k = 17): flag off (kernel-argument break table)
              against flag on (table-path kernels), same layout
  two_digests two 1024-byte digests with the flag, one hsw_gadget_digest call each (as the shim makes them): back to
              back against an interlude (digest 1 declared 3 columns further on, 100 caller lookup entries)
A pass = reset (+ declaration) + the digest calls, as the shim makes them: set_origin only when the origin changed,
digest 1's origin declared every pass (the same declaration again changes nothing).  interlude_set_origin also calls
set_origin every pass (it drops the declaration: a relayout and a re-declaration per pass).  Prints one JSON line.  usage: shared_context_rate.py [--only=NAME]
(NAME: one of off, on, back_to_back, interlude, interlude_set_origin -- one layout alone, for a profiler run that must not mix them)"""
import ctypes as C
import hashlib
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
MAX_ROWS = (1 << 17) - 9
MSG = bytes(range(256)) * 3


def make(eng, n, shared, form):
    g = hsw.Sha256DynamicConfig(eng, [1024] * n, True, whole_digest=True, shared_context=shared)
    if form == "montgomery":
        g.set_repr(N.HSW_REPR_MONTGOMERY)
    cols = g.set_columns(MAX_ROWS)
    return g, cols


def compare(eng, layouts, form):
    L = eng.lib
    buf = (C.c_uint8 * len(MSG)).from_buffer_copy(MSG)
    st = {}
    for name, (n, shared, decl) in layouts.items():
        g, cols = make(eng, n, shared, form)
        st[name] = dict(g=g, n=n, decl=decl, cols=cols, t=[], res=N.HashResult(), set_origin=name.endswith("set_origin"))
    for name, d in st.items():            # where digest 1 may land: 3 columns past digest 0's end
        if d["decl"]:
            L.hsw_gadget_reset(d["g"].h)
            assert L.hsw_gadget_digest(d["g"].h, buf, len(MSG), 0, C.byref(d["res"])) == 0
            c, r = d["g"].cell_position(d["res"].end_cell - 1)
            d["decl"] = (c + 3, 500, int(d["g"].view().lookup_cells) + 100)
    names = list(st)
    for i in range(3 + 9):                # 3 warm-up passes, then the median of 9; alternated
        for name in names if i % 2 == 0 else names[::-1]:
            d = st[name]
            t1 = time.perf_counter()
            assert L.hsw_gadget_reset(d["g"].h) == 0
            if d["set_origin"]:
                assert L.hsw_gadget_set_origin(d["g"].h, 0, 0, 0, 0) == 0
            for h in range(d["n"]):
                if h == 1 and d["decl"]:
                    assert L.hsw_gadget_set_digest_origin(d["g"].h, 1, *d["decl"]) == 0
                assert L.hsw_gadget_digest(d["g"].h, buf, len(MSG), 0, C.byref(d["res"])) == 0
            d["t"].append(time.perf_counter() - t1)
            d["launch"] = eng.last_launch()
    out = {}
    for name, d in st.items():
        assert bytes(d["res"].output_bytes) == hashlib.sha256(MSG).digest()
        out[name] = {"ms": float(np.median(d["t"][3:])) * 1e3, "columns": int(d["g"].view().columns),
                     "kernel": d["launch"]["kernel"]}
        d["g"].close()
    for other in names[1:]:
        out["%s_over_%s" % (other, names[0])] = out[other]["ms"] / out[names[0]]["ms"]
    return out


def main():
    import torch
    assert torch.cuda.is_available(), "no HIP device"
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    eng = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    groups = {"one_digest": {"off": (1, False, None), "on": (1, True, None)},
              "two_digests": {"back_to_back": (2, True, None), "interlude": (2, True, True),
                              "interlude_set_origin": (2, True, True)}}
    res = {"tool": "shared_context_rate", "commit": commit or None, "message_bytes": len(MSG), "max_rows": MAX_ROWS,
           "cases": {}}
    for form in ("montgomery", "canonical"):
        for gname, lay in groups.items():
            if only:
                lay = {k: v for k, v in lay.items() if k in only}
                if not lay:
                    continue
            res["cases"]["%s_%s" % (gname, form)] = compare(eng, lay, form)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
