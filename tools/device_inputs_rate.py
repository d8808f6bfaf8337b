#!/usr/bin/env python3
"""Messages that already live in device memory: wall time per call of Sha256DynamicConfig.digest_batch_device on
uint8 device tensors, next to what such a caller had to do before -- copy the same tensors to the host (D2H, which
synchronises) and call digest_batch.  Three cases, all gadgets in ONE process, the two timed calls of a case
alternated, 3 warm-ups and the median of 9:
  bench     (i)   the bench circuit, 1 x 16 blocks, whole digest with a column image
  images    (ii)  K = 256 context images of it
  blocks    (iii) 4,096 single-block messages on a plain gadget
No threshold: for tiny batches the host's SHA-extension chain is hard to beat; the point is that the bytes never
leave HBM.  Prints one JSON line and writes it to profiles/device_inputs_rate.json.
usage: device_inputs_rate.py [--only=bench|images|blocks]"""
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
MAX_ROWS = (1 << 17) - 9


def main():
    assert torch.cuda.is_available(), "no HIP device"
    only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
    names = ("bench", "images", "blocks")
    cases = tuple(only) if only else names
    assert all(x in names for x in cases), cases
    eng_i = hsw.WitnessEngine(0, 8, 2, mode=N.HSW_MODE_HALO2_INTERNALS)
    eng_p = hsw.WitnessEngine(0, 8, 2)
    rng = np.random.default_rng(7)

    def make(name):
        if name == "bench":
            g = hsw.Sha256DynamicConfig(eng_i, [1024], True, whole_digest=True)
            g.set_columns(MAX_ROWS)
            msgs = [b"\x01" * 56]
        elif name == "images":
            g = hsw.Sha256DynamicConfig(eng_i, [1024] * 256, True, whole_digest=True, independent=True, context_images=True)
            g.set_columns(MAX_ROWS)
            msgs = [b"\x01" * 56] * 256
        else:
            g = hsw.Sha256DynamicConfig(eng_p, [64] * 4096, False)
            msgs = [rng.integers(0, 256, int(rng.integers(0, 56)), dtype=np.uint8).tobytes() for _ in range(4096)]
        return g, msgs

    out = {}
    for name in cases:
        (gd, msgs), (gh, _) = make(name), make(name)
        # every message a tensor of its own view into one allocation, one byte apart from 16-byte alignment
        at, pos = [], 0
        for m in msgs:
            pos = (pos + 15) // 16 * 16 + 1
            at.append(pos)
            pos += len(m)
        host = np.zeros(pos, dtype=np.uint8)
        for a, m in zip(at, msgs):
            host[a:a + len(m)] = np.frombuffer(m, dtype=np.uint8)
        dev = torch.from_numpy(host).cuda()
        tensors = [dev[a:a + len(m)] for a, m in zip(at, msgs)]
        torch.cuda.synchronize()
        t = {"device": [], "d2h_host": []}
        for i in range(3 + 9):
            for how in ("device", "d2h_host") if i % 2 == 0 else ("d2h_host", "device"):
                g = gd if how == "device" else gh
                g.reset()
                t0 = time.perf_counter()
                if how == "device":
                    res = g.digest_batch_device(tensors)
                else:
                    res = g.digest_batch([x.cpu().numpy().tobytes() for x in tensors])
                t[how].append(time.perf_counter() - t0)
                assert res[-1].output_bytes == hashlib.sha256(msgs[-1]).digest()
        med = {k: float(np.median(v[3:])) * 1e3 for k, v in t.items()}
        out[name] = {"messages": len(msgs), "blocks": int(gd.view().blocks_done), "device_ms": med["device"], "d2h_host_ms": med["d2h_host"],
                     "device_over_d2h_host": med["device"] / med["d2h_host"],
                     "all_ms": {k: [x * 1e3 for x in v[3:]] for k, v in t.items()}}
        gd.close()
        gh.close()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    line = json.dumps({"tool": "device_inputs_rate", "commit": commit or None, "cases": out})
    eng_i.close()
    eng_p.close()
    if not only:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "device_inputs_rate.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
