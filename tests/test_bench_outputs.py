"""bench.py's plain / --full split and --dump-outputs.

* a plain run prints the headline line only: no extras, no CPU baseline, no figures that need runs of their own;
* --full adds them;
* --dump-outputs writes the last timed step's four outputs as float64 .npy files whose rows do not depend on where
  the buffers were placed or on --full, and whose next_states are the SHA-256 states of the benchmark's messages."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MSG = 512
SHAPES = {"gate": (1 << 18, 8), "dense": (1 << 16, 8), "spread": (1 << 16, 8), "next_states": (N_MSG, 8)}


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HSW_BENCH_SAME_DEVICE")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env,
                          capture_output=True, text=True, timeout=600)


def test_steps_below_one_is_refused():
    r = _bench("--steps", "0")
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Three runs of the same workload: plain with the placement search, plain on plain buffers, --full."""
    d = tmp_path_factory.mktemp("bench_dump")
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--messages-per-gpu", str(N_MSG)]
    res = {}
    for name, extra in (("plain", []), ("plain_unplaced", ["--placement-candidates", "1"]),
                        ("full", ["--full", "--no-cpu-baseline"])):
        r = _bench(*(common + extra + ["--dump-outputs", str(d / name)]))
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        res[name] = (json.loads(lines[0]), d / name)
    return res


@pytest.mark.gpu
def test_plain_line_holds_the_headline_only(runs):
    for name in ("plain", "plain_unplaced"):
        j = runs[name][0]
        assert j["metric"].startswith("SHA256 compression blocks/sec") and j["unit"] == "blocks/s"
        assert j["higher_is_better"] is True and j["dtype"] == "u32/u64"
        assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
        assert j["full"] is False and j["extra"] == {} and "cpu_baseline" not in j
        assert "calibrated_fill_GBps" not in j["roofline"] and "kernel_ms_engine_events" not in j["roofline"]
    assert runs["plain_unplaced"][0]["roofline"]["placement"]["candidates"] == 1


@pytest.mark.gpu
def test_full_line_adds_the_side_measurements(runs):
    j = runs["full"][0]
    assert j["full"] is True and j["steps"] == 2
    assert "kernel_ms" in j["extra"]["montgomery_repr"] and j["extra"]["verify_on_device"]["violations"] == 0
    assert j["roofline"]["calibrated_fill_GBps"] > 0 and j["roofline"]["kernel_ms_engine_events"] > 0


@pytest.mark.gpu
def test_dumped_outputs_are_float64_placement_independent_and_right(runs):
    ref = {}
    for name in ("plain", "plain_unplaced", "full"):
        d = runs[name][1]
        assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in SHAPES)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
        for n, shape in SHAPES.items():
            a = np.load(os.path.join(d, n + ".npy"))
            assert a.dtype == np.float64 and a.shape == shape, (name, n, a.dtype, a.shape)
            assert np.all((a >= 0) & (a < 2.0 ** 32) & (a == np.floor(a)))
            if n in ref:
                assert np.array_equal(a, ref[n]), (name, n)
            else:
                ref[n] = a
    # next_states is written whole: row i is the SHA-256 state after message i (seed 0xC3, 55-byte messages)
    msgs = np.random.default_rng(0xC3).integers(0, 256, (N_MSG, 55), dtype=np.uint8)
    words = ref["next_states"].astype(np.uint32)
    for i in (0, 1, N_MSG - 1):
        assert b"".join(int(x).to_bytes(4, "big") for x in words[i]) == hashlib.sha256(msgs[i].tobytes()).digest()
    assert np.count_nonzero(ref["gate"]) > 0 and np.count_nonzero(ref["spread"]) > 0
