"""examples/bound_columns.c: K = 8 bench-circuit proofs written straight into one caller-owned slab per proof
(hsw_gadget_bind_region), from plain C99."""
import hashlib
import os
import re
import subprocess

import pytest

from tests.test_c_example import ROOT, _build

SRC = os.path.join(ROOT, "examples", "bound_columns.c")


def test_bound_columns_example_links(tmp_path):
    _build(tmp_path, SRC)


@pytest.mark.gpu
def test_bound_columns_example_runs(tmp_path):
    exe = _build(tmp_path, SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    want = [hashlib.sha256(bytes([h + 1] * 56)).hexdigest() for h in range(8)]
    got = re.findall(r"proof (\d): (\d+) columns of 131072 cells, digest ([0-9a-f]{64})", out)
    assert [int(h) for h, _, _ in got] == list(range(8))
    assert all(int(c) == 9 for _, c, _ in got) and [d for _, _, d in got] == want
    assert re.search(r"verified on the device: \d+ constraints, 0 violations", out)
