"""examples/k_proofs_columns.c: K = 8 bench-circuit proofs as column images of their own, from plain C99."""
import hashlib
import os
import re
import subprocess

import pytest

from tests.test_c_example import ROOT, _build

SRC = os.path.join(ROOT, "examples", "k_proofs_columns.c")


def test_k_proofs_example_links(tmp_path):
    _build(tmp_path, SRC)


@pytest.mark.gpu
def test_k_proofs_example_runs_both_origins(tmp_path):
    exe = _build(tmp_path, SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    passes = out.split("pass 2:")
    assert len(passes) == 2
    want = [hashlib.sha256(bytes([h + 1] * 56)).hexdigest() for h in range(8)]
    one = int(re.search(r"single-proof gadget at \(2, 131000\): (\d+) columns", out).group(1))
    for text, cols in ((passes[0], 9), (passes[1], one)):
        got = re.findall(r"proof (\d): (\d+) x 131063, digest ([0-9a-f]{64})", text)
        assert [int(h) for h, _, _ in got] == list(range(8))
        assert all(int(c) == cols for _, c, _ in got) and [d for _, _, d in got] == want
        assert re.search(r"verified on the device: \d+ constraints, 0 violations", text)
    assert "proof 0: 9 x 131063" in passes[0]
