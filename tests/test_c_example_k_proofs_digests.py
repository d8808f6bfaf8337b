"""examples/k_proofs_digests.c: K = 4 proofs of a two-digest circuit with an interlude (hsw_gadget_create_contexts),
from plain C99: verified on the device, every proof read back through hsw_gadget_context_region."""
import hashlib
import os
import re
import subprocess

import pytest

from tests.test_c_example import ROOT, _build

SRC = os.path.join(ROOT, "examples", "k_proofs_digests.c")


def test_k_proofs_digests_example_links(tmp_path):
    _build(tmp_path, SRC)


@pytest.mark.gpu
def test_k_proofs_digests_example_runs(tmp_path):
    exe = _build(tmp_path, SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    assert "8 digests, 2 expansion launches" in out                   # one per digest index, not one per digest
    assert re.search(r"verified on the device: \d+ constraints, 0 violations", out)
    got = re.findall(r"proof (\d) digest (\d): starts at \((\d+), (\d+)\) of (\d+) x 131063, digest ([0-9a-f]{64})", out)
    assert [(int(c), int(j)) for c, j, *_ in got] == [(c, j) for c in range(4) for j in range(2)]
    want = [hashlib.sha256(m).hexdigest() for c in range(4) for m in (bytes([c + 1] * 100), bytes([0x80 + c] * 55))]
    assert [g[5] for g in got] == want
    # every proof is laid out alike: digest 0 at the origin, digest 1 behind the interlude, at the same place in every image
    starts = {(int(j), int(col), int(row)) for _, j, col, row, _, _ in got}
    assert len(starts) == 2 and (0, 0, 0) in starts
    assert len({g[4] for g in got}) == 1
