"""examples/merkle_device.c: an 8-leaf Merkle tree in ONE hsw_gadget_digest_levels_device call on a whole-digest
gadget with a column image, every inner message read in place from the digests below it, from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import ROOT, _build

SRC = os.path.join(ROOT, "examples", "merkle_device.c")


def test_merkle_device_example_links(tmp_path):
    _build(tmp_path, SRC)


@pytest.mark.gpu
def test_merkle_device_example_runs(tmp_path):
    exe = _build(tmp_path, SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("merkle device ok")
    assert re.search(r"8 leaves, 15 digests in \d+ advice columns, root [0-9a-f]{64}", out)
    assert re.search(r"verified on the device: [1-9]\d* constraints, 0 violations", out)
