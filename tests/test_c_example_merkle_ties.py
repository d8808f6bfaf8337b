"""examples/merkle_ties.c: the 8-leaf tree of examples/merkle_device.c, the 448 copy constraints between its digests
from hsw_gadget_ties, one of them resolved to FlexGate positions, all of them checked on the device -- from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import ROOT, _build

SRC = os.path.join(ROOT, "examples", "merkle_ties.c")


def test_merkle_ties_example_links(tmp_path):
    _build(tmp_path, SRC)


@pytest.mark.gpu
def test_merkle_ties_example_runs(tmp_path):
    exe = _build(tmp_path, SRC)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("merkle ties ok")
    assert re.search(r"^448 ties, 0 prefix bytes untied$", out, flags=re.M)
    assert re.search(r"tie 447: output byte 31 of digest 13 at \(column \d+, row \d+\) = input byte 63 of digest 14 at \(column \d+, row \d+\)", out)
    assert re.search(r"ties checked on the device: 448 pairs, 0 violations", out)
