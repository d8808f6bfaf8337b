"""examples/lookup_product.c: K = 2 bench-circuit proofs bound by hsw_gadget_bind_column_tables, the permuted pair and
then the grand-product column Z of all three lookup arguments per proof written on the device
(hsw_gadget_lookup_permuted, hsw_gadget_lookup_product), and the argument's recurrence checked on the host row by row --
from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "lookup_product.c")


def _build(tmp_path):
    exe = str(tmp_path / "lookup_product")
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_lookup_product_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_lookup_product_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    u, per_range, per_chip = (1 << 17) - 9, 3 + 2 * 1024 + 16 * 3184 + 64, 16 * 4120 // 2
    assert re.search(r"range: 2 arguments, %d cells written, open 0, refused 0, tiles of \d+ rows" % (2 * (u + 1)), out)
    assert re.search(r"spread: 4 arguments, %d cells written, open 0, refused 0, tiles of \d+ rows" % (4 * (u + 1)), out)
    got = re.findall(r"argument (\d) \((range|spread)\): (\d+) assigned rows, Z closes and satisfies the recurrence: (yes|NO)", out)
    assert [(int(a), kind, int(n), ok) for a, kind, n, ok in got] == [(a, "range" if a < 2 else "spread", per_range if a < 2 else per_chip, "yes")
                                                                     for a in range(6)]
    assert re.search(r"verified on the device: \d+ constraints, 0 violations", out)
