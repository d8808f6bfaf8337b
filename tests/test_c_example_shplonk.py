"""examples/shplonk_columns.c: four columns taken from Lagrange to coefficient form (hsw_gadget_ntt) and opened with
SHPLONK over three rotation sets of {x, x omega, x omega^-1} (hsw_gadget_shplonk_quotient, hsw_gadget_shplonk_open), each
output committed (hsw_gadget_msm), all on the device; the host checks every cell of h and of w by successive division --
from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "shplonk_columns.c")


def _build(tmp_path):
    exe = str(tmp_path / "shplonk_columns")
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_shplonk_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_shplonk_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    assert re.search(r"lagrange_to_coeff: 4 columns of 2\^10 points, refused 0", out)
    assert re.search(r"shplonk quotient: 3 sets, 6 \(set, point\) items, 1024 cells written, 3 launches, refused 0", out)
    assert re.search(r"shplonk open: 5 columns with h, 1024 cells written, 3 launches, refused 0", out)
    assert re.search(r"H = \(0x[0-9a-f]{64}, 0x[0-9a-f]{64}\)", out) and re.search(r"W = \(0x[0-9a-f]{64}, 0x[0-9a-f]{64}\)", out)
    for line in ("h is sum_i v^i floor(c_i / Z_i) by successive division, cell for cell: yes",
                 "w is (L(X) - L(u)) / ((X - u) zd_0), cell for cell, and the top cells are zero: yes"):
        assert line in out
