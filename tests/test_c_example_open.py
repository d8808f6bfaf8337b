"""examples/open_columns.c: three columns taken from Lagrange to coefficient form (hsw_gadget_ntt), evaluated at x and
x omega (hsw_gadget_evaluate), opened in two groups (hsw_gadget_open) and the quotients committed (hsw_gadget_msm), all on
the device; the host checks the evaluations by Horner's rule, c(z) = c[0] + z q[0] and one commitment by double-and-add
-- from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "open_columns.c")


def _build(tmp_path):
    exe = str(tmp_path / "open_columns")
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_open_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_open_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    assert re.search(r"lagrange_to_coeff: 3 columns of 2\^10 points, refused 0", out)
    assert re.search(r"evaluate: 4 queries of 3 columns, 1 tile\(s\) of 2048 rows, 2 launches, refused 0", out)
    assert re.search(r"open: 2 groups, 2048 cells written, 3 launches, refused 0", out)
    assert re.search(r"commit\(q\): 2 columns of 1024 rows, refused 0, bad bases 0", out)
    assert re.search(r"W_x = \(0x[0-9a-f]{64}, 0x[0-9a-f]{64}\)", out) and re.search(r"W_x_omega = \(0x[0-9a-f]{64}, 0x[0-9a-f]{64}\)", out)
    for line in ("every evaluation is Horner's over the coefficients: yes", "out_evals is the fold of the evaluations with v: yes",
                 "c(z) = c[0] + z q[0], and the last row of a quotient is zero: yes", "W_x is sum_j q[j] * G[j], byte for byte: yes"):
        assert line in out
