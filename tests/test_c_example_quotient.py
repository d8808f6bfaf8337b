"""examples/quotient_columns.c: a satisfied toy circuit taken from base columns to the committed pieces of h(X) on the
device -- lagrange_to_coeff and coeff_to_extended (hsw_gadget_ntt), hsw_gadget_quotient, extended_to_coeff, the pieces
committed (hsw_gadget_msm); the host checks the degree of h, the identity at a point and one commitment -- from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "quotient_columns.c")


def _build(tmp_path):
    exe = str(tmp_path / "quotient_columns")
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_quotient_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_quotient_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    assert re.search(r"lagrange_to_coeff: 24 columns of 2\^4 points, refused 0", out)
    assert re.search(r"coeff_to_extended: 24 columns of 2\^6 points, refused 0", out)
    assert re.search(r"quotient: 1 proof, 17 expressions, 64 cells written, 4 launches, refused 0", out)
    assert re.search(r"extended_to_coeff: 1 column of 2\^6 points, refused 0", out)
    assert re.search(r"commit\(h\): 3 pieces of 16 rows, refused 0, bad bases 0", out)
    assert re.search(r"H_0 = \(0x[0-9a-f]{64}, 0x[0-9a-f]{64}\)", out)
    for line in ("h has degree below 3 n: yes", "the folded expressions at x are h(x) (x^n - 1): yes", "H_0 is sum_j h[j] * G[j], byte for byte: yes"):
        assert line in out
