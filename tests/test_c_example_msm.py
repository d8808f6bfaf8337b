"""examples/msm_columns.c: a grand-product column Z made on the device (hsw_gadget_permutation_product), committed in
Lagrange form with hsw_gadget_msm against bases uploaded once, and the 64 bytes checked on the host by double-and-add over
the same rows -- from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "msm_columns.c")


def _build(tmp_path):
    exe = str(tmp_path / "msm_columns")
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_msm_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_msm_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    assert re.search(r"commit_lagrange\(Z\): 1019 rows, windows of 8 bits x 32, 1 slice\(s\) of 4096 rows, 3 launches, refused 0, bad bases 0", out)
    assert re.search(r"Z: 1019 rows, closes: yes, constant: no", out)
    assert "the commitment is sum_j Z[j] * G[j], byte for byte: yes" in out
