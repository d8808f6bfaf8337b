"""examples/ntt_columns.c: a grand-product column Z made on the device (hsw_gadget_permutation_product) and taken through
halo2's lagrange_to_coeff, coeff_to_extended and extended_to_coeff with hsw_gadget_ntt, the coefficients checked by Horner
on the domain and on the coset and the round trip cell for cell -- from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "ntt_columns.c")


def _build(tmp_path):
    exe = str(tmp_path / "ntt_columns")
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_ntt_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_ntt_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    assert re.search(r"Z: 4091 rows, closes: yes, constant: no", out)
    got = re.findall(r"(\w+): 2\^(\d+) points, (\d+) launch\(es\), (\d+) cells written, refused 0", out)
    assert got == [("lagrange_to_coeff", "12", "2", "4096"), ("coeff_to_extended", "14", "2", "16384"), ("extended_to_coeff", "14", "2", "16384")]
    assert "the coefficients evaluate to Z on the domain (0 on the blinding rows): yes" in out
    assert "the extended column is the polynomial on the coset: yes" in out
    assert "extended_to_coeff returns the coefficients cell for cell, zeros above them: yes" in out
