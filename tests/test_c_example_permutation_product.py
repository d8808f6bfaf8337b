"""examples/permutation_product.c: two leaves and their parent hashed in circuit, the 64 copy constraints of
hsw_gadget_ties turned into sigma columns on the host, the permutation argument's grand products written on the device
(hsw_gadget_permutation_product) over the advice columns where the digests wrote them, and the argument's recurrence
checked on the host row by row -- from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "permutation_product.c")


def _build(tmp_path):
    exe = str(tmp_path / "permutation_product")
    cmd = ["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_permutation_product_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_permutation_product_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    u = (1 << 17) - 9
    got = re.search(r"1 proof, (\d+) products over (\d+) columns, (\d+) cells written, open 0, refused 0, tiles of 1024 rows", out)
    assert got
    S, m, written = (int(x) for x in got.groups())
    assert S == (m + 1) // 2 and m >= 2 and written == S * (u + 1)
    assert re.findall(r"chunk (\d+): starts where the last one ended and satisfies the recurrence: (yes|NO)", out) == [(str(s), "yes") for s in range(S)]
    assert "the last value is 1: yes" in out
    assert re.search(r"ties checked on the device: 64 pairs, 0 violations", out)
