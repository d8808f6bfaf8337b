"""examples/bound_every_column.c: K = 2 bench-circuit proofs with EVERY advice column a hipMalloc of its own -- 18 image
columns, 2 lookup columns and 8 chip columns (hsw_gadget_bind_column_tables) -- from plain C99."""
import hashlib
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "bound_every_column.c")


def _build(tmp_path):
    exe = str(tmp_path / "bound_every_column")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_bound_every_column_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_bound_every_column_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    want = [hashlib.sha256(bytes([h + 1] * 56)).hexdigest() for h in range(2)]
    got = re.findall(r"proof (\d): (\d+) \+ 1 \+ 4 columns by pointer, digest ([0-9a-f]{64})", out)
    assert [int(h) for h, _, _ in got] == [0, 1]
    assert all(int(c) == 9 for _, c, _ in got) and [d for _, _, d in got] == want
    assert re.search(r"verified on the device: \d+ constraints, 0 violations", out)
