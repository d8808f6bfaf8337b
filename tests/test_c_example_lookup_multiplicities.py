"""examples/lookup_multiplicities.c: K = 2 bench-circuit proofs bound by hsw_gadget_bind_column_tables, their range and
spread multiplicity tables counted on the device (hsw_gadget_lookup_runs, hsw_gadget_lookup_multiplicities) and the
totals checked against the closed forms -- from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "lookup_multiplicities.c")


def _build(tmp_path):
    exe = str(tmp_path / "lookup_multiplicities")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_lookup_multiplicities_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_lookup_multiplicities_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    per_range, per_chip = 3 + 2 * 1024 + 16 * 3184 + 64, 16 * 4120
    assert per_range == 53059
    assert "range entries %d, spread entries %d, not in table 0" % (2 * per_range, 2 * per_chip) in out
    got = re.findall(r"proof (\d): range (\d+) entries over (\d+) rows, spread (\d+) entries over (\d+) rows", out)
    assert [(int(h), int(a), int(c)) for h, a, _, c, _ in got] == [(0, per_range, per_chip), (1, per_range, per_chip)]
    assert all(0 < int(u) <= 65536 and 0 < int(v) <= 256 for _, _, u, _, v in got)
    assert re.search(r"verified on the device: \d+ constraints, 0 violations", out)
