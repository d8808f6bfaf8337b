"""examples/lookup_permuted.c: K = 2 bench-circuit proofs bound by hsw_gadget_bind_column_tables, the permuted lookup
columns of all three arguments per proof written on the device (hsw_gadget_lookup_permuted) and the two permuted-pair
constraints checked on the host -- from plain C99."""
import os
import re
import subprocess

import pytest

from tests.test_c_example import LIBDIR, ROOT

SRC = os.path.join(ROOT, "examples", "lookup_permuted.c")


def _build(tmp_path):
    exe = str(tmp_path / "lookup_permuted")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), SRC,
           "-L" + LIBDIR, "-lhsw", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_lookup_permuted_example_links(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_lookup_permuted_example_runs(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.strip().endswith("ok")
    u, per_range, per_chip = (1 << 17) - 9, 3 + 2 * 1024 + 16 * 3184 + 64, 16 * 4120
    assert "range: 2 arguments, %d entries, %d cells written, not in table 0" % (2 * per_range, 2 * u * 2) in out
    assert "spread: 4 arguments, %d entries, %d cells written, not in table 0" % (2 * per_chip, 2 * u * 4) in out
    got = re.findall(r"argument (\d) \((range|spread)\): (\d+) distinct rows in A', constraints hold: (yes|NO)", out)
    assert [(int(a), kind, ok) for a, kind, _, ok in got] == [(a, "range" if a < 2 else "spread", "yes") for a in range(6)]
    assert all(1 < int(n) <= (65536 if kind == "range" else 256) for _, kind, n, _ in got)
    assert re.search(r"verified on the device: \d+ constraints, 0 violations", out)
