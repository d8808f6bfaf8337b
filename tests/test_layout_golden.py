"""Where the gadget puts every cell, pinned as text: tests/cpp/layout_dump.cpp walks a fixed list of gadgets -- linear
streams, column images at several origins, context images, shared contexts with interludes, 35- and 77-column batches,
layout changes between passes -- against the stand-in HIP runtime (no GPU) and prints their streams, results, cell
positions, context regions, delivered host cells and pack plans.  tests/golden/gadget_layouts.txt is that text as
commit 6cabe45 printed it, before the layout walk and the launch builder were each written once: the layouts of
every later commit must be the same, character for character."""
import difflib
import os

from tests.test_host_sanitizers import ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)


def test_layouts_are_those_of_the_recorded_commit(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "layout_dump.cpp"), out)]
    res = _link_and_run(hipcc, out, objs + extra, kernels, "layout_dump", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert res.stdout.endswith("layout dump done\n")
    want = open(os.path.join(ROOT, "tests", "golden", "gadget_layouts.txt")).read()
    diff = list(difflib.unified_diff(want.splitlines(), res.stdout.splitlines(), "recorded", "now", lineterm="", n=1))
    assert not diff, "\n".join(diff[:80])
