"""Where the gadget puts every cell, pinned as text: tests/cpp/layout_dump.cpp walks a fixed list of gadgets -- linear
streams, column images at several origins, context images, shared contexts with interludes, 35- and 77-column batches,
layout changes between passes -- against the stand-in HIP runtime (no GPU) and prints their streams, results, cell
positions, context regions, delivered host cells and pack plans.  tests/golden/gadget_layouts.txt is that text as
commit 6cabe45 printed it, before the layout walk and the launch builder were each written once: the layouts of
every later commit must be the same, character for character.

With the argument `tables` the same program prints a second list: the smallest gadgets that reach every form of the
device jump table -- a shared context with an interlude (unbound, and bound by pitch), a plain image with columns by
pointer table, context images and a Context group with image, lookup and chip columns by pointer table -- every column
of a gadget carved out of one allocation in descending address order.  tests/golden/gadget_place_tables.txt is that
text as commit fc92681 printed it, before the table's word layout, the run walk of the download and the frame
descriptors were each written once.  (That commit adds a cell offset taken modulo 2^64 to a pointer, which
UndefinedBehaviorSanitizer's pointer-overflow check reports for a column below column 0: the text was recorded with
that one check off.  The addresses are computed in integers since, and the text is the same.)"""
import difflib
import os
import subprocess

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


def test_place_tables_are_those_of_the_recorded_commit(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra = [_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "layout_dump.cpp"), out)]
    exe = os.path.join(out, "layout_dump_tables")               # (linked as _link_and_run links, run with the argument)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-no-hip-rt", "-Xarch_host", "-fsanitize=address,undefined", "-Wno-option-ignored"]
                       + objs + extra + kernels + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe, "tables"], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert res.stdout.endswith("place table dump done\n")
    want = open(os.path.join(ROOT, "tests", "golden", "gadget_place_tables.txt")).read()
    diff = list(difflib.unified_diff(want.splitlines(), res.stdout.splitlines(), "recorded", "now", lineterm="", n=1))
    assert not diff, "\n".join(diff[:80])
