"""The scratch that the calls of the proving round share (hsw_gadget::scratch, csrc/hsw_gadget_call.hpp) without a GPU:
tests/cpp/round_scratch_lifecycle.cpp runs every family of calls on one gadget, small and large needs mixed, under
ASan + UBSan + LeakSanitizer with the stand-in HIP runtime -- an upload or a read-back longer than the scratch is an
ordinary ASan report there."""
import os
import subprocess

from tests.test_host_sanitizers import CSRC, ROOT, _compile, _link_and_run, host_objects  # noqa: F401 (fixture)

ROUND = ("permuted", "product", "permutation", "ntt", "msm", "open", "shplonk", "quotient")
# the kernels those entry points refer to (hsw_gadget_permuted.cpp: the counting kernel of the lookup entries too)
ROUND_KERNELS = ("hsw_lookup_counts.o", "hsw_lookup_permuted.o", "hsw_lookup_product.o", "hsw_permutation_product.o", "hsw_ntt.o", "hsw_msm.o", "hsw_open.o",
                 "hsw_shplonk.o", "hsw_quotient.o")


def test_round_scratch_lifecycle_under_asan_with_a_stub_runtime(host_objects):  # noqa: F811
    hipcc, out, objs, kernels = host_objects
    extra_kernels = [os.path.join(CSRC, k) for k in ROUND_KERNELS]
    if not all(os.path.exists(k) for k in extra_kernels):
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    extra = [_compile(hipcc, os.path.join(CSRC, "hsw_gadget_%s.cpp" % f), out) for f in ("lookup",) + ROUND]
    extra.append(_compile(hipcc, os.path.join(ROOT, "tests", "cpp", "round_scratch_lifecycle.cpp"), out))
    res = _link_and_run(hipcc, out, objs + extra, kernels + extra_kernels, "round_scratch_lifecycle", leaks=1)
    assert res.returncode == 0, (res.stdout + res.stderr)[-6000:]
    assert "round scratch lifecycle ok" in res.stdout
