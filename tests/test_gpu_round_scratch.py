"""The calls of the proving round share one scratch on the device (hsw_gadget::scratch, csrc/hsw_gadget_call.hpp): on ONE
gadget, in Montgomery cells, an NTT and an opening, then a lookup grand product and a quotient that each replace the
block by a larger one or stage over what the earlier calls left, then the first NTT and opening again with the first
inputs.  Every call is checked as in its own test -- against the Python models of tests/ntt_model.py, tests/open_model.py
and tests/quotient_model.py and the recurrence of tests/test_gpu_lookup_product.py, with the sentinel cells around every
column -- and the repeated calls must give the bytes they gave the first time.  These are the smallest shapes at which
sharing could go wrong: a later call writes over what an earlier one staged, and an earlier family is used again after
a larger one has replaced the block."""
import numpy as np
import pytest

from tests.constraint_check import P_INT
from tests.test_gpu_lookup_product import Case as ProductCase, spread_cfg
from tests.test_gpu_ntt import Case as NttCase
from tests.test_gpu_open import Case as OpenCase, random_column
from tests.test_gpu_quotient import Case as QuotientCase, toy_gates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_int(hsw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    e = hsw.WitnessEngine(0, 8, 2, mode=hsw._native.HSW_MODE_HALO2_INTERNALS)
    yield e
    e.close()


def test_calls_of_a_round_on_one_gadget_do_not_disturb_each_other(hsw, eng_int):
    N = hsw._native
    mont = True
    cfg = spread_cfg(hsw, eng_int, mont)                                      # three proofs: six spread arguments
    rng = np.random.default_rng(7001)
    # ---- the NTT of 2 columns at log_n = 9; an opening of a group of 2 columns and a group of 1, at 512 rows
    ntt = NttCase(cfg, hsw, 9, mont, [512, 512], 7002)
    ntt_first, status, _ = ntt.run(launches=1)
    assert not status.any()
    opening = OpenCase(cfg, hsw, 512, mont, [random_column(rng, 512) for _ in range(3)], n_quotients=2)
    groups, points, challenges = [[0, 1], [2]], random_column(rng, 2), random_column(rng, 2)
    q_first, evals_first, status, _ = opening.open(groups, points, challenges)
    assert not status.any()
    # ---- the lookup grand product at the smallest usable_rows of its own test (its columns A', S' come from
    # hsw_gadget_lookup_permuted, one more call on the same scratch); a cell of argument 4 stored as m + p: refused alone
    product = ProductCase(cfg, hsw, N.HSW_LOOKUP_SPREAD, 256, 3, mont, 7003)
    product.poke("pin", 4, 129, product.peek("pin", 4, 129) + P_INT)
    zs, status, rep = product.run()
    assert status.tolist() == [0, 0, 0, 0, N.HSW_PRODUCT_CELL_NOT_BELOW_P, 0] and zs[4] is None
    assert rep["refused_arguments"] == 1 and rep["first_refused"] == 4 and rep["written"] == 5 * 257
    # ---- the quotient of the smallest circuit of its own test: gates only, 2^4 rows on a coset of 2^6
    QuotientCase(hsw, cfg, mont, 4, 2, 7004, gates=toy_gates(16, 3, 2)).run(launches=2)
    # ---- the first two again, with the first inputs: the same bytes
    ntt_again, status, rep = ntt.run(launches=1)
    assert not status.any() and rep["twiddle_ms"] == 0                        # (the table of the root is still the gadget's)
    assert all(np.array_equal(x, y) for x, y in zip(ntt_first, ntt_again))
    q_again, evals_again, status, _ = opening.open(groups, points, challenges)
    assert not status.any() and np.array_equal(evals_first, evals_again)
    assert all(np.array_equal(x, y) for x, y in zip(q_first, q_again))
    cfg.close()
