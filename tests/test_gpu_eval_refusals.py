"""The whole refusal sequence of the 13 evaluation entry points on a live handle (tests/eval_refusal_cases.py: NULL handle, then a ref_compat
handle, then the live one of (n_scenes, mno, K, T_pred) = (1, 4, 3, 6) without weights) against what the parent commit's library answered
(tests/golden/eval_refusals.json).  Every call is refused and leaves its outputs untouched; the one kernel that runs is the legal desire_plan_risk
call at the end."""
import json

import pytest

from tests.eval_refusal_cases import GOLDEN, HZ, Buffers, compare, live_handles, run

pytestmark = pytest.mark.gpu


def test_every_check_comes_in_the_recorded_order_and_nothing_is_written():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from desire_amd import _lib
    want = json.load(open(GOLDEN))
    bufs = Buffers(torch)
    h, rc = live_handles(_lib)
    diff = compare(run(_lib.load(), bufs, [None, rc._h, h._h]), want["gpu"])
    print("\n".join(diff))
    assert not diff
    assert bufs.untouched()
    # ... and the handle still works
    z, M = bufs.ins["Z"], 2
    risk = torch.full((M * len(HZ),), bufs.FILL, device="cuda")
    h.plan_risk(z, z, 0, 0, z, 0, M, list(HZ), 0.0, 1.0, 1.0, risk.data_ptr())
    torch.cuda.synchronize()
    assert bool((risk == 0).all())
    assert bufs.untouched()
    h.close(); rc.close()
