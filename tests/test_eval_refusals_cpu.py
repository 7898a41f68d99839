"""The order in which the 13 evaluation entry points refuse their arguments, as far as it needs no handle (tests/eval_refusal_cases.py), against
what the parent commit's library answered (tests/golden/eval_refusals.json).  The rest of each sequence needs a device:
tests/test_gpu_eval_refusals.py."""
import json

from tests.eval_refusal_cases import GOLDEN, OPS, Buffers, compare, run


def test_the_checks_that_need_no_handle_come_in_the_recorded_order():
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    want = json.load(open(GOLDEN))
    assert sorted(want["cpu"]) == sorted(OPS) and len(want["recorded_from"]) == 40
    bufs = Buffers()
    diff = compare(run(_lib.load(), bufs, [None]), want["cpu"])
    print("\n".join(diff))
    assert not diff
    assert bufs.untouched()
    # the recorded halves agree: without a handle the peeling is the full one up to its "null handle"
    for fn, rec in want["cpu"].items():
        n = len(rec["peel"])
        assert [s[:2] for s in want["gpu"][fn]["peel"][:n]] == [s[:2] for s in rec["peel"]] and rec["peel"][-1][1] == "null handle", fn
