"""desire_amd.evaluate's walk pinned on the CPU: with the stub model and the videos of tests/evaluate_walk_cases.py, what main() would print is
byte for byte the stored text, and the model is called with exactly the stored arguments (in any order), for no optional flag, every optional flag
at once, --occupancy_mode at, and --modes with seeds by score.  tests/golden/evaluate_walk.json was written by
tests/golden/make_evaluate_walk_golden.py from the single-function evaluate() that preceded the report blocks."""
import json
import os

import pytest

from tests import evaluate_walk_cases as WC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluate_walk.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_videos_tell_the_masks_apart(golden):
    res = json.loads(golden["every_flag"]["text"])
    assert len(set(res["agents"])) > 1                                     # a horizon's own agent count: a swapped mask would show
    assert res["occupancy"]["agents_at_frame"] != res["agents"]            # counted at the horizon's frame is not counted before it
    assert res["windows"] == 7 and json.loads(golden["plain"]["text"])["windows"] == 8
    assert sorted({json.loads(c)[1] for c in golden["plain"]["calls"]}) == [0, 3, 6]       # batches of 3, 3 and a short last one


@pytest.mark.parametrize("tag", list(WC.CASES))
def test_the_walk_prints_the_stored_text_and_makes_the_stored_calls(golden, tag):
    text, calls = WC.walk(WC.CASES[tag])
    assert text == golden[tag]["text"]
    assert calls == golden[tag]["calls"]
