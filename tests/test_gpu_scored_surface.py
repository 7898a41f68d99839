"""The scored-sample surface of DESIREModel (desire_amd/scored.py) pinned on one small planted case: every public method once or twice, each
returned array's dtype, shape and bytes, and per call how often each _lib.Handle method ran, against tests/golden/scored_surface_digests.json
(written by tests/golden/make_scored_surface_digests.py on an MI355X before the methods moved out of model.py).  Exact equality: the device calls
are the same ones, the kernels are bitwise reproducible by contract and the torch post-processing is elementwise on fixed shapes; the call counts
say that no launch was added or dropped."""
import json
import os

import pytest

from tests import scored_surface_cases as SC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scored_surface_digests.json")


def test_every_method_returns_the_recorded_bytes_through_the_recorded_calls(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    with open(GOLDEN) as fh:
        want = json.load(fh)
    res = SC.run(torch, monkeypatch)
    SC.check_paths(res)
    got = SC.digest(res)
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name]["keys"] == want[name]["keys"], name
        assert got[name]["handle_calls"] == want[name]["handle_calls"], name
        for key in got[name]["keys"]:
            assert got[name]["arrays"][key] == want[name]["arrays"][key], (name, key)
