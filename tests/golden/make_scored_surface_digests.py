#!/usr/bin/env python3
"""Digests of what every public scored-sample method of DESIREModel hands back on the planted case of tests/scored_surface_cases.py, and how often
each _lib.Handle method ran per call, for tests/test_gpu_scored_surface.py.

Run on an MI355X at the commit whose host surface is the reference (the parent of the change under test):

    python tests/golden/make_scored_surface_digests.py        # writes tests/golden/scored_surface_digests.json (or into $SCORED_SURFACE_DIGESTS_DIR)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import pytest  # noqa: E402
import torch  # noqa: E402

from tests import scored_surface_cases as SC  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the digests come from an MI355X"
    with pytest.MonkeyPatch.context() as mp:
        res = SC.run(torch, mp)
    out = SC.digest(res)
    for name, r in out.items():
        print("%-30s %s  %s" % (name, " ".join("%s x%d" % kv for kv in r["handle_calls"].items()),
                                " ".join("%s %s" % (k, v["sha256"][:8]) for k, v in r["arrays"].items())), flush=True)
    path = os.path.join(os.environ.get("SCORED_SURFACE_DIGESTS_DIR", HERE), "scored_surface_digests.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)
    SC.check_paths(res)
    print("paths ok")


if __name__ == "__main__":
    main()
