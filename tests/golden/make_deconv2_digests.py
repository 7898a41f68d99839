#!/usr/bin/env python3
"""Digests of k_deconv2's input and output on the cases of tests/deconv2_cases.py, for tests/test_gpu_deconv2_regs.py.

Run on an MI355X at the commit whose k_deconv2 is the reference for bit identity (the parent of the change under test):

    python tests/golden/make_deconv2_digests.py        # writes tests/golden/deconv2_digests.json (or into $DECONV2_DIGESTS_DIR)

Per case: the SHA-256 of the live rows of "d1" (what deconv2 read) and of "d2" (what it wrote, through the normalisation pass where dims.bn_mode = 1),
that commit's max|d2 - float64 stage reference| on the rows held to the reference, its tolerance under tests/stage_reference.py, and max|d2|.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import deconv2_cases as DC  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the digests come from an MI355X"
    out = {}
    for cid in DC.CASES:
        run = DC.run_case(torch, cid)
        err, tol, top = DC.reference_error(run, check=False)
        out[cid] = {"rows": int(run[2].shape[0]), "d1_sha256": DC.sha(run[2]), "d2_sha256": DC.sha(run[3]), "max_err_vs_float64": err,
                    "tolerance": tol, "max_abs_d2": top}
        print("%-6s rows %5d  err %.3e  tol %.3e  max|d2| %.3e  d2 %s" % (cid, out[cid]["rows"], err, tol, top, out[cid]["d2_sha256"][:16]), flush=True)
    path = os.path.join(os.environ.get("DECONV2_DIGESTS_DIR", HERE), "deconv2_digests.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
