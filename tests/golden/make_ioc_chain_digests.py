#!/usr/bin/env python3
"""Digests of the IOC stage's outputs on the cases of tests/ioc_chain_cases.py, for tests/test_gpu_ioc_chain_bits.py.

Run on an MI355X at the commit whose k_ioc is the reference for bit identity (the parent of the change under test):

    python tests/golden/make_ioc_chain_digests.py        # writes tests/golden/ioc_chain_digests.json (or into $IOC_CHAIN_DIGESTS_DIR)

Per case: the SHA-256 of "Y0" (the positions the IOC stage read), of "Y" and of "score" after one desire_forward, in training mode also of the saved
hidden states "ioc_sv_h", and the fewest / most populated social bins of a ((scene, k) group, step) on those positions.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import ioc_chain_cases as IC  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the digests come from an MI355X"
    out = {}
    for cid in IC.CASES:
        Y, score, Y0, sv_h = IC.run_case(torch, cid)
        occ = IC.occupancy(cid, Y0)
        out[cid] = {"rows": int(Y.shape[0]), "Y0_sha256": IC.sha(Y0), "Y_sha256": IC.sha(Y), "score_sha256": IC.sha(score),
                    "bins_min": int(occ.min()), "bins_max": int(occ.max())}
        if sv_h is not None:
            out[cid]["sv_h_sha256"], out[cid]["sv_h_max_abs"] = IC.sha(sv_h), float(abs(sv_h).max())
        print("%-12s rows %4d  bins per group and step %2d .. %2d  Y %s  score %s" % (cid, out[cid]["rows"], occ.min(), occ.max(),
                                                                                     out[cid]["Y_sha256"][:16], out[cid]["score_sha256"][:16]), flush=True)
    path = os.path.join(os.environ.get("IOC_CHAIN_DIGESTS_DIR", HERE), "ioc_chain_digests.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
