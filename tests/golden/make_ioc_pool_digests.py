#!/usr/bin/env python3
"""Digests of the IOC stage's outputs on the cases of tests/ioc_pool_cases.py, for tests/test_gpu_ioc_pool_rows.py.

Run on an MI355X at the commit whose k_ioc is the reference for bit identity (the parent of the change under test: its pooling builds every
operand tile, whatever the neighbour counts):

    python tests/golden/make_ioc_pool_digests.py        # writes tests/golden/ioc_pool_digests.json (or into $IOC_POOL_DIGESTS_DIR)

Per case: the SHA-256 of "Y0" (the positions the IOC stage read), of "Y" and of "score" after one desire_forward, in training mode also of the saved
hidden states "ioc_sv_h"; and, counted on the CPU on those positions, the fewest / most (row, bin) pairs with two or more neighbours of a tile-step
and the most neighbours of one pair.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import ioc_pool_cases as PC  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the digests come from an MI355X"
    out = {}
    for cid in PC.CASES:
        Y, score, Y0, sv_h = PC.run_case(torch, cid)
        lo, hi = PC.multi_pairs(cid, Y0)
        out[cid] = {"rows": int(Y.shape[0]), "Y0_sha256": PC.sha(Y0), "Y_sha256": PC.sha(Y), "score_sha256": PC.sha(score),
                    "slots": PC.slots(cid), "multi_min": int(lo.min()), "multi_max": int(hi.max()), "neighbours_max": int(PC.neighbours(cid, Y0).max())}
        if sv_h is not None:
            out[cid]["sv_h_sha256"], out[cid]["sv_h_max_abs"] = PC.sha(sv_h), float(abs(sv_h).max())
        print("%-24s rows %4d  slots %3d  pairs with two or more neighbours per (tile, step) %s  Y %s  score %s" % (
            cid, out[cid]["rows"], out[cid]["slots"], lo.tolist(), out[cid]["Y_sha256"][:16], out[cid]["score_sha256"][:16]), flush=True)
    path = os.path.join(os.environ.get("IOC_POOL_DIGESTS_DIR", HERE), "ioc_pool_digests.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
