#!/usr/bin/env python3
"""Digests of the inputs and outputs of k_deconv3 and k_decoder on the cases of tests/gen_chain_cases.py, for tests/test_gpu_gen_chain_bits.py.

Run on an MI355X at the commit whose kernels are the reference for bit identity (the parent of the change under test):

    python tests/golden/make_gen_chain_digests.py        # writes tests/golden/gen_chain_digests.json (or into $GEN_CHAIN_DIGESTS_DIR)

Per case: the SHA-256 of every buffer tests/gen_chain_cases.py reads ("d2", "xz", "HxHy": what the two kernels read; "d3", "Y0" or "dec_states", the
training-mode saves and the flat gradient: what they and the stages behind them wrote) and, for the deconv3 cases, that commit's max|d3 - float64
stage reference| on the rows held to the reference, its tolerance under tests/stage_reference.py, and max|d3|.  The training step runs twice: its
gradient is only worth pinning if the same build gives the same bits twice.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import gen_chain_cases as GC  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the digests come from an MI355X"
    out = {}
    for cid in GC.CASES:
        run = GC.run_case(torch, cid)
        out[cid] = dict(GC.digests(run), rows=int(run[2]["d3"].shape[0]))
        if cid == "train_step":
            again = GC.digests(GC.run_case(torch, cid))
            assert again == GC.digests(run), "the training step is not reproducible on one build: %s" % sorted(k for k in again if again[k] != out[cid][k])
        if cid in GC.D3_CASES:
            err, tol, top = GC.reference_error(run, check=False)
            out[cid].update(max_err_vs_float64=err, tolerance=tol, max_abs_d3=top)
            print("%-10s rows %5d  err %.3e  tol %.3e  max|d3| %.3e" % (cid, out[cid]["rows"], err, tol, top), flush=True)
        print("%-10s %s" % (cid, " ".join("%s %s" % (k[:-7], v[:12]) for k, v in sorted(out[cid].items()) if k.endswith("_sha256"))), flush=True)
    path = os.path.join(os.environ.get("GEN_CHAIN_DIGESTS_DIR", HERE), "gen_chain_digests.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
