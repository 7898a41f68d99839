"""k_ioc's dense pooling chain unrolled over two statically named fragment sets (desire_amd/csrc/kernels_rnn.hip: ioc_bin_chain): bits against
the rolled mma_begin / mma_run chain it replaced, on one case per kind of instantiation of the branch (tests/ioc_chain_cases.py).

tests/golden/ioc_chain_digests.json was written by tests/golden/make_ioc_chain_digests.py on the commit before the change.  Every output is the
same chain of products in the same order, so bit identity is the requirement: no tolerance."""
import json
import os

import numpy as np
import pytest

from tests import ioc_chain_cases as IC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ioc_chain_digests.json")) as _fh:
    GOLD = json.load(_fh)
_RUNS = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def run(torch, cid):
    if cid not in _RUNS:
        _RUNS[cid] = IC.run_case(torch, cid)
    return _RUNS[cid]


def test_the_digests_cover_the_cases():
    assert sorted(GOLD) == sorted(IC.CASES)


@pytest.mark.parametrize("cid", list(IC.CASES))
def test_ioc_outputs_bit_identical_to_the_rolled_chain(torch_cuda, cid):
    Y, score, Y0, sv_h = run(torch_cuda, cid)
    assert Y.shape[0] == GOLD[cid]["rows"] and np.isfinite(Y).all() and np.isfinite(score).all()
    assert np.abs(Y - Y0).max() > 0 and np.abs(score).max() > 0, "the IOC stage left no trace: the case checks nothing"
    assert IC.sha(Y0) == GOLD[cid]["Y0_sha256"], ("%s: the INPUT of the IOC stage (Y0) differs from the one the digests were taken on -- sample "
                                                  "generation or the case's inputs moved; this says nothing about k_ioc" % cid)
    assert IC.sha(Y) == GOLD[cid]["Y_sha256"], "%s: Y is not bit-identical to the kernel before the change (on a bit-identical Y0)" % cid
    assert IC.sha(score) == GOLD[cid]["score_sha256"], "%s: score is not bit-identical to the kernel before the change" % cid
    assert (sv_h is not None) == IC.CASES[cid][2] == ("sv_h_sha256" in GOLD[cid])
    if sv_h is not None:                                                    # training mode: the hidden states saved for the backward pass
        assert np.isfinite(sv_h).all() and np.abs(sv_h).max() > 0.01 and np.abs(sv_h[:, -1]).max() > 0.01, "no saves: the case checks nothing"
        assert IC.sha(sv_h) == GOLD[cid]["sv_h_sha256"], "%s: ioc_sv_h is not bit-identical to the kernel before the change" % cid


def test_the_cases_hold_the_occupancies_they_are_there_for(torch_cuda):
    """full_plain: steps with every bin populated; sparse: tiles with no populated bin and tiles with a few, not adjacent; sparse5: tiles with exactly
    one populated bin (nothing to prefetch behind it) and tiles with none; grid6: bins beyond the 32nd, the upper half of the occupancy word."""
    full = IC.occupancy("full_plain", run(torch_cuda, "full_plain")[2])
    assert full.max() == 16, full
    sp, sp5 = (IC.occupancy(c, run(torch_cuda, c)[2]) for c in ("sparse", "sparse5"))
    print("populated bins per (tile, step): sparse", sp.tolist(), "sparse5", sp5.tolist())
    assert (sp == 0).any() and ((sp >= 2) & (sp < 16)).any(), sp
    assert (sp5 == 0).any() and (sp5 == 1).any(), sp5
    g6 = IC.occupied("grid6", run(torch_cuda, "grid6")[2])
    assert g6[..., 32:].any() and g6[..., :32].any(), g6.sum((0, 1))
    for cid in ("full_plain", "sparse", "sparse5", "grid6"):
        occ = IC.occupancy(cid, run(torch_cuda, cid)[2])
        assert (int(occ.min()), int(occ.max())) == (GOLD[cid]["bins_min"], GOLD[cid]["bins_max"])
