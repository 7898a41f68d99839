"""k_ioc's dense pooling with the operand rows read in place (desire_amd/csrc/kernels_rnn.hip: pool_rows): bits against the kernel that built every
pooled operand tile in LDS, on one case per regime of the row sources (tests/ioc_pool_cases.py).

tests/golden/ioc_pool_digests.json was written by tests/golden/make_ioc_pool_digests.py on the commit before the change.  A row with one neighbour
is that neighbour's h row (h + 0 = h), a row with more is the same sum in the same order, every MFMA runs on the same operand values in the same
order: bit identity is the requirement, no tolerance.  Each case's regime is counted on the CPU from the positions the IOC stage ran on."""
import json
import os

import numpy as np
import pytest

from tests import ioc_pool_cases as PC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ioc_pool_digests.json")) as _fh:
    GOLD = json.load(_fh)
_RUNS = {}
OVER = ("crowd_over", "crowd_over_mno16", "crowd_over_mno64", "crowd_over_train_dense", "crowd_over_pad")
ALTERNATING = ("crowd_over", "crowd_over_mno16", "crowd_over_mno64", "crowd_over_train_dense")     # ... within the steps of ONE tile


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def run(torch, cid):
    if cid not in _RUNS:
        _RUNS[cid] = PC.run_case(torch, cid)
    return _RUNS[cid]


def test_the_digests_cover_the_cases():
    assert sorted(GOLD) == sorted(PC.CASES)
    assert {c: GOLD[c]["slots"] for c in GOLD} == {c: PC.slots(c) for c in PC.CASES}, "the regimes were chosen for another slot count"


@pytest.mark.parametrize("cid", list(PC.CASES))
def test_ioc_outputs_bit_identical_to_the_built_operands(torch_cuda, cid):
    Y, score, Y0, sv_h = run(torch_cuda, cid)
    assert Y.shape[0] == GOLD[cid]["rows"] and np.isfinite(Y).all() and np.isfinite(score).all()
    assert np.abs(Y - Y0).max() > 0 and np.abs(score).max() > 0, "the IOC stage left no trace: the case checks nothing"
    assert PC.sha(Y0) == GOLD[cid]["Y0_sha256"], ("%s: the INPUT of the IOC stage (Y0) differs from the one the digests were taken on -- sample "
                                                  "generation or the case's inputs moved; this says nothing about k_ioc" % cid)
    assert PC.sha(Y) == GOLD[cid]["Y_sha256"], "%s: Y is not bit-identical to the kernel before the change (on a bit-identical Y0)" % cid
    assert PC.sha(score) == GOLD[cid]["score_sha256"], "%s: score is not bit-identical to the kernel before the change" % cid
    assert (sv_h is not None) == PC.CASES[cid][2] == ("sv_h_sha256" in GOLD[cid])
    if sv_h is not None:                                                    # training mode: the hidden states saved for the backward pass
        assert np.isfinite(sv_h).all() and np.abs(sv_h).max() > 0.01 and np.abs(sv_h[:, -1]).max() > 0.01, "no saves: the case checks nothing"
        assert PC.sha(sv_h) == GOLD[cid]["sv_h_sha256"], "%s: ioc_sv_h is not bit-identical to the kernel before the change" % cid


@pytest.mark.parametrize("cid", list(PC.CASES))
def test_the_case_lies_in_the_regime_it_is_there_for(torch_cuda, cid):
    """Pairs = (row, bin) pairs with two or more neighbours per (tile, step), the kernel's slot counter; slots = spec.ioc_pool_slots of the case's tile."""
    Y0 = run(torch_cuda, cid)[2]
    n, (lo, hi), slots = PC.neighbours(cid, Y0), PC.multi_pairs(cid, Y0), PC.slots(cid)
    print(cid, "slots", slots, "pairs per (tile, step)", lo.tolist(), "most neighbours of a pair", int(n.max()))
    assert (int(lo.min()), int(hi.max()), int(n.max())) == (GOLD[cid]["multi_min"], GOLD[cid]["multi_max"], GOLD[cid]["neighbours_max"])
    if cid == "single":
        assert n.max() == 1 and hi.max() == 0 and (n == 1).sum((2, 3)).max(1).min() > 0, "every tile has populated pairs, none with a second neighbour"
    elif cid == "bench":
        assert n.max() >= 2 and 0 < lo.min() and hi.max() <= slots
    elif cid == "crowd_fit":
        assert 2 * lo.max() >= slots and hi.max() <= slots
    elif cid == "one_cell":
        d = PC.dims(cid)
        pos = Y0.reshape(d.n_scenes * d.K, d.mno, d.T_pred, 2)
        extent = (pos.max(1) - pos.min(1)).max((0, 1))                     # per axis, the widest group-step
        assert extent[0] < d.nb_w / d.grid_size and extent[1] < d.nb_h / d.grid_size, "all agents of a group inside one bin cell"
        assert n.max() == d.mno - 1 == 31 and hi.max() <= slots, "a sum of 31 rows, in a slot"
    else:
        assert cid in OVER
        assert (lo > slots).any() and (hi <= slots).any(), "tile-steps on the build loop and tile-steps on the new loop in one launch"
        if cid in ALTERNATING:
            both = ((lo > slots).any(1) & (hi <= slots).any(1))
            assert both.any(), "one tile takes both paths within its steps: they alternate on one carried state"
