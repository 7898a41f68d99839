"""k_deconv3 with a chain's weight fragments requested a chain ahead and k_decoder on the unrolled chain of k_ioc (desire_amd/csrc/kernels_conv.hip,
kernels_rnn.hip): bits against the kernels before the change, and d3 against the float64 reference of the stage, where a tile is partly empty, where a workgroup runs a second
tile, and on one case per instantiation of the decoder (tests/gen_chain_cases.py).

tests/golden/gen_chain_digests.json was written by tests/golden/make_gen_chain_digests.py on the commit before the change.  Every accumulator
receives the same products in the same order and every store writes the same value, so bit identity is the requirement: no tolerance."""
import json
import os

import numpy as np
import pytest

from tests import gen_chain_cases as GC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_chain_digests.json")) as _fh:
    GOLD = json.load(_fh)
_RUNS = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def run(torch, cid):
    if cid not in _RUNS:
        _RUNS[cid] = GC.run_case(torch, cid)
    return _RUNS[cid]


def test_the_digests_cover_the_cases():
    assert sorted(GOLD) == sorted(GC.CASES)


@pytest.mark.parametrize("cid", GC.D3_CASES)
def test_d3_against_the_float64_stage_reference(torch_cuda, cid):
    r = run(torch_cuda, cid)
    assert r[2]["d3"].shape[0] == GOLD[cid]["rows"] and np.isfinite(r[2]["d3"]).all()
    err, tol, top = GC.reference_error(r, check=False)
    print("%-6s max|d3 - float64| = %.3e (before the change: %.3e), bound %.3e, max|d3| = %.3e" % (cid, err, GOLD[cid]["max_err_vs_float64"], tol, top))
    assert top > 0.1, "d3 is (nearly) all zeros: the case checks nothing"
    GC.reference_error(r)                                                   # stage_reference.check_stage: the parity test's own bound


@pytest.mark.parametrize("cid", GC.CASES)
def test_outputs_bit_identical_to_the_kernels_before(torch_cuda, cid):
    buf = run(torch_cuda, cid)[2]
    got = GC.digests(run(torch_cuda, cid))
    assert sorted(got) == sorted(k for k in GOLD[cid] if k.endswith("_sha256"))
    for name in GC.INPUTS:
        assert got[name + "_sha256"] == GOLD[cid][name + "_sha256"], (
            "%s: an INPUT of the changed kernels (%s) differs from the one the digests were taken on -- the stages before them or the case's "
            "inputs moved; this says nothing about k_deconv3 or k_decoder" % (cid, name))
    assert np.abs(buf["d3"]).max() > 0.1, "d3 is (nearly) all zeros: the case checks nothing"
    out = "dec_states" if cid == "ref_compat" else "Y0"
    assert np.isfinite(buf[out]).all() and np.abs(buf[out]).max() > 0.01, "%s is (nearly) all zeros: the case checks nothing" % out
    assert np.abs(np.diff(buf[out], axis=1)).max() > 0, "the decoder's steps all gave the same output: the case checks nothing"
    for name in ("d3", out):
        assert got[name + "_sha256"] == GOLD[cid][name + "_sha256"], "%s: %s is not bit-identical to the kernel before the change (on bit-identical inputs)" % (cid, name)
    assert all((s in buf) == (cid in GC.TRAIN or cid == "train_step") for s in GC.SAVES) and ("grad" in buf) == (cid == "train_step")
    for name in GC.SAVES:
        if name in buf:                                                     # training mode: what the decoder keeps for the backward pass
            assert np.isfinite(buf[name]).all() and np.abs(buf[name][:, -1]).max() > 0.01, "no saves in %s: the case checks nothing" % name
            assert got[name + "_sha256"] == GOLD[cid][name + "_sha256"], "%s: %s is not bit-identical to the kernel before the change" % (cid, name)
    if "grad" in buf:
        assert np.isfinite(buf["grad"]).all() and np.abs(buf["grad"]).max() > 0
        assert got["grad_sha256"] == GOLD[cid]["grad_sha256"], "%s: the flat gradient is not bit-identical to the build before the change" % cid
