"""k_deconv2 with the output tile accumulated in registers (desire_amd/csrc/kernels_conv.hip): bits against the LDS-scatter kernel it replaced, and
the float64 reference of the stage, where a pair or a tile is partly empty and where a workgroup runs a second tile (tests/deconv2_cases.py).

tests/golden/deconv2_digests.json was written by tests/golden/make_deconv2_digests.py on the commit before the change.  Every output element is
the same sum 0 + G_tap0 + G_tap1 + .. in ascending tap order of the same 64-MFMA chains, so bit identity is the requirement: no tolerance."""
import json
import os

import numpy as np
import pytest

from tests import deconv2_cases as DC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deconv2_digests.json")) as _fh:
    GOLD = json.load(_fh)
_RUNS = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def run(torch, cid):
    if cid not in _RUNS:
        _RUNS[cid] = DC.run_case(torch, cid)
    return _RUNS[cid]


def test_the_digests_cover_the_cases():
    assert sorted(GOLD) == sorted(DC.CASES)


@pytest.mark.parametrize("cid", DC.CASES)
def test_d2_against_the_float64_stage_reference(torch_cuda, cid):
    r = run(torch_cuda, cid)
    assert r[2].shape[0] == GOLD[cid]["rows"] and np.isfinite(r[3]).all()
    err, tol, top = DC.reference_error(r, check=False)
    print("%-6s max|d2 - float64| = %.3e (before the change: %.3e), bound %.3e, max|d2| = %.3e" % (cid, err, GOLD[cid]["max_err_vs_float64"], tol, top))
    assert top > 0.1, "d2 is (nearly) all zeros: the case checks nothing"
    DC.reference_error(r)                                                   # stage_reference.check_stage: the parity test's own bound


@pytest.mark.parametrize("cid", DC.CASES)
def test_d2_bits_equal_the_scatter_kernels(torch_cuda, cid):
    r = run(torch_cuda, cid)
    assert DC.sha(r[2]) == GOLD[cid]["d1_sha256"], ("%s: the INPUT of deconv2 (d1) differs from the one the digests were taken on -- the stages before "
                                                    "deconv2 or the case's inputs moved; this says nothing about k_deconv2" % cid)
    assert DC.sha(r[3]) == GOLD[cid]["d2_sha256"], "%s: d2 is not bit-identical to the kernel before the change (on a bit-identical d1)" % cid
