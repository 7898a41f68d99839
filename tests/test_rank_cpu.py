"""Ranking by IOC score, the parts that need no GPU: the two exports, the defaults of the protocol, the command-line flags, and the
numpy statement of the contract (tests/rank_reference.py) against the oracle's independent ADE / FDE."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import make_case, small_dims, to_oracle_layout
from tests.rank_reference import planted_scores, rank_order, ranked_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("desire_rank_samples", "desire_ranked_errors")


def test_the_two_calls_are_declared_exported_and_refuse_a_null_handle():
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "desire_hip.h")).read()
    declared = set(re.findall(r"^int (desire_\w+)\(", hdr, re.M))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    hz = (ctypes.c_int32 * 1)(1)
    assert lib.desire_rank_samples(None, None, None, 1, None, None, None, None) == -1          # DESIRE_ERR_ARG
    assert b"handle" in lib.desire_last_error()
    assert lib.desire_ranked_errors(None, None, None, None, 1, hz, 1, ctypes.c_float(1), ctypes.c_float(1), None, None) == -1
    assert b"handle" in lib.desire_last_error()
    assert hasattr(_lib.Handle, "rank_samples") and hasattr(_lib.Handle, "ranked_errors")


def test_default_top_and_horizons():
    from desire_amd.model import default_horizons, default_top
    assert [default_top(K) for K in (1, 9, 10, 20, 50)] == [1, 1, 1, 2, 5]
    assert [default_horizons(T) for T in (1, 3, 12, 40)] == [[1], [1, 2, 3], [3, 6, 9, 12], [10, 20, 30, 40]]


def test_command_line_flags():
    from desire_amd import evaluate as E
    from desire_amd import train as T
    a = T.build_parser().parse_args([])
    assert a.report_ranked is False and a.eval_top is None and a.eval_horizons is None and a.report_ade is False
    a = T.build_parser().parse_args(["--report_ranked", "--eval_top", "3", "--eval_horizons", "3,6,9,12"])
    assert a.report_ranked and a.eval_top == 3 and T.parse_horizons(a.eval_horizons, 12) == [3, 6, 9, 12]
    assert T.parse_horizons(None, 12) == [3, 6, 9, 12]
    for bad in ("6,3", "0,2", "3,13", "1,2,3,4,5,6,7,8,9"):
        with pytest.raises(ValueError):
            T.parse_horizons(bad, 12)
    e = E.build_parser().parse_args(["--checkpoint", "c.npz", "--units", "0.2", "--max_windows", "7", "--out", "r.json"])
    assert (e.checkpoint, e.units, e.max_windows, e.out, e.num_samples) == ("c.npz", "0.2", 7, "r.json", 20)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")      # no GPU in the child
    p = subprocess.run([sys.executable, "-m", "desire_amd.evaluate", "--help"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "--checkpoint" in p.stdout and "--eval_horizons" in p.stdout, p.stderr[-2000:]


def _case():
    """3 windows x 8 slots, K = 7, T_pred = 12, sx != sy; objects leaving early / never in the target / with gaps."""
    d = small_dims(n_scenes=3, mno=8, K=7, T_obs=4, T_pred=12, n_grids=1, H=64)
    _, fut, _, _, _ = make_case(d, seed=3, n_absent=2)
    fut = fut.copy()
    fut[0, 3:, 1] = 0; fut[0, 1:, 4] = 0; fut[0, :, 3] = 0; fut[1, 2:5, 2] = 0; fut[2, :2, 0] = 0; fut[1, d.T_pred - 1:, 0] = 0
    rng = np.random.default_rng(4)
    Y = (rng.uniform(0.1, 0.9, (d.R, d.T_pred, 2))).astype(np.float32)
    return d, Y, fut, planted_scores(d, 5)


def test_reference_order_rules():
    d, _, _, s = _case()
    o = rank_order(s, d)
    assert o.dtype == np.int32 and o.shape == (d.A, d.K)
    assert (np.sort(o, 1) == np.arange(d.K)).all()
    ident = np.arange(d.K)
    a_last = (d.n_scenes - 1) * d.mno
    for a in (1, 3, a_last, a_last + 2):                          # tied / all-zero / all-zero / all-NaN agents
        np.testing.assert_array_equal(o[a], ident)
    assert list(o[0]).index(0) + 1 == list(o[0]).index(2)         # the planted tie: k = 0 right before k = 2
    assert o[4, 0] == 1 and o[4, -1] == 0 and o[4, -2] == d.K - 1  # +inf first, -inf before the NaN
    np.testing.assert_array_equal(o[5, :3], [0, 1, 2])            # -0, +0, -0 tie
    np.testing.assert_array_equal(o[6, -4:], [0, 2, 4, 6])        # NaNs last, among themselves by k
    assert o[a_last + d.mno - 1, -1] == 0                         # the NaN at k = 0


def test_reference_errors_against_the_oracle():
    from oracle import desire_oracle as O
    d, Y, fut, s = _case()
    o = rank_order(s, d)
    fo = to_oracle_layout(fut)
    want = O.ade_fde_k(Y, O.normalise(fo, d), d, present=fo[:, :, 0] != 0)
    got = ranked_errors(Y, fut, o, d.K, [d.T_pred], 1.0, 1.0, d)
    np.testing.assert_allclose(got[:, 0, 2:], want[:, 2:], atol=1e-6)
    absent = ~(fut[..., 0] != 0).any(1).reshape(-1)
    assert absent.any() and not got[absent].any()
    hz = [1, 3, 6, 9, 12]
    prev = None
    for n_top in range(1, d.K + 1):                               # best-of-top-n never gets worse with n
        r = ranked_errors(Y, fut, o, n_top, hz, 1400.0, 1100.0, d)
        if prev is not None:
            assert (r[..., 2:] <= prev[..., 2:]).all()
        np.testing.assert_array_equal(r[..., :2], ranked_errors(Y, fut, o, 1, hz, 1400.0, 1100.0, d)[..., 2:])
        prev = r
    np.testing.assert_array_equal(prev[:, 0, 0], prev[:, 0, 1])   # h = 1: ADE = FDE
