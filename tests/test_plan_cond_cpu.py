"""The numpy statements of the conditioned plan-risk contract (tests/plan_cond_reference.py) against each other, the coverage conditions their
generator has to meet (asserted on the float64 form alone), the exact anchors of the contract on the statements themselves, and the mirror of the
kernel's LDS geometry against desire_amd/csrc/eval_lds.h (tests/c_host/plan_cond_lds_driver.cpp, compiled with g++: no ROCm header, no GPU)."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.plan_cond_reference import (MARGIN, SHAPES, cond_case, cond_ref, cw_bound, ess_bound, plan_cond_f32, plan_cond_f64, plan_cond_geometry,
                                       planted_identical, planted_nan, planted_one_hot, risk_bound, support_bound)
from tests.plan_reference import plan_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "plan_cond_lds_driver.cpp")
IDS = lambda s: "n%d_m%d_K%d_T%d_M%d" % s
UNITS = pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _args(c, **kw):
    ux, uy, radius = c["unit"]
    a = dict(Y=c["Y"], fut=c["fut"], present=None, score=c["score"], plans=c["plans"], ego=c["ego"], horizons=c["hz"], radius=radius, ux=ux, uy=uy,
             d=c["d"], sigma=2 * radius, t_cond=c["d"].T_pred)
    a.update(kw)
    return a


def test_the_call_is_declared_exported_and_wrapped():
    from desire_amd import _lib
    with open(os.path.join(ROOT, "include", "desire_hip.h")) as fh:
        declared = set(re.findall(r"\b(desire_[a-z0-9_]+)\s*\(", fh.read()))
    assert "desire_plan_risk_cond" in declared and "desire_plan_risk_cond" in _lib.EXPORTS and callable(getattr(_lib.Handle, "plan_risk_cond"))
    from desire_amd import _build
    assert "kernels_plan_cond.hip" in _build.SOURCES


@UNITS
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_generator_meets_the_coverage_conditions(shape, unit):
    """On the float64 form alone, at sigma = 2 radii: the margin of the contact rule; (a) a conditioned plan whose weights are neither one world's
    nor the prior's flat ones; (b) where there is anybody to touch, a conditioned plan whose risk moves against the prior's."""
    c = cond_case(shape, unit)
    d = c["d"]
    f64 = cond_ref(c, plan_cond_f64, 2 * c["unit"][2], d.T_pred)
    assert f64["margin"] > MARGIN
    cond = f64["conditioned"]
    graded = cond & (f64["ess"] > 1.5) & (f64["ess"] < d.K - 0.05)
    moved = cond & (np.abs(f64["risk"] - f64["risk_prior"]).max(-1) > 0.02)
    print("%s unit %d: %d conditioned, %d graded, %d moved" % (IDS(shape), unit, cond.sum(), graded.sum(), moved.sum()))
    assert graded.any()
    if d.mno > 1:
        assert moved.any()


@UNITS
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_two_precisions_agree(shape, unit):
    c = cond_case(shape, unit)
    d = c["d"]
    radius = c["unit"][2]
    for sigma, t_cond in ((2 * radius, d.T_pred), (radius / 2, max(1, d.T_pred // 2))):
        f32, f64 = cond_ref(c, plan_cond_f32, sigma, t_cond), cond_ref(c, plan_cond_f64, sigma, t_cond)
        for key in ("first", "cond", "conditioned", "dist", "logit"):       # C1 - C3 are fp32 in both; first holds under the margin
            np.testing.assert_array_equal(f32[key], f64[key], err_msg=key)
        assert float(np.abs(f32["cw"].astype(np.float64) - f64["cw"]).max()) <= cw_bound(d)
        for key in ("risk", "blame"):
            assert float(np.abs(f32[key].astype(np.float64) - f64[key]).max()) <= risk_bound(d), key
        assert float(np.abs(f32["support"].astype(np.float64) - f64["support"]).max()) <= support_bound(d)
        assert (np.abs(f32["ess"].astype(np.float64) - f64["ess"]) <= ess_bound(d, f64["ess"])).all()
        np.testing.assert_allclose(f64["cw"].sum(-1), 1.0, rtol=1e-12)
        assert (f64["ess"] >= 1 - 1e-9).all() and (f64["ess"] <= d.K + 1e-9).all()
        assert (f64["support"] >= 0).all() and (f64["support"] <= 1 + 1e-12).all()      # (0 where a far plan's kernel underflows)
        assert (f64["cond"] <= t_cond).all() and ((f64["cond"] > 0) == f64["conditioned"]).all()
        assert (f64["blame"] <= f64["risk"][..., None] + 1e-12).all()


def test_without_an_ego_slot_the_call_is_plan_risk():
    c = cond_case(SHAPES[2], 1)
    d = c["d"]
    base = plan_f32(c["Y"], c["fut"], None, c["score"], c["plans"], None, c["hz"], c["unit"][2], c["unit"][0], c["unit"][1], d)
    for ego in (None, np.full_like(c["ego"], -1), np.full_like(c["ego"], d.mno)):
        r = plan_cond_f32(**_args(c, ego=ego))
        for key in ("first", "clear", "risk", "blame"):
            np.testing.assert_array_equal(_bits(r[key]), _bits(base[key]), err_msg=key)
        np.testing.assert_array_equal(_bits(r["cw"]), _bits(np.broadcast_to(base["W"][:, None], r["cw"].shape)))
        assert (r["support"] == 1).all() and (r["dist"] == 0).all() and (r["cond"] == 0).all()


def test_a_sigma_whose_square_overflows_gives_the_prior():
    c = cond_case(SHAPES[2], 1)
    d = c["d"]
    base = plan_f32(c["Y"], c["fut"], None, c["score"], c["plans"], c["ego"], c["hz"], c["unit"][2], c["unit"][0], c["unit"][1], d)
    r = plan_cond_f32(**_args(c, sigma=1e20))
    assert r["inv"] == 0
    fin = np.isfinite(r["dist"]).all(-1)
    assert fin.any() and (r["cond"][fin & (r["n_c"] > 0)] > 0).all()
    np.testing.assert_array_equal(_bits(r["cw"][fin]), _bits(np.broadcast_to(base["W"][:, None], r["cw"].shape)[fin]))
    for key in ("risk", "blame"):
        np.testing.assert_array_equal(_bits(r[key][fin]), _bits(base[key][fin]), err_msg=key)


def test_identical_ego_rows_give_equal_weights():
    c = cond_case(SHAPES[0], 1)
    d = c["d"]
    Y, ego = planted_identical(c)
    r = plan_cond_f32(**_args(c, Y=Y, ego=ego, score=None))
    assert (r["cond"] > 0).any()
    np.testing.assert_array_equal(_bits(r["cw"]), _bits(np.full(r["cw"].shape, np.float32(1) / np.float32(d.K), np.float32)))
    base = plan_f32(Y, c["fut"], None, None, c["plans"], ego, c["hz"], c["unit"][2], c["unit"][0], c["unit"][1], d)
    for key in ("risk", "blame"):
        np.testing.assert_array_equal(_bits(r[key]), _bits(base[key]), err_msg=key)


def test_a_plan_that_is_one_worlds_ego_row_takes_that_world():
    c = cond_case(SHAPES[0], 1)
    d = c["d"]
    plans, ego, k0, sigma, live = planted_one_hot(c)
    r = plan_cond_f32(**_args(c, plans=plans, ego=ego, score=None, sigma=sigma))
    assert np.isfinite(r["inv"]) and (r["cond"][live] == d.T_pred).all() and (r["cond"][~live] == 0).all()
    lk = r["logit"][live]
    for mi in range(c["M"]):
        assert (np.delete(lk[:, mi], k0[mi], axis=-1) < -104).all() and (lk[:, mi, k0[mi]] == 0).all()
    hot = np.zeros(r["cw"].shape, np.float32)
    hot[:, np.arange(c["M"]), k0] = 1
    np.testing.assert_array_equal(_bits(r["cw"][live]), _bits(hot[live]))
    assert (r["ess"][live] == 1).all()
    want = (r["first"][:, np.arange(c["M"]), k0][..., None] < np.asarray(c["hz"])).astype(np.float32)
    np.testing.assert_array_equal(_bits(r["risk"][live]), _bits(want[live]))


def test_a_nan_in_one_worlds_ego_row_leaves_the_plan_with_the_prior():
    c = cond_case(SHAPES[2], 1)
    f64 = cond_ref(c, plan_cond_f64, 2 * c["unit"][2], c["d"].T_pred)
    Y, w, mi, k1 = planted_nan(c, f64)
    r = plan_cond_f32(**_args(c, Y=Y))
    assert f64["cond"][w, mi] > 0 and r["cond"][w, mi] == 0 and np.isnan(r["dist"][w, mi, k1]) and np.isfinite(np.delete(r["dist"][w, mi], k1)).all()
    np.testing.assert_array_equal(_bits(r["cw"][w, mi]), _bits(r["W"][w]))
    assert r["support"][w, mi] == 1
    others = np.ones(r["cond"].shape, bool)
    others[w] = c["ego"][w] != c["ego"][w, mi]
    np.testing.assert_array_equal(r["cond"][others], f64["cond"][others])


# ---- the geometry mirror against the header
KS = [1, 2, 3, 4, 20, 64, 200, 256, 1024, 1300, 8191]
TS = [1, 5, 7, 20, 40, 100, 200, 3800, 7681]
MS = [1, 3, 5, 9, 51, 64, 65, 70, 257]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("plan_cond_lds") / "plan_cond_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_geometry_mirror_equals_the_header(driver):
    shapes = list(itertools.product(KS, TS, MS))
    reqs = ["budget"] + ["cond %d %d %d" % s for s in shapes]
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs) and rows[0] == (60 * 1024, 256, 64, 1024)
    budget = rows[0][0]
    staged = passes = 0
    for (K, T, M), (pc, tc, rows_in, nbytes, end, nxt) in zip(shapes, rows[1:]):
        assert (pc, tc, rows_in) == plan_cond_geometry(K, T, M), (K, T, M)
        chunks = -(-M // pc)
        assert 1 <= pc <= 64 and pc * K <= max(K, 1024) and (chunks - 1) * pc < M <= chunks * pc, (K, T, M, pc)
        assert 1 <= tc <= T and nbytes == end <= budget, (K, T, M)
        assert nbytes == 8 * (pc + (K if rows_in else 0)) * (tc | 1) + 8 * pc, (K, T, M)
        assert not rows_in or tc == T                                      # the ego rows are staged whole or not at all
        assert tc == T or nxt + 8 * pc > budget, (K, T, M)                  # passes only where one more frame (at the odd stride's worst) does not fit
        staged += rows_in
        passes += tc < T
    assert staged > 0 and passes > 0 and staged < len(shapes)
    assert plan_cond_geometry(20, 40, 64) == (32, 40, 1) and plan_cond_geometry(20, 40, 9) == (9, 40, 1) and plan_cond_geometry(2, 40, 70) == (35, 40, 1)
