"""The numpy statements of the plan-risk contract (tests/plan_reference.py) against each other, against scipy's distances, against the conditions
their generator promises, and its mirror of the kernel's LDS geometry against desire_amd/csrc/eval_lds.h (tests/c_host/plan_lds_driver.cpp,
compiled with g++: no ROCm header, no GPU)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import small_dims
from tests.plan_reference import (KINDS, MARGIN, RADIUS_PX, SHAPES, brute_force_first, equal_joint_scores, make_inputs, plan_centres, plan_f32,
                                  plan_f64, plan_geometry, planted_joint_scores, risk_bound)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "plan_lds_driver.cpp")
IDS = lambda s: "n%d_m%d_K%d_T%d_M%d" % s
_CACHE = {}


def dims(shape):
    n, m, K, T, _ = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64)


def horizons(T):
    return sorted({max(1, T // 4), max(1, T // 2), T})


def case(shape):
    """The shape's inputs in pixel units and both references, computed once and left unchanged."""
    if shape not in _CACHE:
        d = dims(shape)
        M = shape[4]
        ux, uy, radius = 1.0 / d.sx, 1.0 / d.sy, RADIUS_PX
        Y, fut, present, plans, ego, info = make_inputs(d, M, radius, ux, uy, seed=5, centres=plan_centres(d.mno, d.T_pred, M))
        s = planted_joint_scores(d, 9)
        hz = horizons(d.T_pred)
        args = (Y, fut, None, s, plans, ego, hz, radius, ux, uy, d)
        for a in (Y, fut, plans, ego, s):
            a.setflags(write=False)
        _CACHE[shape] = dict(d=d, M=M, args=args, info=info, hz=hz, f64=plan_f64(*args), f32=plan_f32(*args))
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_margin_holds_and_the_two_precisions_agree(shape):
    c = case(shape)
    d, f32, f64 = c["d"], c["f32"], c["f64"]
    assert f64["margin"] > MARGIN                                          # the float64 pass alone, before any comparison
    for key in ("first", "first_slot"):
        np.testing.assert_array_equal(f32[key], f64[key], err_msg=key)
    fin = np.isfinite(f64["clear"])
    assert (fin == np.isfinite(f32["clear"])).all()
    np.testing.assert_allclose(f32["clear"][fin], f64["clear"][fin], rtol=8 * 2.0 ** -24, atol=0)
    for key in ("risk", "blame"):
        assert float(np.abs(f32[key].astype(np.float64) - f64[key]).max()) <= risk_bound(d), key
    np.testing.assert_array_equal(f32["jscore"].astype(np.float64), f64["jscore"])      # the grid of 1/64: exact sums
    np.testing.assert_allclose(f64["W"].sum(-1), 1.0, rtol=1e-12)
    assert (f64["risk"] <= 1 + 1e-12).all() and (f64["blame"] <= f64["risk"][..., None] + 1e-12).all()
    if d.mno > 1:
        assert (f64["first"] < d.T_pred).any() and (f64["first"] == d.T_pred).any()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scipy_agrees_on_first(shape):
    pytest.importorskip("scipy")
    c = case(shape)
    Y, fut, _, _, plans, ego, _, radius, ux, uy, d = c["args"]
    np.testing.assert_array_equal(brute_force_first(Y, fut, plans, ego, radius, ux, uy, d), c["f64"]["first"])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_plan_behaves_as_labelled(shape):
    c = case(shape)
    d, f64, hz = c["d"], c["f64"], c["hz"]
    Y, fut, _, _, plans, ego, _, radius, ux, uy, _ = c["args"]
    T, r2 = d.T_pred, (float(np.float32(radius))) ** 2
    Yk = Y.reshape(d.n_scenes, d.K, d.mno, T, 2)
    checked = set()
    for w, row in enumerate(c["info"]["plans"]):
        for mi, (kind, i, k, cs, checkable) in enumerate(row):
            fs, e = f64["first_slot"][w, mi], int(ego[w, mi])
            assert (f64["blame"][w, mi][:, e] == 0).all() if e >= 0 else True
            if d.mno == 1:
                assert e == 0 and (f64["first"][w, mi] == T).all() and np.isinf(f64["clear"][w, mi]).all() and not f64["risk"][w, mi].any()
                continue
            if kind == "far":
                assert (f64["first"][w, mi] == T).all() and not f64["risk"][w, mi].any() and not f64["blame"][w, mi].any()
                assert (f64["clear"][w, mi] > 100 * r2).all()
                checked.add(kind)
            if not checkable:
                continue
            if kind == "cross":
                assert fs[k, i] == max(cs - 1, 0), (w, mi)
            elif kind == "follow":
                assert fs[k, i] == 0 and f64["clear"][w, mi, k, 0] < r2
            elif kind == "same":
                assert np.array_equal(plans[w, mi].view(np.uint32), Yk[w, k, i].view(np.uint32))
                assert fs[k, i] == 0 and (f64["clear"][w, mi, k] == 0).all()
            elif kind == "ego":
                assert e == i and np.array_equal(plans[w, mi].view(np.uint32), Yk[w, k, i].view(np.uint32))
                assert f64["first"][w, mi, k] == T and (fs[:, i] == T).all() and (f64["clear"][w, mi, k] > r2).all()
                free = plan_f64(*c["args"][:5], None, *c["args"][6:])       # nobody replaced: the same plan sits on the slot
                assert free["first_slot"][w, mi, k, i] == 0
            elif kind == "nan":
                assert np.isnan(plans[w, mi, T // 2:]).all() and np.isfinite(plans[w, mi, :T // 2]).all() and fs[k, i] == T
                assert ((f64["first"][w, mi] < T // 2) | (f64["first"][w, mi] == T)).all()         # no contact from the middle frame on
            elif kind == "gone":
                gone = fut[w, :, i, 0] == 0
                assert gone.any() and not gone.all() and (fs[:, i] == T).all()
                p = (plans[w, mi].astype(np.float64) - Yk[w, k, i]) * np.array([float(np.float32(ux)), float(np.float32(uy))])
                assert ((p ** 2).sum(-1)[gone] < r2).all() and ((p ** 2).sum(-1)[~gone] > r2).all()
            checked.add(kind)
    _CACHE.setdefault("kinds", set()).update(checked)


def test_every_kind_occurs_over_the_shapes():
    for shape in SHAPES:
        test_every_plan_behaves_as_labelled(shape)
    assert _CACHE["kinds"] == set(KINDS)


def test_the_chunked_shape_has_contacts_on_both_sides_of_the_border():
    shape = SHAPES[5]
    c = case(shape)
    d = c["d"]
    pc, tc = plan_geometry(d.mno, d.T_pred, c["M"])
    assert (pc, tc) == (1, 29) and plan_centres(d.mno, d.T_pred, c["M"]) == [7, 28, 29, 34]
    crossed = [f64k for row in c["info"]["plans"] for f64k in row if f64k[0] == "cross" and f64k[4]]
    assert {cs for _, _, _, cs, _ in crossed} >= {7, 28, 29, 34}
    first = c["f64"]["first_slot"][:, :, :d.K]                            # per (plan, slot): what a lane carries across the passes
    assert (first < tc - 2).any() and (first == tc - 1).any() and ((first >= tc) & (first < d.T_pred)).any()


def test_equal_joint_scores_give_equal_weights_and_null_scores_too():
    c = case(SHAPES[0])
    d = c["d"]
    a = list(c["args"])
    a[3] = equal_joint_scores(d, 4)
    eq = plan_f32(*a)
    a[3] = None
    flat = plan_f32(*a)
    assert (eq["W"] == np.float32(1) / np.float32(d.K)).all()
    for key in ("risk", "blame", "first", "clear"):
        np.testing.assert_array_equal(eq[key], flat[key])
    big = case(SHAPES[2])                                                  # K = 20: window 0 holds a NaN and an infinite joint score
    bad = ~np.isfinite(big["f32"]["jscore"]).all(-1)
    assert bad[0] and not bad[1]
    assert (big["f32"]["W"][bad] == np.float32(1) / np.float32(big["d"].K)).all() and len(set(big["f32"]["W"][1].tolist())) > 2
    assert (c["f32"]["jscore"][0, 2] == c["f32"]["jscore"][0, 0]).all() and c["f32"]["W"][0, 2] == c["f32"]["W"][0, 0]      # the tie


def test_present_form_has_no_truth_row():
    c = case(SHAPES[0])
    d = c["d"]
    Y, fut, _, s, plans, ego, hz, radius, ux, uy, _ = c["args"]
    present = (fut[:, 0, :, 0] != 0).reshape(-1).astype(np.uint8)
    res = plan_f32(Y, None, present, s, plans, ego, hz, radius, ux, uy, d)
    assert (res["first"][:, :, d.K] == d.T_pred).all() and np.isinf(res["clear"][:, :, d.K]).all()


# ---- the geometry mirror against the header
MNO = [1, 2, 4, 8, 16, 32, 64, 96, 160, 256]
TS = [1, 5, 7, 28, 29, 30, 40, 200, 3800, 7681]
MS = [1, 3, 5, 9, 31, 32, 33, 64, 70, 257]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("plan_lds") / "plan_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_geometry_mirror_equals_the_header(driver):
    shapes = list(itertools.product(MNO, TS, MS))
    reqs = ["budget"] + ["plan %d %d %d" % s for s in shapes]
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs) and rows[0] == (60 * 1024, 256, 8, 32)
    budget = rows[0][0]
    for (m, T, M), (pc, tc, nbytes, end, nxt) in zip(shapes, rows[1:]):
        assert (pc, tc) == plan_geometry(m, T, M), (m, T, M)
        chunks = -(-M // pc)
        assert 1 <= pc <= 32 and pc * m <= max(m, 256) and (chunks - 1) * pc < M <= chunks * pc, (m, T, M, pc)      # one item per lane, every plan once
        assert 1 <= tc <= T and nbytes == end <= budget, (m, T, M)
        stride = m + 1 if m >= 32 else m
        assert nbytes == 8 * (pc * (tc | 1) + tc * stride) + 72 * pc, (m, T, M)
        assert tc == T or nxt + 8 * pc > budget, (m, T, M)                  # chunked only where one more frame (at the odd stride's worst) does not fit
    assert plan_geometry(32, 40, 64) == (8, 40) and plan_geometry(32, 40, 9) == (5, 40) and plan_geometry(256, 40, 70) == (1, 29)
