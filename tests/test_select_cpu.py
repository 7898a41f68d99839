"""The selection contract without a GPU (tests/select_reference.py): the fp32 restatement against the float64 pass on the generator's inputs, the
greedy pass against a plain-Python one, the limiting cases, the margin condition of every shape the GPU test uses, and the argument checks of
desire_select_diverse that the loaded library makes before it needs a handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.helpers import small_dims
from tests.rank_reference import planted_scores, rank_order
from tests.select_reference import (DIST_FINAL, DIST_MAX, DIST_MEAN, MARGIN, METRICS, brute_force, cases_of, make_inputs, margin_of_values, near_matrix, pair_values,
                                    select_f32, select_f64, weights)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n_scenes, mno, K, T_pred) of tests/test_gpu_select.py
GPU_SHAPES = [(2, 8, 5, 12), (2, 8, 3, 7), (3, 1, 3, 7), (2, 4, 1, 5), (3, 32, 20, 40), (2, 160, 130, 9), (2, 32, 3, 200)]
RADIUS_PX = 20.0


def dims_of(shape):
    n, m, K, T = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64)


def units_of(d):
    return [(1.0, 1.0, float(np.float32(RADIUS_PX * d.sx))), (1.0 / d.sx, 1.0 / d.sy, RADIUS_PX)]      # (unit_x, unit_y, radius in that unit)


SMALL = [s for s in GPU_SHAPES if s[1] * s[2] * s[2] <= 20000]


def test_the_call_is_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    from desire_amd.model import DESIREModel
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "desire_hip.h")).read()
    assert "desire_select_diverse" in set(re.findall(r"\b(desire_[a-z_]+)\s*\(", hdr))
    assert "desire_select_diverse" in _lib.EXPORTS and hasattr(lib, "desire_select_diverse") and hasattr(_lib.Handle, "select_diverse")
    assert (_lib.DIST_FINAL, _lib.DIST_MEAN, _lib.DIST_MAX) == (DIST_FINAL, DIST_MEAN, DIST_MAX) == (0, 1, 2)
    for name, v in (("DESIRE_DIST_FINAL", 0), ("DESIRE_DIST_MEAN", 1), ("DESIRE_DIST_MAX", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, v), hdr)
    import inspect
    for fn in (DESIREModel.predict, DESIREModel.predict_device, DESIREModel.evaluate_ranked):
        p = inspect.signature(fn).parameters
        assert p["select"].default == "score" and p["nms_radius"].default is None and p["nms_metric"].default == "final" and p["nms_horizon"].default is None


def test_bad_arguments_are_refused_before_a_handle_is_needed():
    """Every check that depends on the arguments alone returns DESIRE_ERR_ARG (-1) with its text; a NULL handle is refused after them.  The checks
    against the handle's dims (t_end > T_pred, n_top > K, the LDS plan) need a device: tests/test_gpu_select.py."""
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    nan, inf = float("nan"), float("inf")
    good = dict(h=None, Y=p, order=p, score=p, metric=0, t_end=1, radius=1.0, ux=1.0, uy=1.0, n_top=1, out=p, count=p, mass=p, top_Y=p, top_score=p)
    cases = [(dict(metric=-1), b"metric"), (dict(metric=3), b"metric"), (dict(t_end=0), b"t_end"), (dict(t_end=-5), b"t_end"),
             (dict(n_top=0), b"n_top"), (dict(radius=-1.0), b"radius"), (dict(radius=nan), b"radius"), (dict(radius=inf), b"radius"),
             (dict(ux=0.0), b"unit_x"), (dict(ux=-1.0), b"unit_x"), (dict(ux=nan), b"unit_x"), (dict(ux=inf), b"unit_x"),
             (dict(uy=0.0), b"unit_y"), (dict(uy=-2.0), b"unit_y"), (dict(uy=nan), b"unit_y"), (dict(uy=inf), b"unit_y"),
             (dict(Y=None), b"dev_Yhat"), (dict(order=None), b"dev_order"), (dict(out=None), b"dev_order_out"), (dict(count=None), b"dev_count"),
             (dict(score=None), b"dev_score"), ({}, b"handle")]
    for kw, word in cases:
        a = dict(good); a.update(kw)
        rc = lib.desire_select_diverse(a["h"], a["Y"], a["order"], a["score"], a["metric"], a["t_end"], C.c_float(a["radius"]), C.c_float(a["ux"]),
                                       C.c_float(a["uy"]), a["n_top"], a["out"], a["count"], a["mass"], a["top_Y"], a["top_score"], None)
        assert rc == -1, kw
        assert word in lib.desire_last_error(), (kw, lib.desire_last_error())
    assert not any(buf)


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_every_gpu_shape_keeps_the_margin_and_both_forms_agree(shape, unit):
    d = dims_of(shape)
    s = planted_scores(d, 9)
    order = rank_order(s, d)
    for ui, (ux, uy, radius) in list(enumerate(units_of(d)))[unit:unit + 1]:
        Y, kind = make_inputs(d, radius, ux, uy, seed=31 + ui)
        n_kept = []
        for metric, t_end in cases_of(d):
            v64 = pair_values(Y, metric, t_end, ux, uy, d, np.float64)
            assert margin_of_values(v64, metric, radius) > MARGIN                 # on the float64 distances alone, before any comparison
            a, b = select_f32(Y, order, s, metric, t_end, radius, ux, uy, d), select_f64(Y, order, s, metric, t_end, radius, ux, uy, d, values=v64)
            for key in ("order", "count", "owner"):
                np.testing.assert_array_equal(a[key], b[key])
            assert (np.sort(a["order"], 1) == np.arange(d.K)).all() and (a["count"] >= 1).all()
            np.testing.assert_allclose(a["mass"].astype(np.float64), b["mass"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(b["mass"].sum(1), 1.0, rtol=0, atol=1e-12)
            assert (b["mass"][np.arange(d.K)[None] >= b["count"][:, None]] == 0).all()
            n_kept.append(b["count"])
        n_kept = np.stack(n_kept)
        if d.K >= 3:                                       # the inputs exercise the pass: something is suppressed and something is not
            assert (n_kept < d.K).any() and (n_kept > 1).any()
        if d.mno >= 2:                                     # the absent slot: one kept, the order the input's
            assert (n_kept[:, d.mno - 1] == 1).all()
            np.testing.assert_array_equal(a["order"][d.mno - 1], order[d.mno - 1])


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_the_vectorised_pass_is_the_plain_one(shape):
    d = dims_of(shape)
    ux, uy, radius = units_of(d)[1]
    Y, kind = make_inputs(d, radius, ux, uy, seed=5)
    s = planted_scores(d, 3)
    order = rank_order(s, d)
    for metric in METRICS:
        near = near_matrix(Y, metric, d.T_pred, radius, ux, uy, d, np.float64)
        got = select_f64(Y, order, s, metric, d.T_pred, radius, ux, uy, d)
        w = weights(s, d, np.float64)
        for a in range(min(d.A, 12)):
            want_order, want_count, want_owner = brute_force(near[a], order[a])
            assert list(got["order"][a]) == want_order and got["count"][a] == want_count and list(got["owner"][a]) == want_owner
            m = np.zeros(d.K)
            for j, k in enumerate(order[a]):
                m[want_owner[j]] += w[a, k]
            np.testing.assert_allclose(got["mass"][a], m, rtol=0, atol=1e-15)


def test_a_chain_depends_on_the_score_order():
    d = small_dims(n_scenes=1, mno=1, K=3, T_obs=4, T_pred=4, n_grids=1, H=64)
    Y = np.zeros((3, 4, 2), np.float32)
    Y[:, :, 0] = np.array([0.0, 0.7, 1.4], np.float32)[:, None]                   # A - B - C, radius 1
    for order, want, count in (([0, 1, 2], [0, 2, 1], 2), ([1, 0, 2], [1, 0, 2], 1), ([2, 0, 1], [2, 0, 1], 2)):
        for metric in METRICS:
            for sel in (select_f32, select_f64):
                r = sel(Y, np.array([order]), None, metric, 4, 1.0, 1.0, 1.0, d)
                assert list(r["order"][0]) == want and r["count"][0] == count, (order, metric)
    r = select_f32(Y, np.array([[0, 1, 2]]), None, DIST_MEAN, 4, 1.0, 1.0, 1.0, d)
    np.testing.assert_array_equal(r["mass"][0], np.array([np.float32(1) / np.float32(3) + np.float32(1) / np.float32(3), np.float32(1) / np.float32(3), 0], np.float32))
    assert list(r["owner"][0]) == [0, 0, 1]


def test_radius_zero_is_the_identity_and_a_huge_radius_keeps_one():
    d = dims_of((2, 8, 5, 12))
    ux, uy, radius = units_of(d)[1]
    Y, _ = make_inputs(d, radius, ux, uy, seed=2)
    s = planted_scores(d, 4)
    order = rank_order(s, d)
    for metric in METRICS:
        for sel, dt in ((select_f32, np.float32), (select_f64, np.float64)):
            z = sel(Y, order, s, metric, d.T_pred, 0.0, ux, uy, d)
            np.testing.assert_array_equal(z["order"], order)
            assert (z["count"] == d.K).all()
            w = weights(s, d, dt)
            np.testing.assert_array_equal(z["mass"], np.take_along_axis(w, order.astype(np.int64), 1))      # w in processing order
            big = sel(Y, order, s, metric, d.T_pred, 1e30, ux, uy, d)
            np.testing.assert_array_equal(big["order"], order)
            assert (big["count"] == 1).all() and (big["owner"] == 0).all()
    # a NaN is never near: the sample with one keeps apart under every metric that walks its frame
    Yn = Y.copy()
    Yn.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2)[0, 1, 0, d.T_pred - 1, 0] = np.nan
    for metric in METRICS:
        r = select_f32(Yn, order, None, metric, d.T_pred, 1e30, ux, uy, d)
        assert r["count"][0] == 2 and (r["count"][1:] == 1).all()
