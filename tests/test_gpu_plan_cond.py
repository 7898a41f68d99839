"""The K joint futures conditioned on each candidate ego plan on the device (desire_plan_risk_cond, csrc/kernels_plan_cond.hip and the per-plan
instantiation of csrc/kernels_plan.hip's walk) against the numpy statements of its contract (tests/plan_cond_reference.py): dist, cond, first and
clear bit for bit with plan_cond_f32; cw within (K + 8) 2^-24, risk and blame within plan_reference.risk_bound, support and ess within the bounds
derived in the reference's docstring, all of plan_cond_f64.  Then the exact anchors of the contract, independence and reproducibility, alignment,
the optional outputs, the prediction form, capture, refused arguments, and the calls through DESIREModel and the command line.

Observed on an MI355X: see DESIGN.md section 7m."""
import collections
import ctypes as C
import inspect
import itertools
import json

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import EVAL_FLAGS as _FLAGS, PLAIN_KEYS as _PLAIN_KEYS, walking_video as _video, at_byte_offset, make_case, small_dims
from tests.plan_cond_reference import (MARGIN, SHAPES, cond_case, cond_dims, cond_ref, cw_bound, ess_bound, plan_cond_f32, plan_cond_f64,
                                       plan_cond_geometry, planted_identical, planted_nan, planted_one_hot, risk_bound, support_bound)

pytestmark = pytest.mark.gpu
FILL, IFILL = -7.0, -77
RISK_KEYS = ("first", "clear", "risk", "blame")
KEYS = RISK_KEYS + ("cw", "dist", "ess", "support", "cond")
OPTIONAL = ("first", "clear", "blame", "dist", "ess", "support", "cond")
IDS = lambda s: "n%d_m%d_K%d_T%d_M%d" % s
PASSES = (2, 8, 3, 200, 64)      # 64 plans of 200 frames: the weights walk the frames in two passes (118 + 82) with the ego rows in global memory


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _t(torch, a):
    return None if a is None else torch.as_tensor(np.array(a, order="C"), device="cuda")      # (a copy: the shared inputs are read-only)


def _ptr(x):
    return x.data_ptr() if x is not None else 0


def _buffers(torch, d, M, nh, want=OPTIONAL):
    n, K, m = d.n_scenes, d.K, d.mno
    i32 = torch.int32
    shapes = {"first": ((n, M, K + 1), i32), "clear": ((n, M, K + 1, nh), None), "risk": ((n, M, nh), None), "blame": ((n, M, nh, m), None),
              "cw": ((n, M, K), None), "dist": ((n, M, K), None), "ess": ((n, M), None), "support": ((n, M), None), "cond": ((n, M), i32)}
    return {k: (torch.full(s, IFILL if t is i32 else FILL, device="cuda", dtype=t or torch.float32) if k in ("risk", "cw") or k in want else None)
            for k, (s, t) in shapes.items()}


def _call(torch, h, d, M, Y_t, fut_t, pres_t, s_t, plans_t, ego_t, hz, radius, ux, uy, sigma, t_cond, want=OPTIONAL, stream=0):
    buf = _buffers(torch, d, M, len(hz), want)
    h.plan_risk_cond(Y_t.data_ptr(), _ptr(fut_t), _ptr(pres_t), _ptr(s_t), plans_t.data_ptr(), _ptr(ego_t), M, hz, radius, ux, uy, sigma, t_cond,
                     buf["risk"].data_ptr(), buf["cw"].data_ptr(), _ptr(buf["first"]), _ptr(buf["clear"]), _ptr(buf["blame"]), _ptr(buf["dist"]),
                     _ptr(buf["ess"]), _ptr(buf["support"]), _ptr(buf["cond"]), stream)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in buf.items()}


def _plain(torch, h, d, M, Y_t, fut_t, pres_t, s_t, plans_t, ego_t, hz, radius, ux, uy):
    """desire_plan_risk on the same inputs."""
    buf = _buffers(torch, d, M, len(hz), ("first", "clear", "blame"))
    h.plan_risk(Y_t.data_ptr(), _ptr(fut_t), _ptr(pres_t), _ptr(s_t), plans_t.data_ptr(), _ptr(ego_t), M, hz, radius, ux, uy, buf["risk"].data_ptr(),
                buf["first"].data_ptr(), buf["clear"].data_ptr(), buf["blame"].data_ptr(), 0)
    torch.cuda.synchronize()
    return {k: buf[k].cpu().numpy() for k in RISK_KEYS}


def _inputs(c, **kw):
    a = dict(Y=c["Y"], fut=c["fut"], present=None, score=c["score"], plans=c["plans"], ego=c["ego"])
    a.update(kw)
    return a


def _run(torch, h, c, sigma, t_cond, plain=False, want=OPTIONAL, **kw):
    a = _inputs(c, **kw)
    ux, uy, radius = c["unit"]
    args = (torch, h, c["d"], int(np.asarray(a["plans"]).shape[1]), _t(torch, a["Y"]), _t(torch, a["fut"]), _t(torch, a["present"]), _t(torch, a["score"]),
            _t(torch, a["plans"]), _t(torch, a["ego"]), c["hz"], radius, ux, uy)
    return _plain(*args) if plain else _call(*args, sigma, t_cond, want=want)


def _reference(c, fn, sigma, t_cond, **kw):
    a = _inputs(c, **kw)
    ux, uy, radius = c["unit"]
    return fn(a["Y"], a["fut"], a["present"], a["score"], a["plans"], a["ego"], c["hz"], radius, ux, uy, c["d"], sigma, t_cond)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b, keys=KEYS, rows=slice(None)):
    for key in keys:
        if a.get(key) is None or b.get(key) is None:
            continue
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key][rows]), err_msg=key)


def _check(got, f32, f64, d, tag=""):
    """The device against both statements: C1 - C3 and the weight-free outputs bit for bit, the rest within the derived bounds of float64."""
    for key in ("cond", "first", "clear"):
        np.testing.assert_array_equal(_bits(got[key]), _bits(f32[key]), err_msg=key)
    nan = np.isnan(f32["dist"])                                            # a NaN distance is a NaN on both sides (its sign and payload are nobody's contract)
    np.testing.assert_array_equal(np.isnan(got["dist"]), nan)
    np.testing.assert_array_equal(_bits(got["dist"])[~nan], _bits(f32["dist"])[~nan], err_msg="dist")
    np.testing.assert_array_equal(got["first"], f64["first"])
    gaps = {}
    for key, bound in (("cw", cw_bound(d)), ("risk", risk_bound(d)), ("blame", risk_bound(d)), ("support", support_bound(d)),
                       ("ess", ess_bound(d, f64["ess"]))):
        gap = np.abs(got[key].astype(np.float64) - f64[key])
        basis = np.abs(f32[key].astype(np.float64) - f64[key])
        rel = float((gap / bound).max()) if key == "ess" else float(gap.max()) / bound
        gaps[key] = rel
        print("%s %s: max |dev - f64| = %.3g, |f32 - f64| = %.3g, bound %.3g (%.2f of it)"
              % (tag, key, float(gap.max()), float(basis.max()), float(np.max(bound)), rel))
    for key, rel in gaps.items():
        assert rel <= 1.0, key


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES + [PASSES], ids=IDS)
def test_everything_matches_the_references(torch_cuda, shape, unit):
    torch = torch_cuda
    from desire_amd import _lib
    c = cond_case(shape, unit)
    d = c["d"]
    if shape == PASSES:
        assert plan_cond_geometry(d.K, d.T_pred, c["M"]) == (64, 118, 0) and plan_cond_geometry(d.K, d.T_pred // 2, c["M"]) == (64, 100, 1)
    radius = c["unit"][2]
    h = _lib.Handle(d)
    seen = 0
    for sigma, t_cond in itertools.product((radius / 2, 2 * radius), (d.T_pred, max(1, d.T_pred // 2))):
        f64 = cond_ref(c, plan_cond_f64, sigma, t_cond)
        assert f64["margin"] > MARGIN                                      # the float64 pass alone, before any comparison
        f32 = cond_ref(c, plan_cond_f32, sigma, t_cond)
        got = _run(torch, h, c, sigma, t_cond)
        _check(got, f32, f64, d, "%s u%d s%.3g t%d" % (IDS(shape), unit, sigma, t_cond))
        seen += int((got["cond"] > 0).sum())
    assert seen > 0
    h.close()


def test_the_exact_anchors(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    c = cond_case(SHAPES[2], 1)
    d, M = c["d"], c["M"]
    radius = c["unit"][2]
    sigma, T = 2 * radius, d.T_pred
    h = _lib.Handle(d)
    one = np.float32(1)
    # ---- nobody replaced (NULL, negative, >= mno): desire_plan_risk, the prior's weights in every row
    for ego, plain_ego in ((None, None), (np.full_like(c["ego"], -1), None), (np.full_like(c["ego"], d.mno), None)):
        got = _run(torch, h, c, sigma, T, ego=ego)
        base = _run(torch, h, c, sigma, T, plain=True, ego=plain_ego)
        _same_bits(got, base, keys=RISK_KEYS)
        W = plan_cond_f32(**_ref_args(c, sigma, T, ego=ego))["W"]
        assert np.abs(got["cw"] - W[:, None]).max() <= cw_bound(d) and (got["cw"] == got["cw"][:, :1]).all()
        assert (got["support"] == 1).all() and (got["dist"] == 0).all() and (got["cond"] == 0).all()
    # ---- a sigma whose square overflows: inv = 0, the prior again wherever the distances are finite
    prior_cw = got["cw"]
    big = _run(torch, h, c, 1e20, T)
    base = _run(torch, h, c, sigma, T, plain=True)
    fin = np.isfinite(big["dist"]).all(-1)
    assert fin.any() and (big["cond"][fin] > 0).any()
    np.testing.assert_array_equal(_bits(big["cw"][fin]), _bits(prior_cw[fin]))
    for key in ("risk", "blame"):
        np.testing.assert_array_equal(_bits(big[key][fin]), _bits(base[key][fin]), err_msg=key)
    _same_bits(big, base, keys=("first", "clear"))
    # ---- NULL scores, the ego slot's K rows identical: 1 / K exactly
    Y, ego = planted_identical(c)
    flat = _run(torch, h, c, sigma, T, Y=Y, ego=ego, score=None)
    assert (flat["cond"] > 0).any()
    np.testing.assert_array_equal(_bits(flat["cw"]), _bits(np.full(flat["cw"].shape, one / np.float32(d.K), np.float32)))
    _same_bits(flat, _run(torch, h, c, sigma, T, plain=True, Y=Y, ego=ego, score=None), keys=RISK_KEYS)
    # ---- the plan is world k0's own ego row: that world alone
    plans, ego, k0, small, live = planted_one_hot(c)
    hot = _run(torch, h, c, small, T, plans=plans, ego=ego, score=None)
    want = np.zeros(hot["cw"].shape, np.float32)
    want[:, np.arange(M), k0] = 1
    assert (hot["cond"][live] == T).all() and (hot["cond"][~live] == 0).all()
    np.testing.assert_array_equal(_bits(hot["cw"][live]), _bits(want[live]))
    assert (hot["ess"][live] == 1).all()
    risk = (hot["first"][:, np.arange(M), k0][..., None] < np.asarray(c["hz"])).astype(np.float32)
    np.testing.assert_array_equal(_bits(hot["risk"][live]), _bits(risk[live]))
    # ---- a NaN in one world's ego row: not conditioned, the prior's weights, and dist carries the NaN
    f64 = cond_ref(c, plan_cond_f64, sigma, T)
    Y, w, mi, k1 = planted_nan(c, f64)
    bad = _run(torch, h, c, sigma, T, Y=Y)
    assert bad["cond"][w, mi] == 0 and np.isnan(bad["dist"][w, mi, k1]) and np.isfinite(np.delete(bad["dist"][w, mi], k1)).all()
    np.testing.assert_array_equal(_bits(bad["cw"][w, mi]), _bits(prior_cw[w, mi]))
    assert bad["support"][w, mi] == 1
    _check(bad, _reference(c, plan_cond_f32, sigma, T, Y=Y), _reference(c, plan_cond_f64, sigma, T, Y=Y), d, "nan row")
    h.close()


def _ref_args(c, sigma, t_cond, **kw):
    a = _inputs(c, **kw)
    ux, uy, radius = c["unit"]
    return dict(a, horizons=c["hz"], radius=radius, ux=ux, uy=uy, d=c["d"], sigma=sigma, t_cond=t_cond)


def test_results_are_bitwise_reproducible_and_depend_on_the_window_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    for shape in ((4, 8, 3, 7, 5), (4, 256, 2, 40, 3)):                    # the second one walks the risk's frames in chunks
        c = cond_case(shape, 1, seed=11)
        d, M, hz = c["d"], c["M"], c["hz"]
        ux, uy, radius = c["unit"]
        sigma, t_cond = 2 * radius, d.T_pred
        s = c["score"]
        h = _lib.Handle(d)
        hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
        h2 = _lib.Handle(d.replace(n_scenes=2))
        ref = _run(torch, h, c, sigma, t_cond)
        assert (ref["cond"] > 0).any() and ref["risk"].max() > 0
        _same_bits(_run(torch, h, c, sigma, t_cond), ref)                  # run to run
        _same_bits(_run(torch, hc, c, sigma, t_cond), ref)                 # the padding-skipping flags are not its business
        Yw = c["Y"].reshape(d.n_scenes, d.K * d.mno, d.T_pred, 2)

        def sub(hh, rows, plans=None, ego=None, MM=M):
            return _call(torch, hh, hh.dims, MM, _t(torch, Yw[rows]), _t(torch, c["fut"][rows]), None, _t(torch, s[rows]),
                         _t(torch, c["plans"][rows] if plans is None else plans), _t(torch, c["ego"][rows] if ego is None else ego), hz, radius, ux, uy,
                         sigma, t_cond)

        for lo in (0, 2):                                                  # four windows in one call = two calls of two
            _same_bits(sub(h2, slice(lo, lo + 2)), ref, rows=slice(lo, lo + 2))
        perm = np.array([0, 3, 1, 2])                                      # the other windows permuted: every window keeps its results
        _same_bits(sub(h, perm), {k: v[perm] for k, v in ref.items()})
        extra = 70                                                         # M padded by extra plans: another cut into chunks, the same bits
        assert plan_cond_geometry(d.K, t_cond, M + extra)[0] < M + extra
        pl = np.concatenate([c["plans"], np.repeat(c["plans"][:, :1], extra, 1) + np.float32(0.001)], 1)
        eg = np.concatenate([c["ego"], np.full((d.n_scenes, extra), -1, np.int32)], 1)
        wide = sub(h, slice(None), plans=pl, ego=eg, MM=M + extra)
        _same_bits({k: v[:, :M] for k, v in wide.items()}, ref)
        for x in (h, hc, h2):
            x.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[0], (2, 32, 2, 200, 4)], ids=IDS)
def test_buffers_off_16_byte_alignment(torch_cuda, shape, off):
    """The 8-byte path of the streaming loop, for the sample tensor (the staged ego rows) and for the plans: the aligned call's bits."""
    torch = torch_cuda
    from desire_amd import _lib
    c = cond_case(shape, 1)
    d, M, hz = c["d"], c["M"], c["hz"]
    ux, uy, radius = c["unit"]
    h = _lib.Handle(d)
    Y_t, fut_t, s_t, pl_t, ego_t = (_t(torch, x) for x in (c["Y"], c["fut"], c["score"], c["plans"], c["ego"]))
    tail = (hz, radius, ux, uy, 2 * radius, d.T_pred)
    ref = _call(torch, h, d, M, Y_t, fut_t, None, s_t, pl_t, ego_t, *tail)
    np.testing.assert_array_equal(ref["dist"], cond_ref(c, plan_cond_f32, 2 * radius, d.T_pred)["dist"])
    for ya, pa in ((True, False), (False, True), (True, True)):
        got = _call(torch, h, d, M, at_byte_offset(Y_t, off) if ya else Y_t, fut_t, None, s_t, at_byte_offset(pl_t, off) if pa else pl_t, ego_t, *tail)
        _same_bits(got, ref)
    h.close()


def test_plans_of_one_chunk_that_name_different_slots(torch_cuda):
    """Mixed ego slots take the rows from global memory, one slot per call stages them in the LDS: the same bits plan by plan."""
    torch = torch_cuda
    from desire_amd import _lib
    c = cond_case(SHAPES[2], 1)
    d, M = c["d"], c["M"]
    sigma, T = 2 * c["unit"][2], d.T_pred
    assert plan_cond_geometry(d.K, T, M) == (M, T, 1) and plan_cond_geometry(d.K, T, 1) == (1, T, 1)
    assert len(set(c["ego"][0][c["ego"][0] >= 0].tolist())) > 1             # one chunk, several slots
    h = _lib.Handle(d)
    whole = _run(torch, h, c, sigma, T)
    for mi in range(M):
        one = _run(torch, h, c, sigma, T, plans=c["plans"][:, mi:mi + 1], ego=c["ego"][:, mi:mi + 1])
        _same_bits(one, {k: v[:, mi:mi + 1] for k, v in whole.items()})
    same = np.ascontiguousarray(np.broadcast_to(c["ego"].max(1, keepdims=True), c["ego"].shape))      # ... and every plan on one slot
    assert (same >= 0).all()
    whole = _run(torch, h, c, sigma, T, ego=same)
    assert (whole["cond"] > 0).any()
    for mi in (0, M - 1):
        one = _run(torch, h, c, sigma, T, plans=c["plans"][:, mi:mi + 1], ego=same[:, mi:mi + 1])
        _same_bits(one, {k: v[:, mi:mi + 1] for k, v in whole.items()})
    h.close()


def test_the_present_form_and_every_choice_of_optional_outputs(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    c = dict(cond_case(SHAPES[0], 1))
    d = c["d"]
    sigma, T = 2 * c["unit"][2], d.T_pred
    fut = c["fut"].copy()
    fut[..., 0] = fut[:, :1, :, 0]                                         # ids constant over t: the two forms count the same frames
    c["fut"] = fut
    present = (fut[:, 0, :, 0] != 0).reshape(-1).astype(np.uint8)
    h = _lib.Handle(d)
    full = _run(torch, h, c, sigma, T)
    assert (full["cond"] > 0).any()
    pres = _run(torch, h, c, sigma, T, fut=None, present=present)
    _check(pres, _reference(c, plan_cond_f32, sigma, T, fut=None, present=present), _reference(c, plan_cond_f64, sigma, T, fut=None, present=present),
           d, "present")
    for key in ("first", "clear"):
        np.testing.assert_array_equal(_bits(pres[key][:, :, :d.K]), _bits(full[key][:, :, :d.K]), err_msg=key)
    _same_bits(pres, full, keys=("risk", "blame", "cw", "dist", "ess", "support", "cond"))
    np.testing.assert_array_equal(pres["first"][:, :, d.K], d.T_pred)      # no ground truth: row K says so, as desire_plan_risk fills it
    assert np.isposinf(pres["clear"][:, :, d.K]).all()
    _same_bits(pres, _run(torch, h, c, sigma, T, plain=True, fut=None, present=present), keys=("first", "clear"))
    for kw, whole in ((dict(), full), (dict(fut=None, present=present), pres)):
        for n_opt in range(len(OPTIONAL) + 1):
            for want in itertools.combinations(OPTIONAL, n_opt):
                _same_bits(_run(torch, h, c, sigma, T, want=want, **kw), whole)
    h.close()


def test_forward_and_the_call_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=4, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    a = make_case(d, seed=21, n_absent=2)
    p, f, e, g = (_t(torch, x) for x in a[:4])
    h = _lib.Handle(d); h.set_weights(w); h.set_scene_grids(g.data_ptr(), a[4])
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    hz, M, radius, sigma, t_cond = [3, 6, 9, 12], 5, 400.0, 300.0, 9
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    out = _buffers(torch, d, M, len(hz))
    plans = torch.zeros((d.n_scenes, M, d.T_pred, 2), device="cuda")
    ego_np = np.tile(np.arange(M, dtype=np.int32), (d.n_scenes, 1))
    ego = _t(torch, ego_np)
    bufs = (Y, sc) + tuple(out[k] for k in KEYS)
    side = torch.cuda.Stream(); sp = side.cuda_stream

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.plan_risk_cond(Y.data_ptr(), f.data_ptr(), 0, sc.data_ptr(), plans.data_ptr(), ego.data_ptr(), M, hz, radius, ux, uy, sigma, t_cond,
                         out["risk"].data_ptr(), out["cw"].data_ptr(), out["first"].data_ptr(), out["clear"].data_ptr(), out["blame"].data_ptr(),
                         out["dist"].data_ptr(), out["ess"].data_ptr(), out["support"].data_ptr(), out["cond"].data_ptr(), sp)

    torch.cuda.synchronize()
    calls()                                                                # eager once: the samples the plans are laid against
    side.synchronize()
    Yk = Y.cpu().numpy().reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2)
    sets = {"near": np.ascontiguousarray(Yk[:, 0, :M]) + np.float32(1e-4), "far": np.full((d.n_scenes, M, d.T_pred, 2), -50.0, np.float32)}
    ref = {}
    for tag in ("far", "near"):
        plans.copy_(_t(torch, sets[tag]))
        torch.cuda.synchronize()
        calls()
        side.synchronize()
        ref[tag] = [x.clone() for x in bufs]
    h.graph_begin(sp)
    calls()
    gid = h.graph_end(sp)
    i32 = torch.int32
    for rep in range(4):
        tag = "far" if rep % 2 == 0 else "near"
        plans.copy_(_t(torch, sets[tag]))                                  # in place: the graph keeps its pointers
        for x in bufs:
            x.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        for x, r in zip(bufs, ref[tag]):
            assert torch.equal(x.view(i32), r.view(i32)), (rep, tag)
    near = dict(zip(KEYS, (x.cpu().numpy() for x in ref["near"][2:])))
    far = dict(zip(KEYS, (x.cpu().numpy() for x in ref["far"][2:])))
    assert (near["cond"] > 0).any() and not np.array_equal(near["cw"], far["cw"]) and float(far["risk"].max()) == 0
    want = plan_cond_f32(ref["near"][0].cpu().numpy(), a[1], None, ref["near"][1].cpu().numpy(), sets["near"], ego_np, hz, radius, ux, uy, d, sigma, t_cond)
    for key in ("dist", "cond", "clear"):
        np.testing.assert_array_equal(_bits(near[key]), _bits(want[key]), err_msg=key)
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = cond_dims((1, 4, 3, 6))
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") + 0.5
    pr = torch.ones(64, device="cuda", dtype=torch.uint8)
    eg = torch.full((64,), -1, device="cuda", dtype=torch.int32)
    i32 = torch.int32
    M = 2
    outs = {k + "_ptr": v for k, v in _buffers(torch, d, M, 8).items()}
    nan, inf = float("nan"), float("inf")
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(plans_ptr=0), "dev_plans"), (dict(risk_ptr=0), "dev_risk"), (dict(cw_ptr=0), "dev_cw"),
             (dict(horizons=[]), "n_h"), (dict(horizons=list(range(1, 10))), "n_h"), (dict(horizons=[0]), "host_horizons"), (dict(horizons=[7]), "host_horizons"),
             (dict(horizons=[3, 3]), "increasing"), (dict(horizons=[4, 2]), "increasing"),
             (dict(M=0), "M must"), (dict(M=-3), "M must"), (dict(radius=-1e-3), "radius"), (dict(radius=nan), "radius"), (dict(radius=inf), "radius"),
             (dict(unit_x=0.0), "unit_x"), (dict(unit_x=-1.0), "unit_x"), (dict(unit_x=nan), "unit_x"), (dict(unit_x=inf), "unit_x"),
             (dict(unit_y=0.0), "unit_y"), (dict(unit_y=-2.0), "unit_y"), (dict(unit_y=nan), "unit_y"), (dict(unit_y=inf), "unit_y"),
             (dict(present_ptr=pr.data_ptr()), "both"), (dict(fut_ptr=0), "both NULL"),
             (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=nan), "sigma"), (dict(sigma=inf), "sigma"),
             (dict(t_cond=0), "t_cond"), (dict(t_cond=-2), "t_cond"), (dict(t_cond=d.T_pred + 1), "t_cond")]
    for kw, word in cases:
        args = dict(yhat_ptr=z.data_ptr(), fut_ptr=z.data_ptr(), present_ptr=0, score_ptr=z.data_ptr(), plans_ptr=z.data_ptr(), ego_ptr=eg.data_ptr(), M=M,
                    horizons=[2, 6], radius=1.0, unit_x=1.0, unit_y=1.0, sigma=1.0, t_cond=d.T_pred, **{k: v.data_ptr() for k, v in outs.items()})
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.plan_risk_cond(**args)
    lib = _lib.load()
    one = C.c_float(1)
    hz2 = (C.c_int32 * 2)(2, 6)
    o = {k: v.data_ptr() for k, v in outs.items()}
    tail = (one, one, one, one, d.T_pred, o["first_ptr"], o["clear_ptr"], o["risk_ptr"], o["blame_ptr"], o["cw_ptr"], o["dist_ptr"], o["ess_ptr"],
            o["support_ptr"], o["cond_ptr"], None)
    assert lib.desire_plan_risk_cond(None, z.data_ptr(), z.data_ptr(), None, None, z.data_ptr(), None, M, hz2, 2, *tail) == -1
    assert b"handle" in lib.desire_last_error()
    assert lib.desire_plan_risk_cond(h._h, z.data_ptr(), z.data_ptr(), None, None, z.data_ptr(), None, M, None, 2, *tail) == -1
    assert b"host_horizons" in lib.desire_last_error()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.plan_risk_cond(z.data_ptr(), z.data_ptr(), 0, 0, z.data_ptr(), 0, M, [8], 1.0, 1.0, 1.0, 1.0, 8, o["risk_ptr"], o["cw_ptr"])
    torch.cuda.synchronize()
    assert all(bool((v == (IFILL if v.dtype == i32 else FILL)).all()) for v in outs.values())
    # ... and the handle still works
    h.plan_risk_cond(z.data_ptr(), z.data_ptr(), 0, 0, z.data_ptr(), 0, M, [2, 6], 0.0, 1.0, 1.0, 1.0, d.T_pred, o["risk_ptr"], o["cw_ptr"])
    torch.cuda.synchronize()
    risk = outs["risk_ptr"].view(-1)[:M * 2]                               # the call's own layout: two horizons
    cw = outs["cw_ptr"].view(-1)[:M * d.K]
    assert bool((risk == 0).all()) and bool((cw == 1.0 / d.K).all()) and bool((outs["first_ptr"] == IFILL).all()) and bool((outs["dist_ptr"] == FILL).all())
    for x in (h, rc):
        x.close()


def _counted(monkeypatch):
    from desire_amd import _lib
    ran = collections.Counter()

    def counted(name, fn):
        def call(self, *a, **kw):
            ran[name] += 1
            return fn(self, *a, **kw)
        return call

    for name, fn in list(vars(_lib.Handle).items()):
        if inspect.isfunction(fn) and name in ("plan_risk", "plan_risk_cond"):
            monkeypatch.setattr(_lib.Handle, name, counted(name, fn))
    return ran


def test_score_plans_and_evaluate_plan_risk_condition_only_under_the_keyword(torch_cuda, monkeypatch):
    torch = torch_cuda
    from desire_amd import evaluate as E
    from desire_amd.model import DESIREModel
    from tests import scored_surface_cases as SC
    past, fut, Y, score, plans, _ = SC.planted()
    m = DESIREModel(E.build_parser().parse_args(_FLAGS), seed=4)
    h = m._handle(SC.N, False)
    d = h.dims
    Yt, st = torch.as_tensor(Y, device="cuda"), torch.as_tensor(score, device="cuda")
    monkeypatch.setattr(m, "forward_device", lambda *a, **kw: (Yt.reshape(d.R, d.T_pred, 2), st.reshape(d.R)))
    ran = _counted(monkeypatch)
    hz, radius, sigma, ego = list(SC.HZ), 30.0, 25.0, [[0, 2, -1], [-1, 2, 0]]
    plain = m.score_plans(list(past), plans, radius, horizons=hz, ego_slot=ego)
    assert dict(ran) == {"plan_risk": 1} and sorted(plain) == ["best", "blame", "clearance", "first", "present", "risk"]
    ran.clear()
    out = m.score_plans(list(past), plans, radius, horizons=hz, ego_slot=ego, condition=True, condition_sigma=sigma, condition_horizon=4)
    assert dict(ran) == {"plan_risk_cond": 1}
    assert sorted(out) == sorted(list(plain) + ["cond_weights", "plan_distance", "ess", "support", "conditioned", "risk_prior"])
    for key in ("first", "clearance", "present"):
        assert torch.equal(out[key], plain[key]), key
    np.testing.assert_allclose(out["risk_prior"].cpu().numpy(), plain["risk"].cpu().numpy(), atol=1e-6)
    pres8 = out["present"].cpu().numpy().reshape(-1).astype(np.uint8)
    scale = np.array([d.sx, d.sy], np.float32)
    args = (Y.reshape(d.R, d.T_pred, 2), None, pres8, score, (plans * scale).astype(np.float32), np.asarray(ego, np.int32), hz, radius, 1.0 / d.sx, 1.0 / d.sy, d,
            sigma, 4)
    f32, f64 = plan_cond_f32(*args), plan_cond_f64(*args)
    got = {"cw": out["cond_weights"], "risk": out["risk"], "blame": out["blame"], "ess": out["ess"], "support": out["support"]}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    np.testing.assert_array_equal(out["conditioned"].cpu().numpy(), f32["conditioned"])
    np.testing.assert_allclose(out["plan_distance"].cpu().numpy(), np.sqrt(f32["dist"]), rtol=1e-6)
    assert f32["conditioned"].any() and not f32["conditioned"].all()
    for key, bound in (("cw", cw_bound(d)), ("risk", risk_bound(d)), ("blame", risk_bound(d)), ("support", support_bound(d)), ("ess", ess_bound(d, f64["ess"]))):
        assert (np.abs(got[key].astype(np.float64) - f64[key]) <= bound).all(), key
    for bad in (dict(condition_sigma=None), dict(condition_sigma=0.0), dict(condition_sigma=float("nan")), dict(condition_sigma=sigma, condition_horizon=0),
                dict(condition_sigma=sigma, condition_horizon=d.T_pred + 1)):
        with pytest.raises(ValueError, match="condition"):
            m.score_plans(list(past), plans, radius, ego_slot=ego, condition=True, **bad)
    with pytest.raises(ValueError, match="ego_slot"):
        m.score_plans(list(past), plans, radius, condition=True, condition_sigma=sigma)
    # ---- the leave-one-out form
    ran.clear()
    base = m.evaluate_plan_risk(Yt, st, list(fut), radius, horizons=hz)
    assert dict(ran) == {"plan_risk": 1} and sorted(base) == ["actual", "agents", "first", "predicted", "risk", "takes_part"]
    ran.clear()
    given = m.evaluate_plan_risk(Yt, st, list(fut), radius, horizons=hz, condition=True, condition_sigma=sigma)
    assert dict(ran) == {"plan_risk": 1, "plan_risk_cond": 1}
    assert sorted(given) == sorted(list(base) + ["risk_given", "ess", "predicted_given", "ess_mean"])
    for key in base:
        np.testing.assert_array_equal(given[key], base[key], err_msg=key)
    assert given["risk_given"].shape == base["risk"].shape and given["predicted_given"].shape == base["predicted"].shape
    assert (given["ess"] >= 1 - 1e-5).all() and (given["ess"] <= d.K + 1e-4).all() and (given["ess_mean"][given["agents"] > 0] >= 1 - 1e-5).all()
    assert not np.array_equal(given["risk_given"], base["risk"])


def test_the_command_line_adds_the_conditioned_columns_only_when_asked(torch_cuda):
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    video = _video()
    res = {}
    for tag, extra in (("plain", []), ("risk", ["--plan_risk", "--collision_radius", "40"]),
                       ("given", ["--plan_risk", "--collision_radius", "40", "--plan_risk_sigma", "30", "--plan_risk_cond_horizon", "4"])):
        a = E.build_parser().parse_args(_FLAGS + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=DESIREModel(a, seed=4))
    assert list(res["plain"]) == _PLAIN_KEYS
    nh = len(res["plain"]["horizons"])
    assert list(res["risk"]["plan_risk"]) == ["collision_radius_px", "agents", "predicted_risk", "actual_rate"]      # without the flag: the block it was
    blk = dict(res["given"]["plan_risk"])
    assert list(blk) == ["collision_radius_px", "agents", "predicted_risk", "actual_rate", "predicted_risk_given", "ess"]
    given, ess = blk.pop("predicted_risk_given"), blk.pop("ess")
    res["given"]["plan_risk"] = blk
    assert json.dumps(res["given"], indent=1) == json.dumps(res["risk"], indent=1)      # ... and with it, the same bytes plus two columns
    assert len(given) == len(ess) == nh and all(0.0 <= v <= 1.0 + 1e-6 for v in given) and all(v >= 1.0 - 1e-5 for v in ess)
