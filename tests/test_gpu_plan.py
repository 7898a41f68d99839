"""Candidate ego plans against the K joint futures on the device (desire_plan_risk, csrc/kernels_plan.hip) against the numpy statements of its
contract (tests/plan_reference.py).  `first` is compared exactly with plan_f32 AND plan_f64 -- on inputs whose every (plan, slot, frame) keeps, in
float64, a margin of 1e-3 r2 from r2, asserted first on the float64 pass alone -- `clear` with plan_f32 bit for bit, `risk` and `blame` with
plan_f32 bit for bit where every weight is 1 / K (NULL scores, equal joint scores) and within (K + 8) * 2^-24 of plan_f64 under the planted scores.
Then the anchors to desire_joint_metrics, the exact boundary, independence and reproducibility, alignment, the optional outputs, capture, refused
arguments, and the calls through DESIREModel and the command line.

Observed on an MI355X: see DESIGN.md section 7i."""
import ctypes as C
import itertools

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import (EVAL_FLAGS as _FLAGS, PLAIN_KEYS as _PLAIN_KEYS, walking_video as _video,
                           at_byte_offset, make_case, small_dims)
from tests.plan_reference import (MARGIN, RADIUS_PX, SHAPES, equal_joint_scores, brute_force_first, make_inputs, plan_centres, plan_f32, plan_f64,
                                  plan_geometry, planted_joint_scores, risk_bound)

pytestmark = pytest.mark.gpu
FILL, IFILL = -7.0, -77
KEYS = ("first", "clear", "risk", "blame")
IDS = lambda s: "n%d_m%d_K%d_T%d_M%d" % s
_CASES = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _t(torch, a):
    return None if a is None else torch.as_tensor(np.array(a, order="C"), device="cuda")      # (a copy: the shared inputs are read-only)


def _dims(shape, **kw):
    n, m, K, T = shape[:4]
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64, **kw)


def _units(d):
    return [(1.0, 1.0, float(np.float32(RADIUS_PX * d.sx))), (1.0 / d.sx, 1.0 / d.sy, RADIUS_PX)]      # (unit_x, unit_y, the radius in that unit)


def _hz(T):
    return sorted({max(1, T // 4), max(1, T // 2), T})


def _case(shape, unit, seed=5):
    """Inputs of (shape, unit) and the score-free part of both references, computed once and left unchanged."""
    key = (shape, unit, seed)
    if key not in _CASES:
        d = _dims(shape)
        M = shape[4]
        ux, uy, radius = _units(d)[unit]
        Y, fut, present, plans, ego, info = make_inputs(d, M, radius, ux, uy, seed=seed + unit, centres=plan_centres(d.mno, d.T_pred, M))
        for a in (Y, fut, present, plans, ego):
            a.setflags(write=False)
        _CASES[key] = dict(d=d, M=M, Y=Y, fut=fut, present=present, plans=plans, ego=ego, info=info, hz=_hz(d.T_pred), unit=(ux, uy, radius))
    return _CASES[key]


def _ref(c, fn, score, fut=True, ego=True):
    ux, uy, radius = c["unit"]
    return fn(c["Y"], c["fut"] if fut else None, None if fut else c["present"], score, c["plans"], c["ego"] if ego else None, c["hz"], radius, ux, uy,
              c["d"])


def _call(torch, h, d, M, Y_t, fut_t, pres_t, s_t, plans_t, ego_t, hz, radius, ux, uy, first=True, clear=True, blame=True, stream=0):
    n, K, m, nh = d.n_scenes, d.K, d.mno, len(hz)
    buf = {"first": torch.full((n, M, K + 1), IFILL, device="cuda", dtype=torch.int32) if first else None,
           "clear": torch.full((n, M, K + 1, nh), FILL, device="cuda") if clear else None,
           "risk": torch.full((n, M, nh), FILL, device="cuda"),
           "blame": torch.full((n, M, nh, m), FILL, device="cuda") if blame else None}
    ptr = lambda x: x.data_ptr() if x is not None else 0
    h.plan_risk(Y_t.data_ptr(), ptr(fut_t), ptr(pres_t), ptr(s_t), plans_t.data_ptr(), ptr(ego_t), M, hz, radius, ux, uy, buf["risk"].data_ptr(),
                ptr(buf["first"]), ptr(buf["clear"]), ptr(buf["blame"]), stream)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in buf.items()}


def _run(torch, h, c, score, fut=True, ego=True, **kw):
    ux, uy, radius = c["unit"]
    return _call(torch, h, c["d"], c["M"], _t(torch, c["Y"]), _t(torch, c["fut"]) if fut else None, None if fut else _t(torch, c["present"]),
                 _t(torch, score), _t(torch, c["plans"]), _t(torch, c["ego"]) if ego else None, c["hz"], radius, ux, uy, **kw)


def _same_bits(a, b, keys=KEYS, rows=slice(None)):
    for key in keys:
        if a[key] is None or b[key] is None:
            continue
        np.testing.assert_array_equal(a[key].view(np.uint32), b[key][rows].view(np.uint32), err_msg=key)


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_everything_matches_the_reference(torch_cuda, shape, unit):
    torch = torch_cuda
    from desire_amd import _lib
    c = _case(shape, unit)
    d = c["d"]
    s = planted_joint_scores(d, 9)
    f64 = _ref(c, plan_f64, s)
    assert f64["margin"] > MARGIN                                          # the float64 pass alone, before any comparison
    f32 = _ref(c, plan_f32, s)
    h = _lib.Handle(d)
    got = _run(torch, h, c, s)
    np.testing.assert_array_equal(got["first"], f32["first"])
    np.testing.assert_array_equal(got["first"], f64["first"])
    ux, uy, radius = c["unit"]
    np.testing.assert_array_equal(got["first"], brute_force_first(c["Y"], c["fut"], c["plans"], c["ego"], radius, ux, uy, d))
    np.testing.assert_array_equal(got["clear"].view(np.uint32), f32["clear"].view(np.uint32))
    if d.mno > 1:
        assert (got["first"] < d.T_pred).any() and (got["first"] == d.T_pred).any() and np.isfinite(got["clear"]).any()
    for key in ("risk", "blame"):
        gap = float(np.abs(got[key].astype(np.float64) - f64[key]).max())
        basis = float(np.abs(f32[key].astype(np.float64) - f64[key]).max())
        print("%s: max |dev - f64| = %.3g, |f32 - f64| = %.3g, bound %.3g" % (key, gap, basis, risk_bound(d)))
        assert gap <= risk_bound(d), key
    # every weight 1 / K: NULL scores, and scores whose K joint sums are equal -- the bits of the fp32 statement
    flat = _run(torch, h, c, None)
    r32 = _ref(c, plan_f32, None)
    _same_bits(flat, r32)
    eq = _run(torch, h, c, equal_joint_scores(d, 4))
    _same_bits(eq, r32)
    _same_bits(flat, got, keys=("first", "clear"))
    if d.mno > 1:
        assert flat["risk"].max() > 0 and flat["blame"].max() > 0
    h.close()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=IDS)
def test_anchored_to_joint_metrics(torch_cuda, shape):
    """Plan m = slot m's own row of sample k0, replacing slot m: its first contact with the others in joint future k0 is what desire_joint_metrics
    reports for slot m there.  Plan m = the recorded future of slot m: row K is the joint call's ground-truth row, for slots counted in every frame."""
    torch = torch_cuda
    from desire_amd import _lib
    c = _case(shape, 1)
    d, hz = c["d"], c["hz"]
    ux, uy, radius = c["unit"]
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    h = _lib.Handle(d)
    Y_t, fut_t, p_t = _t(torch, c["Y"]), _t(torch, c["fut"]), _t(torch, c["present"])
    ego_t = _t(torch, np.broadcast_to(np.arange(m, dtype=np.int32), (n, m)))
    i32 = torch.int32

    def joint(fut, pres):
        first = torch.full((n, K + 1, m), IFILL, device="cuda", dtype=i32)
        cnt = torch.zeros((n, K + 1, len(hz), 2), device="cuda", dtype=i32)
        jo = torch.zeros((n, K), device="cuda", dtype=i32)
        h.joint_metrics(Y_t.data_ptr(), fut.data_ptr() if fut is not None else 0, pres.data_ptr() if pres is not None else 0, 0, hz, 1, radius, ux, uy,
                        cnt.data_ptr(), jo.data_ptr(), first.data_ptr())
        torch.cuda.synchronize()
        return first.cpu().numpy()

    Yk = c["Y"].reshape(n, K, m, T, 2)
    jp = joint(None, p_t)
    pres = c["present"].reshape(n, m) != 0
    touched = 0
    for k0 in sorted({0, K // 2, K - 1}):
        got = _call(torch, h, d, m, Y_t, None, p_t, None, _t(torch, Yk[:, k0]), ego_t, hz, radius, ux, uy)
        np.testing.assert_array_equal(got["first"][:, :, k0][pres], jp[:, k0][pres])
        touched += int((jp[:, k0][pres] < T).sum())
    assert touched > 0
    g = np.stack([c["fut"][..., 1] * np.float32(d.sx), c["fut"][..., 2] * np.float32(d.sy)], -1).astype(np.float32).transpose(0, 2, 1, 3)
    got = _call(torch, h, d, m, Y_t, fut_t, None, None, _t(torch, g), ego_t, hz, radius, ux, uy)
    whole = (c["fut"][..., 0] != 0).all(1)                                  # [n, m]: counted in every frame
    jf = joint(fut_t, None)
    np.testing.assert_array_equal(got["first"][:, :, K][whole], jf[:, K][whole])
    assert (jf[:, K][whole] < T).any() and (jf[:, K][whole] == T).any()
    h.close()


def _ulps_around(x, n):
    """The 2 n + 1 floats around x."""
    lo = np.float32(x)
    for _ in range(n):
        lo = np.nextafter(lo, np.float32(-np.inf))
    out = []
    for _ in range(2 * n + 1):
        out.append(lo)
        lo = np.nextafter(lo, np.float32(np.inf))
    return out


def test_the_boundary_is_exact(torch_cuda):
    """Slot 0 of sample 1 stands at the origin, so a and b are the plan's own coordinates: three plans near (3/8, 4/8) whose fp32 q is one ulp
    below r2 = 0.625^2 = 25/64, equal to it and one ulp above it.  Only the first touches (the comparison is strict).  Radius 0: nothing touches,
    not even a coincident plan."""
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((2, 4, 2, 6))
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    f32 = np.float32
    r0 = f32(0.625)
    r2 = f32(r0 * r0)
    assert r2 == f32(25 / 64)
    want = {"below": np.nextafter(r2, f32(0)), "equal": r2, "above": np.nextafter(r2, f32(1))}
    at = {}
    for b, a in itertools.product(_ulps_around(0.5, 4), _ulps_around(0.375, 16)):
        q = f32(f32(a * a) + f32(b * b))
        for name, v in want.items():
            if q == v:
                at.setdefault(name, (a, b))
    assert sorted(at) == ["above", "below", "equal"]
    Yk = np.zeros((n, K, m, T, 2), f32)
    Yk[:, 0, 0] = 300.0                                                    # slot 0 of sample 0: far off
    for i in range(1, m):
        Yk[:, :, i] = f32(40.0 * i)
    Y = np.ascontiguousarray(Yk.reshape(d.R, T, 2))
    names = ("below", "equal", "above")
    plans = np.zeros((n, 4, T, 2), f32)                                    # plan 3: the origin itself
    for j, name in enumerate(names):
        plans[:, j] = np.array(at[name], f32)
    present = np.ones(n * m, np.uint8)
    h = _lib.Handle(d)
    Y_t, p_t, pl_t = _t(torch, Y), _t(torch, present), _t(torch, plans)
    hz = [1, T]
    got = _call(torch, h, d, 4, Y_t, None, p_t, None, pl_t, None, hz, float(r0), 1.0, 1.0)
    np.testing.assert_array_equal(got["first"][:, 0, 1], 0)                # one ulp below r2: touches from frame 0
    np.testing.assert_array_equal(got["first"][:, 1:3, 1], T)              # equal, and one ulp above: not
    np.testing.assert_array_equal(got["first"][:, 3, 1], 0)
    np.testing.assert_array_equal(got["first"][:, :, 0], T)
    for j, name in enumerate(names):
        np.testing.assert_array_equal(got["clear"][:, j, 1].view(np.uint32), np.full((n, 2), want[name], f32).view(np.uint32))
    np.testing.assert_array_equal(got["risk"][:, 0], f32(1) / f32(K))      # one of the K futures, equal weights
    np.testing.assert_array_equal(got["risk"][:, 1:3], 0)
    np.testing.assert_array_equal(got["blame"][:, 0, :, 0], f32(1) / f32(K))
    zero = _call(torch, h, d, 4, Y_t, None, p_t, None, pl_t, None, hz, 0.0, 1.0, 1.0)
    np.testing.assert_array_equal(zero["first"], T)
    np.testing.assert_array_equal(zero["risk"], 0)
    np.testing.assert_array_equal(zero["clear"][:, 3, 1], 0)
    for r, res in ((float(r0), got), (0.0, zero)):
        _same_bits(res, plan_f32(Y, None, present, None, plans, None, hz, r, 1.0, 1.0, d))
    h.close()


def test_results_are_bitwise_reproducible_and_depend_on_the_window_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    for shape in ((4, 8, 3, 7, 5), (4, 256, 2, 40, 3)):                    # the second one walks the frames in chunks
        c = _case(shape, 1, seed=11)
        d, M, hz = c["d"], c["M"], c["hz"]
        ux, uy, radius = c["unit"]
        s = planted_joint_scores(d, 12)
        s[0] = np.nan_to_num(s[0], nan=0.25, posinf=0.5)                   # finite: every window's weights differ over k
        h = _lib.Handle(d)
        hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
        h2 = _lib.Handle(d.replace(n_scenes=2))
        ref = _run(torch, h, c, s)
        assert (ref["first"] < d.T_pred).any() and ref["risk"].max() > 0
        _same_bits(_run(torch, h, c, s), ref)                              # run to run
        _same_bits(_run(torch, hc, c, s), ref)                             # the padding-skipping flags are not its business
        Yw = c["Y"].reshape(d.n_scenes, d.K * d.mno, d.T_pred, 2)

        def sub(hh, rows, plans=None, ego=None, MM=M):
            return _call(torch, hh, hh.dims, MM, _t(torch, Yw[rows]), _t(torch, c["fut"][rows]), None, _t(torch, s[rows]),
                         _t(torch, c["plans"][rows] if plans is None else plans), _t(torch, c["ego"][rows] if ego is None else ego), hz, radius, ux, uy)

        for lo in (0, 2):                                                  # four windows in one call = two calls of two
            _same_bits(sub(h2, slice(lo, lo + 2)), ref, rows=slice(lo, lo + 2))
        perm = np.array([0, 3, 1, 2])                                      # the other windows permuted: every window keeps its results
        _same_bits(sub(h, perm), {k: v[perm] for k, v in ref.items()})
        extra = 30                                                         # M padded by extra plans: another cut into chunks, the same bits
        pc = plan_geometry(d.mno, d.T_pred, M + extra)[0]
        assert pc < M + extra and (pc != plan_geometry(d.mno, d.T_pred, M)[0] or d.mno == 256)
        pl = np.concatenate([c["plans"], np.repeat(c["plans"][:, :1], extra, 1) + np.float32(0.001)], 1)
        eg = np.concatenate([c["ego"], np.full((d.n_scenes, extra), -1, np.int32)], 1)
        wide = sub(h, slice(None), plans=pl, ego=eg, MM=M + extra)
        _same_bits({k: v[:, :M] for k, v in wide.items()}, ref)
        for x in (h, hc, h2):
            x.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[0], (2, 32, 2, 200, 4), (2, 256, 2, 40, 3)], ids=IDS)
def test_buffers_off_16_byte_alignment(torch_cuda, shape, off):
    """The 8-byte path of the streaming loop, for the sample tensor and for the plans: the aligned call's bits."""
    torch = torch_cuda
    from desire_amd import _lib
    c = _case(shape, 1, seed=6)
    d, M, hz = c["d"], c["M"], c["hz"]
    ux, uy, radius = c["unit"]
    s = planted_joint_scores(d, 9)
    h = _lib.Handle(d)
    Y_t, fut_t, s_t, pl_t, ego_t = (_t(torch, x) for x in (c["Y"], c["fut"], s, c["plans"], c["ego"]))
    ref = _call(torch, h, d, M, Y_t, fut_t, None, s_t, pl_t, ego_t, hz, radius, ux, uy)
    np.testing.assert_array_equal(ref["first"], _ref(c, plan_f64, s)["first"])
    for ya, pa in ((True, False), (False, True), (True, True)):
        got = _call(torch, h, d, M, at_byte_offset(Y_t, off) if ya else Y_t, fut_t, None, s_t, at_byte_offset(pl_t, off) if pa else pl_t, ego_t, hz,
                    radius, ux, uy)
        _same_bits(got, ref)
    h.close()


def test_the_present_form_null_ego_and_every_choice_of_optional_outputs(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    c = dict(_case(SHAPES[0], 1))
    d = c["d"]
    fut = c["fut"].copy()
    fut[..., 0] = fut[:, :1, :, 0]                                         # ids constant over t: the two forms count the same frames
    c["fut"] = fut
    s = planted_joint_scores(d, 9)
    h = _lib.Handle(d)
    full = _run(torch, h, c, s)
    assert (full["first"][:, :, :d.K] < d.T_pred).any()
    pres = _run(torch, h, c, s, fut=False)
    _same_bits(pres, _ref(c, plan_f32, s, fut=False), keys=("first", "clear"))
    np.testing.assert_array_equal(pres["first"][:, :, :d.K], full["first"][:, :, :d.K])
    np.testing.assert_array_equal(pres["clear"][:, :, :d.K].view(np.uint32), full["clear"][:, :, :d.K].view(np.uint32))
    _same_bits(pres, full, keys=("risk", "blame"))
    np.testing.assert_array_equal(pres["first"][:, :, d.K], d.T_pred)      # no ground truth: row K says so
    assert np.isposinf(pres["clear"][:, :, d.K]).all()
    free = _run(torch, h, c, None, ego=False)
    _same_bits(free, _ref(c, plan_f32, None, ego=False))
    assert any(not np.array_equal(free[k], _run(torch, h, c, None)[k]) for k in ("first", "blame"))      # the ego slot matters
    for fut_form, ego in itertools.product((True, False), repeat=2):
        whole = _run(torch, h, c, s, fut=fut_form, ego=ego)
        for first, clear, blame in itertools.product((False, True), repeat=3):
            _same_bits(_run(torch, h, c, s, fut=fut_form, ego=ego, first=first, clear=clear, blame=blame), whole)
    h.close()


def test_forward_and_plan_risk_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=4, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    a = make_case(d, seed=21, n_absent=2)
    p, f, e, g = (_t(torch, x) for x in a[:4])
    h = _lib.Handle(d); h.set_weights(w); h.set_scene_grids(g.data_ptr(), a[4])
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    hz, M, radius = [3, 6, 9, 12], 5, 400.0
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    i32 = torch.int32
    first = torch.zeros((d.n_scenes, M, d.K + 1), device="cuda", dtype=i32); clear = torch.zeros((d.n_scenes, M, d.K + 1, 4), device="cuda")
    risk = torch.zeros((d.n_scenes, M, 4), device="cuda"); blame = torch.zeros((d.n_scenes, M, 4, d.mno), device="cuda")
    plans = torch.zeros((d.n_scenes, M, d.T_pred, 2), device="cuda")
    ego = torch.full((d.n_scenes, M), -1, device="cuda", dtype=i32)
    bufs = (Y, sc, first, clear, risk, blame)
    side = torch.cuda.Stream(); sp = side.cuda_stream

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.plan_risk(Y.data_ptr(), f.data_ptr(), 0, sc.data_ptr(), plans.data_ptr(), ego.data_ptr(), M, hz, radius, ux, uy, risk.data_ptr(),
                    first.data_ptr(), clear.data_ptr(), blame.data_ptr(), sp)

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
    assert float(ref["far"][4].abs().max()) == 0 and float(ref["near"][4].max()) > 0 and not torch.equal(ref["near"][2], ref["far"][2])
    want = plan_f32(ref["near"][0].cpu().numpy(), a[1], None, ref["near"][1].cpu().numpy(), sets["near"], np.full((d.n_scenes, M), -1), hz, radius, ux, uy, d)
    np.testing.assert_array_equal(ref["near"][3].cpu().numpy().view(np.uint32), want["clear"].view(np.uint32))
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((1, 4, 3, 6))
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") + 0.5
    pr = torch.ones(64, device="cuda", dtype=torch.uint8)
    eg = torch.full((64,), -1, device="cuda", dtype=torch.int32)
    i32 = torch.int32
    M = 2
    outs = {"first_ptr": torch.full((1, M, d.K + 1), IFILL, device="cuda", dtype=i32), "clear_ptr": torch.full((1, M, d.K + 1, 8), FILL, device="cuda"),
            "risk_ptr": torch.full((1, M, 8), FILL, device="cuda"), "blame_ptr": torch.full((1, M, 8, d.mno), FILL, device="cuda")}
    nan, inf = float("nan"), float("inf")
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(plans_ptr=0), "dev_plans"), (dict(risk_ptr=0), "dev_risk"),
             (dict(horizons=[]), "n_h"), (dict(horizons=list(range(1, 10))), "n_h"), (dict(horizons=[0]), "host_horizons"), (dict(horizons=[7]), "host_horizons"),
             (dict(horizons=[3, 3]), "increasing"), (dict(horizons=[4, 2]), "increasing"),
             (dict(M=0), "M must"), (dict(M=-3), "M must"), (dict(radius=-1e-3), "radius"), (dict(radius=nan), "radius"), (dict(radius=inf), "radius"),
             (dict(unit_x=0.0), "unit_x"), (dict(unit_x=-1.0), "unit_x"), (dict(unit_x=nan), "unit_x"), (dict(unit_x=inf), "unit_x"),
             (dict(unit_y=0.0), "unit_y"), (dict(unit_y=-2.0), "unit_y"), (dict(unit_y=nan), "unit_y"), (dict(unit_y=inf), "unit_y"),
             (dict(present_ptr=pr.data_ptr()), "both"), (dict(fut_ptr=0), "both NULL")]
    for kw, word in cases:
        args = dict(yhat_ptr=z.data_ptr(), fut_ptr=z.data_ptr(), present_ptr=0, score_ptr=z.data_ptr(), plans_ptr=z.data_ptr(), ego_ptr=eg.data_ptr(), M=M,
                    horizons=[2, 6], radius=1.0, unit_x=1.0, unit_y=1.0, **{k: v.data_ptr() for k, v in outs.items()})
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.plan_risk(**args)
    lib = _lib.load()
    one = C.c_float(1)
    hz2 = (C.c_int32 * 2)(2, 6)
    o = {k: v.data_ptr() for k, v in outs.items()}
    tail = (one, one, one, o["first_ptr"], o["clear_ptr"], o["risk_ptr"], o["blame_ptr"], None)
    assert lib.desire_plan_risk(None, z.data_ptr(), z.data_ptr(), None, None, z.data_ptr(), None, M, hz2, 2, *tail) == -1
    assert b"handle" in lib.desire_last_error()
    assert lib.desire_plan_risk(h._h, z.data_ptr(), z.data_ptr(), None, None, z.data_ptr(), None, M, None, 2, *tail) == -1
    assert b"host_horizons" in lib.desire_last_error()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.plan_risk(z.data_ptr(), z.data_ptr(), 0, 0, z.data_ptr(), 0, M, [8], 1.0, 1.0, 1.0, o["risk_ptr"])
    torch.cuda.synchronize()
    assert all(bool((v == (IFILL if v.dtype == i32 else FILL)).all()) for v in outs.values())
    # ... and the handle still works
    h.plan_risk(z.data_ptr(), z.data_ptr(), 0, 0, z.data_ptr(), 0, M, [2, 6], 0.0, 1.0, 1.0, o["risk_ptr"])
    torch.cuda.synchronize()
    risk = outs["risk_ptr"].view(-1)[:M * 2]                               # the call's own layout: two horizons
    assert bool((risk == 0).all()) and bool((outs["first_ptr"] == IFILL).all()) and bool((outs["blame_ptr"] == FILL).all())
    for x in (h, rc):
        x.close()


def test_score_plans_prefers_the_far_plan(torch_cuda):
    torch = torch_cuda
    from desire_amd import evaluate as E
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    a = E.build_parser().parse_args(_FLAGS)
    m = DESIREModel(a, seed=4)
    video = _video()
    past, _ = split_windows([video[i * 10 + 20:i * 10 + 30] for i in range(2)], a.seq_length)
    m.predict(past, seed=3, device_rng=True)
    Y = m.final_output.clone()
    h = m._handle(2, False)
    d = h.dims
    T, K = d.T_pred, d.K
    scale = np.array([d.sx, d.sy], np.float32)
    Yk = Y.cpu().numpy().reshape(2, K, d.mno, T, 2)
    hz = [2, 4, 6]
    plans = np.zeros((2, 3, T, 2), np.float32)
    plans[:, 0] = Yk[:, :, 0].mean(1) / scale                              # through the middle of slot 0's samples
    plans[:, 1] = -5000.0                                                  # far from everybody
    plans[:, 2] = -5000.0
    spread = float(np.abs((Yk[:, :, 0] - Yk[:, :, 0].mean(1, keepdims=True)) / scale).max())
    radius = 2.0 * spread * np.sqrt(2.0) + 1.0                             # every sample of slot 0 lies within it of their mean
    out = m.score_plans(past, plans, radius, horizons=hz, seed=3, device_rng=True)
    assert torch.equal(m.final_output, Y)                                  # the same forward
    assert sorted(out) == ["best", "blame", "clearance", "first", "present", "risk"]
    assert tuple(out["risk"].shape) == (2, 3, 3) and tuple(out["clearance"].shape) == (2, 3, K, 3) and tuple(out["first"].shape) == (2, 3, K)
    assert tuple(out["blame"].shape) == (2, 3, 3, d.mno) and tuple(out["best"].shape) == (2, 3)
    risk = out["risk"].cpu().numpy()
    np.testing.assert_allclose(risk[:, 0], 1.0, atol=1e-6)                 # every joint future is hit from frame 0 on
    assert (risk[:, 1:] == 0).all() and (out["first"][:, 0] == 0).all() and (out["first"][:, 1:] == T).all()
    assert (out["best"] == 1).all()                                        # the far plan, and of the two far ones the lower index
    np.testing.assert_allclose(out["blame"][:, 0, :, 0].cpu().numpy(), 1.0, atol=1e-6)
    pres8 = out["present"].cpu().numpy().reshape(-1).astype(np.uint8)
    ref = plan_f32(Yk.reshape(d.R, T, 2), None, pres8, m.final_states.cpu().numpy(), plans * scale, None, hz, radius, 1.0 / d.sx, 1.0 / d.sy, d)
    np.testing.assert_array_equal(out["first"].cpu().numpy(), ref["first"][:, :, :K])
    replaced = m.score_plans(past, plans, radius, horizons=hz, ego_slot=[0, 0], weights="uniform", seed=3, device_rng=True)
    assert (replaced["blame"][:, :, :, 0] == 0).all()
    with pytest.raises(ValueError, match="collision_radius"):
        m.score_plans(past, plans, -1.0)
    with pytest.raises(ValueError, match="plans"):
        m.score_plans(past, plans[:, :, :3], 1.0)
    with pytest.raises(ValueError, match="weights"):
        m.score_plans(past, plans, 1.0, weights="best")


def test_evaluate_plan_risk_and_the_evaluation_walk(torch_cuda):
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    import json
    video = _video()
    a = E.build_parser().parse_args(_FLAGS)
    m = DESIREModel(a, seed=4)
    past, fut = split_windows([video[i * 10 + 20:i * 10 + 30] for i in range(2)], a.seq_length)
    m.predict(past, seed=3, device_rng=True)
    Y, score = m.final_output.clone(), m.final_states.clone()
    hz = [2, 4, 6]
    none = m.evaluate_plan_risk(Y, score, fut, 0.0, horizons=hz)
    assert sorted(none) == ["actual", "agents", "first", "predicted", "risk", "takes_part"]
    assert not none["predicted"].any() and not none["actual"].any() and (none["agents"] == [9, 9, 9]).all()
    wide = m.evaluate_plan_risk(Y, score, fut, 1e5, horizons=hz)
    np.testing.assert_allclose(wide["predicted"], 1.0, atol=1e-6)
    np.testing.assert_allclose(wide["actual"], 1.0)
    res = {}
    for tag, extra in (("plain", []), ("zero", ["--plan_risk"]), ("wide", ["--plan_risk", "--collision_radius", "100000"])):
        a = E.build_parser().parse_args(_FLAGS + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=DESIREModel(a, seed=4))
    assert list(res["plain"]) == _PLAIN_KEYS                           # without the flag: the result it has always been
    plain_text = json.dumps(res["plain"], indent=1)
    nh = len(res["plain"]["horizons"])
    for tag in ("zero", "wide"):
        blk = res[tag].pop("plan_risk")
        assert json.dumps(res[tag], indent=1) == plain_text            # ... and with it, the same result plus one block
        assert set(blk) == {"collision_radius_px", "agents", "predicted_risk", "actual_rate"}
        assert len(blk["predicted_risk"]) == len(blk["actual_rate"]) == nh and min(blk["agents"]) > 0
        res[tag]["plan_risk"] = blk
    assert all(v == 0.0 for v in res["zero"]["plan_risk"]["predicted_risk"] + res["zero"]["plan_risk"]["actual_rate"])
    assert all(abs(v - 1.0) < 1e-6 for v in res["wide"]["plan_risk"]["predicted_risk"] + res["wide"]["plan_risk"]["actual_rate"])
