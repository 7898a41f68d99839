"""Distinct joint futures on the device (desire_select_worlds, csrc/kernels_worlds.hip) against the numpy statements of its contract
(tests/worlds_reference.py).  Order, count and label are compared exactly with both statements -- on inputs whose every compared value keeps,
in float64, a margin of 1e-3 radius from the radius, asserted first on the float64 pass alone.  The mass follows tests/test_gpu_select.py's rule:
against worlds_f64, the bar four times the distance of worlds_f32 from worlds_f64 on the same inputs (the 4 x covers the device's expf against
numpy's), never below 1e-5; bit for bit where no expf enters (NULL scores).  Then the anchors to desire_select_diverse and desire_joint_metrics,
the exact boundary, the limiting cases, run to run, batch split, permutation, garbage in absent slots, padding flags, capture, refused arguments,
and the call through DESIREModel and the evaluation command line.

Observed on an MI355X (the parity test over every shape, both units): max |mass - f64| = 1.5e-7 with scores, bar 1e-5."""
import ctypes as C
import json

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import EVAL_FLAGS as _FLAGS, PLAIN_KEYS as _PLAIN_KEYS, walking_video as _video, MISALIGNED_SHAPES, at_byte_offset, make_case, small_dims
from tests.joint_reference import make_inputs as joint_inputs, planted_joint_scores
from tests.rank_reference import planted_scores
from tests.select_reference import DIST_FINAL, DIST_MAX, DIST_MEAN, METRICS, make_inputs as select_inputs
from tests.worlds_reference import (MARGIN, RADIUS_PX, REDUCES, SHAPES, WORLD_ALL, WORLD_MEAN, cases_of, make_inputs, planted_world_scores,
                                    world_weights, worlds_f32, worlds_f64)

pytestmark = pytest.mark.gpu
FILL, IFILL = -7.0, -77
# tests/worlds_reference.py's shapes -- K = 70 at 8 slots, not 5: a handle's mno divides 32 or is a multiple of it --, long rows, and 256 slots
# (two slot chunks of 128 under MEAN / MAX at 40 frames)
ALL_SHAPES = [(2, 8, 70, 6) if s == (2, 5, 70, 6) else s for s in SHAPES] + [(2, 32, 3, 200), (2, 256, 2, 40)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _t(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _dims(shape, **kw):
    n, m, K, T = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64, **kw)


def _units(d):
    return [(1.0, 1.0, float(np.float32(RADIUS_PX * d.sx))), (1.0 / d.sx, 1.0 / d.sy, RADIUS_PX)]      # (unit_x, unit_y, the radius in that unit)


def _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, t_end, radius, ux, uy, mass=True, label=True, stream=0):
    n = d.n_scenes
    out = {"order": torch.full((n, d.K), IFILL, device="cuda", dtype=torch.int32), "count": torch.full((n,), IFILL, device="cuda", dtype=torch.int32),
           "mass": torch.full((n, d.K), FILL, device="cuda") if mass else None,
           "label": torch.full((n, d.K), IFILL, device="cuda", dtype=torch.int32) if label else None}
    ptr = lambda x: x.data_ptr() if x is not None else 0
    h.select_worlds(Y_t.data_ptr(), ptr(pres_t), ptr(ws_t), metric, reduce, t_end, radius, ux, uy, out["order"].data_ptr(), out["count"].data_ptr(),
                    ptr(out["mass"]), ptr(out["label"]), stream)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _same(a, b, rows=slice(None)):
    for key in ("order", "count", "mass", "label"):
        np.testing.assert_array_equal(a[key].view(np.uint32), b[key][rows].view(np.uint32), err_msg=key)


def _check(torch, h, d, Y, Y_t, present, pres_t, ws, ws_t, metric, reduce, t_end, radius, ux, uy):
    """One (metric, reduce, t_end) of the parity: the margin on the float64 pass, the statements' agreement, then the device."""
    f64 = worlds_f64(Y, present, ws, metric, reduce, t_end, radius, ux, uy, d)
    assert f64["margin"] > MARGIN, (metric, reduce, t_end, f64["margin"])
    f32 = worlds_f32(Y, present, ws, metric, reduce, t_end, radius, ux, uy, d)
    got = _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, t_end, radius, ux, uy)
    for key in ("order", "count", "label"):
        np.testing.assert_array_equal(f32[key], f64[key], err_msg=key)
        np.testing.assert_array_equal(got[key], f32[key], err_msg="%s %s" % (key, (metric, reduce, t_end)))
    basis = float(np.abs(f32["mass"].astype(np.float64) - f64["mass"]).max())
    bar = max(4.0 * basis, 1e-5)
    err = float(np.abs(got["mass"].astype(np.float64) - f64["mass"]).max())
    print("metric %d reduce %d t_end %d: kept %.2f per window, max |mass - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g"
          % (metric, reduce, t_end, f32["count"].mean(), err, basis, bar))
    assert err <= bar
    assert (got["mass"][np.arange(d.K)[None] >= got["count"][:, None]] == 0).all()
    return got, f32, err


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_order_count_label_and_mass_match_the_reference(torch_cuda, shape, unit):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims(shape)
    ux, uy, radius = _units(d)[unit]
    Y, present, info = make_inputs(d, radius, ux, uy, seed=41 + unit)
    ws = planted_world_scores(d, 9)
    h = _lib.Handle(d)
    Y_t, pres_t, ws_t = _t(torch, Y), _t(torch, present), _t(torch, ws)
    worst = 0.0
    for metric, reduce, t_end in cases_of(d):
        got, f32, err = _check(torch, h, d, Y, Y_t, present, pres_t, ws, ws_t, metric, reduce, t_end, radius, ux, uy)
        worst = max(worst, err)
        w, k, _ = info["nan"]
        assert k in got["order"][w, :got["count"][w]]                          # the world with a NaN row is near nothing: kept
        if d.n_scenes >= 2:
            assert got["count"][-1] == 1                                        # nobody present: everything is near the first
        # NULL scores: the identity order, equal weights, no expf -- bit for bit; the optional outputs left out change nothing
        flat = worlds_f32(Y, present, None, metric, reduce, t_end, radius, ux, uy, d)
        eq = _call(torch, h, d, Y_t, pres_t, None, metric, reduce, t_end, radius, ux, uy)
        for key in ("order", "count", "label"):
            np.testing.assert_array_equal(eq[key], flat[key], err_msg=key)
        np.testing.assert_array_equal(eq["mass"].view(np.uint32), flat["mass"].view(np.uint32))
        bare = _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, t_end, radius, ux, uy, mass=False, label=False)
        np.testing.assert_array_equal(bare["order"], f32["order"]); np.testing.assert_array_equal(bare["count"], f32["count"])
    print("worst |mass - f64| of the shape: %.3g" % worst)
    h.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_a_sample_tensor_off_16_byte_alignment(torch_cuda, shape, off):
    """The 4-byte loads of a whole buffer: the reference as in the parity test, and the aligned call's bits."""
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims(shape)
    ux, uy, radius = _units(d)[1]
    Y, present, _ = make_inputs(d, radius, ux, uy, seed=43)
    ws = planted_world_scores(d, 9)
    h = _lib.Handle(d)
    Y_t, pres_t, ws_t = _t(torch, Y), _t(torch, present), _t(torch, ws)
    Y_off = at_byte_offset(Y_t, off)
    for metric, reduce in ((DIST_MEAN, WORLD_MEAN), (DIST_FINAL, WORLD_ALL), (DIST_MAX, WORLD_ALL)):
        got, _, _ = _check(torch, h, d, Y, Y_off, present, pres_t, ws, ws_t, metric, reduce, d.T_pred, radius, ux, uy)
        _same(got, _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, d.T_pred, radius, ux, uy))
    h.close()


def test_one_slot_is_desire_select_diverse_bit_for_bit(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((3, 1, 3, 7))
    ux, uy, radius = _units(d)[1]
    Y, _ = select_inputs(d, radius, ux, uy, seed=31, absent=False)
    s = planted_scores(d, 9)                                                   # [n, K, mno = 1]: the world scores of a one-slot window
    h = _lib.Handle(d)
    Y_t, s_t = _t(torch, Y), _t(torch, s)
    ones = torch.ones((d.A,), device="cuda", dtype=torch.uint8)
    order = torch.empty((d.A, d.K), device="cuda", dtype=torch.int32)
    h.rank_samples(s_t.data_ptr(), 0, 1, order.data_ptr(), 0, 0)
    for metric in METRICS:
        for t_end in (1, 4, d.T_pred):
            div, cnt = torch.full((d.A, d.K), IFILL, device="cuda", dtype=torch.int32), torch.full((d.A,), IFILL, device="cuda", dtype=torch.int32)
            mass = torch.full((d.A, d.K), FILL, device="cuda")
            h.select_diverse(Y_t.data_ptr(), order.data_ptr(), s_t.data_ptr(), metric, t_end, radius, ux, uy, 1, div.data_ptr(), cnt.data_ptr(),
                             mass.data_ptr(), 0, 0)
            for pres in (ones, None):
                got = _call(torch, h, d, Y_t, pres, s_t, metric, WORLD_ALL, t_end, radius, ux, uy)
                np.testing.assert_array_equal(got["order"], div.cpu().numpy())
                np.testing.assert_array_equal(got["count"], cnt.cpu().numpy())
                np.testing.assert_array_equal(got["mass"].view(np.uint32), mass.cpu().numpy().view(np.uint32))
    h.close()


def test_radius_zero_is_desire_joint_metrics_order(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((2, 8, 5, 12))
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    Y, fut, present, _ = joint_inputs(d, RADIUS_PX, ux, uy, seed=3)
    s = planted_joint_scores(d, 4)
    h = _lib.Handle(d)
    Y_t, pres_t, s_t = _t(torch, Y), _t(torch, present), _t(torch, s)
    cnt = torch.empty((d.n_scenes, d.K + 1, 1, 2), device="cuda", dtype=torch.int32)
    js, jo = torch.empty((d.n_scenes, d.K), device="cuda"), torch.empty((d.n_scenes, d.K), device="cuda", dtype=torch.int32)
    h.joint_metrics(Y_t.data_ptr(), 0, pres_t.data_ptr(), s_t.data_ptr(), [d.T_pred], 1, 0.0, ux, uy, cnt.data_ptr(), jo.data_ptr(), 0, 0, js.data_ptr(), 0)
    for metric in METRICS:
        for reduce in REDUCES:
            got = _call(torch, h, d, Y_t, pres_t, js, metric, reduce, d.T_pred, 0.0, ux, uy)
            np.testing.assert_array_equal(got["order"], jo.cpu().numpy())
            np.testing.assert_array_equal(got["count"], d.K)
            np.testing.assert_array_equal(got["label"], np.argsort(jo.cpu().numpy(), 1))
    h.close()


def test_the_boundary_is_exact(torch_cuda):
    """Coordinates on multiples of 1/8, world 1 = world 0 + (3/8, 4/8) in every taking-part slot and frame: q = 25/64, sqrt(q) = 5/8, their sums
    over 6 frames and 3 slots and the means exactly.  radius = 0.625f: the strict comparison does not suppress; the next float up does.  The
    absent slot holds world 1 far away."""
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((2, 4, 4, 6))
    rng = np.random.default_rng(3)
    Yk = np.zeros((d.n_scenes, d.K, d.mno, d.T_pred, 2), np.float32)
    Yk[:] = rng.integers(8, 24, (d.n_scenes, 1, d.mno, d.T_pred, 2)).astype(np.float32) / 8
    Yk[:, 1] += np.array([3 / 8, 4 / 8], np.float32)            # the partner of world 0
    Yk[:, 2] += np.array([40 / 8, 0], np.float32)               # far from both
    Yk[:, 3] += np.array([40 / 8 + 4 / 8, 3 / 8], np.float32)   # the partner of world 2
    present = np.ones((d.n_scenes, d.mno), np.uint8)
    present[:, 2] = 0
    Yk[:, :, 2] = rng.integers(-800, 800, (d.n_scenes, d.K, d.T_pred, 2)).astype(np.float32)
    Y = np.ascontiguousarray(Yk.reshape(d.R, d.T_pred, 2))
    ws = np.array([[4, 3, 2, 1], [1, 2, 3, 4]], np.float32)
    h = _lib.Handle(d)
    Y_t, pres_t, ws_t = _t(torch, Y), _t(torch, present.reshape(-1)), _t(torch, ws)
    r0 = np.float32(0.625)
    r1 = np.nextafter(r0, np.float32(1))
    assert r0 * r0 == np.float32(25 / 64) and r1 > r0
    for metric in METRICS:
        for reduce in REDUCES:
            for t_end in (1, d.T_pred):
                at = _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, t_end, float(r0), 1.0, 1.0)
                np.testing.assert_array_equal(at["count"], d.K)
                np.testing.assert_array_equal(at["order"], [[0, 1, 2, 3], [3, 2, 1, 0]])
                up = _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, t_end, float(r1), 1.0, 1.0)
                np.testing.assert_array_equal(up["count"], 2)
                np.testing.assert_array_equal(up["order"], [[0, 2, 1, 3], [3, 1, 2, 0]])
                np.testing.assert_array_equal(up["label"], [[0, 0, 1, 1], [1, 1, 0, 0]])
                for got, r in ((at, r0), (up, r1)):
                    ref = worlds_f32(Y, present, ws, metric, reduce, t_end, float(r), 1.0, 1.0, d)
                    np.testing.assert_array_equal(got["order"], ref["order"])
    h.close()


def test_limiting_cases(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((2, 8, 5, 12))
    ux, uy, radius = _units(d)[1]
    Y, present, info = make_inputs(d, radius, ux, uy, seed=2)
    ws = planted_world_scores(d, 4)
    ws[0, 4] = 0.5                                                          # (finite scores: the masses below are softmax's)
    h = _lib.Handle(d)
    Y_t, pres_t, ws_t = _t(torch, Y), _t(torch, present), _t(torch, ws)
    proc = worlds_f32(Y, present, ws, DIST_FINAL, WORLD_ALL, 1, 0.0, ux, uy, d)["processing"]
    w64 = np.take_along_axis(world_weights(ws, d.n_scenes, d.K, np.float64), proc.astype(np.int64), 1)
    w32u = world_weights(None, d.n_scenes, d.K, np.float32)
    ident = np.broadcast_to(np.arange(d.K, dtype=np.int32), (d.n_scenes, d.K))
    all_ones = torch.ones((d.A,), device="cuda", dtype=torch.uint8)
    for metric in METRICS:
        for reduce in REDUCES:
            for t_end in (1, 7, d.T_pred):
                z = _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, t_end, 0.0, ux, uy)        # radius 0: the processing order, the mass is W
                np.testing.assert_array_equal(z["order"], proc); np.testing.assert_array_equal(z["count"], d.K)
                np.testing.assert_array_equal(np.take_along_axis(z["label"], proc.astype(np.int64), 1), ident)
                assert float(np.abs(z["mass"].astype(np.float64) - w64).max()) <= 1e-5
                z0 = _call(torch, h, d, Y_t, pres_t, None, metric, reduce, t_end, 0.0, ux, uy)         # NULL scores: the identity, 1 / K
                np.testing.assert_array_equal(z0["order"], ident)
                np.testing.assert_array_equal(z0["mass"].view(np.uint32), w32u.view(np.uint32))
                big = _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, t_end, 1e30, ux, uy)
                w_nan = info["nan"][0]
                for w in range(d.n_scenes):
                    if w == w_nan:                                              # everything is near the first, but the world with a NaN row: kept too
                        assert big["count"][w] == 2
                    else:
                        assert big["count"][w] == 1 and (big["order"][w] == proc[w]).all() and (big["label"][w] == 0).all()
                        np.testing.assert_allclose(big["mass"][w, 0], 1.0, rtol=0, atol=1e-5)
                tiny = _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, t_end, 1e-15, ux, uy)     # the empty window: any radius > 0
                assert tiny["count"][-1] == 1 and (tiny["order"][-1] == proc[-1]).all()
                # NULL dev_present is all ones
                _same(_call(torch, h, d, Y_t, None, ws_t, metric, reduce, t_end, radius, ux, uy),
                      _call(torch, h, d, Y_t, all_ones, ws_t, metric, reduce, t_end, radius, ux, uy))
    h.close()


def test_results_are_bitwise_reproducible_and_depend_on_the_window_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((4, 8, 5, 12))
    ux, uy, radius = _units(d)[1]
    Y, present, _ = make_inputs(d, radius, ux, uy, seed=11)
    ws = planted_world_scores(d, 12)
    h = _lib.Handle(d)
    hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
    h2 = _lib.Handle(d.replace(n_scenes=2))
    d2 = h2.dims
    Y_t, pres_t, ws_t = _t(torch, Y), _t(torch, present), _t(torch, ws)
    Yw, pw = Y.reshape(d.n_scenes, d.K * d.mno, d.T_pred, 2), present.reshape(d.n_scenes, d.mno)
    perm = np.array([2, 0, 3, 1])
    Yg = Y.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).copy()
    Yg[:, :, :][np.broadcast_to((pw == 0)[:, None, :], Yg.shape[:3])] = 12345.0      # other garbage in the slots that do not take part
    for metric in METRICS:
        for reduce in REDUCES:
            ref = _call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, d.T_pred, radius, ux, uy)
            assert (ref["count"] > 1).any() and (ref["count"] < d.K).any()
            _same(_call(torch, h, d, Y_t, pres_t, ws_t, metric, reduce, d.T_pred, radius, ux, uy), ref)          # run to run
            _same(_call(torch, hc, d, Y_t, pres_t, ws_t, metric, reduce, d.T_pred, radius, ux, uy), ref)         # the padding-skipping flags
            _same(_call(torch, h, d, _t(torch, Yg.reshape(Y.shape)), pres_t, ws_t, metric, reduce, d.T_pred, radius, ux, uy), ref)
            for w0 in (0, 2):                                                                                      # four windows = two calls of two
                half = _call(torch, h2, d2, _t(torch, Yw[w0:w0 + 2]), _t(torch, pw[w0:w0 + 2]), _t(torch, ws[w0:w0 + 2]), metric, reduce, d.T_pred,
                             radius, ux, uy)
                _same(half, ref, slice(w0, w0 + 2))
            mixed = _call(torch, h, d, _t(torch, Yw[perm]), _t(torch, pw[perm]), _t(torch, ws[perm]), metric, reduce, d.T_pred, radius, ux, uy)
            _same(mixed, ref, perm)                                                                                # permuted windows
    for x in (h, hc, h2):
        x.close()


def test_forward_joint_metrics_and_select_worlds_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=4, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    a, b = make_case(d, seed=21, n_absent=2), make_case(d, seed=22, n_absent=3)
    p, f, e, g = (_t(torch, x) for x in a[:4])
    h = _lib.Handle(d); h.set_weights(w); h.set_scene_grids(g.data_ptr(), a[4])
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    i32 = torch.int32
    pres = torch.zeros((d.A,), device="cuda", dtype=torch.uint8)
    cnt = torch.zeros((d.n_scenes, d.K + 1, 1, 2), device="cuda", dtype=i32)
    js = torch.zeros((d.n_scenes, d.K), device="cuda"); jo = torch.zeros((d.n_scenes, d.K), device="cuda", dtype=i32)
    wo, wl = torch.zeros_like(jo), torch.zeros_like(jo)
    wc = torch.zeros((d.n_scenes,), device="cuda", dtype=i32); wm = torch.zeros((d.n_scenes, d.K), device="cuda")
    bufs = (Y, sc, cnt, js, jo, wo, wc, wm, wl)
    side = torch.cuda.Stream(); sp = side.cuda_stream
    ux, uy = 1.0 / d.sx, 1.0 / d.sy

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.joint_metrics(Y.data_ptr(), 0, pres.data_ptr(), sc.data_ptr(), [d.T_pred], 1, 400.0, ux, uy, cnt.data_ptr(), jo.data_ptr(), 0, 0, js.data_ptr(), 0, sp)
        h.select_worlds(Y.data_ptr(), pres.data_ptr(), js.data_ptr(), DIST_MEAN, WORLD_MEAN, d.T_pred, 1e-3, ux, uy, wo.data_ptr(), wc.data_ptr(),
                        wm.data_ptr(), wl.data_ptr(), sp)

    def load(case):
        p.copy_(_t(torch, case[0])); f.copy_(_t(torch, case[1])); e.copy_(_t(torch, case[2]))      # in place: the graph keeps its pointers
        pres.copy_((p[:, -1, :, 0] != 0).reshape(-1).to(torch.uint8))

    torch.cuda.synchronize()
    ref = {}
    for tag, case in (("b", b), ("a", a)):                        # eager calls (the first also warms lazy allocations up outside capture)
        load(case)
        torch.cuda.synchronize()
        calls()
        side.synchronize()
        ref[tag] = [x.clone() for x in bufs]
    h.graph_begin(sp)
    calls()
    gid = h.graph_end(sp)
    for rep in range(4):
        tag, case = ("b", b) if rep % 2 == 0 else ("a", a)
        load(case)
        for x in bufs:
            x.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        for x, r in zip(bufs, ref[tag]):
            assert torch.equal(x.view(i32), r.view(i32)), (rep, tag)
    assert not torch.equal(ref["a"][0], ref["b"][0])
    for tag in ("a", "b"):
        assert (np.sort(ref[tag][5].cpu().numpy(), 1) == np.arange(d.K)).all() and bool((ref[tag][6] >= 1).all())
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((1, 4, 3, 6))
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") + 0.5
    p8 = torch.ones(64, device="cuda", dtype=torch.uint8)
    outs = {"worder_ptr": torch.full((1, d.K), IFILL, device="cuda", dtype=torch.int32), "wcount_ptr": torch.full((1,), IFILL, device="cuda", dtype=torch.int32),
            "wmass_ptr": torch.full((1, d.K), FILL, device="cuda"), "wlabel_ptr": torch.full((1, d.K), IFILL, device="cuda", dtype=torch.int32)}
    nan, inf = float("nan"), float("inf")
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(worder_ptr=0), "dev_worder"), (dict(wcount_ptr=0), "dev_wcount"),
             (dict(metric=-1), "metric"), (dict(metric=3), "metric"), (dict(reduce=-1), "reduce"), (dict(reduce=2), "reduce"),
             (dict(t_end=0), "t_end"), (dict(t_end=7), "t_end"), (dict(t_end=-1), "t_end"),
             (dict(radius=-1e-3), "radius"), (dict(radius=nan), "radius"), (dict(radius=inf), "radius"),
             (dict(unit_x=0.0), "unit_x"), (dict(unit_x=-1.0), "unit_x"), (dict(unit_x=nan), "unit_x"), (dict(unit_x=inf), "unit_x"),
             (dict(unit_y=0.0), "unit_y"), (dict(unit_y=-2.0), "unit_y"), (dict(unit_y=nan), "unit_y"), (dict(unit_y=inf), "unit_y")]
    for kw, word in cases:
        args = dict(yhat_ptr=z.data_ptr(), present_ptr=p8.data_ptr(), wscore_ptr=z.data_ptr(), metric=DIST_MEAN, reduce=WORLD_MEAN, t_end=6, radius=1.0,
                    unit_x=1.0, unit_y=1.0, **{k: v.data_ptr() for k, v in outs.items()})
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.select_worlds(**args)
    lib = _lib.load()
    one = C.c_float(1)
    assert lib.desire_select_worlds(None, z.data_ptr(), None, None, 0, 0, 1, one, one, one, outs["worder_ptr"].data_ptr(), outs["wcount_ptr"].data_ptr(),
                                    None, None, None) == -1
    assert b"handle" in lib.desire_last_error()
    # the LDS plan: 44 K + 4 mno + 8 (F | 1) <= 61440 -- K = 1400 is beyond it even at one frame, K = 1300 fits
    big = _lib.Handle(_dims((1, 4, 1400, 6)))
    ob, cb = torch.full((1, 1400), IFILL, device="cuda", dtype=torch.int32), torch.full((1,), IFILL, device="cuda", dtype=torch.int32)
    Yb = torch.zeros((4 * 1400, 6, 2), device="cuda")
    for metric in METRICS:
        with pytest.raises(_lib.DesireError, match="error -1.*LDS"):
            big.select_worlds(Yb.data_ptr(), 0, 0, metric, WORLD_ALL, 6, 1.0, 1.0, 1.0, ob.data_ptr(), cb.data_ptr())
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.select_worlds(z.data_ptr(), 0, 0, 0, 0, 8, 1.0, 1.0, 1.0, outs["worder_ptr"].data_ptr(), outs["wcount_ptr"].data_ptr())
    torch.cuda.synchronize()
    assert all(bool((v == (IFILL if v.dtype == torch.int32 else FILL)).all()) for v in outs.values())
    assert bool((ob == IFILL).all()) and bool((cb == IFILL).all())
    # ... and the handles still work: a large K that fits (coincident zero rows: one world kept), and radius 0 on the small one
    fit = _lib.Handle(_dims((1, 4, 1300, 6)))
    of, cf = torch.full((1, 1300), IFILL, device="cuda", dtype=torch.int32), torch.full((1,), IFILL, device="cuda", dtype=torch.int32)
    fit.select_worlds(Yb.data_ptr(), 0, 0, DIST_MAX, WORLD_MEAN, 6, 1.0, 1.0, 1.0, of.data_ptr(), cf.data_ptr())
    torch.cuda.synchronize()
    assert int(cf[0]) == 1 and torch.equal(of[0], torch.arange(1300, device="cuda", dtype=torch.int32))
    h.select_worlds(z.data_ptr(), 0, 0, DIST_MAX, WORLD_ALL, 6, 0.0, 1.0, 1.0, outs["worder_ptr"].data_ptr(), outs["wcount_ptr"].data_ptr())
    torch.cuda.synchronize()
    assert int(outs["wcount_ptr"][0]) == d.K and outs["worder_ptr"][0].tolist() == [0, 1, 2] and bool((outs["wmass_ptr"] == FILL).all())
    for x in (h, big, rc, fit):
        x.close()


def _radius_with_a_margin(Yn, present, metric, reduce, t_end, ux, uy, d):
    """A radius in the widest gap of the sorted world distances (D of WORLD_MEAN, float64) of samples the test did not lay out."""
    from tests.select_reference import pair_values
    v = pair_values(Yn, metric, t_end, ux, uy, d, np.float64).reshape(d.n_scenes, d.mno, d.K, d.K)
    di = v if metric == DIST_MEAN else np.sqrt(v)
    part = present.reshape(d.n_scenes, d.mno).astype(bool)
    D = np.stack([di[w][part[w]].mean(0) for w in range(d.n_scenes)])
    dist = np.sort(D[:, np.triu(np.ones((d.K, d.K), bool), 1)].reshape(-1))
    dist = dist[dist > 0]
    i = int(np.argmax(np.diff(dist) / dist[1:]))
    return float(np.float32(0.5 * (dist[i] + dist[i + 1])))


def test_predict_and_evaluate_joint_select_distinct_worlds(torch_cuda):
    torch = torch_cuda
    from desire_amd import evaluate as E
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    a = E.build_parser().parse_args(_FLAGS)
    m = DESIREModel(a, seed=4)
    video = _video()
    wins = [video[i * 10 + 20:i * 10 + 30] for i in range(2)]
    past, fut = split_windows(wins, a.seq_length)
    top = 3
    joint = m.predict(past, top=top, seed=3, device_rng=True, select="joint")
    Y, score = m.final_output.clone(), m.final_states.clone()
    h = m._handle(2, False)
    d = h.dims
    Yn = Y.cpu().numpy().reshape(d.R, d.T_pred, 2)
    present = joint["present"].cpu().numpy()
    pr8 = present.reshape(-1).astype(np.uint8)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    radius = _radius_with_a_margin(Yn, pr8, DIST_FINAL, WORLD_MEAN, d.T_pred, ux, uy, d)
    out = m.predict(past, top=top, seed=3, device_rng=True, select="worlds", worlds_radius=radius)
    assert sorted(out) == ["collisions", "count", "joint_score", "order", "present", "prob", "score", "traj"]
    assert torch.equal(m.final_output, Y) and torch.equal(m.final_states, score)
    order = out["order"].cpu().numpy()
    assert (order == order[:, :1]).all()                                        # the same world index for every slot of a window
    assert all(len(set(order[w, 0, :top].tolist())) == top for w in range(2))   # `top` distinct worlds
    assert tuple(out["count"].shape) == (2,) and out["count"].dtype == torch.int32 and tuple(out["prob"].shape) == (2, top)
    assert float(out["prob"].sum(-1).max()) <= 1 + 1e-5 and float(out["prob"].min()) >= 0
    # penalty 0 is the unpenalised order: the reference on the joint scores of the select="joint" call
    js = torch.empty((2, d.K), device="cuda"); jo = torch.empty((2, d.K), device="cuda", dtype=torch.int32)
    cnt = torch.empty((2, d.K + 1, 1, 2), device="cuda", dtype=torch.int32)
    p8 = _t(torch, pr8)
    h.joint_metrics(Y.data_ptr(), 0, p8.data_ptr(), score.data_ptr(), [d.T_pred], top, 0.0, ux, uy, cnt.data_ptr(), jo.data_ptr(), 0, 0, js.data_ptr(), 0)
    f64 = worlds_f64(Yn, pr8, js.cpu().numpy(), DIST_FINAL, WORLD_MEAN, d.T_pred, radius, ux, uy, d)
    assert f64["margin"] > MARGIN
    ref = worlds_f32(Yn, pr8, js.cpu().numpy(), DIST_FINAL, WORLD_MEAN, d.T_pred, radius, ux, uy, d)
    np.testing.assert_array_equal(order[:, 0], ref["order"])
    np.testing.assert_array_equal(out["count"].cpu().numpy(), ref["count"])
    zero = m.predict(past, top=top, seed=3, device_rng=True, select="worlds", worlds_radius=radius, collision_penalty=0.0, collision_radius=1e6)
    assert torch.equal(zero["order"], out["order"])
    scale = torch.tensor([d.sx, d.sy], device="cuda", dtype=torch.float32)
    idx = torch.as_tensor(ref["order"][:, :top].astype(np.int64), device="cuda")
    want = Y.reshape(2, d.K, d.mno, d.T_pred, 2)[torch.arange(2, device="cuda")[:, None], idx].permute(0, 2, 1, 3, 4) / scale
    assert torch.equal(out["traj"], want)
    # ---- a planted colliding world: sample k_hit runs two present agents through each other and has the best joint score; a penalty moves it
    # behind the clean ones
    k_best = int(jo[0, 0])
    slots = np.nonzero(present[0])[0]
    Yp = Y.clone().reshape(2, d.K, d.mno, d.T_pred, 2)
    Yp[0, k_best, slots[1]] = Yp[0, k_best, slots[0]]
    Yp = Yp.reshape(Y.shape).contiguous()
    wargs0 = m._worlds_args("worlds", 0.0, "final", "mean", None, 0.0, d.T_pred)
    wargsP = m._worlds_args("worlds", 0.0, "final", "mean", None, 1e6, d.T_pred)
    h.joint_metrics(Yp.data_ptr(), 0, p8.data_ptr(), score.data_ptr(), [d.T_pred], top, 1.0, ux, uy, cnt.data_ptr(), jo.data_ptr(), 0, 0, js.data_ptr(), 0)
    hit = cnt[:, :d.K, 0, 0]
    assert int(hit[0, k_best]) == 2 and int(hit[0].sum()) == 2
    o0 = m._select_worlds(h, Yp, p8, js, hit, wargs0, 0.0, ux, uy)[0].cpu().numpy()
    oP = m._select_worlds(h, Yp, p8, js, hit, wargsP, 0.0, ux, uy)[0].cpu().numpy()
    assert o0[0, 0] == k_best and oP[0, -1] == k_best and (oP[0, :-1] == o0[0, 1:]).all() and (oP[1] == o0[1]).all()
    # ---- evaluate_joint(select="worlds")
    hz = [2, 4, 6]
    base = m.evaluate_joint(Y, score, fut, top=top, horizons=hz, units="px")
    assert sorted(base) == ["cnt", "first", "jerr", "jscore", "order", "out"]
    ev = m.evaluate_joint(Y, score, fut, top=top, horizons=hz, units="px", select="worlds", worlds_radius=radius, worlds_reduce="mean")
    assert sorted(ev) == sorted(list(base) + ["out_distinct", "wcount", "wlabel", "worder", "wprob"])
    for key in base:
        np.testing.assert_array_equal(ev[key].view(np.uint32), base[key].view(np.uint32), err_msg=key)
    assert tuple(ev["out_distinct"].shape) == (2, len(hz), 2) and (np.sort(ev["worder"], 1) == np.arange(d.K)).all()
    pick = ev["jerr"][np.arange(2)[:, None], ev["worder"][:, :top].astype(np.int64)]
    np.testing.assert_array_equal(ev["out_distinct"].view(np.uint32), pick.min(1).view(np.uint32))
    np.testing.assert_array_equal(ev["wlabel"][np.arange(2)[:, None], ev["worder"].astype(np.int64)][:, 0], 0)
    assert (ev["wcount"] >= 1).all() and float(ev["wprob"].sum(1).max()) <= 1 + 1e-5
    for kw, word in ((dict(worlds_radius=5.0), "select='worlds'"), (dict(collision_penalty=1.0), "select='worlds'"),
                     (dict(select="worlds"), "worlds_radius"), (dict(select="worlds", worlds_radius=5.0, worlds_metric="median"), "worlds_metric"),
                     (dict(select="worlds", worlds_radius=5.0, worlds_reduce="any"), "worlds_reduce"),
                     (dict(select="worlds", worlds_radius=5.0, worlds_horizon=7), "worlds_horizon"), (dict(select="joint", worlds_reduce="all"), "select='worlds'")):
        with pytest.raises(ValueError, match=word):
            m.predict(past, **kw)


def test_the_evaluation_walk_reports_the_distinct_worlds(torch_cuda):
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    video = _video()
    res = {}
    for tag, extra in (("plain", ["--joint"]), ("nms", ["--joint", "--joint_select", "nms", "--joint_radius", "6", "--joint_metric", "mean", "--joint_reduce", "all",
                                                       "--joint_horizon", "4", "--collision_penalty", "0.5", "--collision_radius", "3"]),
                       ("wide", ["--joint", "--joint_select", "nms", "--joint_radius", "100000"]), ("zero", ["--joint", "--joint_select", "nms", "--joint_radius", "0"])):
        a = E.build_parser().parse_args(_FLAGS + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=DESIREModel(a, seed=4))
    assert set(res["plain"]["joint"]) == {"collision_radius_px", "windows", "top1", "best_of_top", "collision_rate", "slots"}      # unchanged without the flag
    plain_text = json.dumps(res["plain"], indent=1)
    K = res["plain"]["K"]
    for tag in ("wide", "zero"):
        blk = res[tag]["joint"].pop("select")
        assert json.dumps(res[tag], indent=1) == plain_text                     # with it: the same result plus one entry of the joint block
        assert set(blk) == {"mode", "radius_px", "metric", "reduce", "horizon", "collision_penalty", "mean_count", "best_of_top_distinct"}
        assert (blk["mode"], blk["metric"], blk["reduce"], blk["horizon"], blk["collision_penalty"]) == ("nms", "final", "mean", 6, 0.0)
        assert blk["mean_count"] == (1.0 if tag == "wide" else float(K))
        assert blk["best_of_top_distinct"] == res["plain"]["joint"]["best_of_top"]      # nothing suppressed, or everything: the order by joint score
    blk = res["nms"]["joint"]["select"]
    assert (blk["metric"], blk["reduce"], blk["horizon"], blk["radius_px"], blk["collision_penalty"]) == ("mean", "all", 4, 6.0, 0.5)
    assert 1.0 <= blk["mean_count"] <= K and np.isfinite(blk["best_of_top_distinct"]["jade"] + blk["best_of_top_distinct"]["jfde"]).all()
    a = E.build_parser().parse_args(_FLAGS + ["--joint", "--joint_select", "nms"])
    with pytest.raises(ValueError, match="joint_radius"):
        E.evaluate(a, data_loader=DataLoader(2, 10, 8, a.leave_dataset, frames=[video]), model=DESIREModel(a, seed=4))
