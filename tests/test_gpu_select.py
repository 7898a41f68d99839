"""Score-ordered non-maximum suppression on the device (desire_select_diverse, csrc/kernels_select.hip) against the numpy statement of its
contract (tests/select_reference.py).  Order and count are compared exactly with select_f32 -- on inputs whose every pair keeps, in float64, a
margin of 1e-3 radius from the radius, asserted first on the float64 pass alone.  The mass follows tests/test_gpu_kde.py's rule: against
select_f64, the bar four times the distance of select_f32 from select_f64 on the same inputs (the 4 x covers the device's expf against numpy's),
never below 1e-5; bit for bit where no expf enters (NULL scores).  Then the exact properties: the boundary, the limiting cases, run to run, batch
split, padding flags, capture, refused arguments, and the call through DESIREModel and the evaluation command line."""
import ctypes as C

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import (EVAL_FLAGS as _FLAGS, PLAIN_KEYS as _PLAIN_KEYS, walking_video as _video,
                           MISALIGNED_SHAPES, at_byte_offset, make_case, small_dims)
from tests.rank_reference import planted_scores, rank_order, ranked_errors
from tests.select_reference import (DIST_FINAL, DIST_MAX, DIST_MEAN, MARGIN, METRICS, cases_of, make_inputs, margin_of_values, pair_values,
                                    select_f32, select_f64, weights)

pytestmark = pytest.mark.gpu
FILL, IFILL = -7.0, -77
RADIUS_PX = 20.0
# (n_scenes, mno, K, T_pred)
SHAPES = [(2, 8, 5, 12),                # the plain case
          (2, 8, 3, 7),                 # odd T_pred
          (3, 1, 3, 7),                 # rows off 16-byte alignment
          (2, 4, 1, 5),                 # K = 1
          (3, 32, 20, 40),              # the headline's tiling: eight agents per workgroup at t_end 40, sixteen at 20 and 1
          (2, 160, 130, 9),             # K beyond a wave and beyond 64; at t_end 5 chunks of seven slots, the last one partial
          (2, 32, 3, 200)]              # long rows


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


def _rank(torch, h, d, s_t):
    order = torch.full((d.A, d.K), IFILL, device="cuda", dtype=torch.int32)
    h.rank_samples(s_t.data_ptr(), 0, 1, order.data_ptr(), 0, 0)
    return order


def _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, radius, ux, uy, n_top, mass=True, gather=True, stream=0):
    out = {"order": torch.full((d.A, d.K), IFILL, device="cuda", dtype=torch.int32), "count": torch.full((d.A,), IFILL, device="cuda", dtype=torch.int32),
           "mass": torch.full((d.A, d.K), FILL, device="cuda") if mass else None,
           "top_Y": torch.full((d.A, n_top, d.T_pred, 2), FILL, device="cuda") if gather else None,
           "top_score": torch.full((d.A, n_top), FILL, device="cuda") if gather and s_t is not None else None}
    ptr = lambda x: x.data_ptr() if x is not None else 0
    h.select_diverse(Y_t.data_ptr(), order_t.data_ptr(), ptr(s_t), metric, t_end, radius, ux, uy, n_top, out["order"].data_ptr(),
                     out["count"].data_ptr(), ptr(out["mass"]), ptr(out["top_Y"]), ptr(out["top_score"]), stream)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _rows(Y, s, order_out, n_top, d):
    """The rows and scores of the first n_top entries, indexed on the host: [A, n_top, T, 2], [A, n_top]."""
    Yk = Y.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).transpose(0, 2, 1, 3, 4).reshape(d.A, d.K, d.T_pred, 2)
    sk = s.reshape(d.n_scenes, d.K, d.mno).transpose(0, 2, 1).reshape(d.A, d.K)
    idx = order_out[:, :n_top].astype(np.int64)
    a = np.arange(d.A)[:, None]
    return Yk[a, idx], sk[a, idx]


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_order_count_mass_and_gather_match_the_reference(torch_cuda, shape, unit):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims(shape)
    ux, uy, radius = _units(d)[unit]
    s = planted_scores(d, 9)
    Y, _ = make_inputs(d, radius, ux, uy, seed=31 + unit)
    h = _lib.Handle(d)
    Y_t, s_t = _t(torch, Y), _t(torch, s)
    order_t = _rank(torch, h, d, s_t)
    order = order_t.cpu().numpy()
    np.testing.assert_array_equal(order, rank_order(s, d))
    n_top = min(d.K, 3)
    worst = 0.0
    for metric, t_end in cases_of(d):
        # the float64 pass alone, before any comparison: no pair within the margin of the radius
        v64 = pair_values(Y, metric, t_end, ux, uy, d, np.float64)
        assert margin_of_values(v64, metric, radius) > MARGIN
        v32 = pair_values(Y, metric, t_end, ux, uy, d, np.float32)
        f64 = select_f64(Y, order, s, metric, t_end, radius, ux, uy, d, values=v64)
        f32 = select_f32(Y, order, s, metric, t_end, radius, ux, uy, d, values=v32)
        flat = select_f32(Y, order, None, metric, t_end, radius, ux, uy, d, values=v32)
        for key in ("order", "count"):
            np.testing.assert_array_equal(f32[key], f64[key])
        got = _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, radius, ux, uy, n_top)
        np.testing.assert_array_equal(got["order"], f32["order"])
        np.testing.assert_array_equal(got["count"], f32["count"])
        basis = float(np.abs(f32["mass"].astype(np.float64) - f64["mass"]).max())
        bar = max(4.0 * basis, 1e-5)
        err = float(np.abs(got["mass"].astype(np.float64) - f64["mass"]).max())
        worst = max(worst, err)
        print("metric %d t_end %d: kept %.2f per agent, max |mass - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g"
              % (metric, t_end, f32["count"].mean(), err, basis, bar))
        assert err <= bar
        assert (got["mass"][np.arange(d.K)[None] >= got["count"][:, None]] == 0).all()
        want_Y, want_s = _rows(Y, s, got["order"], n_top, d)
        np.testing.assert_array_equal(got["top_Y"].view(np.uint32), want_Y.view(np.uint32))
        np.testing.assert_array_equal(got["top_score"].view(np.uint32), want_s.view(np.uint32))
        # NULL scores: equal weights, no expf -- bit for bit; the optional outputs left out change nothing
        eq = _call(torch, h, d, Y_t, order_t, None, metric, t_end, radius, ux, uy, n_top)
        np.testing.assert_array_equal(eq["order"], f32["order"]); np.testing.assert_array_equal(eq["count"], f32["count"])
        np.testing.assert_array_equal(eq["mass"].view(np.uint32), flat["mass"].view(np.uint32))
        np.testing.assert_array_equal(eq["top_Y"].view(np.uint32), want_Y.view(np.uint32))
        bare = _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, radius, ux, uy, n_top, mass=False, gather=False)
        np.testing.assert_array_equal(bare["order"], f32["order"]); np.testing.assert_array_equal(bare["count"], f32["count"])
    print("worst |mass - f64| of the shape: %.3g" % worst)
    h.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_a_sample_tensor_off_16_byte_alignment(torch_cuda, shape, off):
    """The 8-byte path of the streaming loop for a whole buffer (MEAN and FINAL): the reference as in the parity test, and the aligned call's bits."""
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims(shape)
    ux, uy, radius = _units(d)[1]
    s = planted_scores(d, 9)
    Y, _ = make_inputs(d, radius, ux, uy, seed=32)
    h = _lib.Handle(d)
    Y_t, s_t = _t(torch, Y), _t(torch, s)
    Y_off = at_byte_offset(Y_t, off)
    order_t = _rank(torch, h, d, s_t)
    order = order_t.cpu().numpy()
    n_top = min(d.K, 3)
    for metric in (DIST_MEAN, DIST_FINAL):
        t_end = d.T_pred
        v64 = pair_values(Y, metric, t_end, ux, uy, d, np.float64)
        assert margin_of_values(v64, metric, radius) > MARGIN
        f64 = select_f64(Y, order, s, metric, t_end, radius, ux, uy, d, values=v64)
        f32 = select_f32(Y, order, s, metric, t_end, radius, ux, uy, d)
        for key in ("order", "count"):
            np.testing.assert_array_equal(f32[key], f64[key])
        got = _call(torch, h, d, Y_off, order_t, s_t, metric, t_end, radius, ux, uy, n_top)
        np.testing.assert_array_equal(got["order"], f32["order"])
        np.testing.assert_array_equal(got["count"], f32["count"])
        basis = float(np.abs(f32["mass"].astype(np.float64) - f64["mass"]).max())
        bar = max(4.0 * basis, 1e-5)
        err = float(np.abs(got["mass"].astype(np.float64) - f64["mass"]).max())
        print("offset %d metric %d: max |mass - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g" % (off, metric, err, basis, bar))
        assert err <= bar
        want_Y, want_s = _rows(Y, s, got["order"], n_top, d)
        np.testing.assert_array_equal(got["top_Y"].view(np.uint32), want_Y.view(np.uint32))
        np.testing.assert_array_equal(got["top_score"].view(np.uint32), want_s.view(np.uint32))
        aligned = _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, radius, ux, uy, n_top)
        for key in got:
            np.testing.assert_array_equal(got[key].view(np.uint32), aligned[key].view(np.uint32), err_msg=key)
    h.close()


def test_the_boundary_is_exact(torch_cuda):
    """Coordinates on multiples of 1/8, partners (3/8, 4/8) apart in every frame: q = 25/64 and sqrt(q) = 5/8 exactly, sums of 5/8 over 6 frames and
    their mean too.  radius = 0.625f: r2 = 25/64, the strict comparison does not suppress; the next float up does."""
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((2, 4, 4, 6))
    rng = np.random.default_rng(3)
    Yk = np.zeros((d.n_scenes, d.K, d.mno, d.T_pred, 2), np.float32)
    base = rng.integers(8, 24, (d.n_scenes, 1, d.mno, d.T_pred, 2)).astype(np.float32) / 8
    Yk[:] = base
    Yk[:, 1] += np.array([3 / 8, 4 / 8], np.float32)            # the partner of sample 0
    Yk[:, 2] += np.array([40 / 8, 0], np.float32)               # far from both
    Yk[:, 3] += np.array([40 / 8 + 4 / 8, 3 / 8], np.float32)   # the partner of sample 2
    Y = np.ascontiguousarray(Yk.reshape(d.R, d.T_pred, 2))
    s = np.random.default_rng(4).standard_normal((d.n_scenes, d.K, d.mno)).astype(np.float32)
    h = _lib.Handle(d)
    Y_t, s_t = _t(torch, Y), _t(torch, s)
    order_t = _rank(torch, h, d, s_t)
    order = order_t.cpu().numpy()
    r0 = np.float32(0.625)
    r1 = np.nextafter(r0, np.float32(1))
    assert r0 * r0 == np.float32(25 / 64) and r1 > r0
    for metric in (DIST_FINAL, DIST_MAX, DIST_MEAN):
        for t_end in (1, d.T_pred):
            at = _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, float(r0), 1.0, 1.0, 2)
            np.testing.assert_array_equal(at["count"], d.K)
            np.testing.assert_array_equal(at["order"], order)
            up = _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, float(r1), 1.0, 1.0, 2)
            np.testing.assert_array_equal(up["count"], 2)
            for key, r in (("at", r0), ("up", r1)):
                ref = select_f32(Y, order, s, metric, t_end, float(r), 1.0, 1.0, d)
                np.testing.assert_array_equal((at if key == "at" else up)["order"], ref["order"])
    h.close()


def test_limiting_cases(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((2, 8, 5, 12))
    ux, uy, radius = _units(d)[1]
    Y, _ = make_inputs(d, radius, ux, uy, seed=2)
    Yk = Y.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2)
    Yk[1, :, 2] = 0; Yk[1, :, 5] = 0                               # two more absent slots (the generator's: agent mno - 1)
    absent = [d.mno - 1, d.mno + 2, d.mno + 5]
    s = planted_scores(d, 4)
    h = _lib.Handle(d)
    Y_t, s_t = _t(torch, Y), _t(torch, s)
    order_t = _rank(torch, h, d, s_t)
    order = order_t.cpu().numpy()
    w32 = np.take_along_axis(weights(None, d, np.float32), order.astype(np.int64), 1)
    w64 = np.take_along_axis(weights(s, d, np.float64), order.astype(np.int64), 1)
    basis = float(np.abs(np.take_along_axis(weights(s, d, np.float32), order.astype(np.int64), 1).astype(np.float64) - w64).max())
    for metric in METRICS:
        for t_end in (1, 7, d.T_pred):
            z = _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, 0.0, ux, uy, 2)          # radius 0: the identity, the mass is w in processing order
            np.testing.assert_array_equal(z["order"], order)
            np.testing.assert_array_equal(z["count"], d.K)
            assert float(np.abs(z["mass"].astype(np.float64) - w64).max()) <= max(4.0 * basis, 1e-5)
            z0 = _call(torch, h, d, Y_t, order_t, None, metric, t_end, 0.0, ux, uy, 2)
            np.testing.assert_array_equal(z0["mass"].view(np.uint32), w32.view(np.uint32))
            big = _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, 1e30, ux, uy, 2)        # everything is near the first
            np.testing.assert_array_equal(big["order"], order)
            np.testing.assert_array_equal(big["count"], 1)
            assert (big["mass"][:, 1:] == 0).all()
            np.testing.assert_allclose(big["mass"][:, 0], 1.0, rtol=0, atol=1e-5)
            for r in (radius, 1e-15):                                                          # an absent slot's zero rows coincide: any radius > 0
                got = _call(torch, h, d, Y_t, order_t, s_t, metric, t_end, r, ux, uy, 2)
                np.testing.assert_array_equal(got["count"][absent], 1)
                np.testing.assert_array_equal(got["order"][absent], order[absent])
    h.close()


def test_results_are_bitwise_reproducible_and_depend_on_the_agent_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((4, 8, 5, 12))
    ux, uy, radius = _units(d)[1]
    Y, _ = make_inputs(d, radius, ux, uy, seed=11)
    s = planted_scores(d, 12)
    h = _lib.Handle(d)
    Y_t, s_t = _t(torch, Y), _t(torch, s)
    order_t = _rank(torch, h, d, s_t)

    def same(a, b, rows=slice(None)):
        for key in ("order", "count", "mass", "top_Y", "top_score"):
            np.testing.assert_array_equal(a[key].view(np.uint32), b[key][rows].view(np.uint32), err_msg=key)

    hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
    h1 = _lib.Handle(d.replace(n_scenes=1))
    d1 = h1.dims
    Yw, sw = Y.reshape(d.n_scenes, d.K * d.mno, d.T_pred, 2), s.reshape(d.n_scenes, d.K, d.mno)
    for metric in METRICS:
        ref = _call(torch, h, d, Y_t, order_t, s_t, metric, d.T_pred, radius, ux, uy, 2)
        assert (ref["count"] > 1).any() and (ref["count"] < d.K).any()
        same(_call(torch, h, d, Y_t, order_t, s_t, metric, d.T_pred, radius, ux, uy, 2), ref)          # run to run
        same(_call(torch, hc, d, Y_t, order_t, s_t, metric, d.T_pred, radius, ux, uy, 2), ref)         # the padding-skipping flags are not its business
        for w in range(d.n_scenes):                                                                    # every window alone
            one = _call(torch, h1, d1, _t(torch, Yw[w]), order_t[w * d.mno:(w + 1) * d.mno].contiguous(), _t(torch, sw[w]), metric, d.T_pred,
                        radius, ux, uy, 2)
            same(one, ref, slice(w * d.mno, (w + 1) * d.mno))
    for x in (h, hc, h1):
        x.close()


def test_rank_select_and_errors_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((3, 8, 6, 12))
    ux, uy, radius = _units(d)[1]
    cases = {}
    for tag, seed in (("a", 21), ("b", 22)):
        past, fut, _, _, _ = make_case(d, seed=seed, n_absent=2)
        cases[tag] = (make_inputs(d, radius, ux, uy, seed=seed)[0], planted_scores(d, seed + 5), fut)
    h = _lib.Handle(d); h.set_weights(init_weights(d, 5))            # (desire_graph_begin wants a finalised handle; the three calls read no weight)
    Y, sc, f = (_t(torch, x) for x in cases["a"])
    order = torch.zeros((d.A, d.K), device="cuda", dtype=torch.int32); div = torch.zeros_like(order)
    count = torch.zeros((d.A,), device="cuda", dtype=torch.int32); mass = torch.zeros((d.A, d.K), device="cuda")
    top_Y = torch.zeros((d.A, 2, d.T_pred, 2), device="cuda"); top_s = torch.zeros((d.A, 2), device="cuda")
    errs = torch.zeros((d.A, 4, 4), device="cuda")
    hz = [3, 6, 9, 12]
    side = torch.cuda.Stream(); sp = side.cuda_stream                 # explicit and non-default

    def calls():
        h.rank_samples(sc.data_ptr(), 0, 2, order.data_ptr(), 0, 0, sp)
        h.select_diverse(Y.data_ptr(), order.data_ptr(), sc.data_ptr(), DIST_MEAN, d.T_pred, radius, ux, uy, 2, div.data_ptr(), count.data_ptr(),
                         mass.data_ptr(), top_Y.data_ptr(), top_s.data_ptr(), sp)
        h.ranked_errors(Y.data_ptr(), f.data_ptr(), div.data_ptr(), 2, hz, ux, uy, errs.data_ptr(), sp)

    bufs = (order, div, count, mass, top_Y, top_s, errs)
    torch.cuda.synchronize()
    ref = {}
    for tag in ("b", "a"):                                            # eager calls
        for dst, src in zip((Y, sc, f), cases[tag]):
            dst.copy_(_t(torch, src))
        torch.cuda.synchronize()
        calls()
        side.synchronize()
        ref[tag] = [x.clone() for x in bufs]
    h.graph_begin(sp)
    calls()
    gid = h.graph_end(sp)
    for rep in range(4):
        tag = "b" if rep % 2 == 0 else "a"
        for dst, src in zip((Y, sc, f), cases[tag]):                  # in place: the graph keeps its pointers
            dst.copy_(_t(torch, src))
        for x in bufs:
            x.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        for x, r in zip(bufs, ref[tag]):
            assert torch.equal(x.view(torch.int32), r.view(torch.int32)), (rep, tag)      # bit patterns: the planted scores hold NaNs
    assert not torch.equal(ref["a"][1], ref["b"][1]) and not torch.equal(ref["a"][1], ref["a"][0])      # the selection reorders, and differently
    sel = select_f32(cases["a"][0], ref["a"][0].cpu().numpy(), cases["a"][1], DIST_MEAN, d.T_pred, radius, ux, uy, d)
    np.testing.assert_array_equal(ref["a"][1].cpu().numpy(), sel["order"])
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((1, 4, 3, 6))
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") + 0.5
    zi = torch.zeros(4096, device="cuda", dtype=torch.int32)
    outs = {"order_out_ptr": torch.full((d.A, d.K), IFILL, device="cuda", dtype=torch.int32), "count_ptr": torch.full((d.A,), IFILL, device="cuda", dtype=torch.int32),
            "mass_ptr": torch.full((d.A, d.K), FILL, device="cuda"), "top_y_ptr": torch.full((d.A, d.K, d.T_pred, 2), FILL, device="cuda"),
            "top_score_ptr": torch.full((d.A, d.K), FILL, device="cuda")}
    nan, inf = float("nan"), float("inf")
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(order_ptr=0), "dev_order"), (dict(order_out_ptr=0), "dev_order_out"), (dict(count_ptr=0), "dev_count"),
             (dict(score_ptr=0), "dev_score"),
             (dict(metric=-1), "metric"), (dict(metric=3), "metric"), (dict(t_end=0), "t_end"), (dict(t_end=7), "t_end"), (dict(t_end=-1), "t_end"),
             (dict(n_top=0), "n_top"), (dict(n_top=4), "n_top"), (dict(radius=-1e-3), "radius"), (dict(radius=nan), "radius"), (dict(radius=inf), "radius"),
             (dict(unit_x=0.0), "unit_x"), (dict(unit_x=-1.0), "unit_x"), (dict(unit_x=nan), "unit_x"), (dict(unit_x=inf), "unit_x"),
             (dict(unit_y=0.0), "unit_y"), (dict(unit_y=-2.0), "unit_y"), (dict(unit_y=nan), "unit_y"), (dict(unit_y=inf), "unit_y")]
    for kw, word in cases:
        args = dict(yhat_ptr=z.data_ptr(), order_ptr=zi.data_ptr(), score_ptr=z.data_ptr(), metric=DIST_MEAN, t_end=6, radius=1.0, unit_x=1.0, unit_y=1.0,
                    n_top=2, **{k: v.data_ptr() for k, v in outs.items()})
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.select_diverse(**args)
    lib = _lib.load()
    one = C.c_float(1)
    assert lib.desire_select_diverse(None, z.data_ptr(), zi.data_ptr(), None, 0, 1, one, one, one, 1, outs["order_out_ptr"].data_ptr(),
                                     outs["count_ptr"].data_ptr(), None, None, None, None) == -1
    assert b"handle" in lib.desire_last_error()
    # the LDS plan: 130 samples of 200 frames do not fit (130 * (8 * 201 + 20) + 8 bytes), nor of 56 (61888 > 61440); 55 do, and the last frame alone
    big = _lib.Handle(_dims((1, 4, 130, 200)))
    ob, cb = torch.full((4, 130), IFILL, device="cuda", dtype=torch.int32), torch.full((4,), IFILL, device="cuda", dtype=torch.int32)
    Yb = torch.zeros((4 * 130, 200, 2), device="cuda"); ib = torch.arange(130, device="cuda", dtype=torch.int32).repeat(4, 1).contiguous()
    for metric, t_end in ((DIST_MEAN, 200), (DIST_MAX, 200), (DIST_MEAN, 56)):
        with pytest.raises(_lib.DesireError, match="error -1.*LDS"):
            big.select_diverse(Yb.data_ptr(), ib.data_ptr(), 0, metric, t_end, 1.0, 1.0, 1.0, 1, ob.data_ptr(), cb.data_ptr())
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.select_diverse(z.data_ptr(), zi.data_ptr(), 0, 0, 8, 1.0, 1.0, 1.0, 1, outs["order_out_ptr"].data_ptr(), outs["count_ptr"].data_ptr())
    torch.cuda.synchronize()
    assert all(bool((v == (IFILL if v.dtype == torch.int32 else FILL)).all()) for v in outs.values())
    assert bool((ob == IFILL).all()) and bool((cb == IFILL).all())
    # ... and the handles still work: the largest plan that fits, and the last frame of the long rows
    big.select_diverse(Yb.data_ptr(), ib.data_ptr(), 0, DIST_MEAN, 55, 1.0, 1.0, 1.0, 1, ob.data_ptr(), cb.data_ptr())
    torch.cuda.synchronize()
    assert bool((cb == 1).all()) and torch.equal(ob, ib)
    cb.fill_(IFILL)
    big.select_diverse(Yb.data_ptr(), ib.data_ptr(), 0, DIST_FINAL, 200, 1.0, 1.0, 1.0, 1, ob.data_ptr(), cb.data_ptr())
    torch.cuda.synchronize()
    assert bool((cb == 1).all())
    h.select_diverse(z.data_ptr(), zi.data_ptr(), 0, DIST_MAX, 6, 0.0, 1.0, 1.0, 1, outs["order_out_ptr"].data_ptr(), outs["count_ptr"].data_ptr())
    torch.cuda.synchronize()
    assert bool((outs["count_ptr"] == d.K).all()) and bool((outs["order_out_ptr"] == 0).all()) and bool((outs["mass_ptr"] == FILL).all())
    for x in (h, big, rc):
        x.close()


def _radius_with_a_margin(Y, metric, t_end, ux, uy, d, present):
    """A radius in the middle of the widest gap between the sorted pair distances of the present agents (their middle half), so that select_f32 is
    a valid reference for samples the test did not lay out; the caller asserts the margin."""
    v = pair_values(Y, metric, t_end, ux, uy, d, np.float64)
    dist = (v if metric == DIST_MEAN else np.sqrt(v))[present][:, np.triu(np.ones((d.K, d.K), bool), 1)].reshape(-1)
    dist = np.sort(dist[dist > 0])
    mid = dist[len(dist) // 4: max(len(dist) // 4 + 2, 3 * len(dist) // 4)]
    i = int(np.argmax(np.diff(mid) / mid[1:]))
    return float(np.float32(0.5 * (mid[i] + mid[i + 1])))


def test_predict_and_evaluate_ranked_select_distinct_futures(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib, evaluate as E
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    a = E.build_parser().parse_args(_FLAGS)
    m = DESIREModel(a, seed=4)
    video = _video()
    wins = [video[i * 10:i * 10 + 10] for i in range(2)]
    past, fut = split_windows(wins, a.seq_length)
    top = 3
    # the default is today's path: exactly the keys and tensors of a direct desire_rank_samples call
    plain = m.predict(past, top=top, seed=3, device_rng=True)
    Y, score = m.final_output.clone(), m.final_states.clone()
    h = m._handle(2, False)
    d = h.dims
    assert sorted(plain) == ["order", "present", "score", "traj"]
    order = torch.empty((d.A, d.K), device="cuda", dtype=torch.int32)
    tY = torch.empty((d.A, top, d.T_pred, 2), device="cuda"); ts = torch.empty((d.A, top), device="cuda")
    h.rank_samples(score.data_ptr(), Y.data_ptr(), top, order.data_ptr(), tY.data_ptr(), ts.data_ptr())
    scale = torch.tensor([d.sx, d.sy], device="cuda", dtype=torch.float32)
    assert torch.equal(plain["order"].reshape(d.A, d.K), order) and torch.equal(plain["score"].reshape(d.A, top), ts)
    assert torch.equal(plain["traj"].reshape(d.A, top, d.T_pred, 2), tY / scale)
    again = m.predict(past, top=top, seed=3, device_rng=True, select="score")
    assert all(torch.equal(again[k], plain[k]) for k in plain)
    Yn, sn = Y.cpu().numpy().reshape(d.R, d.T_pred, 2), score.cpu().numpy()
    present = plain["present"].cpu().numpy().reshape(-1)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    for name, metric, horizon in (("final", DIST_FINAL, None), ("mean", DIST_MEAN, 4), ("max", DIST_MAX, None)):
        t_end = horizon or d.T_pred
        radius = _radius_with_a_margin(Yn, metric, t_end, ux, uy, d, present)
        out = m.predict(past, top=top, seed=3, device_rng=True, select="nms", nms_radius=radius, nms_metric=name, nms_horizon=horizon)
        assert sorted(out) == ["count", "order", "present", "prob", "score", "traj"]
        assert torch.equal(m.final_output, Y) and torch.equal(m.final_states, score)                   # the same samples: the device generator's draw
        got = _call(torch, h, d, Y, order, score, metric, t_end, radius, ux, uy, top)
        np.testing.assert_array_equal(out["order"].cpu().numpy().reshape(d.A, d.K), got["order"])
        np.testing.assert_array_equal(out["count"].cpu().numpy().reshape(d.A), got["count"])
        np.testing.assert_array_equal(out["prob"].cpu().numpy().reshape(d.A, top).view(np.uint32), got["mass"][:, :top].view(np.uint32))
        np.testing.assert_array_equal(out["traj"].cpu().numpy().reshape(d.A, top, d.T_pred, 2), (_t(torch, got["top_Y"]) / scale).cpu().numpy())
        np.testing.assert_array_equal(out["score"].cpu().numpy().reshape(d.A, top), got["top_score"])
        assert tuple(out["count"].shape) == (2, d.mno) and tuple(out["prob"].shape) == (2, d.mno, top) and out["count"].dtype == torch.int32
        assert float(out["prob"].sum(-1).max()) <= 1 + 1e-5 and float(out["prob"].min()) >= 0
        # evaluate_ranked under the selection = the stand-alone error reference fed the reference's diverse order
        v64 = pair_values(Yn, metric, t_end, ux, uy, d, np.float64)
        off = ~np.eye(d.K, dtype=bool)
        dist = (v64 if metric == DIST_MEAN else np.sqrt(v64))[present][:, off]
        assert float(np.abs(dist - radius).min()) > MARGIN * radius
        ref = select_f32(Yn, order.cpu().numpy(), sn, metric, t_end, radius, ux, uy, d)
        np.testing.assert_array_equal(got["order"][present], ref["order"][present])
        assert (ref["count"][present] > 1).any() and (ref["count"][present] < d.K).any()
        futp = m._pad_windows(fut, d.mno)
        ev, kept = m.evaluate_ranked(Y, score, fut, top=top, horizons=[2, 4, 6], units="px", select="nms", nms_radius=radius, nms_metric=name,
                                     nms_horizon=horizon, return_count=True)
        want = ranked_errors(Yn, futp.cpu().numpy(), got["order"], top, [2, 4, 6], ux, uy, d)
        np.testing.assert_allclose(ev, want, rtol=0, atol=1e-5 / min(d.sx, d.sy))
        np.testing.assert_array_equal(kept, got["count"])
        base = m.evaluate_ranked(Y, score, fut, top=top, horizons=[2, 4, 6], units="px")
        np.testing.assert_array_equal(ev[..., :2], base[..., :2])                                       # the best-scored sample is always kept first
    with pytest.raises(ValueError, match="nms_radius"):
        m.predict(past, select="nms")
    with pytest.raises(ValueError, match="nms_metric"):
        m.predict(past, select="nms", nms_radius=5.0, nms_metric="median")
    with pytest.raises(ValueError, match="nms_horizon"):
        m.predict(past, select="nms", nms_radius=5.0, nms_horizon=7)
    with pytest.raises(ValueError, match="select"):
        m.predict(past, select="best")


def test_the_evaluation_walk_reports_the_selection(torch_cuda):
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    import json
    video = _video()
    res = {}
    for tag, extra in (("plain", []), ("nms", ["--select", "nms", "--nms_radius", "6", "--nms_metric", "mean", "--nms_horizon", "4"]),
                       ("wide", ["--select", "nms", "--nms_radius", "100000"]), ("zero", ["--select", "nms", "--nms_radius", "0"])):
        a = E.build_parser().parse_args(_FLAGS + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=DESIREModel(a, seed=4))
    assert list(res["plain"]) == _PLAIN_KEYS                           # without the flag: the result it has always been
    plain_text = json.dumps(res["plain"], indent=1)
    for tag in ("nms", "wide", "zero"):
        blk = res[tag].pop("select")
        assert json.dumps(res[tag], indent=1) == plain_text            # ... and with it, the same result plus one block
        assert set(blk) == {"mode", "radius_px", "metric", "horizon", "mean_count", "present_agents", "best_of_top_distinct"} and blk["mode"] == "nms"
        assert len(blk["best_of_top_distinct"]["ade"]) == len(blk["best_of_top_distinct"]["fde"]) == len(res["plain"]["horizons"])
        assert np.isfinite(blk["best_of_top_distinct"]["ade"] + blk["best_of_top_distinct"]["fde"]).all() and blk["present_agents"] > 0
        res[tag]["select"] = blk
    K, top = res["plain"]["K"], res["plain"]["top"]
    assert (res["nms"]["select"]["metric"], res["nms"]["select"]["horizon"], res["nms"]["select"]["radius_px"]) == ("mean", 4, 6.0)
    assert (res["wide"]["select"]["metric"], res["wide"]["select"]["horizon"]) == ("final", 6)
    assert res["wide"]["select"]["mean_count"] == 1.0 and res["zero"]["select"]["mean_count"] == float(K)
    assert 1.0 <= res["nms"]["select"]["mean_count"] <= K
    # nothing suppressed, or everything: the order is the order by score, so the distinct column is best_of_top
    for tag in ("wide", "zero"):
        assert res[tag]["select"]["best_of_top_distinct"] == res["plain"]["best_of_top"]
    # the top-1 is always the first kept; more distinct futures cannot be worse than the best of all K
    for i in range(len(res["plain"]["horizons"])):
        d_ade = res["nms"]["select"]["best_of_top_distinct"]["ade"][i]
        assert res["plain"]["best_of_K"]["ade"][i] - 1e-12 <= d_ade <= res["plain"]["top1"]["ade"][i] + 1e-12
    a = E.build_parser().parse_args(_FLAGS + ["--select", "nms"])
    with pytest.raises(ValueError, match="nms_radius"):
        E.evaluate(a, data_loader=DataLoader(2, 10, 8, a.leave_dataset, frames=[video]), model=DESIREModel(a, seed=4))
