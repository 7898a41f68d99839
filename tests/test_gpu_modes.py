"""n modes with covariances fitted to the K samples on the device (desire_fit_modes, csrc/kernels_modes.hip) against the numpy statements of its
contract (tests/modes_reference.py).  Labels, counts and pass counts are compared exactly with modes_f32 AND modes_f64 -- on inputs whose float64
fit keeps a relative margin of 1e-3 between a sample's best and second-best distance in every assign, asserted first on the float64 pass alone;
mean, prob and cov with modes_f32 bit for bit where every weight is 1 / K (NULL scores), and within the derived bounds of modes_f64 under the
planted scores (fit_bounds).  The likelihood follows test_gpu_kde.py's rule: the bar is four times the fp32 statement's own distance from
modes_f64, never below 1e-5.  Then the exact properties, independence and reproducibility, alignment, the optional outputs, capture, refused
arguments, and the calls through DESIREModel and the command line.

Observed on an MI355X: see DESIGN.md section 7j."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import (EVAL_FLAGS as _FLAGS, PLAIN_KEYS as _PLAIN_KEYS, walking_video as _video, _same_bits as _same_bits_of,
                           _likelihood, _t, _within, at_byte_offset, make_case, small_dims)
from tests.modes_reference import (LOG_FLOOR, MARGIN, SHAPES, fit_bounds, make_inputs, modes_f32, modes_f64, padded_mno, var_floor_of)

pytestmark = pytest.mark.gpu
FILL, IFILL = -7.0, -77
ITERS = 8
FIT = ("label", "count", "prob", "mean", "cov", "passes")
ALL = FIT + ("out", "frame")
IDS = lambda s: "n%d_m%d_K%d_T%d_n%d" % s
_CASES = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _dims(shape, **kw):
    """The handle of a shape: its objects padded up to a slot count a handle takes (3 -> 4, 5 -> 8), the padding being absent slots."""
    n, m, K, T = shape[:4]
    return small_dims(n_scenes=n, mno=padded_mno(m), K=K, T_obs=4, T_pred=T, n_grids=1, H=64, **kw)


def _units(d):
    return [(1.0, 1.0), (1.0 / d.sx, 1.0 / d.sy)]


def _hz(T):
    return sorted({max(1, T // 4), max(1, T // 2), T})


def _case(shape, unit, t_end=None, seed=5):
    """Inputs of (shape, unit, t_end), computed once and left unchanged; the references are added per (scores, iters, floor) on first use."""
    key = (shape, unit, t_end, seed)
    if key not in _CASES:
        d = _dims(shape)
        ux, uy = _units(d)[unit]
        te = d.T_pred if t_end is None else t_end
        Y, order, score, fut, info = make_inputs(d, shape[4], te, ux, uy, seed=seed + unit, live=shape[1])
        for a in (Y, order, score, fut):
            a.setflags(write=False)
        _CASES[key] = dict(d=d, n=shape[4], t_end=te, Y=Y, order=order, score=score, fut=fut, info=info, hz=_hz(d.T_pred), unit=(ux, uy),
                           vf=var_floor_of(ux, d.sx), refs={})
    return _CASES[key]


def _ref(c, fn, scored, iters=ITERS, vf=None, fut=True):
    key = (fn.__name__, scored, iters, vf, fut)
    if key not in c["refs"]:
        ux, uy = c["unit"]
        c["refs"][key] = fn(c["Y"], c["order"], c["score"] if scored else None, c["fut"] if fut else None, c["n"], c["t_end"], iters, ux, uy,
                            c["vf"] if vf is None else vf, c["d"], c["hz"])
    return c["refs"][key]


def _call(torch, h, d, n, Y_t, order_t, s_t, fut_t, t_end, iters, ux, uy, vf, hz, want=ALL, stream=0, log_floor=LOG_FLOOR):
    A, K, T = d.A, d.K, d.T_pred
    i32 = torch.int32
    buf = {"label": torch.full((A, K), IFILL, device="cuda", dtype=i32), "count": torch.full((A, n), IFILL, device="cuda", dtype=i32),
           "prob": torch.full((A, n), FILL, device="cuda"), "mean": torch.full((A, n, T, 2), FILL, device="cuda"),
           "cov": torch.full((A, n, T, 3), FILL, device="cuda"), "passes": torch.full((A,), IFILL, device="cuda", dtype=i32),
           "out": torch.full((A, len(hz), 2), FILL, device="cuda"), "frame": torch.full((A, T), FILL, device="cuda")}
    ptr = lambda k: buf[k].data_ptr() if k in want else 0
    h.fit_modes(Y_t.data_ptr(), order_t.data_ptr(), s_t.data_ptr() if s_t is not None else 0, n, t_end, iters, ux, uy, vf, buf["count"].data_ptr(),
                buf["prob"].data_ptr(), ptr("label"), ptr("mean"), ptr("cov"), ptr("passes"), fut_t.data_ptr() if fut_t is not None else 0,
                hz if fut_t is not None else None, log_floor, ptr("out") if fut_t is not None else 0, ptr("frame") if fut_t is not None else 0, stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in buf.items()}


def _run(torch, h, c, scored, iters=ITERS, vf=None, fut=True, **kw):
    ux, uy = c["unit"]
    return _call(torch, h, c["d"], c["n"], _t(torch, c["Y"]), _t(torch, c["order"]), _t(torch, c["score"]) if scored else None,
                 _t(torch, c["fut"]) if fut else None, c["t_end"], iters, ux, uy, c["vf"] if vf is None else vf, c["hz"], **kw)


_same_bits = functools.partial(_same_bits_of, keys=ALL)             # this file's default: every output


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_everything_matches_the_reference(torch_cuda, shape, unit):
    torch = torch_cuda
    from desire_amd import _lib
    c = _case(shape, unit)
    d = c["d"]
    ux, uy = c["unit"]
    h = _lib.Handle(d)
    for scored in (True, False):
        f64 = _ref(c, modes_f64, scored)
        assert f64["margin"].min() > MARGIN                                # the float64 pass alone, before any comparison
        f32 = _ref(c, modes_f32, scored)
        got = _run(torch, h, c, scored)
        for key in ("label", "count", "passes"):
            np.testing.assert_array_equal(got[key], f32[key], err_msg=key)
            np.testing.assert_array_equal(got[key], f64[key], err_msg=key)
        if scored:
            for key, bound in zip(("prob", "mean", "cov"), fit_bounds(c["Y"], f64, ux, uy, c["vf"], d)):
                gap, worst = _within(got[key], f64[key], bound, key)
                base, _ = _within(f32[key], f64[key], bound, key)
                print("%s: max |dev - f64| = %.3g (%.3g of its bound), |f32 - f64| = %.3g" % (key, gap, worst, base))
                assert worst <= 1.0, key
        else:                                                              # every weight 1 / K: the bits of the fp32 statement
            _same_bits(got, f32, keys=("prob", "mean", "cov"))
        _likelihood(got, f32, f64, "scored" if scored else "uniform")
    if d.K > 2 and d.A > 2:
        assert got["passes"].max() >= 1 and (got["count"] > 0).sum() > d.A and (got["frame"] > LOG_FLOOR).any()
    h.close()


def test_the_exact_properties(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    shape = SHAPES[1]
    c = _case(shape, 1)
    d, n, K, T = c["d"], c["n"], c["d"].K, c["d"].T_pred
    h = _lib.Handle(d)
    base = _run(torch, h, c, False)
    assert base["passes"].max() < ITERS and base["passes"].max() >= 2
    # iters = 0: the weighted means of the seeds' Voronoi cells
    zero = _run(torch, h, c, False, iters=0)
    _same_bits(zero, _ref(c, modes_f32, False, iters=0), keys=FIT)
    assert (zero["passes"] == 0).all() and (zero["label"] != base["label"]).any()
    # more passes than the convergence point needs: the converged bits
    _same_bits(_run(torch, h, c, False, iters=32), base)
    _same_bits(_run(torch, h, c, True, iters=32), _run(torch, h, c, True))
    # a pass cap below it: the labels of that pass
    one = _run(torch, h, c, False, iters=1)
    _same_bits(one, _ref(c, modes_f32, False, iters=1), keys=FIT)
    assert (one["passes"] == 1).all()
    # the assignment looks at t < t_end only: a NaN behind it stays out of the labels and shows in that frame's mean and covariance alone
    te = T // 2
    ce = _case(shape, 1, t_end=te)
    assert "nanlate" in ce["info"]["kinds"]
    got = _run(torch, h, ce, False)
    f32 = _ref(ce, modes_f32, False)
    _same_bits(got, f32, keys=FIT)
    np.testing.assert_array_equal(got["label"], _ref(ce, modes_f64, False)["label"])
    a = ce["info"]["kinds"].index("nanlate")
    assert (got["label"][a] >= 0).all() and np.isnan(got["mean"][a]).any() and not np.isnan(got["mean"][a][:, :te]).any()
    a = ce["info"]["kinds"].index("nanrow")
    assert (got["label"][a] == -1).sum() == 1 and got["count"][a].sum() == K - 1 and got["prob"][a].sum() < 1 - 0.5 / K
    a = ce["info"]["kinds"].index("zero")
    assert got["count"][a].tolist() == [K] + [0] * (n - 1) and (got["cov"][a][0] == np.float32(ce["vf"]) * np.array([1, 1, 0], np.float32)).all()
    assert not got["cov"][a][1:].any() and not got["mean"][a].any()
    # var_floor = 0: a mode of one member has no spread and is left out of the likelihood
    flat = _run(torch, h, c, False, vf=0.0)
    f32, f64 = _ref(c, modes_f32, False, vf=0.0), _ref(c, modes_f64, False, vf=0.0)
    _same_bits(flat, f32, keys=FIT)
    single = flat["count"] == 1                                            # (w * y) / w is y to an ulp, so its spread is rounding noise, and rank one
    tiny = (2.0 ** -22 * c["unit"][0]) ** 2
    assert np.abs(flat["cov"][single]).max() <= tiny
    _likelihood(flat, f32, f64, "var_floor 0")
    counted = (c["fut"][..., 0] != 0).transpose(0, 2, 1).reshape(d.A, T)
    c3 = _case(SHAPES[6], 1)                                               # K = n = 3: every mode has one member at most, so no frame has a usable mode
    h3 = _lib.Handle(c3["d"])
    lone = _run(torch, h3, c3, False, vf=0.0)
    _same_bits(lone, _ref(c3, modes_f32, False, vf=0.0), keys=FIT)
    cnt3 = (c3["fut"][..., 0] != 0).transpose(0, 2, 1).reshape(c3["d"].A, c3["d"].T_pred)
    assert (lone["count"] == 1).any() and np.abs(lone["cov"]).max() <= tiny and (lone["frame"][cnt3] == np.float32(LOG_FLOOR)).all() and not lone["frame"][~cnt3].any()
    assert (_run(torch, h3, c3, False)["frame"][cnt3] > LOG_FLOOR).any()   # ... and with the floor variance they have one
    h3.close()
    # a BAD order row: an index out of range, and a repeated one, among the first n entries only
    order = np.array(c["order"])
    order[3, 1] = K; order[5, n - 1] = order[5, 0]; order[7, n] = -4 if K > n else order[7, n]
    cb = dict(c, order=order, refs={})
    bad = _run(torch, h, cb, True)
    _same_bits(bad, _ref(cb, modes_f32, True), keys=("label", "count", "passes"))
    for a in (3, 5):
        assert (bad["label"][a] == -1).all() and not bad["count"][a].any() and not bad["prob"][a].any() and not bad["mean"][a].any()
        assert not bad["cov"][a].any() and bad["passes"][a] == 0
        assert (bad["frame"][a][counted[a]] == np.float32(LOG_FLOOR)).all() and not bad["frame"][a][~counted[a]].any()
    good = np.setdiff1d(np.arange(d.A), [3, 5])
    _same_bits({k: v[good] for k, v in bad.items()}, {k: v[good] for k, v in _run(torch, h, c, True).items()})
    h.close()


def test_results_are_bitwise_reproducible_and_depend_on_the_agent_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    for shape in ((4, 8, 5, 7, 3), (4, 64, 20, 12, 6)):
        c = _case(shape, 1, seed=11)
        d, n = c["d"], c["n"]
        ux, uy = c["unit"]
        h = _lib.Handle(d)
        hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
        h2 = _lib.Handle(d.replace(n_scenes=2))
        ref = _run(torch, h, c, True)
        assert ref["passes"].max() >= 1
        _same_bits(_run(torch, h, c, True), ref)                            # run to run
        _same_bits(_run(torch, hc, c, True), ref)                           # the padding-skipping flags are not its business
        Yw = c["Y"].reshape(d.n_scenes, d.K * d.mno, d.T_pred, 2)
        ow = c["order"].reshape(d.n_scenes, d.mno, d.K)
        for rows in ([0, 1], [2, 3], [3, 1]):                               # any two windows, in any place of a batch of two
            got = _call(torch, h2, h2.dims, n, _t(torch, Yw[rows]), _t(torch, ow[rows]), _t(torch, c["score"][rows]), _t(torch, c["fut"][rows]),
                        c["t_end"], ITERS, ux, uy, c["vf"], c["hz"])
            ag = np.concatenate([np.arange(r * d.mno, (r + 1) * d.mno) for r in rows])
            _same_bits(got, {k: v[ag] for k, v in ref.items()})
        for off in (8, 4):                                                  # Y off 16-byte alignment: the streamer's 8- and 4-byte loads
            got = _call(torch, h, d, n, at_byte_offset(_t(torch, c["Y"]), off), _t(torch, c["order"]), _t(torch, c["score"]), _t(torch, c["fut"]),
                        c["t_end"], ITERS, ux, uy, c["vf"], c["hz"])
            _same_bits(got, ref)
        for x in (h, hc, h2):
            x.close()


def test_every_subset_of_the_optional_outputs(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    c = _case(SHAPES[0], 0)
    h = _lib.Handle(c["d"])
    full = _run(torch, h, c, True)
    opt = ("label", "mean", "cov", "passes", "frame")
    for r in range(len(opt) + 1):
        for sub in itertools.combinations(opt, r):
            want = ("count", "prob", "out") + sub
            got = _run(torch, h, c, True, want=want)
            _same_bits(got, full, keys=want)
            for key in set(opt) - set(sub):
                assert (got[key] == (IFILL if got[key].dtype.kind == "i" else FILL)).all(), key
    nofut = _run(torch, h, c, True, fut=False)                              # no targets: the fit alone
    _same_bits(nofut, full, keys=FIT)
    assert (nofut["out"] == FILL).all() and (nofut["frame"] == FILL).all()
    h.close()


def test_forward_rank_nms_and_fit_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=6, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    n, hz = 3, [3, 6, 12]
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    i32 = torch.int32
    h = _lib.Handle(d); h.set_weights(w)
    cases = [make_case(d, seed=21 + i, n_absent=2) for i in range(2)]
    g = _t(torch, cases[0][3]); h.set_scene_grids(g.data_ptr(), cases[0][4])
    p, f, e = (torch.zeros_like(_t(torch, x)) for x in cases[0][:3])
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    by_score = torch.zeros((d.A, d.K), device="cuda", dtype=i32); order = torch.zeros((d.A, d.K), device="cuda", dtype=i32)
    kept = torch.zeros((d.A,), device="cuda", dtype=i32)
    label = torch.zeros((d.A, d.K), device="cuda", dtype=i32); count = torch.zeros((d.A, n), device="cuda", dtype=i32)
    prob = torch.zeros((d.A, n), device="cuda"); mean = torch.zeros((d.A, n, d.T_pred, 2), device="cuda")
    cov = torch.zeros((d.A, n, d.T_pred, 3), device="cuda"); passes = torch.zeros((d.A,), device="cuda", dtype=i32)
    out = torch.zeros((d.A, 3, 2), device="cuda"); frame = torch.zeros((d.A, d.T_pred), device="cuda")
    bufs = (Y, sc, order, label, count, prob, mean, cov, passes, out, frame)
    side = torch.cuda.Stream(); sp = side.cuda_stream

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.rank_samples(sc.data_ptr(), 0, n, by_score.data_ptr(), 0, 0, sp)
        h.select_diverse(Y.data_ptr(), by_score.data_ptr(), sc.data_ptr(), _lib.DIST_FINAL, d.T_pred, 2.0, ux, uy, n, order.data_ptr(), kept.data_ptr(),
                         0, 0, 0, sp)
        h.fit_modes(Y.data_ptr(), order.data_ptr(), sc.data_ptr(), n, d.T_pred, ITERS, ux, uy, 0.25, count.data_ptr(), prob.data_ptr(), label.data_ptr(),
                    mean.data_ptr(), cov.data_ptr(), passes.data_ptr(), f.data_ptr(), hz, LOG_FLOOR, out.data_ptr(), frame.data_ptr(), sp)

    ref = []
    for a in cases:
        for dst, src in zip((p, f, e), a[:3]):
            dst.copy_(_t(torch, src))
        torch.cuda.synchronize()
        calls()
        side.synchronize()
        ref.append([x.clone() for x in bufs])
    assert not torch.equal(ref[0][6], ref[1][6])
    h.graph_begin(sp)
    calls()
    gid = h.graph_end(sp)
    for rep in range(4):
        a = cases[rep % 2]
        for dst, src in zip((p, f, e), a[:3]):                              # in place: the graph keeps its pointers
            dst.copy_(_t(torch, src))
        for x in bufs:
            x.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        for x, r in zip(bufs, ref[rep % 2]):
            assert torch.equal(x.view(i32), r.view(i32)), rep
    # the captured fit is the contract's on the captured forward's samples
    Yn, on, sn = ref[1][0].cpu().numpy(), ref[1][2].cpu().numpy(), ref[1][1].cpu().numpy().reshape(d.n_scenes, d.K, d.mno)
    want = modes_f32(Yn, on, None, None, n, d.T_pred, ITERS, ux, uy, 0.25, d)
    flat = torch.zeros_like(prob)
    h.fit_modes(ref[1][0].data_ptr(), ref[1][2].data_ptr(), 0, n, d.T_pred, ITERS, ux, uy, 0.25, count.data_ptr(), flat.data_ptr(), label.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(label.cpu().numpy(), want["label"])
    np.testing.assert_array_equal(flat.cpu().numpy().view(np.uint32), want["prob"].view(np.uint32))
    assert sn.shape[1] == d.K
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((1, 4, 3, 6))
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") + 0.5
    od = torch.arange(3, device="cuda", dtype=torch.int32).repeat(4).contiguous()
    i32 = torch.int32
    outs = {"label_ptr": torch.full((64,), IFILL, device="cuda", dtype=i32), "count_ptr": torch.full((64,), IFILL, device="cuda", dtype=i32),
            "prob_ptr": torch.full((64,), FILL, device="cuda"), "mean_ptr": torch.full((512,), FILL, device="cuda"),
            "cov_ptr": torch.full((512,), FILL, device="cuda"), "passes_ptr": torch.full((64,), IFILL, device="cuda", dtype=i32),
            "out_ptr": torch.full((64,), FILL, device="cuda"), "frame_ptr": torch.full((64,), FILL, device="cuda")}
    nan, inf = float("nan"), float("inf")
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(order_ptr=0), "dev_order"), (dict(count_ptr=0), "dev_count"), (dict(prob_ptr=0), "dev_prob"),
             (dict(n_modes=0), "n_modes"), (dict(n_modes=4), "n_modes"), (dict(n_modes=17), "n_modes"), (dict(t_end=0), "t_end"), (dict(t_end=7), "t_end"),
             (dict(iters=-1), "iters"), (dict(iters=33), "iters"),
             (dict(unit_x=0.0), "unit_x"), (dict(unit_x=nan), "unit_x"), (dict(unit_x=inf), "unit_x"), (dict(unit_y=-2.0), "unit_y"), (dict(unit_y=nan), "unit_y"),
             (dict(var_floor=-1e-9), "var_floor"), (dict(var_floor=nan), "var_floor"), (dict(var_floor=inf), "var_floor"),
             (dict(log_floor=nan), "log_floor"), (dict(log_floor=-inf), "log_floor"),
             (dict(horizons=[]), "n_h"), (dict(horizons=list(range(1, 10))), "n_h"), (dict(horizons=[0]), "host_horizons"), (dict(horizons=[7]), "host_horizons"),
             (dict(horizons=[3, 3]), "increasing"), (dict(horizons=None), "host_horizons"),
             (dict(fut_ptr=0), "dev_out needs dev_fut"), (dict(fut_ptr=0, out_ptr=0), "dev_frame needs dev_fut"), (dict(out_ptr=0), "dev_out is NULL")]
    for kw, word in cases:
        args = dict(yhat_ptr=z.data_ptr(), order_ptr=od.data_ptr(), score_ptr=z.data_ptr(), n_modes=2, t_end=6, iters=4, unit_x=1.0, unit_y=1.0,
                    var_floor=0.0, fut_ptr=z.data_ptr(), horizons=[2, 6], log_floor=LOG_FLOOR, **{k: v.data_ptr() for k, v in outs.items()})
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.fit_modes(**args)
    lib = _lib.load()
    one, zero = C.c_float(1), C.c_float(0)
    o = {k: v.data_ptr() for k, v in outs.items()}
    assert lib.desire_fit_modes(None, z.data_ptr(), od.data_ptr(), None, None, 2, 6, 4, one, one, zero, None, 0, zero, None, o["count_ptr"], o["prob_ptr"],
                                None, None, None, None, None, None) == -1
    assert b"handle" in lib.desire_last_error()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.fit_modes(z.data_ptr(), od.data_ptr(), 0, 1, 8, 4, 1.0, 1.0, 0.0, o["count_ptr"], o["prob_ptr"])
    big = _lib.Handle(_dims((1, 1, 40, 200)))                                # 8 * 56 * 201 + 12 * 16 * 200 + ... > 61440: beyond the LDS plan
    with pytest.raises(_lib.DesireError, match="error -1.*LDS.*61440"):
        big.fit_modes(z.data_ptr(), od.data_ptr(), 0, 16, 200, 4, 1.0, 1.0, 0.0, o["count_ptr"], o["prob_ptr"])
    torch.cuda.synchronize()
    assert all(bool((v == (IFILL if v.dtype == i32 else FILL)).all()) for v in outs.values())
    # ... and the handle still works
    h.fit_modes(z.data_ptr(), od.data_ptr(), 0, 2, 6, 4, 1.0, 1.0, 0.0, o["count_ptr"], o["prob_ptr"])
    torch.cuda.synchronize()
    assert int(outs["count_ptr"][:8].sum()) == 12 and bool((outs["count_ptr"][8:] == IFILL).all()) and bool((outs["label_ptr"] == IFILL).all())
    for x in (h, rc, big):
        x.close()


def test_predict_modes_finds_the_two_planted_modes(torch_cuda, monkeypatch):
    torch = torch_cuda
    from desire_amd import evaluate as E
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    a = E.build_parser().parse_args(_FLAGS)
    m = DESIREModel(a, seed=4)
    video = _video()
    past, _ = split_windows([video[i * 10 + 20:i * 10 + 30] for i in range(2)], a.seq_length)
    # the model's own forward: shapes, and the samples stay available
    out = m.predict_modes(past, modes=2, seeds="score", iters=4, seed=3, device_rng=True)
    d = m._handle(2, False).dims
    K, T, mno = d.K, d.T_pred, d.mno
    assert sorted(out) == ["count", "cov", "label", "mean", "passes", "present", "prob"]
    assert tuple(out["mean"].shape) == (2, mno, 2, T, 2) and tuple(out["cov"].shape) == (2, mno, 2, T, 3) and tuple(out["label"].shape) == (2, mno, K)
    assert tuple(m.final_output.shape) == (2, K, mno, T, 2) and bool((out["count"].sum(-1) == K).all())
    np.testing.assert_allclose(out["prob"].sum(-1).cpu().numpy(), 1.0, atol=1e-6)
    assert bool((out["cov"][..., :2][out["prob"] > 0] >= 1.0).all())       # min_std = 1 px: the floor on the variances of a mode with mass
    # a planted scene in place of the forward: per agent three samples around one straight track and two around another, equal scores
    t = np.arange(1, T + 1, dtype=np.float32)
    centre = np.zeros((2, mno, 2, T, 2), np.float32)                      # pixels
    for w in range(2):
        for s in range(mno):
            centre[w, s, 0] = np.stack([300 + 40 * s + 6 * t, 200 + 30 * w + 2 * t], -1)
            centre[w, s, 1] = np.stack([300 + 40 * s - 3 * t, 200 + 30 * w + 9 * t], -1)
    off = np.array([[1.0, -0.5], [-2.0, 1.5], [1.0, -1.0], [0.75, 0.25], [-0.75, -0.25]], np.float32)       # sums to zero within each mode
    of_mode = [0, 0, 0, 1, 1]
    Ypx = np.stack([centre[:, :, of_mode[k]] + off[k] for k in range(K)], 1)                                # [2, K, mno, T, 2]
    Yn = torch.as_tensor(Ypx * np.array([d.sx, d.sy], np.float32), device="cuda").contiguous()
    flat = torch.zeros((2, K, mno), device="cuda")
    monkeypatch.setattr(m, "forward_device", lambda *args, **kw: (Yn, flat))
    out = m.predict_modes(past, modes=2, seeds="nms", nms_radius=8.0, iters=8, min_std=0.5)
    assert bool((out["label"] == torch.tensor(of_mode, device="cuda", dtype=torch.int32)).all()) and bool((out["passes"] == 1).all())
    np.testing.assert_allclose(out["prob"].cpu().numpy(), np.broadcast_to(np.array([0.6, 0.4], np.float32), (2, mno, 2)), atol=1e-6)
    np.testing.assert_allclose(out["prob"].sum(-1).cpu().numpy(), 1.0, atol=1e-6)
    np.testing.assert_allclose(out["mean"].cpu().numpy(), centre, atol=2e-3)                                 # pixels
    want = np.stack([(off[:3] ** 2).mean(0), (off[3:] ** 2).mean(0)]) + 0.25                                 # [mode, (xx, yy)] px^2
    np.testing.assert_allclose(out["cov"][..., :2].cpu().numpy(), np.broadcast_to(want[None, None, :, None, :], (2, mno, 2, T, 2)), rtol=2e-3)
    # seeds by score alone: samples 0 and 1 share a mode, and the iteration still separates the two tracks
    both = m.predict_modes(past, modes=2, seeds="score", iters=8, min_std=0.5)
    assert bool((both["count"].sort(-1).values == torch.tensor([2, 3], device="cuda", dtype=torch.int32)).all())
    for kw, word in ((dict(modes=0), "modes"), (dict(modes=6), "modes"), (dict(seeds="best"), "seeds"), (dict(seeds="nms"), "nms_radius"),
                     (dict(iters=33, seeds="score"), "iters"), (dict(min_std=-1.0, seeds="score"), "min_std"), (dict(weights="best", seeds="score"), "weights"),
                     (dict(horizon=9, seeds="score"), "horizon")):
        with pytest.raises(ValueError, match=word):
            m.predict_modes(past, **dict(dict(modes=2), **kw))


def test_evaluate_modes_and_the_evaluation_walk(torch_cuda):
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
    d = m._handle(2, False).dims
    hz, n = [2, 4, 6], 2
    got = m.evaluate_modes(Y, score, fut, modes=n, seeds="score", iters=4, min_std=0.5, weights="uniform", horizons=hz, units="px")
    assert sorted(got) == ["best", "count", "nll", "passes", "prob", "top1"]
    # the same call in numpy: equal weights, so the fit is the fp32 statement's bit for bit, and the errors follow from its means
    Yn, sn = Y.cpu().numpy().reshape(d.R, d.T_pred, 2), score.cpu().numpy()
    futn = m._pad_windows(fut, d.mno).cpu().numpy()
    order = np.argsort(-sn.transpose(0, 2, 1).reshape(d.A, d.K), 1, kind="stable").astype(np.int32)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    f32 = modes_f32(Yn, order, None, futn, n, d.T_pred, 4, ux, uy, 0.25, d, hz)
    np.testing.assert_array_equal(got["count"], f32["count"])
    np.testing.assert_array_equal(got["prob"].view(np.uint32), f32["prob"].view(np.uint32))
    np.testing.assert_array_equal(got["passes"], f32["passes"])
    np.testing.assert_allclose(got["nll"], f32["out"], rtol=0, atol=2e-3)
    f = futn.transpose(0, 2, 1, 3).reshape(d.A, d.T_pred, 3)
    g = np.stack([f[..., 1] * np.float32(d.sx), f[..., 2] * np.float32(d.sy)], -1)
    e = np.sqrt((((f32["mean"] - g[:, None]) * np.array([ux, uy], np.float32)) ** 2).sum(-1))                 # [A, n, T] pixels
    for i, x in enumerate(hz):
        for ag in range(d.A):
            ts = np.nonzero(f[ag, :x, 0])[0]
            if ts.size == 0:
                assert not got["top1"][ag, i].any() and not got["best"][ag, i].any() and not got["nll"][ag, i].any()
                continue
            alive = f32["prob"][ag] > 0
            ade, fde = e[ag][:, ts].mean(1), e[ag][:, ts[-1]]
            top = int(np.argmax(f32["prob"][ag]))
            np.testing.assert_allclose(got["top1"][ag, i], [ade[top], fde[top]], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(got["best"][ag, i], [ade[alive].min(), fde[alive].min()], rtol=1e-4, atol=1e-4)
    assert (got["best"] <= got["top1"] + 1e-6).all() and got["top1"].max() > 0
    res = {}
    for tag, extra in (("plain", []), ("nms", ["--modes", "3", "--nms_radius", "20"]), ("score", ["--modes", "2", "--modes_seeds", "score", "--modes_iters", "2"])):
        a = E.build_parser().parse_args(_FLAGS + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=DESIREModel(a, seed=4))
    assert list(res["plain"]) == _PLAIN_KEYS                           # without the flag: the result it has always been
    plain_text = json.dumps(res["plain"], indent=1)
    nh = len(res["plain"]["horizons"])
    for tag in ("nms", "score"):
        blk = res[tag].pop("modes")
        assert json.dumps(res[tag], indent=1) == plain_text            # ... and with it, the same result plus one block
        assert set(blk) == {"n", "seeds", "iters", "min_std_px", "log_floor", "mean_passes", "nll", "top1", "best"}
        assert len(blk["nll"]["mean"]) == len(blk["nll"]["final"]) == len(blk["top1"]["ade"]) == len(blk["best"]["fde"]) == nh
        assert all(b <= t + 1e-9 for b, t in zip(blk["best"]["ade"], blk["top1"]["ade"])) and all(np.isfinite(blk["nll"]["mean"]))
