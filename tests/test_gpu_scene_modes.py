"""n scene modes with covariances fitted to a window's K joint futures on the device (desire_fit_scene_modes, csrc/kernels_scene_modes.hip) against
the numpy statements of its contract (tests/scene_modes_reference.py).  Labels, counts and pass counts are compared exactly with scene_modes_f32
AND scene_modes_f64 -- on inputs whose float64 fit keeps a relative margin of 1e-3 between a world's best and second-best distance in every
assign, asserted first on the float64 pass alone; mean, prob and cov with scene_modes_f32 bit for bit where every weight is 1 / K (NULL scores),
and within the derived bounds of scene_modes_f64 under the planted scores (scene_bounds).  The likelihood follows test_gpu_kde.py's rule: the bar
is four times the fp32 statement's own distance from scene_modes_f64, never below 1e-5.  Then the anchor (one slot: desire_fit_modes' bits), the
exact properties, independence and reproducibility, alignment, the optional outputs, a forced small slot chunk, capture, refused arguments, and
the calls through DESIREModel and the command line.

Observed on an MI355X: see DESIGN.md section 7l."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import (EVAL_FLAGS as _FLAGS, PLAIN_KEYS as _PLAIN_KEYS, walking_video as _video, _same_bits as _same_bits_of,
                           _likelihood, _t, _within, at_byte_offset, make_case, small_dims)
from tests.scene_modes_reference import (ITERS, LOG_FLOOR, MARGIN, SHAPES, case, scene_bounds, scene_modes_f32, scene_modes_f64, t_ends)

pytestmark = pytest.mark.gpu
FILL, IFILL = -7.0, -77
FIT = ("label", "count", "prob", "mean", "cov", "passes")
ALL = FIT + ("out", "frame")
IDS = lambda s: "n%d_m%d_K%d_T%d_n%d" % s


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _ref(c, fn, scored, iters=ITERS, vf=None, **over):
    """A reference of the case at other settings (or on changed inputs: over), computed on first use."""
    key = (fn.__name__, scored, iters, vf) + tuple(sorted(over))
    if over or key not in c.setdefault("refs", {}):
        x = dict(c, **over)
        r = fn(x["Y"], x["present"], x["worder"], x["wscore"] if scored else None, x["fut"], c["n"], c["t_end"], iters, c["ux"], c["uy"],
               c["vf"] if vf is None else vf, c["d"], c["hz"])
        if over:
            return r
        c["refs"][key] = r
    return c["refs"][key]


def _call(torch, h, d, n, Y_t, pres_t, wo_t, ws_t, fut_t, t_end, iters, ux, uy, vf, hz, want=ALL, stream=0, log_floor=LOG_FLOOR):
    N, K, T, m = d.n_scenes, d.K, d.T_pred, d.mno
    i32 = torch.int32
    buf = {"label": torch.full((N, K), IFILL, device="cuda", dtype=i32), "count": torch.full((N, n), IFILL, device="cuda", dtype=i32),
           "prob": torch.full((N, n), FILL, device="cuda"), "mean": torch.full((N, n, m, T, 2), FILL, device="cuda"),
           "cov": torch.full((N, n, m, T, 3), FILL, device="cuda"), "passes": torch.full((N,), IFILL, device="cuda", dtype=i32),
           "out": torch.full((N, len(hz), 2), FILL, device="cuda"), "frame": torch.full((N, T), FILL, device="cuda")}
    ptr = lambda k: buf[k].data_ptr() if k in want else 0
    fp = fut_t is not None
    h.fit_scene_modes(Y_t.data_ptr(), pres_t.data_ptr() if pres_t is not None else 0, wo_t.data_ptr(), ws_t.data_ptr() if ws_t is not None else 0, n,
                      t_end, iters, ux, uy, vf, buf["count"].data_ptr(), buf["prob"].data_ptr(), ptr("label"), ptr("mean"), ptr("cov"), ptr("passes"),
                      fut_t.data_ptr() if fp else 0, hz if fp else None, log_floor, ptr("out") if fp else 0, ptr("frame") if fp else 0, stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in buf.items()}


def _run(torch, h, c, scored, iters=ITERS, vf=None, fut=True, **kw):
    over = {k: kw.pop(k) for k in ("Y", "present", "worder", "wscore") if k in kw}
    x = dict(c, **over)
    return _call(torch, h, c["d"], c["n"], _t(torch, x["Y"]), _t(torch, x["present"]), _t(torch, x["worder"]),
                 _t(torch, x["wscore"]) if scored else None, _t(torch, c["fut"]) if fut else None, c["t_end"], iters, c["ux"], c["uy"],
                 c["vf"] if vf is None else vf, c["hz"], **kw)


def _same_bits(a, b, keys=ALL, rows=slice(None)):                  # this file's default: every output; rows of both sides
    _same_bits_of(a, b, keys, rows, rows)


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_everything_matches_the_reference(torch_cuda, shape, unit):
    torch = torch_cuda
    from desire_amd import _lib
    h = None
    for te in t_ends(shape[3]):
        c = case(shape, unit, te)
        d = c["d"]
        h = h or _lib.Handle(d)
        for scored in (True, False):
            tag = "scored" if scored else "uniform"
            f32, f64 = c[tag]["f32"], c[tag]["f64"]
            assert f64["margin"].min() > MARGIN                            # the float64 pass alone, before any comparison
            got = _run(torch, h, c, scored)
            for key in ("label", "count", "passes"):
                np.testing.assert_array_equal(got[key], f32[key], err_msg=key)
                np.testing.assert_array_equal(got[key], f64[key], err_msg=key)
            if scored:
                for key, bound in zip(("prob", "mean", "cov"), scene_bounds(c["Y"], f64, c["ux"], c["uy"], c["vf"], d)):
                    gap, worst = _within(got[key], f64[key], bound, key)
                    base, _ = _within(f32[key], f64[key], bound, key)
                    print("t_end %d %s: max |dev - f64| = %.3g (%.3g of its bound), |f32 - f64| = %.3g" % (te, key, gap, worst, base))
                    assert worst <= 1.0, key
            else:                                                          # every weight 1 / K: the bits of the fp32 statement
                _same_bits(got, f32, keys=("prob", "mean", "cov"))
            _likelihood(got, f32, f64, "t_end %d %s" % (te, tag))
            gone = c["present"].reshape(d.n_scenes, d.mno) == 0            # the slots that do not take part: zeros, whatever their rows hold
            assert not got["mean"].transpose(0, 2, 1, 3, 4)[gone].any() and not got["cov"].transpose(0, 2, 1, 3, 4)[gone].any()
    h.close()


def test_one_slot_has_the_bits_of_fit_modes(torch_cuda):
    """The anchor on the device: at mno = 1 with the slot present every output equals desire_fit_modes' given the same order row, the agent's
    scores and the same targets."""
    torch = torch_cuda
    from desire_amd import _lib
    for unit in (0, 1):
        for te in t_ends(SHAPES[1][3]):
            c = case(SHAPES[1], unit, te)
            d, n = c["d"], c["n"]
            here = np.nonzero(c["present"])[0]
            assert d.mno == 1 and here.size >= 2 and 1 in c["info"]["bad"]
            h = _lib.Handle(d)
            for scored in (True, False):
                mine = _run(torch, h, c, scored)
                A, K, T = d.A, d.K, d.T_pred
                i32 = torch.int32
                buf = {"label": torch.zeros((A, K), device="cuda", dtype=i32), "count": torch.zeros((A, n), device="cuda", dtype=i32),
                       "prob": torch.zeros((A, n), device="cuda"), "mean": torch.zeros((A, n, 1, T, 2), device="cuda"),
                       "cov": torch.zeros((A, n, 1, T, 3), device="cuda"), "passes": torch.zeros((A,), device="cuda", dtype=i32),
                       "out": torch.zeros((A, len(c["hz"]), 2), device="cuda"), "frame": torch.zeros((A, T), device="cuda")}
                Y_t, o_t, s_t, f_t = _t(torch, c["Y"]), _t(torch, c["worder"]), _t(torch, c["wscore"]), _t(torch, c["fut"])
                h.fit_modes(Y_t.data_ptr(), o_t.data_ptr(), s_t.data_ptr() if scored else 0, n, te, ITERS, c["ux"], c["uy"], c["vf"],
                            buf["count"].data_ptr(), buf["prob"].data_ptr(), buf["label"].data_ptr(), buf["mean"].data_ptr(), buf["cov"].data_ptr(),
                            buf["passes"].data_ptr(), f_t.data_ptr(), c["hz"], LOG_FLOOR, buf["out"].data_ptr(), buf["frame"].data_ptr())
                torch.cuda.synchronize()
                _same_bits(mine, {k: v.cpu().numpy() for k, v in buf.items()}, rows=here)
            h.close()


def test_the_exact_properties(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    shape = (4, 64, 20, 12, 6)                                             # several chunks; windows of 3, 0 (BAD), 2 and 1 passes
    c = case(shape, 1)
    d, n, K, T = c["d"], c["n"], c["d"].K, c["d"].T_pred
    sp, em = c["info"]["special"], c["info"]["empty"]
    h = _lib.Handle(d)
    base = _run(torch, h, c, False)
    assert 2 <= base["passes"].max() < ITERS
    # iters = 0: the weighted means of the seeds' Voronoi cells; iters = 1: the labels of that pass
    zero = _run(torch, h, c, False, iters=0)
    _same_bits(zero, _ref(c, scene_modes_f32, False, iters=0), keys=FIT)
    assert (zero["passes"] == 0).all() and (zero["label"] != base["label"]).any()
    one = _run(torch, h, c, False, iters=1)
    _same_bits(one, _ref(c, scene_modes_f32, False, iters=1), keys=FIT)
    assert (np.delete(one["passes"], c["info"]["bad"]) == 1).all()
    # more passes than the convergence point needs: the converged bits
    _same_bits(_run(torch, h, c, False, iters=32), base)
    _same_bits(_run(torch, h, c, True, iters=32), _run(torch, h, c, True))
    # a score that is not finite: the window falls back to 1 / K, the bits of the call without scores
    plain = [w for w in range(d.n_scenes) if w not in [sp, em] + c["info"]["bad"]][0]
    assert np.isfinite(c["wscore"][plain]).all()
    ws = np.array(c["wscore"]); ws[plain, 1] = np.inf
    _same_bits(_run(torch, h, c, True, wscore=ws), base, rows=[plain])
    # the assignment looks at t < t_end only: a NaN behind it stays out of the labels and shows in that frame's mean and covariance alone
    te = T // 2
    ce = case(shape, 1, te)
    k = int(ce["worder"][sp, 0])
    slot = int(np.nonzero(ce["present"].reshape(d.n_scenes, d.mno)[sp])[0][0])
    Yn = np.array(ce["Y"]).reshape(d.n_scenes, K, d.mno, T, 2)
    Yn[sp, k, slot, te + (T - te) // 2, 0] = np.nan
    Yn = Yn.reshape(d.R, T, 2)
    got = _run(torch, h, ce, False, Y=Yn)
    f32 = _ref(ce, scene_modes_f32, False, Y=Yn)
    _same_bits(got, f32, keys=FIT)
    np.testing.assert_array_equal(got["label"], _ref(ce, scene_modes_f64, False, Y=Yn)["label"])
    np.testing.assert_array_equal(got["label"], ce["uniform"]["f32"]["label"])          # the labels of the inputs without it
    i = got["label"][sp, k]
    assert i >= 0 and np.isnan(got["mean"][sp, i, slot]).any() and not np.isnan(got["mean"][sp, i, slot, :te]).any()
    assert not np.isnan(np.delete(got["mean"][sp, i], slot, 0)[np.delete(ce["present"].reshape(d.n_scenes, d.mno)[sp], slot) != 0]).any()
    # the NaN world: label -1, as a seed or not; its mass is missing
    w, kn, _ = c["info"]["nan"]
    assert base["label"][w, kn] == -1 and base["count"][w].sum() == K - 1 and base["prob"][w].sum() < 1 - 0.5 / K
    # var_floor = 0: a mode of one member world has no spread in any agent and is left out of the likelihood
    flat = _run(torch, h, c, False, vf=0.0)
    f32, f64 = _ref(c, scene_modes_f32, False, vf=0.0), _ref(c, scene_modes_f64, False, vf=0.0)
    _same_bits(flat, f32, keys=FIT)
    single = flat["count"] == 1
    assert single.any() and np.abs(flat["cov"][single]).max() <= (2.0 ** -22 * c["ux"]) ** 2
    _likelihood(flat, f32, f64, "var_floor 0")
    # the window with nobody taking part runs the same sequence: every D is 0.f, every world joins mode 0, the fit stops at p = 1
    assert (base["label"][em] == 0).all() and base["passes"][em] == 1 and base["count"][em].tolist() == [K] + [0] * (n - 1)
    assert not base["mean"][em].any() and not base["cov"][em].any() and not base["frame"][em].any() and not base["out"][em].any()
    np.testing.assert_array_equal(base["prob"][em].view(np.uint32), c["uniform"]["f32"]["prob"][em].view(np.uint32))
    # a BAD order row: an index out of range among the first n entries
    bad = _run(torch, h, c, True, worder=c["info"]["bad_order"])
    _same_bits(bad, _ref(c, scene_modes_f32, True, worder=c["info"]["bad_order"]), keys=("label", "count", "passes"))
    assert (bad["label"][sp] == -1).all() and not bad["count"][sp].any() and not bad["prob"][sp].any() and not bad["mean"][sp].any()
    assert not bad["cov"][sp].any() and bad["passes"][sp] == 0
    part = c["present"].reshape(d.n_scenes, d.mno)[sp] != 0
    counted = ((c["fut"][sp, :, :, 0] != 0) & part[None]).any(1)
    assert (bad["frame"][sp][counted] == np.float32(LOG_FLOOR)).all() and not bad["frame"][sp][~counted].any()
    good = np.setdiff1d(np.arange(d.n_scenes), [sp])
    _same_bits(bad, _run(torch, h, c, True), rows=good)
    h.close()


def test_results_are_bitwise_reproducible_and_depend_on_the_window_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    for shape in ((4, 8, 5, 7, 3), (4, 64, 20, 12, 6)):
        c = case(shape, 1)
        d, n = c["d"], c["n"]
        h = _lib.Handle(d)
        hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
        h2 = _lib.Handle(d.replace(n_scenes=2))
        ref = _run(torch, h, c, True)
        assert ref["passes"].max() >= 1
        _same_bits(_run(torch, h, c, True), ref)                            # run to run
        _same_bits(_run(torch, hc, c, True), ref)                           # the padding-skipping flags are not its business
        Yw = c["Y"].reshape(d.n_scenes, d.K * d.mno, d.T_pred, 2)
        pw = c["present"].reshape(d.n_scenes, d.mno)
        for rows in ([0, 1], [2, 0], [3, 2]):                               # any two windows, in any place of a batch of two
            got = _call(torch, h2, h2.dims, n, _t(torch, Yw[rows]), _t(torch, pw[rows]), _t(torch, c["worder"][rows]), _t(torch, c["wscore"][rows]),
                        _t(torch, c["fut"][rows]), c["t_end"], ITERS, c["ux"], c["uy"], c["vf"], c["hz"])
            _same_bits(got, {k: v[rows] for k, v in ref.items()})
        for off in (8, 4):                                                  # Y off 16-byte alignment: the streamer's 8- and 4-byte loads
            got = _call(torch, h, d, n, at_byte_offset(_t(torch, c["Y"]), off), _t(torch, c["present"]), _t(torch, c["worder"]), _t(torch, c["wscore"]),
                        _t(torch, c["fut"]), c["t_end"], ITERS, c["ux"], c["uy"], c["vf"], c["hz"])
            _same_bits(got, ref)
        for x in (h, hc, h2):
            x.close()


def test_a_forced_small_slot_chunk_has_the_bits_of_the_natural_one(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    for shape in (SHAPES[0], SHAPES[2], SHAPES[3]):
        c = case(shape, 1)
        h = _lib.Handle(c["d"])
        ref = _run(torch, h, c, True)
        for chunk in (1, 3):
            h.set_option("scene_modes_chunk", chunk)
            _same_bits(_run(torch, h, c, True), ref)
        h.set_option("scene_modes_chunk", 0)
        _same_bits(_run(torch, h, c, True), ref)
        h.close()


def test_every_subset_of_the_optional_outputs(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    c = case(SHAPES[0], 0)
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
    nopres = _run(torch, h, c, True, present=None)                          # NULL presence: every slot takes part, the garbage too
    allp = _ref(c, scene_modes_f32, True, present=np.ones_like(c["present"]))
    np.testing.assert_array_equal(nopres["label"], allp["label"])
    h.close()


def test_forward_joint_metrics_select_worlds_and_fit_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=6, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    n, hz = 3, [3, 6, 12]
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    i32 = torch.int32
    a, b = make_case(d, seed=21, n_absent=2), make_case(d, seed=22, n_absent=3)
    p, f, e, g = (_t(torch, x) for x in a[:4])
    h = _lib.Handle(d); h.set_weights(w); h.set_scene_grids(g.data_ptr(), a[4])
    N, K, T, m = d.n_scenes, d.K, d.T_pred, d.mno
    Y = torch.zeros((d.R, T, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    pres = torch.zeros((d.A,), device="cuda", dtype=torch.uint8)
    cnt = torch.zeros((N, K + 1, 1, 2), device="cuda", dtype=i32)
    js = torch.zeros((N, K), device="cuda"); jo = torch.zeros((N, K), device="cuda", dtype=i32)
    wo = torch.zeros_like(jo); wc = torch.zeros((N,), device="cuda", dtype=i32)
    label = torch.zeros((N, K), device="cuda", dtype=i32); count = torch.zeros((N, n), device="cuda", dtype=i32)
    prob = torch.zeros((N, n), device="cuda"); mean = torch.zeros((N, n, m, T, 2), device="cuda")
    cov = torch.zeros((N, n, m, T, 3), device="cuda"); passes = torch.zeros((N,), device="cuda", dtype=i32)
    out = torch.zeros((N, 3, 2), device="cuda"); frame = torch.zeros((N, T), device="cuda")
    bufs = (Y, sc, js, jo, wo, wc, label, count, prob, mean, cov, passes, out, frame)
    side = torch.cuda.Stream(); sp = side.cuda_stream

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.joint_metrics(Y.data_ptr(), 0, pres.data_ptr(), sc.data_ptr(), [T], 1, 0.0, ux, uy, cnt.data_ptr(), jo.data_ptr(), 0, 0, js.data_ptr(), 0, sp)
        h.select_worlds(Y.data_ptr(), pres.data_ptr(), js.data_ptr(), _lib.DIST_FINAL, _lib.WORLD_MEAN, T, 1e-3, ux, uy, wo.data_ptr(), wc.data_ptr(), 0, 0, sp)
        h.fit_scene_modes(Y.data_ptr(), pres.data_ptr(), wo.data_ptr(), js.data_ptr(), n, T, ITERS, ux, uy, 0.25, count.data_ptr(), prob.data_ptr(),
                          label.data_ptr(), mean.data_ptr(), cov.data_ptr(), passes.data_ptr(), f.data_ptr(), hz, LOG_FLOOR, out.data_ptr(), frame.data_ptr(), sp)

    def load(cs):
        p.copy_(_t(torch, cs[0])); f.copy_(_t(torch, cs[1])); e.copy_(_t(torch, cs[2]))      # in place: the graph keeps its pointers
        pres.copy_((p[:, -1, :, 0] != 0).reshape(-1).to(torch.uint8))

    torch.cuda.synchronize()
    ref = {}
    for tag, cs in (("b", b), ("a", a)):                          # eager calls (the first also warms lazy allocations up outside capture)
        load(cs)
        torch.cuda.synchronize()
        calls()
        side.synchronize()
        ref[tag] = [x.clone() for x in bufs]
    assert not torch.equal(ref["a"][9], ref["b"][9])
    h.graph_begin(sp)
    calls()
    gid = h.graph_end(sp)
    for rep in range(4):
        tag, cs = ("b", b) if rep % 2 == 0 else ("a", a)
        load(cs)
        for x in bufs:
            x.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        for x, r in zip(bufs, ref[tag]):
            assert torch.equal(x.view(i32) if x.dtype != torch.uint8 else x, r.view(i32) if r.dtype != torch.uint8 else r), (rep, tag)
    # the captured fit is the contract's on the captured forward's samples (equal weights: the bits of the fp32 statement)
    load(a)
    flat = torch.zeros_like(prob)
    h.fit_scene_modes(ref["a"][0].data_ptr(), pres.data_ptr(), ref["a"][4].data_ptr(), 0, n, T, ITERS, ux, uy, 0.25, count.data_ptr(), flat.data_ptr(),
                      label.data_ptr())
    torch.cuda.synchronize()
    want = scene_modes_f32(ref["a"][0].cpu().numpy(), pres.cpu().numpy(), ref["a"][4].cpu().numpy(), None, None, n, T, ITERS, ux, uy, 0.25, d)
    np.testing.assert_array_equal(label.cpu().numpy(), want["label"])
    np.testing.assert_array_equal(flat.cpu().numpy().view(np.uint32), want["prob"].view(np.uint32))
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=1, mno=4, K=3, T_obs=4, T_pred=6, n_grids=1, H=64)
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") + 0.5
    od = torch.arange(3, device="cuda", dtype=torch.int32).contiguous()
    pr = torch.ones(4, device="cuda", dtype=torch.uint8)
    i32 = torch.int32
    outs = {"label_ptr": torch.full((64,), IFILL, device="cuda", dtype=i32), "count_ptr": torch.full((64,), IFILL, device="cuda", dtype=i32),
            "prob_ptr": torch.full((64,), FILL, device="cuda"), "mean_ptr": torch.full((512,), FILL, device="cuda"),
            "cov_ptr": torch.full((512,), FILL, device="cuda"), "passes_ptr": torch.full((64,), IFILL, device="cuda", dtype=i32),
            "out_ptr": torch.full((64,), FILL, device="cuda"), "frame_ptr": torch.full((64,), FILL, device="cuda")}
    nan, inf = float("nan"), float("inf")
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(worder_ptr=0), "dev_worder"), (dict(count_ptr=0), "dev_count"), (dict(prob_ptr=0), "dev_prob"),
             (dict(n_modes=0), "n_modes"), (dict(n_modes=4), "n_modes"), (dict(n_modes=17), "n_modes"), (dict(t_end=0), "t_end"), (dict(t_end=7), "t_end"),
             (dict(iters=-1), "iters"), (dict(iters=33), "iters"),
             (dict(unit_x=0.0), "unit_x"), (dict(unit_x=nan), "unit_x"), (dict(unit_x=inf), "unit_x"), (dict(unit_y=-2.0), "unit_y"), (dict(unit_y=nan), "unit_y"),
             (dict(var_floor=-1e-9), "var_floor"), (dict(var_floor=nan), "var_floor"), (dict(var_floor=inf), "var_floor"),
             (dict(log_floor=nan), "log_floor"), (dict(log_floor=-inf), "log_floor"),
             (dict(horizons=[]), "n_h"), (dict(horizons=list(range(1, 10))), "n_h"), (dict(horizons=[0]), "host_horizons"), (dict(horizons=[7]), "host_horizons"),
             (dict(horizons=[3, 3]), "increasing"), (dict(horizons=None), "host_horizons"),
             (dict(fut_ptr=0), "dev_out needs dev_fut"), (dict(fut_ptr=0, out_ptr=0), "dev_frame needs dev_fut"), (dict(out_ptr=0), "dev_out is NULL")]
    for kw, word in cases:
        args = dict(yhat_ptr=z.data_ptr(), present_ptr=pr.data_ptr(), worder_ptr=od.data_ptr(), wscore_ptr=z.data_ptr(), n_modes=2, t_end=6, iters=4,
                    unit_x=1.0, unit_y=1.0, var_floor=0.0, fut_ptr=z.data_ptr(), horizons=[2, 6], log_floor=LOG_FLOOR,
                    **{k: v.data_ptr() for k, v in outs.items()})
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.fit_scene_modes(**args)
    lib = _lib.load()
    one, zero = C.c_float(1), C.c_float(0)
    o = {k: v.data_ptr() for k, v in outs.items()}
    assert lib.desire_fit_scene_modes(None, z.data_ptr(), None, od.data_ptr(), None, None, 2, 6, 4, one, one, zero, None, 0, zero, None, o["count_ptr"],
                                      o["prob_ptr"], None, None, None, None, None, None) == -1
    assert b"handle" in lib.desire_last_error()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.fit_scene_modes(z.data_ptr(), 0, od.data_ptr(), 0, 1, 8, 4, 1.0, 1.0, 0.0, o["count_ptr"], o["prob_ptr"])
    big = _lib.Handle(small_dims(n_scenes=1, mno=1, K=40, T_obs=4, T_pred=200, n_grids=1, H=64))      # 8 * 56 * 201 alone > 61440: beyond the LDS plan
    with pytest.raises(_lib.DesireError, match=r"error -1.*LDS.*8 \* \(K \+ n_modes\) \* \(T_pred \| 1\).*61440"):
        big.fit_scene_modes(z.data_ptr(), 0, od.data_ptr(), 0, 16, 200, 4, 1.0, 1.0, 0.0, o["count_ptr"], o["prob_ptr"])
    with pytest.raises(_lib.DesireError, match="error -1.*scene_modes_chunk"):
        h.set_option("scene_modes_chunk", -1)
    torch.cuda.synchronize()
    assert all(bool((v == (IFILL if v.dtype == i32 else FILL)).all()) for v in outs.values())
    # ... and the handle still works
    h.fit_scene_modes(z.data_ptr(), pr.data_ptr(), od.data_ptr(), 0, 2, 6, 4, 1.0, 1.0, 0.0, o["count_ptr"], o["prob_ptr"])
    torch.cuda.synchronize()
    assert int(outs["count_ptr"][:2].sum()) == 3 and bool((outs["count_ptr"][2:] == IFILL).all()) and bool((outs["label_ptr"] == IFILL).all())
    for x in (h, rc, big):
        x.close()


def test_predict_scene_modes_hands_out_the_documented_tensors(torch_cuda):
    torch = torch_cuda
    from desire_amd import evaluate as E
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    a = E.build_parser().parse_args(_FLAGS)
    m = DESIREModel(a, seed=4)
    video = _video()
    past, _ = split_windows([video[i * 10 + 20:i * 10 + 30] for i in range(2)], a.seq_length)
    calls = []
    forward = m.forward_device
    m.forward_device = lambda *args, **kw: calls.append(1) or forward(*args, **kw)
    for kw, word in ((dict(modes=0), "modes"), (dict(modes=6), "modes"), (dict(seeds="nms"), "seeds"), (dict(seeds="worlds"), "worlds_radius"),
                     (dict(iters=33, seeds="score"), "iters"), (dict(min_std=-1.0, seeds="score"), "min_std"), (dict(weights="best", seeds="score"), "weights"),
                     (dict(horizon=9, seeds="score"), "horizon"), (dict(seeds="score", worlds_radius=5.0), "seeds='worlds'"),
                     (dict(seeds="score", collision_penalty=1.0), "seeds='worlds'"), (dict(seeds="score", collision_radius=-1.0), "collision_radius"),
                     (dict(worlds_radius=5.0, worlds_reduce="some"), "worlds_reduce")):
        with pytest.raises(ValueError, match=word):
            m.predict_scene_modes(past, **dict(dict(modes=2), **kw))
    assert not calls                                                     # refused before the forward runs
    d = m._handle(2, False).dims
    K, T, mno = d.K, d.T_pred, d.mno
    for kw in (dict(seeds="score", iters=4), dict(seeds="worlds", worlds_radius=8.0, collision_radius=10.0, collision_penalty=0.5, horizon=4),
               dict(seeds="worlds", worlds_radius=8.0, worlds_metric="mean", worlds_reduce="all", weights="uniform")):
        out = m.predict_scene_modes(past, modes=2, seed=3, device_rng=True, **kw)
        assert sorted(out) == ["count", "cov", "label", "mean", "passes", "present", "prob"]
        assert tuple(out["mean"].shape) == (2, 2, mno, T, 2) and tuple(out["cov"].shape) == (2, 2, mno, T, 3) and tuple(out["label"].shape) == (2, K)
        assert tuple(out["prob"].shape) == tuple(out["count"].shape) == (2, 2) and tuple(out["passes"].shape) == (2,)
        assert tuple(out["present"].shape) == (2, mno) and tuple(m.final_output.shape) == (2, K, mno, T, 2)
        assert bool((out["count"].sum(-1) == K).all())
        np.testing.assert_allclose(out["prob"].sum(-1).cpu().numpy(), 1.0, atol=1e-6)
        here = out["present"][:, None, :].expand(2, 2, mno) & (out["prob"] > 0)[:, :, None]
        assert bool((out["cov"][..., :2][here] >= 1.0).all())              # min_std = 1 px: the floor on the variances of a mode with mass
        assert not bool(out["cov"].permute(0, 2, 1, 3, 4)[~out["present"]].any()) and not bool(out["mean"].permute(0, 2, 1, 3, 4)[~out["present"]].any())
    assert len(calls) == 3


def test_evaluate_scene_modes_on_the_planted_case_and_the_evaluation_walk(torch_cuda):
    torch = torch_cuda
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    from tests.scored_surface_cases import HZ, N, planted
    past, fut, Yp, score, _, _ = planted()
    a = E.build_parser().parse_args(_FLAGS)
    m = DESIREModel(a, seed=4)
    m._handle(N, False)
    Y, st = torch.as_tensor(Yp, device="cuda"), torch.as_tensor(score, device="cuda")
    d = m._handle(N, False).dims
    n, K, T = 3, d.K, d.T_pred
    got = m.evaluate_scene_modes(Y, st, list(fut), modes=n, seeds="score", iters=4, min_std=0.5, weights="uniform", horizons=HZ, units="px")
    assert sorted(got) == ["best", "count", "nll", "passes", "prob", "top1"]
    # the same call in numpy: equal weights, so the fit is the fp32 statement's bit for bit, and the joint errors follow from its means
    jm = m.evaluate_joint(Y, st, list(fut), top=n, horizons=HZ, units="px")
    futn = m._pad_windows(list(fut), d.mno).cpu().numpy()
    part = (futn[..., 0] != 0).any(1)                                      # [N, mno]
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    f32 = scene_modes_f32(Yp.reshape(d.R, T, 2), part.astype(np.uint8), jm["order"], None, futn, n, T, 4, ux, uy, 0.25, d, HZ)
    np.testing.assert_array_equal(got["count"], f32["count"])
    np.testing.assert_array_equal(got["prob"].view(np.uint32), f32["prob"].view(np.uint32))
    np.testing.assert_array_equal(got["passes"], f32["passes"])
    np.testing.assert_allclose(got["nll"], f32["out"], rtol=0, atol=2e-3)
    assert (got["count"] > 0).sum() >= N + 1 and np.isfinite(got["nll"]).all()
    # half a pixel is far below the planted distance of the truth from either track: every frame sits on the floor; 30 px puts it inside
    wide = m.evaluate_scene_modes(Y, st, list(fut), modes=n, seeds="score", iters=4, min_std=30.0, weights="uniform", horizons=HZ, units="px")
    w32 = scene_modes_f32(Yp.reshape(d.R, T, 2), part.astype(np.uint8), jm["order"], None, futn, n, T, 4, ux, uy, 900.0, d, HZ)
    np.testing.assert_allclose(wide["nll"], w32["out"], rtol=0, atol=2e-3)
    assert (got["nll"] == -LOG_FLOOR).all() and (wide["nll"] < -LOG_FLOOR).all() and (wide["nll"] > 0).all()
    g = np.stack([futn[..., 1] * np.float32(d.sx), futn[..., 2] * np.float32(d.sy)], -1).transpose(0, 2, 1, 3)       # [N, mno, T, 2]
    e = np.sqrt((((f32["mean"] - g[:, None]) * np.array([ux, uy], np.float32)) ** 2).sum(-1))                         # [N, n, mno, T] pixels
    cnt = (futn[..., 0] != 0).transpose(0, 2, 1)                           # [N, mno, T]
    for i, x in enumerate(HZ):
        for w in range(N):
            slots = [s for s in range(d.mno) if cnt[w, s, :x].any()]
            assert slots
            ade = np.mean([[e[w, j, s][np.nonzero(cnt[w, s, :x])[0]].mean() for s in slots] for j in range(n)], 1)
            fde = np.mean([[e[w, j, s][np.nonzero(cnt[w, s, :x])[0][-1]] for s in slots] for j in range(n)], 1)
            alive = f32["prob"][w] > 0
            top = int(np.argmax(f32["prob"][w]))
            np.testing.assert_allclose(got["top1"][w, i], [ade[top], fde[top]], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(got["best"][w, i], [ade[alive].min(), fde[alive].min()], rtol=1e-4, atol=1e-4)
    assert (got["best"] <= got["top1"] + 1e-6).all() and got["top1"].max() > 0
    # with the suppression the seeds are distinct worlds: the two tracks of the planted case
    nms = m.evaluate_scene_modes(Y, st, list(fut), modes=2, seeds="worlds", worlds_radius=20.0, horizons=HZ)
    assert (np.sort(nms["count"], 1) == [2, 3]).all() and (nms["passes"] == 1).all()
    # the evaluation walk: without the flag the result it has always been, with it the same result plus one block
    video = _video()
    res = {}
    for tag, extra in (("plain", []), ("nms", ["--joint_modes", "3", "--joint_radius", "20"]),
                       ("score", ["--joint_modes", "2", "--joint_modes_seeds", "score", "--joint_modes_iters", "2", "--joint_modes_min_std", "0.5"])):
        a = E.build_parser().parse_args(_FLAGS + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=DESIREModel(a, seed=4))
    assert list(res["plain"]) == _PLAIN_KEYS
    plain_text = json.dumps(res["plain"], indent=1)
    nh = len(res["plain"]["horizons"])
    for tag in ("nms", "score"):
        blk = res[tag].pop("joint_modes")
        assert json.dumps(res[tag], indent=1) == plain_text
        assert set(blk) == {"n", "seeds", "iters", "min_std_px", "log_floor", "windows", "mean_passes", "nll", "top1", "best"}
        assert len(blk["nll"]["mean"]) == len(blk["nll"]["final"]) == len(blk["top1"]["jade"]) == len(blk["best"]["jfde"]) == nh
        assert all(b <= t + 1e-9 for b, t in zip(blk["best"]["jade"], blk["top1"]["jade"])) and all(np.isfinite(blk["nll"]["mean"]))
    with pytest.raises(ValueError, match="joint_radius"):                  # refused before a model or a window is touched
        E.evaluate(E.build_parser().parse_args(_FLAGS + ["--joint_modes", "4"]), data_loader=object(), model=object())
