"""KDE log-likelihood on the device (desire_kde_nll, csrc/kernels_kde.hip) against scipy's float64 density (tests/kde_reference.py:
kde_nll_f64).  The bar of a comparison is four times the distance of the fp32 restatement of the contract (kde_nll_f32) from that reference on
the same inputs -- the 4 x covers the device's expf / logf against numpy's -- and never below 1e-5, the ADE / FDE harness's own atol; the code
under test is never its own reference.  Then the exact properties: planted degenerate frames, run to run, batch split, padding flags, capture,
refused arguments, and the call through DESIREModel and the evaluation command line."""
import ctypes as C

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import MISALIGNED_SHAPES, at_byte_offset, make_case, small_dims
from tests.kde_reference import LOG_FLOOR, kde_nll_f32, kde_nll_f64, kde_outputs, make_samples
from tests.rank_reference import planted_scores

pytestmark = pytest.mark.gpu
FILL = -7.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _t(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _leaving(d, seed):
    """tests/test_gpu_rank.py's kind of targets: objects leaving, a track gap, a slot never in the target (where the shape has them)."""
    past, fut, eps, grids, gos = make_case(d, seed=seed, n_absent=min(3, d.mno - 1))
    fut = fut.copy()
    if d.mno >= 8:
        fut[0, 3:, 1] = 0; fut[0, 1:, 4] = 0; fut[0, :, 3] = 0
        fut[1, 2:5, 2] = 0; fut[1, d.T_pred - 1:, 0] = 0; fut[1, :2, 5] = 0
    else:
        fut[0, d.T_pred // 2:, 0] = 0
        if d.n_scenes > 2:
            fut[2, :, 0] = 0
    return past, fut, eps, grids, gos


def _units(d):
    return [(1.0, 1.0), (1.0 / d.sx, 1.0 / d.sy), (0.2 / d.sx, 0.2 / d.sy)]


def _inputs(d, seed=7):
    """(fut, scores, Y, planted, counted): the samples are drawn for the worst of the three units (pixels: the lowest log-density)."""
    _, fut, _, _, _ = _leaving(d, seed)
    s = planted_scores(d, seed + 2)
    Y, planted = make_samples(d, fut, s, seed + 1, worst_log_unit=float(np.log(1.0 / (d.sx * d.sy))))
    counted = (fut[..., 0] != 0).transpose(0, 2, 1).reshape(d.A, d.T_pred)
    return fut, s, Y, planted, counted


def _call(torch, h, d, Y_t, fut_t, s_t, hz, ux, uy, frame=True, floor=LOG_FLOOR, stream=0):
    out = torch.full((d.A, len(hz), 2), FILL, device="cuda")
    fr = torch.full((d.A, d.T_pred), FILL, device="cuda") if frame else None
    h.kde_nll(Y_t.data_ptr(), fut_t.data_ptr(), s_t.data_ptr() if s_t is not None else 0, hz, ux, uy, floor, out.data_ptr(),
              fr.data_ptr() if frame else 0, stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (fr.cpu().numpy() if frame else None)


SHAPES = [dict(n_scenes=2, mno=8, K=5, T_pred=12),           # masks and gaps
          dict(n_scenes=2, mno=8, K=3, T_pred=7),            # odd T_pred
          dict(n_scenes=3, mno=1, K=3, T_pred=7),            # rows off 16-byte alignment
          dict(n_scenes=2, mno=4, K=1, T_pred=5),            # K = 1: all floor
          dict(n_scenes=2, mno=4, K=2, T_pred=5),            # K = 2: two points are collinear
          dict(n_scenes=3, mno=32, K=20, T_pred=40),         # the headline's tiling (six agents per workgroup) and a partial last tile
          dict(n_scenes=2, mno=160, K=130, T_pred=9),        # K beyond the register classes, mno > a wave
          dict(n_scenes=2, mno=32, K=3, T_pred=200)]         # long rows


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "m%d_K%d_T%d" % (s["mno"], s["K"], s["T_pred"]))
def test_log_density_matches_scipy_in_every_unit(torch_cuda, shape):
    torch = torch_cuda
    from desire_amd import _lib
    from desire_amd.model import default_horizons
    d = small_dims(T_obs=4, n_grids=1, H=64, **shape)
    fut, s, Y, planted, counted = _inputs(d)
    T = d.T_pred
    eight = [1, 2, 3, 5, 7, 9, 11, 12] if T >= 12 else list(range(1, min(T, 8) + 1))
    if T > 12:
        eight[-1] = T
    h = _lib.Handle(d)
    Y_t, fut_t, s_t = _t(torch, Y), _t(torch, fut), _t(torch, s)
    free = counted & ~planted
    worst = 0.0
    for score, sc_t in ((None, None), (s, s_t)):
        for ux, uy in _units(d):
            # the float64 reference alone, before any comparison: the inputs are what the bar assumes
            want, shp, raw = kde_nll_f64(Y, fut, score, ux, uy, LOG_FLOOR, d, want_shape=True)
            if d.K >= 3:
                assert (np.abs(raw[free] - LOG_FLOOR) > 0.05).all()
                assert (shp[free] >= 0.05).all()
                assert 0 < planted[counted].sum() <= 0.1 * counted.sum()
                assert (want[free] > LOG_FLOOR).all() and (want[counted & planted] == LOG_FLOOR).all()
            else:                                               # one or two samples: every frame is degenerate, nothing to plant
                assert not planted.any() and (want[counted] == LOG_FLOOR).all()
            f32 = kde_nll_f32(Y, fut, score, ux, uy, LOG_FLOOR, d)
            basis = float(np.abs(f32.astype(np.float64) - want).max())
            bar = max(4.0 * basis, 1e-5)
            for hz in ([1], default_horizons(T), eight):
                out, fr = _call(torch, h, d, Y_t, fut_t, sc_t, hz, ux, uy)
                err = float(np.abs(fr.astype(np.float64) - want).max())
                worst = max(worst, err)
                print("%s units (%g, %g) horizons %s: max |frame - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g"
                      % ("weighted" if score is not None else "uniform", ux, uy, hz, err, basis, bar))
                assert err <= bar
                np.testing.assert_array_equal(fr[counted & planted], np.float32(LOG_FLOOR))
                np.testing.assert_array_equal(fr[~counted], np.float32(0))
                if d.K < 3:
                    np.testing.assert_array_equal(fr[counted], np.float32(LOG_FLOOR))
                np.testing.assert_allclose(out, kde_outputs(want, fut, hz, d), rtol=0, atol=bar)
                np.testing.assert_allclose(out, kde_outputs(fr, fut, hz, d, dtype=np.float32), rtol=0, atol=1e-6)
                assert not out[~counted.any(1)].any()
    print("worst |frame - f64| of the shape: %.3g" % worst)
    h.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_a_sample_tensor_off_16_byte_alignment(torch_cuda, shape, off):
    """The sample tensor 8 and 4 bytes past an allocation (4: the kernel's scalar loads in place of its 8-byte ones): the reference within the parity
    test's bar, and the aligned call's bits."""
    torch = torch_cuda
    from desire_amd import _lib
    from desire_amd.model import default_horizons
    n, m, K, T = shape
    d = small_dims(T_obs=4, n_grids=1, H=64, n_scenes=n, mno=m, K=K, T_pred=T)
    fut, s, Y, planted, counted = _inputs(d)
    h = _lib.Handle(d)
    Y_t, fut_t, s_t = _t(torch, Y), _t(torch, fut), _t(torch, s)
    Y_off = at_byte_offset(Y_t, off)
    hz = default_horizons(T)
    ux, uy = _units(d)[1]
    for score, sc_t in ((None, None), (s, s_t)):
        want = kde_nll_f64(Y, fut, score, ux, uy, LOG_FLOOR, d)
        basis = float(np.abs(kde_nll_f32(Y, fut, score, ux, uy, LOG_FLOOR, d).astype(np.float64) - want).max())
        bar = max(4.0 * basis, 1e-5)
        out, fr = _call(torch, h, d, Y_off, fut_t, sc_t, hz, ux, uy)
        err = float(np.abs(fr.astype(np.float64) - want).max())
        print("offset %d %s: max |frame - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g" % (off, "weighted" if score is not None else "uniform", err, basis, bar))
        assert err <= bar
        np.testing.assert_allclose(out, kde_outputs(want, fut, hz, d), rtol=0, atol=bar)
        out_a, fr_a = _call(torch, h, d, Y_t, fut_t, sc_t, hz, ux, uy)
        np.testing.assert_array_equal(out.view(np.uint32), out_a.view(np.uint32))
        np.testing.assert_array_equal(fr.view(np.uint32), fr_a.view(np.uint32))
    h.close()


def test_results_are_bitwise_reproducible_and_depend_on_the_agent_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=4, mno=8, K=5, T_obs=4, T_pred=12, n_grids=1, H=64)
    fut, s, Y, _, counted = _inputs(d, seed=11)
    hz, (ux, uy) = [3, 6, 9, 12], _units(d)[1]
    h = _lib.Handle(d)
    Y_t, fut_t, s_t = _t(torch, Y), _t(torch, fut), _t(torch, s)
    bits = lambda x: x.view(np.uint32)
    ref = {}
    for tag, sc in (("uniform", None), ("weighted", s_t)):
        out, fr = _call(torch, h, d, Y_t, fut_t, sc, hz, ux, uy)
        out2, fr2 = _call(torch, h, d, Y_t, fut_t, sc, hz, ux, uy)
        np.testing.assert_array_equal(bits(out), bits(out2)); np.testing.assert_array_equal(bits(fr), bits(fr2))      # run to run
        out3, none = _call(torch, h, d, Y_t, fut_t, sc, hz, ux, uy, frame=False)                                     # dev_frame = NULL
        assert none is None
        np.testing.assert_array_equal(bits(out), bits(out3))
        ref[tag] = (out, fr)
    assert (ref["uniform"][1] != ref["weighted"][1]).any()
    # equal scores are equal weights
    flat = torch.full((d.R,), 0.375, device="cuda")
    out, fr = _call(torch, h, d, Y_t, fut_t, flat, hz, ux, uy)
    np.testing.assert_array_equal(bits(out), bits(ref["uniform"][0])); np.testing.assert_array_equal(bits(fr), bits(ref["uniform"][1]))
    # four windows in one call = two calls of two
    d2 = d.replace(n_scenes=2)
    h2 = _lib.Handle(d2)
    Yw = Y.reshape(4, d.K * d.mno, d.T_pred, 2); sw = s.reshape(4, d.K, d.mno)
    for half in (0, 1):
        sl = slice(2 * half, 2 * half + 2)
        for tag, sc in (("uniform", None), ("weighted", _t(torch, sw[sl]))):
            out, fr = _call(torch, h2, d2, _t(torch, Yw[sl]), _t(torch, fut[sl]), sc, hz, ux, uy)
            rows = slice(2 * half * d.mno, (2 * half + 2) * d.mno)
            np.testing.assert_array_equal(bits(out), bits(ref[tag][0][rows])); np.testing.assert_array_equal(bits(fr), bits(ref[tag][1][rows]))
    # the padding-skipping flags are not the call's business
    hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
    for tag, sc in (("uniform", None), ("weighted", s_t)):
        out, fr = _call(torch, hc, d, Y_t, fut_t, sc, hz, ux, uy)
        np.testing.assert_array_equal(bits(out), bits(ref[tag][0])); np.testing.assert_array_equal(bits(fr), bits(ref[tag][1]))
    # an absent slot's zero rows report the floor without a validity input
    Yz = Y.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).copy()
    slot = int(np.nonzero(counted.reshape(d.n_scenes, d.mno, -1)[0].any(1))[0][0])
    Yz[0, :, slot] = 0
    _, fr = _call(torch, h, d, _t(torch, Yz), fut_t, s_t, hz, ux, uy)
    c = counted[slot]
    assert c.any()
    np.testing.assert_array_equal(fr[slot][c], np.float32(LOG_FLOOR))
    for x in (h, h2, hc):
        x.close()


def test_forward_rank_and_nll_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=4, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    a, b = _leaving(d, 21), _leaving(d, 22)
    p, f, e, g = (_t(torch, x) for x in a[:4])
    h = _lib.Handle(d); h.set_weights(w); h.set_scene_grids(g.data_ptr(), a[4])
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    order = torch.zeros((d.A, d.K), device="cuda", dtype=torch.int32)
    out_u = torch.zeros((d.A, 4, 2), device="cuda"); out_w = torch.zeros((d.A, 4, 2), device="cuda"); fr_w = torch.zeros((d.A, d.T_pred), device="cuda")
    hz = [3, 6, 9, 12]
    floor = -1e30                                                     # an untrained model's samples lie far from the targets: keep their densities apart
    side = torch.cuda.Stream(); sp = side.cuda_stream                 # explicit and non-default

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.rank_samples(sc.data_ptr(), Y.data_ptr(), 1, order.data_ptr(), 0, 0, sp)
        h.kde_nll(Y.data_ptr(), f.data_ptr(), 0, hz, 1.0 / d.sx, 1.0 / d.sy, floor, out_u.data_ptr(), 0, sp)
        h.kde_nll(Y.data_ptr(), f.data_ptr(), sc.data_ptr(), hz, 1.0 / d.sx, 1.0 / d.sy, floor, out_w.data_ptr(), fr_w.data_ptr(), sp)

    bufs = (Y, sc, order, out_u, out_w, fr_w)
    torch.cuda.synchronize()
    ref = {}
    for tag, case in (("b", b), ("a", a)):                        # eager calls
        p.copy_(_t(torch, case[0])); f.copy_(_t(torch, case[1])); e.copy_(_t(torch, case[2]))
        torch.cuda.synchronize()
        calls()
        side.synchronize()
        ref[tag] = [x.clone() for x in bufs]
    h.graph_begin(sp)
    calls()
    gid = h.graph_end(sp)
    for rep in range(4):
        tag, case = ("b", b) if rep % 2 == 0 else ("a", a)
        p.copy_(_t(torch, case[0])); f.copy_(_t(torch, case[1])); e.copy_(_t(torch, case[2]))      # in place: the graph keeps its pointers
        for x in bufs:
            x.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        for x, r in zip(bufs, ref[tag]):
            assert torch.equal(x, r), (rep, tag)
    assert not torch.equal(ref["a"][3], ref["b"][3]) and float(ref["a"][3].abs().max()) > 0
    assert not torch.equal(ref["a"][3], ref["a"][4])              # the score weights change the density
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=1, mno=4, K=3, T_obs=4, T_pred=6, n_grids=1, H=64)
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") + 0.5
    out = torch.full((d.A, 8, 2), FILL, device="cuda"); fr = torch.full((d.A, d.T_pred), FILL, device="cuda")
    p = z.data_ptr()
    nan, inf = float("nan"), float("inf")
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(fut_ptr=0), "dev_fut"), (dict(out_ptr=0), "dev_out"),
             (dict(horizons=[0]), "host_horizons"), (dict(horizons=[7]), "host_horizons"), (dict(horizons=[2, 2]), "increasing"),
             (dict(horizons=[3, 2]), "increasing"), (dict(horizons=[]), "n_h"),
             (dict(log_floor=nan), "log_floor"), (dict(log_floor=-inf), "log_floor"), (dict(log_floor=inf), "log_floor"),
             (dict(unit_x=0.0), "unit_x"), (dict(unit_x=-1.0), "unit_x"), (dict(unit_x=nan), "unit_x"), (dict(unit_x=inf), "unit_x"),
             (dict(unit_y=0.0), "unit_y"), (dict(unit_y=-2.0), "unit_y"), (dict(unit_y=nan), "unit_y"), (dict(unit_y=inf), "unit_y")]
    for kw, word in cases:
        args = dict(yhat_ptr=p, fut_ptr=p, score_ptr=p, horizons=[6], unit_x=1.0, unit_y=1.0, log_floor=LOG_FLOOR, out_ptr=out.data_ptr(),
                    frame_ptr=fr.data_ptr())
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.kde_nll(**args)
    d9 = d.replace(T_pred=9)
    h9 = _lib.Handle(d9)
    with pytest.raises(_lib.DesireError, match="error -1.*n_h"):
        h9.kde_nll(p, p, p, list(range(1, 10)), 1.0, 1.0, LOG_FLOOR, out.data_ptr(), 0)
    lib = _lib.load()
    one = C.c_float(1)
    assert lib.desire_kde_nll(h._h, p, p, p, None, 1, one, one, C.c_float(LOG_FLOOR), out.data_ptr(), fr.data_ptr(), None) == -1
    assert b"host_horizons" in lib.desire_last_error()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.kde_nll(p, p, p, [8], 1.0, 1.0, LOG_FLOOR, out.data_ptr(), 0)
    torch.cuda.synchronize()
    assert (out == FILL).all() and (fr == FILL).all()
    ok = torch.full((d.A, 1, 2), FILL, device="cuda")
    h.kde_nll(p, p, 0, [6], 1.0, 1.0, LOG_FLOOR, ok.data_ptr(), fr.data_ptr())       # ... and the handle still works (NULL scores are legal)
    torch.cuda.synchronize()
    assert (ok != FILL).all() and (fr != FILL).all() and (out == FILL).all()
    for x in (h, h9, rc):
        x.close()


def test_the_model_and_the_evaluation_walk_report_the_nll(torch_cuda):
    torch = torch_cuda
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    flags = ["--batch_size", "2", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--d_dim", "64", "--latent_size", "64",
             "--num_samples", "5", "--neighborhood_size", "256", "--max_windows", "4", "--device_rng", "--seed", "3", "--checkpoint", "none.npz", "--units", "norm"]
    t = np.arange(60, dtype=np.float32)
    video = np.zeros((60, 8, 3), np.float32)                          # five objects walking straight lines, the last one leaves half way
    for i in range(5):
        video[:, i, 0] = i + 1
        video[:, i, 1] = 200 + 150 * i + 3 * t
        video[:, i, 2] = 150 + 100 * i + 2 * t
    video[30:, 4] = 0
    res = {}
    for tag, extra in (("plain", []), ("nll", ["--nll"])):
        a = E.build_parser().parse_args(flags + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=DESIREModel(a, seed=4))
    assert "kde_nll" not in res["plain"]
    blk = res["nll"].pop("kde_nll")
    assert res["nll"] == res["plain"]                                 # the rest of the result is what it is without the flag
    hz = res["plain"]["horizons"]
    assert blk["log_floor"] == LOG_FLOOR and set(blk) == {"log_floor", "uniform", "score_weighted", "floored_frames", "frames"}
    for k in ("uniform", "score_weighted"):
        assert len(blk[k]["mean"]) == len(blk[k]["final"]) == len(hz) and np.isfinite(blk[k]["mean"] + blk[k]["final"]).all()
        assert max(blk[k]["mean"] + blk[k]["final"]) <= -LOG_FLOOR
    assert 0 <= blk["floored_frames"] <= blk["frames"] and blk["frames"] > 0
    # the same walk through the handle: evaluate_nll is the handle's call, and the block is the float64 host mean of its per-agent output
    a = E.build_parser().parse_args(flags + ["--nll"])
    dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
    m = DESIREModel(a, seed=4)
    tot, cnt, nw, frames, floored = np.zeros(len(hz)), np.zeros(len(hz), np.int64), 0, 0, 0
    for xs, _ in E.iter_batches(dl, a.batch_size, a.max_windows):
        past, fut = split_windows(xs, a.seq_length)
        m.predict(past, top=res["plain"]["top"], seed=a.seed, device_rng=True, window_base=nw)
        Y, score = m.final_output, m.final_states
        n = len(xs)
        h = m._handles.get((n, 0, 0)) or m._handle(n, True)
        d = h.dims
        fut_t = m._pad_windows(fut, d.mno)
        for weighted in (False, True):
            out, fr = _call(torch, h, d, Y, fut_t, score if weighted else None, hz, 1.0, 1.0)
            ev, evf = m.evaluate_nll(Y, score, fut, horizons=hz, units="norm", weighted=weighted, return_frames=True)
            np.testing.assert_array_equal(ev.view(np.uint32), out.view(np.uint32)); np.testing.assert_array_equal(evf.view(np.uint32), fr.view(np.uint32))
            if weighted:
                continue
            np.testing.assert_array_equal(m.evaluate_nll(Y, None, fut_t, horizons=hz, units="norm").view(np.uint32), out.view(np.uint32))      # a device tensor, the defaults
            pw, fw = np.stack(past), np.stack(fut)
            valid = np.zeros((n, d.mno), bool); valid[:, :pw.shape[2]] = pw[:, -1, :, 0] != 0
            seen = np.zeros((n, d.T_pred, d.mno), bool); seen[:, :, :pw.shape[2]] = fw[:, :, :, 0] != 0
            for i, hh in enumerate(hz):
                c = (valid & seen[:, :hh].any(1)).reshape(-1)
                tot[i] += out[c, i, 0].astype(np.float64).sum(); cnt[i] += int(c.sum())
            cf = (valid[:, None, :] & seen).transpose(0, 2, 1).reshape(fr.shape)
            frames += int(cf.sum()); floored += int((cf & (fr <= np.float32(LOG_FLOOR))).sum())
        nw += n
    assert nw == res["plain"]["windows"] and list(cnt) == res["plain"]["agents"]
    print("uniform mean NLL per horizon: evaluate %s, handle %s" % (blk["uniform"]["mean"], list(tot / cnt)))
    np.testing.assert_allclose(blk["uniform"]["mean"], tot / cnt, rtol=0, atol=1e-5)
    assert (blk["frames"], blk["floored_frames"]) == (frames, floored)


def test_the_training_report_prints_both_means(torch_cuda):
    import re
    from desire_amd import train as T
    from desire_amd.model import DESIREModel
    a = T.build_parser().parse_args(["--batch_size", "2", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--d_dim", "64",
                                     "--latent_size", "64", "--num_samples", "5", "--neighborhood_size", "256", "--report_nll"])
    t = np.arange(10, dtype=np.float32)
    win = np.zeros((2, 10, 8, 3), np.float32)                         # two windows of four objects walking straight lines
    for n in range(2):
        for i in range(4):
            win[n, :, i, 0] = i + 1
            win[n, :, i, 1] = 200 + 150 * i + (3 + n) * t
            win[n, :, i, 2] = 150 + 100 * i + 2 * t
    past, fut = T.split_windows(list(win), a.seq_length)
    m = DESIREModel(a, seed=4)
    lines = []
    T._report(a, m, past, fut, 7, 0, lines.append)
    assert len(lines) == 1, lines
    mt = re.fullmatch(r"epoch 7 rank 0: KDE NLL px @h=6: uniform = (-?[0-9.]+), score-weighted = (-?[0-9.]+) \(8 agents\)", lines[0])
    assert mt, lines[0]
    assert all(np.isfinite(float(v)) and float(v) <= -LOG_FLOOR for v in mt.groups())
    lines.clear()
    T._report(T.build_parser().parse_args([]), m, past, fut, 7, 0, lines.append)      # off by default
    assert lines == []
