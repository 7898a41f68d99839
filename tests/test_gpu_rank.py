"""Ranking by IOC score on the device (desire_rank_samples / desire_ranked_errors, csrc/kernels_rank.hip) against the numpy statement of
the contract in tests/rank_reference.py: the order bit for bit, the gather bit for bit, the errors within the ADE / FDE harness's own
tolerance (tests/test_gpu_loss_masking.py: atol 1e-5 in normalised units, scaled by the unit because the error is linear in it), through
DESIREModel.predict, from a captured graph, and through the training loop and the evaluation command line."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from desire_amd.spec import init_weights
from tests.helpers import MISALIGNED_LONG, MISALIGNED_SHAPES, at_byte_offset, make_case, small_dims
from tests.rank_reference import planted_scores, rank_order, ranked_errors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _t(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _order(torch, h, d, score_t, n_top=1, Y_t=None, gather=False):
    order = torch.full((d.A, d.K), -1, device="cuda", dtype=torch.int32)
    top_Y = torch.full((d.A, n_top, d.T_pred, 2), -7.0, device="cuda") if gather else None
    top_s = torch.full((d.A, n_top), -7.0, device="cuda") if gather else None
    h.rank_samples(score_t.data_ptr(), Y_t.data_ptr() if Y_t is not None else 0, n_top, order.data_ptr(),
                   top_Y.data_ptr() if gather else 0, top_s.data_ptr() if gather else 0)
    torch.cuda.synchronize()
    return order.cpu().numpy(), (top_Y.cpu().numpy() if gather else None), (top_s.cpu().numpy() if gather else None)


def _errors(torch, h, d, Y_t, fut_t, order_t, n_top, hz, ux, uy):
    out = torch.full((d.A, len(hz), 4), -7.0, device="cuda")
    h.ranked_errors(Y_t.data_ptr(), fut_t.data_ptr(), order_t.data_ptr(), n_top, hz, ux, uy, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _leaving(d, seed):
    """tests/test_gpu_loss_masking.py's kind of case: objects leaving, a track gap, a slot never in the target (where the shape has them)."""
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


@pytest.mark.parametrize("K,mno", [(1, 1), (3, 8), (20, 4), (7, 32), (20, 32), (50, 96), (130, 160)])
def test_order_and_gather_are_bit_exact(torch_cuda, K, mno):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=2, mno=mno, K=K, T_obs=4, T_pred=5, n_grids=1, H=64)
    h = _lib.Handle(d)
    s = planted_scores(d, 100 + K)
    rng = np.random.default_rng(K)
    Y = rng.standard_normal((d.R, d.T_pred, 2)).astype(np.float32)
    want = rank_order(s, d)
    s_t, Y_t = _t(torch, s), _t(torch, Y)
    got, _, _ = _order(torch, h, d, s_t)                          # NULL dev_Yhat / dev_top_Y / dev_top_score accepted
    np.testing.assert_array_equal(got, want)
    rows = lambda o: (np.arange(d.A)[:, None] // mno * K + o) * mno + np.arange(d.A)[:, None] % mno      # [A, n] rows of samples o
    for n_top in sorted({1, min(2, K), K}):
        got, top_Y, top_s = _order(torch, h, d, s_t, n_top, Y_t, gather=True)
        np.testing.assert_array_equal(got, want)
        r = rows(want[:, :n_top])
        np.testing.assert_array_equal(top_Y, Y[r])
        np.testing.assert_array_equal(top_s.view(np.uint32), s.reshape(-1)[r].view(np.uint32))      # (bit patterns: NaN scores included)
    # only one of the two outputs
    order = torch.empty((d.A, d.K), device="cuda", dtype=torch.int32); top_s = torch.empty((d.A, 1), device="cuda")
    h.rank_samples(s_t.data_ptr(), 0, 1, order.data_ptr(), 0, top_s.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(top_s.cpu().numpy().view(np.uint32), s.reshape(-1)[rows(want[:, :1])].view(np.uint32))
    h.close()


ERR_SHAPES = [dict(n_scenes=2, mno=8, K=5, T_pred=12),           # the loss-masking case
              dict(n_scenes=2, mno=8, K=3, T_pred=7),            # odd T_pred
              dict(n_scenes=3, mno=1, K=3, T_pred=7),            # odd row length in floats / 2: rows that do not start on 16 bytes
              dict(n_scenes=3, mno=32, K=20, T_pred=40),         # the headline's chunking: every slot, three sample chunks per window
              dict(n_scenes=2, mno=160, K=3, T_pred=9),          # one sample per chunk
              dict(n_scenes=2, mno=32, K=2, T_pred=200)]         # slot chunks: segments per sample


@pytest.mark.parametrize("shape", ERR_SHAPES, ids=lambda s: "m%d_K%d_T%d" % (s["mno"], s["K"], s["T_pred"]))
def test_errors_match_the_reference_in_every_unit(torch_cuda, shape):
    torch = torch_cuda
    from desire_amd import _lib
    from desire_amd.model import default_horizons, default_top
    d = small_dims(T_obs=4, n_grids=1, H=64, **shape)
    h = _lib.Handle(d)
    _, fut, _, _, _ = _leaving(d, 7)
    rng = np.random.default_rng(8)
    Y = rng.uniform(0.05, 0.95, (d.R, d.T_pred, 2)).astype(np.float32)
    s = planted_scores(d, 9)
    order = rank_order(s, d)
    Y_t, fut_t, s_t = _t(torch, Y), _t(torch, fut), _t(torch, s)
    got_order, _, _ = _order(torch, h, d, s_t)
    np.testing.assert_array_equal(got_order, order)
    order_t = _t(torch, got_order)
    T = d.T_pred
    eight = [1, 2, 3, 5, 7, 9, 11, 12] if T >= 12 else list(range(1, min(T, 8) + 1))
    if T > 12:
        eight[-1] = T
    units = [(1.0, 1.0), (1.0 / d.sx, 1.0 / d.sy), (0.2 / d.sx, 0.2 / d.sy)]
    worst = 0.0
    for ux, uy in units:
        for hz in ([1], default_horizons(T), eight):
            for n_top in sorted({1, default_top(d.K), d.K}):
                got = _errors(torch, h, d, Y_t, fut_t, order_t, n_top, hz, ux, uy)
                want = ranked_errors(Y, fut, order, n_top, hz, ux, uy, d)
                err = float(np.abs(got - want).max()) / max(ux, uy)
                worst = max(worst, err)
                print("units (%g, %g) horizons %s n_top %d: max |diff| / unit = %.3g" % (ux, uy, hz, n_top, err))
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * max(ux, uy))
    # consistency with the existing harness: n_top = K, h = T_pred, units (1, 1) -> its best-of-K columns
    af = torch.zeros((d.A, 4), device="cuda")
    h.ade_fde(Y_t.data_ptr(), fut_t.data_ptr(), af.data_ptr())
    got = _errors(torch, h, d, Y_t, fut_t, order_t, d.K, [T], 1.0, 1.0)
    np.testing.assert_allclose(got[:, 0, 2:], af.cpu().numpy()[:, 2:], rtol=0, atol=1e-5)
    # exact properties
    hz = default_horizons(T)
    ux, uy = units[1]
    prev = None
    for n_top in range(1, d.K + 1):
        r = _errors(torch, h, d, Y_t, fut_t, order_t, n_top, hz, ux, uy)
        if prev is not None:
            assert (r[..., 2:] <= prev[..., 2:]).all(), n_top      # best-of-top-n never gets worse with n
            np.testing.assert_array_equal(r[..., :2], prev[..., :2])
        else:
            np.testing.assert_array_equal(r[..., :2], r[..., 2:])   # n_top = 1: both pairs of columns are the top-1 sample's
        prev = r
    again = _errors(torch, h, d, Y_t, fut_t, order_t, d.K, hz, ux, uy)
    np.testing.assert_array_equal(again.view(np.uint32), prev.view(np.uint32))      # run to run: bitwise
    one = _errors(torch, h, d, Y_t, fut_t, order_t, d.K, [1], ux, uy)
    np.testing.assert_array_equal(one[..., 0], one[..., 1])          # h = 1: ADE = FDE
    np.testing.assert_array_equal(one[..., 2], one[..., 3])
    counted = (fut[..., 0] != 0).any(1).reshape(-1)
    assert not prev[~counted].any() and (prev[counted][:, -1] > 0).all()
    h.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES + [MISALIGNED_LONG], ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_errors_of_a_sample_tensor_off_16_byte_alignment(torch_cuda, shape, off):
    """The 8-byte path of the streaming loop for a whole buffer: the reference within the parity test's bar, and the aligned call's bits."""
    torch = torch_cuda
    from desire_amd import _lib
    from desire_amd.model import default_horizons, default_top
    n, m, K, T = shape
    d = small_dims(T_obs=4, n_grids=1, H=64, n_scenes=n, mno=m, K=K, T_pred=T)
    h = _lib.Handle(d)
    _, fut, _, _, _ = _leaving(d, 7)
    Y = np.random.default_rng(8).uniform(0.05, 0.95, (d.R, d.T_pred, 2)).astype(np.float32)
    order = rank_order(planted_scores(d, 9), d)
    Y_t, fut_t, order_t = _t(torch, Y), _t(torch, fut), _t(torch, order.astype(np.int32))
    hz, n_top, ux, uy = default_horizons(T), default_top(d.K), 1.0 / d.sx, 1.0 / d.sy
    aligned = _errors(torch, h, d, Y_t, fut_t, order_t, n_top, hz, ux, uy)
    got = _errors(torch, h, d, at_byte_offset(Y_t, off), fut_t, order_t, n_top, hz, ux, uy)
    want = ranked_errors(Y, fut, order, n_top, hz, ux, uy, d)
    print("offset %d: max |diff| / unit = %.3g" % (off, float(np.abs(got - want).max()) / max(ux, uy)))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * max(ux, uy))
    np.testing.assert_array_equal(got.view(np.uint32), aligned.view(np.uint32))
    h.close()


def test_bad_arguments_are_refused_with_a_message(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=1, mno=4, K=3, T_obs=4, T_pred=6, n_grids=1, H=64)
    h = _lib.Handle(d)
    z = torch.zeros(4096, device="cuda")
    zi = torch.zeros(4096, device="cuda", dtype=torch.int32)
    p, pi = z.data_ptr(), zi.data_ptr()
    for kw, word in ((dict(score_ptr=0), "dev_score"), (dict(order_ptr=0), "dev_order"), (dict(n_top=0), "n_top"), (dict(n_top=4), "n_top"),
                     (dict(yhat_ptr=0, top_y_ptr=p), "dev_Yhat")):
        args = dict(score_ptr=p, yhat_ptr=p, n_top=1, order_ptr=pi)
        args.update(kw)
        with pytest.raises(_lib.DesireError, match=word):
            h.rank_samples(**args)
    for kw, word in ((dict(yhat_ptr=0), "dev_Yhat"), (dict(fut_ptr=0), "dev_fut"), (dict(order_ptr=0), "dev_order"), (dict(out_ptr=0), "dev_out"),
                     (dict(n_top=0), "n_top"), (dict(n_top=4), "n_top"), (dict(horizons=[0]), "host_horizons"), (dict(horizons=[7]), "host_horizons"),
                     (dict(horizons=[2, 2]), "increasing"), (dict(horizons=[3, 2]), "increasing"), (dict(horizons=[]), "n_h")):
        args = dict(yhat_ptr=p, fut_ptr=p, order_ptr=pi, n_top=1, horizons=[6], unit_x=1.0, unit_y=1.0, out_ptr=p)
        args.update(kw)
        with pytest.raises(_lib.DesireError, match=word):
            h.ranked_errors(**args)
    d9 = d.replace(T_pred=9)
    h9 = _lib.Handle(d9)
    with pytest.raises(_lib.DesireError, match="n_h"):
        h9.ranked_errors(p, p, pi, 1, list(range(1, 10)), 1.0, 1.0, p)
    import ctypes as C
    lib = _lib.load()
    assert lib.desire_ranked_errors(h._h, p, p, pi, 1, None, 1, C.c_float(1), C.c_float(1), p, None) == -1 and b"host_horizons" in lib.desire_last_error()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="ref_compat"):
        rc.rank_samples(p, p, 1, pi)
    with pytest.raises(_lib.DesireError, match="ref_compat"):
        rc.ranked_errors(p, p, pi, 1, [8], 1.0, 1.0, p)
    torch.cuda.synchronize()
    for x in (h, h9, rc):
        x.close()


@pytest.mark.parametrize("bf16", [0, 2])
@pytest.mark.parametrize("keep_padding", [False, True])
def test_predict_ranks_a_real_window(torch_cuda, golden_dir, bf16, keep_padding):
    """DESIREModel.predict on the bookstore window of tests/golden/e2e_cfg1.npz (9 of 32 slots present), the model's own initial weights."""
    torch = torch_cuda
    import argparse
    from desire_amd.model import DESIREModel, default_top
    g = np.load(os.path.join(golden_dir, "e2e_cfg1.npz"))
    past = g["past"]
    assert past.shape == (1, 8, 32, 3) and int((past[0, -1, :, 0] != 0).sum()) == 9
    args = argparse.Namespace(rnn_size=512, seq_length=8, pred_length=12, d_dim=64, latent_size=64, max_num_obj=32, num_samples=20,
                              learning_rate=0.005, grad_clip=10.0, neighborhood_size=200, img_width=1424.0, img_height=1088.0,
                              bf16=bf16, keep_padding=keep_padding)
    m = DESIREModel(args, seed=3)
    out = m.predict([past[0]], seed=5)
    torch.cuda.synchronize()
    d = m._handle(1, False).dims
    top = default_top(d.K)
    assert top == 2 and (d.flags == 0) == keep_padding
    Y, score = m.final_output, m.final_states                     # [1, K, mno, T, 2], [1, K, mno]: the model's own samples and scores
    assert tuple(out["traj"].shape) == (1, 32, top, 12, 2) and tuple(out["score"].shape) == (1, 32, top)
    assert tuple(out["order"].shape) == (1, 32, 20) and out["order"].dtype == torch.int32
    present = past[0, -1, :, 0] != 0
    np.testing.assert_array_equal(out["present"].cpu().numpy()[0], present)
    sc = score.cpu().numpy()
    want = rank_order(sc, d)
    order = out["order"].cpu().numpy().reshape(d.A, d.K)
    np.testing.assert_array_equal(order, want)
    assert len({tuple(o) for o in order[present]}) > 1            # the present agents are really ranked
    if not keep_padding:                                          # absent slots: scores all zero -> identity
        np.testing.assert_array_equal(order[~present], np.broadcast_to(np.arange(d.K), (int((~present).sum()), d.K)))
    Yn = Y.cpu().numpy()[0]                                       # [K, mno, T, 2]
    slots = np.arange(d.mno)[:, None]
    gathered = Yn[want[:, :top], slots]                           # [mno, top, T, 2]
    scale = torch.tensor([d.sx, d.sy], device="cuda", dtype=torch.float32)
    np.testing.assert_array_equal(out["traj"].cpu().numpy()[0], (_t(torch, gathered) / scale).cpu().numpy())
    np.testing.assert_array_equal(out["score"].cpu().numpy()[0], sc[0][want[:, :top], slots])
    px = out["traj"].cpu().numpy()[0][present]
    assert np.isfinite(px).all() and np.abs(px).max() > 1.0       # pixels, not normalised units
    # evaluate_ranked on the same samples agrees with the stand-alone reference
    fut = g["fut"][:, :12]
    ev = m.evaluate_ranked(Y, score, _t(torch, fut), units="px")
    ref = ranked_errors(Y.cpu().numpy().reshape(d.R, d.T_pred, 2), fut, want, top, [3, 6, 9, 12], 1.0 / d.sx, 1.0 / d.sy, d)
    np.testing.assert_allclose(ev, ref, rtol=0, atol=1e-5 / min(d.sx, d.sy))


def test_forward_rank_and_errors_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=4, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    a, b = _leaving(d, 21), _leaving(d, 22)
    p, f, e, g = (_t(torch, x) for x in a[:4])
    h = _lib.Handle(d); h.set_weights(w); h.set_scene_grids(g.data_ptr(), a[4])
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    order = torch.zeros((d.A, d.K), device="cuda", dtype=torch.int32)
    top_Y = torch.zeros((d.A, 2, d.T_pred, 2), device="cuda"); top_s = torch.zeros((d.A, 2), device="cuda")
    out = torch.zeros((d.A, 4, 4), device="cuda")
    hz = [3, 6, 9, 12]
    side = torch.cuda.Stream(); sp = side.cuda_stream

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.rank_samples(sc.data_ptr(), Y.data_ptr(), 2, order.data_ptr(), top_Y.data_ptr(), top_s.data_ptr(), sp)
        h.ranked_errors(Y.data_ptr(), f.data_ptr(), order.data_ptr(), 2, hz, 1.0 / d.sx, 1.0 / d.sy, out.data_ptr(), sp)

    torch.cuda.synchronize()
    ref = {}
    for tag, case in (("b", b), ("a", a)):                        # eager calls (the first also warms lazy allocations up outside capture)
        p.copy_(_t(torch, case[0])); f.copy_(_t(torch, case[1])); e.copy_(_t(torch, case[2]))
        torch.cuda.synchronize()
        calls()
        side.synchronize()
        ref[tag] = [x.clone() for x in (Y, sc, order, top_Y, top_s, out)]
    h.graph_begin(sp)
    calls()
    gid = h.graph_end(sp)
    for rep in range(4):
        tag, case = ("b", b) if rep % 2 == 0 else ("a", a)
        p.copy_(_t(torch, case[0])); f.copy_(_t(torch, case[1])); e.copy_(_t(torch, case[2]))      # in place: the graph keeps its pointers
        for x in (Y, sc, order, top_Y, top_s, out):
            x.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        for x, r in zip((Y, sc, order, top_Y, top_s, out), ref[tag]):
            assert torch.equal(x, r), (rep, tag)
    assert not torch.equal(ref["a"][5], ref["b"][5]) and float(ref["a"][5].abs().max()) > 0
    np.testing.assert_array_equal(ref["a"][2].cpu().numpy(), rank_order(ref["a"][1].cpu().numpy(), d))
    h.close()


def _synthetic_csv(path, n_frames, n_ids, rng):
    """One video in the loader's CSV layout (4 rows: frame, track id, x, y): smooth tracks, some of which leave early."""
    t = np.arange(n_frames)
    cols = []
    for i in range(n_ids):
        x0, y0, vx, vy = rng.uniform(300, 1100), rng.uniform(300, 900), rng.normal(0, 3), rng.normal(0, 3)
        last = n_frames if i % 3 else int(n_frames * 0.7)
        for fr in t[:last]:
            cols.append((fr, i + 1, x0 + vx * fr, y0 + vy * fr))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savetxt(path, np.asarray(cols, np.float64).T, delimiter=",", fmt="%.1f")


def test_training_loop_reports_ranked_errors_and_the_command_line_evaluates(tmp_path):
    from desire_amd import evaluate as E
    from desire_amd import train as T
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    rng = np.random.default_rng(0)
    data = str(tmp_path / "data") + "/"
    _synthetic_csv(os.path.join(data, "synth", "video0", "annotations_processed.csv"), 120, 6, rng)
    _synthetic_csv(os.path.join(data, "synth", "video1", "annotations_processed.csv"), 90, 5, rng)
    flags = ["--batch_size", "4", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--d_dim", "64", "--latent_size", "64",
             "--num_samples", "5", "--neighborhood_size", "256", "--leave_dataset", "9", "--data_dir", data]
    a = T.build_parser().parse_args(flags + ["--num_epochs", "3", "--save_every", "5", "--learning_rate", "0.0005", "--save_dir", str(tmp_path / "save"),
                                             "--report_ranked", "--report_ade", "--eval_top", "2", "--eval_horizons", "2,4,6"])
    import random
    random.seed(0)
    lines = []
    losses = T.train(a, log=lines.append)
    assert len(losses) > 0 and np.isfinite(losses).all()
    ranked = [l for l in lines if "ranked px" in l]
    ade = [l for l in lines if "ADE/FDE mean-of-K" in l]
    assert len(ranked) == a.num_epochs and len(ade) == a.num_epochs, lines
    for l in ade:                                                 # --report_ade's line: unchanged in format
        assert re.fullmatch(r"epoch \d+ rank 0: ADE/FDE mean-of-K = [0-9.]+ / [0-9.]+, best-of-K = [0-9.]+ / [0-9.]+ \(\d+ agents\)", l), l
    lst = r"\[([-0-9., naife+]*)\]"
    for l in ranked:
        mt = re.fullmatch(r"epoch \d+ rank 0: ranked px @h=\[2, 4, 6\]: top-1 ADE/FDE = %s / %s, best-of-top-2 = %s / %s \((\d+) agents\)"
                          % (lst, lst, lst, lst), l)
        assert mt, l
        t1a, t1f, bna, bnf = ([float(v) for v in mt.group(i).split(",")] for i in (1, 2, 3, 4))
        assert len(t1a) == len(t1f) == len(bna) == len(bnf) == 3 and int(mt.group(5)) > 0
        assert all(b <= t + 1e-9 for b, t in zip(bna + bnf, t1a + t1f)), l
        assert np.isfinite(t1a + t1f).all() and min(t1a) > 0
    saved = sorted((f for f in os.listdir(tmp_path / "save") if f.endswith(".npz")), key=lambda f: int(f.split("-")[1][:-4]))
    assert saved
    ckpt = str(tmp_path / "save" / saved[-1])
    out = str(tmp_path / "result.json")
    cmd = [sys.executable, "-m", "desire_amd.evaluate", "--checkpoint", ckpt, "--units", "norm", "--out", out, "--seed", "3"] + flags
    pr = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, (pr.stdout + pr.stderr)[-3000:]
    res = json.load(open(out))
    assert res["K"] == 5 and res["top"] == 1 and res["horizons"] == [2, 3, 5, 6] and res["units"] == "norm" and res["seed"] == 3
    assert len(res["agents"]) == 4 and res["agents"][0] > 0 and all(x <= y for x, y in zip(res["agents"], res["agents"][1:]))
    for i in range(4):
        assert res["best_of_K"]["ade"][i] <= res["best_of_top"]["ade"][i] <= res["top1"]["ade"][i]
        assert res["best_of_K"]["fde"][i] <= res["best_of_top"]["fde"][i] <= res["top1"]["fde"][i]
    # the same walk through the existing harness: float64 mean of evaluate()'s best-of-K ADE over the same agents and batches
    e = E.build_parser().parse_args(["--checkpoint", ckpt, "--seed", "3"] + flags)
    dl = DataLoader(e.batch_size, e.seq_length + e.pred_length, e.max_num_obj, e.leave_dataset, data_dir=data)
    m = DESIREModel.restore(e, ckpt)
    tot, cnt, nw = 0.0, 0, 0
    for xs, _ in E.iter_batches(dl, e.batch_size):
        past, fut = T.split_windows(xs, e.seq_length)
        Y, _ = m.forward(past, None, seed=3)
        ev = m.evaluate(Y, fut).astype(np.float64)
        c = np.zeros((len(xs), ev.shape[0] // len(xs)), bool)
        c[:, :8] = (np.stack(past)[:, -1, :, 0] != 0) & (np.stack(fut)[:, :, :, 0] != 0).any(1)
        tot += ev[c.reshape(-1), 2].sum(); cnt += int(c.sum()); nw += len(xs)
    assert nw == res["windows"] and cnt == res["agents"][-1] == res["mean_of_K"]["agents"]
    print("best-of-K ADE (norm): evaluate.py %.9g, harness %.9g over %d agents" % (res["best_of_K"]["ade"][-1], tot / cnt, cnt))
    assert abs(res["best_of_K"]["ade"][-1] - tot / cnt) <= 1e-5
