"""desire_rollout_samples: K Gaussian-head rollouts per agent in one launch, in the sample layout (include/desire_hip.h; csrc/kernels_rollout.hip).

  1. oracle parity: every sample k against oracle.rollout in float64 on the normals of row k, the clip hit and missed; the bar is four times the
     error the existing desire_rollout makes against the same oracle on the same inputs (room for the head's regrouped sum), and never the
     project's 1e-3 trajectory gate.  Shapes: 3 windows x 3 samples x 9 steps, H in {16 (zero-padded to the 64-wide tile), 64, 128}, 16 and 8 slots.
     R = 144 / 72 rows are 4.5 / 2.25 tiles of 32: the last tile is partial, and with K odd the (scene, k) groups of a tile belong to two windows.
     (A handle takes slot counts that divide 32 or are multiples of 32 -- desire_create refuses 12 or 24 -- so a group never straddles two tiles at an
     odd offset through the ABI; the 64-slot case puts every group on two tiles.)
  2. a row does not depend on the batch: four windows in one call == two calls of two windows at scene_base 0 and 2; an 8-slot handle at slot_base 8
     == slots 8..15 of a 16-slot handle, both drawing on the device.  Bit for bit.
  3. the noise twin: a NULL-normals call in draw d == the explicit call on desire_rng_fill(kind ROLLOUT, stream_id d), bit for bit; the fill equals
     the numpy restatement (tests/rollout_reference.py) to 1e-5; one draw per call; re-seeding reproduces the call.
  4. downstream: encode -> rollout_samples -> ioc_refine -> rank_samples -> ranked_errors runs on the new layout; predict(generator="rollout")
     returns those rows in pixels; "Hx" is untouched by the rollout.
  5. that sequence captured in a graph draws fresh noise per replay, equal to the uncaptured calls of the same draws.
  6. refusals: DESIRE_ERR_ARG, and nothing is launched.
  7. desire_amd.evaluate with generator "rollout" walks a video under the ranked protocol and names the generator in its result."""
import argparse

import numpy as np
import pytest

from desire_amd.spec import init_weights
from tests import rollout_reference as RR
from tests.helpers import make_case, small_dims, to_oracle_layout

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD9876F00D
NORMAL_TOL = 1e-5                            # fp32 normals against float64 on the same bits (derivation: tests/test_rng_cpu.py)
HEAD_BIAS = [0.45, 0.5, -3.0, -3.5, 0.3]     # sigma ~ 0.05 / 0.03 of the frame (tests/test_gpu_sample_rollout.py)
TRAJ_GATE = 1e-3                             # the project's trajectory gate
SENTINEL = 7.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def weights(d, seed=71):
    w = init_weights(d, seed)
    w["gauss_head/b"] = np.array(HEAD_BIAS, np.float32)
    return w


def handle(torch, d, w, grids=None, gos=None):
    from desire_amd import _lib
    h = _lib.Handle(d)
    h.set_weights(w)
    if grids is not None:
        h._grids = dev(torch, grids)                                   # rides along so that it outlives the calls
        h.set_scene_grids(h._grids.data_ptr(), gos)
    return h


def roll(torch, h, past_t, normals_t=None, stream=0):
    """desire_rollout_samples into a sentinel-filled Y; normals_t None = NULL normals.  Returns Y [n, K, mno, T_pred, 2] as numpy."""
    d = h.dims
    Y = torch.full((d.R, d.T_pred, 2), SENTINEL, device="cuda")
    h.rollout_samples(past_t.data_ptr(), 0 if normals_t is None else normals_t.data_ptr(), Y.data_ptr(), stream)
    torch.cuda.synchronize()
    return Y.cpu().numpy().reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2)


def filled_normals(torch, h, seed, draw):
    from desire_amd import _lib
    d = h.dims
    n = torch.full((d.R * d.T_pred * 2 + 8,), 9.0, device="cuda")
    h.rng_fill(seed, draw, 0, _lib.RNG_ROLLOUT, n.data_ptr(), d.R * d.T_pred * 2)
    torch.cuda.synchronize()
    assert (n[d.R * d.T_pred * 2:] == 9.0).all(), "the rollout fill wrote past its tensor"
    return n[: d.R * d.T_pred * 2].clone()


# ---- 1. oracle parity ---------------------------------------------------------------------------------------------------------------------------
_PARITY = {}


def parity_case(mno, H):
    """Inputs and the float64 oracle of one shape, computed once."""
    if (mno, H) not in _PARITY:
        from oracle import desire_oracle as O
        d = small_dims(n_scenes=3, mno=mno, K=3, T_pred=9, H=H, posterior=0, n_grids=1)
        w = weights(d)
        past, _, _, _, _ = make_case(d, seed=72, n_absent=2)
        N = np.random.default_rng(73).standard_normal((d.n_scenes, d.K, d.mno, d.T_pred, 2)).astype(np.float32)
        N[:, :, :, 3] += 12.0                                          # forces the clip at 1.0 for a step
        ref = np.empty(N.shape, np.float64)
        for k in range(d.K):
            Nk = np.ascontiguousarray(N[:, k].transpose(2, 0, 1, 3).reshape(d.T_pred, d.A, 2))
            r = O.rollout(to_oracle_layout(past), w, d, Nk, dt=np.float64)                     # [T, A, 2]
            ref[:, k] = r.reshape(d.T_pred, d.n_scenes, d.mno, 2).transpose(1, 2, 0, 3)
        ref.setflags(write=False)
        _PARITY[(mno, H)] = (d, w, past, N, ref)
    return _PARITY[(mno, H)]


@pytest.mark.parametrize("mno,H", [(16, 16), (16, 64), (16, 128), (8, 16), (8, 64), (8, 128), (64, 64)])
def test_every_sample_matches_the_float64_oracle_within_four_times_the_old_kernels_error(torch_cuda, mno, H):
    torch = torch_cuda
    d, w, past, N, ref = parity_case(mno, H)
    assert (ref == 1.0).any() and (ref < 1.0).any()
    if mno < 32:
        assert d.R % 32 != 0 and (d.K * d.mno) % 32 != 0               # a partial last tile; a window's rows end inside a tile
    h = handle(torch, d, w)
    past_t = dev(torch, past)
    # the existing kernel, one call per sample, on the normals of that sample
    old = np.empty(N.shape, np.float32)
    for k in range(d.K):
        Nk = dev(torch, N[:, k].transpose(2, 0, 1, 3).reshape(d.T_pred, d.A, 2))
        out = torch.zeros((d.T_pred, d.A, 2), device="cuda")
        h.rollout(past_t.data_ptr(), Nk.data_ptr(), d.T_pred, out.data_ptr())
        torch.cuda.synchronize()
        old[:, k] = out.cpu().numpy().reshape(d.T_pred, d.n_scenes, d.mno, 2).transpose(1, 2, 0, 3)
    got = roll(torch, h, past_t, dev(torch, N))
    h.close()
    err_old = float(np.abs(old.astype(np.float64) - ref).max())
    err_new = float(np.abs(got.astype(np.float64) - ref).max())
    print("mno %d H %d: max |Y - float64 oracle|: desire_rollout (K calls) %.3e, desire_rollout_samples %.3e" % (mno, H, err_old, err_new))
    assert np.isfinite(got).all() and (got == 1.0).any() and (got < 1.0).any()
    assert err_new <= TRAJ_GATE, err_new
    assert err_new <= 4.0 * err_old, (err_new, err_old)


# ---- 2. a row does not depend on the batch ------------------------------------------------------------------------------------------------------
def test_four_windows_in_one_call_equal_two_calls_of_two_windows(torch_cuda):
    torch = torch_cuda
    d4 = small_dims(n_scenes=4, mno=8, K=3, T_obs=4, T_pred=7, H=64, posterior=0, n_grids=1)          # R = 96: tile 1 holds rows of windows 1 and 2
    d2 = d4.replace(n_scenes=2)
    w = weights(d4)
    past, _, _, _, _ = make_case(d4, seed=7, n_absent=2)
    h4 = handle(torch, d4, w)
    h4.set_rng(SEED, 3)
    whole = roll(torch, h4, dev(torch, past))
    h4.close()
    assert np.abs(whole - SENTINEL).min() > 0
    for base in (0, 2):
        h2 = handle(torch, d2, w)
        h2.set_rng(SEED, 3)
        h2.set_rng_origin(base, 0)
        part = roll(torch, h2, dev(torch, past[base:base + 2]))
        np.testing.assert_array_equal(part, whole[base:base + 2], err_msg="scene_base %d" % base)
        h2.close()
    assert not np.array_equal(whole[0], whole[2])


def test_a_slot_shard_equals_its_slots_of_the_wider_handle(torch_cuda):
    torch = torch_cuda
    d16 = small_dims(n_scenes=2, mno=16, K=3, T_obs=4, T_pred=7, H=64, posterior=0, n_grids=1)
    d8 = d16.replace(mno=8)
    w = weights(d16)
    past, _, _, _, _ = make_case(d16, seed=8, n_absent=0)
    h16 = handle(torch, d16, w)
    h16.set_rng(SEED, 4)
    wide = roll(torch, h16, dev(torch, past))
    h16.close()
    h8 = handle(torch, d8, w)
    h8.set_rng(SEED, 4)
    h8.set_rng_origin(0, 8)
    shard = roll(torch, h8, dev(torch, past[:, :, 8:]))
    h8.close()
    np.testing.assert_array_equal(shard, wide[:, :, 8:])
    assert not np.array_equal(shard, wide[:, :, :8])


# ---- 3. the noise twin ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_pred", [9, 20])                           # odd: a half-used last block; 20: a second refill of the normals' LDS image
def test_a_null_normals_call_equals_the_explicit_call_on_the_filled_normals(torch_cuda, T_pred):
    torch = torch_cuda
    d = small_dims(n_scenes=3, mno=8, K=3, T_obs=4, T_pred=T_pred, H=64, posterior=0, n_grids=1)
    w = weights(d)
    past, _, _, _, _ = make_case(d, seed=5, n_absent=2)
    past_t = dev(torch, past)
    draw, base, slot_base = 5, 0xFFFFFFFE, 100                          # (windows 2^32 - 2, 2^32 - 1, 0: the wrap)
    a, b = handle(torch, d, w), handle(torch, d, w)
    for h in (a, b):
        h.set_rng_origin(base, slot_base)
    a.set_rng(SEED, draw)
    Ya = roll(torch, a, past_t)
    assert a.rng_state() == (draw + 1, draw)
    n_t = filled_normals(torch, b, SEED, draw)
    ref = RR.rollout_normals(SEED, draw, d.n_scenes, d.K, d.mno, d.T_pred, scene_base=base, slot_base=slot_base)
    err = float(np.abs(n_t.cpu().numpy().astype(np.float64).reshape(ref.shape) - ref).max())
    print("rollout fill against the restatement: max |normal - float64| = %.2e" % err)
    assert err <= NORMAL_TOL, err
    Yb = roll(torch, b, past_t, n_t)
    np.testing.assert_array_equal(Ya, Yb)
    assert np.isfinite(Ya).all() and np.abs(Ya - SENTINEL).min() > 0
    # one draw per NULL call, none per explicit call; another draw is other noise; re-seeding reproduces the call
    Y2 = roll(torch, a, past_t)
    assert a.rng_state() == (draw + 2, draw + 1) and not np.array_equal(Y2, Ya)
    np.testing.assert_array_equal(Y2, roll(torch, b, past_t, filled_normals(torch, b, SEED, draw + 1)))
    roll(torch, a, past_t, n_t)
    assert a.rng_state() == (draw + 2, draw + 1)
    a.set_rng(SEED, draw)
    np.testing.assert_array_equal(roll(torch, a, past_t), Ya)
    a.close(); b.close()


# ---- 4. downstream --------------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    a = argparse.Namespace(rnn_size=512, num_layers=1, batch_size=2, seq_length=8, pred_length=12, d_dim=64, e_dim=256,
                           latent_size=64, max_num_obj=16, learning_rate=0.001, grad_clip=10.0, stride=1,
                           neighborhood_size=300, grid_size=4, num_samples=3, img_width=1400.0, img_height=1100.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_ioc_ranking_and_predict_run_on_the_rollouts(torch_cuda):
    torch = torch_cuda
    import warnings
    from desire_amd.model import DESIREModel, default_horizons
    m = DESIREModel(_args(), seed=4)
    n, top, seed = 2, 2, 11
    d = m._handle(n, False).dims                                       # the model's own prior-path dims (mno = 16)
    assert d.mno == 16 and d.K == 3
    w = m._weights
    past, fut, _, grids, gos = make_case(d, seed=74, n_absent=3)
    m.set_scene_grids(grids, gos)
    with pytest.warns(UserWarning, match="gauss_head"):                # the head holds its initial values: sample()'s warning
        out = m.predict(list(past), top=top, seed=seed, device_rng=True, generator="rollout")
    with pytest.raises(ValueError):
        m.predict(list(past), top=top, generator="gan")
    m._head_given = True
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*gauss_head.*")
        again = m.predict(list(past), top=top, seed=seed, device_rng=True, generator="rollout")
    assert torch.equal(out["traj"], again["traj"]) and torch.equal(out["order"], again["order"])
    # the same stages by hand on a handle of the same dims
    h = handle(torch, d, w, grids, gos)
    past_t, fut_t = dev(torch, past), dev(torch, fut)
    h.encode(past_t.data_ptr(), 0)
    hx0 = h.read_buffer("Hx", (d.A, d.H))
    h.set_rng(seed, 0)
    Y = torch.full((d.R, d.T_pred, 2), SENTINEL, device="cuda")
    h.rollout_samples(past_t.data_ptr(), 0, Y.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(h.read_buffer("Hx", (d.A, d.H)), hx0)            # the rollout warms up into its own buffer
    Y_raw = Y.cpu().numpy().copy()
    score = torch.full((d.R,), SENTINEL, device="cuda")
    h.ioc_refine(Y.data_ptr(), score.data_ptr())
    order = torch.full((d.A, d.K), -1, device="cuda", dtype=torch.int32)
    top_Y = torch.zeros((d.A, top, d.T_pred, 2), device="cuda"); top_s = torch.zeros((d.A, top), device="cuda")
    h.rank_samples(score.data_ptr(), Y.data_ptr(), top, order.data_ptr(), top_Y.data_ptr(), top_s.data_ptr())
    hz = default_horizons(d.T_pred)
    errs = torch.full((d.A, len(hz), 4), -1.0, device="cuda")
    h.ranked_errors(Y.data_ptr(), fut_t.data_ptr(), order.data_ptr(), top, hz, 1.0 / d.sx, 1.0 / d.sy, errs.data_ptr())
    torch.cuda.synchronize()
    sc, od, er = score.cpu().numpy(), order.cpu().numpy(), errs.cpu().numpy()
    assert np.isfinite(sc).all() and np.isfinite(Y.cpu().numpy()).all() and np.isfinite(er).all() and (er >= 0).all()
    np.testing.assert_array_equal(np.sort(od, axis=1), np.broadcast_to(np.arange(d.K), od.shape))       # a permutation per agent
    present = past[:, -1, :, 0] != 0
    moved = np.abs(Y.cpu().numpy() - Y_raw).reshape(d.n_scenes, d.K, d.mno, -1).max(-1)
    assert (moved[np.broadcast_to(present[:, None], moved.shape)] > 0).all()                           # the IOC stage refined the present rows
    px = top_Y.cpu().numpy() / np.array([d.sx, d.sy], np.float32)
    np.testing.assert_array_equal(out["order"].cpu().numpy().reshape(d.A, d.K), od)
    np.testing.assert_array_equal(out["traj"].cpu().numpy().reshape(px.shape), px)
    np.testing.assert_array_equal(out["score"].cpu().numpy().reshape(d.A, top), top_s.cpu().numpy())
    np.testing.assert_array_equal(m.final_output.cpu().numpy().reshape(d.R, d.T_pred, 2), Y.cpu().numpy())
    # the default generator is the path it was
    cv = m.predict(list(past), top=top, seed=seed)
    Y_cv = m.final_output.clone()
    Yc, _ = m.forward(list(past), None, seed=seed)
    assert torch.equal(Y_cv, Yc) and cv["traj"].shape == out["traj"].shape and not torch.equal(cv["traj"], out["traj"])
    h.close()


# ---- 5. graph -------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_pipeline_draws_fresh_noise_equal_to_the_uncaptured_draws(torch_cuda):
    torch = torch_cuda
    d = small_dims(n_scenes=2, mno=16, K=3, T_obs=4, T_pred=6, H=64, posterior=0, n_grids=1)
    w = weights(d)
    past, fut, _, grids, gos = make_case(d, seed=5, n_absent=2)
    h = handle(torch, d, w, grids, gos)
    side = torch.cuda.Stream(); sp = side.cuda_stream
    p_t, f_t = dev(torch, past), dev(torch, fut)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    order = torch.zeros((d.A, d.K), device="cuda", dtype=torch.int32); errs = torch.zeros((d.A, 1, 4), device="cuda")

    def run():
        h.encode(p_t.data_ptr(), 0, sp)
        h.rollout_samples(p_t.data_ptr(), 0, Y.data_ptr(), sp)
        h.ioc_refine(Y.data_ptr(), sc.data_ptr(), sp)
        h.rank_samples(sc.data_ptr(), 0, 1, order.data_ptr(), 0, 0, sp)
        h.ranked_errors(Y.data_ptr(), f_t.data_ptr(), order.data_ptr(), 1, [d.T_pred], 1.0, 1.0, errs.data_ptr(), sp)

    def result():
        side.synchronize()
        return tuple(x.cpu().numpy().copy() for x in (Y, sc, order, errs))

    draw0 = 20
    h.set_rng(SEED, 0, sp)                              # (allocates the words: before the capture)
    run(); side.synchronize()                           # the warm-up call: lazy allocations outside capture
    h.graph_begin(sp)
    run()
    g = h.graph_end(sp)
    h.set_rng(SEED, draw0, sp)
    replays = []
    for _ in range(2):
        h.graph_launch(g, sp)
        replays.append(result())
    assert h.rng_state(sp) == (draw0 + 2, draw0 + 1)
    assert not np.array_equal(replays[0][0], replays[1][0])
    h.set_rng(SEED, draw0, sp)
    for i in range(2):
        run()
        for a, b in zip(result(), replays[i]):
            np.testing.assert_array_equal(a, b, err_msg="draw %d" % (draw0 + i))
    h.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_and_launch_nothing(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=1, mno=8, K=2, T_obs=4, T_pred=6, H=64, posterior=0, n_grids=1)
    w = weights(d)
    past, _, _, _, _ = make_case(d, seed=5, n_absent=2)
    h = handle(torch, d, w)
    past_t = dev(torch, past)
    Y = torch.full((d.R, d.T_pred, 2), SENTINEL, device="cuda")
    nrm = torch.zeros((d.R, d.T_pred, 2), device="cuda")
    p, y, nz = past_t.data_ptr(), Y.data_ptr(), nrm.data_ptr()
    with pytest.raises(_lib.DesireError, match="error -1"):
        h.rollout_samples(p, 0, y)                        # NULL normals before desire_set_rng
    h.set_rng(SEED, 9)
    for args in ((0, nz, y), (p, nz, 0), (0, 0, y), (p, 0, 0)):
        with pytest.raises(_lib.DesireError, match="error -1"):
            h.rollout_samples(*args)
    torch.cuda.synchronize()
    assert h.rng_state() == (9, 9) and (Y == SENTINEL).all()       # no draw was taken, nothing was written
    with pytest.raises(_lib.DesireError, match="error -1"):
        h.rng_fill(SEED, 0, 0, _lib.RNG_ROLLOUT, nz, nrm.numel() - 2)      # the fill writes the whole tensor
    with pytest.raises(_lib.DesireError, match="error -1"):
        h.rng_fill(SEED, 0, 2, _lib.RNG_ROLLOUT, nz, nrm.numel())
    h.rollout_samples(p, 0, y)                            # ... and the handle still works
    torch.cuda.synchronize()
    assert h.rng_state() == (10, 9) and (Y != SENTINEL).all()
    h.close()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.rollout_samples(p, nz, y)
    rc.close()
    # T_pred beyond the counter's step field: the generating call and the fill are refused, the explicit call is not the counter's business
    dl = small_dims(n_scenes=1, mno=1, K=1, T_obs=4, T_pred=RR.MAX_T + 2, H=64, posterior=0, n_grids=1)
    hl = handle(torch, dl, weights(dl))
    hl.set_rng(SEED, 0)
    Yl = torch.full((dl.R, dl.T_pred, 2), SENTINEL, device="cuda")
    pl = dev(torch, make_case(dl, seed=5, n_absent=0)[0])
    with pytest.raises(_lib.DesireError, match="error -1.*2048"):
        hl.rollout_samples(pl.data_ptr(), 0, Yl.data_ptr())
    with pytest.raises(_lib.DesireError, match="error -1.*2048"):
        hl.rng_fill(SEED, 0, 0, _lib.RNG_ROLLOUT, Yl.data_ptr(), Yl.numel())
    torch.cuda.synchronize()
    assert hl.rng_state() == (0, 0) and (Yl == SENTINEL).all()
    hl.close()
    ok = small_dims(n_scenes=1, mno=1, K=1, T_obs=4, T_pred=RR.MAX_T, H=64, posterior=0, n_grids=1)      # T_pred = 2048 fits: the last block's counter
    ho = handle(torch, ok, weights(ok))
    ho.set_rng(SEED, 0)
    n_t = filled_normals(torch, ho, SEED, 0)
    ref = RR.rollout_normals(SEED, 0, 1, 1, 1, RR.MAX_T)
    assert np.abs(n_t.cpu().numpy().astype(np.float64).reshape(ref.shape) - ref).max() <= NORMAL_TOL
    ho.close()


# ---- 7. the evaluation walk ------------------------------------------------------------------------------------------------------------------------
def test_the_evaluation_walk_takes_the_rollout_generator(torch_cuda):
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    flags = ["--batch_size", "2", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--d_dim", "64", "--latent_size", "64",
             "--num_samples", "3", "--neighborhood_size", "256", "--max_windows", "4", "--device_rng", "--seed", "3"]
    t = np.arange(60, dtype=np.float32)
    video = np.zeros((60, 8, 3), np.float32)                          # five objects walking straight lines, the last one leaves half way
    for i in range(5):
        video[:, i, 0] = i + 1
        video[:, i, 1] = 200 + 150 * i + 3 * t
        video[:, i, 2] = 150 + 100 * i + 2 * t
    video[30:, 4] = 0
    res = {}
    for gen in ("cvae", "rollout"):
        a = E.build_parser().parse_args(["--checkpoint", "none.npz", "--generator", gen] + flags)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        m = DESIREModel(a, seed=4)
        m._head_given = True                                           # (the warning of an untrained head is held in test 4)
        res[gen] = E.evaluate(a, data_loader=dl, model=m)
    assert E.build_parser().parse_args(["--checkpoint", "none.npz"]).generator == "cvae"
    for gen, r in res.items():
        assert r["generator"] == gen and r["windows"] == 4 and r["K"] == 3 and r["agents"][-1] > 0
        for name in ("top1", "best_of_top", "best_of_K"):
            assert np.isfinite(r[name]["ade"]).all() and np.isfinite(r[name]["fde"]).all() and min(r[name]["ade"]) > 0
        for i in range(len(r["horizons"])):
            assert r["best_of_K"]["ade"][i] <= r["best_of_top"]["ade"][i] <= r["top1"]["ade"][i]
    assert res["rollout"]["agents"] == res["cvae"]["agents"] and res["rollout"]["top1"] != res["cvae"]["top1"]
