"""The collision penalty on the K joint futures on the device (desire_collision_loss, desire_set_collision_loss; csrc/kernels_collision.hip)
against the numpy statements of its contract and float64 autograd of the rebuilt loss (tests/collision_reference.py).  Shapes are (n_scenes, mno,
K, T_pred) on small_dims(T_obs=6, n_grids=1)."""
import functools

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.collision_reference import (AGENT, MEAN, SCENE, SOFTMIN, coll_chunk_frames, collision_f32, collision_f64, collision_loss_and_grads,
                                       make_collision_inputs, past_with_valid)
from tests.helpers import MISALIGNED_SHAPES, at_byte_offset, make_case, small_dims, to_oracle_layout
from tests.joint_reference import MARGIN, RADIUS_PX
from tests.test_gpu_recon_loss import TAU, _check_done_gradients, _dims, _grads, _step, _t, _training_handle, _weights

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 3, 7),                 # the plain case, odd T_pred
          (3, 1, 3, 7),                 # no pairs at all: everything is 0
          (1, 32, 20, 40),              # the headline's per-window shape
          (2, 160, 4, 9),               # more slots than lanes per frame
          (2, 256, 2, 40)]              # the frame-chunked walk (11 + 11 + 11 + 7 frames)


def _units(d):
    return [(1.0, 1.0, float(np.float32(RADIUS_PX * d.sx))), (1.0 / d.sx, 1.0 / d.sy, RADIUS_PX)]      # (unit_x, unit_y, the radius in that unit)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _op_handle(d, valid, fut):
    """A handle whose "valid" is `valid`, the way it gets there in use: desire_encode reads it off the last observed frame."""
    from desire_amd import _lib
    h = _lib.Handle(d)
    h.set_weights(init_weights(d, 41))
    past_t, fut_t = _t(past_with_valid(d, valid)), _t(fut)
    h.encode(past_t.data_ptr(), fut_t.data_ptr())
    np.testing.assert_array_equal(h.device_tensor("valid", "|u1").cpu().numpy()[: valid.size], valid)
    return h, fut_t


def _op(h, d, fut_t, Y_t, radius, ux, uy, want=(True, True, True, True), fill=-7.0):
    import torch
    A = d.n_scenes * d.mno
    out = {"col": torch.full((A, d.K), fill, device="cuda") if want[0] else None,
           "touch": torch.full((d.n_scenes, d.K), -7, device="cuda", dtype=torch.int32) if want[1] else None,
           "dY": torch.full((d.R, d.T_pred, 2), fill, device="cuda") if want[2] else None,
           "term": torch.full((1,), fill, device="cuda") if want[3] else None}
    p = lambda k: out[k].data_ptr() if out[k] is not None else 0
    h.collision_loss(fut_t.data_ptr(), Y_t.data_ptr(), radius, ux, uy, p("col"), p("touch"), p("dY"), p("term"))
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _close(got, f32, f64, unit, what):
    """The float rule of tests/test_gpu_joint.py: within max(4 |f32 - f64|, 1e-5 x unit) of the float64 statement."""
    basis = float(np.abs(f32.astype(np.float64) - f64).max(initial=0.0))
    err = float(np.abs(got.astype(np.float64) - f64).max(initial=0.0))
    bar = max(4.0 * basis, 1e-5 * unit)
    print("%s: |got - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g" % (what, err, basis, bar))
    assert err <= bar, (what, err, bar)


# ---- 1. the op against the statements ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [0, 1], ids=["normalised", "pixels"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_op_matches_the_contract(shape, unit):
    d = _dims(shape)
    ux, uy, radius = _units(d)[unit]
    Y, fut, valid = make_collision_inputs(d, radius, ux, uy, seed=5 + unit)
    f64 = collision_f64(Y, fut, valid, radius, ux, uy, d)
    assert f64["margin"] > MARGIN                                          # the float64 pass alone, before any comparison
    f32 = collision_f32(Y, fut, valid, radius, ux, uy, d)
    if shape[1] > 1:
        assert f64["touch"].sum() > 0 and f64["term"][0] > 0
        if coll_chunk_frames(d.mno, d.T_pred) < d.T_pred:                  # contacts in the first chunk, across the border and in the last chunk
            tc = coll_chunk_frames(d.mno, d.T_pred)
            hot = np.abs(f64["dY"]).reshape(d.R, d.T_pred, 2).max((0, 2)) > 0
            assert hot[:tc].any() and hot[tc - 1] and hot[tc] and hot[(d.T_pred - 1) // tc * tc:].any()
    h, fut_t = _op_handle(d, valid, fut)
    got = _op(h, d, fut_t, _t(Y), radius, ux, uy)
    np.testing.assert_array_equal(got["touch"], f32["touch"])
    np.testing.assert_array_equal(got["touch"], f64["touch"])
    for k in ("col", "dY", "term"):
        np.testing.assert_array_equal(_bits(got[k]), _bits(f32[k]), err_msg=k)
    # the gradient's unit: one over the position's; col and the term are pure numbers
    _close(got["col"], f32["col"], f64["col"], 1.0, "col")
    _close(got["term"], f32["term"], f64["term"], 1.0, "term")
    _close(got["dY"], f32["dY"], f64["dY"], max(ux, uy), "dY")
    if shape[1] == 1:
        assert not got["touch"].any() and not got["col"].any() and not got["dY"].any() and got["term"][0] == 0
    h.close()


# ---- 2. the boundary, coincident points, radius 0 -----------------------------------------------------------------------------------------------
def test_boundary_coincident_points_and_radius_zero():
    d = _dims((1, 8, 2, 3))
    n, m, K, T = 1, 8, 2, 3
    Y = np.zeros((n, K, m, T, 2), np.float32)
    Y[..., 0] = (8.0 * np.arange(m, dtype=np.float32))[None, None, :, None]      # eight slots 8 apart: nobody near anybody
    Y[..., 1] = 3.0
    Y[:, :, 1, 0, 0] = 0.5                                                   # frame 0: slot 1 at the radius exactly (q == r2): no contact
    Y[:, :, 1, 1, 0] = 0.0                                                   # frame 1: on top of slot 0: phi = 1, gradient 0
    Y[:, :, 1, 2, 0] = 0.25                                                  # frame 2: half way in: u = 0.5, phi = 0.25
    fut = np.zeros((n, T, m, 3), np.float32)
    fut[..., 0] = np.arange(1, m + 1)
    valid = np.ones(m, np.uint8)
    Yr = np.ascontiguousarray(Y.reshape(d.R, T, 2))
    h, fut_t = _op_handle(d, valid, fut)
    got = _op(h, d, fut_t, _t(Yr), 0.5, 1.0, 1.0)
    f32 = collision_f32(Yr, fut, valid, 0.5, 1.0, 1.0, d)
    for k in got:
        np.testing.assert_array_equal(_bits(got[k]), _bits(f32[k]), err_msg=k)
    assert (got["touch"] == 2).all()                                         # frames 1 and 2; the pair at the radius does not touch
    want = np.float32(np.float32(1.0 + 0.25) / np.float32(3.0))
    assert (got["col"][:2] == want).all() and not got["col"][2:].any()
    g = got["dY"].reshape(K, m, T, 2)
    assert not g[:, :, :2].any() and not g[:, 2:].any() and not g[..., 1].any()      # nothing at the radius, nothing at dist == 0, nothing in y
    # d phi / d x_1 = -2 u / radius * sign = -2; the coefficient (1/3 + 1/3) / (nvalid K) = (2/3) / 16
    np.testing.assert_allclose(g[:, 1, 2, 0], -2.0 * (2.0 / 3.0) / 16.0, rtol=1e-6)
    np.testing.assert_array_equal(g[:, 0, 2, 0], -g[:, 1, 2, 0])
    zero = _op(h, d, fut_t, _t(Yr), 0.0, 1.0, 1.0)
    assert not zero["touch"].any() and not zero["col"].any() and not zero["dY"].any() and zero["term"][0] == 0
    h.close()


# ---- 3. the gradient is the gradient (the reference alone, on the CPU) ------------------------------------------------------------------------
def test_the_float64_statement_is_checked_by_central_differences():
    from tests.test_collision_cpu import test_the_gradient_is_the_gradient
    test_the_gradient_is_the_gradient()


# ---- 4. independence and reproducibility ----------------------------------------------------------------------------------------------------------
def test_windows_are_independent_and_runs_reproducible():
    d = _dims((2, 8, 3, 7))
    ux, uy, radius = _units(d)[1]
    Y, fut, valid = make_collision_inputs(d, radius, ux, uy, seed=6)
    fut[1] = fut[0]                                                          # both windows populated, the same targets
    valid[d.mno:] = valid[: d.mno]
    h, fut_t = _op_handle(d, valid, fut)
    a = _op(h, d, fut_t, _t(Y), radius, ux, uy)
    b = _op(h, d, fut_t, _t(Y), radius, ux, uy)
    for k in a:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
    Y2 = Y.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).copy()
    Y2[1] = Y2[1][::-1] * np.float32(0.5)                                    # the other window's rows change; nvalid does not
    c = _op(h, d, fut_t, _t(Y2.reshape(Y.shape)), radius, ux, uy)
    rows = d.K * d.mno
    np.testing.assert_array_equal(_bits(a["col"][: d.mno]), _bits(c["col"][: d.mno]))
    np.testing.assert_array_equal(a["touch"][0], c["touch"][0])
    np.testing.assert_array_equal(_bits(a["dY"][:rows]), _bits(c["dY"][:rows]))
    assert not np.array_equal(_bits(a["dY"][rows:]), _bits(c["dY"][rows:]))
    # all sixteen NULL / non-NULL output choices write the same bits into what they do write, and the rest into the workspace
    for mask in range(16):
        want = tuple(bool(mask >> i & 1) for i in range(4))
        part = _op(h, d, fut_t, _t(Y), radius, ux, uy, want)
        for k, on, ws, dt in zip(("col", "touch", "dY", "term"), want, ("col_val", "col_touch", "col_grad", "col_term"), ("<f4", "<i4", "<f4", "<f4")):
            if on:
                np.testing.assert_array_equal(_bits(part[k]), _bits(a[k]), err_msg=k)
            else:
                assert part[k] is None
                kept = h.device_tensor(ws, dt).cpu().numpy()[: a[k].size].reshape(a[k].shape)
                np.testing.assert_array_equal(_bits(kept), _bits(a[k]), err_msg=ws)
    h.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_op_on_tensors_off_16_byte_alignment(shape, off):
    import torch
    d = _dims(shape)
    ux, uy, radius = _units(d)[1]
    Y, fut, valid = make_collision_inputs(d, radius, ux, uy, seed=6)
    h, fut_t = _op_handle(d, valid, fut)
    Y_t = _t(Y)
    aligned = _op(h, d, fut_t, Y_t, radius, ux, uy)
    f32 = collision_f32(Y, fut, valid, radius, ux, uy, d)
    got = _op(h, d, fut_t, at_byte_offset(Y_t, off), radius, ux, uy)
    for k in got:
        np.testing.assert_array_equal(_bits(got[k]), _bits(aligned[k]), err_msg=k)
        np.testing.assert_array_equal(_bits(got[k]), _bits(f32[k]), err_msg=k)
    dY = at_byte_offset(torch.full((d.R, d.T_pred, 2), -7.0, device="cuda"), off)      # the gradient's 16-byte stores fall back too
    h.collision_loss(fut_t.data_ptr(), Y_t.data_ptr(), radius, ux, uy, 0, 0, dY.data_ptr(), 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(dY.cpu().numpy()), _bits(aligned["dY"]))
    h.close()


# ---- 5. weight 0 leaves every bit as it was -------------------------------------------------------------------------------------------------------
def test_weight_zero_leaves_every_bit_as_it_was():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    case = make_case(d, seed=42, n_absent=4)
    res = []
    for touch in (True, False):
        h, ten = _training_handle(d, w, case)
        if touch:
            h.set_collision_loss(0.0, 123.0, 1.0 / d.sx, 1.0 / d.sy)
        _step(h, ten)
        torch.cuda.synchronize()
        res.append((h.grad_tensor().clone(), h.train_loss(ten["fut"].data_ptr()), ten["Y"].clone()))
        with pytest.raises(Exception):
            h.device_tensor("col_term")                                       # the default never allocates or runs the new code
        h.close()
    assert float(res[0][0].abs().max()) > 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])
    assert res[0][1] == res[1][1]


# ---- 6. / 7. training gradients against float64 autograd, and the reported term -----------------------------------------------------------------
CASES = {"mean": ((2, 32, 3, 7), 42, 4, MEAN, 0.0, AGENT),               # tests/test_gpu_train.py's own case
         "scene_softmin": ((2, 8, 3, 7), 84, 2, SOFTMIN, TAU, SCENE)}      # two absent agents


@functools.lru_cache(maxsize=None)
def _reference(tag):
    """Float64 autograd of loss(mode, scope) + weight * L_col on make_case(seed, n_absent), radius and weight chosen from the oracle's Y0:
    computed once per case, shared, never modified."""
    shape, seed, n_absent, mode, tau, scope = CASES[tag]
    d = _dims(shape)
    past, fut, eps, grids, gos = make_case(d, seed=seed, n_absent=n_absent)
    return collision_loss_and_grads(to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos, _weights(d), d, mode, tau, scope,
                                    1.0 / d.sx, 1.0 / d.sy)


def _collision_step(tag, bf16=0, flags=None):
    import torch
    shape, seed, n_absent, mode, tau, scope = CASES[tag]
    d = _dims(shape)
    w = _weights(d)
    vals, ref = _reference(tag)
    # on the reference alone: pairs do touch, and the term carries at least a tenth of the gradient on head/w
    assert vals["touching"] > 0 and vals["share"] >= 0.1, (vals["touching"], vals["share"])
    print("%s: radius %.4g px, weight %.4g, L_col %.6g, share of |d loss / d head/w| %.2f" % (tag, vals["radius"], vals["weight"], vals["L_col"], vals["share"]))
    dd = d.replace(bf16=bf16) if bf16 else d
    h, ten = _training_handle(dd, w, make_case(d, seed=seed, n_absent=n_absent))
    if mode != MEAN:
        h.set_recon_loss(mode, tau)
        h.set_recon_scope(scope)
    ioc = [k for k in w if k.startswith("ioc/")]
    _step(h, ten)                                                            # the same step at weight 0: what the term must not reach
    torch.cuda.synchronize()
    base = (_grads(h, w, ioc), h.train_loss(ten["fut"].data_ptr()))
    h.set_collision_loss(vals["weight"], vals["radius"], 1.0 / d.sx, 1.0 / d.sy)
    _step(h, ten)
    torch.cuda.synchronize()
    return h, ten, w, d, vals, ref, ioc, base


@pytest.mark.parametrize("tag", list(CASES))
def test_training_gradients_match_float64_autograd(tag):
    h, ten, w, d, vals, ref, ioc, base = _collision_step(tag)
    _check_done_gradients(h, w, ref)
    # the IOC module sees detached trajectories, and KL / cross-entropy / regression do not see the term: bit for bit the step at weight 0
    now = _grads(h, w, ioc)
    for k in ioc:
        np.testing.assert_array_equal(_bits(now[k]), _bits(base[0][k]), err_msg=k)
    loss = h.train_loss(ten["fut"].data_ptr())
    for key in ("recon", "kld", "ce", "reg", "n_present"):
        assert loss[key] == base[1][key], key
    # 7. col_term reports what is trained: the float rule against the float64 L_col (a pure number)
    got = float(h.device_tensor("col_term").cpu().numpy()[0])
    Y0 = h.read_buffer("Y0", (d.R, d.T_pred, 2))
    fut, valid = ten["fut"].cpu().numpy(), h.device_tensor("valid", "|u1").cpu().numpy()[: d.A]
    f32 = collision_f32(Y0, fut, valid, vals["radius"], 1.0 / d.sx, 1.0 / d.sy, d)
    f64 = collision_f64(Y0, fut, valid, vals["radius"], 1.0 / d.sx, 1.0 / d.sy, d)
    assert np.float32(got).view(np.uint32) == f32["term"].view(np.uint32)[0]      # the step's kernel is the op's: the bits of the statement on the device's Y0
    np.testing.assert_array_equal(h.device_tensor("col_touch", "<i4").cpu().numpy()[: d.n_scenes * d.K].reshape(d.n_scenes, d.K), f32["touch"])
    bar = max(4.0 * abs(float(f32["term"][0]) - float(f64["term"][0])), 1e-5)
    print("%s: col_term %.9g, float64 L_col of the oracle %.9g (bar %.3g)" % (tag, got, vals["L_col"], bar))
    assert abs(got - float(f64["term"][0])) <= bar
    # against the oracle's own trajectories: phi is Lipschitz in the distance with constant 2 / radius, a pair's distance moves by at most twice
    # the largest displacement of a position (measured here between the device's Y0 and the oracle's, in the unit of the radius), and `near` is
    # L_col's reduction of the number of partners that can contribute -- so |L_col(device Y0) - L_col(oracle Y0)| <= (2 / radius) * 2 delta * near
    dev = (Y0.astype(np.float64) - vals["Y0"]) * np.array([1.0 / d.sx, 1.0 / d.sy])
    delta = float(np.sqrt((dev ** 2).sum(-1)).max())
    lip = 2.0 / vals["radius"] * 2.0 * delta * vals["near"]
    print("%s: largest displacement device - oracle %.3g px, Lipschitz bound %.3g, |col_term - oracle L_col| = %.3g" % (tag, delta, lip, abs(got - vals["L_col"])))
    assert abs(got - vals["L_col"]) <= lip + bar, (got, vals["L_col"], lip, bar)
    h.close()


def test_training_gradients_with_split_operands():
    """dims.bf16 = 2: tests/test_gpu_split.py's bar for this configuration (2e-4 on its first case, which is this one)."""
    h, ten, w, d, vals, ref, ioc, base = _collision_step("mean", bf16=2)
    _check_done_gradients(h, w, ref, tol=2e-4)
    h.close()


# ---- 8. compacted rows ----------------------------------------------------------------------------------------------------------------------------
def test_compacted_step_matches_the_padded_one():
    """DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC: the term is taken on the full layout before the gather; held to what
    tests/test_gpu_compact_rows.py holds the mean-mode step on slot classes to (loss terms 2e-6, gradients 3e-5 of the largest entry)."""
    import torch
    from tests.test_gpu_compact_rows import _spread, ragged_counts
    d = small_dims(n_scenes=8, K=3, T_obs=6, T_pred=7, n_grids=1)
    w = _spread(init_weights(d, 41))
    case = ragged_counts(d, seed=44, counts=[3, 9, 0, 14, 8, d.mno, 1, 20])
    res = []
    for dd, min_rows in ((d, None), (d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC), 0)):
        h, ten = _training_handle(dd, w, case, min_rows)
        h.set_collision_loss(0.5, 400.0, 1.0 / d.sx, 1.0 / d.sy)
        _step(h, ten)
        torch.cuda.synchronize()
        res.append((h.train_loss(ten["fut"].data_ptr()), _grads(h, w), h.device_tensor("col_touch", "<i4").cpu().numpy()[: d.n_scenes * d.K].copy(),
                    h.device_tensor("col_val").cpu().numpy()[: d.A * d.K].copy(), float(h.device_tensor("col_term").cpu().numpy()[0])))
        h.close()
    (la, ga, ta, ca, ma), (lb, gb, tb, cb, mb) = res
    assert ta.sum() > 0 and ma > 0
    np.testing.assert_array_equal(ta, tb)
    assert np.abs(ca - cb).max() <= 2e-6 * max(1.0, np.abs(ca).max()) and abs(ma - mb) <= 2e-6 * max(1.0, abs(ma))
    for key in ("recon", "kld", "ce", "reg", "loss"):
        assert abs(la[key] - lb[key]) <= 2e-6 * max(1.0, abs(la[key])), (key, la[key], lb[key])
    worst = ("", 0.0)
    for k in ga:
        if k == "ioc/score/b":
            assert np.abs(gb[k]).max() < 1e-6
            continue
        ref = np.abs(ga[k]).max()
        err = float(np.abs(ga[k] - gb[k]).max() / (ref + 1e-12)) if ref > 1e-9 else float(np.abs(gb[k]).max())
        if err > worst[1]:
            worst = (k, err)
        assert np.isfinite(gb[k]).all()
    print("slot classes vs padded step with the collision term: worst relative gradient difference %.2e (%s)" % (worst[1], worst[0]))
    assert worst[1] < 3e-5, worst


# ---- 9. capture -----------------------------------------------------------------------------------------------------------------------------------
def test_step_with_the_term_replays_from_a_hipgraph():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    h, ten = _training_handle(d, w, make_case(d, seed=42, n_absent=4))
    h.set_collision_loss(0.5, 400.0, 1.0 / d.sx, 1.0 / d.sy)
    side = torch.cuda.Stream()
    sp = side.cuda_stream

    def step(stream):
        _step(h, ten, stream)
        h.clip_grads(1e-3, stream=stream)

    torch.cuda.synchronize()
    step(sp)                                             # warm-up outside capture: lazy allocations and function attributes
    side.synchronize()
    g_ref, Y_ref = h.grad_tensor().clone(), ten["Y"].clone()
    c_ref, t_ref = h.device_tensor("col_val").clone(), h.device_tensor("col_touch", "<i4").clone()
    assert int(t_ref.sum()) > 0
    step(sp)                                             # a second eager run: the same bits
    side.synchronize()
    assert torch.equal(h.grad_tensor(), g_ref) and torch.equal(ten["Y"], Y_ref) and torch.equal(h.device_tensor("col_val"), c_ref)
    h.graph_begin(sp)
    step(sp)
    gid = h.graph_end(sp)
    for _ in range(3):
        h.grad_tensor().zero_(); ten["Y"].zero_(); h.device_tensor("col_val").zero_(); h.device_tensor("col_touch", "<i4").zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        assert torch.equal(ten["Y"], Y_ref)
        assert torch.equal(h.device_tensor("col_val"), c_ref) and torch.equal(h.device_tensor("col_touch", "<i4"), t_ref)
        assert torch.equal(h.grad_tensor(), g_ref)
    assert float(g_ref.abs().max()) > 0
    h.close()


# ---- 10. the term moves what it should --------------------------------------------------------------------------------------------------------------
def test_the_term_lowers_the_penalty_on_a_fixed_batch():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    vals, _ = _reference("mean")
    radius, weight = vals["radius"], vals["weight"]
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    run = {}
    for tag, wt in (("on", weight), ("off", 0.0)):
        h, ten = _training_handle(d, w, make_case(d, seed=42, n_absent=4))
        if wt > 0:
            h.set_collision_loss(wt, radius, ux, uy)
        term, touch = torch.zeros(1, device="cuda"), torch.zeros((d.n_scenes, d.K), device="cuda", dtype=torch.int32)
        trace = []
        for it in range(41):                             # the steps of tests/test_gpu_train.py::test_loss_decreases_on_a_fixed_batch
            _step(h, ten)
            if it in (0, 40):                            # the op on the step's own Y0: the same read-out with the term on and off
                h.collision_loss(ten["fut"].data_ptr(), h.device_tensor("Y0").data_ptr(), radius, ux, uy, 0, touch.data_ptr(), 0, term.data_ptr())
                torch.cuda.synchronize()
                trace.append((float(term[0]), int(touch.sum())))
            if it == 40:
                break
            h.clip_grads(10.0)
            h.adam_step(0.002)
        run[tag] = trace
        h.close()
    print("L_col, touch: with the term %s, without %s" % (run["on"], run["off"]))
    assert run["on"][0] == run["off"][0] and run["on"][0][0] > 0
    assert run["on"][1][0] < run["on"][0][0]                                 # the term went down,
    assert run["on"][1][1] <= run["on"][0][1]                                # the touching (pair, frame)s did not go up,
    assert run["on"][1][0] < run["off"][1][0]                                # and it ends below the control


# ---- 11. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    import torch
    from desire_amd import _lib
    d = _dims((2, 8, 3, 7))
    w = _weights(d)
    h, ten = _training_handle(d, w, make_case(d, seed=84, n_absent=2))
    lib = h.lib
    A = d.n_scenes * d.mno
    col = torch.full((A, d.K), -7.0, device="cuda")
    dY = torch.full((d.R, d.T_pred, 2), -7.0, device="cuda")
    fp, yp, cp, dp = ten["fut"].data_ptr(), ten["Y"].data_ptr(), col.data_ptr(), dY.data_ptr()
    nan, inf = float("nan"), float("inf")
    assert lib.desire_collision_loss(None, fp, yp, 1.0, 1.0, 1.0, cp, None, dp, None, None) == -1 and b"handle" in lib.desire_last_error()
    assert lib.desire_collision_loss(h._h, None, yp, 1.0, 1.0, 1.0, cp, None, dp, None, None) == -1 and b"dev_fut" in lib.desire_last_error()
    assert lib.desire_collision_loss(h._h, fp, None, 1.0, 1.0, 1.0, cp, None, dp, None, None) == -1 and b"dev_Yhat" in lib.desire_last_error()
    for r in (-1.0, nan, inf):
        assert lib.desire_collision_loss(h._h, fp, yp, r, 1.0, 1.0, cp, None, dp, None, None) == -1 and b"radius" in lib.desire_last_error(), r
        assert lib.desire_set_collision_loss(h._h, 1.0, r, 1.0, 1.0) == -1 and b"radius" in lib.desire_last_error(), r
    for u in (0.0, -1.0, nan, inf):
        assert lib.desire_collision_loss(h._h, fp, yp, 1.0, u, 1.0, cp, None, dp, None, None) == -1 and b"unit_x" in lib.desire_last_error(), u
        assert lib.desire_collision_loss(h._h, fp, yp, 1.0, 1.0, u, cp, None, dp, None, None) == -1 and b"unit_y" in lib.desire_last_error(), u
        assert lib.desire_set_collision_loss(h._h, 1.0, 1.0, u, 1.0) == -1 and lib.desire_set_collision_loss(h._h, 1.0, 1.0, 1.0, u) == -1
    for wt in (-1.0, nan, inf):
        assert lib.desire_set_collision_loss(h._h, wt, 1.0, 1.0, 1.0) == -1 and b"weight" in lib.desire_last_error(), wt
    with pytest.raises(_lib.DesireError):
        h.set_collision_loss(1.0, -2.0)
    hr = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    assert lib.desire_collision_loss(hr._h, fp, yp, 1.0, 1.0, 1.0, cp, None, dp, None, None) == -1 and b"ref_compat" in lib.desire_last_error()
    assert lib.desire_set_collision_loss(hr._h, 1.0, 1.0, 1.0, 1.0) != 0 and b"ref_compat" in lib.desire_last_error()
    hr.close()
    torch.cuda.synchronize()
    assert bool((col == -7.0).all()) and bool((dY == -7.0).all())          # nothing was launched or written
    with pytest.raises(Exception):
        h.device_tensor("col_term")                                           # and nothing allocated
    h.set_collision_loss(0.5, 400.0, 1.0 / d.sx, 1.0 / d.sy)                  # the handle still trains, with the term
    _step(h, ten)
    torch.cuda.synchronize()
    assert np.isfinite(h.train_loss(ten["fut"].data_ptr())["loss"]) and float(h.grad_tensor().abs().max()) > 0
    assert np.isfinite(float(h.device_tensor("col_term")[0]))
    h.close()


# ---- 12. the host surface --------------------------------------------------------------------------------------------------------------------------
def test_model_reaches_the_handle():
    from types import SimpleNamespace
    from desire_amd.model import DESIREModel
    base = dict(seq_length=6, pred_length=7, d_dim=64, rnn_size=512, latent_size=64, max_num_obj=8, learning_rate=0.0005, grad_clip=10.0,
                neighborhood_size=256, grid_size=4, num_samples=3, batch_size=2)
    rng = np.random.default_rng(0)
    ids = np.arange(1, 9, dtype=np.float32)[None, :, None]
    x = [np.concatenate([ids.repeat(6, 0), rng.uniform(200, 1800, (6, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    y = [np.concatenate([ids.repeat(7, 0), rng.uniform(200, 1800, (7, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    m = DESIREModel(SimpleNamespace(**base), seed=3)
    terms = m.train_step(x, y, seed=1)
    assert "col" not in terms
    with pytest.raises(Exception):
        m._trained.device_tensor("col_term")                                  # the default never allocates or runs the new code
    # a fresh model's samples of one agent nearly coincide and the agents start hundreds of pixels apart: a radius that spans the frame
    m = DESIREModel(SimpleNamespace(collision_weight=0.5, collision_radius=3000.0, **base), seed=3)
    terms = m.train_step(x, y, seed=1)
    h = m._trained
    assert np.isfinite(terms["loss"]) and terms["col"] > 0
    assert terms["col"] == float(h.device_tensor("col_term")[0])
    assert int(h.device_tensor("col_touch", "<i4")[: h.dims.n_scenes * h.dims.K].sum()) > 0
    pend = m.train_step(x, y, seed=1, sync=False)
    assert pend.get()["col"] > 0
    m2 = DESIREModel(SimpleNamespace(collision_weight=0.5, collision_radius=3000.0, collision_loss_radius=1.0, **base), seed=3)
    assert m2.train_step(x, y, seed=1)["col"] == 0.0                          # the loss radius of its own wins: nobody within a pixel
    for bad in (dict(collision_weight=0.5), dict(collision_weight=0.5, collision_radius=0.0), dict(collision_weight=-1.0, collision_radius=5.0)):
        with pytest.raises(ValueError):
            DESIREModel(SimpleNamespace(**bad, **base), seed=3).train_step(x, y, seed=1)


def test_train_runs_an_epoch_with_the_collision_column(tmp_path):
    import re
    from desire_amd import train as T
    common = ["--batch_size", "2", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--d_dim", "64", "--latent_size", "64",
              "--num_samples", "5", "--neighborhood_size", "256", "--num_epochs", "1", "--prefetch", "0", "--save_dir", str(tmp_path)]
    t = np.arange(10, dtype=np.float32)
    win = np.zeros((2, 10, 8, 3), np.float32)                         # two windows of four objects walking straight lines
    for n in range(2):
        for i in range(4):
            win[n, :, i, 0] = i + 1
            win[n, :, i, 1] = 200 + 150 * i + (3 + n) * t
            win[n, :, i, 2] = 150 + 100 * i + 2 * t

    class Loader:                                                     # the reference loader's surface (next_batch only): the serial loop
        seq_length, num_batches = 10, 2

        def reset_batch_pointer(self):
            pass

        def next_batch(self):
            return list(win), None, [0, 0]

    lines = []
    a = T.build_parser().parse_args(common + ["--collision_weight", "0.25", "--collision_radius", "60", "--collision_loss_radius", "2000"])
    losses = T.train(a, data_loader=Loader(), log=lines.append)
    assert len(losses) == 2 and np.isfinite(losses).all()
    steps = [ln for ln in lines if "train_loss" in ln]
    assert len(steps) == 2 and all(re.search(r", col\[r=2000 w=0\.25\] [0-9.]+$", ln) for ln in steps), steps
    assert float(steps[0].rsplit(" ", 1)[1]) > 0
    plain = []
    T.train(T.build_parser().parse_args(common), data_loader=Loader(), log=plain.append)
    assert all(re.fullmatch(r"\d+/2 \(epoch 0\), train_loss = [0-9.]+, time/batch = [0-9.]+", ln) for ln in plain if "train_loss" in ln), plain
    with pytest.raises(ValueError):
        T.train(T.build_parser().parse_args(common + ["--collision_weight", "0.25"]), data_loader=Loader(), log=plain.append)
