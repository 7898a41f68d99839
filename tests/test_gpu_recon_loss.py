"""Best-of-many / soft-min reconstruction loss on the device (desire_set_recon_loss, desire_recon_weights; csrc/kernels_recon.hip,
k_loss_grad_y_w) against the numpy statements of its contract and float64 autograd of the rebuilt loss (tests/recon_reference.py).
Shapes are (n_scenes, mno, K, T_pred) on small_dims(T_obs=6, n_grids=1)."""
import functools

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import MISALIGNED_SHAPES, at_byte_offset, make_case, small_dims, to_oracle_layout
from tests.recon_reference import MEAN, MIN, SOFTMIN, bom_loss_and_grads, make_recon_case, recon_f32, recon_f64

pytestmark = pytest.mark.gpu

TAU = 0.01


def _dims(shape, **kw):
    n, m, K, T = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=6, T_pred=T, n_grids=1, **kw)


def _weights(d):
    from tests.stage_reference import spread_weights
    return spread_weights(init_weights(d, 41))


@functools.lru_cache(maxsize=None)
def _reference(shape, seed, n_absent, mode, tau):
    """Float64 autograd of the loss under `mode` on make_case(seed, n_absent): computed once per case, shared, never modified."""
    d = _dims(shape)
    past, fut, eps, grids, gos = make_case(d, seed=seed, n_absent=n_absent)
    return bom_loss_and_grads(to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos, _weights(d), d, mode, tau)


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _training_handle(d, w, case, min_rows=None):
    import torch
    from desire_amd import _lib
    past, fut, eps, grids, gos = case[:5]
    h = _lib.Handle(d)
    h.set_weights(w)
    if min_rows is not None:
        h.set_option("compact_min_rows", min_rows)
    h.set_training(True)
    ten = dict(past=_t(past), fut=_t(fut), eps=_t(eps), grids=_t(grids))
    h.set_scene_grids(ten["grids"].data_ptr(), gos)
    ten["Y"] = torch.zeros((d.R, d.T_pred, 2), device="cuda")
    ten["score"] = torch.zeros((d.R,), device="cuda")
    return h, ten


def _step(h, ten, stream=0):
    h.forward(ten["past"].data_ptr(), ten["fut"].data_ptr(), ten["eps"].data_ptr(), ten["Y"].data_ptr(), ten["score"].data_ptr(), stream)
    h.backward(ten["past"].data_ptr(), ten["fut"].data_ptr(), ten["eps"].data_ptr(), stream)


def _grads(h, w, names=None):
    return {k: h.get_grad(k, w[k].shape) for k in (names or w) if not k.startswith("gauss_head/") and "/moving_" not in k and "/gamma" not in k and "/beta" not in k}


def _check_done_gradients(h, w, ref, tol=2e-4):
    from tests.test_gpu_train import DONE, rel_err
    bad, worst = {}, ("", 0.0)
    for name in DONE:
        got = h.get_grad(name, w[name].shape)
        assert np.isfinite(got).all(), name
        if name == "ioc/score/b":       # softmax over K is shift invariant: the exact gradient is 0
            assert np.abs(got).max() < 1e-6
            continue
        r = rel_err(got, ref[name])
        if not r <= worst[1]:
            worst = (name, r)
        if not r < tol:
            bad[name] = r
    print("worst gradient of %d names: %s at %.2e of its largest float64 entry (bar %.0e)" % (len(DONE), worst[0], worst[1], tol))
    assert not bad, bad


# ---- 1. the op against the numpy statements -----------------------------------------------------------------------------------------------
def _op(h, d, fut_t, Y_t, mode, tau, want=(True, True, True, True)):
    import torch
    A = d.n_scenes * d.mno
    out = {"e": torch.full((A, d.K), -7.0, device="cuda") if want[0] else None, "w": torch.full((A, d.K), -7.0, device="cuda") if want[1] else None,
           "winner": torch.full((A,), -7, device="cuda", dtype=torch.int32) if want[2] else None,
           "recon": torch.full((A,), -7.0, device="cuda") if want[3] else None}
    p = lambda k: out[k].data_ptr() if out[k] is not None else 0
    h.recon_weights(fut_t.data_ptr(), Y_t.data_ptr(), mode, tau, p("e"), p("w"), p("winner"), p("recon"))
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("shape", [(2, 8, 3, 7), (3, 1, 1, 7), (1, 32, 20, 40), (2, 32, 70, 5)])
def test_op_matches_the_contract(shape):
    from desire_amd import _lib
    d = _dims(shape)
    Y, fut, valid, ties = make_recon_case(d, seed=100 + sum(shape))
    # `valid` reaches the handle the way it does in use: desire_encode reads it off the last observed frame
    past = np.zeros((d.n_scenes, d.T_obs, d.mno, 3), np.float32)
    past[..., 0] = valid.reshape(d.n_scenes, 1, d.mno)
    past[..., 1:] = np.random.default_rng(3).uniform(200, 900, past[..., 1:].shape) * (past[..., :1] != 0)
    h = _lib.Handle(d)
    h.set_weights(init_weights(d, 41))
    past_t, fut_t, Y_t = _t(past), _t(fut), _t(Y)
    h.encode(past_t.data_ptr(), fut_t.data_ptr())
    np.testing.assert_array_equal(h.device_tensor("valid", "|u1").cpu().numpy()[: valid.size], valid)

    f32, f64 = recon_f32(Y, fut, valid, d, MIN), recon_f64(Y, fut, valid, d, MIN)
    got = _op(h, d, fut_t, Y_t, MIN, 0.0)
    np.testing.assert_array_equal(got["e"].view(np.uint32), f32["e"].view(np.uint32))
    np.testing.assert_array_equal(got["recon"].view(np.uint32), f32["recon"].view(np.uint32))
    np.testing.assert_array_equal(got["winner"], f32["winner"])
    np.testing.assert_array_equal(got["winner"], f64["winner"])                # ties included: the lower k in either precision
    np.testing.assert_array_equal(got["w"], f32["w"])
    assert (got["w"].sum(1) == 1).all() and (got["e"][~f32["lmask"]] == 0).all()

    m0 = _op(h, d, fut_t, Y_t, MEAN, 0.0)                                      # the mean form of the op: the same e and winner, w = 1 / K
    r0 = recon_f32(Y, fut, valid, d, MEAN)
    for k in ("e", "w", "recon"):
        np.testing.assert_array_equal(m0[k].view(np.uint32), r0[k].view(np.uint32))
    np.testing.assert_array_equal(m0["winner"], f32["winner"])

    for tau in (0.01, 1.0):
        s32, s64 = recon_f32(Y, fut, valid, d, SOFTMIN, tau), recon_f64(Y, fut, valid, d, SOFTMIN, tau)
        g = _op(h, d, fut_t, Y_t, SOFTMIN, tau)
        np.testing.assert_array_equal(g["e"].view(np.uint32), f32["e"].view(np.uint32))
        np.testing.assert_array_equal(g["winner"], f32["winner"])
        for key in ("w", "recon"):
            basis = float(np.abs(s32[key].astype(np.float64) - s64[key]).max())
            bar = max(4.0 * basis, 1e-5)
            err = float(np.abs(g[key].astype(np.float64) - s64[key]).max())
            print("shape %s tau %g: max |%s - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g" % (shape, tau, key, err, basis, bar))
            assert err <= bar, (key, tau, err, bar)

    # all sixteen NULL / non-NULL output choices write the same bits into what they do write
    full = _op(h, d, fut_t, Y_t, SOFTMIN, 0.01)
    for mask in range(16):
        want = tuple(bool(mask >> i & 1) for i in range(4))
        part = _op(h, d, fut_t, Y_t, SOFTMIN, 0.01, want)
        for k, on in zip(("e", "w", "winner", "recon"), want):
            if on:
                np.testing.assert_array_equal(part[k].view(np.uint32), full[k].view(np.uint32))
            else:
                assert part[k] is None
    h.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_op_on_a_sample_tensor_off_16_byte_alignment(shape, off):
    """The 8-byte path of the streaming loop for a whole buffer: the contract as test_op_matches_the_contract holds it, and the aligned call's bits."""
    from desire_amd import _lib
    d = _dims(shape)
    Y, fut, valid, _ = make_recon_case(d, seed=100 + sum(shape))
    past = np.zeros((d.n_scenes, d.T_obs, d.mno, 3), np.float32)
    past[..., 0] = valid.reshape(d.n_scenes, 1, d.mno)
    past[..., 1:] = np.random.default_rng(3).uniform(200, 900, past[..., 1:].shape) * (past[..., :1] != 0)
    h = _lib.Handle(d)
    h.set_weights(init_weights(d, 41))
    past_t, fut_t, Y_t = _t(past), _t(fut), _t(Y)
    Y_off = at_byte_offset(Y_t, off)
    h.encode(past_t.data_ptr(), fut_t.data_ptr())
    for mode, tau in ((MIN, 0.0), (MEAN, 0.0), (SOFTMIN, TAU)):
        f32, f64 = recon_f32(Y, fut, valid, d, mode, tau), recon_f64(Y, fut, valid, d, mode, tau)
        got = _op(h, d, fut_t, Y_off, mode, tau)
        np.testing.assert_array_equal(got["e"].view(np.uint32), f32["e"].view(np.uint32))
        np.testing.assert_array_equal(got["winner"], f32["winner"])
        np.testing.assert_array_equal(got["winner"], f64["winner"])
        for key in ("w", "recon"):
            if mode == SOFTMIN:
                basis = float(np.abs(f32[key].astype(np.float64) - f64[key]).max())
                bar = max(4.0 * basis, 1e-5)
                err = float(np.abs(got[key].astype(np.float64) - f64[key]).max())
                print("offset %d: max |%s - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g" % (off, key, err, basis, bar))
                assert err <= bar, (key, err, bar)
            else:
                np.testing.assert_array_equal(got[key].view(np.uint32), f32[key].view(np.uint32))
        aligned = _op(h, d, fut_t, Y_t, mode, tau)
        for key in got:
            np.testing.assert_array_equal(got[key].view(np.uint32), aligned[key].view(np.uint32), err_msg=key)
    h.close()


# ---- 2. the default is untouched ------------------------------------------------------------------------------------------------------------
def test_mean_mode_leaves_every_bit_as_it_was():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    case = make_case(d, seed=42, n_absent=4)
    res = []
    for touch in (True, False):
        h, ten = _training_handle(d, w, case)
        if touch:
            h.set_recon_loss(0, 123.0)
        _step(h, ten)
        torch.cuda.synchronize()
        res.append((h.grad_tensor().clone(), h.train_loss(ten["fut"].data_ptr()), ten["Y"].clone()))
        h.close()
    assert float(res[0][0].abs().max()) > 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])
    assert res[0][1] == res[1][1]


# ---- 3. / 4. gradients against float64 autograd -----------------------------------------------------------------------------------------------
def test_softmin_gradients_match_float64_autograd():
    import torch
    shape = (2, 32, 3, 7)
    d = _dims(shape)
    w = _weights(d)
    vals, ref = _reference(shape, 42, 4, SOFTMIN, TAU)
    c = vals["counted"]
    spread = (vals["e"][c].max(1) - vals["e"][c].min(1)).mean()
    assert spread > TAU                                                        # the weights are far from uniform at this temperature
    h, ten = _training_handle(d, w, make_case(d, seed=42, n_absent=4))
    h.set_recon_loss(SOFTMIN, TAU)
    _step(h, ten)
    torch.cuda.synchronize()
    _check_done_gradients(h, w, ref)
    h.close()


@pytest.mark.parametrize("shape,seed,n_absent,n_counted", [((2, 8, 3, 7), 84, 2, 12), ((3, 1, 3, 7), 99, 0, 3)])
def test_hard_min_gradients_match_float64_autograd(shape, seed, n_absent, n_counted):
    """Both cases keep every counted agent's two smallest float64 errors at least 1e-4 apart, the device picks the float64 winners, and every
    gradient is held to 2e-4 of the largest entry of its float64 counterpart.

    Measured on one MI355X: (2, 8, 3, 7), seed 84, worst name vae_dec/deconv1/w at 9.0e-6; (3, 1, 3, 7), seed 99, vae_dec/deconv2/b at 1.2e-5.
    The second case is the one that needs the centred mask backward (k_mask_bwd<true>): its three winner rows have a softmax mask
    within 2e-4 of one-hot, where the plain fp32 form loses mask_fc/w and vae_dec/* to cancellation (2.2e-4 - 5.7e-4 there)."""
    import torch
    d = _dims(shape)
    w = _weights(d)
    vals, ref = _reference(shape, seed, n_absent, MIN, 0.0)
    c = vals["counted"]
    # on the float64 reference alone: every counted agent's best and second-best error are at least 1e-4 apart, five times the recorded
    # device-to-oracle trajectory deviation -- nobody is left out
    assert c.sum() == n_counted and (vals["gap"][c] >= 1e-4).all(), vals["gap"][c].min()
    h, ten = _training_handle(d, w, make_case(d, seed=seed, n_absent=n_absent))
    h.set_recon_loss(MIN)
    _step(h, ten)
    torch.cuda.synchronize()
    win = h.device_tensor("recon_win", "<i4").cpu().numpy()[: d.A]
    np.testing.assert_array_equal(win[c], vals["winner"][c])
    _check_done_gradients(h, w, ref)
    h.close()


def test_softmin_gradients_with_split_operands():
    """dims.bf16 = 2 in mode SOFTMIN: tests/test_gpu_split.py's bar for this configuration (2e-4 on its first case, which is this one)."""
    import torch
    shape = (2, 32, 3, 7)
    d = _dims(shape)
    w = _weights(d)
    _, ref = _reference(shape, 42, 4, SOFTMIN, TAU)
    h, ten = _training_handle(d.replace(bf16=2), w, make_case(d, seed=42, n_absent=4))
    h.set_recon_loss(SOFTMIN, TAU)
    _step(h, ten)
    torch.cuda.synchronize()
    _check_done_gradients(h, w, ref, tol=2e-4)
    h.close()


# ---- 5. anchors, bitwise ------------------------------------------------------------------------------------------------------------------------
def test_modes_share_everything_but_the_reconstruction_gradient():
    import torch
    shape = (2, 8, 3, 7)
    d = _dims(shape)
    w = _weights(d)
    h, ten = _training_handle(d, w, make_case(d, seed=84, n_absent=2))
    ioc = [k for k in w if k.startswith("ioc/")]
    res = {}
    for tag, mode, tau in (("mean", MEAN, 0.0), ("min", MIN, 0.0), ("softmin", SOFTMIN, TAU), ("cold", SOFTMIN, 1e-6)):
        h.set_recon_loss(mode, tau)
        _step(h, ten)                                                          # the same forward every time: the same bits
        torch.cuda.synchronize()
        res[tag] = (h.grad_tensor().clone(), h.train_loss(ten["fut"].data_ptr()), _grads(h, w, ioc), ten["Y"].clone())
    for tag in ("min", "softmin", "cold"):
        assert torch.equal(res[tag][3], res["mean"][3])
        for k in ioc:                                                          # the IOC module sees detached trajectories
            np.testing.assert_array_equal(res[tag][2][k].view(np.uint32), res["mean"][2][k].view(np.uint32))
        for key in ("kld", "ce", "reg", "n_present"):
            assert res[tag][1][key] == res["mean"][1][key], (tag, key)
        assert not torch.equal(res[tag][0], res["mean"][0])
    # gap / tau >= 140 > 104: every loser's expf is 0.f at tau = 1e-6, the weights are exactly one-hot and the step is the hard-min step
    assert torch.equal(res["cold"][0], res["min"][0])
    assert res["min"][1]["recon"] <= res["softmin"][1]["recon"] <= res["mean"][1]["recon"]
    assert res["min"][1]["recon"] < res["mean"][1]["recon"]
    h.close()


# ---- 6. the reported loss -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tau", [(MIN, 0.0), (SOFTMIN, TAU)])
def test_train_loss_reports_the_term_that_is_trained(mode, tau):
    import torch
    shape = (2, 8, 3, 7)
    d = _dims(shape)
    w = _weights(d)
    vals, _ = _reference(shape, 84, 2, mode, tau)
    h, ten = _training_handle(d, w, make_case(d, seed=84, n_absent=2))
    h.set_recon_loss(mode, tau)
    h.forward(ten["past"].data_ptr(), ten["fut"].data_ptr(), ten["eps"].data_ptr(), ten["Y"].data_ptr(), ten["score"].data_ptr())
    got = h.train_loss(ten["fut"].data_ptr())                                  # before any backward: the call computes the term itself
    v = vals["counted"]
    n = max(v.sum(), 1)
    for key in ("recon", "kld", "ce", "reg"):
        want = float((vals[key] * v).sum() / n)
        print("mode %d %s: got %.9g want %.9g" % (mode, key, got[key], want))
        assert abs(got[key] - want) <= 2e-5 * max(1.0, abs(want)), (key, got[key], want)
    assert got["n_present"] == n
    assert abs(got["loss"] - vals["loss"]) < 1e-4 * max(1.0, abs(vals["loss"]))
    dev8 = torch.zeros(8, device="cuda")
    h.train_loss_async(ten["fut"].data_ptr(), dev8.data_ptr())
    torch.cuda.synchronize()
    assert float(dev8[0]) == got["recon"]
    h.close()


# ---- 7. compacted rows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tau", [(MIN, 0.0), (SOFTMIN, TAU)])
def test_compacted_step_matches_the_padded_one(mode, tau):
    """DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC: the weights are taken on the full layout before the gather; held to what
    tests/test_gpu_compact_rows.py holds the mean-mode step on slot classes to (loss terms 2e-6, gradients 3e-5 of the largest entry)."""
    import torch
    from tests.test_gpu_compact_rows import _spread, ragged_counts
    d = small_dims(n_scenes=8, K=3, T_obs=6, T_pred=7, n_grids=1)
    w = _spread(init_weights(d, 41))
    case = ragged_counts(d, seed=44, counts=[3, 9, 0, 14, 8, d.mno, 1, 20])
    res = []
    for dd, min_rows in ((d, None), (d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC), 0)):
        h, ten = _training_handle(dd, w, case, min_rows)
        h.set_recon_loss(mode, tau)
        _step(h, ten)
        torch.cuda.synchronize()
        res.append((h.train_loss(ten["fut"].data_ptr()), _grads(h, w), h.device_tensor("recon_win", "<i4").cpu().numpy()[: d.A].copy()))
        h.close()
    (la, ga, wa), (lb, gb, wb) = res
    np.testing.assert_array_equal(wa, wb)
    for key in ("recon", "kld", "ce", "reg", "loss"):
        assert abs(la[key] - lb[key]) <= 2e-6 * max(1.0, abs(la[key])), (key, la[key], lb[key])
    assert la["n_present"] == lb["n_present"] > 0
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
    print("mode %d, slot classes vs padded step: worst relative gradient difference %.2e (%s)" % (mode, worst[1], worst[0]))
    assert worst[1] < 3e-5, worst


# ---- 8. capture ---------------------------------------------------------------------------------------------------------------------------------------
def test_softmin_step_replays_from_a_hipgraph_and_is_reproducible():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    case = make_case(d, seed=42, n_absent=4)
    h, ten = _training_handle(d, w, case)
    h.set_recon_loss(SOFTMIN, TAU)
    side = torch.cuda.Stream()
    sp = side.cuda_stream

    def step(stream):
        _step(h, ten, stream)
        h.clip_grads(1e-3, stream=stream)

    torch.cuda.synchronize()
    step(sp)                                             # warm-up outside capture: lazy allocations and function attributes
    side.synchronize()
    g_ref, Y_ref = h.grad_tensor().clone(), ten["Y"].clone()
    w_ref = h.device_tensor("recon_w").clone()
    step(sp)                                             # a second eager run: the same bits
    side.synchronize()
    assert torch.equal(h.grad_tensor(), g_ref) and torch.equal(ten["Y"], Y_ref) and torch.equal(h.device_tensor("recon_w"), w_ref)
    h.graph_begin(sp)
    step(sp)
    gid = h.graph_end(sp)
    for _ in range(3):
        h.grad_tensor().zero_(); ten["Y"].zero_(); h.device_tensor("recon_w").zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        assert torch.equal(ten["Y"], Y_ref)
        assert torch.equal(h.device_tensor("recon_w"), w_ref)
        assert torch.equal(h.grad_tensor(), g_ref)
    assert float(g_ref.abs().max()) > 0
    h.close()


# ---- 9. descent -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tau", [(MIN, 0.0), (SOFTMIN, TAU)])
def test_loss_decreases_on_a_fixed_batch(mode, tau):
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    h, ten = _training_handle(d, w, make_case(d, seed=42, n_absent=4))
    h.set_recon_loss(mode, tau)
    losses = []
    for _ in range(40):                                  # the steps of tests/test_gpu_train.py::test_loss_decreases_on_a_fixed_batch
        _step(h, ten)
        losses.append(h.train_loss(ten["fut"].data_ptr())["loss"])
        h.clip_grads(10.0)
        h.adam_step(0.002)
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0], losses[::8]
    h.close()


# ---- 10. refusals and the Python surface -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    import torch
    from desire_amd import _lib
    d = _dims((2, 8, 3, 7))
    w = _weights(d)
    h, ten = _training_handle(d, w, make_case(d, seed=84, n_absent=2))
    lib = h.lib
    A = d.n_scenes * d.mno
    e = torch.zeros((A, d.K), device="cuda")
    assert lib.desire_set_recon_loss(h._h, 3, 0.1) == -1 and b"mode" in lib.desire_last_error()
    assert lib.desire_set_recon_loss(h._h, -1, 0.1) == -1
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.desire_set_recon_loss(h._h, 2, tau) == -1 and b"tau" in lib.desire_last_error(), tau
        assert lib.desire_recon_weights(h._h, ten["fut"].data_ptr(), ten["Y"].data_ptr(), 2, tau, e.data_ptr(), None, None, None, None) == -1
    assert lib.desire_recon_weights(h._h, ten["fut"].data_ptr(), ten["Y"].data_ptr(), 3, 0.1, e.data_ptr(), None, None, None, None) == -1
    assert lib.desire_recon_weights(h._h, None, ten["Y"].data_ptr(), 1, 0.0, e.data_ptr(), None, None, None, None) == -1
    assert lib.desire_recon_weights(h._h, ten["fut"].data_ptr(), None, 1, 0.0, e.data_ptr(), None, None, None, None) == -1
    assert lib.desire_recon_weights(None, ten["fut"].data_ptr(), ten["Y"].data_ptr(), 1, 0.0, e.data_ptr(), None, None, None, None) == -1
    with pytest.raises(_lib.DesireError):
        h.set_recon_loss(2, 0.0)
    h.set_recon_loss(1, float("nan"))                    # tau is ignored outside SOFTMIN
    h.set_recon_loss(0, float("inf"))
    assert not e.any()                                   # nothing was launched or written
    h.set_recon_loss(SOFTMIN, TAU)                       # and the handle still trains
    _step(h, ten)
    torch.cuda.synchronize()
    assert np.isfinite(h.train_loss(ten["fut"].data_ptr())["loss"]) and float(h.grad_tensor().abs().max()) > 0
    h.close()


def test_model_reaches_the_handle():
    from types import SimpleNamespace
    from desire_amd.model import DESIREModel
    base = dict(seq_length=6, pred_length=7, d_dim=64, rnn_size=512, latent_size=64, max_num_obj=8, learning_rate=0.0005, grad_clip=10.0,
                neighborhood_size=256, grid_size=4, num_samples=3, batch_size=2)
    rng = np.random.default_rng(0)
    ids = np.arange(1, 9, dtype=np.float32)[None, :, None]
    x = [np.concatenate([ids.repeat(6, 0), rng.uniform(200, 1800, (6, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    y = [np.concatenate([ids.repeat(7, 0), rng.uniform(200, 1800, (7, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    terms = {}
    for mode, tau in (("mean", None), ("softmin", 0.05), ("min", None)):
        m = DESIREModel(SimpleNamespace(recon_loss=mode, recon_tau=tau, **base), seed=3)
        terms[mode] = m.train_step(x, y, seed=1)
        assert np.isfinite(terms[mode]["loss"])
        h = m._trained
        if mode == "mean":
            with pytest.raises(Exception):
                h.device_tensor("recon_w")                 # the default never allocates or runs the new code
        else:
            A, K = h.dims.n_scenes * h.dims.mno, h.dims.K
            wk = h.device_tensor("recon_w").cpu().numpy()[: A * K].reshape(A, K)
            np.testing.assert_allclose(wk.sum(1), 1.0, rtol=0, atol=1e-6)
            assert ((wk == 1).any(1)).all() if mode == "min" else ((wk > 0) & (wk < 1)).all()
    # (a fresh model's K samples nearly coincide: the three terms agree to fp32 rounding, which is all the order is held to here)
    assert terms["min"]["recon"] <= terms["softmin"]["recon"] + 1e-6 and terms["softmin"]["recon"] <= terms["mean"]["recon"] + 1e-6
    with pytest.raises(ValueError):
        DESIREModel(SimpleNamespace(recon_loss="softmin", recon_tau=None, **base), seed=3).train_step(x, y, seed=1)
    with pytest.raises(ValueError):
        DESIREModel(SimpleNamespace(recon_loss="best", **base), seed=3).train_step(x, y, seed=1)
