"""The recon mode, the collision term and the off-road term on the REFINED trajectories (desire_set_refined_loss; csrc/backward.hip: ioc_bwd,
csrc/train.hip: slot 3) against float64 autograd of the rebuilt loss (tests/refined_reference.py) and against the stand-alone ops on the step's
own Y.  Shapes are (n_scenes, mno, K, T_pred) on small_dims(T_obs=6, n_grids=1): (2, 8, 3, 7) with two absent agents, (2, 32, 3, 7) with four,
and an iters = 2 case at (2, 8, 3, 7).  What was observed on one MI355X is in DESIGN.md section 7q."""
import functools

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import make_case, small_dims, to_oracle_layout
from tests.offroad_reference import cell_sizes, make_masks, mask_field_f32
from tests.refined_reference import AGENT, MEAN, MIN, SCENE, SOFTMIN, Spec, refined_loss_and_grads
from tests.test_gpu_collision_loss import _bits
from tests.test_gpu_offroad_loss import _attach
from tests.test_gpu_recon_loss import TAU, _check_done_gradients, _dims, _grads, _step, _training_handle, _weights

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -2
# tag: shape, seed, absent agents, extra dims, what is on.  The seeds are chosen on the CPU, from the float64 reference alone, to meet the
# conditions _conditions() asserts before a device is asked.
CASES = {"mean8": ((2, 8, 3, 7), 47, 2, {}, Spec(rcol=True, roff=True)),
         "mean32": ((2, 32, 3, 7), 42, 4, {}, Spec(rcol=True, roff=True)),                      # tests/test_gpu_train.py's own case
         "scene_softmin": ((2, 8, 3, 7), 47, 2, {}, Spec(mode=SOFTMIN, tau=TAU, scope=SCENE, recon=True, rcol=True, roff=True)),
         "min_agent": ((2, 8, 3, 7), 47, 2, {}, Spec(mode=MIN, scope=AGENT, recon=True)),
         "min_scene": ((2, 8, 3, 7), 42, 2, {}, Spec(mode=MIN, scope=SCENE, recon=True)),       # tests/test_gpu_recon_scene.py's seed (why not 47)
         "all_four": ((2, 32, 3, 7), 42, 4, {}, Spec(rcol=True, roff=True, col=True, off=True)),
         "iters2": ((2, 8, 3, 7), 52, 2, dict(iters=2), Spec(mode=SOFTMIN, tau=TAU, scope=AGENT, recon=True, rcol=True, roff=True))}


def _case_dims(tag):
    shape, seed, n_absent, kw, spec = CASES[tag]
    return _dims(shape, **kw)


@functools.lru_cache(maxsize=None)
def _reference(tag):
    """Float64 autograd of the loss of CASES[tag]; radius, masks and weights chosen from the oracle's Y: computed once, shared, never modified."""
    shape, seed, n_absent, kw, spec = CASES[tag]
    d = _case_dims(tag)
    past, fut, eps, grids, gos = make_case(d, seed=seed, n_absent=n_absent)
    return refined_loss_and_grads(to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos, _weights(d), d, spec)


def _conditions(tag, vals):
    """On the reference alone: pairs touch on the oracle's Y, each refined term carries at least 0.1 of |d loss / d ioc/reg/w|, every counted
    position keeps 1e-4 cells from a cell line or centre line (fp32 and float64 trajectories differ by about 1e-6: a flipped cell would be a
    test artefact), and in MIN the winner leads its runner-up by 1e-3 of its error (tests/recon_reference.py's GAP)."""
    spec = vals["spec"]
    if spec.rcol:
        assert vals["touching"] > 0 and vals["L_col_Y"] > 0 and vals["share_rcol"] >= 0.1, (vals["touching"], vals["share_rcol"])
    if spec.roff:
        assert vals["margin"] >= 1e-4 and 0.25 <= vals["positive"] <= 0.75 and vals["share_roff"] >= 0.1, (vals["margin"], vals["positive"], vals["share_roff"])
    if spec.recon and spec.mode == MIN:
        assert vals["win_gap"] >= 1e-3 and vals["win_keep"].any(), vals["win_gap"]
    print("%s: radius %s px, weights rcol %s roff %s col %s off %s; shares of |d loss / d ioc/reg/w| %s / %s; margin %s cells, lead %s"
          % (tag, spec.radius, spec.rcw, spec.row, spec.cw, spec.ow, vals.get("share_rcol"), vals.get("share_roff"), vals.get("margin"), vals.get("win_gap")))


def _configure(h, d, ten, spec, refined=True):
    """The handle as `spec` says: the recon mode and scope, the radius and the field (at their Y0 weights, 0 where only the refined side is on),
    then -- with `refined` -- the refined terms."""
    if spec.mode != MEAN:
        h.set_recon_loss(spec.mode, spec.tau)
        h.set_recon_scope(spec.scope)
    if spec.col or spec.rcol:
        h.set_collision_loss(spec.cw if spec.col else 0.0, spec.radius, 1.0 / d.sx, 1.0 / d.sy)
    if spec.off or spec.roff:
        if "field" not in ten:
            ten["field"] = _attach(h, spec.masks, cell_sizes(d, spec.Mh, spec.Mw), mask_field_f32(spec.masks, *cell_sizes(d, spec.Mh, spec.Mw)),
                                   np.arange(d.n_scenes, dtype=np.int32))
        h.set_offroad_loss(spec.ow if spec.off else 0.0, spec.scale)
    if refined:
        h.set_refined_loss(1 if spec.recon else 0, spec.rcw if spec.rcol else 0.0, spec.row if spec.roff else 0.0)


def _refined_step(tag, bf16=0):
    """(h, ten, w, d, vals, ref, base): the step of CASES[tag] after the same step with the refined terms off (base = its gradients and loss words)."""
    import torch
    shape, seed, n_absent, kw, _ = CASES[tag]
    d = _case_dims(tag)
    w = _weights(d)
    vals, ref = _reference(tag)
    _conditions(tag, vals)
    spec = vals["spec"]
    h, ten = _training_handle(d.replace(bf16=bf16) if bf16 else d, w, make_case(d, seed=seed, n_absent=n_absent))
    _configure(h, d, ten, spec, refined=False)
    _step(h, ten)
    torch.cuda.synchronize()
    base = (_grads(h, w), h.train_loss(ten["fut"].data_ptr()))
    _configure(h, d, ten, spec)
    _step(h, ten)
    torch.cuda.synchronize()
    return h, ten, w, d, vals, ref, base


def _y(h, d):
    return h.device_tensor("Y_ref")[: d.R * d.T_pred * 2]


def _r_tensors(h, d, spec):
    """The refined side's tensors that `spec` fills, trimmed to their shapes."""
    A, K, n = d.A, d.K, d.n_scenes
    out = {}
    if spec.recon and spec.mode != MEAN:
        out.update(rrecon_e=h.device_tensor("rrecon_e")[: A * K], rrecon_w=h.device_tensor("rrecon_w")[: A * K],
                   rrecon_win=h.device_tensor("rrecon_win", "<i4")[:A], rrecon_val=h.device_tensor("rrecon_val")[:A])
        if spec.scope == SCENE:
            out.update(rrecon_E=h.device_tensor("rrecon_E")[: n * K], rrecon_cnt=h.device_tensor("rrecon_cnt", "<i4")[:n])
    if spec.rcol:
        out.update(rcol_val=h.device_tensor("rcol_val")[: A * K], rcol_touch=h.device_tensor("rcol_touch", "<i4")[: n * K], rcol_term=h.device_tensor("rcol_term")[:1])
    if spec.roff:
        out.update(roff_val=h.device_tensor("roff_val")[: A * K], roff_count=h.device_tensor("roff_count", "<i4")[: n * K], roff_term=h.device_tensor("roff_term")[:1])
    return out


# ---- 1. the default -----------------------------------------------------------------------------------------------------------------------------
def test_default_and_all_zero_leave_every_bit_as_it_was():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    case = make_case(d, seed=42, n_absent=4)
    res = []
    for touch in (False, True):
        h, ten = _training_handle(d, w, case)
        if touch:
            h.set_refined_loss(0, 0.0, 0.0)
        _step(h, ten)
        torch.cuda.synchronize()
        dev8 = torch.zeros(8, device="cuda")
        h.train_loss_async(ten["fut"].data_ptr(), dev8.data_ptr())
        torch.cuda.synchronize()
        res.append((h.grad_tensor().clone(), h.train_loss(ten["fut"].data_ptr()), ten["Y"].clone(), dev8))
        assert torch.equal(_y(h, d).view(d.R, d.T_pred, 2), ten["Y"])          # the tensor the terms read is the step's own output
        for name in ("rcol_term", "rcol_val", "rcol_touch", "roff_term", "roff_val", "roff_count", "rrecon_e", "rrecon_w", "rrecon_win", "rrecon_val",
                     "rrecon_E", "rrecon_cnt"):
            with pytest.raises(Exception):
                h.device_tensor(name)                                          # nothing is allocated, as "col_term" on an untouched handle
        with pytest.raises(Exception):
            h.device_tensor("col_term")
        h.close()
    assert float(res[0][0].abs().max()) > 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])
    assert res[0][1] == res[1][1]


def test_recon_flag_in_mean_mode_changes_neither_launches_nor_bits():
    import torch
    d = _dims((2, 8, 3, 7))
    w = _weights(d)
    case = make_case(d, seed=47, n_absent=2)
    res = []
    for recon in (0, 1):
        h, ten = _training_handle(d, w, case)
        h.set_refined_loss(recon, 0.0, 0.0)
        names = [("rrecon_e", "<f4"), ("rrecon_w", "<f4"), ("rrecon_win", "<i4"), ("rrecon_val", "<f4"), ("rrecon_E", "<f4"), ("rrecon_cnt", "<i4")]
        if recon:                                                             # allocated by the setter (fresh device memory holds anything): pre-filled,
            for name, dt in names:                                            # to see that mode MEAN never writes them
                h.device_tensor(name, dt).fill_(-7)
        _step(h, ten)
        torch.cuda.synchronize()
        res.append((h.grad_tensor().clone(), h.train_loss(ten["fut"].data_ptr())))
        if recon:
            for name, dt in names:
                assert bool((h.device_tensor(name, dt) == -7).all()), name
        h.close()
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


# ---- 2. float64 autograd ------------------------------------------------------------------------------------------------------------------------
def _check_winner(h, d, vals):
    spec = vals["spec"]
    win = h.device_tensor("rrecon_win", "<i4").cpu().numpy()[: d.A]
    if spec.scope == SCENE:
        keep = np.repeat(vals["win_keep"], d.mno)
        np.testing.assert_array_equal(win[keep], np.repeat(vals["winner"], d.mno)[keep])       # the window's winner on every slot of the window
    else:
        np.testing.assert_array_equal(win[vals["win_keep"]], vals["winner"][vals["win_keep"]])


@pytest.mark.parametrize("tag", ["mean8", "mean32", "scene_softmin", "min_agent", "min_scene", "all_four", "iters2"])
def test_training_gradients_match_float64_autograd(tag):
    h, ten, w, d, vals, ref, base = _refined_step(tag)
    spec = vals["spec"]
    if spec.recon and spec.mode == MIN:
        _check_winner(h, d, vals)
    _check_done_gradients(h, w, ref)
    # the terms that are reported, against the oracle's own: phi of either penalty is Lipschitz in the positions and the fp32 Y is about 1e-6 from
    # the float64 one, so 1e-4 of max(1, term) is generous (the bits are section 4's)
    for key, name in (("L_col_Y", "rcol_term"), ("L_off_Y", "roff_term")):
        if key in vals:
            got = float(h.device_tensor(name)[0])
            print("%s: %s %.9g, float64 %.9g" % (tag, name, got, vals[key]))
            assert abs(got - vals[key]) <= 1e-4 * max(1.0, abs(vals[key]))
    loss = h.train_loss(ten["fut"].data_ptr())
    v = vals["counted"]
    want = float((vals["reg"] * v).sum() / max(v.sum(), 1))
    print("%s: slot 3 %.9g, float64 %.9g" % (tag, loss["reg"], want))
    assert abs(loss["reg"] - want) <= 2e-5 * max(1.0, abs(want))              # tests/test_gpu_recon_loss.py's bar for slot 0
    h.close()


def test_training_gradients_with_split_operands():
    """dims.bf16 = 2 on the MEAN case with both refined penalties: tests/test_gpu_split.py's bar for this configuration."""
    h, ten, w, d, vals, ref, base = _refined_step("mean32", bf16=2)
    _check_done_gradients(h, w, ref, tol=2e-4)
    h.close()


# ---- 3. what the terms may not touch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["scene_softmin", "all_four", "iters2"])
def test_terms_reach_the_ioc_module_and_the_x_encoder_only(tag):
    h, ten, w, d, vals, ref, base = _refined_step(tag)
    now = _grads(h, w)
    moved = []
    for k in now:
        if (k.startswith("ioc/") and not k.startswith("ioc/score/")) or k.startswith("enc_x/"):
            if not np.array_equal(_bits(now[k]), _bits(base[0][k])):
                moved.append(k)
            continue
        np.testing.assert_array_equal(_bits(now[k]), _bits(base[0][k]), err_msg=k)       # the decoder's side, enc_y, the score head: bit for bit
    assert "ioc/reg/w" in moved and "ioc/gates/kernel" in moved and "enc_x/gates/kernel" in moved, moved
    loss = h.train_loss(ten["fut"].data_ptr())
    for key in ("recon", "kld", "ce", "n_present"):
        assert loss[key] == base[1][key], key
    if not (vals["spec"].recon and vals["spec"].mode != MEAN):
        assert loss["reg"] == base[1]["reg"]                                    # the penalties are not in slot 3
    h.close()


# ---- 4. the reported terms ----------------------------------------------------------------------------------------------------------------------
def _sum_loss_f32(val, lmask):
    """k_sum_loss (csrc/train.hip) on one slot: 256 strided sums in increasing a, met in increasing lane, over max(the counted agents, 1)."""
    red = np.zeros(256, np.float32)
    for a in range(val.size):
        red[a % 256] = np.float32(red[a % 256] + np.float32(val[a]))
    t = np.float32(0.0)
    for i in range(256):
        t = np.float32(t + red[i])
    return np.float32(t / np.float32(max(int(lmask.sum()), 1)))


@pytest.mark.parametrize("tag", ["scene_softmin", "min_agent", "all_four", "iters2"])
def test_reported_terms_are_the_stand_alone_ops_on_the_steps_own_y(tag):
    import torch
    h, ten, w, d, vals, ref, base = _refined_step(tag)
    spec = vals["spec"]
    got = {k: v.clone() for k, v in _r_tensors(h, d, spec).items()}
    reg = h.train_loss(ten["fut"].data_ptr())["reg"]
    Y, fut = _y(h, d).clone(), ten["fut"]
    A, K, n = d.A, d.K, d.n_scenes
    if spec.rcol:
        col, touch, term = torch.zeros(A * K, device="cuda"), torch.zeros(n * K, device="cuda", dtype=torch.int32), torch.zeros(1, device="cuda")
        h.collision_loss(fut.data_ptr(), Y.data_ptr(), spec.radius, 1.0 / d.sx, 1.0 / d.sy, col.data_ptr(), touch.data_ptr(), 0, term.data_ptr())
        torch.cuda.synchronize()
        assert int(touch.sum()) > 0 and float(term[0]) > 0
        assert torch.equal(got["rcol_touch"], touch)
        assert torch.equal(got["rcol_val"].view(torch.int32), col.view(torch.int32)) and torch.equal(got["rcol_term"].view(torch.int32), term.view(torch.int32))
    if spec.roff:
        off, count, term = torch.zeros(A * K, device="cuda"), torch.zeros(n * K, device="cuda", dtype=torch.int32), torch.zeros(1, device="cuda")
        h.offroad_loss(fut.data_ptr(), Y.data_ptr(), spec.scale, off.data_ptr(), count.data_ptr(), 0, term.data_ptr())
        torch.cuda.synchronize()
        assert int(count.sum()) > 0 and float(term[0]) > 0
        assert torch.equal(got["roff_count"], count)
        assert torch.equal(got["roff_val"].view(torch.int32), off.view(torch.int32)) and torch.equal(got["roff_term"].view(torch.int32), term.view(torch.int32))
    if spec.recon and spec.mode != MEAN:
        e, wt = torch.zeros(A * K, device="cuda"), torch.zeros(A * K, device="cuda")
        win, val = torch.zeros(A, device="cuda", dtype=torch.int32), torch.zeros(A, device="cuda")
        if spec.scope == SCENE:
            h.recon_weights_scene(fut.data_ptr(), Y.data_ptr(), spec.mode, spec.tau, e.data_ptr(), 0, 0, wt.data_ptr(), win.data_ptr(), val.data_ptr())
        else:
            h.recon_weights(fut.data_ptr(), Y.data_ptr(), spec.mode, spec.tau, e.data_ptr(), wt.data_ptr(), win.data_ptr(), val.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(got["rrecon_win"], win)
        for name, t in (("rrecon_e", e), ("rrecon_w", wt), ("rrecon_val", val)):
            assert torch.equal(got[name].view(torch.int32), t.view(torch.int32)), name
        lmask = h.device_tensor("lmask", "|u1").cpu().numpy()[:A]
        term = val.cpu().numpy()
        if spec.scope == SCENE:
            term = np.where(lmask != 0, term, np.float32(0.0))                 # every slot carries the window's term: the agents that do not count are zeroed
        assert np.float32(reg).view(np.uint32) == _sum_loss_f32(term, lmask).view(np.uint32)
    else:
        assert reg == base[1]["reg"]
    h.close()


# ---- 5. compaction ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,scope", [(MEAN, AGENT), (SOFTMIN, SCENE)])
def test_compacted_step_matches_the_padded_one(mode, scope):
    """DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC on tests/test_gpu_compact_rows.py's ragged case (8 windows; counts include 0, 1 and mno):
    the terms are taken on the full layout before the class gather.  That file's bars: terms 2e-6, gradients 3e-5 of the largest entry, counts
    equal."""
    import torch
    from tests.test_gpu_compact_rows import _spread, ragged_counts
    d = small_dims(n_scenes=8, K=3, T_obs=6, T_pred=7, n_grids=1)
    w = _spread(init_weights(d, 41))
    case = ragged_counts(d, seed=44, counts=[3, 9, 0, 14, 8, d.mno, 1, 20])
    masks = make_masks(2, 64, 64, 8)
    cell = cell_sizes(d, 64, 64)
    F = mask_field_f32(masks, *cell)
    fos = np.array([0, 1, 0, -1, 1, 0, 1, 0], np.int32)
    res = []
    for dd, min_rows in ((d, None), (d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC), 0)):
        h, ten = _training_handle(dd, w, case, min_rows)
        f_t = _attach(h, masks, cell, F, fos)
        if mode != MEAN:
            h.set_recon_loss(mode, TAU)
            h.set_recon_scope(scope)
        h.set_collision_loss(0.0, 400.0, 1.0 / d.sx, 1.0 / d.sy)
        h.set_offroad_loss(0.0, 120.0)
        h.set_refined_loss(1, 0.5, 0.5)
        _step(h, ten)
        torch.cuda.synchronize()
        n, K, A = d.n_scenes, d.K, d.A
        res.append((h.train_loss(ten["fut"].data_ptr()), _grads(h, w),
                    (h.device_tensor("rcol_touch", "<i4").cpu().numpy()[: n * K].copy(), h.device_tensor("roff_count", "<i4").cpu().numpy()[: n * K].copy()),
                    (h.device_tensor("rcol_val").cpu().numpy()[: A * K].copy(), h.device_tensor("roff_val").cpu().numpy()[: A * K].copy()),
                    (float(h.device_tensor("rcol_term")[0]), float(h.device_tensor("roff_term")[0])),
                    h.device_tensor("rrecon_win", "<i4").cpu().numpy()[:A].copy() if mode != MEAN else None))
        del f_t
        h.close()
    (la, ga, ta, ca, ma, wa), (lb, gb, tb, cb, mb, wb) = res
    assert ta[0].sum() > 0 and ta[1].sum() > 0 and ma[0] > 0 and ma[1] > 0
    for i in range(2):
        np.testing.assert_array_equal(ta[i], tb[i])
        assert np.abs(ca[i] - cb[i]).max() <= 2e-6 * max(1.0, np.abs(ca[i]).max()) and abs(ma[i] - mb[i]) <= 2e-6 * max(1.0, abs(ma[i]))
    if wa is not None:
        np.testing.assert_array_equal(wa, wb)
    for key in ("recon", "kld", "ce", "reg", "loss"):
        assert abs(la[key] - lb[key]) <= 2e-6 * max(1.0, abs(la[key])), (key, la[key], lb[key])
    assert la["n_present"] == lb["n_present"] > 0
    worst = ("", 0.0)
    for k in ga:
        if k == "ioc/score/b":
            continue
        ref = np.abs(ga[k]).max()
        err = float(np.abs(ga[k] - gb[k]).max() / (ref + 1e-12)) if ref > 1e-9 else float(np.abs(gb[k]).max())
        if err > worst[1]:
            worst = (k, err)
        assert np.isfinite(gb[k]).all()
    print("mode %d, slot classes vs padded step with the refined terms: worst relative gradient difference %.2e (%s)" % (mode, worst[1], worst[0]))
    assert worst[1] < 3e-5, worst


# ---- 6. capture ---------------------------------------------------------------------------------------------------------------------------------
def test_step_with_every_refined_term_replays_from_a_hipgraph():
    import torch
    tag = "scene_softmin"
    shape, seed, n_absent, kw, _ = CASES[tag]
    d = _case_dims(tag)
    w = _weights(d)
    vals, _ = _reference(tag)
    spec = vals["spec"]
    h, ten = _training_handle(d, w, make_case(d, seed=seed, n_absent=n_absent))
    _configure(h, d, ten, spec)
    side = torch.cuda.Stream()
    sp = side.cuda_stream

    def step(stream):
        _step(h, ten, stream)
        h.clip_grads(1e-3, stream=stream)

    torch.cuda.synchronize()
    step(sp)                                             # warm-up outside capture: lazy allocations and function attributes
    side.synchronize()
    g_ref, Y_ref = h.grad_tensor().clone(), ten["Y"].clone()
    r_ref = {k: v.clone() for k, v in _r_tensors(h, d, spec).items()}
    assert len(r_ref) == 12 and int(r_ref["rcol_touch"].sum()) > 0 and int(r_ref["roff_count"].sum()) > 0
    step(sp)                                             # a second eager run: the same bits
    side.synchronize()
    assert torch.equal(h.grad_tensor(), g_ref) and torch.equal(ten["Y"], Y_ref)
    h.graph_begin(sp)
    step(sp)
    gid = h.graph_end(sp)
    for _ in range(3):
        h.grad_tensor().zero_(); ten["Y"].zero_()
        for v in _r_tensors(h, d, spec).values():
            v.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        assert torch.equal(ten["Y"], Y_ref) and torch.equal(h.grad_tensor(), g_ref)
        for k, v in _r_tensors(h, d, spec).items():
            assert torch.equal(v.view(torch.int32), r_ref[k].view(torch.int32)), k
    assert float(g_ref.abs().max()) > 0
    h.close()


# ---- 7. it moves what it should -----------------------------------------------------------------------------------------------------------------
STEPS_WEIGHT = 0.5


def _forty_steps(kind, side, spec):
    """(start, end) = (L, count) of the stand-alone op on the step's own Y before the first and after the 40th Adam step: the steps of
    tests/test_gpu_train.py::test_loss_decreases_on_a_fixed_batch, with the term of `kind` at STEPS_WEIGHT on the refined side or on Y0."""
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    h, ten = _training_handle(d, w, make_case(d, seed=42, n_absent=4))
    if kind == "col":
        h.set_collision_loss(STEPS_WEIGHT if side == "y0" else 0.0, spec.radius, 1.0 / d.sx, 1.0 / d.sy)
    else:
        ten["field"] = _attach(h, spec.masks, cell_sizes(d, spec.Mh, spec.Mw), mask_field_f32(spec.masks, *cell_sizes(d, spec.Mh, spec.Mw)),
                               np.arange(d.n_scenes, dtype=np.int32))
        h.set_offroad_loss(STEPS_WEIGHT if side == "y0" else 0.0, spec.scale)
    if side == "refined":
        h.set_refined_loss(0, STEPS_WEIGHT if kind == "col" else 0.0, STEPS_WEIGHT if kind == "off" else 0.0)
    term, count = torch.zeros(1, device="cuda"), torch.zeros((d.n_scenes, d.K), device="cuda", dtype=torch.int32)
    trace = []
    for it in range(41):
        _step(h, ten)
        if it in (0, 40):
            if kind == "col":
                h.collision_loss(ten["fut"].data_ptr(), _y(h, d).data_ptr(), spec.radius, 1.0 / d.sx, 1.0 / d.sy, 0, count.data_ptr(), 0, term.data_ptr())
            else:
                h.offroad_loss(ten["fut"].data_ptr(), _y(h, d).data_ptr(), spec.scale, 0, count.data_ptr(), 0, term.data_ptr())
            torch.cuda.synchronize()
            trace.append((float(term[0]), int(count.sum())))
        if it == 40:
            break
        h.clip_grads(10.0)
        h.adam_step(0.002)
    h.close()
    return trace


@pytest.mark.parametrize("kind", ["col", "off"])
def test_the_refined_term_lowers_the_penalty_of_the_refined_trajectories(kind):
    vals, _ = _reference("mean32")
    run = {side: _forty_steps(kind, side, vals["spec"]) for side in ("refined", "y0")}
    print("L_%s(Y), count at weight %g: refined term %s, Y0 term alone %s" % (kind, STEPS_WEIGHT, run["refined"], run["y0"]))
    assert run["refined"][0] == run["y0"][0] and run["refined"][0][0] > 0      # the same first forward
    assert run["refined"][1][0] < run["refined"][0][0]                          # the term went down
    assert run["refined"][1][0] < run["y0"][1][0]                               # and ends below the run that penalises Y0 alone


# ---- 8. refusals and the host surface -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_and_its_settings_as_they_were():
    import torch
    from desire_amd import _lib
    tag = "mean8"
    shape, seed, n_absent, kw, _ = CASES[tag]
    d = _case_dims(tag)
    w = _weights(d)
    vals, _ = _reference(tag)
    spec = vals["spec"]
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    # a fresh handle: nothing set yet
    h, ten = _training_handle(d, w, make_case(d, seed=seed, n_absent=n_absent))
    assert lib.desire_set_refined_loss(None, 0, 0.0, 0.0) == ERR_ARG and lib.desire_last_error()
    for recon in (-1, 2, 7):
        assert lib.desire_set_refined_loss(h._h, recon, 0.0, 0.0) == ERR_ARG and b"recon" in lib.desire_last_error()
    for bad in (-0.5, nan, inf, -inf):
        assert lib.desire_set_refined_loss(h._h, 0, bad, 0.0) == ERR_ARG and b"collision_weight" in lib.desire_last_error()
        assert lib.desire_set_refined_loss(h._h, 0, 0.0, bad) == ERR_ARG and b"offroad_weight" in lib.desire_last_error()
    assert lib.desire_set_refined_loss(h._h, 2, -1.0, nan) == ERR_ARG and b"recon" in lib.desire_last_error()          # in the stated order
    assert lib.desire_set_refined_loss(h._h, 0, 0.5, 0.0) == ERR_STATE and b"radius" in lib.desire_last_error()        # no radius yet
    assert lib.desire_set_refined_loss(h._h, 0, 0.0, 0.5) == ERR_STATE and b"field" in lib.desire_last_error()         # no field yet
    h.set_collision_loss(0.0, 0.0, 1.0, 1.0)                                    # radius 0 is a radius at which nothing touches, not one to divide by
    assert lib.desire_set_refined_loss(h._h, 0, 0.5, 0.0) == ERR_STATE and b"radius" in lib.desire_last_error()
    ten["field"] = _attach(h, spec.masks, cell_sizes(d, spec.Mh, spec.Mw), mask_field_f32(spec.masks, *cell_sizes(d, spec.Mh, spec.Mw)),
                           np.arange(d.n_scenes, dtype=np.int32))
    assert lib.desire_set_refined_loss(h._h, 0, 0.0, 0.5) == ERR_STATE and b"scale" in lib.desire_last_error()         # a field, no scale
    h.set_offroad_loss(0.0, nan)
    assert lib.desire_set_refined_loss(h._h, 0, 0.0, 0.5) == ERR_STATE and b"scale" in lib.desire_last_error()
    assert lib.desire_set_refined_loss(h._h, 0, 0.5, 0.5) == ERR_STATE and b"radius" in lib.desire_last_error()        # the collision side is asked first
    for name in ("rcol_term", "roff_term", "rrecon_w"):
        with pytest.raises(Exception):
            h.device_tensor(name)                                               # a refused call allocates nothing
    with pytest.raises(_lib.DesireError):
        h.set_refined_loss(0, 0.5, 0.0)
    from tests.helpers import small_dims as sd
    hr = _lib.Handle(sd(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    assert lib.desire_set_refined_loss(hr._h, 0, 0.0, 0.0) == ERR_STATE and b"ref_compat" in lib.desire_last_error()
    assert lib.desire_set_refined_loss(hr._h, 0, -1.0, 0.0) == ERR_ARG                                                 # the argument checks come first
    hr.close()
    # a configured handle: every refusal leaves the settings, the step and the r* tensors as they were
    _configure(h, d, ten, spec)
    _step(h, ten)
    torch.cuda.synchronize()
    g_ref, l_ref = h.grad_tensor().clone(), h.train_loss(ten["fut"].data_ptr())
    fill = {k: v.fill_(-7) for k, v in _r_tensors(h, d, spec).items()}
    torch.cuda.synchronize()
    assert lib.desire_set_refined_loss(h._h, 2, 0.0, 0.0) == ERR_ARG
    assert lib.desire_set_refined_loss(h._h, 1, nan, 0.0) == ERR_ARG
    assert lib.desire_set_refined_loss(h._h, 1, 0.25, -1.0) == ERR_ARG
    h.set_offroad_loss(0.0, 0.0)                                                # the scale is gone: the refined off-road term cannot be set again ...
    assert lib.desire_set_refined_loss(h._h, 1, 0.25, 0.125) == ERR_STATE and b"scale" in lib.desire_last_error()
    assert lib.desire_backward(h._h, ten["past"].data_ptr(), ten["fut"].data_ptr(), ten["eps"].data_ptr(), None) == ERR_STATE      # ... nor run
    h.set_offroad_loss(0.0, spec.scale)
    torch.cuda.synchronize()
    for k, v in fill.items():
        assert bool((v == -7).all()), k                                         # nothing was launched or written
    _step(h, ten)
    torch.cuda.synchronize()
    assert torch.equal(h.grad_tensor(), g_ref) and h.train_loss(ten["fut"].data_ptr()) == l_ref      # weights 0.25 / 0.125 and recon = 1 were not taken
    assert float(h.device_tensor("rcol_term")[0]) > 0 and float(h.device_tensor("roff_term")[0]) > 0
    h.set_refined_loss(0, 0.0, 0.0)                                             # and off again: the step without the terms
    _step(h, ten)
    torch.cuda.synchronize()
    assert not torch.equal(h.grad_tensor(), g_ref) and float(h.device_tensor("rcol_term")[0]) > 0      # (the last step's term stays where it was)
    h.close()


def _model_batch():
    rng = np.random.default_rng(0)
    ids = np.arange(1, 9, dtype=np.float32)[None, :, None]
    x = [np.concatenate([ids.repeat(6, 0), rng.uniform(200, 1800, (6, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    y = [np.concatenate([ids.repeat(7, 0), rng.uniform(200, 1800, (7, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    return x, y


def test_model_reaches_the_handle():
    from types import SimpleNamespace
    from desire_amd.model import DESIREModel
    base = dict(seq_length=6, pred_length=7, d_dim=64, rnn_size=512, latent_size=64, max_num_obj=8, learning_rate=0.0005, grad_clip=10.0,
                neighborhood_size=256, grid_size=4, num_samples=3, batch_size=2)
    x, y = _model_batch()
    m = DESIREModel(SimpleNamespace(**base), seed=3)
    terms = m.train_step(x, y, seed=1)
    assert "rcol" not in terms and "roff" not in terms
    with pytest.raises(Exception):
        m._trained.device_tensor("rcol_term")                                   # the default never allocates or runs the new code
    walls = np.zeros((2, 8, 8), np.uint8)
    walls[0, 0, 0] = 1                                                          # one road cell in a corner: everybody stands off the road
    walls[1] = 1                                                                # all road
    m = DESIREModel(SimpleNamespace(refine_collision_weight=0.5, collision_radius=3000.0, refine_offroad_weight=0.25, offroad_scale=200.0,
                                    refine_recon=True, recon_loss="min", **base), seed=3)
    m.set_scene_masks(walls, [0, 0])
    terms = m.train_step(x, y, seed=1)
    h = m._trained
    assert np.isfinite(terms["loss"]) and terms["rcol"] > 0 and terms["roff"] > 0 and "col" not in terms and "off" not in terms
    assert terms["rcol"] == float(h.device_tensor("rcol_term")[0]) and terms["roff"] == float(h.device_tensor("roff_term")[0])
    assert int(h.device_tensor("rrecon_win", "<i4")[: h.dims.A].max()) > 0      # the refined weights ran: some agent's winner is not sample 0
    with pytest.raises(Exception):
        h.device_tensor("col_term")                                             # the Y0 terms stay off: radius and scale went in at weight 0
    assert m.train_step(x, y, seed=1, mask_of_scene=[1, 1])["roff"] == 0.0     # the batch's own mapping: all road
    pend = m.train_step(x, y, seed=1, sync=False, mask_of_scene=[0, 0])
    got = pend.get()
    assert got["rcol"] > 0 and got["roff"] > 0 and "col" not in got
    both = DESIREModel(SimpleNamespace(collision_weight=0.5, collision_radius=3000.0, refine_collision_weight=0.5, offroad_weight=0.5,
                                       refine_offroad_weight=0.25, offroad_scale=200.0, **base), seed=3)
    both.set_scene_masks(walls, [0, 0])
    t2 = both.train_step(x, y, seed=1, sync=False).get()
    assert t2["col"] > 0 and t2["off"] > 0 and t2["rcol"] > 0 and t2["roff"] > 0
    for bad, name in ((dict(refine_collision_weight=0.5), "refine_collision_weight"), (dict(refine_offroad_weight=0.5), "refine_offroad_weight"),
                      (dict(refine_offroad_weight=-1.0, offroad_scale=5.0), "refine_offroad_weight")):
        mb = DESIREModel(SimpleNamespace(**bad, **base), seed=3)
        mb.set_scene_masks(walls, [0, 0])
        with pytest.raises(ValueError, match=name):
            mb.train_step(x, y, seed=1)
    with pytest.raises(ValueError, match="set_scene_masks"):
        DESIREModel(SimpleNamespace(refine_offroad_weight=0.5, offroad_scale=5.0, **base), seed=3).train_step(x, y, seed=1)


def test_train_runs_an_epoch_with_the_refined_columns(tmp_path):
    import re
    from desire_amd import train as T
    common = ["--batch_size", "2", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--d_dim", "64", "--latent_size", "64",
              "--num_samples", "5", "--neighborhood_size", "256", "--num_epochs", "1", "--prefetch", "0", "--save_dir", str(tmp_path),
              "--data_dir", str(tmp_path)]
    t = np.arange(10, dtype=np.float32)
    win = np.zeros((2, 10, 8, 3), np.float32)                         # two windows of four objects walking straight lines
    for n in range(2):
        for i in range(4):
            win[n, :, i, 0] = i + 1
            win[n, :, i, 1] = 200 + 150 * i + (3 + n) * t
            win[n, :, i, 2] = 150 + 100 * i + 2 * t

    class Loader:                                                     # the reference loader's surface, and the two videos the windows come from
        seq_length, num_batches, leave_dataset = 10, 2, 2

        def _csv_paths(self):
            return [str(tmp_path / "a" / "v0" / "x.csv"), str(tmp_path / "a" / "v1" / "x.csv")]

        def reset_batch_pointer(self):
            pass

        def next_batch(self):
            return list(win), None, [0, 1]

    road = np.ones((8, 8), np.uint8)
    wall = np.zeros((8, 8), np.uint8)
    wall[7, 7] = 1
    path = str(tmp_path / "masks.npz")
    np.savez(path, **{"a/v0": wall, "a/v1": road})
    lines = []
    a = T.build_parser().parse_args(common + ["--refine_recon", "--recon_loss", "softmin", "--recon_tau", "0.05", "--refine_collision_weight", "0.5",
                                              "--collision_radius", "2500", "--refine_offroad_weight", "0.25", "--offroad_scale", "150",
                                              "--scene_masks", path])
    losses = T.train(a, data_loader=Loader(), log=lines.append)
    assert len(losses) == 2 and np.isfinite(losses).all()
    steps = [ln for ln in lines if "train_loss" in ln]
    assert len(steps) == 2 and all(re.search(r", recon\[softmin tau=0\.05\] = [0-9.]+, rcol\[w=0\.5\] [0-9.]+, roff\[w=0\.25\] [0-9.]+$", ln) for ln in steps), steps
    assert float(steps[0].rsplit(" ", 1)[1]) > 0 and float(steps[0].rsplit(", roff", 1)[0].rsplit(" ", 1)[1]) > 0
    plain = []
    T.train(T.build_parser().parse_args(common), data_loader=Loader(), log=plain.append)
    assert all(re.fullmatch(r"\d+/2 \(epoch 0\), train_loss = [0-9.]+, time/batch = [0-9.]+", ln) for ln in plain if "train_loss" in ln), plain
    with pytest.raises(ValueError, match="--refine_collision_weight"):
        T.train(T.build_parser().parse_args(common + ["--refine_collision_weight", "0.5"]), data_loader=Loader(), log=plain.append)
    with pytest.raises(ValueError, match="--refine_offroad_weight"):
        T.train(T.build_parser().parse_args(common + ["--refine_offroad_weight", "0.25", "--offroad_scale", "150"]), data_loader=Loader(), log=plain.append)
