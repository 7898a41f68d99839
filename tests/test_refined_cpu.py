"""CPU-side checks of the terms on the refined trajectories (desire_set_refined_loss): the ABI symbol and its binding, the
float64 reference (tests/refined_reference.py) against the oracle's own loss with everything off and against central differences with
everything on, the model's hook on a recording handle, and train.py's flags, argument checks and log columns."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from desire_amd.spec import init_weights
from tests.helpers import make_case, small_dims, to_oracle_layout
from tests.refined_reference import AGENT, MIN, SCENE, SOFTMIN, Spec, pair_distances, refined_forward, refined_loss_and_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, SEED, N_ABSENT = (2, 8, 3, 7), 47, 2          # tests/test_gpu_refined_loss.py's small case
TAU = 0.01


def _case(seed=SEED, **kw):
    from tests.stage_reference import spread_weights
    n, m, K, T = SHAPE
    d = small_dims(n_scenes=n, mno=m, K=K, T_obs=6, T_pred=T, n_grids=1, **kw)
    past, fut, eps, grids, gos = make_case(d, seed=seed, n_absent=N_ABSENT)
    return d, spread_weights(init_weights(d, 41)), (to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos)


def test_abi_symbol_and_binding():
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "desire_hip.h")).read()
    name = "desire_set_refined_loss"
    assert re.search(r"\bint %s\s*\(\s*desire_handle\s*\*\s*\w*,\s*int32_t \w+,\s*float \w+,\s*float \w+\)" % name, hdr)
    assert name in _lib.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == 4
    assert callable(_lib.Handle.set_refined_loss)
    assert lib.desire_set_refined_loss(None, 0, 0.0, 0.0) == -1 and lib.desire_last_error()      # needs no device: a NULL handle is refused with a text


@pytest.mark.parametrize("iters", [1, 2])
def test_everything_off_is_the_oracles_own_loss(iters):
    from oracle import desire_torch as OT
    d, w, case = _case(iters=iters)
    vals, grads = refined_loss_and_grads(*case, w, d, Spec())
    ref_vals, ref_grads = OT.loss_and_grads(*case, w, d)
    assert vals["loss"] == float(ref_vals["loss"])
    assert sorted(grads) == sorted(ref_grads)
    for k in ref_grads:
        np.testing.assert_array_equal(grads[k], ref_grads[k], err_msg=k)
    np.testing.assert_array_equal(vals["reg"], ref_vals["reg"])
    # recon = True in mode MEAN is the same loss; so is recon = False in another mode on the regression term
    v2, g2 = refined_loss_and_grads(*case, w, d, Spec(recon=True))
    assert v2["loss"] == vals["loss"]
    for k in ("ioc/reg/w", "enc_x/gates/kernel", "head/w"):
        np.testing.assert_array_equal(g2[k], grads[k], err_msg=k)
    v3, g3 = refined_loss_and_grads(*case, w, d, Spec(mode=MIN))
    np.testing.assert_array_equal(v3["reg"], vals["reg"])
    np.testing.assert_array_equal(g3["ioc/reg/w"], grads["ioc/reg/w"])            # Y is built on the detached Y0: the recon mode on Y0 does not reach it
    assert np.abs(g3["head/w"] - grads["head/w"]).max() > 0


def test_a_term_on_the_refined_trajectories_reaches_the_ioc_module_and_the_x_encoder_only():
    d, w, case = _case()
    base, g0 = refined_loss_and_grads(*case, w, d, Spec())
    vals, g1 = refined_loss_and_grads(*case, w, d, Spec(mode=SOFTMIN, tau=TAU, scope=SCENE, recon=True, rcol=True, roff=True))
    assert vals["touching"] > 0 and vals["positive"] > 0.25 and vals["share_rcol"] >= 0.1 and vals["share_roff"] >= 0.1
    base_soft, gs = refined_loss_and_grads(*case, w, d, Spec(mode=SOFTMIN, tau=TAU, scope=SCENE))
    moved = [k for k in g1 if np.abs(g1[k] - gs[k]).max() > 0]
    assert moved and all(k.startswith("ioc/") or k.startswith("enc_x/") for k in moved), moved
    assert "ioc/reg/w" in moved and "enc_x/gates/kernel" in moved
    assert not [k for k in moved if k.startswith("ioc/score/")]                   # the score head does not see Y
    for k in ("kld", "ce"):
        np.testing.assert_array_equal(vals[k], base[k])


# (spec, seed): the seeds are chosen from the float64 reference alone so that the counted positions -- of Y, and of Y0 where its terms are on -- keep
# 1e-4 cells from a cell line or centre line and 1e-4 of the radius from the hinge's kink
SPECS = {"scene_min": (Spec(mode=MIN, scope=SCENE, recon=True, rcol=True, roff=True), SEED),
         "agent_softmin_all_four": (Spec(mode=SOFTMIN, tau=TAU, scope=AGENT, recon=True, rcol=True, roff=True, col=True, off=True), 46)}


@pytest.mark.parametrize("tag", list(SPECS))
def test_the_gradient_is_the_gradient(tag):
    """Central differences of the rebuilt loss on entries of ioc/reg/w, ioc/reg/b and enc_x/*, the stop-gradient quantities pinned (fixed=) and
    every choice of the reference pinned by the resolved Spec.  The step moves a position by far less than its distance to a kink: the cells, the
    touching pairs and the winner of both displaced points are asserted to be the base point's.  Bar: the truncation h^2 f''' / 6 and the rounding
    2^-52 |loss| / h at h = 1e-6 are below 1e-9 for a loss of order 1; 1e-5 of the name's largest entry leaves a factor of a hundred."""
    import torch
    from oracle import desire_torch as OT
    d, w, case = _case(seed=SPECS[tag][1])
    vals, grads = refined_loss_and_grads(*case, w, d, SPECS[tag][0])
    spec = vals["spec"]
    assert vals["hinge_gap"] >= 1e-4 and vals["margin"] >= 1e-4 and vals["touching"] > 0
    if spec.mode == MIN:
        assert vals["win_gap"] >= 1e-3
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    with torch.no_grad():
        res0 = refined_forward(*case, OT.leaf_weights(w), d, spec)
    fixed = {"Yd": res0["out"]["Yd"].numpy(), "dmax": res0["out"]["dmax"].numpy()}
    assert abs(float(res0["loss"]) - vals["loss"]) <= 1e-12 * abs(vals["loss"])
    counted = (res0["M"]["cc"].reshape(n, m, T) > 0).numpy()

    def kinks(res):
        cells, touch = [], []
        for Yt in (res["Y"], res["Y0"]):
            Yn = Yt.numpy()
            cells.append(np.floor(np.stack([Yn[..., 0] * spec.Mw - 0.5, Yn[..., 1] * spec.Mh - 0.5], -1))[np.broadcast_to(counted[:, None], (n, K, m, T))])
            dist, pair = pair_distances(Yt, res["M"], d)
            touch.append(((dist < spec.radius) & (pair > 0)).numpy())
        win = res["E1"].argmin(1).numpy() if res["E1"] is not None else None
        return np.stack(cells), np.stack(touch), win

    k0 = kinks(res0)
    h, worst = 1e-6, 0.0
    rng = np.random.default_rng(5)
    for name in ("ioc/reg/w", "ioc/reg/b", "enc_x/gates/kernel", "enc_x/candidate/kernel", "enc_x/candidate/bias"):
        g = grads[name]
        assert np.abs(g).max() > 0, name
        idx = [int(np.abs(g).argmax())] + [int(i) for i in rng.integers(0, g.size, 2)]
        for i in idx:
            val = []
            for sgn in (1.0, -1.0):
                wp = {k: np.asarray(v, np.float64).copy() for k, v in w.items()}      # (the weights are fp32 arrays: the step must not be rounded to them)
                wp[name].reshape(-1)[i] += sgn * h
                with torch.no_grad():
                    res = refined_forward(*case, OT.leaf_weights(wp), d, spec, fixed=fixed)
                kp = kinks(res)
                assert np.array_equal(kp[0], k0[0]) and np.array_equal(kp[1], k0[1]) and (k0[2] is None or np.array_equal(kp[2], k0[2]))
                val.append(float(res["loss"]))
            fd = (val[0] - val[1]) / (2 * h)
            err = abs(fd - g.reshape(-1)[i]) / np.abs(g).max()
            worst = max(worst, err)
            assert err <= 1e-5, (name, i, fd, g.reshape(-1)[i])
    print("%s: worst |central difference - autograd| = %.2e of the name's largest entry (bar 1e-5)" % (tag, worst))


class _Recorder:
    """A handle that records what the model's hook sets."""
    dims = SimpleNamespace(sx=1.0 / 2000.0, sy=1.0 / 1000.0)

    def __init__(self):
        self.calls = []

    def set_collision_loss(self, *a):
        self.calls.append(("col",) + a)

    def set_offroad_loss(self, *a):
        self.calls.append(("off",) + a)

    def set_refined_loss(self, *a):
        self.calls.append(("ref",) + a)


def _hook(h, masks=None, **args):
    from desire_amd.model import DESIREModel
    DESIREModel._configure_refined_loss(SimpleNamespace(args=SimpleNamespace(**args), _masks=masks), h)
    return h.calls


def test_model_hook_sets_what_the_y0_terms_left_unset_and_refuses_by_argument_name():
    assert _hook(_Recorder()) == []                                               # nothing asked: the handle is not touched
    assert _hook(_Recorder(), refine_recon=True) == [("ref", 1, 0.0, 0.0)]
    calls = _hook(_Recorder(), refine_collision_weight=0.5, collision_radius=300.0)
    assert calls == [("col", 0.0, 300.0, 2000.0, 1000.0), ("ref", 0, 0.5, 0.0)]  # the radius goes in at weight 0, in pixels
    calls = _hook(_Recorder(), refine_collision_weight=0.5, collision_radius=300.0, collision_loss_radius=200.0)
    assert calls[0] == ("col", 0.0, 200.0, 2000.0, 1000.0)
    h = _Recorder()
    h._col_on = True                                                              # the Y0 term is on: its radius stands
    assert _hook(h, refine_collision_weight=0.5, collision_weight=0.25, collision_radius=300.0) == [("ref", 0, 0.5, 0.0)]
    calls = _hook(_Recorder(), masks=object(), refine_offroad_weight=0.25, offroad_scale=90.0, refine_recon=True)
    assert calls == [("off", 0.0, 90.0), ("ref", 1, 0.0, 0.25)]
    h = _Recorder()
    h._off_on = True
    assert _hook(h, masks=object(), refine_offroad_weight=0.25, offroad_scale=90.0) == [("ref", 0, 0.0, 0.25)]
    assert h._roff_on and not h._rcol_on
    for bad, name in ((dict(refine_collision_weight=-1.0, collision_radius=5.0), "refine_collision_weight"),
                      (dict(refine_collision_weight=float("nan"), collision_radius=5.0), "refine_collision_weight"),
                      (dict(refine_collision_weight=0.5), "refine_collision_weight"),
                      (dict(refine_collision_weight=0.5, collision_radius=0.0), "refine_collision_weight"),
                      (dict(refine_offroad_weight=float("inf"), offroad_scale=5.0), "refine_offroad_weight"),
                      (dict(refine_offroad_weight=0.5), "refine_offroad_weight"),
                      (dict(refine_offroad_weight=0.5, offroad_scale=-2.0), "refine_offroad_weight"),
                      (dict(refine_recon="yes"), "refine_recon"), (dict(refine_recon=2), "refine_recon")):
        h = _Recorder()
        with pytest.raises(ValueError, match="args." + name):
            _hook(h, masks=object(), **bad)
        assert h.calls == []                                                      # refused before anything reaches the handle
    with pytest.raises(ValueError, match="set_scene_masks"):
        _hook(_Recorder(), refine_offroad_weight=0.5, offroad_scale=5.0)


def test_train_flags_argument_checks_and_log_columns():
    from desire_amd import train as T
    p = T.build_parser()
    a = p.parse_args([])
    assert a.refine_recon is False and a.refine_collision_weight == 0.0 and a.refine_offroad_weight == 0.0
    T.check_recon_args(a)
    T.check_recon_args(p.parse_args(["--refine_recon"]))                          # with --recon_loss mean: accepted, changes nothing
    T.check_recon_args(p.parse_args(["--refine_recon", "--recon_loss", "min", "--recon_scope", "scene"]))
    T.check_recon_args(p.parse_args(["--refine_collision_weight", "0.5", "--collision_radius", "40"]))      # --collision_weight stays 0
    T.check_recon_args(p.parse_args(["--refine_collision_weight", "0.5", "--collision_loss_radius", "40"]))
    T.check_recon_args(p.parse_args(["--refine_offroad_weight", "0.5", "--offroad_scale", "50", "--scene_masks", "m.npz"]))
    for bad, flag in ((["--refine_collision_weight", "0.5"], "--refine_collision_weight"),
                      (["--refine_collision_weight", "0.5", "--collision_radius", "0"], "--refine_collision_weight"),
                      (["--refine_collision_weight", "-0.5", "--collision_radius", "40"], "--refine_collision_weight"),
                      (["--refine_collision_weight", "nan", "--collision_radius", "40"], "--refine_collision_weight"),
                      (["--refine_offroad_weight", "0.5", "--scene_masks", "m.npz"], "--refine_offroad_weight"),
                      (["--refine_offroad_weight", "0.5", "--offroad_scale", "inf", "--scene_masks", "m.npz"], "--refine_offroad_weight"),
                      (["--refine_offroad_weight", "0.5", "--offroad_scale", "50"], "--refine_offroad_weight"),
                      (["--refine_offroad_weight", "-1", "--offroad_scale", "50", "--scene_masks", "m.npz"], "--refine_offroad_weight"),
                      (["--refine_offroad_weight", "inf", "--offroad_scale", "50", "--scene_masks", "m.npz"], "--refine_offroad_weight")):
        with pytest.raises(ValueError, match=flag):
            T.check_recon_args(p.parse_args(bad))
    with pytest.raises(ValueError, match="--scene_masks"):
        T.check_recon_args(p.parse_args(["--refine_offroad_weight", "0.5", "--offroad_scale", "50"]))
    with pytest.raises(ValueError, match="--offroad_scale"):
        T.check_recon_args(p.parse_args(["--refine_offroad_weight", "0.5", "--scene_masks", "m.npz"]))
    terms = {"loss": 1.0, "recon": 0.5, "col": 0.25, "off": 0.125, "rcol": 0.0625, "roff": 0.03125}
    plain = "1/2 (epoch 0), train_loss = 1.000, time/batch = 0.100"
    assert T.step_line(p.parse_args([]), 1, 2, 0, terms, 0.1) == plain            # without the flags: the line as it was, byte for byte
    assert T.step_line(p.parse_args(["--refine_recon"]), 1, 2, 0, terms, 0.1) == plain
    a = p.parse_args(["--refine_collision_weight", "0.5", "--collision_radius", "40"])
    assert T.step_line(a, 1, 2, 0, terms, 0.1) == plain + ", rcol[w=0.5] 0.06250"
    a = p.parse_args(["--refine_offroad_weight", "0.25", "--offroad_scale", "50", "--scene_masks", "m.npz", "--refine_collision_weight", "2",
                      "--collision_radius", "40", "--collision_weight", "1"])
    assert T.step_line(a, 1, 2, 0, terms, 0.1) == plain + ", col[r=40 w=1] 0.25000, rcol[w=2] 0.06250, roff[w=0.25] 0.03125"
