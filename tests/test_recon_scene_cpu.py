"""CPU-side checks of the scene scope of the reconstruction loss: the numpy statements of its contract (tests/recon_scene_reference.py) against each
other and against the per-agent statements they are built on, the counting, ties and NaN rules, the identity that makes the reported loss the
mean over the counted agents, the margin the GPU hard-min gradient test relies on (through the float64 oracle), the ABI surface and train.py's
flags."""
import os
import re

import numpy as np
import pytest

from tests.helpers import make_case, small_dims, to_oracle_layout
from tests.recon_reference import make_recon_case, recon_f32, recon_f64
from tests.recon_scene_reference import MEAN, MIN, SCENE_GAP, SOFTMIN, make_scene_case, scene_f32, scene_f64, scene_loss_and_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 8, 3, 7), (3, 1, 1, 7), (1, 32, 20, 40), (2, 32, 70, 5)]
MODES = ((MEAN, 0.0), (MIN, 0.0), (SOFTMIN, 0.01), (SOFTMIN, 1.0))


def _dims(shape):
    n, m, K, T = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=6, T_pred=T, n_grids=1)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, s in enumerate(SHAPES):
        d = _dims(s)
        out[s] = (d,) + make_scene_case(d, seed=300 + i, empty_window=1 if s == (2, 8, 3, 7) else None, tie_window=0 if d.K > 1 else None)
    return out


def test_surface_is_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "desire_hip.h")).read()
    declared = set(re.findall(r"\b(desire_[a-z_]+)\s*\(", hdr))
    for name in ("desire_set_recon_scope", "desire_recon_weights_scene"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert (_lib.RECON_SCOPE_AGENT, _lib.RECON_SCOPE_SCENE) == (0, 1) and _lib.RECON_SCOPES == {"agent": 0, "scene": 1}
    for k, v in (("AGENT", 0), ("SCENE", 1)):
        assert re.search(r"#define DESIRE_RECON_SCOPE_%s %d\b" % (k, v), hdr)
    assert hasattr(_lib.Handle, "set_recon_scope") and hasattr(_lib.Handle, "recon_weights_scene")
    # argument checks that need no device: the handle comes first
    assert lib.desire_set_recon_scope(None, 1) == -1
    assert lib.desire_recon_weights_scene(None, None, None, 1, 0.0, None, None, None, None, None, None, None) == -1


@pytest.mark.parametrize("shape", SHAPES)
def test_f32_statement_against_f64(cases, shape):
    d, Y, fut, valid, tied = cases[shape]
    # e: T_pred additions of correctly rounded terms and a division; E: mno more additions and a division
    bound = (d.T_pred + d.mno + 5) * 2.0 ** -24
    for mode, tau in MODES:
        a, b = scene_f32(Y, fut, valid, d, mode, tau), scene_f64(Y, fut, valid, d, mode, tau)
        for key in ("e", "E", "w", "recon", "W", "R"):
            assert a[key].dtype == np.float32, key
        assert a["count"].dtype == np.int32 and a["winner"].dtype == np.int32
        assert (np.abs(a["E"] - b["E"]) <= bound * b["E"]).all()
        np.testing.assert_array_equal(a["count"], b["count"])
        np.testing.assert_array_equal(a["winner"], b["winner"])              # ties included: the lower k in either precision
        wtol = 4 * bound * (1.0 + (b["E"].max() / tau if mode == SOFTMIN else 0.0)) + 1e-7
        assert np.abs(a["w"] - b["w"]).max() <= wtol
        assert np.abs(a["recon"] - b["recon"]).max() <= 4 * bound * max(1.0, b["E"].max()) + 1e-7
        np.testing.assert_allclose(b["W"].sum(1), 1.0, rtol=0, atol=1e-12)
        # step 1 is the per-agent statement's
        np.testing.assert_array_equal(a["e"].view(np.uint32), recon_f32(Y, fut, valid, d, mode, tau)["e"].view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES)
def test_counts_broadcast_and_ties(cases, shape):
    d, Y, fut, valid, tied = cases[shape]
    n, m, K = d.n_scenes, d.mno, d.K
    r = scene_f64(Y, fut, valid, d, MIN)
    counted = (fut[..., 0] != 0).any(1).reshape(n * m) & (valid != 0)
    np.testing.assert_array_equal(r["lmask"], counted)
    np.testing.assert_array_equal(r["count"], counted.reshape(n, m).sum(1))
    # E is the plain mean of e over the counted agents of the window
    e = r["e"].reshape(n, m, K)
    want = np.where(r["count"][:, None] > 0, (e * counted.reshape(n, m, 1)).sum(1) / np.maximum(r["count"], 1)[:, None], 0.0)
    np.testing.assert_allclose(r["E"], want, rtol=1e-13, atol=0)
    # every slot of a window -- counted or not -- carries the window's weights, winner and term
    for key in ("w", "winner", "recon"):
        v = r[key].reshape((n, m) + r[key].shape[1:])
        assert (v == v[:, :1]).all(), key
    assert (r["w"].sum(1) == 1).all() and ((r["w"] == 1).sum(1) == 1).all()
    if K > 1:
        t = tied & (r["count"] > 0)
        assert t.any() and (r["gap"][t] == 0).all()
        Et = r["E"][t]
        assert (r["winner_w"][t] == np.argmax(Et == Et.min(1, keepdims=True), axis=1)).all()      # the tie goes to the lower k
        plain = ~tied & (r["count"] > 0)
        if plain.any():
            assert (r["gap"][plain] >= SCENE_GAP * r["E"].min(1)[plain]).all()


def test_a_window_with_no_counted_agent(cases):
    d, Y, fut, valid, tied = cases[(2, 8, 3, 7)]
    for stmt in (scene_f32, scene_f64):
        for mode, tau in MODES:
            r = stmt(Y, fut, valid, d, mode, tau)
            assert r["count"][1] == 0 and r["count"][0] > 0
            assert (r["E"][1] == 0).all() and r["winner_w"][1] == 0 and r["R"][1] == 0
            np.testing.assert_allclose(r["W"][1], [1, 0, 0] if mode == MIN else [1 / 3] * 3, rtol=0, atol=1e-7)
            assert (r["e"][d.mno:] == 0).all()


def test_all_nan_and_partly_nan_windows():
    d = _dims((1, 2, 4, 3))
    fut = np.ones((1, 3, 2, 3), np.float32)
    for stmt in (scene_f32, scene_f64):
        Y = np.zeros((4 * 2, 3, 2), np.float32)                              # row = k * mno + slot
        Y[:, :, 0] = np.repeat(np.array([3.0, 2.0, 1.0, 2.5], np.float32), 2)[:, None]
        Y[0, 1, 0] = np.nan                                                  # world 0: one agent's error is a NaN, so E[0] is
        r = stmt(Y, fut, np.ones(2, np.uint8), d, MIN)
        assert np.isnan(r["E"][0, 0]) and r["winner_w"][0] == 2
        Y[2 * 2 + 1, 0, 1] = np.nan                                          # the smallest becomes a NaN too: the next strict minimum wins
        assert stmt(Y, fut, np.ones(2, np.uint8), d, MIN)["winner_w"][0] == 1
        Y[:, 0, 0] = np.nan                                                  # every world a NaN: nobody replaces world 0
        r = stmt(Y, fut, np.ones(2, np.uint8), d, MIN)
        assert np.isnan(r["E"]).all() and r["winner_w"][0] == 0 and (r["W"][0] == [1, 0, 0, 0]).all() and np.isnan(r["R"][0])


@pytest.mark.parametrize("shape", SHAPES)
def test_reported_loss_is_the_mean_over_counted_agents(cases, shape):
    d, Y, fut, valid, tied = cases[shape]
    for mode, tau in MODES:
        r = scene_f64(Y, fut, valid, d, mode, tau)
        c = r["lmask"]
        lhs = (r["count"] * r["R"]).sum() / max(r["count"].sum(), 1)
        rhs = r["recon"][c].mean() if c.any() else 0.0
        assert abs(lhs - rhs) <= 1e-14 * max(1.0, abs(rhs))


def test_modes_are_ordered(cases):
    d, Y, fut, valid, tied = cases[(2, 32, 70, 5)]
    mean, mn = scene_f64(Y, fut, valid, d, MEAN), scene_f64(Y, fut, valid, d, MIN)
    for tau in (1e-3, 0.01, 1.0):
        sm = scene_f64(Y, fut, valid, d, SOFTMIN, tau)
        assert (mn["R"] <= sm["R"] + 1e-15).all() and (sm["R"] <= mean["R"] + 1e-15).all()
    # the mean over k of a mean over agents is the mean over both: the scope does not matter in MEAN
    a = recon_f64(Y, fut, valid, d, MEAN)
    c = a["lmask"]
    assert abs((mean["count"] * mean["R"]).sum() / mean["count"].sum() - a["recon"][c].mean()) < 1e-14
    # ... and it does in MIN: a window's best world is no better than every agent's own best sample
    b = recon_f64(Y, fut, valid, d, MIN)
    assert (mn["count"] * mn["R"]).sum() / mn["count"].sum() > b["recon"][c].mean()


@pytest.mark.parametrize("K", [1, 3])
def test_one_slot_windows_are_the_per_agent_statement(K):
    d = _dims((3, 1, K, 7))
    Y, fut, valid, _ = make_recon_case(d, seed=11)
    for mode, tau in MODES:
        for scene, agent in ((scene_f32, recon_f32), (scene_f64, recon_f64)):
            s, a = scene(Y, fut, valid, d, mode, tau), agent(Y, fut, valid, d, mode, tau)
            assert s["lmask"].all()                                          # (small cases have no absent agent: e / 1.f is e)
            for key in ("e", "w", "recon"):
                np.testing.assert_array_equal(s[key], a[key], err_msg=key)
            np.testing.assert_array_equal(s["winner"], a["winner"])
            np.testing.assert_array_equal(s["E"], a["e"])


def test_margin_of_the_scene_hard_min_gradient_case():
    """The case the GPU scene hard-min gradient test uses -- (2, 8, 3, 7), make_case seed 42 with 2 absent agents -- keeps each window's best
    and second-best float64 world error at least 1e-4 apart (5.6e-4 and 1.1e-3), and its two windows pick different worlds (2 and 0)."""
    from desire_amd.spec import init_weights
    from tests.stage_reference import spread_weights
    d = _dims((2, 8, 3, 7))
    w = spread_weights(init_weights(d, 41))
    past, fut, eps, grids, gos = make_case(d, seed=42, n_absent=2)
    vals, g = scene_loss_and_grads(to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos, w, d, MIN)
    print("scene hard-min case: counts %s, world gaps %s, winners %s" % (vals["count"], vals["gap"], vals["winner_w"]))
    assert (vals["count"] > 0).all() and vals["count"].sum() == 12
    assert vals["gap"].min() >= 1e-4, vals["gap"]
    assert abs(vals["gap"].min() - 5.63e-4) < 1e-6
    np.testing.assert_array_equal(vals["winner_w"], [2, 0])
    assert abs(vals["L_recon"] - (vals["count"] * vals["E"].min(1)).sum() / vals["count"].sum()) < 1e-15
    assert np.abs(g["head/w"]).max() > 0


def test_train_flags_parse_and_refuse():
    from types import SimpleNamespace
    from desire_amd.train import build_parser, check_recon_args, step_line
    p = build_parser()
    a = p.parse_args([])
    assert a.recon_scope == "agent" and a.report_joint is False and a.collision_radius is None
    check_recon_args(a)
    for argv in (["--recon_scope", "scene"], ["--recon_scope", "scene", "--recon_loss", "min"],
                 ["--recon_scope", "scene", "--recon_loss", "softmin", "--recon_tau", "0.01"]):
        check_recon_args(p.parse_args(argv))
    with pytest.raises(SystemExit):
        p.parse_args(["--recon_scope", "world"])
    with pytest.raises(ValueError):
        check_recon_args(SimpleNamespace(recon_loss="min", recon_tau=None, recon_scope="world"))
    with pytest.raises(ValueError):
        check_recon_args(p.parse_args(["--recon_scope", "scene", "--recon_loss", "softmin"]))
    terms = {"loss": 1.5, "recon": 0.25}
    assert step_line(p.parse_args(["--recon_scope", "scene"]), 3, 10, 0, terms, 0.1) == "3/10 (epoch 0), train_loss = 1.500, time/batch = 0.100"
    assert "recon[min] = 0.25000" in step_line(p.parse_args(["--recon_loss", "min"]), 3, 10, 0, terms, 0.1)
    assert "recon[scene min] = 0.25000" in step_line(p.parse_args(["--recon_loss", "min", "--recon_scope", "scene"]), 3, 10, 0, terms, 0.1)
    assert "recon[scene softmin tau=0.01] = 0.25000" in step_line(
        p.parse_args(["--recon_loss", "softmin", "--recon_tau", "0.01", "--recon_scope", "scene"]), 3, 10, 0, terms, 0.1)
    a = p.parse_args(["--report_joint", "--collision_radius", "12.5"])
    assert a.report_joint and a.collision_radius == 12.5
