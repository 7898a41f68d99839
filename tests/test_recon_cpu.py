"""CPU-side checks of the best-of-many / soft-min reconstruction loss: the numpy statements of its contract (tests/recon_reference.py) against
each other and against finite differences, the limits and the ordering of the three modes, the generator's conditions, the margins the GPU
gradient tests rely on (through the float64 oracle), the ABI surface and train.py's flags."""
import os
import re

import numpy as np
import pytest

from tests.helpers import make_case, small_dims, to_oracle_layout
from tests.recon_reference import GAP, MEAN, MIN, SOFTMIN, bom_loss_and_grads, make_recon_case, recon_f32, recon_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 8, 3, 7), (3, 1, 1, 7), (1, 32, 20, 40), (2, 32, 70, 5)]


def _dims(shape):
    n, m, K, T = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=6, T_pred=T, n_grids=1)


@pytest.fixture(scope="module")
def cases():
    return {s: (_dims(s),) + make_recon_case(_dims(s), seed=100 + i) for i, s in enumerate(SHAPES)}


def test_surface_is_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "desire_hip.h")).read()
    declared = set(re.findall(r"\b(desire_[a-z_]+)\s*\(", hdr))
    for name in ("desire_set_recon_loss", "desire_recon_weights"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert (_lib.RECON_MEAN, _lib.RECON_MIN, _lib.RECON_SOFTMIN) == (0, 1, 2) == (MEAN, MIN, SOFTMIN)
    for k, v in (("MEAN", 0), ("MIN", 1), ("SOFTMIN", 2)):
        assert re.search(r"#define DESIRE_RECON_%s %d\b" % (k, v), hdr)
    assert hasattr(_lib.Handle, "set_recon_loss") and hasattr(_lib.Handle, "recon_weights")
    # argument checks that need no device: the handle comes first
    assert lib.desire_set_recon_loss(None, 1, 0.0) == -1
    assert lib.desire_recon_weights(None, None, None, 1, 0.0, None, None, None, None, None) == -1


@pytest.mark.parametrize("shape", SHAPES)
def test_generator_conditions(cases, shape):
    d, Y, fut, valid, ties = cases[shape]
    r = recon_f64(Y, fut, valid, d, MIN)
    A = d.n_scenes * d.mno
    counted = (fut[..., 0] != 0).transpose(0, 2, 1).reshape(A, d.T_pred)
    if A >= 8:
        assert (valid == 0).any()                                            # absent agents
        assert ((valid != 0) & ~counted.any(1)).any()                        # present, no counted frame
    part = counted.any(1) & ~counted.all(1)
    assert part.any()                                                        # partly counted rows
    assert ((r["e"] == 0).all(1) == ~r["lmask"]).all()                       # e is 0 exactly where the agent does not count
    if d.K > 1:
        t = ties & r["lmask"]
        assert t.any() and (r["gap"][t] == 0).all()
        e = r["e"][t]
        assert (r["winner"][t] == np.argmax(e == e.min(1, keepdims=True), axis=1)).all()      # the tie goes to the lower k
    plain = r["lmask"] & ~ties
    assert plain.any() and (r["gap"][plain] >= GAP * r["e"].min(1)[plain]).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_f32_statement_against_f64(cases, shape):
    d, Y, fut, valid, ties = cases[shape]
    bound = (d.T_pred + 4) * 2.0 ** -24                                      # T_pred additions of correctly rounded terms, one division
    for mode, tau in ((MEAN, 0.0), (MIN, 0.0), (SOFTMIN, 0.01), (SOFTMIN, 1.0)):
        a, b = recon_f32(Y, fut, valid, d, mode, tau), recon_f64(Y, fut, valid, d, mode, tau)
        assert a["e"].dtype == np.float32 and a["w"].dtype == np.float32 and a["recon"].dtype == np.float32
        assert (np.abs(a["e"] - b["e"]) <= bound * b["e"]).all()
        np.testing.assert_array_equal(a["winner"], b["winner"])
        np.testing.assert_array_equal(a["lmask"], b["lmask"])
        # the weights: a relative error of e of `bound` moves (e - m) / tau by bound * e / tau
        wtol = 4 * bound * (1.0 + (b["e"].max() / tau if mode == SOFTMIN else 0.0)) + 1e-7
        assert np.abs(a["w"] - b["w"]).max() <= wtol
        assert np.abs(a["recon"] - b["recon"]).max() <= 4 * bound * max(1.0, b["e"].max()) + 1e-7
        np.testing.assert_allclose(b["w"].sum(1), 1.0, rtol=0, atol=1e-12)


def test_a_nan_never_wins_against_a_number():
    d = _dims((1, 1, 4, 3))
    fut = np.ones((1, 3, 1, 3), np.float32)
    for dt in (recon_f32, recon_f64):
        Y = np.zeros((4, 3, 2), np.float32)
        Y[:, :, 0] = np.array([3.0, 2.0, 1.0, 2.5], np.float32)[:, None]
        Y[0, 1, 0] = np.nan                                                  # e[0] is a NaN; the numbers 2, 1, 2.5 follow
        r = dt(Y, fut, np.ones(1, np.uint8), d, MIN)
        assert np.isnan(r["e"][0, 0]) and r["winner"][0] == 2
        Y[2, 0, 1] = np.nan                                                  # the smallest becomes a NaN too: the next strict minimum wins
        assert dt(Y, fut, np.ones(1, np.uint8), d, MIN)["winner"][0] == 1


@pytest.mark.parametrize("shape", SHAPES[:2] + SHAPES[3:])
def test_modes_are_ordered_and_meet_at_the_limits(cases, shape):
    d, Y, fut, valid, ties = cases[shape]
    mean, mn = recon_f64(Y, fut, valid, d, MEAN), recon_f64(Y, fut, valid, d, MIN)
    for tau in (1e-3, 0.01, 0.1, 1.0):
        sm = recon_f64(Y, fut, valid, d, SOFTMIN, tau)
        assert (mn["recon"] <= sm["recon"] + 1e-15).all() and (sm["recon"] <= mean["recon"] + 1e-15).all()
    big, small = recon_f64(Y, fut, valid, d, SOFTMIN, 1e6), recon_f64(Y, fut, valid, d, SOFTMIN, 1e-6)
    np.testing.assert_allclose(big["recon"], mean["recon"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(big["w"], mean["w"], rtol=0, atol=1e-7)
    # tau -> 0: the min, and its one-hot weights -- away from ties and from agents that do not count (all errors 0), where the equal rows share the mass
    np.testing.assert_allclose(small["recon"], mn["recon"], rtol=0, atol=1e-6 * np.log(d.K) + 1e-15)
    plain = ~ties & mn["lmask"]
    assert np.abs(small["w"][plain] - mn["w"][plain]).max() <= d.K * np.exp(-mn["gap"][plain].min() / 1e-6) + 1e-12      # (a loser keeps exp(-gap / tau) at most)
    if d.K > 1:
        t = ties & mn["lmask"]
        assert (np.sort(small["w"][t], 1)[:, -2:] == 0.5).all()


def test_softmin_gradient_against_central_differences(cases):
    """d recon / d e_k = w_k, and through e the contract's d recon / d Y = w / (nfut nrm) (Y - g) on counted frames: float64 central differences
    of the statement's own recon."""
    d, Y, fut, valid, ties = cases[(2, 8, 3, 7)]
    tau = float(np.float32(0.01))                                            # (the statements take tau as the fp32 value the ABI carries)
    r = recon_f64(Y, fut, valid, d, SOFTMIN, tau)
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    g = np.stack([fut[..., 1] * np.float32(d.sx), fut[..., 2] * np.float32(d.sy)], -1).astype(np.float32).astype(np.float64)      # [n, T, m, 2]
    counted = fut[..., 0] != 0
    nfut = counted.sum(1)                                                    # [n, m]
    Y64 = Y.astype(np.float64).reshape(n, K, m, T, 2)
    rng = np.random.default_rng(5)
    h = 1e-6
    checked = 0
    for _ in range(60):
        sc, k, s, t, c = (int(rng.integers(x)) for x in (n, K, m, T, 2))
        a = sc * m + s
        if not r["lmask"][a]:
            continue
        diff = Y64[sc, k, s, t] - g[sc, t, s]
        want = r["w"][a, k] / (nfut[sc, s] * np.linalg.norm(diff)) * diff[c] if counted[sc, t, s] else 0.0

        def f(delta):
            # (float64 perturbations of an fp32 input: evaluate the float64 statement on float64 rows directly)
            Yp = Y64.copy()
            Yp[sc, k, s, t, c] += delta
            dx = Yp[sc, :, s, :, 0] - g[sc, :, s, 0][None]
            dy = Yp[sc, :, s, :, 1] - g[sc, :, s, 1][None]
            e = (np.sqrt(dx * dx + dy * dy) * counted[sc, :, s][None]).sum(1) / nfut[sc, s]
            return e.min() - tau * np.log(np.exp(-(e - e.min()) / tau).sum() / K)

        assert abs(f(0.0) - r["recon"][a]) < 1e-12
        got = (f(h) - f(-h)) / (2 * h)
        assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (sc, k, s, t, c, got, want)
        checked += 1
    assert checked >= 20


def _oracle_case(shape, seed, n_absent, mode, tau=0.0):
    from desire_amd.spec import init_weights
    from tests.stage_reference import spread_weights
    d = _dims(shape)
    w = spread_weights(init_weights(d, 41))
    past, fut, eps, grids, gos = make_case(d, seed=seed, n_absent=n_absent)
    return bom_loss_and_grads(to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos, w, d, mode, tau)


def test_margins_of_the_hard_min_gradient_cases():
    """The two cases the GPU hard-min gradient test uses keep every counted agent's best and second-best float64 error at least 1e-4 apart
    (five times the 2e-5 device-to-oracle trajectory deviation the README records); test_gpu_train.py's own case does not (3.7e-8)."""
    vals, _ = _oracle_case((2, 8, 3, 7), 84, 2, MIN)
    c = vals["counted"]
    assert c.sum() == 12 and vals["gap"][c].min() >= 1e-4
    assert abs(vals["gap"][c].min() - 1.40e-4) < 1e-6
    np.testing.assert_array_equal(np.bincount(vals["winner"][c], minlength=3), [5, 3, 4])
    vals, _ = _oracle_case((3, 1, 3, 7), 99, 0, MIN)
    c = vals["counted"]
    assert c.sum() == 3 and vals["gap"][c].min() >= 1e-4
    assert abs(vals["gap"][c].min() - 9.96e-3) < 1e-5
    # gap / tau >= 140 > 104 = -log(the smallest fp32 subnormal): at tau = 1e-6 every loser's expf is 0.f and the soft-min weights are one-hot
    assert 1.40e-4 / 1e-6 > 104 > -np.log(2.0 ** -149)


def test_rebuilt_loss_reduces_to_the_oracles_in_mean_mode_and_orders_the_modes():
    from desire_amd.spec import init_weights
    from oracle import desire_torch as OT
    from tests.stage_reference import spread_weights
    d = _dims((2, 8, 3, 7))
    w = spread_weights(init_weights(d, 41))
    past, fut, eps, grids, gos = make_case(d, seed=84, n_absent=2)
    ref_vals, ref_g = OT.loss_and_grads(to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos, w, d)
    v0, g0 = _oracle_case((2, 8, 3, 7), 84, 2, MEAN)
    assert abs(v0["loss"] - float(ref_vals["loss"])) < 1e-12
    for k in ("head/w", "dec/gates/kernel", "enc_x/gates/kernel", "ioc/reg/w"):
        np.testing.assert_allclose(g0[k], ref_g[k], rtol=0, atol=1e-12 * max(1.0, np.abs(ref_g[k]).max()))
    v1, g1 = _oracle_case((2, 8, 3, 7), 84, 2, MIN)
    v2, g2 = _oracle_case((2, 8, 3, 7), 84, 2, SOFTMIN, 0.01)
    c = v0["counted"]
    assert (v1["recon"][c] <= v2["recon"][c]).all() and (v2["recon"][c] <= v0["recon"][c]).all()
    assert (v1["recon"][c] < v0["recon"][c]).any()
    for k in ("ioc/reg/w", "ioc/gates/kernel", "ioc/score/w"):             # the IOC module sees detached trajectories: its gradients do not move
        np.testing.assert_array_equal(g1[k], g0[k])
        np.testing.assert_array_equal(g2[k], g0[k])
    assert np.abs(g1["head/w"] - g0["head/w"]).max() > 0


def test_train_flags_parse_and_refuse():
    from desire_amd.train import build_parser, check_recon_args, step_line
    p = build_parser()
    a = p.parse_args([])
    assert a.recon_loss == "mean" and a.recon_tau is None
    check_recon_args(a)
    a = p.parse_args(["--recon_loss", "min"])
    check_recon_args(a)
    a = p.parse_args(["--recon_loss", "softmin", "--recon_tau", "0.02"])
    check_recon_args(a)
    assert a.recon_tau == 0.02
    with pytest.raises(SystemExit):
        p.parse_args(["--recon_loss", "best"])
    for argv in (["--recon_loss", "softmin"], ["--recon_loss", "softmin", "--recon_tau", "0"], ["--recon_loss", "softmin", "--recon_tau", "-1"],
                 ["--recon_loss", "softmin", "--recon_tau", "nan"], ["--recon_loss", "softmin", "--recon_tau", "inf"],
                 ["--recon_loss", "min", "--recon_tau", "0.1"], ["--recon_tau", "0.1"]):
        with pytest.raises(ValueError):
            check_recon_args(p.parse_args(argv))
    terms = {"loss": 1.5, "recon": 0.25}
    assert "recon" not in step_line(p.parse_args([]), 3, 10, 0, terms, 0.1)
    assert step_line(p.parse_args([]), 3, 10, 0, terms, 0.1) == "3/10 (epoch 0), train_loss = 1.500, time/batch = 0.100"
    assert "recon[min] = 0.25000" in step_line(p.parse_args(["--recon_loss", "min"]), 3, 10, 0, terms, 0.1)
    assert "recon[softmin tau=0.02] = 0.25000" in step_line(p.parse_args(["--recon_loss", "softmin", "--recon_tau", "0.02"]), 3, 10, 0, terms, 0.1)
