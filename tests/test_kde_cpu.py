"""KDE log-likelihood, the parts that need no GPU: the export and the Python surface, and the two statements of the contract in
tests/kde_reference.py against each other -- the fp32 restatement against scipy's float64 density, the shift under a change of units, the
planted degenerate frames and the non-finite scores."""
import os
import re

import numpy as np
import pytest

from tests.helpers import make_case, small_dims
from tests.kde_reference import LOG_FLOOR, kde_nll_f32, kde_nll_f64, kde_outputs, make_samples
from tests.rank_reference import planted_scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_call_is_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    import ctypes
    from desire_amd import _lib, evaluate as E, train as T
    from desire_amd.model import DESIREModel
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "desire_hip.h")).read()
    declared = set(re.findall(r"^int (desire_\w+)\(", hdr, re.M))
    assert "desire_kde_nll" in declared and "desire_kde_nll" in _lib.EXPORTS and hasattr(lib, "desire_kde_nll")
    assert "#define DESIRE_KDE_MIN_DET_RATIO 1e-5f" in hdr
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    hz = (ctypes.c_int32 * 1)(1)
    one = ctypes.c_float(1)
    assert lib.desire_kde_nll(None, None, None, None, hz, 1, one, one, ctypes.c_float(-20), None, None, None) == -1      # DESIRE_ERR_ARG
    assert b"handle" in lib.desire_last_error()
    assert hasattr(_lib.Handle, "kde_nll") and hasattr(DESIREModel, "evaluate_nll") and _lib.KDE_LOG_FLOOR == -20.0
    e = E.build_parser().parse_args(["--checkpoint", "c.npz"])
    assert e.nll is False
    assert E.build_parser().parse_args(["--checkpoint", "c.npz", "--nll"]).nll is True
    assert T.build_parser().parse_args([]).report_nll is False and T.build_parser().parse_args(["--report_nll"]).report_nll is True


def _case(K=7, seed=3, **kw):
    """3 windows x 8 slots, T_pred = 12, sx != sy; objects leaving early / never in the target / with gaps; the planted scores."""
    d = small_dims(n_scenes=3, mno=8, K=K, T_obs=4, T_pred=12, n_grids=1, H=64)
    _, fut, _, _, _ = make_case(d, seed=seed, n_absent=2)
    fut = fut.copy()
    fut[0, 3:, 1] = 0; fut[0, 1:, 4] = 0; fut[0, :, 3] = 0; fut[1, 2:5, 2] = 0; fut[2, :2, 0] = 0; fut[1, d.T_pred - 1:, 0] = 0
    s = planted_scores(d, seed + 2)
    Y, planted = make_samples(d, fut, s, seed + 1, worst_log_unit=float(np.log(1.0 / (d.sx * d.sy))), **kw)
    return d, Y, fut, s, planted


def _counted(fut, d):
    return (fut[..., 0] != 0).transpose(0, 2, 1).reshape(d.A, d.T_pred)


@pytest.fixture(scope="module")
def case():
    return _case()


def test_the_fp32_restatement_agrees_with_scipy(case):
    d, Y, fut, s, planted = case
    c = _counted(fut, d)
    worst = 0.0
    for K in (3, 7, 20, 130):
        dd, YY, ff, ss, pl = (d, Y, fut, s, planted) if K == 7 else _case(K=K, seed=10 + K)
        cc = _counted(ff, dd)
        for score in (None, ss):
            for ux, uy in ((1.0, 1.0), (1.0 / dd.sx, 1.0 / dd.sy), (0.2 / dd.sx, 0.2 / dd.sy)):
                w64, shape, raw = kde_nll_f64(YY, ff, score, ux, uy, LOG_FLOOR, dd, want_shape=True)
                w32 = kde_nll_f32(YY, ff, score, ux, uy, LOG_FLOOR, dd)
                free = cc & ~pl
                assert free.sum() > 10 * pl[cc].sum() > 0
                assert (shape[free] >= 0.05).all() and (np.abs(raw[free] - LOG_FLOOR) > 0.05).all()      # the inputs are what they claim to be
                assert (w64[free] > LOG_FLOOR).all()
                err = float(np.abs(w32.astype(np.float64) - w64).max())
                worst = max(worst, err)
                print("K %d %s units (%g, %g): max |f32 - f64| = %.3g" % (K, "weighted" if score is not None else "uniform", ux, uy, err))
                # fp32 against float64 on frames with 1 - rho^2 >= 0.05: the determinant loses a factor 20 to cancellation, the moments are
                # sums of K terms of one sign: some tens of 6e-8 relative on det, i.e. absolute on a log-density of magnitude <= 20
                assert err <= 2e-4
                np.testing.assert_array_equal(w32[cc & pl], np.float32(LOG_FLOOR))
                np.testing.assert_array_equal(w64[cc & pl], LOG_FLOOR)
                assert not w32[~cc].any() and not w64[~cc].any()
    print("max |kde_nll_f32 - kde_nll_f64| over every case: %.3g" % worst)


def test_outputs_are_the_mean_and_the_last_counted_frame(case):
    d, Y, fut, s, _ = case
    fr = kde_nll_f64(Y, fut, s, 1.0, 1.0, LOG_FLOOR, d)
    c = _counted(fut, d)
    out = kde_outputs(fr, fut, [1, 3, 6, 12], d)
    for a in range(d.A):
        for i, h in enumerate([1, 3, 6, 12]):
            idx = np.nonzero(c[a, :h])[0]
            want = (-fr[a, idx].mean(), -fr[a, idx[-1]]) if idx.size else (0.0, 0.0)
            np.testing.assert_allclose(out[a, i], want, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(out[:, 0, 0], out[:, 0, 1])      # h = 1: mean = final
    assert not out[~c.any(1)].any() and (~c.any(1)).any()


def test_scaling_both_units_shifts_the_log_density(case):
    d, Y, fut, s, planted = case
    c = _counted(fut, d) & ~planted
    for score in (None, s):
        for cc in (5.0, 0.25):
            a64 = kde_nll_f64(Y, fut, score, 3.0, 7.0, -1e30, d)
            b64 = kde_nll_f64(Y, fut, score, 3.0 * cc, 7.0 * cc, -1e30, d)
            np.testing.assert_allclose(b64[c], a64[c] - 2.0 * np.log(cc), rtol=0, atol=1e-9)
            a32 = kde_nll_f32(Y, fut, score, 3.0, 7.0, -1e30, d)
            b32 = kde_nll_f32(Y, fut, score, 3.0 * cc, 7.0 * cc, -1e30, d)
            # each fp32 value is within the agreement test's bound of its float64 value
            np.testing.assert_allclose(b32[c].astype(np.float64), a32[c].astype(np.float64) - 2.0 * np.log(cc), rtol=0, atol=4e-4)


def _floor_everywhere(d, Y, fut, s, agents=None):
    c = _counted(fut, d)
    if agents is not None:
        c = c & np.isin(np.arange(d.A), agents)[:, None]
    assert c.sum() > 0
    for score in (None, s):
        for ux, uy in ((1.0, 1.0), (1.0 / d.sx, 1.0 / d.sy)):
            np.testing.assert_array_equal(kde_nll_f32(Y, fut, score, ux, uy, LOG_FLOOR, d)[c], np.float32(LOG_FLOOR))
            np.testing.assert_array_equal(kde_nll_f64(Y, fut, score, ux, uy, LOG_FLOOR, d)[c], LOG_FLOOR)


@pytest.mark.parametrize("K", [1, 2])
def test_one_and_two_samples_are_the_floor(K):
    d, Y, fut, s, _ = _case(K=K, seed=5)
    _floor_everywhere(d, Y, fut, s)


def test_coincident_and_equal_y_samples_are_the_floor():
    d, Y, fut, s, _ = _case(K=5, seed=6, plant=False)
    Yk = Y.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2)
    Yk[1, :, 1] = Yk[1, :1, 1]                                    # agent (1, 1): the K samples coincide
    Yk[2, :, 3, :, 1] = Yk[2, :1, 3, :, 1]                        # agent (2, 3): equal y
    Yk[0, :, 0] = 0                                               # an absent slot's rows under the padding-skipping flags
    _floor_everywhere(d, Y, fut, s, agents=[1 * d.mno + 1, 2 * d.mno + 3, 0])


def test_a_one_hot_score_is_the_floor():
    d, Y, fut, s, _ = _case(K=5, seed=7, plant=False)
    s = s.copy()
    hot = [(1, 1), (2, 3)]
    for n, m in hot:
        s[n, :, m] = np.random.default_rng(n).standard_normal(d.K).astype(np.float32)
        s[n, 2, m] += 80.0
    c = _counted(fut, d) & np.isin(np.arange(d.A), [n * d.mno + m for n, m in hot])[:, None]
    assert c.sum() > 0
    for ux, uy in ((1.0, 1.0), (1.0 / d.sx, 1.0 / d.sy)):
        np.testing.assert_array_equal(kde_nll_f32(Y, fut, s, ux, uy, LOG_FLOOR, d)[c], np.float32(LOG_FLOOR))
        np.testing.assert_array_equal(kde_nll_f64(Y, fut, s, ux, uy, LOG_FLOOR, d)[c], LOG_FLOOR)


def test_an_agent_with_a_non_finite_score_gets_equal_weights(case):
    d, Y, fut, s, _ = case
    sa = np.asarray(s).reshape(d.n_scenes, d.K, d.mno).transpose(0, 2, 1).reshape(d.A, d.K)
    bad = ~np.isfinite(sa).all(1)
    kinds = sa[bad]
    assert np.isnan(kinds).any() and np.isposinf(kinds).any() and np.isneginf(kinds).any()
    c = _counted(fut, d)
    assert (c & bad[:, None]).sum() > 0
    for fn in (kde_nll_f32, kde_nll_f64):
        u = fn(Y, fut, None, 1.0, 1.0, LOG_FLOOR, d)
        w = fn(Y, fut, s, 1.0, 1.0, LOG_FLOOR, d)
        np.testing.assert_array_equal(w[bad], u[bad])
        assert (w[~bad] != u[~bad]).any()
