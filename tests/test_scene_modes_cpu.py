"""The numpy statements of the scene-mode contract (tests/scene_modes_reference.py) against each other, against the per-agent statement
(tests/modes_reference.py) where the two must coincide, against scikit-learn's k-means and scipy's Gaussian density, against the conditions their
generator promises, the ABI of desire_fit_scene_modes, and the mirror of the kernel's LDS geometry against desire_amd/csrc/eval_lds.h
(tests/c_host/scene_modes_lds_driver.cpp, compiled with g++: no ROCm header, no GPU)."""
import itertools
import json
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from tests.modes_reference import modes_f32
from tests.scene_modes_reference import (ITERS, LOG_FLOOR, MARGIN, MODES_MAX, MODES_MAX_ITERS, SHAPES, case, fixed_bytes, scene_bounds, scene_modes_f32,
                                         scene_modes_f64, scene_modes_geometry, slot_bytes, t_ends)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "scene_modes_lds_driver.cpp")
IDS = lambda s: "n%d_m%d_K%d_T%d_n%d" % s


def all_cases():
    return [case(s, u, te) for s in SHAPES for u in (0, 1) for te in t_ends(s[3])]


def test_the_abi_is_declared_listed_and_exported():
    from desire_amd import _lib
    with open(os.path.join(ROOT, "include", "desire_hip.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint desire_fit_scene_modes\(desire_handle\* h, const float\* dev_Yhat, const uint8_t\* dev_present, const int32_t\* dev_worder,", text)
    assert "desire_fit_scene_modes" in _lib.EXPORTS and callable(getattr(_lib.Handle, "fit_scene_modes"))
    lib = _lib.load()
    assert len(lib.desire_fit_scene_modes.argtypes) == 24
    # refused without a handle, before anything touches a device: the checks that need none come first
    none = [None] * 9
    assert lib.desire_fit_scene_modes(None, None, None, None, None, None, 0, 1, 1, 1.0, 1.0, 0.0, None, 0, 0.0, *none) == -1
    assert b"n_modes" in lib.desire_last_error()
    assert lib.desire_fit_scene_modes(None, None, None, None, None, None, 2, 1, 1, 1.0, 1.0, 0.0, None, 0, 0.0, *none) == -1
    assert b"dev_Yhat" in lib.desire_last_error()
    # the limit of the LDS plan is stated as the same formula in the header and in the message
    formula = "8 * (K + n_modes) * (T_pred | 1) + 20 * n_modes * T_pred + 12 * K * n_modes + 12 * K + 20 * n_modes + 4 * n_modes * ceil(K / 32) + 12 * T_pred + 4 * mno"
    assert formula in re.sub(r"\s*\n \*\s*", " ", text)
    with open(os.path.join(ROOT, "desire_amd", "csrc", "api_eval.hip")) as fh:
        assert "scene-mode kernel's LDS" in fh.read()


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_margin_holds_and_the_two_precisions_agree(shape, unit):
    for te in t_ends(shape[3]):
        c = case(shape, unit, te)
        d = c["d"]
        assert d.mno * te <= 4096 and (d.mno * te + 4) * 2.0 ** -24 * 2 < MARGIN      # the margin stays above twice the summation bound of a D
        for tag in ("scored", "uniform"):
            f32, f64 = c[tag]["f32"], c[tag]["f64"]
            assert f64["margin"].min() > MARGIN                            # the float64 pass alone, before any comparison
            for key in ("label", "count", "passes"):
                np.testing.assert_array_equal(f32[key], f64[key], err_msg=key)
            for key, bound in zip(("prob", "mean", "cov"), scene_bounds(c["Y"], f64, c["ux"], c["uy"], c["vf"], d)):
                fin = np.isfinite(f64[key])
                np.testing.assert_array_equal(np.isnan(f32[key]), np.isnan(f64[key]), err_msg=key)
                assert (np.abs(f32[key].astype(np.float64) - f64[key])[fin] <= bound[fin]).all(), key
            gone = ~f64["part"]
            assert not f64["mean"].transpose(0, 2, 1, 3, 4)[gone].any() and not f64["cov"].transpose(0, 2, 1, 3, 4)[gone].any()
            assert (f64["count"].sum(1) == (f64["label"] >= 0).sum(1)).all() and f64["passes"].max() <= ITERS
            for w in c["info"]["bad"]:
                assert (f64["label"][w] == -1).all() and not f64["prob"][w].any() and f64["passes"][w] == 0
            if c["info"]["empty"] >= 0:                                    # nobody takes part: every D is 0, every world joins mode 0, p = 1
                w = c["info"]["empty"]
                assert (f64["label"][w] == 0).all() and f64["passes"][w] == 1 and f64["count"][w, 0] == d.K and not f64["mean"][w].any()
                assert not f64["frame"][w].any() and not f64["out"][w].any()
            if c["info"]["nan"] is not None:                               # the NaN world: label -1, its mass missing
                w, k, _ = c["info"]["nan"]
                assert f64["label"][w, k] == -1 and f64["prob"][w].sum() < 1 - 0.5 * f64["weights"][w, k]


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_statements_reproduce_the_recorded_digests(shape, unit):
    """Every array of scene_modes_f32 and scene_modes_f64 has the bytes it had when tests/golden/modes_reference_digests.json was recorded."""
    from tests.golden.make_modes_reference_digests import PATH, digest, name
    with open(PATH) as fh:
        assert digest(case(shape, unit)) == json.load(fh)[name("scene_modes", shape, unit)]


def test_the_redraw_caps_hold_and_the_iteration_is_exercised():
    cs = all_cases()
    redraws, windows = sum(c["info"]["redraws"] for c in cs), sum(c["info"]["windows"] for c in cs)
    hist = np.bincount(np.concatenate([c["scored"]["f64"]["passes"] for c in cs]))
    print("redrawn %d of %d windows; passes %s" % (redraws, windows, hist.tolist()))
    assert redraws <= 0.10 * windows
    for s in SHAPES:
        mine = [c for c in cs if c["d"].n_scenes == s[0] and (c["d"].mno, c["d"].K, c["d"].T_pred, c["n"]) == s[1:]]
        assert sum(c["info"]["redraws"] for c in mine) <= 0.25 * sum(c["info"]["windows"] for c in mine), s
    assert hist[2:].sum() >= 5                                             # more than one pass: update and assign both run


def test_one_slot_is_the_per_agent_statement_bit_for_bit():
    """The anchor: at mno = 1 the window IS the agent -- every output of scene_modes_f32 has the bits of modes_f32 given the same order row, the
    agent's scores and the same targets."""
    for unit in (0, 1):
        for te in t_ends(SHAPES[1][3]):
            c = case(SHAPES[1], unit, te)
            d, n = c["d"], c["n"]
            here = np.nonzero(c["present"])[0]                           # the anchor speaks of a present slot: the last window has nobody
            assert d.mno == 1 and here.tolist() == [0, 1]
            for tag, s in (("scored", c["wscore"]), ("uniform", None)):
                mine = c[tag]["f32"]
                per = modes_f32(c["Y"], c["worder"], None if s is None else s.reshape(d.n_scenes, d.K, 1), c["fut"], n, te, ITERS, c["ux"], c["uy"],
                                c["vf"], d, c["hz"])
                for key in ("label", "count", "passes"):
                    np.testing.assert_array_equal(mine[key][here], per[key][here], err_msg=key)
                for key in ("prob", "frame", "out"):
                    np.testing.assert_array_equal(mine[key][here].view(np.uint32), per[key][here].view(np.uint32), err_msg=key)
                np.testing.assert_array_equal(mine["mean"][here, :, 0].view(np.uint32), per["mean"][here].view(np.uint32))
                np.testing.assert_array_equal(mine["cov"][here, :, 0].view(np.uint32), per["cov"][here].view(np.uint32))
            assert c["info"]["bad"] == [1] and (mine["label"][1] == -1).all()


def test_one_slot_taking_part_out_of_several_is_that_slots_per_agent_fit():
    c = case(SHAPES[0], 1)
    d, n, K, m = c["d"], c["n"], c["d"].K, c["d"].mno
    slot = 3
    present = np.zeros((d.n_scenes, m), np.uint8)
    present[:, slot] = 1
    order = np.repeat(c["worder"][:, None], m, 1).reshape(d.A, K)
    score = np.repeat(c["wscore"][:, :, None], m, 2)                       # every agent of a window holds the window's scores
    for s_w, s_a in ((c["wscore"], score), (None, None)):
        mine = scene_modes_f32(c["Y"], present, c["worder"], s_w, c["fut"], n, d.T_pred, ITERS, c["ux"], c["uy"], c["vf"], d, c["hz"])
        per = modes_f32(c["Y"], order, s_a, c["fut"], n, d.T_pred, ITERS, c["ux"], c["uy"], c["vf"], d, c["hz"])
        ag = np.arange(d.n_scenes) * m + slot
        for key in ("label", "count", "passes"):
            np.testing.assert_array_equal(mine[key], per[key][ag], err_msg=key)
        for key in ("prob", "frame", "out"):
            np.testing.assert_array_equal(mine[key].view(np.uint32), per[key][ag].view(np.uint32), err_msg=key)
        np.testing.assert_array_equal(np.nan_to_num(mine["mean"][:, :, slot]), np.nan_to_num(per["mean"][ag]))
        np.testing.assert_array_equal(np.nan_to_num(mine["cov"][:, :, slot]), np.nan_to_num(per["cov"][ag]))
        others = np.setdiff1d(np.arange(m), [slot])
        assert not mine["mean"][:, :, others].any() and not mine["cov"][:, :, others].any()


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=IDS)
def test_the_converged_partition_is_scikit_learns(shape):
    cluster = pytest.importorskip("sklearn.cluster")
    c = case(shape)
    d, n, K, T = c["d"], c["n"], c["d"].K, c["d"].T_pred
    f64 = scene_modes_f64(c["Y"], c["present"], c["worder"], c["wscore"], None, n, T, MODES_MAX_ITERS, c["ux"], c["uy"], c["vf"], d)
    u2 = np.array([float(np.float32(c["ux"])), float(np.float32(c["uy"]))])
    Yk = c["Y"].reshape(d.n_scenes, K, d.mno, T, 2).astype(np.float64)
    done = 0
    for w in range(d.n_scenes):
        sl = np.nonzero(f64["part"][w])[0]
        keep = f64["label"][w] >= 0                                        # the NaN world takes no part in either
        if sl.size == 0 or (f64["count"][w] == 0).any() or f64["passes"][w] >= MODES_MAX_ITERS or not keep[c["worder"][w, :n]].all():
            continue                                                       # (scikit-learn relocates an empty cluster; the contract keeps its mean)
        X = (Yk[w][:, sl] * u2).reshape(K, -1)                              # the worlds flattened over taking-part slots and frames
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            km = cluster.KMeans(n_clusters=n, init=X[c["worder"][w, :n]], n_init=1, algorithm="lloyd", tol=0, max_iter=300)
            km.fit(X[keep], sample_weight=f64["weights"][w][keep])
        np.testing.assert_array_equal(km.labels_, f64["label"][w][keep], err_msg="window %d" % w)
        done += 1
    assert done >= 1


def test_the_joint_log_density_is_scipys():
    stats = pytest.importorskip("scipy.stats")
    special = pytest.importorskip("scipy.special")
    checked = 0
    for shape in (SHAPES[0], SHAPES[2], SHAPES[4]):
        c = case(shape, 0)
        d, n, T = c["d"], c["n"], c["d"].T_pred
        f64 = c["scored"]["f64"]
        f = np.asarray(c["fut"], np.float32)                               # [N, T, mno, 3]
        g = np.stack([f[..., 1] * np.float32(d.sx), f[..., 2] * np.float32(d.sy)], -1).astype(np.float64)
        u2 = np.array([float(np.float32(c["ux"])), float(np.float32(c["uy"]))])
        for w in range(d.n_scenes):
            for t in range(0, T, 5):
                Ct = [s for s in np.nonzero(f64["part"][w])[0] if f[w, t, s, 0] != 0]
                if not Ct or not f64["frame"][w, t] > LOG_FLOOR or np.isnan(f64["mean"][w][:, Ct, t]).any():
                    continue
                terms = []
                for i in range(n):
                    covs = f64["cov"][w, i, Ct, t]
                    if f64["prob"][w, i] > 0 and (covs[:, 0] * covs[:, 1] - covs[:, 2] ** 2 > 1e-5 * covs[:, 0] * covs[:, 1]).all():
                        lp = np.log(f64["prob"][w, i])
                        for s, (cxx, cyy, cxy) in zip(Ct, covs):               # agents are independent given the mode
                            lp += stats.multivariate_normal.logpdf((f64["mean"][w, i, s, t] - g[w, t, s]) * u2, mean=[0, 0], cov=[[cxx, cxy], [cxy, cyy]])
                        terms.append(lp)
                np.testing.assert_allclose(f64["frame"][w, t], special.logsumexp(terms) / len(Ct), rtol=1e-9, atol=1e-9)
                checked += 1
    assert checked >= 8


# ---- the geometry mirror against the header
MNO = [1, 2, 4, 8, 32, 64, 160, 256]
KS = [1, 2, 3, 20, 33, 64, 65, 130, 600]
TS = [1, 5, 9, 12, 40, 200, 2000]
NS = [1, 2, 6, 16]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("scene_modes_lds") / "scene_modes_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_geometry_mirror_equals_the_header(driver):
    shapes = [s for s in itertools.product(MNO, KS, TS, NS) if s[3] <= s[1]]
    reqs = ["budget"] + ["scene %d %d %d %d" % s for s in shapes]
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs) and rows[0] == (60 * 1024, 256, MODES_MAX, MODES_MAX_ITERS)
    budget = rows[0][0]
    fits = 0
    for (m, K, T, n), (ok, sc, nbytes, end, fixed, slot) in zip(shapes, rows[1:]):
        assert (fixed, slot) == (fixed_bytes(K, T, n, m), slot_bytes(K, T, n)), (m, K, T, n)
        want = scene_modes_geometry(m, K, T, n)
        assert bool(ok) == (want is not None) == (fixed + slot <= budget), (m, K, T, n)
        if not ok:
            continue
        fits += 1
        assert sc == want, (m, K, T, n)
        assert nbytes == end == fixed + sc * slot <= budget, (m, K, T, n)
        chunks = -(-m // sc)
        assert 1 <= sc <= m and (chunks - 1) * sc < m <= chunks * sc, (m, K, T, n)      # every slot once
    assert 0 < fits < len(shapes)
    for s in SHAPES + [(1, 256, 20, 40, 6)]:                               # every tested shape, and the widest window of the headline, is served
        assert scene_modes_geometry(*s[1:]) is not None, s
    assert scene_modes_geometry(32, 20, 40, 6) == 4 and scene_modes_geometry(256, 20, 40, 6) == 4 and scene_modes_geometry(160, 4, 9, 2) < 160
    assert scene_modes_geometry(1, 40, 200, 16) is None
