"""The numpy statements of the mode-fit contract (tests/modes_reference.py) against each other, against scikit-learn's and scipy's k-means and
scipy's Gaussian density, against the conditions their generator promises, the ABI of desire_fit_modes, and the mirror of the kernel's LDS
geometry against desire_amd/csrc/eval_lds.h (tests/c_host/modes_lds_driver.cpp, compiled with g++: no ROCm header, no GPU)."""
import itertools
import json
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from tests.helpers import small_dims
from tests.modes_reference import (LOG_FLOOR, MARGIN, MODES_MAX, MODES_MAX_ITERS, SHAPES, _rows, agent_bytes, fit_bounds, make_inputs, modes_f32,
                                   modes_f64, modes_geometry, padded_mno, var_floor_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "modes_lds_driver.cpp")
IDS = lambda s: "n%d_m%d_K%d_T%d_n%d" % s
ITERS = 8
_CACHE = {}


def case(shape, unit=1):
    """The shape's inputs and both references under the planted scores and under equal weights, computed once and left unchanged."""
    key = (shape, unit)
    if key not in _CACHE:
        n_s, m, K, T, n = shape
        d = small_dims(n_scenes=n_s, mno=padded_mno(m), K=K, T_obs=4, T_pred=T, n_grids=1, H=64)
        ux, uy = [(1.0, 1.0), (1.0 / d.sx, 1.0 / d.sy)][unit]
        Y, order, score, fut, info = make_inputs(d, n, T, ux, uy, seed=5 + unit, live=m)
        for a in (Y, order, score, fut):
            a.setflags(write=False)
        hz = sorted({max(1, T // 4), max(1, T // 2), T})
        vf = var_floor_of(ux, d.sx)
        c = dict(d=d, n=n, Y=Y, order=order, score=score, fut=fut, info=info, hz=hz, ux=ux, uy=uy, vf=vf)
        for tag, s in (("scored", score), ("uniform", None)):
            c[tag] = {"f32": modes_f32(Y, order, s, fut, n, T, ITERS, ux, uy, vf, d, hz), "f64": modes_f64(Y, order, s, fut, n, T, ITERS, ux, uy, vf, d, hz)}
        _CACHE[key] = c
    return _CACHE[key]


def test_the_abi_is_declared_listed_and_exported():
    from desire_amd import _lib
    with open(os.path.join(ROOT, "include", "desire_hip.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint desire_fit_modes\(desire_handle\* h, const float\* dev_Yhat, const int32_t\* dev_order,", text)
    assert int(re.search(r"#define DESIRE_MODES_MAX (\d+)", text).group(1)) == _lib.MODES_MAX == MODES_MAX
    assert int(re.search(r"#define DESIRE_MODES_MAX_ITERS (\d+)", text).group(1)) == _lib.MODES_MAX_ITERS == MODES_MAX_ITERS
    assert "desire_fit_modes" in _lib.EXPORTS and callable(getattr(_lib.Handle, "fit_modes"))
    lib = _lib.load()
    assert len(lib.desire_fit_modes.argtypes) == 23
    # refused without a handle, before anything touches a device: the checks that need none come first
    assert lib.desire_fit_modes(None, None, None, None, None, 0, 1, 1, 1.0, 1.0, 0.0, None, 0, 0.0, None, None, None, None, None, None, None, None, None) == -1
    assert b"n_modes" in lib.desire_last_error()
    assert lib.desire_fit_modes(None, None, None, None, None, 2, 1, 1, 1.0, 1.0, 0.0, None, 0, 0.0, None, None, None, None, None, None, None, None, None) == -1
    assert b"dev_Yhat" in lib.desire_last_error()


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_margin_holds_and_the_two_precisions_agree(shape, unit):
    c = case(shape, unit)
    d = c["d"]
    for tag in ("scored", "uniform"):
        f32, f64 = c[tag]["f32"], c[tag]["f64"]
        assert f64["margin"].min() > MARGIN                                # the float64 pass alone, before any comparison
        for key in ("label", "count", "passes"):
            np.testing.assert_array_equal(f32[key], f64[key], err_msg=key)
        for key, bound in zip(("prob", "mean", "cov"), fit_bounds(c["Y"], f64, c["ux"], c["uy"], c["vf"], d)):
            fin = np.isfinite(f64[key])
            np.testing.assert_array_equal(np.isnan(f32[key]), np.isnan(f64[key]), err_msg=key)
            assert (np.abs(f32[key].astype(np.float64) - f64[key])[fin] <= bound[fin]).all(), key
        live = np.array([k != "absent" for k in c["info"]["kinds"]])
        np.testing.assert_allclose(f64["prob"].sum(1)[live & (f64["label"] >= 0).all(1)], 1.0, rtol=1e-12)
        assert (f64["count"].sum(1) == (f64["label"] >= 0).sum(1)).all() and f64["passes"].max() <= ITERS


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_statements_reproduce_the_recorded_digests(shape, unit):
    """Every array of modes_f32 and modes_f64 has the bytes it had when tests/golden/modes_reference_digests.json was recorded."""
    from tests.golden.make_modes_reference_digests import PATH, digest, name
    with open(PATH) as fh:
        assert digest(case(shape, unit)) == json.load(fh)[name("modes", shape, unit)]


def test_the_redraw_share_is_small_and_the_special_agents_behave():
    redraws = sum(case(s, u)["info"]["redraws"] for s in SHAPES for u in (0, 1))
    agents = sum(case(s, u)["info"]["agents"] for s in SHAPES for u in (0, 1))
    hist = np.bincount(np.concatenate([case(s, u)["scored"]["f64"]["passes"] for s in SHAPES for u in (0, 1)]))
    print("redrawn %d of %d agents; passes %s" % (redraws, agents, hist.tolist()))
    assert redraws <= 0.05 * agents
    c = case(SHAPES[1])
    d, K, n, f64 = c["d"], c["d"].K, c["n"], c["uniform"]["f64"]
    kinds = c["info"]["kinds"]
    a = kinds.index("zero")
    assert f64["count"][a].tolist() == [K] + [0] * (n - 1) and not f64["mean"][a].any() and (f64["cov"][a][0, :, :2] == float(np.float32(c["vf"]))).all()
    a = kinds.index("nanrow")
    assert (f64["label"][a] == -1).sum() == 1 and abs(f64["prob"][a].sum() - (K - 1) / K) < 1e-12
    a = kinds.index("badscore")
    assert (c["scored"]["f64"]["weights"][a] == 1.0 / K).all() and not np.isfinite(c["score"].transpose(0, 2, 1).reshape(d.A, K)[a]).all()
    a = kinds.index("onehot")
    assert c["scored"]["f64"]["weights"][a].max() > 1 - 1e-10 and (c["scored"]["f64"]["weights"][a] > 0).all()
    a = kinds.index("twoseeds")
    assert f64["passes"].max() >= 2


def _features(c, a, t_end):
    """Agent a's rows over the frames t < t_end, scaled to the call's unit and flattened: the space the assignment distance is Euclidean in."""
    rows = _rows(c["Y"], c["d"]).astype(np.float64)[a, :, :t_end] * np.array([float(np.float32(c["ux"])), float(np.float32(c["uy"]))])
    return rows.reshape(rows.shape[0], -1)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=IDS)
def test_the_converged_partition_is_scikit_learns(shape):
    cluster = pytest.importorskip("sklearn.cluster")
    c = case(shape)
    d, n = c["d"], c["n"]
    f64 = modes_f64(c["Y"], c["order"], c["score"], None, n, d.T_pred, MODES_MAX_ITERS, c["ux"], c["uy"], c["vf"], d)
    done = 0
    for a in range(d.A):
        if c["info"]["kinds"][a] in ("absent", "zero", "nanrow", "nanlate") or (f64["count"][a] == 0).any() or f64["passes"][a] >= MODES_MAX_ITERS:
            continue                                                       # (scikit-learn relocates an empty cluster; the contract keeps its mean)
        X = _features(c, a, d.T_pred)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            km = cluster.KMeans(n_clusters=n, init=X[c["order"][a, :n]], n_init=1, algorithm="lloyd", tol=0, max_iter=300)
            km.fit(X, sample_weight=f64["weights"][a])
        np.testing.assert_array_equal(km.labels_, f64["label"][a], err_msg="agent %d" % a)
        done += 1
    assert done >= 0.8 * sum(k not in ("absent", "zero", "nanrow", "nanlate") for k in c["info"]["kinds"])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=IDS)
def test_equal_weights_are_scipys_kmeans2_at_the_same_pass_count(shape):
    vq = pytest.importorskip("scipy.cluster.vq")
    c = case(shape)
    d, n, T = c["d"], c["n"], c["d"].T_pred
    u2 = np.array([float(np.float32(c["ux"])), float(np.float32(c["uy"]))])
    for p in (0, 1, 2):                                                    # kmeans2's pass i assigns, then updates: p + 1 of them are the contract at iters = p
        f64 = modes_f64(c["Y"], c["order"], None, None, n, T, p, c["ux"], c["uy"], c["vf"], d)
        done = 0
        for a in range(d.A):
            if c["info"]["kinds"][a] in ("absent", "nanrow", "nanlate"):
                continue
            X = _features(c, a, T)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                book, label = vq.kmeans2(X, X[c["order"][a, :n]].copy(), iter=p + 1, minit="matrix", missing="warn")
            if f64["passes"][a] == p:                                      # (an agent that stopped earlier stands still in both)
                np.testing.assert_array_equal(label, f64["label"][a], err_msg="agent %d" % a)
            full = f64["count"][a] > 0
            np.testing.assert_allclose(book[full], (f64["mean"][a] * u2).reshape(n, -1)[full], rtol=1e-9, atol=1e-12)
            done += 1
        assert done > 0


def test_the_mixture_log_density_is_scipys():
    stats = pytest.importorskip("scipy.stats")
    special = pytest.importorskip("scipy.special")
    c = case(SHAPES[1])
    d, n, T = c["d"], c["n"], c["d"].T_pred
    f64 = c["scored"]["f64"]
    f = np.asarray(c["fut"], np.float32).transpose(0, 2, 1, 3).reshape(d.A, T, 3)
    g = np.stack([(f[..., 1] * np.float32(d.sx)), (f[..., 2] * np.float32(d.sy))], -1).astype(np.float64)
    u2 = np.array([float(np.float32(c["ux"])), float(np.float32(c["uy"]))])
    checked = 0
    for a in range(0, d.A, 3):
        for t in range(0, T, 7):
            if f[a, t, 0] == 0 or not f64["frame"][a, t] > LOG_FLOOR or np.isnan(f64["mean"][a, :, t]).any():
                continue
            terms = []
            for i in range(n):
                cxx, cyy, cxy = f64["cov"][a, i, t]
                if f64["prob"][a, i] > 0 and cxx * cyy - cxy * cxy > 1e-5 * cxx * cyy:
                    x = (f64["mean"][a, i, t] - g[a, t]) * u2
                    terms.append(np.log(f64["prob"][a, i]) + stats.multivariate_normal.logpdf(x, mean=[0, 0], cov=[[cxx, cxy], [cxy, cyy]]))
            np.testing.assert_allclose(f64["frame"][a, t], special.logsumexp(terms), rtol=1e-9, atol=1e-9)
            checked += 1
    assert checked > 20


def test_the_evaluation_arguments():
    from desire_amd import evaluate as E
    base = ["--checkpoint", "none.npz"]
    a = E.build_parser().parse_args(base)
    assert (a.modes, a.modes_iters, a.modes_min_std, a.modes_seeds) == (0, 8, 1.0, "nms")
    a = E.build_parser().parse_args(base + ["--modes", "4", "--modes_iters", "3", "--modes_min_std", "0.5", "--modes_seeds", "score"])
    assert (a.modes, a.modes_iters, a.modes_min_std, a.modes_seeds) == (4, 3, 0.5, "score")
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(base + ["--modes", "4", "--modes_seeds", "best"])
    with pytest.raises(ValueError, match="nms_radius"):                    # refused before a model or a window is touched
        E.evaluate(E.build_parser().parse_args(base + ["--modes", "4"]), data_loader=object(), model=object())


# ---- the geometry mirror against the header
MNO = [1, 2, 4, 8, 32, 64, 256]
KS = [1, 2, 3, 20, 33, 64, 65, 130, 600]
TS = [1, 5, 9, 12, 40, 200, 2000]
NS = [1, 2, 6, 16]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("modes_lds") / "modes_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_geometry_mirror_equals_the_header(driver):
    shapes = [s for s in itertools.product(MNO, KS, TS, NS) if s[3] <= s[1]]
    reqs = ["budget"] + ["modes %d %d %d %d" % s for s in shapes]
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs) and rows[0] == (60 * 1024, 256, MODES_MAX, MODES_MAX_ITERS)
    budget = rows[0][0]
    fits = 0
    for (m, K, T, n), (ok, sc, g, nbytes, end, agent) in zip(shapes, rows[1:]):
        assert agent == agent_bytes(K, T, n), (m, K, T, n)
        want = modes_geometry(m, K, T, n)
        assert bool(ok) == (want is not None) == (agent <= budget), (m, K, T, n)
        if not ok:
            continue
        fits += 1
        assert (sc, g) == want, (m, K, T, n)
        assert nbytes == end == sc * agent <= budget, (m, K, T, n)
        chunks = -(-m // sc)
        assert 1 <= sc and sc * g <= max(g, 256) and (chunks - 1) * sc < m <= chunks * sc, (m, K, T, n)      # a group per agent, every slot once
        assert g == min(64, 1 << max(0, (K - 1).bit_length())), (m, K, T, n)
    assert 0 < fits < len(shapes)
    assert modes_geometry(32, 20, 40, 6) == (5, 32) and modes_geometry(2, 130, 9, 4) == (2, 64) and modes_geometry(8, 64, 9, 16) == (4, 64)
    assert modes_geometry(1, 40, 200, 16) is None and modes_geometry(4, 3, 200, 3) is not None
