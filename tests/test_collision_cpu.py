"""CPU-side checks of the collision penalty (desire_collision_loss / desire_set_collision_loss): the LDS plan and frame chunk of k_collision_unit
(desire_amd/csrc/eval_lds.h: CollLds, coll_chunk_frames) compiled with g++ through tests/c_host/coll_lds_driver.cpp -- no ROCm header, no GPU --,
the ABI symbols and their Python binding, the numpy statements against each other and against central differences, and train.py's argument
checks."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.collision_reference import (LDS_BYTES, coll_chunk_centres, coll_chunk_frames, coll_lds_bytes, collision_f32, collision_f64,
                                       make_collision_inputs)
from tests.helpers import small_dims
from tests.joint_reference import MARGIN, RADIUS_PX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "coll_lds_driver.cpp")
# (n_scenes, mno, K, T_pred) of tests/test_gpu_collision_loss.py, and one frame of 256 slots against a very long horizon
SHAPES = [(2, 8, 3, 7), (3, 1, 3, 7), (1, 32, 20, 40), (2, 160, 4, 9), (2, 256, 2, 40), (2, 32, 3, 7), (1, 256, 1, 4000)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("coll_lds") / "coll_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, reqs):
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs)
    return rows


def test_plan_fits_the_budget_and_the_chunk_is_the_largest_that_does(driver):
    (lds, threads), = ask(driver, ["budget"])
    assert lds == LDS_BYTES == 60 * 1024 and threads == 256
    shapes = sorted({(m, T) for _, m, _, T in SHAPES} | set(itertools.product([1, 4, 8, 31, 32, 33, 96, 160, 256], [1, 5, 7, 40, 200, 4000])))
    for (m, T), (tc, nbytes, end, nxt, park) in zip(shapes, ask(driver, ["coll %d %d" % s for s in shapes])):
        assert 1 <= tc <= T, (m, T, tc)
        assert nbytes == end <= lds, (m, T, nbytes, end)
        assert park == tc | 1
        assert tc == T or nxt > lds, (m, T)                                # chunked only where one more frame does not fit
        assert tc == coll_chunk_frames(m, T) and nbytes == coll_lds_bytes(m, tc), (m, T)      # tests/collision_reference.py's own statement


def test_documented_cases(driver):
    got = dict(zip(("32 40", "256 40", "256 4000"), ask(driver, ["coll 32 40", "coll 256 40", "coll 256 4000"])))
    assert got["32 40"][:2] == (40, 33 * 40 * 8 + 32 * 41 * 12 + 4 * (64 + 1))
    assert got["256 40"][0] == got["256 4000"][0] == 11                    # the frame-chunked walk: 11 + 11 + 11 + 7 frames
    assert coll_chunk_centres(256, 40) == [5, 10, 11, 36] and coll_chunk_centres(32, 40) is None


def test_abi_symbols_and_binding():
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "desire_hip.h")).read()
    for name in ("desire_collision_loss", "desire_set_collision_loss"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert len(lib.desire_collision_loss.argtypes) == 11 and len(lib.desire_set_collision_loss.argtypes) == 5
    assert callable(_lib.Handle.collision_loss) and callable(_lib.Handle.set_collision_loss)
    # the checks that need no device: a NULL handle is refused with a text
    assert lib.desire_collision_loss(None, None, None, 1.0, 1.0, 1.0, None, None, None, None, None) == -1
    assert b"handle" in lib.desire_last_error()
    assert lib.desire_set_collision_loss(None, 1.0, 1.0, 1.0, 1.0) == -1


def _case(shape=(2, 8, 3, 7), unit=1):
    n, m, K, T = shape
    d = small_dims(n_scenes=n, mno=m, K=K, T_obs=6, T_pred=T, n_grids=1)
    ux, uy, radius = [(1.0, 1.0, float(np.float32(RADIUS_PX * d.sx))), (1.0 / d.sx, 1.0 / d.sy, RADIUS_PX)][unit]
    Y, fut, valid = make_collision_inputs(d, radius, ux, uy, seed=5 + unit)
    return d, Y, fut, valid, radius, ux, uy


@pytest.mark.parametrize("shape", [(2, 8, 3, 7), (3, 1, 3, 7), (2, 256, 2, 40)])
def test_the_two_statements_agree(shape):
    d, Y, fut, valid, radius, ux, uy = _case(shape)
    f64 = collision_f64(Y, fut, valid, radius, ux, uy, d)
    assert f64["margin"] > MARGIN
    f32 = collision_f32(Y, fut, valid, radius, ux, uy, d)
    np.testing.assert_array_equal(f32["touch"], f64["touch"])
    if d.mno > 1:
        assert f64["touch"][:-1].sum() > 0 and (f64["touch"][-1] == 0).all()       # the last window has nobody in it
        assert f64["term"][0] > 0 and np.abs(f64["dY"]).max() > 0
    else:
        assert not f64["touch"].any() and not f64["col"].any() and not f64["dY"].any() and f64["term"][0] == 0
    for k in ("col", "dY", "term"):
        err = np.abs(f32[k].astype(np.float64) - f64[k]).max()
        assert err <= 64 * 2.0 ** -24 * max(np.abs(f64[k]).max(), 1e-30) * max(1, d.mno // 8), (k, err)
    assert (f64["col"][~f64["lmask"]] == 0).all()
    assert (f64["dY"].reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2)[~np.broadcast_to(f64["counted"][:, None], (d.n_scenes, d.K, d.mno, d.T_pred))] == 0).all()


def test_the_gradient_is_the_gradient():
    """Central differences of the float64 term in every coordinate of every counted position that has a partner inside the radius (and a sample of
    the others): what the device is compared to is the derivative of what it is compared to."""
    d, Y, fut, valid, radius, ux, uy = _case((2, 8, 3, 7))
    Y = np.nan_to_num(Y, nan=0.25)
    ref = collision_f64(Y, fut, valid, radius, ux, uy, d)
    G = ref["dY"]
    # float64 positions are needed for a small step: the statement reads fp32 inputs, so step in units the fp32 grid resolves exactly
    Y64 = Y.astype(np.float64)

    def term(Yp):
        return float(_f64_term(Yp, fut, valid, radius, ux, uy, d))

    idx = np.argwhere(np.abs(G) > 0)
    rest = np.argwhere(G == 0)
    rng = np.random.default_rng(0)
    pick = np.concatenate([idx[rng.permutation(len(idx))[:40]], rest[rng.permutation(len(rest))[:10]]])
    assert len(idx) >= 8
    hstep = 1e-6 / max(ux, uy)
    worst = 0.0
    for r, t, c in pick:
        Yp, Ym = Y64.copy(), Y64.copy()
        Yp[r, t, c] += hstep
        Ym[r, t, c] -= hstep
        num = (term(Yp) - term(Ym)) / (2 * hstep)
        # a coincident pair sits at the kink of dist (gradient 0 by the contract's rule): leave it out of the comparison
        err = abs(num - G[r, t, c])
        scale = max(abs(G[r, t, c]), np.abs(G).max() * 1e-3)
        if _coincident(Y64, r, t, d):
            continue
        worst = max(worst, err / scale)
    print("central differences against the float64 statement: worst relative error %.2e" % worst)
    assert worst < 1e-5


def _coincident(Y64, r, t, d):
    k_unit = r // d.mno
    rows = Y64[k_unit * d.mno:(k_unit + 1) * d.mno, t]
    same = (rows == Y64[r, t]).all(1)
    return same.sum() > 1


def _f64_term(Y64, fut, valid, radius, ux, uy, d):
    """L_col of float64 positions: the mathematics of the contract written directly (no fp32 cast of the inputs)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    c = (np.asarray(fut)[..., 0] != 0).transpose(0, 2, 1)
    nfut = c.sum(-1)
    lmask = (np.asarray(valid).reshape(n, m) != 0) & (nfut > 0)
    cc = c & lmask[:, :, None]
    P = Y64.reshape(n, K, m, T, 2)
    a = (P[:, :, :, None, :, 0] - P[:, :, None, :, :, 0]) * float(np.float32(ux))
    b = (P[:, :, :, None, :, 1] - P[:, :, None, :, :, 1]) * float(np.float32(uy))
    r = float(np.float32(radius))
    dist = np.sqrt(a * a + b * b)
    pair = cc[:, None, :, None, :] & cc[:, None, None, :, :] & ~np.eye(m, dtype=bool)[None, None, :, :, None]
    phi = np.where(pair & (dist < r), (1 - dist / r) ** 2, 0.0)
    col = phi.sum((3, 4)) / np.maximum(nfut, 1)[:, None, :]
    return (col.mean(1) * lmask).sum() / max(lmask.sum(), 1)


def test_the_direct_term_is_the_statements_term():
    d, Y, fut, valid, radius, ux, uy = _case((2, 8, 3, 7))
    Y = np.nan_to_num(Y, nan=0.25)
    ref = collision_f64(Y, fut, valid, radius, ux, uy, d)
    assert abs(_f64_term(Y.astype(np.float64), fut, valid, radius, ux, uy, d) - ref["term"][0]) <= 1e-12 * ref["term"][0]


def test_train_argument_checks():
    from desire_amd import train as T
    p = T.build_parser()
    a = p.parse_args([])
    assert a.collision_weight == 0.0 and a.collision_loss_radius is None
    T.check_recon_args(a)
    T.check_recon_args(p.parse_args(["--collision_weight", "0.5", "--collision_radius", "40"]))
    T.check_recon_args(p.parse_args(["--collision_weight", "0.5", "--collision_loss_radius", "30"]))
    for bad in (["--collision_weight", "0.5"], ["--collision_weight", "0.5", "--collision_radius", "0"], ["--collision_weight", "-1", "--collision_radius", "40"],
                ["--collision_weight", "nan", "--collision_radius", "40"], ["--collision_weight", "1", "--collision_loss_radius", "inf"]):
        with pytest.raises(ValueError):
            T.check_recon_args(p.parse_args(bad))
    terms = {"loss": 1.0, "recon": 0.5, "col": 0.25}
    a = p.parse_args(["--collision_weight", "0.5", "--collision_radius", "40", "--collision_loss_radius", "30"])
    assert T.step_line(a, 1, 2, 0, terms, 0.1).endswith(", col[r=30 w=0.5] 0.25000")
    assert T.step_line(p.parse_args([]), 1, 2, 0, terms, 0.1) == "1/2 (epoch 0), train_loss = 1.000, time/batch = 0.100"
