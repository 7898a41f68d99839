"""CPU-side checks of the off-road penalty (desire_mask_distance, desire_set_offroad_field, desire_offroad_loss / desire_set_offroad_loss): the
LDS plan of k_offroad_unit (desire_amd/csrc/eval_lds.h: OffLds, offroad_geometry) compiled with g++ through tests/c_host/offroad_lds_driver.cpp --
no ROCm header, no GPU --, the ABI symbols and their Python binding, the separable distance field against brute force, the numpy statements
against each other and against central differences, the input generator, and train.py's argument checks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import small_dims
from tests.offroad_reference import (LDS_BYTES, MARGIN, cell_sizes, default_fos, make_masks, make_offroad_inputs, mask_field_f32,
                                     mask_field_separable_f32, off_lds_bytes, offroad_f32, offroad_f64, offroad_geometry, positive_share)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "offroad_lds_driver.cpp")
# (n_scenes, mno, K, T_pred) of tests/test_gpu_offroad_loss.py and the fields they run on
SHAPES = [(2, 8, 3, 7), (3, 1, 3, 7), (1, 32, 20, 40), (2, 160, 4, 9), (2, 256, 2, 40)]
FIELDS = [(4, 5), (64, 64), (128, 128)]
SCALE_PX = 120.0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("off_lds") / "offroad_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, reqs):
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs)
    return rows


def test_plan_fits_the_budget(driver):
    (lds, threads), = ask(driver, ["budget"])
    assert lds == LDS_BYTES and threads == 256
    cases = [(8, 7, 4, 5), (32, 40, 64, 64), (256, 40, 64, 64), (8, 7, 128, 128), (1, 7, 1024, 1024), (256, 4000, 1, 1)]
    cases += [(m, T, Mh, Mw) for _, m, _, T in SHAPES for Mh, Mw in FIELDS]
    got = dict(zip(cases, ask(driver, ["off %d %d %d %d" % c for c in cases])))
    for (m, T, Mh, Mw), (tc, staged, nbytes, end, field) in got.items():
        assert 1 <= tc <= T and nbytes == end <= lds, (m, T, Mh, Mw)
        assert (tc, bool(staged)) == offroad_geometry(m, T, Mh, Mw)                      # tests/offroad_reference.py's own statement
        assert nbytes == off_lds_bytes(m, tc, Mh * Mw if staged else 0)
        assert field % 4 == 0 and field == off_lds_bytes(m, tc, 0)                       # the field is the last region
        assert staged or off_lds_bytes(m, tc, Mh * Mw) > lds                             # global taps only where the field does not fit
    assert got[(8, 7, 4, 5)][:2] == (7, 1)
    assert got[(32, 40, 64, 64)][:3] == (40, 1, 33 * 40 * 8 + 32 * 41 * 12 + 4 * 65 + 4 * 64 * 64)
    assert got[(256, 40, 64, 64)][:2] == (11, 0)                                         # chunked, and the field stays in global memory
    assert got[(8, 7, 128, 128)][:2] == (7, 0) and got[(1, 7, 1024, 1024)][1] == 0


def test_abi_symbols_and_binding():
    import __graft_entry__ as g
    g.build()
    from desire_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "desire_hip.h")).read()
    counts = {"desire_mask_distance": 9, "desire_set_offroad_field": 6, "desire_set_offroad_loss": 3, "desire_offroad_loss": 9}
    for name, n in counts.items():
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == n, name
    for meth in ("mask_distance", "set_offroad_field", "set_offroad_loss", "offroad_loss"):
        assert callable(getattr(_lib.Handle, meth))
    # the checks that need no device: a NULL handle is refused with a text
    assert lib.desire_mask_distance(None, None, 1, 1, 1, 1.0, 1.0, None, None) == -1 and b"handle" in lib.desire_last_error()
    assert lib.desire_set_offroad_field(None, None, 1, 1, 1, None) == -1 and b"handle" in lib.desire_last_error()
    assert lib.desire_offroad_loss(None, None, None, 1.0, None, None, None, None, None) == -1 and b"handle" in lib.desire_last_error()
    assert lib.desire_set_offroad_loss(None, 1.0, 1.0) == -1 and lib.desire_last_error()


def _masks():
    rng = np.random.default_rng(7)
    out = []
    for (Mh, Mw), dens in zip([(5, 7), (16, 16), (9, 33), (24, 20)], [0.3, 0.05, 0.02, 0.5]):
        m = (rng.uniform(size=(2, Mh, Mw)) < dens).astype(np.uint8)
        m[0, Mh // 2, Mw // 2] = 1
        out.append(m)
    out += [np.zeros((1, 6, 5), np.uint8), np.ones((1, 6, 5), np.uint8), np.ones((1, 1, 1), np.uint8), np.zeros((1, 1, 1), np.uint8)]
    line = np.zeros((1, 1, 9), np.uint8)
    line[0, 0, 6] = 1
    out += [line, make_masks(2, 4, 5, 1), make_masks(1, 64, 64, 2)]
    return out


@pytest.mark.parametrize("cell", [(1.0, 1.0), (3.7, 1.3), (0.37, 7.77)])
def test_separable_field_is_the_brute_force_field(cell):
    for m in _masks():
        a, b = mask_field_f32(m, *cell), mask_field_separable_f32(m, *cell)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=str(m.shape))
        for i in range(m.shape[0]):
            if m[i].any():
                assert (a[i][m[i] != 0] == 0).all() and (a[i][m[i] == 0] > 0).all()
            else:
                assert not a[i].any()                                                    # no traversable cell: no constraint


def _case(shape=(2, 8, 3, 7), field=(4, 5), seed=8):
    n, m, K, T = shape
    d = small_dims(n_scenes=n, mno=m, K=K, T_obs=6, T_pred=T, n_grids=1)
    Mh, Mw = field
    masks = make_masks(2, Mh, Mw, seed)
    F = mask_field_f32(masks, *cell_sizes(d, Mh, Mw))
    Y, fut, valid, planted = make_offroad_inputs(d, Mh, Mw, seed)
    return d, Y, fut, valid, planted, F, default_fos(n)


@pytest.mark.parametrize("field", FIELDS, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_generator_and_the_two_statements(shape, field):
    """What the GPU test asserts on the reference before it looks at the device, and the fp32 statement against the float64 one."""
    d, Y, fut, valid, planted, F, fos = _case(shape, field)
    f64 = offroad_f64(Y, fut, valid, F, fos, SCALE_PX, d)
    share = positive_share(f64)
    assert 0.25 <= share <= 0.75, share
    assert f64["margin"][~planted].min() >= MARGIN * 0.999
    assert np.isnan(Y).sum() == 2 and (Y[..., 0] == 1.0).any() and (Y < 0).any()
    xm = Y[..., 0].astype(np.float64) * field[1] - 0.5
    assert (xm < 0).any() and (xm > field[1] - 1).any()
    f32 = offroad_f32(Y, fut, valid, F, fos, SCALE_PX, d)
    np.testing.assert_array_equal(f32["count"], f64["count"])
    assert f64["count"].sum() > 0 and f64["term"][0] > 0 and np.abs(f64["dY"]).max() > 0
    worst = 0.0
    for k in ("off", "dY", "term"):
        err = np.abs(f32[k].astype(np.float64) - f64[k]).max() / np.abs(f64[k]).max()
        worst = max(worst, err)
        # every value is a handful of fp32 operations on numbers of one sign and a sum of at most T_pred terms; the bilinear differences
        # cancel, which is where the few hundred ulps go
        assert err <= 512 * 2.0 ** -24, (k, err)
    print("fp32 statement against float64: worst relative difference %.2e (%.1f ulp)" % (worst, worst * 2.0 ** 24))
    assert (f64["off"][~f64["lmask"]] == 0).all()
    cnt = np.broadcast_to(f64["counted"][:, None], (d.n_scenes, d.K, d.mno, d.T_pred))
    assert (f64["dY"].reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2)[~cnt] == 0).all()
    if d.n_scenes >= 3:                                                                  # the window without a field, the empty window
        A = f64["off"].reshape(d.n_scenes, d.mno, d.K)
        assert not A[1].any() and not f64["count"][1].any() and f64["lmask"].reshape(d.n_scenes, d.mno)[1].any()
        assert not f64["lmask"].reshape(d.n_scenes, d.mno)[-1].any()


def test_the_gradient_is_the_gradient():
    """Central differences of the float64 term in the coordinates of counted positions kept >= 1e-3 cells from every cell line and clamp edge
    (the generator's margin): what the device is compared to is the derivative of what it is compared to."""
    d, Y, fut, valid, planted, F, fos = _case((2, 8, 3, 7), (4, 5))
    Y64 = np.nan_to_num(Y, nan=0.3).astype(np.float64)
    ref = offroad_f64(Y64, fut, valid, F, fos, SCALE_PX, d)
    G = ref["dY"]
    ok = np.broadcast_to((ref["margin"] >= MARGIN * 0.999).reshape(d.R, d.T_pred, 1), G.shape)
    idx = np.argwhere((np.abs(G) > 0) & ok)
    rest = np.argwhere((G == 0) & ok)
    assert len(idx) >= 40
    rng = np.random.default_rng(0)
    pick = np.concatenate([idx[rng.permutation(len(idx))[:60]], rest[rng.permutation(len(rest))[:20]]])
    hstep = 1e-7
    worst = 0.0
    for r, t, c in pick:
        Yp, Ym = Y64.copy(), Y64.copy()
        Yp[r, t, c] += hstep
        Ym[r, t, c] -= hstep
        num = (offroad_f64(Yp, fut, valid, F, fos, SCALE_PX, d)["term"][0] - offroad_f64(Ym, fut, valid, F, fos, SCALE_PX, d)["term"][0]) / (2 * hstep)
        worst = max(worst, abs(num - G[r, t, c]) / max(abs(G[r, t, c]), np.abs(G).max() * 1e-3))
    print("central differences against the float64 statement: worst relative error %.2e" % worst)
    assert worst < 1e-5


def test_train_argument_checks(tmp_path):
    from desire_amd import train as T
    p = T.build_parser()
    a = p.parse_args([])
    assert a.offroad_weight == 0.0 and a.offroad_scale is None and a.scene_masks is None
    T.check_recon_args(a)
    T.check_recon_args(p.parse_args(["--offroad_scale", "50"]))                          # a scale without a weight: nothing is on
    T.check_recon_args(p.parse_args(["--offroad_weight", "0.5", "--offroad_scale", "50", "--scene_masks", "m.npz"]))
    for bad, flag in ((["--offroad_weight", "0.5", "--scene_masks", "m.npz"], "--offroad_scale"),
                      (["--offroad_weight", "0.5", "--offroad_scale", "0", "--scene_masks", "m.npz"], "--offroad_scale"),
                      (["--offroad_weight", "0.5", "--offroad_scale", "inf", "--scene_masks", "m.npz"], "--offroad_scale"),
                      (["--offroad_weight", "0.5", "--offroad_scale", "50"], "--scene_masks"),
                      (["--offroad_weight", "-1", "--offroad_scale", "50", "--scene_masks", "m.npz"], "--offroad_weight"),
                      (["--offroad_weight", "nan", "--offroad_scale", "50", "--scene_masks", "m.npz"], "--offroad_weight")):
        with pytest.raises(ValueError, match=flag):
            T.check_recon_args(p.parse_args(bad))
    terms = {"loss": 1.0, "recon": 0.5, "col": 0.25, "off": 0.125}
    a = p.parse_args(["--offroad_weight", "0.5", "--offroad_scale", "50", "--scene_masks", "m.npz"])
    assert T.step_line(a, 1, 2, 0, terms, 0.1).endswith(", off[s=50 w=0.5] 0.12500")
    assert T.step_line(p.parse_args([]), 1, 2, 0, terms, 0.1) == "1/2 (epoch 0), train_loss = 1.000, time/batch = 0.100"
    # the mask file
    good = str(tmp_path / "m.npz")
    np.savez(good, **{"a/v0": np.ones((4, 5), np.uint8), "a/v1": np.zeros((4, 5), np.uint8)})
    masks, mov = T.load_scene_masks(good, ["a/v1", "a/v0", "a/v1"])
    assert masks.shape == (2, 4, 5) and masks.dtype == np.uint8 and mov.tolist() == [1, 0, 1] and masks[0].all() and not masks[1].any()
    with pytest.raises(ValueError, match="--scene_masks"):
        T.load_scene_masks(good, ["a/v2"])
    bad = str(tmp_path / "b.npz")
    np.savez(bad, **{"a/v0": np.ones((4, 5), np.uint8), "a/v1": np.zeros((5, 4), np.uint8)})
    with pytest.raises(ValueError, match="--scene_masks"):
        T.load_scene_masks(bad, ["a/v0"])
