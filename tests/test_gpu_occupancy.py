"""Predicted occupancy maps on the device (desire_occupancy, csrc/kernels_occ.hip) against the numpy statements of its contract
(tests/occupancy_reference.py).  The generator plants: two samples of one agent in one cell; two and three agents in one cell; a sample that
leaves a cell and returns; positions exactly on a cell edge at dyadic coordinates; x = 1.0 exactly; negatives; a NaN row; an uncounted frame in
the middle of a track; an absent slot; an empty window; a masked cell that is visited and one that is not.  Every other coordinate keeps
EDGE_MARGIN from a cell edge (tests/test_occupancy_cpu.py asserts that, and the generator's three fractions, on float64 alone).

With NULL scores, and with scores drawn from {0, -200} (expf(-200) is exactly 0 in fp32: the weights are 1.f / n or 0 in either implementation),
every output equals occupancy_f32 bit for bit.  With generic scores the weights go through the device's expf: the outputs are held to
occupancy_f64 within four times the distance of occupancy_f32 from occupancy_f64 on the same inputs, never below 1e-6 * max(1, max E).
Then the bitwise checks: run to run, the batch, permuted windows, DESIRE_FLAG_COMPACT_*, a banded grid against another cut, every choice of
NULL outputs, AT against UNTIL at h = 1, the two counting forms, refused arguments, capture; and the calls through DESIREModel and evaluate.py.

The banded case: rows 0 .. 47 of the 96 x 96 grid are the rows of a 48 x 96 grid over the same frame with y doubled (2 y * 48 and y * 96 are one
real number, rounded once either way), and the two grids are cut into bands differently (2 x 48 / 3 x 32 rows against 1 x 48 / 2 x 24).

Observed on an MI355X against occupancy_f64, generic scores: see DESIGN.md section 7h."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import PLAIN_KEYS as _PLAIN_KEYS, at_byte_offset, make_case, small_dims
from tests.occupancy_reference import AT, SEEDS, SHAPES, UNTIL, band_rows, constant_ids, make_inputs, occupancy_f32, occupancy_f64

pytestmark = pytest.mark.gpu
FILL = -7.0
KEYS = ("occ", "exp", "hit", "viol", "off")
IDS = lambda s: "n%d_m%d_K%d_T%d_%dx%d" % (s[:4] + s[4])
MODES = pytest.mark.parametrize("mode", [AT, UNTIL], ids=["at", "until"])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _t(torch, a):
    return torch.as_tensor(np.array(a), device="cuda")                 # (a copy: the shared inputs are read-only)


def _dims(shape, **kw):
    n, m, K, T = shape[:4]
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64, **kw)


def _hz(T):
    return sorted({1, max(1, T // 2), T})


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(Y, fut, present, mask, mask_of_scene) of a shape: generated once, shared, never modified."""
    out = make_inputs(_dims(shape), shape[4], SEEDS.get(shape, 3))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _scores(shape, kind):
    d = _dims(shape)
    rng = np.random.default_rng(17)
    if kind == "none":
        return None
    s = (rng.choice([0.0, -200.0], d.R) if kind == "onoff" else rng.standard_normal(d.R) * 2).astype(np.float32)
    if kind == "onoff":
        s.reshape(d.n_scenes, d.K, d.mno)[:, 0, 0] = 0                    # (an agent whose scores are all -200 weighs uniformly: also exact)
    if kind == "generic" and d.K > 1 and d.mno > 1:
        s.reshape(d.n_scenes, d.K, d.mno)[0, 1, 1] = np.nan               # a non-finite score: that agent weighs uniformly
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _reference(shape, form, mode, kind, prec):
    d = _dims(shape)
    Y, fut, present, mask, mos = _inputs(shape)
    fn = occupancy_f32 if prec == 32 else occupancy_f64
    return fn(Y, fut if form == "fut" else None, present if form == "present" else None, _scores(shape, kind), _hz(d.T_pred), mode, shape[4], mask,
              mos, d)


def _call(torch, h, d, grid, Y_t, fut_t, pres_t, s_t, hz, mode, mask_t=None, mos_t=None, exp=True, hit=None, viol=None, off=True, stream=0):
    n, nh = d.n_scenes, len(hz)
    hit = (fut_t is not None and mode == AT) if hit is None else hit
    viol = (mask_t is not None) if viol is None else viol
    buf = {"occ": torch.full((n, nh) + tuple(grid), FILL, device="cuda"), "exp": torch.full((n, nh) + tuple(grid), FILL, device="cuda") if exp else None,
           "hit": torch.full((d.A, nh), FILL, device="cuda") if hit else None, "viol": torch.full((d.A, nh), FILL, device="cuda") if viol else None,
           "off": torch.full((d.A, nh), FILL, device="cuda") if off else None}
    ptr = lambda x: x.data_ptr() if x is not None else 0
    h.occupancy(Y_t.data_ptr(), ptr(fut_t), ptr(pres_t), ptr(s_t), hz, mode, grid[0], grid[1], buf["occ"].data_ptr(), ptr(buf["exp"]), ptr(buf["hit"]),
                ptr(buf["viol"]), ptr(buf["off"]), ptr(mask_t), ptr(mos_t), stream)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in buf.items()}


def _same_bits(a, b, keys=KEYS, rows=None):
    """a's outputs (those it has) equal b's bit for bit; rows = (window slice, mno): b is a batch that a is a part of."""
    for key in keys:
        if a[key] is None:
            continue
        want = b[key]
        if rows is not None:
            sl, m = rows
            want = want[sl] if key in ("occ", "exp") else want[sl.start * m:sl.stop * m]
        np.testing.assert_array_equal(a[key].view(np.uint32), want.view(np.uint32), err_msg=key)


def _run(torch, shape, form, mode, kind, h=None, **kw):
    d = _dims(shape)
    Y, fut, present, mask, mos = _inputs(shape)
    from desire_amd import _lib
    own = h is None
    h = h or _lib.Handle(d)
    s = _scores(shape, kind)
    got = _call(torch, h, d, shape[4], _t(torch, Y), _t(torch, fut) if form == "fut" else None, _t(torch, present) if form == "present" else None,
                _t(torch, s) if s is not None else None, _hz(d.T_pred), mode, _t(torch, mask), _t(torch, mos), **kw)
    if own:
        h.close()
    return got


@pytest.mark.parametrize("form", ["fut", "present"])
@MODES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_output_equals_the_fp32_statement(torch_cuda, shape, mode, form):
    for kind in ("none", "onoff"):
        got = _run(torch_cuda, shape, form, mode, kind)
        ref = _reference(shape, form, mode, kind, 32)
        for key in KEYS:
            if ref[key] is None:
                assert got[key] is None and key == "hit"
                continue
            np.testing.assert_array_equal(got[key], ref[key], err_msg="%s %s" % (key, kind))
        assert ref["exp"].max() > 0
        if kind == "none":
            assert ref["off"].max() > 0 and ref["viol"].max() > 0 and (ref["hit"] is None or ref["hit"].max() > 0)


# horizons beyond the issue's shapes: more frames than a wave has lanes, and more than one chunk of the LDS plan holds (512: a sample's frames then
# arrive in two chunks, and its flags and its stamp span both)
LONG = [(1, 4, 2, 70, (4, 4)), (1, 2, 2, 600, (4, 4))]


@pytest.mark.parametrize("form", ["fut", "present"])
@pytest.mark.parametrize("shape", LONG, ids=IDS)
def test_long_horizons_equal_the_fp32_statement(torch_cuda, shape, form):
    for mode in (AT, UNTIL):
        got = _run(torch_cuda, shape, form, mode, "onoff")
        ref = _reference(shape, form, mode, "onoff", 32)
        for key in KEYS:
            if ref[key] is not None:
                np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
        assert ref["exp"].max() > 0 and ref["off"].max() > 0


@MODES
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_generic_scores_against_float64(torch_cuda, shape, mode):
    got = _run(torch_cuda, shape, "fut", mode, "generic")
    f32, f64 = _reference(shape, "fut", mode, "generic", 32), _reference(shape, "fut", mode, "generic", 64)
    floor = 1e-6 * max(1.0, float(f64["exp"].max()))
    for key in KEYS:
        if f64[key] is None:
            continue
        basis = float(np.abs(f32[key].astype(np.float64) - f64[key]).max())
        err = float(np.abs(got[key].astype(np.float64) - f64[key]).max())
        bar = max(4.0 * basis, floor)
        print("%s: max |dev - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g" % (key, err, basis, bar))
        assert err <= bar, key
        np.testing.assert_array_equal(got[key] > 0, f64[key] > 0, err_msg=key)


@pytest.mark.parametrize("off", [8, 4])
def test_a_sample_tensor_off_16_byte_alignment(torch_cuda, off):
    torch = torch_cuda
    from desire_amd import _lib
    for shape in (SHAPES[0], SHAPES[1]):
        d = _dims(shape)
        Y, fut, present, mask, mos = _inputs(shape)
        h = _lib.Handle(d)
        for mode in (AT, UNTIL):
            got = _call(torch, h, d, shape[4], at_byte_offset(_t(torch, Y), off), _t(torch, fut), None, None, _hz(d.T_pred), mode, _t(torch, mask), _t(torch, mos))
            _same_bits(got, _reference(shape, "fut", mode, "none", 32))
        h.close()


def test_results_are_bitwise_reproducible_and_depend_on_the_window_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    shape = (4, 8, 3, 7, (4, 5))
    d = _dims(shape)
    Y, fut, present, mask, mos = _inputs(shape)
    s = _scores(shape, "generic")
    hz = _hz(d.T_pred)
    h = _lib.Handle(d)
    hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
    h2 = _lib.Handle(d.replace(n_scenes=2))
    Yw, sw = Y.reshape(d.n_scenes, d.K * d.mno, d.T_pred, 2), s.reshape(d.n_scenes, d.K * d.mno)
    for mode in (AT, UNTIL):
        args = lambda idx: (_t(torch, Yw[idx]), _t(torch, fut[idx]), None, _t(torch, sw[idx]), hz, mode, _t(torch, mask), _t(torch, mos[idx]))
        every = slice(0, 4)
        ref = _call(torch, h, d, shape[4], *args(every))
        assert ref["exp"].max() > 0
        _same_bits(_call(torch, h, d, shape[4], *args(every)), ref)                     # run to run
        _same_bits(_call(torch, hc, d, shape[4], *args(every)), ref)                    # the padding-skipping flags are not its business
        for lo in (0, 2):                                                              # four windows in one call = two calls of two
            _same_bits(_call(torch, h2, h2.dims, shape[4], *args(slice(lo, lo + 2))), ref, rows=(slice(lo, lo + 2), d.mno))
        perm = np.array([2, 0, 3, 1])                                                  # permuted windows: every window keeps its results
        moved = _call(torch, h, d, shape[4], *args(perm))
        A = np.arange(d.A).reshape(d.n_scenes, d.mno)[perm].reshape(-1)
        _same_bits(moved, {k: (None if v is None else (v[perm] if k in ("occ", "exp") else v[A])) for k, v in ref.items()})
    for x in (h, hc, h2):
        x.close()


@MODES
def test_a_banded_grid_has_the_bits_of_another_cut(torch_cuda, mode):
    torch = torch_cuda
    from desire_amd import _lib
    shape = SHAPES[4]
    d, hz = _dims(shape), _hz(_dims(shape).T_pred)
    until = mode == UNTIL
    frames = hz[-1] if until else 1
    bands = lambda Oh: -(-Oh // band_rows(d.K, frames, Oh, 96, until))
    assert bands(96) > 1 and bands(96) != bands(48)
    Y, fut, present, mask, mos = _inputs(shape)
    Y2 = Y.copy(); Y2[..., 1] *= 2                                                   # exact
    h = _lib.Handle(d)
    full = _call(torch, h, d, (96, 96), _t(torch, Y), _t(torch, fut), None, None, hz, mode, hit=False)
    half = _call(torch, h, d, (48, 96), _t(torch, Y2), _t(torch, fut), None, None, hz, mode, hit=False)
    assert full["exp"][:, :, :48].max() > 0 and full["exp"][:, :, 48:].max() > 0     # mass on both sides of the border
    for key in ("occ", "exp"):
        np.testing.assert_array_equal(full[key][:, :, :48].view(np.uint32), half[key].view(np.uint32), err_msg=key)
    h.close()


def test_every_choice_of_optional_outputs_and_the_two_forms(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    shape = SHAPES[0]
    d, hz = _dims(shape), _hz(_dims(shape).T_pred)
    Y, fut, present, mask, mos = _inputs(shape)
    s = _scores(shape, "generic")
    fc, pc = constant_ids(fut)
    h = _lib.Handle(d)
    Y_t, s_t, m_t, o_t = _t(torch, Y), _t(torch, s), _t(torch, mask), _t(torch, mos)
    for mode in (AT, UNTIL):
        full = _call(torch, h, d, shape[4], Y_t, _t(torch, fut), None, s_t, hz, mode, m_t, o_t)
        for exp, hit, viol, off in itertools.product((False, True), repeat=4):
            if hit and mode == UNTIL:
                continue
            part = _call(torch, h, d, shape[4], Y_t, _t(torch, fut), None, s_t, hz, mode, m_t if viol else None, o_t if viol else None, exp=exp, hit=hit,
                         viol=viol, off=off)
            _same_bits(part, full)
        # the prediction form equals the evaluation form on constant ids
        ev = _call(torch, h, d, shape[4], Y_t, _t(torch, fc), None, s_t, hz, mode, m_t, o_t, hit=False)
        pr = _call(torch, h, d, shape[4], Y_t, None, _t(torch, pc), s_t, hz, mode, m_t, o_t)
        _same_bits(pr, ev)
        assert ev["exp"].max() > 0
    # AT at h = 1 is UNTIL at h = 1
    a = _call(torch, h, d, shape[4], Y_t, _t(torch, fut), None, s_t, [1], AT, m_t, o_t, hit=False)
    u = _call(torch, h, d, shape[4], Y_t, _t(torch, fut), None, s_t, [1], UNTIL, m_t, o_t)
    _same_bits(u, a)
    assert a["exp"].max() > 0
    h.close()


def test_forward_rank_and_occupancy_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=4, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    a, b = make_case(d, seed=21, n_absent=2), make_case(d, seed=22, n_absent=3)
    p, f, e, g = (_t(torch, x) for x in a[:4])
    h = _lib.Handle(d); h.set_weights(w); h.set_scene_grids(g.data_ptr(), a[4])
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    hz, grid = [3, 6, 9, 12], (12, 16)
    order = torch.zeros((d.A, d.K), device="cuda", dtype=torch.int32)
    occ = torch.zeros((d.n_scenes, 4) + grid, device="cuda"); ex = torch.zeros_like(occ)
    hit = torch.zeros((d.A, 4), device="cuda"); off = torch.zeros_like(hit)
    bufs = (Y, sc, order, occ, ex, hit, off)
    side = torch.cuda.Stream(); sp = side.cuda_stream

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.rank_samples(sc.data_ptr(), 0, 1, order.data_ptr(), 0, 0, sp)
        h.occupancy(Y.data_ptr(), f.data_ptr(), 0, sc.data_ptr(), hz, AT, grid[0], grid[1], occ.data_ptr(), ex.data_ptr(), hit.data_ptr(), 0, off.data_ptr(),
                    0, 0, sp)

    torch.cuda.synchronize()
    ref = {}
    for tag, case in (("b", b), ("a", a)):                        # eager calls (the first also warms lazy allocations up outside capture)
        p.copy_(_t(torch, case[0])); f.copy_(_t(torch, case[1])); e.copy_(_t(torch, case[2]))
        torch.cuda.synchronize()
        calls()
        side.synchronize()
        ref[tag] = [x.clone() for x in bufs]
    h.graph_begin(sp)
    calls()
    gid = h.graph_end(sp)
    for rep in range(4):
        tag, case = ("b", b) if rep % 2 == 0 else ("a", a)
        p.copy_(_t(torch, case[0])); f.copy_(_t(torch, case[1])); e.copy_(_t(torch, case[2]))      # in place: the graph keeps its pointers
        for x in bufs:
            x.zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        for x, r in zip(bufs, ref[tag]):
            assert torch.equal(x.view(torch.int32), r.view(torch.int32)), (rep, tag)
    assert not torch.equal(ref["a"][0], ref["b"][0]) and (float(ref["a"][4].max()) > 0 or float(ref["a"][6].max()) > 0)
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((1, 4, 3, 6))
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") * 0.9
    pr = torch.ones(64, device="cuda", dtype=torch.uint8)
    mk = torch.ones(64, device="cuda", dtype=torch.uint8)
    mo = torch.zeros(4, device="cuda", dtype=torch.int32)
    outs = {"occ_ptr": torch.full((1, 8, 4, 4), FILL, device="cuda"), "exp_ptr": torch.full((1, 8, 4, 4), FILL, device="cuda"),
            "hit_ptr": torch.full((4, 8), FILL, device="cuda"), "viol_ptr": torch.full((4, 8), FILL, device="cuda"), "off_ptr": torch.full((4, 8), FILL, device="cuda")}
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(occ_ptr=0), "dev_occ"),
             (dict(horizons=[]), "n_h"), (dict(horizons=list(range(1, 10))), "n_h"), (dict(horizons=[0]), "host_horizons"), (dict(horizons=[7]), "host_horizons"),
             (dict(horizons=[3, 3]), "increasing"), (dict(horizons=[4, 2]), "increasing"),
             (dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(Oh=0), "Oh"), (dict(Oh=1025), "Oh"), (dict(Ow=0), "Ow"), (dict(Ow=1025), "Ow"),
             (dict(present_ptr=pr.data_ptr()), "both"), (dict(fut_ptr=0), "both NULL"),
             (dict(fut_ptr=0, present_ptr=pr.data_ptr()), "dev_hit"), (dict(mode=UNTIL), "dev_hit"),
             (dict(mask_ptr=0), "dev_viol"), (dict(mask_of_scene_ptr=0), "dev_viol")]
    for kw, word in cases:
        args = dict(yhat_ptr=z.data_ptr(), fut_ptr=z.data_ptr(), present_ptr=0, score_ptr=z.data_ptr(), horizons=[2, 6], mode=AT, Oh=4, Ow=4,
                    mask_ptr=mk.data_ptr(), mask_of_scene_ptr=mo.data_ptr(), **{k: v.data_ptr() for k, v in outs.items()})
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.occupancy(**args)
    lib = _lib.load()
    hz2 = (C.c_int32 * 2)(2, 6)
    o = {k: v.data_ptr() for k, v in outs.items()}
    assert lib.desire_occupancy(None, z.data_ptr(), z.data_ptr(), None, None, hz2, 2, 0, 4, 4, None, None, o["occ_ptr"], o["exp_ptr"], o["hit_ptr"], None,
                                o["off_ptr"], None) == -1
    assert b"handle" in lib.desire_last_error()
    assert lib.desire_occupancy(h._h, z.data_ptr(), z.data_ptr(), None, None, None, 2, 0, 4, 4, None, None, o["occ_ptr"], o["exp_ptr"], o["hit_ptr"], None,
                                o["off_ptr"], None) == -1
    assert b"host_horizons" in lib.desire_last_error()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.occupancy(z.data_ptr(), z.data_ptr(), 0, 0, [8], AT, 4, 4, o["occ_ptr"])
    torch.cuda.synchronize()
    assert all(bool((v == FILL).all()) for v in outs.values())
    # ... and the handle still works
    h.occupancy(z.data_ptr(), 0, pr.data_ptr(), 0, [2, 6], UNTIL, 4, 4, o["occ_ptr"], o["exp_ptr"])
    torch.cuda.synchronize()
    E = outs["exp_ptr"].view(-1)[:2 * 16].view(2, 16)                                   # the call's own layout: two horizons
    assert float(E.sum(1).min()) > 0 and float(E.sum(1).max()) <= 6 * d.mno + 1e-5 and bool((outs["hit_ptr"] == FILL).all())
    for x in (h, rc):
        x.close()


_FLAGS = ["--batch_size", "2", "--seq_length", "8", "--pred_length", "12", "--max_num_obj", "32", "--d_dim", "64", "--latent_size", "64",
          "--num_samples", "5", "--neighborhood_size", "200", "--max_windows", "2", "--device_rng", "--seed", "3", "--checkpoint", "none.npz", "--units", "norm"]
_GRID = (9, 12)


def _bookstore():
    """The 160 preprocessed frames of bookstore/video6 kept as a loader golden: [160, 32, 3] = (id, x_px, y_px), zero rows = absent."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loader_bookstore6_T8.npz"))
    return z["data0"].astype(np.float32)


def _args(extra=()):
    from desire_amd import evaluate as E
    a = E.build_parser().parse_args(_FLAGS + list(extra))
    a.img_width, a.img_height = 1424.0, 1088.0                        # bookstore frame size (pixels -> normalised units)
    return a


def test_predict_and_evaluate_occupancy_on_the_bookstore_windows(torch_cuda):
    """Through DESIREModel on real windows.  The device and occupancy_f32 round x * Ow the same way, so with uniform weights every output is
    the reference's bit for bit whatever the coordinates; with the score weights (the device's expf) it is within 1e-5."""
    torch = torch_cuda
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    a = _args()
    m = DESIREModel(a, seed=4)
    video = _bookstore()
    past, fut = split_windows([video[i * 20:i * 20 + 20] for i in range(2)], a.seq_length)
    h = m._handle(2, False)
    d = h.dims
    pd = m._pad_windows(past, d.mno)
    hz = [3, 6, 12]
    mask = np.ones((1,) + _GRID, np.uint8)
    mask[0, :, ::2] = 0                                               # every other column is closed
    mos = np.zeros(2, np.int32)
    for mode, mid in (("at", AT), ("until", UNTIL)):
        out = m.predict_occupancy(pd, _GRID, horizons=hz, mode=mode, weights="uniform", mask=mask, seed=3, device_rng=True)
        assert sorted(out) == ["expected", "occ", "off", "present", "violation"]
        Yn, sn = m.final_output.cpu().numpy().reshape(d.R, d.T_pred, 2), m.final_states.cpu().numpy().reshape(-1)
        pres = out["present"].cpu().numpy().reshape(-1).astype(np.uint8)
        assert pres.any() and not pres.all()
        ref = occupancy_f32(Yn, None, pres, None, hz, mid, _GRID, mask, mos, d)
        for key, rk in (("occ", "occ"), ("expected", "exp"), ("off", "off"), ("violation", "viol")):
            np.testing.assert_array_equal(out[key].cpu().numpy().reshape(ref[rk].shape), ref[rk], err_msg=key)
        assert ref["exp"].max() > 0 and ref["viol"].max() > 0
        scored = m.predict_occupancy(pd, _GRID, horizons=hz, mode=mode, seed=3, device_rng=True)
        assert sorted(scored) == ["expected", "occ", "off", "present"]
        assert np.array_equal(m.final_output.cpu().numpy().reshape(Yn.shape), Yn)
        rs = occupancy_f32(Yn, None, pres, sn, hz, mid, _GRID, None, None, d)
        for key, rk in (("occ", "occ"), ("expected", "exp"), ("off", "off")):
            np.testing.assert_allclose(scored[key].cpu().numpy().reshape(rs[rk].shape), rs[rk], rtol=0, atol=1e-5, err_msg=key)
        # the evaluation form, with the futures
        futp = m._pad_windows(fut, d.mno).cpu().numpy()
        ev = m.evaluate_occupancy(m.final_output, m.final_states, fut, _GRID, horizons=hz, mode=mode, weights="uniform", mask=mask)
        assert sorted(ev) == sorted(["expected", "occ", "off", "violation"] + (["hit"] if mode == "at" else []))
        re_ = occupancy_f32(Yn, futp, None, None, hz, mid, _GRID, mask, mos, d)
        for key, rk in (("occ", "occ"), ("expected", "exp"), ("off", "off"), ("violation", "viol")) + ((("hit", "hit"),) if mode == "at" else ()):
            np.testing.assert_array_equal(ev[key].reshape(re_[rk].shape), re_[rk], err_msg=key)
    with pytest.raises(ValueError, match="mode"):
        m.predict_occupancy(pd, _GRID, mode="sweep")
    with pytest.raises(ValueError, match="weights"):
        m.predict_occupancy(pd, _GRID, weights="softmax")
    with pytest.raises(ValueError, match="mask"):
        m.predict_occupancy(pd, _GRID, mask=np.ones((3, 3), np.uint8))


@pytest.mark.parametrize("mode", ["at", "until"])
def test_the_evaluation_walk_reports_the_occupancy_block(torch_cuda, mode):
    import json
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    video = _bookstore()
    res = {}
    for tag, extra in (("plain", []), ("occ", ["--occupancy", "%dx%d" % _GRID, "--occupancy_mode", mode])):
        a = _args(extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        model = DESIREModel(a, seed=4)
        res[tag] = E.evaluate(a, data_loader=dl, model=model)
    assert list(res["plain"]) == _PLAIN_KEYS                           # without the flag: the result it has always been
    blk = res["occ"].pop("occupancy")
    assert json.dumps(res["occ"], indent=1) == json.dumps(res["plain"], indent=1)      # ... and with it, the same result plus one block
    assert set(blk) == {"grid", "mode", "weights", "hit_floor", "agents_at_frame", "hit_nll", "off_mass", "expected_in_frame"}
    assert blk["grid"] == list(_GRID) and blk["mode"] == mode
    # the block from the reference: one batch of two windows, whose samples and scores the model still holds
    hz = res["plain"]["horizons"]
    xs, _ = next(E.iter_batches(dl, 2, 2))
    past, fut = split_windows(xs, a.seq_length)
    d = model._handle(2, False).dims
    Yn, sn = model.final_output.cpu().numpy().reshape(d.R, d.T_pred, 2), model.final_states.cpu().numpy().reshape(-1)
    futp = model._pad_windows(fut, d.mno).cpu().numpy()
    ref = occupancy_f32(Yn, futp, None, sn, hz, UNTIL if mode == "until" else AT, _GRID, None, None, d)
    hit = occupancy_f32(Yn, futp, None, sn, hz, AT, _GRID, None, None, d)["hit"].astype(np.float64)
    valid = (np.stack(past)[:, -1, :, 0] != 0).reshape(-1)
    seen = (futp[..., 0] != 0).transpose(0, 2, 1).reshape(d.A, d.T_pred)
    for i, hh in enumerate(hz):
        at, c = valid & seen[:, hh - 1], valid & seen[:, :hh].any(1)
        assert blk["agents_at_frame"][i] == int(at.sum()) > 0 and res["plain"]["agents"][i] == int(c.sum())
        np.testing.assert_allclose(blk["hit_nll"][i], -np.log(np.maximum(hit[at, i], 1e-6)).mean(), rtol=1e-4)
        np.testing.assert_allclose(blk["off_mass"][i], ref["off"].astype(np.float64)[c, i].mean(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(blk["expected_in_frame"][i], ref["exp"].astype(np.float64)[:, i].sum() / 2, rtol=1e-5)
    assert max(blk["expected_in_frame"]) > 0
    with pytest.raises(ValueError, match="occupancy"):
        E.parse_grid("64")
