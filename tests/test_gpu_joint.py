"""Joint (scene-level) metrics on the device (desire_joint_metrics, csrc/kernels_joint.hip) against the numpy statements of its contract
(tests/joint_reference.py).  first, cnt and jorder are compared exactly with joint_f32 AND joint_f64 -- on inputs whose every (pair, frame) keeps,
in float64, a margin of 1e-3 r2 from r2, asserted first on the float64 pass alone.  jerr, jscore and out follow tests/test_gpu_rank.py's and
tests/test_gpu_kde.py's rule: within the harness's 1e-5 x unit of joint_f32, and against joint_f64 within four times the distance of joint_f32
from joint_f64 on the same inputs, never below 1e-5.  Then the anchors to desire_ranked_errors / desire_rank_samples, the exact boundary,
independence and reproducibility, the prediction-time form, capture, refused arguments, and the call through DESIREModel and the command line.

Observed on an MI355X (max over both units; jerr / out in units of the call, against joint_f64): see DESIGN.md section 7f."""
import ctypes as C
import itertools

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import (EVAL_FLAGS as _FLAGS, PLAIN_KEYS as _PLAIN_KEYS, walking_video as _video,
                           MISALIGNED_LONG, MISALIGNED_SHAPES, at_byte_offset, make_case, small_dims)
from tests.joint_reference import (MARGIN, RADIUS_PX, SHAPES, chunk_centres, chunk_frames, joint_f32, joint_f64, make_inputs, planted_joint_scores)
from tests.rank_reference import rank_order

pytestmark = pytest.mark.gpu
FILL, IFILL = -7.0, -77
KEYS = ("first", "cnt", "jerr", "jscore", "order", "out")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _t(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _dims(shape, **kw):
    n, m, K, T = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64, **kw)


def _units(d):
    return [(1.0, 1.0, float(np.float32(RADIUS_PX * d.sx))), (1.0 / d.sx, 1.0 / d.sy, RADIUS_PX)]      # (unit_x, unit_y, the radius in that unit)


def _hz(T):
    return sorted({max(1, T // 4), max(1, T // 2), T})


def _call(torch, h, d, Y_t, fut_t, pres_t, s_t, hz, n_top, radius, ux, uy, first=True, jerr=True, jscore=True, out=True, stream=0):
    n, K, m, nh = d.n_scenes, d.K, d.mno, len(hz)
    i32 = torch.int32
    buf = {"first": torch.full((n, K + 1, m), IFILL, device="cuda", dtype=i32) if first else None,
           "cnt": torch.full((n, K + 1, nh, 2), IFILL, device="cuda", dtype=i32),
           "jerr": torch.full((n, K, nh, 2), FILL, device="cuda") if jerr else None,
           "jscore": torch.full((n, K), FILL, device="cuda") if jscore else None,
           "order": torch.full((n, K), IFILL, device="cuda", dtype=i32),
           "out": torch.full((n, nh, 4), FILL, device="cuda") if out else None}
    ptr = lambda x: x.data_ptr() if x is not None else 0
    h.joint_metrics(Y_t.data_ptr(), ptr(fut_t), ptr(pres_t), ptr(s_t), hz, n_top, radius, ux, uy, buf["cnt"].data_ptr(), buf["order"].data_ptr(),
                    ptr(buf["first"]), ptr(buf["jerr"]), ptr(buf["jscore"]), ptr(buf["out"]), stream)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in buf.items()}


def _same_bits(a, b, keys=KEYS, rows=slice(None)):
    for key in keys:
        if a[key] is None:
            continue
        np.testing.assert_array_equal(a[key].view(np.uint32), b[key][rows].view(np.uint32), err_msg=key)


def _close(got, f32, f64, unit, what):
    """The float rule; returns (|got - f64|, |f32 - f64|) maxima.  NaNs (a NaN row is reported, not hidden) must sit where the references' do."""
    g = got.astype(np.float64)
    assert (np.isnan(g) == np.isnan(f64)).all() and (np.isnan(f32) == np.isnan(f64)).all(), what
    with np.errstate(invalid="ignore"):                                    # (an infinite joint score: inf - inf is skipped like a NaN)
        basis = float(np.nanmax(np.abs(f32.astype(np.float64) - f64), initial=0.0))
        err = float(np.nanmax(np.abs(g - f64), initial=0.0))
        near = float(np.nanmax(np.abs(g - f32.astype(np.float64)), initial=0.0))
    bar = max(4.0 * basis, 1e-5)
    print("%s: max |dev - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g; |dev - f32| = %.3g (harness %.3g)" % (what, err, basis, bar, near, 1e-5 * unit))
    assert near <= 1e-5 * unit, what
    assert err <= bar, what
    return err, basis


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_everything_matches_the_reference(torch_cuda, shape, unit):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims(shape)
    ux, uy, radius = _units(d)[unit]
    Y, fut, present, _ = make_inputs(d, radius, ux, uy, seed=5 + unit, centres=chunk_centres(d.mno, d.T_pred))
    s = planted_joint_scores(d, 9)
    hz, n_top = _hz(d.T_pred), min(d.K, 2)
    f64 = joint_f64(Y, fut, None, s, hz, n_top, radius, ux, uy, d)
    assert f64["margin"] > MARGIN                                          # the float64 pass alone, before any comparison
    f32 = joint_f32(Y, fut, None, s, hz, n_top, radius, ux, uy, d)
    h = _lib.Handle(d)
    Y_t, fut_t, s_t = _t(torch, Y), _t(torch, fut), _t(torch, s)
    got = _call(torch, h, d, Y_t, fut_t, None, s_t, hz, n_top, radius, ux, uy)
    for key in ("first", "cnt", "order"):
        np.testing.assert_array_equal(got[key], f32[key], err_msg=key)
        np.testing.assert_array_equal(got[key], f64[key], err_msg=key)
    if d.mno > 1:
        assert (got["first"][:, :d.K] < d.T_pred).any()
    if chunk_frames(d.mno, d.T_pred) < d.T_pred:                           # the chunked walk: contacts on both sides of the border and across it
        tc = chunk_frames(d.mno, d.T_pred)
        assert (got["first"][:, :d.K] < tc - 2).any() and ((got["first"][:, :d.K] >= tc) & (got["first"][:, :d.K] < d.T_pred)).any()
    m = max(ux, uy)
    _close(got["jerr"], f32["jerr"], f64["jerr"], m, "jerr")
    _close(got["out"], f32["out"], f64["out"], m, "out")
    _close(got["jscore"], f32["jscore"], f64["jscore"], 1.0, "jscore")
    np.testing.assert_array_equal(got["jscore"].view(np.uint32), f32["jscore"].view(np.uint32))      # scores on a grid of 1/64: exact sums
    # n_top = K, and NULL scores: zero joint scores, the identity order
    allk = _call(torch, h, d, Y_t, fut_t, None, s_t, hz, d.K, radius, ux, uy)
    r32 = joint_f32(Y, fut, None, s, hz, d.K, radius, ux, uy, d)
    _close(allk["out"], r32["out"], joint_f64(Y, fut, None, s, hz, d.K, radius, ux, uy, d)["out"], m, "out at n_top = K")
    _same_bits(allk, got, keys=("first", "cnt", "jerr", "jscore", "order"))
    flat = _call(torch, h, d, Y_t, fut_t, None, None, hz, n_top, radius, ux, uy)
    assert (flat["jscore"] == 0).all() and (flat["order"] == np.arange(d.K)[None]).all()
    _same_bits(flat, got, keys=("first", "cnt", "jerr"))
    h.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES + [MISALIGNED_LONG], ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_a_sample_tensor_off_16_byte_alignment(torch_cuda, shape, off):
    """The 8-byte path of the streaming loops (the error table's and the unit's) for a whole buffer, evaluation form: the references as in the parity
    test, and the aligned call's bits."""
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims(shape)
    ux, uy, radius = _units(d)[1]
    Y, fut, present, _ = make_inputs(d, radius, ux, uy, seed=6, centres=chunk_centres(d.mno, d.T_pred))
    s = planted_joint_scores(d, 9)
    hz, n_top = _hz(d.T_pred), min(d.K, 2)
    f64 = joint_f64(Y, fut, None, s, hz, n_top, radius, ux, uy, d)
    assert f64["margin"] > MARGIN
    f32 = joint_f32(Y, fut, None, s, hz, n_top, radius, ux, uy, d)
    h = _lib.Handle(d)
    Y_t, fut_t, s_t = _t(torch, Y), _t(torch, fut), _t(torch, s)
    got = _call(torch, h, d, at_byte_offset(Y_t, off), fut_t, None, s_t, hz, n_top, radius, ux, uy)
    for key in ("first", "cnt", "order"):
        np.testing.assert_array_equal(got[key], f32[key], err_msg=key)
        np.testing.assert_array_equal(got[key], f64[key], err_msg=key)
    m = max(ux, uy)
    _close(got["jerr"], f32["jerr"], f64["jerr"], m, "jerr")
    _close(got["out"], f32["out"], f64["out"], m, "out")
    _close(got["jscore"], f32["jscore"], f64["jscore"], 1.0, "jscore")
    _same_bits(got, _call(torch, h, d, Y_t, fut_t, None, s_t, hz, n_top, radius, ux, uy))
    h.close()


def _table(torch, h, d, Y_t, fut_t, hz, ux, uy):
    """desire_ranked_errors' (ADE_h, FDE_h) of every sample, through its public call: [n, K, mno, n_h, 2]."""
    tab = np.zeros((d.n_scenes, d.K, d.mno, len(hz), 2), np.float32)
    out = torch.zeros((d.A, len(hz), 4), device="cuda")
    for k in range(d.K):
        order = torch.full((d.A, d.K), k, device="cuda", dtype=torch.int32)
        h.ranked_errors(Y_t.data_ptr(), fut_t.data_ptr(), order.data_ptr(), 1, hz, ux, uy, out.data_ptr())
        torch.cuda.synchronize()
        tab[:, k] = out.cpu().numpy()[:, :, :2].reshape(d.n_scenes, d.mno, len(hz), 2)
    return tab


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[0], SHAPES[2], SHAPES[5]], ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_anchored_to_ranked_errors_and_rank_samples(torch_cuda, shape):
    """The parent's own calls, bit for bit.  At one slot per window a joint sample is the agent's sample: dev_out is desire_ranked_errors' and
    dev_jorder desire_rank_samples' (where the slot takes part: elsewhere the joint scores are empty sums, all zero).  At any mno a JADE is the
    sum of the table's rows over the slots that take part, in increasing slot, over their number."""
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims(shape)
    ux, uy, radius = _units(d)[1]
    Y, fut, present, _ = make_inputs(d, radius, ux, uy, seed=6)
    Y = np.nan_to_num(Y, nan=0.25)
    s = np.random.default_rng(3).standard_normal((d.n_scenes, d.K, d.mno)).astype(np.float32)
    if d.K >= 3:
        s[0, 2] = s[0, 0]; s[0, 1, 0] = np.nan
    hz = _hz(d.T_pred)
    h = _lib.Handle(d)
    Y_t, fut_t, s_t = _t(torch, Y), _t(torch, fut), _t(torch, s)
    got = _call(torch, h, d, Y_t, fut_t, None, s_t, hz, d.K, radius, ux, uy)
    tab = _table(torch, h, d, Y_t, fut_t, hz, ux, uy)
    part = np.stack([(fut[:, :hh, :, 0] != 0).any(1) for hh in hz], 1)      # [n, n_h, mno]
    want = np.zeros((d.n_scenes, d.K, len(hz), 2), np.float32)
    for hi in range(len(hz)):
        acc = np.zeros((d.n_scenes, d.K, 2), np.float32)
        for i in range(d.mno):
            acc = np.where(part[:, None, hi, i, None], acc + tab[:, :, i, hi], acc).astype(np.float32)
        nt = part[:, hi].sum(-1).astype(np.float32)[:, None, None]
        want[:, :, hi] = np.where(nt > 0, acc / np.maximum(nt, 1), 0)
    np.testing.assert_array_equal(got["jerr"].view(np.uint32), want.view(np.uint32))
    assert float(np.abs(want).max()) > 0
    if d.mno == 1:
        order = torch.full((d.A, d.K), IFILL, device="cuda", dtype=torch.int32)
        h.rank_samples(s_t.data_ptr(), 0, 1, order.data_ptr(), 0, 0)
        out = torch.full((d.A, len(hz), 4), FILL, device="cuda")
        h.ranked_errors(Y_t.data_ptr(), fut_t.data_ptr(), order.data_ptr(), d.K, hz, ux, uy, out.data_ptr())
        torch.cuda.synchronize()
        takes = part[:, -1, 0]
        assert takes.any() and not takes.all()
        np.testing.assert_array_equal(order.cpu().numpy(), rank_order(s, d))
        np.testing.assert_array_equal(got["order"][takes], order.cpu().numpy()[takes])
        np.testing.assert_array_equal(got["order"][~takes], np.arange(d.K)[None].repeat((~takes).sum(), 0))
        np.testing.assert_array_equal(got["out"].view(np.uint32), out.cpu().numpy().view(np.uint32))
        assert not got["out"][~takes].any() and (got["first"] == d.T_pred).all()
    h.close()


def test_the_boundary_is_exact(torch_cuda):
    """Coordinates on multiples of 1/8, partners (3/8, 4/8) apart in every frame: q = 25/64 exactly.  radius = 0.625f: r2 = 25/64, the strict
    comparison sees no contact; the next float up does.  Radius 0: nothing touches, not even a coincident pair."""
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((2, 4, 2, 6))
    rng = np.random.default_rng(3)
    Yk = np.zeros((d.n_scenes, d.K, d.mno, d.T_pred, 2), np.float32)
    Yk[:, :, 0] = rng.integers(8, 24, (d.n_scenes, d.K, d.T_pred, 2)).astype(np.float32) / 8
    Yk[:, :, 1] = Yk[:, :, 0] + np.array([3 / 8, 4 / 8], np.float32)
    Yk[:, :, 2] = Yk[:, :, 0] + np.array([40 / 8, 0], np.float32)
    Yk[:, :, 3] = Yk[:, :, 2] + np.array([-4 / 8, 3 / 8], np.float32)
    Yk[1, 1, 1] = Yk[1, 1, 0]                                              # one coincident pair: q = 0
    Y = np.ascontiguousarray(Yk.reshape(d.R, d.T_pred, 2))
    fut = np.zeros((d.n_scenes, d.T_pred, d.mno, 3), np.float32)
    fut[..., 0] = 1
    fut[..., 1:] = 50.0 * np.arange(1, d.mno + 1)[None, None, :, None]
    h = _lib.Handle(d)
    Y_t, fut_t = _t(torch, Y), _t(torch, fut)
    r0 = np.float32(0.625)
    r1 = np.nextafter(r0, np.float32(1))
    assert r0 * r0 == np.float32(25 / 64) and r1 > r0
    hz = [1, d.T_pred]
    at = _call(torch, h, d, Y_t, fut_t, None, None, hz, 1, float(r0), 1.0, 1.0)
    want = np.full((d.n_scenes, d.K, d.mno), d.T_pred, np.int32)
    want[1, 1, :2] = 0
    np.testing.assert_array_equal(at["first"][:, :d.K], want)
    up = _call(torch, h, d, Y_t, fut_t, None, None, hz, 1, float(r1), 1.0, 1.0)
    np.testing.assert_array_equal(up["first"][:, :d.K], 0)
    np.testing.assert_array_equal(up["cnt"][:, :d.K], d.mno)
    zero = _call(torch, h, d, Y_t, fut_t, None, None, hz, 1, 0.0, 1.0, 1.0)
    np.testing.assert_array_equal(zero["first"], d.T_pred)
    np.testing.assert_array_equal(zero["cnt"][..., 0], 0)
    np.testing.assert_array_equal(zero["cnt"][..., 1], d.mno)
    for r, res in ((r0, at), (r1, up), (0.0, zero)):
        ref = joint_f32(Y, fut, None, None, hz, 1, float(r), 1.0, 1.0, d)
        np.testing.assert_array_equal(res["first"], ref["first"])
        np.testing.assert_array_equal(res["cnt"], ref["cnt"])
    h.close()


def test_results_are_bitwise_reproducible_and_depend_on_the_window_alone(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    for shape in ((4, 8, 3, 7), (4, 256, 2, 40)):                          # the second one walks the frames in chunks
        d = _dims(shape)
        ux, uy, radius = _units(d)[1]
        Y, fut, present, _ = make_inputs(d, radius, ux, uy, seed=11, centres=chunk_centres(d.mno, d.T_pred))
        s = planted_joint_scores(d, 12)
        hz, n_top = _hz(d.T_pred), 2
        h = _lib.Handle(d)
        hc = _lib.Handle(d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC))
        h2 = _lib.Handle(d.replace(n_scenes=2))
        Y_t, fut_t, s_t = _t(torch, Y), _t(torch, fut), _t(torch, s)
        ref = _call(torch, h, d, Y_t, fut_t, None, s_t, hz, n_top, radius, ux, uy)
        assert (ref["first"][:, :d.K] < d.T_pred).any() and (ref["first"][:3, :d.K] == d.T_pred).any()
        _same_bits(_call(torch, h, d, Y_t, fut_t, None, s_t, hz, n_top, radius, ux, uy), ref)          # run to run
        _same_bits(_call(torch, hc, d, Y_t, fut_t, None, s_t, hz, n_top, radius, ux, uy), ref)         # the padding-skipping flags are not its business
        Yw, sw = Y.reshape(d.n_scenes, d.K * d.mno, d.T_pred, 2), s
        for lo in (0, 2):                                                  # four windows in one call = two calls of two
            two = _call(torch, h2, h2.dims, _t(torch, Yw[lo:lo + 2]), _t(torch, fut[lo:lo + 2]), None, _t(torch, sw[lo:lo + 2]), hz, n_top, radius, ux, uy)
            _same_bits(two, ref, rows=slice(lo, lo + 2))
        perm = np.array([0, 3, 1, 2])                                      # the other windows permuted: every window keeps its results
        moved = _call(torch, h, d, _t(torch, Yw[perm]), _t(torch, fut[perm]), None, _t(torch, sw[perm]), hz, n_top, radius, ux, uy)
        _same_bits(moved, {k: v[perm] for k, v in ref.items()})
        for x in (h, hc, h2):
            x.close()


def test_the_present_form_and_every_choice_of_optional_outputs(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((2, 8, 3, 7))
    ux, uy, radius = _units(d)[1]
    Y, fut, present, _ = make_inputs(d, radius, ux, uy, seed=5)
    fut = fut.copy()
    fut[..., 0] = fut[:, :1, :, 0]                                         # ids constant over t: the two forms count the same frames
    assert present.any() and not present.all()
    s = planted_joint_scores(d, 9)
    hz, n_top = _hz(d.T_pred), 2
    h = _lib.Handle(d)
    Y_t, fut_t, s_t, p_t = _t(torch, Y), _t(torch, fut), _t(torch, s), _t(torch, present)
    full = _call(torch, h, d, Y_t, fut_t, None, s_t, hz, n_top, radius, ux, uy)
    assert (full["first"][:, :d.K] < d.T_pred).any()
    pres = _call(torch, h, d, Y_t, None, p_t, s_t, hz, n_top, radius, ux, uy, jerr=False, out=False)
    ref = joint_f32(Y, None, present, s, hz, n_top, radius, ux, uy, d)
    for key in ("first", "cnt", "order"):
        np.testing.assert_array_equal(pres[key], ref[key], err_msg=key)
    np.testing.assert_array_equal(pres["first"][:, :d.K], full["first"][:, :d.K])
    np.testing.assert_array_equal(pres["cnt"][:, :d.K], full["cnt"][:, :d.K])
    np.testing.assert_array_equal(pres["first"][:, d.K], d.T_pred)         # no ground truth: row K says so
    np.testing.assert_array_equal(pres["cnt"][:, d.K], 0)
    _same_bits(pres, full, keys=("jscore", "order"))
    for first, jerr, jscore, out in itertools.product((False, True), repeat=4):
        part = _call(torch, h, d, Y_t, fut_t, None, s_t, hz, n_top, radius, ux, uy, first=first, jerr=jerr, jscore=jscore, out=out)
        _same_bits(part, full)
    for first, jscore in itertools.product((False, True), repeat=2):
        part = _call(torch, h, d, Y_t, None, p_t, s_t, hz, n_top, radius, ux, uy, first=first, jerr=False, jscore=jscore, out=False)
        _same_bits(part, pres)
    h.close()


def test_forward_and_joint_metrics_replay_from_a_graph(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=3, K=4, T_obs=8, T_pred=12, n_grids=1, mno=8, H=64, posterior=0)
    w = init_weights(d, 5)
    a, b = make_case(d, seed=21, n_absent=2), make_case(d, seed=22, n_absent=3)
    p, f, e, g = (_t(torch, x) for x in a[:4])
    h = _lib.Handle(d); h.set_weights(w); h.set_scene_grids(g.data_ptr(), a[4])
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    hz = [3, 6, 9, 12]
    i32 = torch.int32
    first = torch.zeros((d.n_scenes, d.K + 1, d.mno), device="cuda", dtype=i32); cnt = torch.zeros((d.n_scenes, d.K + 1, 4, 2), device="cuda", dtype=i32)
    jerr = torch.zeros((d.n_scenes, d.K, 4, 2), device="cuda"); js = torch.zeros((d.n_scenes, d.K), device="cuda")
    jo = torch.zeros((d.n_scenes, d.K), device="cuda", dtype=i32); out = torch.zeros((d.n_scenes, 4, 4), device="cuda")
    bufs = (Y, sc, first, cnt, jerr, js, jo, out)
    side = torch.cuda.Stream(); sp = side.cuda_stream

    def calls():
        h.forward(p.data_ptr(), 0, e.data_ptr(), Y.data_ptr(), sc.data_ptr(), sp)
        h.joint_metrics(Y.data_ptr(), f.data_ptr(), 0, sc.data_ptr(), hz, 2, 400.0, 1.0 / d.sx, 1.0 / d.sy, cnt.data_ptr(), jo.data_ptr(), first.data_ptr(),
                        jerr.data_ptr(), js.data_ptr(), out.data_ptr(), sp)

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
            assert torch.equal(x.view(i32), r.view(i32)), (rep, tag)
    assert not torch.equal(ref["a"][4], ref["b"][4]) and float(ref["a"][7].abs().max()) > 0
    ra = joint_f32(ref["a"][0].cpu().numpy(), a[1], None, ref["a"][1].cpu().numpy(), hz, 2, 400.0, 1.0 / d.sx, 1.0 / d.sy, d)
    np.testing.assert_array_equal(ref["a"][6].cpu().numpy(), ra["order"])
    np.testing.assert_array_equal(ref["a"][5].cpu().numpy().view(np.uint32), ra["jscore"].view(np.uint32))
    h.close()


def test_bad_arguments_are_refused_and_nothing_is_written(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = _dims((1, 4, 3, 6))
    h = _lib.Handle(d)
    z = torch.rand(4096, device="cuda") + 0.5
    pr = torch.ones(64, device="cuda", dtype=torch.uint8)
    i32 = torch.int32
    outs = {"first_ptr": torch.full((1, d.K + 1, d.mno), IFILL, device="cuda", dtype=i32), "cnt_ptr": torch.full((1, d.K + 1, 8, 2), IFILL, device="cuda", dtype=i32),
            "jerr_ptr": torch.full((1, d.K, 8, 2), FILL, device="cuda"), "jscore_ptr": torch.full((1, d.K), FILL, device="cuda"),
            "jorder_ptr": torch.full((1, d.K), IFILL, device="cuda", dtype=i32), "out_ptr": torch.full((1, 8, 4), FILL, device="cuda")}
    nan, inf = float("nan"), float("inf")
    cases = [(dict(yhat_ptr=0), "dev_Yhat"), (dict(cnt_ptr=0), "dev_cnt"), (dict(jorder_ptr=0), "dev_jorder"),
             (dict(horizons=[]), "n_h"), (dict(horizons=list(range(1, 10))), "n_h"), (dict(horizons=[0]), "host_horizons"), (dict(horizons=[7]), "host_horizons"),
             (dict(horizons=[3, 3]), "increasing"), (dict(horizons=[4, 2]), "increasing"),
             (dict(n_top=0), "n_top"), (dict(n_top=4), "n_top"), (dict(radius=-1e-3), "radius"), (dict(radius=nan), "radius"), (dict(radius=inf), "radius"),
             (dict(unit_x=0.0), "unit_x"), (dict(unit_x=-1.0), "unit_x"), (dict(unit_x=nan), "unit_x"), (dict(unit_x=inf), "unit_x"),
             (dict(unit_y=0.0), "unit_y"), (dict(unit_y=-2.0), "unit_y"), (dict(unit_y=nan), "unit_y"), (dict(unit_y=inf), "unit_y"),
             (dict(present_ptr=pr.data_ptr()), "both"), (dict(fut_ptr=0), "both NULL"),
             (dict(fut_ptr=0, present_ptr=pr.data_ptr()), "dev_jerr"), (dict(fut_ptr=0, present_ptr=pr.data_ptr(), jerr_ptr=0), "dev_out")]
    for kw, word in cases:
        args = dict(yhat_ptr=z.data_ptr(), fut_ptr=z.data_ptr(), present_ptr=0, score_ptr=z.data_ptr(), horizons=[2, 6], n_top=2, radius=1.0, unit_x=1.0,
                    unit_y=1.0, **{k: v.data_ptr() for k, v in outs.items()})
        args.update(kw)
        with pytest.raises(_lib.DesireError, match="error -1.*" + word):
            h.joint_metrics(**args)
    lib = _lib.load()
    one = C.c_float(1)
    hz2 = (C.c_int32 * 2)(2, 6)
    o = {k: v.data_ptr() for k, v in outs.items()}
    assert lib.desire_joint_metrics(None, z.data_ptr(), z.data_ptr(), None, None, hz2, 2, 1, one, one, one, o["first_ptr"], o["cnt_ptr"], o["jerr_ptr"],
                                    o["jscore_ptr"], o["jorder_ptr"], o["out_ptr"], None) == -1
    assert b"handle" in lib.desire_last_error()
    assert lib.desire_joint_metrics(h._h, z.data_ptr(), z.data_ptr(), None, None, None, 2, 1, one, one, one, o["first_ptr"], o["cnt_ptr"], o["jerr_ptr"],
                                    o["jscore_ptr"], o["jorder_ptr"], o["out_ptr"], None) == -1
    assert b"host_horizons" in lib.desire_last_error()
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    with pytest.raises(_lib.DesireError, match="error -1.*ref_compat"):
        rc.joint_metrics(z.data_ptr(), z.data_ptr(), 0, 0, [8], 1, 1.0, 1.0, 1.0, o["cnt_ptr"], o["jorder_ptr"])
    torch.cuda.synchronize()
    assert all(bool((v == (IFILL if v.dtype == i32 else FILL)).all()) for v in outs.values())
    # ... and the handle still works
    h.joint_metrics(z.data_ptr(), z.data_ptr(), 0, 0, [2, 6], 1, 0.0, 1.0, 1.0, o["cnt_ptr"], o["jorder_ptr"])
    torch.cuda.synchronize()
    cnt = outs["cnt_ptr"].view(-1)[:(d.K + 1) * 2 * 2].view(d.K + 1, 2, 2)            # the call's own layout: two horizons
    assert bool((outs["jorder_ptr"][0] == torch.arange(d.K, device="cuda")).all()) and bool((cnt[..., 0] == 0).all())
    assert bool((cnt[..., 1] == d.mno).all()) and bool((outs["first_ptr"] == IFILL).all()) and bool((outs["out_ptr"] == FILL).all())
    for x in (h, rc):
        x.close()


def _radius_with_a_margin(Y, counted, ux, uy, d):
    """A radius in the middle of the widest gap between the sorted distances of the counted pairs (their middle half), so that joint_f32 is a valid
    reference for samples the test did not lay out; the caller asserts the margin.  counted [n, mno, T]."""
    Yk = Y.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).astype(np.float64)
    a = (Yk[:, :, :, None, :, 0] - Yk[:, :, None, :, :, 0]) * ux
    b = (Yk[:, :, :, None, :, 1] - Yk[:, :, None, :, :, 1]) * uy
    both = (counted[:, None, :, None, :] & counted[:, None, None, :, :]) & np.triu(np.ones((d.mno, d.mno), bool), 1)[None, None, :, :, None]
    dist = np.sort(np.sqrt(a * a + b * b)[np.broadcast_to(both, a.shape)])
    dist = dist[dist > 0]
    mid = dist[len(dist) // 4: max(len(dist) // 4 + 2, 3 * len(dist) // 4)]
    i = int(np.argmax(np.diff(mid) / mid[1:]))
    return float(np.float32(0.5 * (mid[i] + mid[i + 1])))


def test_evaluate_joint_and_predict_select_joint(torch_cuda):
    torch = torch_cuda
    from desire_amd import evaluate as E
    from desire_amd.model import DESIREModel
    from desire_amd.train import split_windows
    a = E.build_parser().parse_args(_FLAGS)
    m = DESIREModel(a, seed=4)
    video = _video()
    wins = [video[i * 10 + 20:i * 10 + 30] for i in range(2)]         # the second window has lost the last object
    past, fut = split_windows(wins, a.seq_length)
    top = 3
    plain = m.predict(past, top=top, seed=3, device_rng=True)
    Y, score = m.final_output.clone(), m.final_states.clone()
    h = m._handle(2, False)
    d = h.dims
    assert sorted(plain) == ["order", "present", "score", "traj"]     # select="score": the dict it returned before
    again = m.predict(past, top=top, seed=3, device_rng=True, select="score")
    assert sorted(again) == sorted(plain) and all(torch.equal(again[k], plain[k]) for k in plain)
    Yn, sn = Y.cpu().numpy().reshape(d.R, d.T_pred, 2), score.cpu().numpy()
    futp = m._pad_windows(fut, d.mno).cpu().numpy()
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    hz = [2, 4, 6]
    # ---- evaluate_joint
    counted = (futp[..., 0] != 0).transpose(0, 2, 1)
    radius = _radius_with_a_margin(Yn, counted, ux, uy, d)
    f64 = joint_f64(Yn, futp, None, sn, hz, top, radius, ux, uy, d)
    assert f64["margin"] > MARGIN
    ref = joint_f32(Yn, futp, None, sn, hz, top, radius, ux, uy, d)
    assert (ref["first"][:, :d.K] < d.T_pred).any()
    ev = m.evaluate_joint(Y, score, fut, top=top, horizons=hz, units="px", collision_radius=radius)
    assert sorted(ev) == ["cnt", "first", "jerr", "jscore", "order", "out"]
    for key in ("first", "cnt", "order"):
        np.testing.assert_array_equal(ev[key], ref[key], err_msg=key)
    np.testing.assert_array_equal(ev["jscore"].view(np.uint32), ref["jscore"].view(np.uint32))        # the same fp32 additions in the same order
    np.testing.assert_allclose(ev["jerr"], ref["jerr"], rtol=0, atol=1e-5 / min(d.sx, d.sy))
    np.testing.assert_allclose(ev["out"], ref["out"], rtol=0, atol=1e-5 / min(d.sx, d.sy))
    none = m.evaluate_joint(Y, score, fut, top=top, horizons=hz, units="px")                            # no radius: "no contact"
    assert (none["first"] == d.T_pred).all() and (none["cnt"][..., 0] == 0).all()
    np.testing.assert_array_equal(none["jerr"].view(np.uint32), ev["jerr"].view(np.uint32))
    # ---- predict(select="joint")
    present = plain["present"].cpu().numpy()
    pr8 = present.reshape(-1).astype(np.uint8)
    r_p = _radius_with_a_margin(Yn, np.broadcast_to(present[:, :, None], (2, d.mno, d.T_pred)), ux, uy, d)
    p64 = joint_f64(Yn, None, pr8, sn, [d.T_pred], top, r_p, ux, uy, d)
    assert p64["margin"] > MARGIN
    pref = joint_f32(Yn, None, pr8, sn, [d.T_pred], top, r_p, ux, uy, d)
    out = m.predict(past, top=top, seed=3, device_rng=True, select="joint", collision_radius=r_p)
    assert sorted(out) == ["collisions", "joint_score", "order", "present", "score", "traj"]
    assert torch.equal(m.final_output, Y) and torch.equal(m.final_states, score)
    idx = pref["order"][:, :top].astype(np.int64)
    w = np.arange(2)[:, None]
    np.testing.assert_array_equal(out["order"].cpu().numpy(), np.broadcast_to(pref["order"][:, None, :], (2, d.mno, d.K)))
    assert out["order"].dtype == torch.int32 and tuple(out["traj"].shape) == (2, d.mno, top, d.T_pred, 2) and tuple(out["score"].shape) == (2, d.mno, top)
    np.testing.assert_array_equal(out["joint_score"].cpu().numpy().view(np.uint32), pref["jscore"][w, idx].view(np.uint32))
    np.testing.assert_array_equal(out["collisions"].cpu().numpy(), pref["cnt"][:, :d.K, 0, 0][w, idx])
    assert (pref["cnt"][:, :d.K, 0, 0] > 0).any()
    scale = torch.tensor([d.sx, d.sy], device="cuda", dtype=torch.float32)
    Yk = Y.reshape(2, d.K, d.mno, d.T_pred, 2)
    want = (Yk[torch.as_tensor(w, device="cuda"), torch.as_tensor(idx, device="cuda")].permute(0, 2, 1, 3, 4) / scale)
    assert torch.equal(out["traj"], want)
    np.testing.assert_array_equal(out["score"].cpu().numpy(), sn.reshape(2, d.K, d.mno)[w, idx].transpose(0, 2, 1))
    bare = m.predict(past, top=top, seed=3, device_rng=True, select="joint")
    assert int(bare["collisions"].abs().sum()) == 0 and torch.equal(bare["order"], out["order"])
    with pytest.raises(ValueError, match="collision_radius"):
        m.predict(past, collision_radius=5.0)
    with pytest.raises(ValueError, match="collision_radius"):
        m.predict(past, select="joint", collision_radius=-1.0)
    with pytest.raises(ValueError, match="select"):
        m.predict(past, select="best")


def test_the_evaluation_walk_reports_the_joint_block(torch_cuda):
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    import json
    video = _video()
    res = {}
    for tag, extra in (("plain", []), ("zero", ["--joint"]), ("wide", ["--joint", "--collision_radius", "100000"])):
        a = E.build_parser().parse_args(_FLAGS + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=DESIREModel(a, seed=4))
    assert list(res["plain"]) == _PLAIN_KEYS                           # without the flag: the result it has always been
    plain_text = json.dumps(res["plain"], indent=1)
    nh = len(res["plain"]["horizons"])
    for tag in ("zero", "wide"):
        blk = res[tag].pop("joint")
        assert json.dumps(res[tag], indent=1) == plain_text            # ... and with it, the same result plus one block
        assert set(blk) == {"collision_radius_px", "windows", "top1", "best_of_top", "collision_rate", "slots"}
        assert set(blk["collision_rate"]) == {"top1", "all_K", "ground_truth"}
        vals = blk["top1"]["jade"] + blk["top1"]["jfde"] + blk["best_of_top"]["jade"] + blk["best_of_top"]["jfde"]
        assert len(vals) == 4 * nh and np.isfinite(vals).all() and min(vals) > 0
        assert all(b <= t + 1e-12 for b, t in zip(blk["best_of_top"]["jade"], blk["top1"]["jade"]))
        assert blk["windows"] == [res["plain"]["windows"]] * nh and min(blk["slots"]) > 0
        res[tag]["joint"] = blk
    assert res["zero"]["joint"]["collision_radius_px"] == 0.0 and res["wide"]["joint"]["collision_radius_px"] == 100000.0
    assert all(v == 0.0 for k in ("top1", "all_K", "ground_truth") for v in res["zero"]["joint"]["collision_rate"][k])
    assert all(v == 1.0 for k in ("top1", "all_K", "ground_truth") for v in res["wide"]["joint"]["collision_rate"][k])      # every window holds >= 2 objects
    assert res["zero"]["joint"]["top1"] == res["wide"]["joint"]["top1"]
