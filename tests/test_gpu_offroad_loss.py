"""The off-road penalty on the device (desire_mask_distance, desire_set_offroad_field, desire_offroad_loss, desire_set_offroad_loss;
csrc/kernels_offroad.hip) against the numpy statements of its contracts and float64 autograd of the rebuilt loss (tests/offroad_reference.py).
Shapes are (n_scenes, mno, K, T_pred) on small_dims(T_obs=6, n_grids=1).

Observed on one MI355X: every field and every output of the op has the fp32 statement's bits, which lie within 45 ulp of the largest float64
entry; training gradients within 1.7e-5 of float64 autograd (bar 2e-4) with the term carrying 1.18 - 1.38 of |d loss / d head/w| (0.77 next to
the collision term); compacted against padded step 1.2e-6; 40 Adam steps, (L_off, count): (0.334, 453) -> (0.283, 696) with the term, ->
(5.325, 861) without."""
import functools

import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.collision_reference import AGENT, MEAN, SCENE, SOFTMIN
from tests.helpers import MISALIGNED_SHAPES, at_byte_offset, make_case, small_dims, to_oracle_layout
from tests.offroad_reference import (MARGIN, cell_sizes, default_fos, make_masks, make_offroad_inputs, mask_field_f32, offroad_f32, offroad_f64,
                                     offroad_geometry, offroad_loss_and_grads, positive_share)
from tests.test_gpu_collision_loss import _bits, _op_handle
from tests.test_gpu_recon_loss import TAU, _check_done_gradients, _dims, _grads, _step, _t, _training_handle, _weights

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 3, 7),                 # the plain case, odd T_pred
          (3, 1, 3, 7),                 # one slot; a window without a field, an empty window
          (1, 32, 20, 40),              # the headline's per-window shape
          (2, 160, 4, 9),               # more slots than lanes per frame
          (2, 256, 2, 40)]              # the frame-chunked walk (11 + 11 + 11 + 7 frames): no field fits next to it
FIELDS = [(4, 5), (64, 64), (128, 128)]     # staged; staged except next to 256 slots; never staged
SCALE_PX = 120.0
SEED = 8
ERR_STATE = -2                                  # DESIRE_ERR_STATE


# ---- 1. the distance field -----------------------------------------------------------------------------------------------------------------------
def _field_masks(tag):
    rng = np.random.default_rng(11)
    if tag == "1x1":
        return np.ones((1, 1, 1), np.uint8), (2.5, 0.75)
    if tag == "5x7":                                                        # anisotropic cells; the second mask is empty
        m = (rng.uniform(size=(2, 5, 7)) < 0.3).astype(np.uint8)
        m[1] = 0
        return m, (3.7, 1.3)
    if tag == "16x16":                                                      # 5 % traversable
        return (rng.uniform(size=(1, 16, 16)) < 0.05).astype(np.uint8), (1.0, 1.0)
    if tag == "9x33":
        return (rng.uniform(size=(1, 9, 33)) < 0.1).astype(np.uint8), (0.37, 7.77)
    if tag == "70x130":                                                     # more than one workgroup's worth of columns is 3x1024's; the second mask is full
        m = make_masks(2, 70, 130, 3)
        m[1] = 1
        return m, (10.77, 15.71)
    m = (rng.uniform(size=(1, 3, 1024)) < 0.1).astype(np.uint8)             # "3x1024": the longest row, four column blocks
    m[0, :, 300:700] = 0
    return m, (1.0, 2.0)


FIELD_TAGS = ["1x1", "5x7", "16x16", "9x33", "70x130", "3x1024"]


@functools.lru_cache(maxsize=None)
def _field_reference(tag):
    m, cell = _field_masks(tag)
    return m, cell, mask_field_f32(m, *cell)


def _any_handle():
    from desire_amd import _lib
    d = _dims((1, 1, 1, 7))
    h = _lib.Handle(d)
    h.set_weights(init_weights(d, 41))
    return h


def _device_field(h, masks, cell, fill=-7.0):
    import torch
    m_t = _t(masks)
    f_t = torch.full(masks.shape, fill, device="cuda", dtype=torch.float32)
    h.mask_distance(m_t.data_ptr(), masks.shape[0], masks.shape[1], masks.shape[2], cell[0], cell[1], f_t.data_ptr())
    torch.cuda.synchronize()
    return f_t


@pytest.mark.parametrize("tag", FIELD_TAGS)
def test_field_is_the_brute_force_statement(tag):
    masks, cell, ref = _field_reference(tag)
    h = _any_handle()
    a = _device_field(h, masks, cell).cpu().numpy()
    b = _device_field(h, masks, cell, fill=3.0).cpu().numpy()
    np.testing.assert_array_equal(_bits(a), _bits(ref))
    np.testing.assert_array_equal(_bits(a), _bits(b))                       # run to run, whatever the buffer held
    for i in range(masks.shape[0]):
        if not masks[i].any():
            assert not a[i].any()                                           # no traversable cell: no constraint
    h.close()


def test_field_refusals_leave_the_output_untouched():
    import torch
    h = _any_handle()
    lib = h.lib
    m = _t(np.ones((2, 4, 5), np.uint8))
    f = torch.full((2, 4, 5), -7.0, device="cuda")
    mp, fp = m.data_ptr(), f.data_ptr()
    nan, inf = float("nan"), float("inf")
    assert lib.desire_mask_distance(None, mp, 2, 4, 5, 1.0, 1.0, fp, None) == -1 and b"handle" in lib.desire_last_error()
    assert lib.desire_mask_distance(h._h, None, 2, 4, 5, 1.0, 1.0, fp, None) == -1 and b"dev_mask" in lib.desire_last_error()
    assert lib.desire_mask_distance(h._h, mp, 2, 4, 5, 1.0, 1.0, None, None) == -1 and b"dev_field" in lib.desire_last_error()
    for n in (0, -1, 65536):
        assert lib.desire_mask_distance(h._h, mp, n, 4, 5, 1.0, 1.0, fp, None) == -1 and b"n_masks" in lib.desire_last_error()
    for side in (0, -3, 1025):
        assert lib.desire_mask_distance(h._h, mp, 2, side, 5, 1.0, 1.0, fp, None) == -1 and b"Mh" in lib.desire_last_error()
        assert lib.desire_mask_distance(h._h, mp, 2, 4, side, 1.0, 1.0, fp, None) == -1 and b"Mw" in lib.desire_last_error()
    for c in (0.0, -1.0, nan, inf):
        assert lib.desire_mask_distance(h._h, mp, 2, 4, 5, c, 1.0, fp, None) == -1 and b"cell_x" in lib.desire_last_error()
        assert lib.desire_mask_distance(h._h, mp, 2, 4, 5, 1.0, c, fp, None) == -1 and b"cell_y" in lib.desire_last_error()
    from desire_amd import _lib
    hr = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    assert lib.desire_mask_distance(hr._h, mp, 2, 4, 5, 1.0, 1.0, fp, None) == -1 and b"ref_compat" in lib.desire_last_error()
    assert lib.desire_set_offroad_field(hr._h, fp, 2, 4, 5, (np.zeros(1, np.int32)).ctypes.data_as(lib.desire_set_offroad_field.argtypes[5])) == -1
    hr.close()
    torch.cuda.synchronize()
    assert bool((f == -7.0).all())
    h.close()


# ---- 2. the op against the statements -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _op_case(shape, field, seed=SEED):
    """Inputs and both statements, computed once per case, shared, never modified."""
    d = _dims(shape)
    Mh, Mw = field
    masks = make_masks(2, Mh, Mw, seed)
    cell = cell_sizes(d, Mh, Mw)
    F = mask_field_f32(masks, *cell)
    Y, fut, valid, planted = make_offroad_inputs(d, Mh, Mw, seed)
    fos = default_fos(d.n_scenes)
    f64 = offroad_f64(Y, fut, valid, F, fos, SCALE_PX, d)
    f32 = offroad_f32(Y, fut, valid, F, fos, SCALE_PX, d)
    return d, masks, cell, F, Y, fut, valid, planted, fos, f32, f64


def _attach(h, masks, cell, F, fos):
    """The field built on the device (and held to the statement), attached with the mapping; the tensor is returned to be kept alive."""
    f_t = _device_field(h, masks, cell)
    np.testing.assert_array_equal(_bits(f_t.cpu().numpy()), _bits(F))
    h.set_offroad_field(f_t.data_ptr(), masks.shape[0], masks.shape[1], masks.shape[2], fos)
    return f_t


def _op(h, d, fut_t, Y_t, scale, want=(True, True, True, True), fill=-7.0):
    import torch
    A = d.n_scenes * d.mno
    out = {"off": torch.full((A, d.K), fill, device="cuda") if want[0] else None,
           "count": torch.full((d.n_scenes, d.K), -7, device="cuda", dtype=torch.int32) if want[1] else None,
           "dY": torch.full((d.R, d.T_pred, 2), fill, device="cuda") if want[2] else None,
           "term": torch.full((1,), fill, device="cuda") if want[3] else None}
    p = lambda k: out[k].data_ptr() if out[k] is not None else 0
    h.offroad_loss(fut_t.data_ptr(), Y_t.data_ptr(), scale, p("off"), p("count"), p("dY"), p("term"))
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("field", FIELDS, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_op_matches_the_contract(shape, field):
    d, masks, cell, F, Y, fut, valid, planted, fos, f32, f64 = _op_case(shape, field)
    # on the reference alone, before the device is looked at: neither all road nor all wall, the margin, and what the inputs must hold
    share = positive_share(f64)
    assert 0.25 <= share <= 0.75, share
    assert f64["margin"][~planted].min() >= MARGIN * 0.999
    u = Y[..., 0].astype(np.float64) * field[1] - 0.5
    assert np.isnan(Y).sum() == 2 and (Y[..., 0] == 1.0).any() and (Y < 0).any() and (u < 0).any() and (u > field[1] - 1).any()
    assert not f64["lmask"].all() and f64["count"].sum() > 0
    print("%s on %dx%d: %s, share of counted positions off the road %.2f" % (shape, field[0], field[1],
                                                                            "staged" if offroad_geometry(d.mno, d.T_pred, *field)[1] else "global taps", share))
    h, fut_t = _op_handle(d, valid, fut)
    f_t = _attach(h, masks, cell, F, fos)
    got = _op(h, d, fut_t, _t(Y), SCALE_PX)
    np.testing.assert_array_equal(got["count"], f32["count"])
    np.testing.assert_array_equal(got["count"], f64["count"])
    for k in ("off", "dY", "term"):
        np.testing.assert_array_equal(_bits(got[k]), _bits(f32[k]), err_msg=k)
        basis = float(np.abs(f32[k].astype(np.float64) - f64[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - f64[k]).max())
        print("%s: |got - f64| = %.3g, |f32 - f64| = %.3g (%.1f ulp of the largest entry)" % (k, err, basis, basis / np.abs(f64[k]).max() * 2.0 ** 24))
        assert err <= basis
    again = _op(h, d, fut_t, _t(Y), SCALE_PX)
    for k in got:
        np.testing.assert_array_equal(_bits(got[k]), _bits(again[k]), err_msg=k)
    del f_t
    h.close()


def test_null_outputs_negative_entry_and_refusals():
    import torch
    from desire_amd import _lib
    d, masks, cell, F, Y, fut, valid, planted, fos, f32, f64 = _op_case((2, 8, 3, 7), (4, 5))
    h, fut_t = _op_handle(d, valid, fut)
    Y_t = _t(Y)
    lib = h.lib
    off = torch.full((d.A, d.K), -7.0, device="cuda")
    dY = torch.full((d.R, d.T_pred, 2), -7.0, device="cuda")
    fp, yp, op, dp = fut_t.data_ptr(), Y_t.data_ptr(), off.data_ptr(), dY.data_ptr()
    # before a field is set
    assert lib.desire_offroad_loss(h._h, fp, yp, 1.0, op, None, dp, None, None) == ERR_STATE and b"field" in lib.desire_last_error()
    assert lib.desire_set_offroad_loss(h._h, 1.0, 1.0) == ERR_STATE and b"field" in lib.desire_last_error()
    f_t = _attach(h, masks, cell, F, fos)
    i32p = lib.desire_set_offroad_field.argtypes[5]
    bad = np.array([0, 2], np.int32)
    assert lib.desire_set_offroad_field(h._h, f_t.data_ptr(), 2, 4, 5, bad.ctypes.data_as(i32p)) == -1 and b"field_of_scene" in lib.desire_last_error()
    assert lib.desire_set_offroad_field(h._h, None, 2, 4, 5, bad.ctypes.data_as(i32p)) == -1 and b"dev_field" in lib.desire_last_error()
    assert lib.desire_set_offroad_field(h._h, f_t.data_ptr(), 2, 4, 5, None) == -1
    assert lib.desire_set_offroad_field(h._h, f_t.data_ptr(), 0, 4, 5, bad.ctypes.data_as(i32p)) == -1 and b"n_fields" in lib.desire_last_error()
    assert lib.desire_set_offroad_field(h._h, f_t.data_ptr(), 2, 4, 1025, bad.ctypes.data_as(i32p)) == -1 and b"Mw" in lib.desire_last_error()
    nan, inf = float("nan"), float("inf")
    assert lib.desire_offroad_loss(None, fp, yp, 1.0, op, None, dp, None, None) == -1 and b"handle" in lib.desire_last_error()
    assert lib.desire_offroad_loss(h._h, None, yp, 1.0, op, None, dp, None, None) == -1 and b"dev_fut" in lib.desire_last_error()
    assert lib.desire_offroad_loss(h._h, fp, None, 1.0, op, None, dp, None, None) == -1 and b"dev_Yhat" in lib.desire_last_error()
    for s in (0.0, -1.0, nan, inf):
        assert lib.desire_offroad_loss(h._h, fp, yp, s, op, None, dp, None, None) == -1 and b"scale" in lib.desire_last_error(), s
        assert lib.desire_set_offroad_loss(h._h, 1.0, s) == -1 and b"scale" in lib.desire_last_error(), s
    for wt in (-1.0, nan, inf):
        assert lib.desire_set_offroad_loss(h._h, wt, 1.0) == -1 and b"weight" in lib.desire_last_error(), wt
    hr = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    assert lib.desire_offroad_loss(hr._h, fp, yp, 1.0, op, None, dp, None, None) == -1 and b"ref_compat" in lib.desire_last_error()
    assert lib.desire_set_offroad_loss(hr._h, 1.0, 1.0) != 0 and b"ref_compat" in lib.desire_last_error()
    hr.close()
    torch.cuda.synchronize()
    assert bool((off == -7.0).all()) and bool((dY == -7.0).all())          # nothing was launched or written
    with pytest.raises(Exception):
        h.device_tensor("off_term")                                           # and nothing allocated
    # the mapping of the refused call did not take effect: the op is the statement's on the mapping attached before
    a = _op(h, d, fut_t, Y_t, SCALE_PX)
    for k in a:
        np.testing.assert_array_equal(_bits(a[k]), _bits(f32[k]), err_msg=k)
    # all sixteen NULL / non-NULL output choices write the same bits into what they do write, and the rest into the workspace
    for mask in range(16):
        want = tuple(bool(mask >> i & 1) for i in range(4))
        part = _op(h, d, fut_t, Y_t, SCALE_PX, want)
        for k, on, ws, dt in zip(("off", "count", "dY", "term"), want, ("off_val", "off_count", "off_grad", "off_term"), ("<f4", "<i4", "<f4", "<f4")):
            if on:
                np.testing.assert_array_equal(_bits(part[k]), _bits(a[k]), err_msg=k)
            else:
                assert part[k] is None
                kept = h.device_tensor(ws, dt).cpu().numpy()[: a[k].size].reshape(a[k].shape)
                np.testing.assert_array_equal(_bits(kept), _bits(a[k]), err_msg=ws)
    # a negative entry silences a window that holds agents; the other window keeps its bits up to nothing (nvalid counts the loss mask)
    fos2 = np.array([-1, 0], np.int32)
    h.set_offroad_field(f_t.data_ptr(), 2, 4, 5, fos2)
    b = _op(h, d, fut_t, Y_t, SCALE_PX)
    ref = offroad_f32(Y, fut, valid, F, fos2, SCALE_PX, d)
    for k in b:
        np.testing.assert_array_equal(_bits(b[k]), _bits(ref[k]), err_msg=k)
    rows = d.K * d.mno
    assert not b["off"][: d.mno].any() and not b["count"][0].any() and not b["dY"][:rows].any()
    np.testing.assert_array_equal(_bits(b["dY"][rows:]), _bits(a["dY"][rows:]))
    h.close()


@pytest.mark.parametrize("off", [8, 4])
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_op_on_tensors_off_16_byte_alignment(shape, off):
    import torch
    d, masks, cell, F, Y, fut, valid, planted, fos, f32, f64 = _op_case(shape, (4, 5))
    h, fut_t = _op_handle(d, valid, fut)
    f_t = _attach(h, masks, cell, F, fos)
    Y_t = _t(Y)
    got = _op(h, d, fut_t, at_byte_offset(Y_t, off), SCALE_PX)
    for k in got:
        np.testing.assert_array_equal(_bits(got[k]), _bits(f32[k]), err_msg=k)
    dY = at_byte_offset(torch.full((d.R, d.T_pred, 2), -7.0, device="cuda"), off)      # the gradient's 16-byte stores fall back too
    h.offroad_loss(fut_t.data_ptr(), Y_t.data_ptr(), SCALE_PX, 0, 0, dY.data_ptr(), 0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(dY.cpu().numpy()), _bits(f32["dY"]))
    del f_t
    h.close()


def test_four_windows_against_two_calls_of_two_and_permuted_windows():
    """A window's off and count depend on its own rows, targets and field; its gradient carries the common factor 1 / nvalid besides: the two
    halves hold the same agents, so nvalid doubles exactly and 2 x the four-window gradient is the two-window gradient bit for bit."""
    Mh, Mw = 64, 64
    d2, d4 = _dims((2, 8, 3, 7)), _dims((4, 8, 3, 7))
    masks = make_masks(2, Mh, Mw, SEED)
    cell = cell_sizes(d2, Mh, Mw)
    F = mask_field_f32(masks, *cell)
    Ya, fut, valid, _ = make_offroad_inputs(d2, Mh, Mw, SEED)
    Yb, _, _, _ = make_offroad_inputs(d2, Mh, Mw, SEED + 1)
    fos_a, fos_b = np.array([1, 0], np.int32), np.array([0, 1], np.int32)
    res = []
    for Y, fos in ((Ya, fos_a), (Yb, fos_b)):
        h, fut_t = _op_handle(d2, valid, fut)
        f_t = _attach(h, masks, cell, F, fos)
        res.append(_op(h, d2, fut_t, _t(Y), SCALE_PX))
        h.close()
    fut4, valid4 = np.concatenate([fut, fut]), np.concatenate([valid, valid])
    h, fut_t = _op_handle(d4, valid4, fut4)
    f_t = _attach(h, masks, cell, F, np.concatenate([fos_a, fos_b]))
    Y4 = np.concatenate([Ya, Yb])
    four = _op(h, d4, fut_t, _t(Y4), SCALE_PX)
    A, R = d2.A, d2.R
    for i, half in enumerate(res):
        np.testing.assert_array_equal(_bits(four["off"][i * A:(i + 1) * A]), _bits(half["off"]))
        np.testing.assert_array_equal(four["count"][2 * i:2 * i + 2], half["count"])
        np.testing.assert_array_equal(_bits(np.float32(2.0) * four["dY"][i * R:(i + 1) * R]), _bits(half["dY"]))
    assert np.abs(four["dY"]).max() > 0 and four["count"].sum() > 0
    # permuted windows: rows, targets, mask and mapping move together, and so do the outputs
    perm = [2, 0, 3, 1]
    rows = d4.K * d4.mno
    Yp = np.concatenate([Y4[p * rows:(p + 1) * rows] for p in perm])
    h.close()
    h, fut_t = _op_handle(d4, valid4.reshape(4, -1)[perm].reshape(-1), fut4[perm])
    f_t = _attach(h, masks, cell, F, np.concatenate([fos_a, fos_b])[perm])
    moved = _op(h, d4, fut_t, _t(Yp), SCALE_PX)
    for j, p in enumerate(perm):
        np.testing.assert_array_equal(_bits(moved["off"][j * d4.mno:(j + 1) * d4.mno]), _bits(four["off"][p * d4.mno:(p + 1) * d4.mno]))
        np.testing.assert_array_equal(moved["count"][j], four["count"][p])
        np.testing.assert_array_equal(_bits(moved["dY"][j * rows:(j + 1) * rows]), _bits(four["dY"][p * rows:(p + 1) * rows]))
    del f_t
    h.close()


# ---- 3. the training step -----------------------------------------------------------------------------------------------------------------------
FIELD_T = (16, 16)
# the seeds are chosen (on the CPU, from the float64 oracle alone) so that no counted position of Y0 lies within 1e-4 cells of a cell line or a
# centre line: the fp32 and float64 Y0 differ by about 1e-6, and a flipped cell would be a test artefact
CASES = {"mean8": ((2, 8, 3, 7), 44, 2, MEAN, 0.0, AGENT),
         "mean32": ((2, 32, 3, 7), 42, 4, MEAN, 0.0, AGENT),               # tests/test_gpu_train.py's own case
         "scene_softmin": ((2, 8, 3, 7), 44, 2, SOFTMIN, TAU, SCENE)}
COLLISION = (400.0, 0.5)                                                    # radius in pixels and weight of the collision term where both are on


@functools.lru_cache(maxsize=None)
def _reference(tag, both=False):
    """Float64 autograd of loss(mode, scope) + weight * L_off (+ the collision term) on make_case(seed, n_absent), masks and weight chosen from
    the oracle's Y0: computed once per case, shared, never modified."""
    shape, seed, n_absent, mode, tau, scope = CASES[tag]
    d = _dims(shape)
    past, fut, eps, grids, gos = make_case(d, seed=seed, n_absent=n_absent)
    return offroad_loss_and_grads(to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos, _weights(d), d, mode, tau, scope, FIELD_T[0], FIELD_T[1],
                                  SCALE_PX, collision=COLLISION if both else None)


def _set_masks(h, d, vals, fos=None):
    masks = vals["masks"]
    f_t = _attach(h, masks, cell_sizes(d, *FIELD_T), vals["field"], np.arange(d.n_scenes, dtype=np.int32) if fos is None else fos)
    return f_t


def _offroad_step(tag, bf16=0, both=False):
    import torch
    shape, seed, n_absent, mode, tau, scope = CASES[tag]
    d = _dims(shape)
    w = _weights(d)
    vals, ref = _reference(tag, both)
    # on the reference alone: the margin, a mask that is neither all road nor all wall, and a term that carries at least half of the gradient
    assert vals["margin"] >= 1e-4, vals["margin"]
    assert 0.25 <= vals["positive"] <= 0.75 and vals["share"] >= 0.5, (vals["positive"], vals["share"])
    print("%s: weight %.4g, scale %g px, L_off %.6g, share of |d loss / d head/w| %.2f, margin %.2e cells" % (tag, vals["weight"], vals["scale"],
                                                                                                             vals["L_off"], vals["share"], vals["margin"]))
    dd = d.replace(bf16=bf16) if bf16 else d
    h, ten = _training_handle(dd, w, make_case(d, seed=seed, n_absent=n_absent))
    if mode != MEAN:
        h.set_recon_loss(mode, tau)
        h.set_recon_scope(scope)
    if both:
        h.set_collision_loss(COLLISION[1], COLLISION[0], 1.0 / d.sx, 1.0 / d.sy)
    ioc = [k for k in w if k.startswith("ioc/")]
    _step(h, ten)                                                            # the same step at weight 0: what the term must not reach
    torch.cuda.synchronize()
    base = (_grads(h, w, ioc), h.train_loss(ten["fut"].data_ptr()))
    ten["field"] = _set_masks(h, d, vals)
    h.set_offroad_loss(vals["weight"], vals["scale"])
    _step(h, ten)
    torch.cuda.synchronize()
    return h, ten, w, d, vals, ref, ioc, base


@pytest.mark.parametrize("tag", list(CASES))
def test_training_gradients_match_float64_autograd(tag):
    h, ten, w, d, vals, ref, ioc, base = _offroad_step(tag)
    _check_done_gradients(h, w, ref)
    # the IOC module sees detached trajectories, and KL / cross-entropy / regression do not see the term: bit for bit the step at weight 0
    now = _grads(h, w, ioc)
    for k in ioc:
        np.testing.assert_array_equal(_bits(now[k]), _bits(base[0][k]), err_msg=k)
    loss = h.train_loss(ten["fut"].data_ptr())
    for key in ("recon", "kld", "ce", "reg", "n_present"):
        assert loss[key] == base[1][key], key
    # off_term reports what is trained: the bits of the statement on the device's own Y0, and the oracle's L_off up to the displacement
    got = float(h.device_tensor("off_term").cpu().numpy()[0])
    Y0 = h.read_buffer("Y0", (d.R, d.T_pred, 2))
    fut, valid = ten["fut"].cpu().numpy(), h.device_tensor("valid", "|u1").cpu().numpy()[: d.A]
    fos = np.arange(d.n_scenes, dtype=np.int32)
    f32 = offroad_f32(Y0, fut, valid, vals["field"], fos, vals["scale"], d)
    assert np.float32(got).view(np.uint32) == f32["term"].view(np.uint32)[0]
    np.testing.assert_array_equal(h.device_tensor("off_count", "<i4").cpu().numpy()[: d.n_scenes * d.K].reshape(d.n_scenes, d.K), f32["count"])
    np.testing.assert_array_equal(_bits(h.device_tensor("off_val").cpu().numpy()[: d.A * d.K].reshape(d.A, d.K)), _bits(f32["off"]))
    f64o = offroad_f64(vals["Y0"], fut, valid, vals["field"], fos, vals["scale"], d)
    np.testing.assert_array_equal(f32["count"], f64o["count"])              # the margin at work: no cell flipped between the two Y0
    # against the oracle's own trajectories: phi = (dist / scale)^2 with a bilinear dist whose slope is at most 1 per axis (neighbouring cells of
    # an exact distance field differ by at most the cell), so |L_off(device Y0) - L_off(oracle Y0)| <= 2 sqrt(max phi) / scale * sqrt(2) * delta,
    # delta the largest displacement in pixels; and the fp32 statement's own distance from the float64 one on the same Y0
    dev = (Y0.astype(np.float64) - vals["Y0"]) * np.array([1.0 / d.sx, 1.0 / d.sy])
    delta = float(np.sqrt((dev ** 2).sum(-1)).max())
    lip = 2.0 * float(np.sqrt(f64o["phi"].max())) / vals["scale"] * np.sqrt(2.0) * delta
    f64d = offroad_f64(Y0, fut, valid, vals["field"], fos, vals["scale"], d)
    bar = lip + 4.0 * abs(float(f32["term"][0]) - float(f64d["term"][0]))
    print("%s: off_term %.9g, float64 L_off of the oracle %.9g; displacement %.3g px, bound %.3g, difference %.3g"
          % (tag, got, vals["L_off"], delta, bar, abs(got - vals["L_off"])))
    assert abs(got - vals["L_off"]) <= bar
    h.close()


def test_training_gradients_with_split_operands():
    """dims.bf16 = 2: tests/test_gpu_split.py's bar for this configuration."""
    h, ten, w, d, vals, ref, ioc, base = _offroad_step("mean32", bf16=2)
    _check_done_gradients(h, w, ref, tol=2e-4)
    h.close()


def test_training_gradients_with_the_collision_term_too():
    h, ten, w, d, vals, ref, ioc, base = _offroad_step("mean32", both=True)
    assert vals["L_col"] > 0
    _check_done_gradients(h, w, ref)
    assert float(h.device_tensor("col_term")[0]) > 0 and float(h.device_tensor("off_term")[0]) > 0
    h.close()


def test_weight_zero_leaves_every_bit_as_it_was():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    case = make_case(d, seed=42, n_absent=4)
    vals, _ = _reference("mean32")
    res = []
    for touch in (True, False):
        h, ten = _training_handle(d, w, case)
        if touch:
            ten["field"] = _set_masks(h, d, vals)                              # a field attached, the weight 0: nothing of the step changes
            h.set_offroad_loss(0.0, 0.0)
        _step(h, ten)
        torch.cuda.synchronize()
        res.append((h.grad_tensor().clone(), h.train_loss(ten["fut"].data_ptr()), ten["Y"].clone()))
        with pytest.raises(Exception):
            h.device_tensor("off_term")                                       # the default never allocates or runs the new code
        h.close()
    assert float(res[0][0].abs().max()) > 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][2], res[1][2])
    assert res[0][1] == res[1][1]


def test_mapping_changed_between_two_steps_takes_effect():
    import torch
    h, ten, w, d, vals, ref, ioc, base = _offroad_step("mean8")
    first = (float(h.device_tensor("off_term")[0]), h.device_tensor("off_count", "<i4")[: d.n_scenes * d.K].clone(), h.grad_tensor().clone())
    swapped = np.array([1, -1], np.int32)                # window 0 reads the other window's field, window 1 none
    h.set_offroad_field(ten["field"].data_ptr(), 2, FIELD_T[0], FIELD_T[1], swapped)
    _step(h, ten)
    torch.cuda.synchronize()
    Y0 = h.read_buffer("Y0", (d.R, d.T_pred, 2))
    fut, valid = ten["fut"].cpu().numpy(), h.device_tensor("valid", "|u1").cpu().numpy()[: d.A]
    f32 = offroad_f32(Y0, fut, valid, vals["field"], swapped, vals["scale"], d)
    assert np.float32(float(h.device_tensor("off_term")[0])).view(np.uint32) == f32["term"].view(np.uint32)[0]
    assert float(h.device_tensor("off_term")[0]) != first[0] and not torch.equal(h.grad_tensor(), first[2])
    h.set_offroad_field(ten["field"].data_ptr(), 2, FIELD_T[0], FIELD_T[1], np.arange(2, dtype=np.int32))      # and back: the first step's bits
    _step(h, ten)
    torch.cuda.synchronize()
    assert float(h.device_tensor("off_term")[0]) == first[0] and torch.equal(h.grad_tensor(), first[2])
    assert torch.equal(h.device_tensor("off_count", "<i4")[: d.n_scenes * d.K], first[1])
    h.close()


def test_compacted_step_matches_the_padded_one():
    """DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC: the term is taken on the full layout before the gather.  The count is an integer
    path and must be equal; the gradient difference is reported, and held to what tests/test_gpu_compact_rows.py holds the mean-mode step on
    slot classes to (3e-5 of the largest entry)."""
    import torch
    from tests.test_gpu_compact_rows import _spread, ragged_counts
    d = small_dims(n_scenes=8, K=3, T_obs=6, T_pred=7, n_grids=1)
    w = _spread(init_weights(d, 41))
    case = ragged_counts(d, seed=44, counts=[3, 9, 0, 14, 8, d.mno, 1, 20])
    masks = make_masks(2, 64, 64, SEED)
    cell = cell_sizes(d, 64, 64)
    F = mask_field_f32(masks, *cell)
    fos = np.array([0, 1, 0, -1, 1, 0, 1, 0], np.int32)
    res = []
    for dd, min_rows in ((d, None), (d.replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC), 0)):
        h, ten = _training_handle(dd, w, case, min_rows)
        f_t = _attach(h, masks, cell, F, fos)
        h.set_offroad_loss(0.5, SCALE_PX)
        _step(h, ten)
        torch.cuda.synchronize()
        res.append((h.train_loss(ten["fut"].data_ptr()), _grads(h, w), h.device_tensor("off_count", "<i4").cpu().numpy()[: d.n_scenes * d.K].copy(),
                    h.device_tensor("off_val").cpu().numpy()[: d.A * d.K].copy(), float(h.device_tensor("off_term").cpu().numpy()[0])))
        del f_t
        h.close()
    (la, ga, ta, ca, ma), (lb, gb, tb, cb, mb) = res
    assert ta.sum() > 0 and ma > 0
    np.testing.assert_array_equal(ta, tb)
    assert np.abs(ca - cb).max() <= 2e-6 * max(1.0, np.abs(ca).max()) and abs(ma - mb) <= 2e-6 * max(1.0, abs(ma))
    worst = ("", 0.0)
    for k in ga:
        if k == "ioc/score/b":
            continue
        ref = np.abs(ga[k]).max()
        err = float(np.abs(ga[k] - gb[k]).max() / (ref + 1e-12)) if ref > 1e-9 else float(np.abs(gb[k]).max())
        if err > worst[1]:
            worst = (k, err)
        assert np.isfinite(gb[k]).all()
    print("slot classes vs padded step with the off-road term: worst relative gradient difference %.2e (%s)" % (worst[1], worst[0]))
    assert worst[1] < 3e-5, worst


def test_step_with_the_term_replays_from_a_hipgraph():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    vals, _ = _reference("mean32")
    h, ten = _training_handle(d, w, make_case(d, seed=42, n_absent=4))
    ten["field"] = _set_masks(h, d, vals)
    h.set_offroad_loss(vals["weight"], vals["scale"])
    side = torch.cuda.Stream()
    sp = side.cuda_stream

    def step(stream):
        _step(h, ten, stream)
        h.clip_grads(1e-3, stream=stream)

    torch.cuda.synchronize()
    step(sp)                                             # warm-up outside capture: lazy allocations and function attributes
    side.synchronize()
    g_ref, Y_ref = h.grad_tensor().clone(), ten["Y"].clone()
    c_ref, t_ref = h.device_tensor("off_val").clone(), h.device_tensor("off_count", "<i4").clone()
    assert int(t_ref.sum()) > 0
    step(sp)                                             # a second eager run: the same bits
    side.synchronize()
    assert torch.equal(h.grad_tensor(), g_ref) and torch.equal(ten["Y"], Y_ref) and torch.equal(h.device_tensor("off_val"), c_ref)
    h.graph_begin(sp)
    step(sp)
    gid = h.graph_end(sp)
    for _ in range(3):
        h.grad_tensor().zero_(); ten["Y"].zero_(); h.device_tensor("off_val").zero_(); h.device_tensor("off_count", "<i4").zero_()
        torch.cuda.synchronize()
        h.graph_launch(gid, sp)
        side.synchronize()
        assert torch.equal(ten["Y"], Y_ref)
        assert torch.equal(h.device_tensor("off_val"), c_ref) and torch.equal(h.device_tensor("off_count", "<i4"), t_ref)
        assert torch.equal(h.grad_tensor(), g_ref)
    assert float(g_ref.abs().max()) > 0
    h.close()


def test_the_term_lowers_the_penalty_on_a_fixed_batch():
    import torch
    d = _dims((2, 32, 3, 7))
    w = _weights(d)
    vals, _ = _reference("mean32")
    run = {}
    for tag, wt in (("on", vals["weight"]), ("off", 0.0)):
        h, ten = _training_handle(d, w, make_case(d, seed=42, n_absent=4))
        ten["field"] = _set_masks(h, d, vals)
        if wt > 0:
            h.set_offroad_loss(wt, vals["scale"])
        term, count = torch.zeros(1, device="cuda"), torch.zeros((d.n_scenes, d.K), device="cuda", dtype=torch.int32)
        trace = []
        for it in range(41):                             # the steps of tests/test_gpu_train.py::test_loss_decreases_on_a_fixed_batch
            _step(h, ten)
            if it in (0, 40):                            # the op on the step's own Y0: the same read-out with the term on and off
                h.offroad_loss(ten["fut"].data_ptr(), h.device_tensor("Y0").data_ptr(), vals["scale"], 0, count.data_ptr(), 0, term.data_ptr())
                torch.cuda.synchronize()
                trace.append((float(term[0]), int(count.sum())))
            if it == 40:
                break
            h.clip_grads(10.0)
            h.adam_step(0.002)
        run[tag] = trace
        h.close()
    print("L_off, count: with the term %s, without %s" % (run["on"], run["off"]))
    assert run["on"][0] == run["off"][0] and run["on"][0][0] > 0
    assert run["on"][1][0] < run["on"][0][0]                                 # the term went down
    assert run["on"][1][0] < run["off"][1][0] and run["on"][1][1] < run["off"][1][1]      # and both end below the control


# ---- 4. the host surface --------------------------------------------------------------------------------------------------------------------------
def _model_batch():
    rng = np.random.default_rng(0)
    ids = np.arange(1, 9, dtype=np.float32)[None, :, None]
    x = [np.concatenate([ids.repeat(6, 0), rng.uniform(200, 1800, (6, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    y = [np.concatenate([ids.repeat(7, 0), rng.uniform(200, 1800, (7, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    return x, y


def test_model_reaches_the_handle():
    from types import SimpleNamespace
    from desire_amd.model import DESIREModel
    base = dict(seq_length=6, pred_length=7, d_dim=64, rnn_size=512, latent_size=64, max_num_obj=8, learning_rate=0.0005, grad_clip=10.0,
                neighborhood_size=256, grid_size=4, num_samples=3, batch_size=2)
    x, y = _model_batch()
    m = DESIREModel(SimpleNamespace(**base), seed=3)
    terms = m.train_step(x, y, seed=1)
    assert "off" not in terms
    with pytest.raises(Exception):
        m._trained.device_tensor("off_term")                                  # the default never allocates or runs the new code
    walls = np.zeros((2, 8, 8), np.uint8)
    walls[0, 0, 0] = 1                                                        # one road cell in a corner: everybody stands off the road
    walls[1] = 1                                                              # all road
    m = DESIREModel(SimpleNamespace(offroad_weight=0.5, offroad_scale=200.0, **base), seed=3)
    m.set_scene_masks(walls, [0, 0])
    terms = m.train_step(x, y, seed=1)
    h = m._trained
    assert np.isfinite(terms["loss"]) and terms["off"] > 0
    assert terms["off"] == float(h.device_tensor("off_term")[0])
    assert int(h.device_tensor("off_count", "<i4")[: h.dims.n_scenes * h.dims.K].sum()) > 0
    d = h.dims
    np.testing.assert_array_equal(_bits(m._mask_field.cpu().numpy()), _bits(mask_field_f32(walls, (1.0 / d.sx) / 8, (1.0 / d.sy) / 8)))
    assert m.train_step(x, y, seed=1, mask_of_scene=[1, 1])["off"] == 0.0     # the batch's own mapping: all road
    cnt = h.device_tensor("off_count", "<i4")[: d.n_scenes * d.K].cpu().numpy().reshape(d.n_scenes, d.K)
    assert not cnt.any()
    assert m.train_step(x, y, seed=1, mask_of_scene=[0, -1])["off"] > 0
    cnt = h.device_tensor("off_count", "<i4")[: d.n_scenes * d.K].cpu().numpy().reshape(d.n_scenes, d.K)
    assert cnt[0].all() and not cnt[1].any()
    pend = m.train_step(x, y, seed=1, sync=False, mask_of_scene=[0, 0])
    assert pend.get()["off"] > 0 and "col" not in pend.get()
    both = DESIREModel(SimpleNamespace(offroad_weight=0.5, offroad_scale=200.0, collision_weight=0.5, collision_radius=3000.0, **base), seed=3)
    both.set_scene_masks(walls, [0, 0])
    t2 = both.train_step(x, y, seed=1, sync=False).get()
    assert t2["col"] > 0 and t2["off"] > 0
    for bad in (dict(offroad_weight=0.5), dict(offroad_weight=0.5, offroad_scale=0.0), dict(offroad_weight=-1.0, offroad_scale=5.0)):
        mb = DESIREModel(SimpleNamespace(**bad, **base), seed=3)
        mb.set_scene_masks(walls, [0, 0])
        with pytest.raises(ValueError):
            mb.train_step(x, y, seed=1)
    with pytest.raises(ValueError, match="set_scene_masks"):
        DESIREModel(SimpleNamespace(offroad_weight=0.5, offroad_scale=5.0, **base), seed=3).train_step(x, y, seed=1)


def test_train_runs_an_epoch_with_the_offroad_column(tmp_path):
    import re
    from desire_amd import train as T
    common = ["--batch_size", "2", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--d_dim", "64", "--latent_size", "64",
              "--num_samples", "5", "--neighborhood_size", "256", "--num_epochs", "1", "--prefetch", "0", "--save_dir", str(tmp_path),
              "--data_dir", str(tmp_path)]
    t = np.arange(10, dtype=np.float32)
    win = np.zeros((2, 10, 8, 3), np.float32)                         # two windows of four objects walking straight lines
    for n in range(2):
        for i in range(4):
            win[n, :, i, 0] = i + 1
            win[n, :, i, 1] = 200 + 150 * i + (3 + n) * t
            win[n, :, i, 2] = 150 + 100 * i + 2 * t

    class Loader:                                                     # the reference loader's surface, and the two videos the windows come from
        seq_length, num_batches, leave_dataset = 10, 2, 2

        def _csv_paths(self):
            return [str(tmp_path / "a" / "v0" / "x.csv"), str(tmp_path / "a" / "v1" / "x.csv")]

        def reset_batch_pointer(self):
            pass

        def next_batch(self):
            return list(win), None, [0, 1]

    road = np.ones((8, 8), np.uint8)
    wall = np.zeros((8, 8), np.uint8)
    wall[7, 7] = 1
    path = str(tmp_path / "masks.npz")
    np.savez(path, **{"a/v0": wall, "a/v1": road})
    lines = []
    a = T.build_parser().parse_args(common + ["--offroad_weight", "0.25", "--offroad_scale", "150", "--scene_masks", path])
    losses = T.train(a, data_loader=Loader(), log=lines.append)
    assert len(losses) == 2 and np.isfinite(losses).all()
    steps = [ln for ln in lines if "train_loss" in ln]
    assert len(steps) == 2 and all(re.search(r", off\[s=150 w=0\.25\] [0-9.]+$", ln) for ln in steps), steps
    assert float(steps[0].rsplit(" ", 1)[1]) > 0
    plain = []
    T.train(T.build_parser().parse_args(common), data_loader=Loader(), log=plain.append)
    assert all(re.fullmatch(r"\d+/2 \(epoch 0\), train_loss = [0-9.]+, time/batch = [0-9.]+", ln) for ln in plain if "train_loss" in ln), plain
    with pytest.raises(ValueError, match="--offroad_scale"):
        T.train(T.build_parser().parse_args(common + ["--offroad_weight", "0.25", "--scene_masks", path]), data_loader=Loader(), log=plain.append)
    with pytest.raises(ValueError, match="--scene_masks"):
        T.train(T.build_parser().parse_args(common + ["--offroad_weight", "0.25", "--offroad_scale", "150"]), data_loader=Loader(), log=plain.append)


def test_the_evaluation_walk_reports_the_offroad_block(tmp_path):
    """python -m desire_amd.evaluate --offroad MASKFILE on the bookstore windows: the block's rates are evaluate_offroad's, which are the
    statement's on the walk's own samples; without the flag the result is the one it has always been."""
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    from tests.test_gpu_occupancy import _PLAIN_KEYS, _args, _bookstore
    video = _bookstore()
    masks = make_masks(1, 16, 16, SEED)
    path = str(tmp_path / "masks.npz")
    np.savez(path, **{"bookstore/video6": masks[0]})
    res = {}
    for tag, extra in (("plain", []), ("off", ["--offroad", path, "--offroad_scale", "90", "--data_dir", str(tmp_path)])):
        a = _args(extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        dl._csv_paths = lambda: [str(tmp_path / "bookstore" / "video6" / "annotations.csv")]      # the key of the one video
        dl.leave_dataset = 1
        model = DESIREModel(a, seed=4)
        res[tag] = E.evaluate(a, data_loader=dl, model=model)
    assert list(res["plain"]) == _PLAIN_KEYS                           # without the flag: the result it has always been
    blk = res["off"].pop("offroad")
    assert res["off"] == res["plain"]
    assert blk["masks"] == path and blk["scale_px"] == 90.0 and blk["frames"] > 0
    for k in ("rate_mean_of_K", "rate_best_of_K", "rate_ground_truth"):
        assert 0.0 <= blk[k] <= 1.0, k
    assert blk["rate_best_of_K"] <= blk["rate_mean_of_K"] and blk["penalty"] >= 0.0 and blk["penalty_ground_truth"] >= 0.0
    assert blk["rate_mean_of_K"] > 0 and blk["penalty"] > 0                # the wall band covers a third of the frame
    # the last batch of the walk against the statement: the model still holds its samples
    Y, score = model.final_output, model.final_states
    n = int(Y.shape[0])
    h = model._handles[(n, 0, 0)]
    d = h.dims
    xs, _ = list(E.iter_batches(dl, int(a.batch_size), int(a.max_windows or 0)))[-1]
    from desire_amd.train import split_windows
    past, fut = split_windows(xs, int(a.seq_length))
    r = model.evaluate_offroad(Y, score, fut, masks, np.zeros(n, np.int32), 90.0)
    F = mask_field_f32(masks, *cell_sizes(d, 16, 16))
    futp = model._pad_windows(fut, d.mno).cpu().numpy()
    valid = h.device_tensor("valid", "|u1").cpu().numpy()[: d.A]
    f32 = offroad_f32(Y.reshape(d.R, d.T_pred, 2).cpu().numpy(), futp, valid, F, np.zeros(n, np.int32), 90.0, d)
    np.testing.assert_array_equal(r["count"], f32["count"])
    assert np.float32(r["penalty"]).view(np.uint32) == f32["term"].view(np.uint32)[0]
    np.testing.assert_array_equal(r["frames"], f32["counted"].sum((1, 2)))
    gtY = (futp[..., 1:] * np.array([d.sx, d.sy], np.float32)).transpose(0, 2, 1, 3)
    gtY = np.ascontiguousarray(np.broadcast_to(gtY[:, None], (n, d.K, d.mno, d.T_pred, 2))).reshape(d.R, d.T_pred, 2)
    g32 = offroad_f32(gtY, futp, valid, F, np.zeros(n, np.int32), 90.0, d)
    np.testing.assert_array_equal(r["gt_count"], g32["count"][:, 0])
    np.testing.assert_allclose(r["rate"], r["count"] / np.maximum(r["frames"], 1)[:, None])
