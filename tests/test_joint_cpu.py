"""The numpy statements of the joint-metrics contract (tests/joint_reference.py) against each other, against an independent brute-force statement
of the pair rule, and the conditions their input generator promises -- on the reference alone, no GPU.  Then the evaluation command line:
without --joint its result keeps the key list it has always had."""
import numpy as np
import pytest

from tests.helpers import EVAL_FLAGS, PLAIN_KEYS as _PLAIN_KEYS, small_dims
from tests.joint_reference import (MARGIN, RADIUS_PX, SHAPES, brute_force_first, chunk_centres, chunk_frames, float_bound, joint_f32, joint_f64,
                                   make_inputs, planted_joint_scores)


def _dims(shape):
    n, m, K, T = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64)


def _units(d):
    return [(1.0, 1.0, float(np.float32(RADIUS_PX * d.sx))), (1.0 / d.sx, 1.0 / d.sy, RADIUS_PX)]


def _hz(T):
    return sorted({max(1, T // 4), max(1, T // 2), T})


_CACHE = {}


def _case(shape, unit):
    if (shape, unit) not in _CACHE:
        d = _dims(shape)
        ux, uy, radius = _units(d)[unit]
        Y, fut, present, _ = make_inputs(d, radius, ux, uy, seed=5 + unit, centres=chunk_centres(d.mno, d.T_pred))
        s = planted_joint_scores(d, 9)
        hz = _hz(d.T_pred)
        n_top = min(d.K, 2)
        _CACHE[(shape, unit)] = (d, Y, fut, present, s, hz, n_top, radius, ux, uy,
                                 joint_f32(Y, fut, None, s, hz, n_top, radius, ux, uy, d), joint_f64(Y, fut, None, s, hz, n_top, radius, ux, uy, d))
    return _CACHE[(shape, unit)]


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_the_fp32_statement_agrees_with_float64(shape, unit):
    d, Y, fut, present, s, hz, n_top, radius, ux, uy, f32, f64 = _case(shape, unit)
    assert f64["margin"] > MARGIN                                          # the float64 pass alone, before any comparison
    for key in ("first", "cnt", "order"):
        np.testing.assert_array_equal(f32[key], f64[key], err_msg=key)
    np.testing.assert_array_equal(f32["jscore"].astype(np.float64), f64["jscore"])      # exact sums in either precision (NaNs in place)
    bound = float_bound(d, f64["e_max"])
    for key in ("jerr", "out"):
        a, b = f32[key].astype(np.float64), f64[key]
        assert (np.isnan(a) == np.isnan(b)).all()
        assert float(np.nanmax(np.abs(a - b), initial=0.0)) <= bound, key


@pytest.mark.parametrize("unit", [0, 1], ids=["norm", "px"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_the_generator_plants_what_it_promises(shape, unit):
    d, Y, fut, present, s, hz, n_top, radius, ux, uy, f32, f64 = _case(shape, unit)
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    ids = fut[..., 0] != 0                                                 # [n, T, m]
    part = ids.any(1)                                                      # [n, m]
    assert not part[-1].any()                                              # a window where nobody takes part
    assert (f64["cnt"][-1] == 0).all() and (f64["first"][-1] == T).all() and (f64["out"][-1] == 0).all()
    if m == 1:                                                             # one slot has no partner: no pair, nothing to touch
        assert (f64["first"] == T).all()
        return
    assert (~part[0]).any()                                                # slots absent from every frame
    assert (part[0] & ~ids[0].all(0)).any()                                # slots that leave
    first = f64["first"]
    hit = (first[:, :K] < T)[np.broadcast_to(part[:, None], (n, K, m))]
    print("first contacts: %.1f %% of the taking-part (window, k, slot)" % (100.0 * hit.mean()))
    assert 0.10 <= hit.mean() <= 0.90
    g = first[:-1, K][part[:-1]]
    assert (g < T).any() and (g == T).any()                                # the ground truth row: touching and not touching slots
    assert np.isnan(Y).any()                                               # a NaN row ...
    Yk = Y.reshape(n, K, m, T, 2)
    nan_rows = np.isnan(Yk).all((3, 4))
    assert (first[:, :K][nan_rows] == T).all()                             # ... that never touches
    # crossings touch at middle frames only; followers and coincident pairs from frame 0
    ta = f64["touch_any"][:, :K]
    assert (ta[..., 0] & ta[..., T - 1]).any() and (~ta[..., 0] & ~ta[..., T - 1] & ta.any(-1)).any()
    Yw = Yk[0].astype(np.float64)
    same = (Yk[0][:, :, None] == Yk[0][:, None, :]).all((3, 4)) & ~np.eye(m, dtype=bool) & (part[0][:, None] & part[0][None, :])
    assert same.any()                                                      # an exactly coincident pair of counted slots
    # a pair inside the radius only at frames where one of them is not counted
    a = (Yw[:, :, None, :, 0] - Yw[:, None, :, :, 0]) * float(np.float32(ux))
    b = (Yw[:, :, None, :, 1] - Yw[:, None, :, :, 1]) * float(np.float32(uy))
    near = (a * a + b * b) < float(np.float32(radius)) ** 2                  # [K, m, m, T]
    c = ids[0].T                                                           # [m, T]
    one_gone = c[None, :, None, :] & ~c[None, None, :, :] & part[0][None, None, :, None]
    both = c[None, :, None, :] & c[None, None, :, :]
    hidden = (near & one_gone).any(-1) & ~(near & both).any(-1)
    assert hidden.any()
    if chunk_frames(m, T) < T:                                             # contacts in the first chunk, the last chunk, and across the border
        tc = chunk_frames(m, T)
        assert (first[:, :K] < tc - 2).any() and ((first[:, :K] >= tc) & (first[:, :K] < T)).any()
        assert (ta[..., tc - 1] & ta[..., tc] & ~ta[..., 0]).any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_first_contact_against_brute_force_pairwise_distances(shape):
    d, Y, fut, present, s, hz, n_top, radius, ux, uy, f32, f64 = _case(shape, 1)
    np.testing.assert_array_equal(f32["first"], brute_force_first(Y, fut, radius, ux, uy, d))
    # and the counts from it, stated independently
    part = (fut[..., 0] != 0)
    for hi, h in enumerate(hz):
        np.testing.assert_array_equal(f32["cnt"][:, :, hi, 0], (f32["first"] < h).sum(-1))
        np.testing.assert_array_equal(f32["cnt"][:, :, hi, 1], np.broadcast_to(part[:, :h].any(1).sum(-1)[:, None], (d.n_scenes, d.K + 1)))


def test_the_present_form_of_the_reference():
    d, Y, fut, present, s, hz, n_top, radius, ux, uy, f32, f64 = _case(SHAPES[0], 1)
    const = fut.copy()
    const[..., 0] = const[:, :1, :, 0]                                     # ids constant over t
    a = joint_f32(Y, const, None, s, hz, n_top, radius, ux, uy, d)
    b = joint_f32(Y, None, present, s, hz, n_top, radius, ux, uy, d)
    for key in ("first", "cnt"):
        np.testing.assert_array_equal(a[key][:, :d.K], b[key][:, :d.K])
    np.testing.assert_array_equal(a["order"], b["order"])
    assert (b["first"][:, d.K] == d.T_pred).all() and (b["cnt"][:, d.K] == 0).all()


class _Stub:
    """A model that answers the evaluation walk with zeros: the walk's own bookkeeping and key list, no device."""
    def __init__(self, K, mno, T):
        self.K, self.mno, self.T = K, mno, T

    def predict(self, past, **kw):
        self.n = len(past)
        self.final_output, self.final_states = None, None

    def evaluate_ranked(self, Y, score, fut, top=None, horizons=None, units="px", **kw):
        return np.zeros((self.n * self.mno, len(horizons), 4), np.float32)

    def evaluate(self, Y, fut):
        return np.zeros((self.n * self.mno, 4), np.float32)

    def evaluate_joint(self, Y, score, fut, top=None, horizons=None, units="px", collision_radius=None):
        n, K, m, nh = self.n, self.K, self.mno, len(horizons)
        cnt = np.zeros((n, K + 1, nh, 2), np.int32)
        cnt[..., 1] = 4
        cnt[:, 0, :, 0] = 1
        cnt[:, K, :, 0] = 2
        return {"jerr": np.ones((n, K, nh, 2), np.float32), "out": np.full((n, nh, 4), 2.0, np.float32), "order": np.zeros((n, K), np.int32),
                "jscore": np.zeros((n, K), np.float32), "cnt": cnt, "first": np.zeros((n, K + 1, m), np.int32)}


_FLAGS = [f for f in EVAL_FLAGS if f != "--device_rng"]


def test_the_command_line_keeps_its_keys_without_the_flag():
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    t = np.arange(60, dtype=np.float32)
    video = np.zeros((60, 8, 3), np.float32)
    for i in range(5):
        video[:, i, 0] = i + 1
        video[:, i, 1] = 200 + 150 * i + 3 * t
        video[:, i, 2] = 150 + 100 * i + 2 * t
    res = {}
    for tag, extra in (("plain", []), ("joint", ["--joint", "--collision_radius", "12.5"]), ("bare", ["--joint"])):
        a = E.build_parser().parse_args(_FLAGS + extra)
        dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=[video])
        res[tag] = E.evaluate(a, data_loader=dl, model=_Stub(5, 8, 6))
    assert list(res["plain"]) == _PLAIN_KEYS
    assert list(res["joint"]) == _PLAIN_KEYS + ["joint"]
    blk = res["joint"].pop("joint")
    assert res["joint"] == res["plain"]
    assert set(blk) == {"collision_radius_px", "windows", "top1", "best_of_top", "collision_rate", "slots"}
    assert blk["collision_radius_px"] == 12.5 and res["bare"]["joint"]["collision_radius_px"] == 0.0
    nh = len(res["plain"]["horizons"])
    assert blk["top1"] == {"jade": [2.0] * nh, "jfde": [2.0] * nh} and blk["best_of_top"] == {"jade": [2.0] * nh, "jfde": [2.0] * nh}
    assert blk["collision_rate"] == {"top1": [0.25] * nh, "all_K": [0.05] * nh, "ground_truth": [0.5] * nh}
    assert blk["windows"] == [res["plain"]["windows"]] * nh and blk["slots"] == [4 * res["plain"]["windows"]] * nh
