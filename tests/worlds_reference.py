"""Numpy statement of the world-selection contract (include/desire_hip.h: desire_select_worlds) in two forms -- worlds_f32, the contract's fp32
operation sequence, and worlds_f64, the same pass in float64 -- and the input generator their tests share.  World k of a window is sample k of
every slot together; agent a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot.  The per-agent values (q, m, s) are
select_reference.pair_values: the same statement.  Order and count of the two forms can only differ where a value the contract compares lies within
rounding of the radius: the generator keeps every one of them further than MARGIN * radius from it ("margin" of the float64 pass)."""
from types import SimpleNamespace

import numpy as np

from tests.joint_reference import _rank
from tests.select_reference import DIST_FINAL, DIST_MAX, DIST_MEAN, METRICS, brute_force, pair_values, weights

WORLD_ALL, WORLD_MEAN = 0, 1
REDUCES = (WORLD_ALL, WORLD_MEAN)
# fp32 rounding of a mean over 256 slots of a 200-frame sum of square roots is below 2^-24 * 456 = 2.8e-5 relative; the band is about 40 times that
MARGIN = 1e-3
# (n_scenes, mno, K, T_pred)
SHAPES = [(2, 8, 5, 12),                # the plain case
          (3, 1, 3, 7),                 # one slot: desire_select_diverse's case; odd T_pred
          (3, 32, 20, 40),              # the headline's per-window shape
          (2, 160, 4, 9),               # more slots than lanes per frame
          (2, 5, 70, 6)]                # K beyond a wave
RADIUS_PX = 20.0


def cases_of(d):
    """(metric, reduce, t_end): three metrics x two reduces x t_end in {1, T / 2, T}."""
    return [(m, r, t) for m in METRICS for r in REDUCES for t in sorted({1, max(1, d.T_pred // 2), d.T_pred})]


def world_weights(wscore, n, K, dtype):
    """[n, K]: desire_plan_risk's step 6 on the world scores (select_reference.weights at one slot per window)."""
    one = SimpleNamespace(n_scenes=n, K=K, mno=1, A=n)
    return weights(None if wscore is None else np.asarray(wscore, np.float32).reshape(n, K, 1), one, dtype)


def _worlds(Y, present, wscore, metric, reduce, t_end, radius, ux, uy, d, dtype):
    n, K, m = d.n_scenes, d.K, d.mno
    v = pair_values(Y, metric, t_end, ux, uy, d, dtype).reshape(n, m, K, K)        # q, m or s / t_end per (window, slot, k, k')
    part = np.ones((n, m), bool) if present is None else np.asarray(present).reshape(n, m) != 0
    num = part.sum(1)
    r = dtype(np.float32(radius))
    off = ~np.eye(K, dtype=bool)
    margin = np.inf
    with np.errstate(all="ignore"):
        if reduce == WORLD_ALL:
            bound = r if metric == DIST_MEAN else r * r
            near = np.where(part[:, :, None, None], v < bound, True).all(1)
            vals = v[part][:, off] if K > 1 else np.zeros(0)
        else:
            di = v if metric == DIST_MEAN else np.sqrt(v)
            D = np.zeros((n, K, K), dtype)
            for i in range(m):                                                      # increasing slot from 0
                D = np.where(part[:, i, None, None], D + di[:, i], D)
            D = D / np.maximum(num, 1).astype(dtype)[:, None, None]
            near = D < r
            bound = r
            vals = D[num > 0][:, off] if K > 1 else np.zeros(0)
        vals = vals[np.isfinite(vals)]
        if vals.size and float(r) > 0:
            margin = float(np.min(np.abs(vals.astype(np.float64) - float(bound))) / float(bound))
    near = np.array(near)
    near[num == 0] = float(r) > 0
    if float(r) == 0:
        near[:] = False
    order = np.broadcast_to(np.arange(K, dtype=np.int32), (n, K)) if wscore is None else _rank(np.asarray(wscore, np.float32).reshape(n, K))
    W = world_weights(wscore, n, K, dtype)
    out = {"order": np.zeros((n, K), np.int32), "count": np.zeros(n, np.int32), "label": np.zeros((n, K), np.int32),
           "mass": np.zeros((n, K), dtype), "near": near, "margin": margin, "processing": np.array(order)}
    for w in range(n):
        o, c, owner = brute_force(near[w], [int(k) for k in order[w]])
        out["order"][w], out["count"][w] = o, c
        for j, k in enumerate(order[w]):                                            # processing order, from 0
            out["mass"][w, owner[j]] = out["mass"][w, owner[j]] + W[w, k]
            out["label"][w, k] = owner[j]
    return out


def worlds_f32(Y, present, wscore, metric, reduce, t_end, radius, ux, uy, d):
    return _worlds(Y, present, wscore, metric, reduce, t_end, radius, ux, uy, d, np.float32)


def worlds_f64(Y, present, wscore, metric, reduce, t_end, radius, ux, uy, d):
    return _worlds(Y, present, wscore, metric, reduce, t_end, radius, ux, uy, d, np.float64)


def planted_world_scores(d, seed):
    """[n, K] fp32 on a grid of 1/64 in [-4, 4] (both references rank alike), with a tie and, where the shape has room, a NaN (window 0: uniform
    weights there)."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(-256, 257, (d.n_scenes, d.K)) / 64.0).astype(np.float32)
    if d.K >= 3:
        s[-1, 2] = s[-1, 0]
    if d.K >= 5:
        s[0, 4] = np.nan
    return s


def make_inputs(d, radius, ux, uy, seed, modes=None):
    """Y [R, T_pred, 2] fp32 (normalised units) and present [A] uint8 whose distances are laid out in the caller's unit (ux, uy) around `radius`.
    Every window has 1 - 4 scene modes: in every slot the modes' centres lie 4 radii apart along the slot's own direction, and every world is a
    mode plus a jitter of 0.05 radius per coordinate and frame.  Worlds 0, 1, 2 (K >= 3) are a chain: world 1 is world 0 shifted 0.7 radius in
    every slot and frame, world 2 shifted 1.4 radius -- 0 ~ 1, 1 ~ 2, 0 !~ 2, so the outcome depends on the processing order.  max(1, mno / 4)
    slots of a window are absent (mno >= 2) and filled with garbage hundreds of radii wide that would separate every world if it were read; the last
    window has nobody present (two windows or more); one taking-part slot of world K - 1 of window 1 (window 0 below three windows) is a NaN row.
    modes: that many scene modes in every window instead (the timing script's layouts).  Returns (Y, present, info)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    rng = np.random.default_rng(seed)
    r = float(radius)
    inv = np.array([1.0 / float(np.float32(ux)), 1.0 / float(np.float32(uy))])
    off = np.zeros((n, K, m, T, 2))
    present = np.ones((n, m), np.uint8)
    mode_of = np.zeros((n, K), np.int64)
    for w in range(n):
        n_modes = 1 + (w + seed) % 4 if modes is None else int(modes)
        mode = rng.integers(0, n_modes, K) if modes is None else rng.permutation(K) % n_modes
        mode[0] = 0
        th = rng.uniform(0, 2 * np.pi, m)
        direc = np.stack([np.cos(th), np.sin(th)], -1)                              # [m, 2]
        walk = np.cumsum(rng.normal(0, 0.1 * r, (n_modes, m, T, 2)), 2)
        for k in range(K):
            off[w, k] = mode[k] * 4.0 * r * direc[:, None, :] + walk[mode[k]] + rng.uniform(-0.05 * r, 0.05 * r, (m, T, 2))
        if K >= 3:
            phi = rng.uniform(0, 2 * np.pi)
            shift = np.array([np.cos(phi), np.sin(phi)]) * 0.7 * r
            off[w, 1], off[w, 2] = off[w, 0] + shift, off[w, 0] + 2 * shift
            mode[1] = mode[2] = 0
        mode_of[w] = mode
        if n >= 2 and w == n - 1:
            present[w] = 0
        elif m >= 2:
            present[w, rng.permutation(m)[:max(1, m // 4)]] = 0
    base = rng.uniform(0.3, 0.7, (n, 1, m, 1, 2))
    Y = (base + off * inv).astype(np.float32)
    gone = present == 0
    garbage = (rng.uniform(-300 * r, 300 * r, (n, K, m, T, 2)) * inv).astype(np.float32)
    Y = np.where(gone[:, None, :, None, None], garbage, Y)
    w_nan = 1 if n >= 3 else 0
    slot_nan = int(np.nonzero(present[w_nan])[0][-1])
    Y[w_nan, K - 1, slot_nan] = np.nan
    return (np.ascontiguousarray(Y.reshape(d.R, T, 2)), np.ascontiguousarray(present.reshape(-1)),
            {"modes": mode_of, "nan": (w_nan, K - 1, slot_nan)})
