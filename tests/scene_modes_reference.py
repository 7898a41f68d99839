"""Two statements of the scene-mode contract (include/desire_hip.h: desire_fit_scene_modes), the bounds their comparison is held to, the mirror of
the kernel's LDS geometry and the synthetic inputs the tests share.

scene_modes_f32 is the contract as written, operation by operation in numpy fp32 and in its order; scene_modes_f64 is the same sequence in
float64 on the same fp32 inputs.  World k of a window is sample k of every slot together; agent a = scene * mno + slot, row r_k = (scene * K +
k) * mno + slot.  Both return a dict: label [n, K], count [n, n_modes], prob [n, n_modes], mean [n, n_modes, mno, T, 2], cov [n, n_modes, mno, T,
3], passes [n], weights [n, K], margin [n] and, with `fut`, frame [n, T] and out [n, n_h, 2].  The weights are worlds_reference.world_weights,
the Lloyd loop with its nearest-mode rule, update and covariance is modes_reference.fit on whole worlds, the mixture modes_reference.mixture, and
the likelihood's horizon reduction is kde_reference.kde_outputs on one pseudo-agent per window: the same statements as the per-agent calls'.

margin [n]: modes_reference's, on the world distances D: over every executed assign and every world with a label, (D2 - D1) / D2 of its smallest
and second smallest distance.  Labels are compared between precisions only on inputs whose float64 margin is above MARGIN; the generator redraws
a window until it is.  MARGIN stays above twice the worst-case fp32 summation bound of a D, (mno * t_end + 4) * 2^-24, for mno * t_end <= 4096
(4.9e-4): every shape of SHAPES keeps to that."""
from types import SimpleNamespace

import numpy as np

from tests.helpers import small_dims
from tests.joint_reference import _rank
from tests.kde_reference import kde_outputs
from tests.modes_reference import LOG_FLOOR, MARGIN, MIN_DET_RATIO, MIN_STD_PX, MODES_MAX, MODES_MAX_ITERS, U, _dist, fit, fit_bounds, mixture, var_floor_of  # noqa: F401
from tests.worlds_reference import planted_world_scores, world_weights

# (n_scenes, mno, K, T_pred, n_modes)
SHAPES = [(2, 8, 5, 12, 2),             # the plain case
          (3, 1, 3, 7, 2),              # the anchor: one slot, desire_fit_modes' case
          (2, 32, 20, 40, 6),           # the headline window; more than one slot chunk
          (2, 160, 4, 9, 2),            # many chunks
          (2, 8, 70, 6, 4),             # K beyond a wave
          (1, 4, 3, 200, 3),            # long horizon
          (1, 1, 1, 1, 1)]              # the degenerate case
ITERS = 8                               # the pass cap of the shared cases
SCALE_PX = 20.0                         # the length the layout is drawn in (the worlds' generator's radius)


def t_ends(T):
    return sorted({1, max(1, T // 2), T})


# ---- the LDS geometry (desire_amd/csrc/eval_lds.h: SceneModesLds, scene_modes_geometry) -------------------------------------------------------
LDS_BYTES, THREADS = 60 * 1024, 256


def fixed_bytes(K, T, n, mno):
    return 4 * (2 * K * n + 3 * K + 5 * n + n * ((K + 31) // 32) + 2 * n * T + 3 * T + mno)


def slot_bytes(K, T, n):
    return 8 * (K + n) * (T | 1) + 4 * (3 * n * T + K * n)


def scene_modes_geometry(mno, K, T, n):
    """SC, or None when the per-window words and one slot do not fit."""
    fixed, per = fixed_bytes(K, T, n, mno), slot_bytes(K, T, n)
    if fixed + per > LDS_BYTES:
        return None
    sc = min(mno, (LDS_BYTES - fixed) // per)
    chunks = -(-mno // sc)
    return -(-mno // chunks)


# ---- the contract -----------------------------------------------------------------------------------------------------------------------------
def _world_dist(Yw, means, t_end, ux, uy, dt):
    """Step 4 for one window: D [K, n] of the worlds Yw [K, P, T, 2] to the means [n, P, T, 2] -- per slot modes_reference's distance (increasing
    t from 0), the slots added in increasing slot from 0."""
    D = np.zeros((Yw.shape[0], means.shape[0]), dt)
    for s in range(Yw.shape[1]):
        D = D + _dist(Yw[:, s], means[:, s], t_end, ux, uy, dt)
    return D


def fit_window(Yw, order, w, n, t_end, iters, ux, uy, var_floor, dt):
    """Steps 3 - 8 for one window: modes_reference.fit on whole worlds -- Yw [K, P, T, 2] and w [K] in dtype dt, order [K] int; the update and
    the covariance run over every slot and every t.  mean [n, P, T, 2] and cov [n, P, T, 3] over the taking-part slots."""
    return fit(Yw, order, w, n, t_end, iters, ux, uy, var_floor, dt, dist=_world_dist)


def frame_values(res, f, ux, uy, log_floor, sx, sy, dt):
    """Step 9 for one window: f [P, T, 3] fp32 (id, x, y) of the taking-part slots -> (the frame values [T], c_t [T])."""
    P, T = f.shape[:2]
    counted = f[..., 0] != 0                                                # [P, T]
    ct = counted.sum(0)
    floor = dt(np.float32(log_floor))
    if res["bad"]:
        return np.where(ct > 0, floor, dt(0)).astype(dt), ct
    ux, uy = dt(np.float32(ux)), dt(np.float32(uy))
    gx, gy = (f[..., 1] * np.float32(sx)).astype(dt), (f[..., 2] * np.float32(sy)).astype(dt)       # the fp32 scaling is part of the inputs
    log2pi = dt(np.float32(1.8378770664093453)) if dt is np.float32 else np.log(2 * np.pi)
    n = res["prob"].shape[0]
    with np.errstate(all="ignore"):
        ls, oks = [], []
        for i in range(n):
            Pi = res["prob"][i]
            l = np.full(T, np.log(Pi), dt)
            ok = np.full(T, bool(Pi > 0))
            for s in range(P):                                              # increasing slot: one chain per (mode, t)
                cxx, cyy, cxy = res["cov"][i, s, :, 0], res["cov"][i, s, :, 1], res["cov"][i, s, :, 2]
                det = cxx * cyy - cxy * cxy
                good = det > dt(MIN_DET_RATIO) * cxx * cyy
                dx, dy = (res["mean"][i, s, :, 0] - gx[s]) * ux, (res["mean"][i, s, :, 1] - gy[s]) * uy
                c2 = dt(2) * cxy
                q = (dt(-0.5) * ((cyy * (dx * dx) - c2 * (dx * dy)) + cxx * (dy * dy))) / det
                step = (((l + q) - log2pi) - dt(0.5) * np.log(det).astype(dt)).astype(dt)
                l = np.where(counted[s] & good, step, l)
                ok = ok & (~counted[s] | good)
            ls.append(l); oks.append(ok)
        v = mixture(ls, oks, floor, dt, per=np.maximum(ct, 1).astype(dt))
    return np.where(ct > 0, v, dt(0)).astype(dt), ct


def _scene_modes(Y, present, worder, wscore, fut, n, t_end, iters, ux, uy, var_floor, hz, log_floor, d, dt):
    N, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Yk = np.asarray(Y, np.float32).reshape(N, K, m, T, 2).astype(dt)
    part = np.ones((N, m), bool) if present is None else np.asarray(present).reshape(N, m) != 0
    worder = np.asarray(worder).reshape(N, K)
    W = world_weights(wscore, N, K, dt)
    out = dict(label=np.zeros((N, K), np.int32), count=np.zeros((N, n), np.int32), prob=np.zeros((N, n), dt), mean=np.zeros((N, n, m, T, 2), dt),
               cov=np.zeros((N, n, m, T, 3), dt), passes=np.zeros(N, np.int32), margin=np.zeros(N), weights=W, part=part)
    f = None if fut is None else np.asarray(fut, np.float32).transpose(0, 2, 1, 3)      # [N, mno, T, 3]
    if f is not None:
        out["frame"], counted = np.zeros((N, T), dt), np.zeros((N, T, 1, 3), np.float32)
    for w in range(N):
        sl = np.nonzero(part[w])[0]
        r = fit_window(Yk[w][:, sl], worder[w], W[w], n, t_end, iters, ux, uy, var_floor, dt)
        for key in ("label", "count", "prob", "passes", "margin"):
            out[key][w] = r[key]
        out["mean"][w][:, sl], out["cov"][w][:, sl] = r["mean"], r["cov"]
        if f is not None:
            out["frame"][w], ct = frame_values(r, f[w][sl], ux, uy, log_floor, d.sx, d.sy, dt)
            counted[w, :, 0, 0] = ct > 0
    if f is not None:                                                       # desire_kde_nll's steps 7 - 8 with `agent` read as `window`
        out["out"] = kde_outputs(out["frame"], counted, hz, SimpleNamespace(A=N, T_pred=T), dtype=dt)
    return out


def scene_modes_f32(Y, present, worder, wscore, fut, n, t_end, iters, ux, uy, var_floor, d, hz=None, log_floor=LOG_FLOOR):
    return _scene_modes(Y, present, worder, wscore, fut, n, t_end, iters, ux, uy, var_floor, hz, log_floor, d, np.float32)


def scene_modes_f64(Y, present, worder, wscore, fut, n, t_end, iters, ux, uy, var_floor, d, hz=None, log_floor=LOG_FLOOR):
    return _scene_modes(Y, present, worder, wscore, fut, n, t_end, iters, ux, uy, var_floor, hz, log_floor, d, np.float64)


# ---- the bounds of |device - scene_modes_f64| under scores (the device's expf is not numpy's: no bits there) ------------------------------------
def scene_bounds(Y, f64, ux, uy, var_floor, d):
    """(prob [n, n_modes], mean [n, n_modes, mno, T, 2], cov [n, n_modes, mno, T, 3]): what a correct fp32 evaluation may differ from
    scene_modes_f64 by, from the contract's operations alone, u = 2^-24, m = the member WORLDS of the mode.  prob, and mean and cov of every
    (slot, t), are desire_fit_modes' expressions with the window's weights, labels and masses in place of the agent's -- the same operations in
    the same number: a weight is an expf within 2 ulp over a sum of K of them ((K + 6) u, the sum's error common to the window's weights), a
    mass m weights and m - 1 additions, a mean's numerator m products and m - 1 additions over that mass, a covariance two roundings per
    centred coordinate, three per product, m - 1 additions, the quotient and the floor.  So the bounds are modes_reference.fit_bounds'
    (derived there, next to the function) evaluated per slot on the window's labels:
      prob  (K + m + 8) u * W_i
      mean  2 (m + 6) u * max over the members of |Y[k, s, t, c]|;  without members or mass: 2 (K + 6) u * max over k of |Y|
      cov   2 (m + 8) u * (sum W |c c'| / W_i + var_floor) + (mean bound * unit)^2
    They are meaningful on the taking-part slots; the others hold zeros in both."""
    N, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    n = f64["count"].shape[1]
    per_agent = dict(count=np.repeat(f64["count"], m, 0), prob=np.repeat(f64["prob"], m, 0), label=np.repeat(f64["label"], m, 0),
                     weights=np.repeat(f64["weights"], m, 0), mean=f64["mean"].transpose(0, 2, 1, 3, 4).reshape(N * m, n, T, 2), cov=np.zeros((N * m, n, T, 3)))
    with np.errstate(all="ignore"):
        bp, bm, bc = fit_bounds(Y, per_agent, ux, uy, var_floor, d)
    return (bp.reshape(N, m, n)[:, 0], bm.reshape(N, m, n, T, 2).transpose(0, 2, 1, 3, 4), bc.reshape(N, m, n, T, 3).transpose(0, 2, 1, 3, 4))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def _draw_window(rng, K, m, T, n_true, order, twoseeds, inv, r):
    """Offsets [K, m, T, 2] in normalised units: in every slot each of the n_true scene modes runs along the slot's own direction, 3 r apart at the
    last frame; a world is its mode plus a jitter of two numbers (sigma 0.6 r) that grows with t, the same in every slot."""
    mode = np.concatenate([np.arange(n_true), rng.integers(0, n_true, K - n_true)])
    rng.shuffle(mode)
    if twoseeds and K >= 2:
        mode[order[1]] = mode[order[0]]                                     # the first two seeds lie in one true mode
    th = rng.uniform(0, 2 * np.pi, m)
    direc = np.stack([np.cos(th), np.sin(th)], -1)                          # [m, 2]
    steps = (np.arange(T) + 1.0) / T
    centre = (mode[:, None, None, None] * 3.0 * r) * steps[None, None, :, None] * direc[None, :, None, :]
    z = rng.normal(0, 0.6 * r, (K, 2))
    return (centre + z[:, None, None, :] * (0.25 + 0.75 * steps)[None, None, :, None]) * inv, mode


def make_inputs(d, n, t_end, ux, uy, seed, iters=MODES_MAX_ITERS):
    """Y [R, T, 2] fp32, present [A] uint8, worder [n_scenes, K] int32 (the rank of the world scores: the top n seed the fit), wscore [n_scenes, K]
    fp32 (worlds_reference.planted_world_scores: the grid of 1/64, a tie, a non-finite score), fut [n_scenes, T, mno, 3] fp32 and info.  Every
    window has 1 - 4 scene modes (_draw_window) and is redrawn until the float64 fit of BOTH weightings (uniform, scored) keeps the margin in
    every assign of up to `iters` passes.  max(1, mno / 4) slots of a window are absent (mno >= 2) and filled with garbage hundreds of lengths
    wide -- in Y and, with nonzero ids, in fut: neither may be read --; one window has nobody taking part (two windows or more: the last one, but
    window 0 of two, whose planted score is the non-finite one, so that the other keeps a fit under finite scores); in the first window with
    somebody (info["special"]) one taking-part row of the worst-scored world is a NaN row (K >= 2) and the first two seeds lie in one true mode;
    with three windows or more the order row of window 1 is BAD (info["bad"] = [1]), and info["bad_order"] is the order with the special window's
    row made BAD."""
    N, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    rng = np.random.default_rng(seed)
    r = SCALE_PX
    u2 = np.array([float(np.float32(ux)), float(np.float32(uy))])
    inv = 1.0 / u2
    wscore = planted_world_scores(d, seed)
    worder = _rank(wscore)
    present = np.ones((N, m), np.uint8)
    Yk = np.zeros((N, K, m, T, 2), np.float32)
    modes = np.zeros((N, K), np.int64)
    redraws, nan_at = 0, None
    empty = -1 if N < 2 else (0 if N == 2 else N - 1)
    special = 1 if N == 2 else 0
    for w in range(N):
        if w == empty:
            present[w] = 0
        elif m >= 2:
            present[w, rng.permutation(m)[:max(1, m // 4)]] = 0
        sl = np.nonzero(present[w])[0]
        n_true = int(min(K, 1 + (w + seed) % 4))
        base = rng.uniform(0.3, 0.7, (1, m, 1, 2))
        for attempt in range(200):
            off, mode = _draw_window(rng, K, m, T, n_true, worder[w], w == special, inv, r)
            rows = (base + off).astype(np.float32)
            if w == special and K >= 2:
                nan_at = (w, int(worder[w, -1]), int(sl[-1]))
                rows[nan_at[1], nan_at[2]] = np.nan
            ok = True
            for sc in (None, wscore[w:w + 1]):
                fit = fit_window(rows[:, sl].astype(np.float64), worder[w], world_weights(sc, 1, K, np.float64)[0], n, t_end, iters, ux, uy, 0.0,
                                 np.float64)
                ok = ok and fit["margin"] > MARGIN
            if ok:
                break
            redraws += 1
        else:
            raise AssertionError("the generator could not draw window %d with the margin" % w)
        Yk[w], modes[w] = rows, mode
    gone = present == 0
    garbage = (rng.uniform(-300 * r, 300 * r, (N, K, m, T, 2)) * inv).astype(np.float32)
    Yk = np.where(gone[:, None, :, None, None], garbage, Yk)
    # the ground truth: in every slot the track of one world of the window, nudged; counted except in a few leading or trailing frames
    fut = np.zeros((N, T, m, 3), np.float32)
    for w in range(N):
        k = int(rng.integers(K))
        g = np.nan_to_num(Yk[w, k].astype(np.float64)) + rng.uniform(-0.004, 0.004, (m, 1, 2))      # [m, T, 2]
        fut[w, :, :, 1] = (g[..., 0] / d.sx).T; fut[w, :, :, 2] = (g[..., 1] / d.sy).T
        fut[w, :, :, 0] = np.arange(1, m + 1)[None]
        for s in range(m):
            if s % 3 == 1 and T > 2:
                fut[w, :int(rng.integers(1, max(2, T // 3))), s, 0] = 0
            if s % 5 == 2 and T > 2:
                fut[w, T - int(rng.integers(1, max(2, T // 3))):, s, 0] = 0
    bad = []
    if N >= 3:
        worder = np.array(worder)
        worder[1, 0] = worder[1, n - 1] if n > 1 else -1                    # a repeated entry; one mode: an entry out of range
        bad = [1]
    bad_order = np.array(worder)
    bad_order[special, n - 1] = K
    return (np.ascontiguousarray(Yk.reshape(d.R, T, 2)), np.ascontiguousarray(present.reshape(-1)), np.ascontiguousarray(worder, np.int32),
            wscore, fut, dict(redraws=redraws, windows=N, modes=modes, nan=nan_at, bad=bad, empty=empty, special=special, bad_order=bad_order.astype(np.int32)))


# ---- the shared cases: inputs and references, computed once per process ---------------------------------------------------------------------
_CACHE = {}


def case(shape, unit=1, t_end=None):
    """The inputs of (shape, unit, t_end) and both references under the planted scores and under equal weights, computed once and left unchanged."""
    key = (shape, unit, t_end)
    if key not in _CACHE:
        n_s, m, K, T, n = shape
        d = small_dims(n_scenes=n_s, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64)
        ux, uy = [(1.0, 1.0), (1.0 / d.sx, 1.0 / d.sy)][unit]
        te = T if t_end is None else t_end
        Y, present, worder, wscore, fut, info = make_inputs(d, n, te, ux, uy, seed=5 + unit)
        for a in (Y, present, worder, wscore, fut):
            a.setflags(write=False)
        hz = sorted({max(1, T // 4), max(1, T // 2), T})
        vf = var_floor_of(ux, d.sx)
        c = dict(d=d, n=n, t_end=te, Y=Y, present=present, worder=worder, wscore=wscore, fut=fut, info=info, hz=hz, ux=ux, uy=uy, vf=vf)
        for tag, s in (("scored", wscore), ("uniform", None)):
            c[tag] = {"f32": scene_modes_f32(Y, present, worder, s, fut, n, te, ITERS, ux, uy, vf, d, hz),
                      "f64": scene_modes_f64(Y, present, worder, s, fut, n, te, ITERS, ux, uy, vf, d, hz)}
        _CACHE[key] = c
    return _CACHE[key]
