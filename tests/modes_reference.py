"""Two statements of the mode-fit contract (include/desire_hip.h: desire_fit_modes), the bounds their comparison is held to, the mirror of the
kernel's LDS geometry and the synthetic inputs the tests share.

modes_f32 is the contract as written, operation by operation in numpy fp32 and in its order (every sum over k or t in increasing index from 0,
every operation rounded once).  modes_f64 is the same sequence in float64 on the same fp32 inputs.  Both return a dict: label [A, K], count
[A, n], prob [A, n], mean [A, n, T, 2], cov [A, n, T, 3], passes [A], margin [A] (below) and, with `fut`, frame [A, T] and out [A, n_h, 2].
Agent a = scene * mno + slot, row r = (scene * K + k) * mno + slot.

margin [A]: over every executed assign and every sample with a label, (d2 - d1) / d2 of its smallest and second smallest distance (inf where
there is one mode, or d2 == 0: coincident rows tie exactly in every precision and go to the lower mode).  Labels are compared between precisions
only on inputs whose float64 margin is above MARGIN; the generator redraws an agent until it is."""
import numpy as np

from tests.kde_reference import kde_outputs

MARGIN = 1e-3
MIN_DET_RATIO = np.float32(1e-5)                   # DESIRE_KDE_MIN_DET_RATIO
LOG_FLOOR = -20.0
MODES_MAX, MODES_MAX_ITERS = 16, 32
MIN_STD_PX = 0.5                                   # the floor of the tests: var_floor = (MIN_STD_PX in the call's unit)^2
U = 2.0 ** -24
# (n_scenes, mno, K, T_pred, n_modes)
SHAPES = [(2, 3, 3, 5, 2), (2, 32, 20, 40, 6), (1, 5, 64, 9, 16), (1, 2, 130, 9, 4), (2, 256, 2, 40, 2), (1, 1, 1, 1, 1), (1, 4, 3, 200, 3)]
KINDS = ("zero", "nanrow", "nanlate", "twoseeds", "onehot", "badscore")      # the special agents: slots 1 .. 6 of the first window


# ---- the LDS geometry (desire_amd/csrc/eval_lds.h: ModesLds, modes_geometry) ------------------------------------------------------------------
LDS_BYTES, THREADS = 60 * 1024, 256


def agent_bytes(K, T, n):
    Tp = T | 1
    return 8 * (K + n) * Tp + 12 * n * T + 8 * Tp + 12 * K + 8 * n + 16


def modes_geometry(mno, K, T, n):
    """(SC, G), or None when one agent does not fit."""
    per = agent_bytes(K, T, n)
    if per > LDS_BYTES:
        return None
    g = 1
    while g < K and g < 64:
        g <<= 1
    sc = min(mno, LDS_BYTES // per, max(1, THREADS // g))
    chunks = -(-mno // sc)
    return -(-mno // chunks), g


# ---- the contract -----------------------------------------------------------------------------------------------------------------------------
def _rows(Y, d):
    return np.asarray(Y, np.float32).reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).transpose(0, 2, 1, 3, 4).reshape(d.A, d.K, d.T_pred, 2)


def _scores(score, d):
    return None if score is None else np.asarray(score, np.float32).reshape(d.n_scenes, d.K, d.mno).transpose(0, 2, 1).reshape(d.A, d.K)


def weights(s, K, dt):
    """Step 1 for one agent: s [K] fp32 or None."""
    w = np.full(K, dt(1) / dt(K), dt)
    if s is None or not np.isfinite(s).all():
        return w
    s = s.astype(dt)
    e = np.exp(s - s.max()).astype(dt)
    tot = dt(0)
    for k in range(K):
        tot = dt(tot + e[k])
    return (e / tot).astype(dt)


def _dist(Yk, means, t_end, ux, uy, dt):
    """D [K, n] of the rows Yk [K, T, 2] to the means [n, T, 2]: the sum over t < t_end in increasing t from 0."""
    D = np.zeros((Yk.shape[0], means.shape[0]), dt)
    for t in range(t_end):
        a = (Yk[:, None, t, 0] - means[None, :, t, 0]) * ux
        b = (Yk[:, None, t, 1] - means[None, :, t, 1]) * uy
        D = D + (a * a + b * b)
    return D


def _nearest(D):
    """labels [K] from the distances D [K, n] (strict <: ties to the lower mode; a NaN is never chosen; -1 without a choice) and their margin."""
    K, n = D.shape
    dt = D.dtype.type
    best = np.full(K, -1, np.int32)
    bd = np.zeros(K, dt)
    for i in range(n):
        take = ~np.isnan(D[:, i]) & ((best < 0) | (D[:, i] < bd))
        best[take] = i
        bd[take] = D[take, i]
    margin = np.inf
    if n > 1:
        S = np.sort(np.where(np.isnan(D), np.inf, D), 1)
        two = np.isfinite(S[:, 1]) & (S[:, 1] > 0)
        if two.any():
            margin = float(((S[two, 1] - S[two, 0]) / S[two, 1]).min())
    return best, margin


def _update(Yk, w, label, means, dt):
    n = means.shape[0]
    W = np.zeros(n, dt)
    cnt = np.zeros(n, np.int32)
    for i in range(n):
        acc = np.zeros(Yk.shape[1:], dt)
        tot = dt(0)
        for k in np.nonzero(label == i)[0]:
            tot = dt(tot + w[k])
            acc = acc + w[k] * Yk[k]
            cnt[i] += 1
        W[i] = tot
        if tot > 0:
            means[i] = acc / tot
    return W, cnt


def _cov(Yk, w, label, means, W, ux, uy, vf, dt):
    """cov [n, ..., 3] about the final means [n, ..., 2] of the rows Yk [K, ..., 2]: a mode's members in increasing k; zeros without mass."""
    cov = np.zeros(means.shape[:-1] + (3,), dt)
    for i in range(means.shape[0]):
        if not W[i] > 0:
            continue
        cxx = cyy = cxy = np.zeros(means.shape[1:-1], dt)
        for k in np.nonzero(label == i)[0]:
            cx, cy = (Yk[k, ..., 0] - means[i, ..., 0]) * ux, (Yk[k, ..., 1] - means[i, ..., 1]) * uy
            cxx = cxx + w[k] * (cx * cx); cyy = cyy + w[k] * (cy * cy); cxy = cxy + w[k] * (cx * cy)
        cov[i] = np.stack([cxx / W[i] + vf, cyy / W[i] + vf, cxy / W[i]], -1)
    return cov


def fit(Yk, order, w, n, t_end, iters, ux, uy, var_floor, dt, dist=_dist):
    """The weighted Lloyd iteration and the covariances for one agent (steps 2 - 7) or one window: Yk [K, ..., T, 2] and w [K] in dtype dt, order
    [K] int, dist(Yk, means, t_end, ux, uy, dt) the distances [K, n] of the assignment.  mean [n, ..., T, 2] and cov [n, ..., T, 3]."""
    K = Yk.shape[0]
    seeds = [int(c) for c in order[:n]]
    res = dict(label=np.full(K, -1, np.int32), count=np.zeros(n, np.int32), prob=np.zeros(n, dt), mean=np.zeros((n,) + Yk.shape[1:], dt),
               cov=np.zeros((n,) + Yk.shape[1:-1] + (3,), dt), passes=0, margin=np.inf, bad=True)
    if any(c < 0 or c >= K for c in seeds) or len(set(seeds)) < n:
        return res
    ux, uy, vf = dt(np.float32(ux)), dt(np.float32(uy)), dt(np.float32(var_floor))
    with np.errstate(all="ignore"):
        means = Yk[seeds].copy()
        label, margin = _nearest(dist(Yk, means, t_end, ux, uy, dt))
        p = 0
        while True:
            W, cnt = _update(Yk, w, label, means, dt)
            if p == iters:
                break
            p += 1
            new, m = _nearest(dist(Yk, means, t_end, ux, uy, dt))
            margin = min(margin, m)
            same = np.array_equal(new, label)
            label = new
            if same:
                break
        cov = _cov(Yk, w, label, means, W, ux, uy, vf, dt)
    res.update(label=label, count=cnt, prob=W, mean=means, cov=cov, passes=p, margin=margin, bad=False)
    return res


fit_agent = fit                                    # one agent: Yk [K, T, 2]


def mixture(ls, oks, floor, dt, per=None):
    """The frame values [T] of the mixture: the log-sum-exp over the usable modes (oks[i] [T]) of their ls[i] [T] in increasing i, divided by
    `per` [T] where given; the floor where that is not above it or no mode is usable."""
    M = np.full(ls[0].shape, -np.inf, dt)
    for l, ok in zip(ls, oks):
        M = np.where(ok, np.fmax(M, l), M)
    S = np.zeros(ls[0].shape, dt)
    for l, ok in zip(ls, oks):
        S = np.where(ok, S + np.exp(l - M).astype(dt), S)
    r = (M + np.log(S).astype(dt)).astype(dt)
    if per is not None:
        r = (r / per).astype(dt)
    return np.where(np.any(oks, 0) & (r > floor), r, floor)


def frame_values(res, f, ux, uy, log_floor, sx, sy, dt):
    """Step 8 for one agent: f [T, 3] fp32 (id, x, y) -> the frame values [T]."""
    T = f.shape[0]
    counted = f[:, 0] != 0
    floor = dt(np.float32(log_floor))
    if res["bad"]:
        return np.where(counted, floor, dt(0)).astype(dt)
    ux, uy = dt(np.float32(ux)), dt(np.float32(uy))
    gx, gy = (f[:, 1] * np.float32(sx)).astype(dt), (f[:, 2] * np.float32(sy)).astype(dt)       # the fp32 scaling is part of the inputs
    log2pi = dt(np.float32(1.8378770664093453)) if dt is np.float32 else np.log(2 * np.pi)
    n = res["prob"].shape[0]
    with np.errstate(all="ignore"):
        ls, oks = [], []
        for i in range(n):
            P = res["prob"][i]
            cxx, cyy, cxy = res["cov"][i, :, 0], res["cov"][i, :, 1], res["cov"][i, :, 2]
            det = cxx * cyy - cxy * cxy
            ok = (P > 0) & (det > dt(MIN_DET_RATIO) * cxx * cyy)
            dx, dy = (res["mean"][i, :, 0] - gx) * ux, (res["mean"][i, :, 1] - gy) * uy
            c2 = dt(2) * cxy
            l = np.log(P).astype(dt) + (dt(-0.5) * ((cyy * (dx * dx) - c2 * (dx * dy)) + cxx * (dy * dy))) / det - log2pi - dt(0.5) * np.log(det).astype(dt)
            ls.append(l.astype(dt)); oks.append(ok)
        v = mixture(ls, oks, floor, dt)
    return np.where(counted, v, dt(0)).astype(dt)


def _modes(Y, order, score, fut, n, t_end, iters, ux, uy, var_floor, hz, log_floor, d, dt):
    Yk = _rows(Y, d).astype(dt)
    s = _scores(score, d)
    order = np.asarray(order).reshape(d.A, d.K)
    A, K, T = d.A, d.K, d.T_pred
    out = dict(label=np.zeros((A, K), np.int32), count=np.zeros((A, n), np.int32), prob=np.zeros((A, n), dt), mean=np.zeros((A, n, T, 2), dt),
               cov=np.zeros((A, n, T, 3), dt), passes=np.zeros(A, np.int32), margin=np.zeros(A), weights=np.zeros((A, K), dt))
    f = None if fut is None else np.asarray(fut, np.float32).transpose(0, 2, 1, 3).reshape(A, T, 3)
    if f is not None:
        out["frame"] = np.zeros((A, T), dt)
    for a in range(A):
        w = weights(None if s is None else s[a], K, dt)
        r = fit_agent(Yk[a], order[a], w, n, t_end, iters, ux, uy, var_floor, dt)
        for key in ("label", "count", "prob", "mean", "cov", "passes", "margin"):
            out[key][a] = r[key]
        out["weights"][a] = w
        if f is not None:
            out["frame"][a] = frame_values(r, f[a], ux, uy, log_floor, d.sx, d.sy, dt)
    if f is not None:
        out["out"] = kde_outputs(out["frame"], fut, hz, d, dtype=dt)
    return out


def modes_f32(Y, order, score, fut, n, t_end, iters, ux, uy, var_floor, d, hz=None, log_floor=LOG_FLOOR):
    return _modes(Y, order, score, fut, n, t_end, iters, ux, uy, var_floor, hz, log_floor, d, np.float32)


def modes_f64(Y, order, score, fut, n, t_end, iters, ux, uy, var_floor, d, hz=None, log_floor=LOG_FLOOR):
    return _modes(Y, order, score, fut, n, t_end, iters, ux, uy, var_floor, hz, log_floor, d, np.float64)


# ---- the bounds of |device - modes_f64| under scores (the device's expf is not numpy's: no bits there) ---------------------------------------------
def fit_bounds(Y, f64, ux, uy, var_floor, d):
    """(prob [A, n], mean [A, n, T, 2], cov [A, n, T, 3]): what a correct fp32 evaluation may differ from modes_f64 by, from the contract's operations
    alone, u = 2^-24, m = the members of the mode.
      weight  e_k is an expf within 2 ulp, the sum of K of them carries (K - 1) u, the division one more: (K + 6) u relative.  The error of the
              sum is COMMON to an agent's weights, so it cancels in every ratio below; what stays per weight is 3 u + the division's u.
      prob    m weights and m - 1 additions:                                 (K + m + 8) u * W_i.
      mean    numerator: per term 4 u (weight) + u (product), m - 1 additions; denominator alike; the quotient and the stored value one each:
              2 (m + 6) u * max over the members of |Y[k, t, c]|  (the weighted mean of |y| is at most that).
      cov     c = (y - mean) * unit is two roundings, its product three more, the weight four, the product with it one, then m - 1 additions,
              the denominator (m + 4) u, the quotient and the floor's addition: 2 (m + 8) u * (sum w |c c'| / W + var_floor).  The shift of the
              device's mean against the float64 one enters squared (the first-order term is sum w c = 0): + (mean bound * unit)^2.
      A mode without members or mass keeps a mean: its seed row (exact) or an earlier pass's mean of at most K rows, 2 (K + 6) u * max |Y|."""
    Yk = np.abs(_rows(Y, d).astype(np.float64))
    A, n = f64["count"].shape
    m = f64["count"].astype(np.float64)
    bp = (d.K + m + 8) * U * f64["prob"]
    bm = np.zeros(f64["mean"].shape)
    bc = np.zeros(f64["cov"].shape)
    u2 = np.array([float(np.float32(ux)), float(np.float32(uy))])
    vf = float(np.float32(var_floor))
    rows = _rows(Y, d).astype(np.float64)
    for a in range(A):
        for i in range(n):
            mem = np.nonzero(f64["label"][a] == i)[0]
            if mem.size == 0 or not f64["prob"][a, i] > 0:             # the mean it kept: its seed row (exact), or an earlier pass's mean of at most K rows
                bm[a, i] = 2 * (d.K + 6) * U * np.max(np.nan_to_num(Yk[a]), 0)
                continue
            bm[a, i] = 2 * (mem.size + 6) * U * Yk[a, mem].max(0)
            w = f64["weights"][a, mem][:, None, None]
            c = np.abs(rows[a, mem] - f64["mean"][a, i][None]) * u2
            mag = np.stack([(w * c[..., :1] * c[..., :1]).sum(0)[:, 0], (w * c[..., 1:] * c[..., 1:]).sum(0)[:, 0],
                            (w * c[..., :1] * c[..., 1:]).sum(0)[:, 0]], -1) / f64["prob"][a, i]
            shift = bm[a, i] * u2
            sq = np.stack([shift[:, 0] ** 2, shift[:, 1] ** 2, shift[:, 0] * shift[:, 1]], -1)
            bc[a, i] = 2 * (mem.size + 8) * U * (mag + np.array([vf, vf, 0.0])) + sq
    return bp, bm, bc


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def _draw_agent(rng, K, T, kind):
    """Rows [K, T, 2] float64 on the 1/4096 lattice, the true mode of every sample, and an order whose first entries are one sample per true mode."""
    n_true = int(min(K, rng.integers(1, 5)))
    p0 = rng.uniform(0.3, 0.7, 2)
    ang = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(n_true) / n_true + rng.uniform(-0.3, 0.3, n_true) / n_true
    speed = rng.uniform(0.15, 0.25, n_true)
    steps = (np.arange(T) + 1.0) / T
    centre = p0 + steps[None, :, None] * (speed[:, None] * np.stack([np.cos(ang), np.sin(ang)], -1))[:, None, :]      # [n_true, T, 2]
    tm = np.concatenate([np.arange(n_true), rng.integers(0, n_true, K - n_true)])
    rng.shuffle(tm)
    z = rng.uniform(-0.02, 0.02, (K, 2))                                    # the jitter: two numbers per sample, growing with t
    rows = centre[tm] + z[:, None, :] * (0.25 + 0.75 * steps)[None, :, None]
    rows = np.round(rows * 4096) / 4096
    first = [int(np.nonzero(tm == j)[0][0]) for j in range(n_true)]
    if kind == "twoseeds" and K >= 2:
        same = np.nonzero(tm == tm[first[0]])[0]
        if same.size >= 2:
            first = [int(same[0]), int(same[1])] + [c for c in first[1:] if c != int(same[1])]
    rest = [k for k in rng.permutation(K) if k not in first]
    return rows, tm, np.array(first + rest, np.int32)


def padded_mno(m):
    """The slot axis a handle takes for m objects: the host pads max_num_obj up to a divisor of 32, or to a multiple of 32."""
    return next(x for x in (1, 2, 4, 8, 16, 32) if x >= m) if m <= 32 else -(-m // 32) * 32


def make_inputs(d, n, t_end, ux, uy, seed, iters=MODES_MAX_ITERS, live=None):
    """Y [R, T, 2] fp32, order [A, K] int32, score [n_scenes, K, mno] fp32 (planted on the grid of 1/64), fut [n_scenes, T, mno, 3] fp32 and info
    (kinds [A], redraws, agents).  Every agent is redrawn until the float64 fit of BOTH weightings (uniform, scored) keeps the margin in every
    assign of up to `iters` passes.  The special agents (KINDS) are slots 1 .. 6 of the first window where the shape has them.  Slots from
    `live` on (the padding of a shape whose objects are no valid slot count) are absent: zero rows, zero scores, the identity order, never counted."""
    rng = np.random.default_rng(seed)
    A, K, T = d.A, d.K, d.T_pred
    Yk = np.zeros((A, K, T, 2), np.float32)
    order = np.zeros((A, K), np.int32)
    s = (rng.integers(-128, 129, (A, K)) / 64.0).astype(np.float32)
    live = d.mno if live is None else live
    kinds = [KINDS[a - 1] if 1 <= a <= len(KINDS) and a < live else "plain" for a in range(A)]
    kinds = ["absent" if a % d.mno >= live else k for a, k in enumerate(kinds)]
    redraws = 0
    for a in range(A):
        kind = kinds[a]
        if kind == "absent":
            s[a] = 0; order[a] = np.arange(K)
            continue
        if kind == "onehot":
            s[a] = 0; s[a, int(rng.integers(K))] = 30.0
        if kind == "badscore":
            s[a, int(rng.integers(K))] = np.nan if a % 2 else np.inf
        for attempt in range(200):
            rows, tm, od = _draw_agent(rng, K, T, kind)
            rows = rows.astype(np.float32)
            if kind == "zero":
                rows[:] = 0
            elif kind == "nanrow":
                rows[od[-1]] = np.nan
            elif kind == "nanlate" and t_end < T:
                rows[od[-1], t_end + (T - t_end) // 2, 0] = np.nan
            ok = True
            for sc in (None, s[a]):
                r = fit_agent(rows.astype(np.float64), od, weights(sc, K, np.float64), n, t_end, iters, ux, uy, 0.0, np.float64)
                ok = ok and r["margin"] > MARGIN
            if ok:
                break
            redraws += 1
        else:
            raise AssertionError("the generator could not draw agent %d with the margin" % a)
        Yk[a], order[a] = rows, od
    Y = np.ascontiguousarray(Yk.reshape(d.n_scenes, d.mno, K, T, 2).transpose(0, 2, 1, 3, 4).reshape(d.R, T, 2))
    score = np.ascontiguousarray(s.reshape(d.n_scenes, d.mno, K).transpose(0, 2, 1))
    # the ground truth: a sample's own track nudged, counted except in a few leading or trailing frames; slot mno - 1 of the last window is absent
    fut = np.zeros((d.n_scenes, T, d.mno, 3), np.float32)
    for a in range(A):
        w_, sl = divmod(a, d.mno)
        if kinds[a] == "absent":
            continue
        k = int(rng.integers(K))
        g = np.nan_to_num(Yk[a, k].astype(np.float64)) + rng.uniform(-0.004, 0.004, 2)
        fut[w_, :, sl, 1] = g[:, 0] / d.sx; fut[w_, :, sl, 2] = g[:, 1] / d.sy
        fut[w_, :, sl, 0] = sl + 1
        if a % 3 == 1 and T > 2:
            fut[w_, :int(rng.integers(1, max(2, T // 3))), sl, 0] = 0
        if a % 5 == 2 and T > 2:
            fut[w_, T - int(rng.integers(1, max(2, T // 3))):, sl, 0] = 0
    if A > 2:
        fut[-1, :, -1, 0] = 0
    return Y, order, score, fut, dict(kinds=kinds, redraws=redraws, agents=A)


def var_floor_of(ux, sx):
    """(MIN_STD_PX pixels in the call's unit)^2: unit_x * sx is 1 in pixel units and sx in normalised ones."""
    return float(np.float32((MIN_STD_PX * float(ux) * sx) ** 2))
