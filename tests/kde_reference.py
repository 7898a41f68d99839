"""Two statements of the KDE log-likelihood contract (include/desire_hip.h: desire_kde_nll) and the synthetic inputs its tests share.

kde_nll_f64 is the definition: scipy.stats.gaussian_kde(points, weights=w).logpdf in float64 per (agent, frame) on the fp32 inputs.
kde_nll_f32 is the contract as written, operation by operation in fp32 and in its order (every sum over k in increasing k, no fused multiply-add).
Both return the per-frame values [A, T_pred] (0 where a frame is not counted); kde_outputs turns them into the call's [A, n_h, 2].
Agent a = scene * mno + slot, row r = (scene * K + k) * mno + slot."""
import warnings

import numpy as np

MIN_DET_RATIO = 1e-5                               # DESIRE_KDE_MIN_DET_RATIO
LOG_FLOOR = -20.0


def _agents(Y, fut, d):
    """Yk [A, K, T, 2] fp32, f [A, T, 3] fp32 (id, x, y), counted [A, T]."""
    Yk = np.asarray(Y, np.float32).reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).transpose(0, 2, 1, 3, 4).reshape(d.A, d.K, d.T_pred, 2)
    f = np.asarray(fut, np.float32).transpose(0, 2, 1, 3).reshape(d.A, d.T_pred, 3)
    return Yk, f, f[..., 0] != 0


def _scores(score, d):
    return None if score is None else np.asarray(score, np.float32).reshape(d.n_scenes, d.K, d.mno).transpose(0, 2, 1).reshape(d.A, d.K)


def _diffs(Yk, f, ux, uy, d, dtype):
    """d_k [A, K, T, 2]: the fp32 scaling of the ground truth is part of the inputs (desire_ranked_errors' rule), the rest runs in `dtype`."""
    gx = (f[..., 1] * np.float32(d.sx)).astype(dtype); gy = (f[..., 2] * np.float32(d.sy)).astype(dtype)
    u = np.asarray([np.float32(ux), np.float32(uy)], dtype)
    return np.stack([(Yk[..., 0].astype(dtype) - gx[:, None]) * u[0], (Yk[..., 1].astype(dtype) - gy[:, None]) * u[1]], -1)


def weights_f64(score, d):
    """[A, K] float64: softmax of the fp32 scores, 1 / K for an agent with a non-finite score or without scores."""
    w = np.full((d.A, d.K), 1.0 / d.K, np.float64)
    s = _scores(score, d)
    if s is not None:
        s = s.astype(np.float64)
        ok = np.isfinite(s).all(1)
        e = np.exp(s[ok] - s[ok].max(1, keepdims=True))
        w[ok] = e / e.sum(1, keepdims=True)
    return w


def kde_nll_f64(Y, fut, score, ux, uy, log_floor, d, want_shape=False):
    """Per-frame values [A, T] float64 from scipy.  A frame whose weighted covariance is not finite or is singular in the contract's sense
    (det <= MIN_DET_RATIO * Cxx * Cyy), or on which scipy raises, is the floor.  want_shape: also 1 - rho^2 of every frame (nan where it has
    none) and the unclipped log-density (-inf for a degenerate frame)."""
    from scipy.stats import gaussian_kde
    Yk, f, counted = _agents(Y, fut, d)
    D = _diffs(Yk, f, ux, uy, d, np.float64)
    w = weights_f64(score, d)
    val = np.zeros((d.A, d.T_pred), np.float64)
    shape = np.full((d.A, d.T_pred), np.nan); raw = np.full((d.A, d.T_pred), -np.inf)
    origin = np.zeros((2, 1))
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for a, t in zip(*np.nonzero(counted)):
            pts = D[a, :, t].T                                     # [2, K]
            val[a, t] = log_floor
            if d.K < 2:
                continue
            try:
                kde = gaussian_kde(pts, weights=w[a])
            except (np.linalg.LinAlgError, ValueError):
                continue
            C = kde.covariance / kde.factor ** 2                  # numpy's cov(aweights = w), as scipy fitted it
            det = C[0, 0] * C[1, 1] - C[0, 1] * C[0, 1]
            if not np.isfinite(C).all() or not det > MIN_DET_RATIO * C[0, 0] * C[1, 1]:
                continue
            shape[a, t] = det / (C[0, 0] * C[1, 1])
            raw[a, t] = kde.logpdf(origin)[0]
            if raw[a, t] > log_floor:
                val[a, t] = raw[a, t]
    return (val, shape, raw) if want_shape else val


def kde_nll_f32(Y, fut, score, ux, uy, log_floor, d):
    """Per-frame values [A, T] float32: the contract in its stated order of operations."""
    f32 = np.float32
    Yk, f, counted = _agents(Y, fut, d)
    D = _diffs(Yk, f, ux, uy, d, f32)
    K = d.K
    zero = np.zeros(d.A, f32)
    w = np.full((d.A, K), f32(1) / f32(K), f32)
    s = _scores(score, d)
    with np.errstate(all="ignore"):
        if s is not None:
            ok = np.isfinite(s).all(1)
            mx = s.max(1)
            e = np.exp((s - mx[:, None]).astype(f32)).astype(f32)
            tot = zero.copy()
            for k in range(K):
                tot = tot + e[:, k]
            w = np.where(ok[:, None], e / tot[:, None], w).astype(f32)
        den, s2 = zero.copy(), zero.copy()
        for k in range(K):
            den = den + w[:, k] * (f32(1) - w[:, k])
            s2 = s2 + w[:, k] * w[:, k]
        den = np.where((w == f32(1)).any(1), f32(0), den)         # a weight of exactly 1: degenerate
        h2 = np.power(f32(1) / s2, f32(-1.0) / f32(3.0)).astype(f32)
        W = w[:, :, None]                                          # [A, K, 1] against [A, K, T]
        dx, dy = D[..., 0], D[..., 1]
        zt = np.zeros((d.A, d.T_pred), f32)
        mx_, my_ = zt.copy(), zt.copy()
        for k in range(K):
            mx_ = mx_ + W[:, k] * dx[:, k]; my_ = my_ + W[:, k] * dy[:, k]
        cxx, cyy, cxy = zt.copy(), zt.copy(), zt.copy()
        for k in range(K):
            cx, cy = dx[:, k] - mx_, dy[:, k] - my_
            cxx = cxx + W[:, k] * (cx * cx); cyy = cyy + W[:, k] * (cy * cy); cxy = cxy + W[:, k] * (cx * cy)
        cxx, cyy, cxy = cxx / den[:, None], cyy / den[:, None], cxy / den[:, None]
        det = cxx * cyy - cxy * cxy
        good = (den[:, None] > 0) & (det > f32(MIN_DET_RATIO) * cxx * cyy)
        dd = det * h2[:, None]; c2 = f32(2) * cxy
        q = np.stack([(f32(-0.5) * ((cyy * (dx[:, k] * dx[:, k]) - c2 * (dx[:, k] * dy[:, k])) + cxx * (dy[:, k] * dy[:, k]))) / dd
                      for k in range(K)], 1).astype(f32)
        M = q.max(1)
        S = zt.copy()
        for k in range(K):
            S = S + W[:, k] * np.exp(q[:, k] - M).astype(f32)
        l = M + np.log(S).astype(f32) - np.log(f32(2 * np.pi)).astype(f32) - f32(0.5) * np.log(det).astype(f32) - np.log(h2).astype(f32)[:, None]
        l = l.astype(f32)
        val = np.where(good & (l > f32(log_floor)), l, f32(log_floor)).astype(f32)
    return np.where(counted, val, f32(0)).astype(f32)


def kde_outputs(frame, fut, horizons, d, dtype=np.float64):
    """[A, n_h, 2] = (-(mean of the frame values over the counted t < h, summed in increasing t), -(the value at the last counted t < h))."""
    counted = (np.asarray(fut)[..., 0] != 0).transpose(0, 2, 1).reshape(d.A, d.T_pred)
    out = np.zeros((d.A, len(horizons), 2), dtype)
    fr = np.asarray(frame, dtype)
    for a in range(d.A):
        for hi, h in enumerate(horizons):
            idx = np.nonzero(counted[a, :h])[0]
            if idx.size == 0:
                continue
            tot = dtype(0)
            for t in idx:
                tot = dtype(tot + fr[a, t])
            out[a, hi] = (-(tot / dtype(idx.size)), -fr[a, idx[-1]])
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _shape_and_logp(Dn, w, h2):
    """float64 closed form on differences [F, K, 2] in normalised units: (1 - rho^2, log-density at the origin).  Only the input maker uses
    it, to choose frames; no test compares against it."""
    m = (w[..., None] * Dn).sum(1)
    c = Dn - m[:, None]
    den = 1.0 - (w * w).sum(1)
    C = np.einsum("fk,fki,fkj->fij", w, c, c) / den[:, None, None]
    det = C[:, 0, 0] * C[:, 1, 1] - C[:, 0, 1] ** 2
    q = -0.5 * (C[:, None, 1, 1] * Dn[..., 0] ** 2 - 2 * C[:, None, 0, 1] * Dn[..., 0] * Dn[..., 1] + C[:, None, 0, 0] * Dn[..., 1] ** 2) \
        / (det * h2)[:, None]
    M = q.max(1)
    lp = M + np.log((w * np.exp(q - M[:, None])).sum(1)) - np.log(2 * np.pi) - 0.5 * np.log(det) - np.log(h2)
    return det / (C[:, 0, 0] * C[:, 1, 1]), lp


def make_samples(d, fut, score, seed, spread=0.01, min_shape=0.1, worst_log_unit=None, log_floor=LOG_FLOOR, plant=True):
    """Y [R, T, 2] fp32 = g + (a per-(agent, frame) random 2 x 2 map of K standard normals) + an offset, in normalised units, and planted [A, T]
    bool.  A frame is redrawn until 1 - rho^2 >= min_shape under equal weights and under softmax(score), and -- with worst_log_unit = the
    largest log(unit_x * unit_y) a test uses -- until its log-density in those units stays a unit above the floor: the unplanted frames are then
    well conditioned and unclipped.  Planted (K >= 3, at most a tenth of the counted frames): frames whose ground truth lies about 50 bandwidths
    from the samples, an agent with coincident samples and one with equal y (single frames of them in a shape too small for whole agents)."""
    rng = np.random.default_rng(seed)
    A, K, T = d.A, d.K, d.T_pred
    f = np.asarray(fut, np.float32).transpose(0, 2, 1, 3).reshape(A, T, 3)
    g = np.stack([f[..., 1] * np.float32(d.sx), f[..., 2] * np.float32(d.sy)], -1).astype(np.float64)      # [A, T, 2]
    ws = [weights_f64(None, d)] + ([weights_f64(score, d)] if score is not None else [])
    Dn = np.zeros((A * T, K, 2))
    todo = np.ones(A * T, bool)
    for _ in range(200):
        n = int(todo.sum())
        if n == 0 or K < 3:
            break
        z = rng.standard_normal((n, K, 2))
        m = rng.standard_normal((n, 2, 2)) * spread
        off = rng.uniform(-0.5, 0.5, (n, 1, 2)) * spread
        Dn[todo] = np.einsum("fij,fkj->fki", m, z) + off
        bad = np.zeros(n, bool)
        for w in ws:
            wf = np.repeat(w, T, 0)[todo]
            sh, lp = _shape_and_logp(Dn[todo], wf, (wf * wf).sum(1) ** (1.0 / 3.0))
            bad |= ~(sh >= min_shape)
            if worst_log_unit is not None:
                bad |= ~(lp - worst_log_unit >= log_floor + 1.0)
        idx = np.nonzero(todo)[0]
        todo[idx[~bad]] = False
    if K < 3:                                                     # K = 1, 2: every frame is degenerate whatever is drawn
        Dn = rng.standard_normal((A * T, K, 2)) * spread
    else:
        assert not todo.any(), "the input maker could not draw well-conditioned frames"
    Dn = Dn.reshape(A, T, K, 2)
    planted = np.zeros((A, T), bool)
    counted = f[..., 0] != 0
    if plant and K >= 3:
        # at most a tenth of the counted frames is planted: whole agents where the shape has room for them, single frames where it has not
        left = int(counted.sum()) // 10
        agents = np.nonzero(counted.any(1))[0]
        picks = [agents[-2], agents[len(agents) // 2]] if len(agents) >= 4 else []
        for kind, a in enumerate(picks):
            ts = np.arange(T) if A >= 32 else np.nonzero(counted[a])[0][:1]
            cost = int(counted[a, ts].sum())
            if cost > left - 1:                                   # (one frame is kept for the far ground truth)
                continue
            if kind == 0:
                Dn[a, ts] = Dn[a, ts][:, :1]                      # coincident samples
            else:
                Dn[a, ts, :, 1] = Dn[a, ts][:, :1, 1]             # equal y
            planted[a, ts] = True
            left -= cost
        free = np.nonzero((counted & ~planted).reshape(-1))[0]
        far = rng.choice(free, min(left, max(1, int(counted.sum()) // 25)), replace=False)
        fa, ft = np.unravel_index(far, (A, T))
        Dn[fa, ft] += 50.0 * spread * np.array([3.0, -2.0])       # the samples keep their spread: the ground truth is ~ 50 bandwidths off
        planted[fa, ft] = True
    Yk = (g[:, :, None] + Dn).transpose(0, 2, 1, 3)               # [A, K, T, 2]
    Y = Yk.reshape(d.n_scenes, d.mno, K, T, 2).transpose(0, 2, 1, 3, 4).reshape(d.R, T, 2)
    return np.ascontiguousarray(Y, np.float32), planted
