"""Numpy statement of the selection contract (include/desire_hip.h: desire_select_diverse) in two forms -- select_f32, the contract's fp32
operation sequence, and select_f64, the same pass in float64 -- and the input generator their tests share.  Agent a = scene * mno + slot, row
r_k = (scene * K + k) * mno + slot.  The order and count of the two forms can only differ where a pair's distance lies within rounding of the
radius: the generator keeps every pair, for every (metric, t_end) under test, further than MARGIN * radius from the radius (margin())."""
import numpy as np

DIST_FINAL, DIST_MEAN, DIST_MAX = 0, 1, 2
METRICS = (DIST_FINAL, DIST_MEAN, DIST_MAX)
# fp32 rounding of a 200-frame sum of square roots is below 2^-24 * 200 = 1.2e-5 relative; the band is about 80 times that
MARGIN = 1e-3


def _agents(Y, d, dtype):
    return np.asarray(Y, np.float32).reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).transpose(0, 2, 1, 3, 4).reshape(d.A, d.K, d.T_pred, 2).astype(dtype)


def _scores(score, d):
    return None if score is None else np.asarray(score, np.float32).reshape(d.n_scenes, d.K, d.mno).transpose(0, 2, 1).reshape(d.A, d.K)


def _pair_values(Ya, metric, t_end, ux, uy, dtype):
    ux, uy = dtype(np.float32(ux)), dtype(np.float32(uy))
    X, Yc = np.ascontiguousarray(Ya[..., 0]), np.ascontiguousarray(Ya[..., 1])

    def q(t):
        a = X[:, :, None, t] - X[:, None, :, t]
        a *= ux
        a *= a
        b = Yc[:, :, None, t] - Yc[:, None, :, t]
        b *= uy
        b *= b
        a += b
        return a

    with np.errstate(all="ignore"):
        if metric == DIST_FINAL:
            return q(t_end - 1)
        if metric == DIST_MAX:
            m = q(0)
            for t in range(1, t_end):
                v = q(t)
                m = np.where((v > m) | np.isnan(v), v, m)
            return m
        s = np.zeros(X.shape[:2] + X.shape[1:2], dtype)
        for t in range(t_end):
            v = q(t)
            np.sqrt(v, out=v)
            s += v
        s /= dtype(t_end)
        return s


def pair_values(Y, metric, t_end, ux, uy, d, dtype):
    """[A, K, K] in dtype: what the contract compares -- FINAL: q at frame t_end - 1; MAX: the largest q over t < t_end (a NaN stays); MEAN: the
    mean over t < t_end of sqrt(q).  Every operation is one numpy operation in dtype, sums and maxima in increasing t."""
    return _pair_values(_agents(Y, d, dtype), metric, t_end, ux, uy, dtype)


def near_of_values(v, metric, radius):
    r = v.dtype.type(np.float32(radius))
    with np.errstate(all="ignore"):
        return v < (r if metric == DIST_MEAN else r * r)


def near_matrix(Y, metric, t_end, radius, ux, uy, d, dtype):
    return near_of_values(pair_values(Y, metric, t_end, ux, uy, d, dtype), metric, radius)


def _distances(v, metric):
    return v if metric == DIST_MEAN else np.sqrt(v)


def distances_f64(Y, metric, t_end, ux, uy, d):
    """[A, K, K] float64 distances in the caller's unit (the square root of the FINAL / MAX values)."""
    return _distances(pair_values(Y, metric, t_end, ux, uy, d, np.float64), metric)


def margin_of_values(v64, metric, radius):
    """min over the pairs k != k' of every agent of |distance - radius| / radius, from float64 pair_values alone."""
    K = v64.shape[1]
    off = ~np.eye(K, dtype=bool)
    if not off.any():
        return np.inf
    r = float(np.float32(radius))
    return float(np.min(np.abs(_distances(v64, metric)[:, off] - r)) / r)


def margin(Y, metric, t_end, radius, ux, uy, d):
    return margin_of_values(pair_values(Y, metric, t_end, ux, uy, d, np.float64), metric, radius)


def weights(score, d, dtype):
    """[A, K]: desire_kde_nll's step 1.  float32: the stated sequence (sum in increasing k); float64: the same in float64."""
    K = d.K
    w = np.full((d.A, K), dtype(1) / dtype(K), dtype)
    s = _scores(score, d)
    if s is None:
        return w
    with np.errstate(all="ignore"):
        ok = np.isfinite(s).all(1)
        s = s.astype(dtype)
        e = np.exp((s - s.max(1)[:, None]).astype(dtype)).astype(dtype)
        tot = np.zeros(d.A, dtype)
        for k in range(K):
            tot = tot + e[:, k]
        return np.where(ok[:, None], e / tot[:, None], w).astype(dtype)


def _select(Y, order, score, metric, t_end, radius, ux, uy, d, dtype, values=None):
    A, K = d.A, d.K
    order = np.asarray(order, np.int64).reshape(A, K)
    near = near_of_values(pair_values(Y, metric, t_end, ux, uy, d, dtype) if values is None else values, metric, radius)
    w = weights(score, d, dtype)
    rows = np.arange(A)
    kept_idx = np.full((A, K), K, np.int64)                # by sample index: its keeping number, K = not kept
    count = np.zeros(A, np.int64)
    owner = np.zeros((A, K), np.int64)                     # by processing position j: the keeping number of its owner (its own when kept)
    is_kept = np.zeros((A, K), bool)                       # by processing position
    mass = np.zeros((A, K), dtype)
    for j in range(K):
        k = order[:, j]
        cand = np.where(near[rows, k, :], kept_idx, K)     # the keeping numbers of the kept samples it is near
        first = cand.min(1)
        keep = first == K
        own = np.where(keep, count, first)
        kept_idx[rows[keep], k[keep]] = count[keep]
        owner[:, j], is_kept[:, j] = own, keep
        mass[rows, own] = mass[rows, own] + w[rows, k]     # processing order, from 0
        count = count + keep
    out = np.zeros((A, K), np.int32)
    for a in range(A):
        out[a] = np.concatenate([order[a, is_kept[a]], order[a, ~is_kept[a]]])
    return {"order": out, "count": count.astype(np.int32), "owner": owner.astype(np.int32), "kept": is_kept, "mass": mass}


def select_f32(Y, order, score, metric, t_end, radius, ux, uy, d, values=None):
    """values: pair_values(..., np.float32) of the same arguments, where the caller has them already."""
    return _select(Y, order, score, metric, t_end, radius, ux, uy, d, np.float32, values)


def select_f64(Y, order, score, metric, t_end, radius, ux, uy, d, values=None):
    """values: pair_values(..., np.float64) of the same arguments, where the caller has them already (the margin check)."""
    return _select(Y, order, score, metric, t_end, radius, ux, uy, d, np.float64, values)


def cases_of(d):
    """The (metric, t_end) pairs the tests run on a shape: every metric at t_end = 1, a middle frame and T_pred.  Where the reference's [A, K, K]
    arrays are large (over 10^6 pairs) a covering choice instead of the product: every metric and every t_end still occurs."""
    one, mid, T = 1, max(1, (d.T_pred + 1) // 2), d.T_pred
    if d.A * d.K * d.K > 1000000:
        return [(DIST_FINAL, T), (DIST_MEAN, mid), (DIST_MAX, one), (DIST_MAX, T)]
    return [(m, t) for m in METRICS for t in sorted({one, mid, T})]


def make_inputs(d, radius, ux, uy, seed, cases=None, absent=True):
    """Y [R, T_pred, 2] fp32 in normalised units whose distances are laid out in the caller's unit (ux, uy) around `radius`.  Per agent a mix of
       modes   cluster centres on a lattice 6 radii apart, jitter <= radius / 4 per coordinate and frame: all near their centre's members;
       chains  three samples spaced 0.7 radius along a line: A-B and B-C are near, A-C is not, so the outcome depends on the score order;
       scatter uniform over about 6 radii, futures a random walk.
    The last slot of the first window is absent (all rows zero) where the shape has room.  Every pair of every (metric, t_end) of `cases` is then
    held further than MARGIN * radius from the radius by redrawing a scatter sample of each offending pair.  Returns (Y, kind [A, K]: 0 mode,
    1 chain, 2 scatter)."""
    rng = np.random.default_rng(seed)
    A, K, T = d.A, d.K, d.T_pred
    cases = cases_of(d) if cases is None else cases
    r = float(radius)
    kind = np.full((A, K), 2, np.int64)
    off = np.zeros((A, K, T, 2))                            # offsets in the caller's unit, on top of the agent's own walk

    def scatter(n):
        return rng.uniform(-3 * r, 3 * r, (n, 1, 2)) + np.cumsum(rng.normal(0, 0.15 * r, (n, T, 2)), 1)

    for a in range(A):
        perm = rng.permutation(K)
        if K >= 8:
            n_chain, n_mode = 3, max(2, (2 * K) // 5)
        elif K >= 3:
            n_chain, n_mode = (3, 0) if a % 3 == 0 else ((0, K - 1) if a % 3 == 1 else (0, 0))
        else:
            n_chain, n_mode = 0, (K if a % 2 == 0 else 0)
        off[a] = scatter(K)
        cells = rng.permutation(9)                          # lattice cells 6 radii apart: the modes' centres and the chain's
        n_clusters = 1 if n_mode < 4 else (2 if n_mode < 7 else 3)
        for i in range(n_mode):
            k = perm[i]
            c = cells[i % n_clusters]
            centre = np.array([c // 3 - 1, c % 3 - 1], float) * 6 * r
            off[a, k] = centre + rng.uniform(-r / 4, r / 4, (T, 2))
            kind[a, k] = 0
        if n_chain:
            c = cells[n_clusters]
            centre = np.array([c // 3 - 1, c % 3 - 1], float) * 6 * r
            th = rng.uniform(0, 2 * np.pi)
            for i in range(n_chain):
                k = perm[n_mode + i]
                off[a, k] = centre + (i - 1) * 0.7 * r * np.array([np.cos(th), np.sin(th)])
                kind[a, k] = 1
    base = rng.uniform(0.3, 0.7, (A, 1, 1, 2)) + np.cumsum(rng.normal(0, 0.004, (A, 1, T, 2)), 2)
    inv = np.array([1.0 / float(np.float32(ux)), 1.0 / float(np.float32(uy))])
    absent_a = d.mno - 1 if (absent and d.mno >= 2) else -1

    def pack(o):
        Ya = (base + o * inv).astype(np.float32)
        if absent_a >= 0:
            Ya[absent_a] = 0
        return np.ascontiguousarray(Ya.reshape(d.n_scenes, d.mno, K, T, 2).transpose(0, 2, 1, 3, 4).reshape(d.R, T, 2))

    if not cases:                                           # (timing inputs: the layout alone)
        return pack(off), kind
    eye = np.eye(K, dtype=bool)
    todo = np.arange(A)                                     # agents whose pairs have not been cleared yet
    for _ in range(200):
        Ya = (base[todo] + off[todo] * inv).astype(np.float32).astype(np.float64)
        bad = _in_band(Ya, cases, r, ux, uy) & ~eye
        if absent_a >= 0:
            bad[todo == absent_a] = False
        for i, k, k2 in zip(*np.nonzero(np.triu(bad))):
            a = todo[i]
            pick = k2 if kind[a, k2] == 2 else k
            if kind[a, pick] != 2:
                raise AssertionError("two structured samples of agent %d lie in the band: the generator's layout is broken" % a)
            off[a, pick] = scatter(1)[0]
        todo = todo[bad.any((1, 2))]
        if todo.size == 0:
            return pack(off), kind
    raise AssertionError("the redraw did not converge")


def _in_band(Ya, cases, r, ux, uy):
    """[A', K, K]: the pairs whose float64 distance lies within 1.5 * MARGIN * r of r for one of the cases; one walk over the frames serves them all."""
    X, Yc = np.ascontiguousarray(Ya[..., 0]), np.ascontiguousarray(Ya[..., 1])
    ux, uy, r = float(np.float32(ux)), float(np.float32(uy)), float(np.float32(r))
    want = {}
    for metric, t_end in cases:
        want.setdefault(t_end, set()).add(metric)
    shape = X.shape[:2] + X.shape[1:2]
    bad, mx, sm = np.zeros(shape, bool), None, np.zeros(shape)
    for t in range(max(want)):
        a = (X[:, :, None, t] - X[:, None, :, t]) * ux
        b = (Yc[:, :, None, t] - Yc[:, None, :, t]) * uy
        dist = np.sqrt(a * a + b * b)
        mx = dist if mx is None else np.maximum(mx, dist)
        sm = sm + dist
        for metric in want.get(t + 1, ()):
            v = dist if metric == DIST_FINAL else (mx if metric == DIST_MAX else sm / (t + 1))
            bad |= np.abs(v - r) <= 1.5 * MARGIN * r
    return bad


def brute_force(near_a, order_a):
    """The greedy pass of one agent in plain Python from its near matrix [K, K]: (order out, count, owner by position)."""
    kept, owner, kept_pos, owned_pos = [], [], [], []
    for j, k in enumerate(order_a):
        hit = [i for i, kk in enumerate(kept) if near_a[k][kk]]
        if hit:
            owner.append(hit[0]); owned_pos.append(k)
        else:
            owner.append(len(kept)); kept.append(k); kept_pos.append(k)
    return kept_pos + owned_pos, len(kept), owner
