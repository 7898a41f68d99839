"""Numpy statement of the joint-metrics contract (include/desire_hip.h: desire_joint_metrics) in two forms -- joint_f32, the contract's fp32
operation sequence, and joint_f64, the same in float64 -- and the input generator their tests share.  Agent a = scene * mno + slot, row
r_k = (scene * K + k) * mno + slot; sample K is the ground truth.  The integer outputs of the two forms can only differ where a pair's q lies
within rounding of r2: the generator keeps every (pair, frame) further than MARGIN * r2 from r2 in float64 (the tests assert it on "margin" of
the float64 pass alone), and draws scores on a grid of 1/64 so that the joint scores are exact sums in either precision."""
import numpy as np

# fp32 rounding of q = a * a + b * b is below 4 * 2^-24 = 2.4e-7 relative; the band is about 4000 times that
MARGIN = 1e-3


def chunk_frames(mno, T):
    """Frames of a (window, k) unit one pass of the kernel's LDS plan holds (include/desire_hip.h): T when the unit fits."""
    stride = mno + 1 if mno >= 32 else mno
    return min(T, (61440 - 8 * mno) // (8 * stride))


def _rank(s):
    """desire_rank_samples' rule on [n, K]: IEEE >, ties to the lower k, NaNs last by index."""
    nan = np.isnan(s)
    key = np.where(nan, -np.inf, s).astype(np.float64)
    k = np.broadcast_to(np.arange(s.shape[1]), s.shape)
    return np.lexsort((k, -key, nan), axis=-1).astype(np.int32)


def _joint(Y, fut, present, score, horizons, n_top, radius, ux, uy, d, dtype):
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    hz = [int(h) for h in horizons]
    f32 = np.float32
    ux, uy, r = dtype(f32(ux)), dtype(f32(uy)), dtype(f32(radius))
    r2 = r * r
    Yk = np.asarray(Y, f32).reshape(n, K, m, T, 2)
    pos = np.full((n, K + 1, m, T, 2), np.nan, dtype)
    pos[:, :K] = Yk
    if fut is not None:
        f = np.asarray(fut, f32)
        c = (f[..., 0] != 0).transpose(0, 2, 1)                            # [n, m, T]
        g = np.stack([f[..., 1] * f32(d.sx), f[..., 2] * f32(d.sy)], -1).astype(f32).transpose(0, 2, 1, 3)      # rounded once in fp32: an input
        pos[:, K] = g
    else:
        c = np.broadcast_to((np.asarray(present).reshape(n, m) != 0)[:, :, None], (n, m, T))
        g = None
    # ---- first contact: the pair rule frame by frame, walking t down so that the smallest t is written last
    first = np.full((n, K + 1, m), T, np.int32)
    touch_any = np.zeros((n, K + 1, m, T), bool)
    off = ~np.eye(m, dtype=bool)
    margin = np.inf
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            x, y = pos[:, :, :, t, 0], pos[:, :, :, t, 1]
            a = x[:, :, :, None] - x[:, :, None, :]
            a = a * ux
            b = y[:, :, :, None] - y[:, :, None, :]
            b = b * uy
            q = a * a + b * b
            both = (c[:, None, :, None, t] & c[:, None, None, :, t]) & off
            touch = both & (q < r2)
            if r2 > 0 and m > 1:
                sel = np.broadcast_to(off, q.shape) & np.isfinite(q)
                if fut is None:
                    sel[:, K] = False
                if sel.any():
                    margin = min(margin, float(np.min(np.abs(q[sel].astype(np.float64) - float(r2)))) / float(r2))
            hit = touch.any(-1)
            if fut is None:
                hit[:, K] = False
            touch_any[..., t] = hit
            first = np.where(hit, np.int32(t), first)
    counted_any = np.stack([c[:, :, :h].any(-1) for h in hz], 1)            # [n, n_h, m]: takes part before h
    cnt = np.zeros((n, K + 1, len(hz), 2), np.int32)
    for hi, h in enumerate(hz):
        cnt[:, :, hi, 0] = (first < h).sum(-1)
        cnt[:, :, hi, 1] = counted_any[:, None, hi].sum(-1)
    if fut is None:
        cnt[:, K] = 0
    res = {"first": first, "cnt": cnt, "touch_any": touch_any, "margin": margin}
    # ---- joint score and its order
    part = c.any(-1)                                                       # [n, m]
    js = np.zeros((n, K), dtype)
    if score is not None:
        s = np.asarray(score, f32).reshape(n, K, m).astype(dtype)
        with np.errstate(all="ignore"):
            for i in range(m):
                js = np.where(part[:, None, i], js + s[:, :, i], js)
    order = _rank(js)
    res["jscore"], res["order"] = js, order
    if fut is None:
        return res
    # ---- per-agent errors (desire_ranked_errors' definitions), then the sums over the slots in increasing slot
    with np.errstate(all="ignore"):
        dx = (Yk[..., 0].astype(dtype) - g[:, None, :, :, 0].astype(dtype)) * ux
        dy = (Yk[..., 1].astype(dtype) - g[:, None, :, :, 1].astype(dtype)) * uy
        e = np.sqrt(dx * dx + dy * dy).astype(dtype)                        # [n, K, m, T]
        ade = np.zeros((n, K, m, len(hz)), dtype)
        fde = np.zeros((n, K, m, len(hz)), dtype)
        sm, last, np_ = np.zeros((n, K, m), dtype), np.zeros((n, K, m), dtype), np.zeros((n, 1, m), np.int64)
        hi = 0
        for t in range(hz[-1]):
            ct = c[:, None, :, t]
            sm = np.where(ct, sm + e[..., t], sm)
            last = np.where(ct, e[..., t], last)
            np_ = np_ + ct
            if t + 1 == hz[hi]:
                ade[..., hi] = np.where(np_ > 0, sm / np.maximum(np_, 1).astype(dtype), 0)
                fde[..., hi] = last
                hi += 1
        jerr = np.zeros((n, K, len(hz), 2), dtype)
        for hi in range(len(hz)):
            sa, sf = np.zeros((n, K), dtype), np.zeros((n, K), dtype)
            for i in range(m):
                tp = counted_any[:, None, hi, i]
                sa = np.where(tp, sa + ade[:, :, i, hi], sa)
                sf = np.where(tp, sf + fde[:, :, i, hi], sf)
            nt = counted_any[:, hi].sum(-1)[:, None]
            jerr[:, :, hi, 0] = np.where(nt > 0, sa / np.maximum(nt, 1).astype(dtype), 0)
            jerr[:, :, hi, 1] = np.where(nt > 0, sf / np.maximum(nt, 1).astype(dtype), 0)
    out = np.zeros((n, len(hz), 4), dtype)
    for w in range(n):
        for hi in range(len(hz)):
            if not counted_any[w, hi].any():
                continue
            top = order[w, :n_top]
            ja, jf = jerr[w, top, hi, 0], jerr[w, top, hi, 1]
            best = [ja[0], jf[0]]
            for v, col in ((ja, 0), (jf, 1)):
                for x in v[1:]:
                    if x < best[col] or np.isnan(x):                        # the minimum keeps a NaN
                        best[col] = x
            out[w, hi] = (ja[0], jf[0], best[0], best[1])
    res.update({"jerr": jerr, "out": out, "ade": ade, "fde": fde, "e_max": float(np.nanmax(np.where(np.isfinite(e), e, 0))) if e.size else 0.0})
    return res


def joint_f32(Y, fut, present, score, horizons, n_top, radius, ux, uy, d):
    return _joint(Y, fut, present, score, horizons, n_top, radius, ux, uy, d, np.float32)


def joint_f64(Y, fut, present, score, horizons, n_top, radius, ux, uy, d):
    return _joint(Y, fut, present, score, horizons, n_top, radius, ux, uy, d, np.float64)


def float_bound(d, e_max):
    """|joint_f32 - joint_f64| of a JADE / JFDE: e carries a few roundings (the difference, two products, the sum, the root: below 4 ulp), a
    sequential sum of n terms at most n ulp of its value, and there are T_pred frames, mno slots and two divisions; every value is at most e_max."""
    return (d.T_pred + d.mno + 8) * 2.0 ** -24 * max(e_max, 1e-30)


def planted_joint_scores(d, seed):
    """[n, K, mno] fp32 on a grid of 1/64 in [-4, 4] -- sums of up to 256 of them are exact in fp32 and float64, so both references rank alike --
    plus, where the shape has room, two joint samples that tie, a NaN and an infinity."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(-256, 257, (d.n_scenes, d.K, d.mno)) / 64.0).astype(np.float32)
    if d.K >= 3:
        s[0, 2] = s[0, 0]                                                  # a tie of joint scores: the lower k first
    if d.K >= 4:
        s[0, 3, 0] = np.nan                                                # (a NaN joint score when slot 0 of window 0 takes part)
    if d.K >= 5:
        s[0, 4, d.mno - 1] = np.inf
    return s


def make_inputs(d, radius, ux, uy, seed, centres=None):
    """Y [R, T_pred, 2] fp32 (normalised units), fut [n, T_pred, mno, 3] fp32 (ids, pixels) and present [A] uint8 whose distances are laid out in
    the caller's unit (ux, uy) around `radius`.  Every slot lives on a lattice 4 radii apart with a jitter below 0.5 radius per sample and a
    small random walk, so nothing touches by itself; then per (window, k) the slots that take part are paired at random and the pairs are
    given, in a cycle that turns with k,
       crossing     j passes i at 0.5 radius per frame, 0.3 radius to the side: they touch at the frames around the centre frame only
                    (`centres`: the centre frames to cycle through; default the middle third);
       follower     j = i + (0.5 radius, 0) in every frame;
       coincident   j = i bit for bit;
       nothing.
    Per window max(1, mno / 8) slots are absent from every frame (zero rows) and as many LEAVE half way (ids 0 from frame max(1, T_pred / 2) on); each of the
    latter sits 0.5 radius from a slot that is otherwise alone at exactly the frames it is not counted in, which must not touch.  One row of
    sample min(1, K - 1) is NaN.  The ground truth has one follower pair.  The last window has nobody in it when there are two or more.
    A unit whose pairs come within 1.5 * MARGIN * r2 of r2 in float64 is drawn again.  Returns (Y, fut, present, info)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    r = float(radius)
    fx, fy = float(np.float32(ux)), float(np.float32(uy))
    side = int(np.ceil(np.sqrt(m)))
    home = np.array([[(i % side) * 4.0 * r, (i // side) * 4.0 * r] for i in range(m)]) + 6.0 * r
    inv = np.array([1.0 / fx, 1.0 / fy])
    rng0 = np.random.default_rng(seed)
    Y = np.zeros((n, K, m, T, 2), np.float32)
    fut = np.zeros((n, T, m, 3), np.float32)
    types = ("cross", "follow", "none", "same", "none")
    n_cross = 0

    def clean(p32, c):
        """p32 [m, T, 2] fp32 normalised: no pair of finite positions within the band of r2 in float64 (and, for the caller, its contacts)."""
        p = p32.astype(np.float64)
        a = (p[:, None, :, 0] - p[None, :, :, 0]) * fx
        b = (p[:, None, :, 1] - p[None, :, :, 1]) * fy
        q = a * a + b * b
        q[np.eye(m, dtype=bool)] = np.inf
        with np.errstate(all="ignore"):
            return not (np.abs(q - r * r) <= 1.5 * MARGIN * r * r).any()

    for w in range(n):
        empty = n >= 2 and w == n - 1
        perm = rng0.permutation(m)
        n_abs = max(1, m // 8) if m >= 2 else 0
        n_par = max(1, m // 8) if m >= 4 else 0
        absent, partial, full = perm[:n_abs], perm[n_abs:n_abs + n_par], perm[n_abs + n_par:]
        ids = np.zeros((T, m), np.float32)
        if not empty:
            ids[:, full] = (full + 1)[None]
            ids[:max(1, T // 2), partial] = (partial + 1)[None]
        for attempt in range(100):                                        # the ground truth of the window
            rng = np.random.default_rng([seed, w, 7777, attempt])
            gt = home[:, None] + np.cumsum(rng.normal(0, 0.02 * r, (m, T, 2)), 1)
            if len(full) >= 3:
                gt[full[1]] = gt[full[0]] + np.array([0.5 * r, 0.0])
            px = (gt * inv / np.array([d.sx, d.sy])).astype(np.float32)    # pixels
            g32 = np.stack([px[..., 0] * np.float32(d.sx), px[..., 1] * np.float32(d.sy)], -1).astype(np.float32)
            if r == 0 or clean(g32, None):
                break
        else:
            raise AssertionError("the ground truth of window %d was not cleared of the band" % w)
        fut[w, :, :, 0] = ids
        fut[w, :, :, 1:] = px.transpose(1, 0, 2)
        for k in range(K):
            for attempt in range(100):
                rng = np.random.default_rng([seed, w, k, attempt])
                p = gt + rng.uniform(-0.5 * r, 0.5 * r, (m, 1, 2)) + np.cumsum(rng.normal(0, 0.03 * r, (m, T, 2)), 1)
                order = rng.permutation(full)
                lonely, nc = [], n_cross
                for pi in range(len(order) // 2):
                    i, j = order[2 * pi], order[2 * pi + 1]
                    kind = types[(pi + k) % len(types)]
                    if kind == "cross" and T >= 3:
                        cs = centres[nc % len(centres)] if centres else int(rng.integers(T // 3, max(T // 3 + 1, (2 * T) // 3)))
                        nc += 1
                        p[j] = p[i] + np.stack([(np.arange(T) - cs) * 0.5 * r, np.full(T, 0.3 * r)], -1)
                    elif kind == "follow":
                        p[j] = p[i] + np.array([0.5 * r, 0.0])
                    elif kind == "same":
                        p[j] = p[i]
                    else:
                        lonely += [i, j]
                for j, i in zip(partial, lonely):                          # near only where j is not counted
                    gone = np.arange(T) >= max(1, T // 2)
                    p[j][gone] = p[i][gone] + np.array([0.0, 0.5 * r])
                p32 = (p * inv).astype(np.float32)
                p32[absent] = 0
                if r == 0 or clean(p32, None):
                    n_cross = nc
                    break
            else:
                raise AssertionError("unit (%d, %d) was not cleared of the band" % (w, k))
            if k == min(1, K - 1) and len(lonely) > len(partial):
                p32[lonely[-1]] = np.nan                                   # a NaN row: never touches, and its errors are reported
            Y[w, k] = p32
    present = np.ascontiguousarray((fut[:, 0, :, 0] != 0).reshape(-1).astype(np.uint8))
    return np.ascontiguousarray(Y.reshape(d.R, T, 2)), fut, present, {"chunk": chunk_frames(m, T)}


def brute_force_first(Y, fut, radius, ux, uy, d):
    """first [n, K + 1, mno] from scipy's pairwise distances frame by frame: an independent statement of the rule (float64 distances; valid on
    inputs that keep the margin)."""
    from scipy.spatial.distance import cdist
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    f = np.asarray(fut, np.float32)
    g = np.stack([f[..., 1] * np.float32(d.sx), f[..., 2] * np.float32(d.sy)], -1).astype(np.float32)     # [n, T, m, 2]
    Yk = np.asarray(Y, np.float32).reshape(n, K, m, T, 2)
    scale = np.array([float(np.float32(ux)), float(np.float32(uy))])
    r = float(np.float32(radius))
    first = np.full((n, K + 1, m), T, np.int32)
    for w in range(n):
        for k in range(K + 1):
            for t in range(T):
                pts = (g[w, t] if k == K else Yk[w, k, :, t]).astype(np.float64) * scale
                c = f[w, t, :, 0] != 0
                ok = c & np.isfinite(pts).all(1)
                idx = np.nonzero(ok)[0]
                if idx.size < 2:
                    continue
                dm = cdist(pts[idx], pts[idx])
                np.fill_diagonal(dm, np.inf)
                for a in idx[(dm < r).any(1)]:
                    if first[w, k, a] == T:
                        first[w, k, a] = t
    return first


# (n_scenes, mno, K, T_pred): the smallest shapes at which each mechanism of the kernel can go wrong
SHAPES = [(2, 8, 3, 7),                 # the plain case, odd T_pred
          (3, 1, 3, 7),                 # no pairs at all; a row boundary falls inside every 16-byte load
          (3, 32, 20, 40),              # the headline's per-window shape
          (2, 160, 4, 9),               # more slots than lanes per frame
          (2, 32, 3, 200),              # long rows
          (2, 256, 2, 40)]              # 82 KB per unit: the frame-chunked walk (28 + 12 frames)
RADIUS_PX = 20.0


def chunk_centres(mno, T):
    """Centre frames of the crossings for a chunked shape: contacts in the first chunk, straddling the chunk border, and in the last chunk alone."""
    tc = chunk_frames(mno, T)
    return None if tc >= T else [tc // 4, tc - 1, tc, min(T - 2, tc + (T - tc) // 2)]
