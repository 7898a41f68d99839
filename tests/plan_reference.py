"""Numpy statement of the plan-risk contract (include/desire_hip.h: desire_plan_risk) in two forms -- plan_f32, the contract's fp32 operation
sequence, and plan_f64, the same in float64 -- an independent statement of its distance rule (brute_force_first, scipy's cdist) and the input
generator their tests share.  Layouts are desire_joint_metrics' (tests/joint_reference.py); plans [n, M, T_pred, 2] are normalised coordinates and
ego [n, M] names the slot a plan replaces.  The integer outputs of the two forms can only differ where a q lies within rounding of r2: the
generator keeps every (plan, slot, frame) further than MARGIN * r2 from r2 in float64 (the tests assert it on "margin" of the float64 pass
alone), and the scores are joint_reference.planted_joint_scores' (a grid of 1/64: the joint scores are exact sums in either precision)."""
import numpy as np

from tests.joint_reference import MARGIN, chunk_centres, planted_joint_scores
from tests.joint_reference import make_inputs as joint_inputs

__all__ = ["MARGIN", "KINDS", "SHAPES", "RADIUS_PX", "plan_geometry", "plan_centres", "plan_f32", "plan_f64", "brute_force_first", "make_inputs",
           "planted_joint_scores", "equal_joint_scores", "risk_bound"]

LDS_BYTES, THREADS, HZ, MAX_PC = 61440, 256, 8, 32


def plan_geometry(mno, T, M):
    """(PC, TC) of desire_amd/csrc/eval_lds.h: plan_geometry -- the plans of a workgroup and the frames of one pass of its LDS plan."""
    chunks = lambda n, per: -(-n // per)
    cap = min(M, MAX_PC, max(1, THREADS // mno))
    pc = chunks(M, chunks(M, cap))
    stride = mno + 1 if mno >= 32 else mno
    fixed = 8 * pc + 4 * 2 * pc * (1 + HZ)
    return pc, min(T, (LDS_BYTES - fixed) // (8 * (pc + stride)))


def plan_centres(mno, T, M):
    """Centre frames of the crossing plans for a chunked shape: contacts in the first pass, straddling the border, and in the last pass alone."""
    tc = plan_geometry(mno, T, M)[1]
    return None if tc >= T else [tc // 4, tc - 1, tc, min(T - 2, tc + (T - tc) // 2)]


def _plan(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d, dtype):
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    hz = [int(h) for h in horizons]
    f32 = np.float32
    ux, uy, r = dtype(f32(ux)), dtype(f32(uy)), dtype(f32(radius))
    r2 = r * r
    P = np.asarray(plans, f32).astype(dtype)
    M = P.shape[1]
    pos = np.full((n, K + 1, m, T, 2), np.nan, dtype)
    pos[:, :K] = np.asarray(Y, f32).reshape(n, K, m, T, 2)
    if fut is not None:
        f = np.asarray(fut, f32)
        c = (f[..., 0] != 0).transpose(0, 2, 1)                            # [n, m, T]
        pos[:, K] = np.stack([f[..., 1] * f32(d.sx), f[..., 2] * f32(d.sy)], -1).astype(f32).transpose(0, 2, 1, 3)
    else:
        c = np.broadcast_to((np.asarray(present).reshape(n, m) != 0)[:, :, None], (n, m, T))
    e = np.full((n, M), -1, np.int64) if ego is None else np.asarray(ego, np.int64).reshape(n, M)
    kept = e[:, :, None] != np.arange(m)[None, None]                       # [n, M, m]: the slot is not the one the plan replaces
    first_slot = np.full((n, M, K + 1, m), T, np.int32)
    mn = np.full((n, M, K + 1, m), np.inf, dtype)
    clear = np.full((n, M, K + 1, len(hz)), np.inf, dtype)
    margin, hi = np.inf, 0
    with np.errstate(all="ignore"):
        for t in range(T):
            a = P[:, :, None, None, t, 0] - pos[:, None, :, :, t, 0]
            a = a * ux
            b = P[:, :, None, None, t, 1] - pos[:, None, :, :, t, 1]
            b = b * uy
            q = a * a + b * b                                              # [n, M, K + 1, m]
            ok = c[:, None, None, :, t] & kept[:, :, None, :]
            touch = ok & (q < r2)
            first_slot = np.where(touch & (first_slot == T), np.int32(t), first_slot)
            mn = np.where(ok & (q < mn), q, mn)
            if r2 > 0:
                sel = np.broadcast_to(ok, q.shape) & np.isfinite(q)
                if fut is None:
                    sel = sel.copy()
                    sel[:, :, K] = False
                if sel.any():
                    margin = min(margin, float(np.min(np.abs(q[sel].astype(np.float64) - float(r2)))) / float(r2))
            if hi < len(hz) and t + 1 == hz[hi]:
                clear[..., hi] = mn.min(-1)
                hi += 1
    if fut is None:
        first_slot[:, :, K] = T
        clear[:, :, K] = np.inf
    first = first_slot.min(-1).astype(np.int32)
    # ---- the weights of the K joint futures
    part = c.any(-1)
    js = np.zeros((n, K), dtype)
    W = np.full((n, K), dtype(1) / dtype(K), dtype)
    if score is not None:
        s = np.asarray(score, f32).reshape(n, K, m).astype(dtype)
        with np.errstate(all="ignore"):
            for i in range(m):
                js = np.where(part[:, None, i], js + s[:, :, i], js)
            for w in range(n):
                if not np.isfinite(js[w]).all():
                    continue
                ek = np.exp(js[w] - js[w].max()).astype(dtype)
                tot = dtype(0)
                for k in range(K):
                    tot = dtype(tot + ek[k])
                W[w] = ek / tot
    hzv = np.asarray(hz)
    risk = np.zeros((n, M, len(hz)), dtype)
    blame = np.zeros((n, M, len(hz), m), dtype)
    for k in range(K):
        wk = W[:, k]
        risk = np.where(first[:, :, k, None] < hzv[None, None], risk + wk[:, None, None], risk).astype(dtype)
        blame = np.where(first_slot[:, :, k, None, :] < hzv[None, None, :, None], blame + wk[:, None, None, None], blame).astype(dtype)
    return {"first": first, "clear": clear, "risk": risk, "blame": blame, "first_slot": first_slot, "W": W, "jscore": js, "margin": margin}


def plan_f32(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d):
    return _plan(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d, np.float32)


def plan_f64(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d):
    return _plan(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d, np.float64)


def risk_bound(d):
    """|device - plan_f64| of a risk or blame entry: a sum of K weights, each one expf of a few ulp over a sum of K terms and one division, on
    values of 1 at most."""
    return (d.K + 8) * 2.0 ** -24


def brute_force_first(Y, fut, plans, ego, radius, ux, uy, d):
    """first [n, M, K + 1] from scipy's distances between the plans and the slots frame by frame: an independent statement of the rule (float64
    distances; valid on inputs that keep the margin)."""
    from scipy.spatial.distance import cdist
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    f = np.asarray(fut, np.float32)
    g = np.stack([f[..., 1] * np.float32(d.sx), f[..., 2] * np.float32(d.sy)], -1).astype(np.float32)     # [n, T, m, 2]
    Yk = np.asarray(Y, np.float32).reshape(n, K, m, T, 2)
    P = np.asarray(plans, np.float32)
    M = P.shape[1]
    e = np.full((n, M), -1) if ego is None else np.asarray(ego).reshape(n, M)
    scale = np.array([float(np.float32(ux)), float(np.float32(uy))])
    r = float(np.float32(radius))
    first = np.full((n, M, K + 1), T, np.int32)
    for w in range(n):
        for k in range(K + 1):
            for t in range(T):
                pts = (g[w, t] if k == K else Yk[w, k, :, t]).astype(np.float64) * scale
                idx = np.nonzero((f[w, t, :, 0] != 0) & np.isfinite(pts).all(1))[0]
                pl = P[w, :, t].astype(np.float64) * scale
                live = np.nonzero(np.isfinite(pl).all(1))[0]
                if idx.size == 0 or live.size == 0:
                    continue
                near = cdist(pl[live], pts[idx]) < r
                near &= idx[None, :] != e[w, live][:, None]
                for mm in live[near.any(1)]:
                    if first[w, mm, k] == T:
                        first[w, mm, k] = t
    return first


KINDS = ("cross", "follow", "same", "ego", "far", "nan", "gone")


def make_inputs(d, M, radius, ux, uy, seed, centres=None):
    """joint_reference.make_inputs' Y, fut and present (slots on a lattice 4 radii apart with a jitter below 0.5 radius) and M plans per window
    that cycle, turning with the window, through KINDS.  A plan is laid out against a TARGET slot i in a reference sample k_ref:
       cross    it passes i at 0.5 radius per frame, 0.3 radius to the side: it touches i at the frames around the centre frame only
                (`centres`: the centre frames to cycle through; default the middle third);
       follow   i + (0.5 radius, 0) in every frame;
       same     i bit for bit;
       ego      i bit for bit, and i is the slot the plan replaces: it must not touch (i is chosen 2 radii or more from every other slot);
       far      30 radii off the lattice;
       nan      a crossing whose contacts lie behind the middle frame, from which on the plan is NaN: it must not touch i;
       gone     0.5 radius from a slot that leaves half way at exactly the frames it is not counted in, far off before: it must not touch it.
    Every kind but `same` and `ego` carries a constant offset below 0.02 radius.  At mno = 1 every plan replaces the one slot.  A plan with a
    finite q within 1.5 * MARGIN * r2 of r2 in float64, against any sample or the ground truth, is drawn again.
    Returns (Y, fut, present, plans, ego, info); info["plans"][w][m] = (kind, i, k_ref, centre or None, checkable)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Y, fut, present, _ = joint_inputs(d, radius, ux, uy, seed, centres=chunk_centres(m, T))
    r = float(radius)
    fx, fy = float(np.float32(ux)), float(np.float32(uy))
    unit, inv = np.array([fx, fy]), np.array([1.0 / fx, 1.0 / fy])
    Yk = Y.reshape(n, K, m, T, 2)
    g = np.stack([fut[..., 1] * np.float32(d.sx), fut[..., 2] * np.float32(d.sy)], -1).astype(np.float32).transpose(0, 2, 1, 3)    # [n, m, T, 2]
    counted = (fut[..., 0] != 0).transpose(0, 2, 1)                        # [n, m, T]
    plans = np.zeros((n, M, T, 2), np.float32)
    ego = np.full((n, M), -1, np.int32)
    info = []
    n_cross = 0
    mid = T // 2
    far = -30.0 * r

    def alone(w, k):
        """Slots of (w, k) that stay 2 radii or more from every other slot (float64)."""
        p = Yk[w, k].astype(np.float64) * unit
        dx = p[:, None, :, 0] - p[None, :, :, 0]
        dy = p[:, None, :, 1] - p[None, :, :, 1]
        q = dx * dx + dy * dy
        q[np.eye(m, dtype=bool)] = np.inf
        with np.errstate(all="ignore"):
            return ~(q < 4 * r * r).any((1, 2)) & np.isfinite(p).all((1, 2))

    def in_band(p32, w, e):
        if r == 0:
            return False
        others = np.concatenate([Yk[w], g[w][None]], 0).astype(np.float64)           # [K + 1, m, T, 2]
        a = (p32.astype(np.float64)[None, None, :, 0] - others[..., 0]) * fx
        b = (p32.astype(np.float64)[None, None, :, 1] - others[..., 1]) * fy
        q = a * a + b * b
        if e >= 0:
            q[:, e] = np.inf
        with np.errstate(all="ignore"):
            return bool((np.abs(q - r * r) <= 1.5 * MARGIN * r * r).any())

    for w in range(n):
        full = np.nonzero(counted[w].all(-1))[0]
        leaves = np.nonzero(counted[w, :, 0] & ~counted[w, :, -1])[0]
        row = []
        for mi in range(M):
            kind = KINDS[(mi + w) % len(KINDS)]
            if kind == "gone" and (leaves.size == 0 or T < 2):
                kind = "far"
            if kind in ("cross", "nan") and T < 3:
                kind = "follow"
            for attempt in range(200):
                rng = np.random.default_rng([seed, w, mi, attempt, 4242])
                k_ref = int(rng.integers(K))
                finite = np.isfinite(Yk[w, k_ref]).all((1, 2))
                cand = full[finite[full]]
                if kind == "ego":
                    cand = cand[alone(w, k_ref)[cand]]
                checkable = cand.size > 0
                i = int(rng.choice(cand)) if checkable else int(rng.integers(m))
                base = Yk[w, k_ref, i].astype(np.float64) * unit             # the caller's unit
                jit = rng.uniform(-0.02 * r, 0.02 * r, 2)
                cs, e = None, -1
                if kind == "cross":
                    cs = centres[n_cross % len(centres)] if centres else int(rng.integers(T // 3, max(T // 3 + 1, (2 * T) // 3)))
                    p = base + np.stack([(np.arange(T) - cs) * 0.5 * r, np.full(T, 0.3 * r)], -1) + jit
                elif kind == "follow":
                    p = base + np.array([0.5 * r, 0.0]) + jit
                elif kind in ("same", "ego"):
                    p = None
                    e = i if kind == "ego" else -1
                elif kind == "far":
                    p = np.full((T, 2), far) + np.cumsum(rng.normal(0, 0.05 * r, (T, 2)), 0)
                elif kind == "nan":
                    cs = min(T - 1, mid + 1)
                    p = base + np.stack([(np.arange(T) - cs) * 0.5 * r, np.full(T, 0.3 * r)], -1) + jit
                else:                                                      # gone
                    i = int(rng.choice(leaves))
                    checkable = bool(np.isfinite(Yk[w, k_ref, i]).all())
                    away = ~counted[w, i]
                    p = np.full((T, 2), far) + jit
                    p[away] = (Yk[w, k_ref, i].astype(np.float64) * unit)[away] + np.array([0.5 * r, 0.0]) + jit
                p32 = Yk[w, k_ref, i].copy() if p is None else (p * inv).astype(np.float32)
                if kind == "nan":
                    p32[mid:] = np.nan
                if m == 1:
                    e = 0
                if not in_band(p32, w, e):
                    break
            else:
                raise AssertionError("plan (%d, %d) was not cleared of the band" % (w, mi))
            if kind == "cross":
                n_cross += 1
            plans[w, mi], ego[w, mi] = p32, e
            row.append((kind, i, k_ref, cs, checkable))
        info.append(row)
    return Y, fut, present, plans, ego, {"plans": info, "geometry": plan_geometry(m, T, M)}


def equal_joint_scores(d, seed):
    """[n, K, mno] fp32 on the grid of 1/64 whose K joint scores are equal in every window: every weight is 1 / K exactly."""
    s = (np.random.default_rng(seed).integers(-256, 257, (d.n_scenes, 1, d.mno)) / 64.0).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(s, (d.n_scenes, d.K, d.mno)))


# (n_scenes, mno, K, T_pred, M): the smallest shapes at which each mechanism of the kernel can go wrong
SHAPES = [(2, 8, 3, 7, 5),              # the plain case, odd T_pred
          (3, 1, 3, 7, 1),              # one slot that is the ego: nothing can touch; a row boundary falls inside every 16-byte load
          (3, 32, 20, 40, 9),           # the headline's window; M is not a multiple of any plan chunk
          (2, 160, 4, 9, 3),            # more slots than lanes per frame
          (2, 32, 3, 200, 4),           # long rows
          (2, 256, 2, 40, 70)]          # the frame-chunked walk (29 + 11 frames) and more plans than one workgroup holds
RADIUS_PX = 20.0
