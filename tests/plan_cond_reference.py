"""Numpy statement of the conditioned plan-risk contract (include/desire_hip.h: desire_plan_risk_cond, steps C1 - C8) on top of
tests/plan_reference.py, in two forms:

  plan_cond_f32   the contract's fp32 operation sequence, every operation rounded once;
  plan_cond_f64   C4 - C7 in float64 ON THE fp32 LOGITS of plan_cond_f32.  C1 - C3 hold no transcendental (differences, products, one sum in a
                  fixed order, one division), so the device reproduces them exactly and they are compared bit for bit; what the float64 form
                  measures is expf, the sums over k and the divisions.  The prior weights W of the float64 form are the softmax, in float64,
                  of the fp32 joint scores.

Bounds on |device - plan_cond_f64|, from the precision of the formats.  Write u = 2^-24 (half an ulp of a value below 1).  A weight is
cw_k = e_k / sum_j e_j with e_k = expf(l_k - m):
  * the fp32 difference l_k - m is off by |l_k - m| u at most, which moves e_k by e_k |l_k - m| u <= u / e (x exp(-x) <= 1 / e), and expf itself
    is good to a few ulp of e_k <= 1;
  * the sum of K terms in fp32 is off by K u relative at most, the division by u.
So |cw_k - cw64_k| <= (K + 8) u: the bound the tests put on every entry of cw, and, the weights of a plan summing to 1, on a sum of any of them
(tests/plan_reference.py: risk_bound).  From it:
  * support = sum_k W_k expf(-x_k), every factor in [0, 1]: the weights contribute (K + 8) u in all as above, expf and the product 4 u
    relative on a sum of 1 at most, the K additions K u.  support_bound = (2 K + 12) u.
  * ess = 1 / s2, s2 = sum_k cw_k^2 in [1 / K, 1]: d(s2) = sum_k 2 cw_k d(cw_k) <= 2 (K + 8) u (the cw_k sum to 1), the K squares and additions
    add (K + 1) u s2, so |d(s2)| <= (3 K + 17) u; and d(ess) = ess^2 d(s2) to first order, the division adding ess u.
    ess_bound = ess^2 (3 K + 18) u: 4.7e-4 at K = 20 and ess = 10.

The generator starts from plan_reference.make_inputs and names ego slots on top (make_cond_inputs)."""
import numpy as np

from tests.plan_reference import MARGIN, RADIUS_PX, SHAPES, make_inputs, plan_centres, plan_f32, plan_f64, risk_bound

__all__ = ["MARGIN", "RADIUS_PX", "SHAPES", "plan_cond_geometry", "plan_cond_f32", "plan_cond_f64", "make_cond_inputs", "cond_scores", "cw_bound",
           "support_bound", "ess_bound", "risk_bound", "plan_centres", "prior_risk", "cond_dims", "cond_units", "cond_horizons", "cond_case",
           "cond_ref", "SEED", "planted_identical", "planted_one_hot", "planted_nan"]

LDS_BYTES, THREADS, MAX_PC, ITEMS = 61440, 256, 64, 1024
U = 2.0 ** -24


def plan_cond_geometry(K, t_cond, M):
    """(PC, TC, rows) of desire_amd/csrc/eval_lds.h: plan_cond_geometry -- the plans of a workgroup, the frames of one pass, and whether the K ego
    rows are staged next to the plans."""
    chunks = lambda n, per: -(-n // per)
    cap = min(M, MAX_PC, max(1, ITEMS // K))
    pc = chunks(M, chunks(M, cap))
    if 8 * (pc + K) * (t_cond | 1) + 8 * pc <= LDS_BYTES:
        return pc, t_cond, 1
    return pc, min(t_cond, (LDS_BYTES - 16 * pc) // (8 * pc)), 0


def cw_bound(d):
    return (d.K + 8) * U


def support_bound(d):
    return (2 * d.K + 12) * U


def ess_bound(d, ess):
    return np.asarray(ess, np.float64) ** 2 * (3 * d.K + 18) * U


def _softmax(l, dtype):
    """eval_weight_stats on one row of K finite logits (fp32 values), in dtype: m = max, e_k = exp(l_k - m), e_k / sum, the sum in increasing k."""
    l = l.astype(dtype)
    e = np.exp((l - l.max()).astype(dtype)).astype(dtype)
    tot = dtype(0)
    for k in range(e.shape[0]):
        tot = dtype(tot + e[k])
    return (e / tot).astype(dtype)


def _logits(Y, fut, present, plans, ego, js, scored, sigma, t_cond, ux, uy, d):
    """C1 - C3 in fp32: (has [n, M], n_c [n, M], D [n, M, K], x = D * inv [n, M, K], l [n, M, K], p [n, K])."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    f32 = np.float32
    ux, uy = f32(ux), f32(uy)
    P = np.asarray(plans, f32)
    M = P.shape[1]
    Yk = np.asarray(Y, f32).reshape(n, K, m, T, 2)
    if fut is not None:
        c = (np.asarray(fut, f32)[..., 0] != 0).transpose(0, 2, 1)          # [n, m, T]
    else:
        c = np.broadcast_to((np.asarray(present).reshape(n, m) != 0)[:, :, None], (n, m, T))
    e = np.full((n, M), -1, np.int64) if ego is None else np.asarray(ego, np.int64).reshape(n, M)
    has = (e >= 0) & (e < m)
    es = np.where(has, e, 0)
    w_idx = np.arange(n)[:, None]
    rows = Yk[w_idx, :, es]                                                 # [n, M, K, T, 2]
    cmp = has[:, :, None] & c[w_idx, es] & ~np.isnan(P).any(-1) & (np.arange(T) < int(t_cond))[None, None]     # [n, M, T]
    n_c = cmp.sum(-1).astype(np.int32)
    S = np.zeros((n, M, K), f32)
    with np.errstate(all="ignore"):
        for t in range(int(t_cond)):
            a = (P[:, :, None, t, 0] - rows[:, :, :, t, 0]) * ux
            b = (P[:, :, None, t, 1] - rows[:, :, :, t, 1]) * uy
            q = a * a + b * b
            S = np.where(cmp[:, :, None, t], S + q, S).astype(f32)
        D = np.where(n_c[:, :, None] >= 1, S / np.maximum(n_c, 1)[:, :, None].astype(f32), f32(0)).astype(f32)
        s = f32(sigma)
        inv = f32(1) / (f32(2) * s * s)
        js = np.asarray(js, f32)
        ok = np.isfinite(js).all(-1) if scored else np.zeros(n, bool)
        p = np.where(ok[:, None], js, f32(0)).astype(f32)                   # [n, K]
        x = (D * inv).astype(f32)
        l = (p[:, None, :] - x).astype(f32)
    return has, n_c, D, x, l, p, inv


def _weights(has, n_c, x, l, W, dtype):
    """C4 - C6 in dtype on the fp32 logits l and products x; W [n, K] in dtype."""
    n, M, K = l.shape
    conditioned = has & (n_c >= 1) & np.isfinite(l).all(-1)
    cw = np.empty((n, M, K), dtype)
    ess = np.empty((n, M), dtype)
    support = np.ones((n, M), dtype)
    with np.errstate(all="ignore"):
        for w in range(n):
            for mi in range(M):
                if conditioned[w, mi]:
                    cw[w, mi] = _softmax(l[w, mi], dtype)
                    g = np.exp(-x[w, mi].astype(dtype)).astype(dtype)
                    sup = dtype(0)
                    for k in range(K):
                        sup = dtype(sup + dtype(W[w, k] * g[k]))
                    support[w, mi] = sup
                else:
                    cw[w, mi] = W[w]
                s2 = dtype(0)
                for k in range(K):
                    s2 = dtype(s2 + dtype(cw[w, mi, k] * cw[w, mi, k]))
                ess[w, mi] = dtype(1) / s2
    return conditioned, cw, ess, support


def _risk(first, first_slot, cw, hz, dtype):
    """desire_plan_risk's steps 7 - 8 with cw [n, M, K] in place of W."""
    n, M, K = cw.shape
    hzv = np.asarray(hz)
    risk = np.zeros((n, M, len(hz)), dtype)
    blame = np.zeros((n, M, len(hz), first_slot.shape[-1]), dtype)
    for k in range(K):
        wk = cw[:, :, k]
        risk = np.where(first[:, :, k, None] < hzv[None, None], risk + wk[:, :, None], risk).astype(dtype)
        blame = np.where(first_slot[:, :, k, None, :] < hzv[None, None, :, None], blame + wk[:, :, None, None], blame).astype(dtype)
    return risk, blame


def prior_risk(first, W, hz, dtype=np.float64):
    """desire_plan_risk's step 7 from first [n, M, >= K] and W [n, K]."""
    K = W.shape[1]
    cw = np.broadcast_to(W[:, None, :], (first.shape[0], first.shape[1], K)).astype(dtype)
    return _risk(first, np.zeros(first.shape[:2] + (K, 0), np.int32), cw, hz, dtype)[0]


def _cond(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d, sigma, t_cond, dtype, base=None):
    hz = [int(h) for h in horizons]
    base = base if base is not None else {}                                # plan_f32 / plan_f64 of the same inputs, kept by the caller
    if "f32" not in base:
        base["f32"] = plan_f32(Y, fut, present, score, plans, ego, hz, radius, ux, uy, d)
    if dtype is not np.float32 and "f64" not in base:
        base["f64"] = plan_f64(Y, fut, present, score, plans, ego, hz, radius, ux, uy, d)
    base32 = base["f32"]
    base = base32 if dtype is np.float32 else base["f64"]
    js = base32["jscore"]
    has, n_c, D, x, l, p, inv = _logits(Y, fut, present, plans, ego, js, score is not None, sigma, t_cond, ux, uy, d)
    if dtype is np.float32:
        W = base32["W"]
    else:                                                                  # the softmax in float64 of the fp32 joint scores
        W = np.full(js.shape, 1.0 / d.K, np.float64)
        if score is not None:
            for w in range(d.n_scenes):
                if np.isfinite(js[w]).all():
                    W[w] = _softmax(js[w], np.float64)
    conditioned, cw, ess, support = _weights(has, n_c, x, l, W, dtype)
    risk, blame = _risk(base["first"], base["first_slot"][:, :, :d.K], cw, hz, dtype)
    return {"first": base["first"], "clear": base["clear"], "first_slot": base["first_slot"], "margin": base["margin"], "W": W, "jscore": js,
            "risk": risk, "blame": blame, "cw": cw, "dist": D, "logit": l, "x": x, "inv": inv, "ess": ess, "support": support,
            "cond": np.where(conditioned, n_c, 0).astype(np.int32), "n_c": n_c, "conditioned": conditioned,
            "risk_prior": prior_risk(base["first"], W, hz, dtype)}


def plan_cond_f32(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d, sigma, t_cond, base=None):
    return _cond(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d, sigma, t_cond, np.float32, base)


def plan_cond_f64(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d, sigma, t_cond, base=None):
    return _cond(Y, fut, present, score, plans, ego, horizons, radius, ux, uy, d, sigma, t_cond, np.float64, base)


def cond_scores(d, seed):
    """[n, K, mno] fp32 scores, 0.3 N(0, 1) / sqrt(mno) per row: joint scores that spread by about 0.3, so no world holds all the prior weight."""
    rng = np.random.default_rng([seed, 77])
    return (0.3 * rng.standard_normal((d.n_scenes, d.K, d.mno)) / np.sqrt(d.mno)).astype(np.float32)


SEED = 6                     # both units meet the coverage conditions of test_plan_cond_cpu.py at this seed
_CASES = {}


def cond_dims(shape, **kw):
    from tests.helpers import small_dims
    n, m, K, T = shape[:4]
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64, **kw)


def cond_units(d):
    """(unit_x, unit_y, the radius in that unit): normalised coordinates, pixels."""
    return [(1.0, 1.0, float(np.float32(RADIUS_PX * d.sx))), (1.0 / d.sx, 1.0 / d.sy, RADIUS_PX)]


def cond_horizons(T):
    return sorted({max(1, T // 4), max(1, T // 2), T})


def cond_case(shape, unit, seed=SEED):
    """Inputs of (shape, unit), computed once and left unchanged; "ref" caches the references per (form, sigma, t_cond) through cond_ref."""
    key = (shape, unit, seed)
    if key not in _CASES:
        d = cond_dims(shape)
        M = shape[4]
        ux, uy, radius = cond_units(d)[unit]
        Y, fut, present, plans, ego, info = make_cond_inputs(d, M, radius, ux, uy, seed, centres=plan_centres(d.mno, d.T_pred, M))
        s = cond_scores(d, 9)
        for a in (Y, fut, present, plans, ego, s):
            a.setflags(write=False)
        _CASES[key] = dict(d=d, M=M, Y=Y, fut=fut, present=present, plans=plans, ego=ego, score=s, info=info, hz=cond_horizons(d.T_pred),
                           unit=(ux, uy, radius), ref={})
    return _CASES[key]


def cond_ref(c, fn, sigma, t_cond):
    """fn (plan_cond_f32 / plan_cond_f64) on the case's inputs in its evaluation form, computed once per (fn, sigma, t_cond)."""
    key = (fn.__name__, float(sigma), int(t_cond))
    if key not in c["ref"]:
        ux, uy, radius = c["unit"]
        c["ref"][key] = fn(c["Y"], c["fut"], None, c["score"], c["plans"], c["ego"], c["hz"], radius, ux, uy, c["d"], sigma, t_cond,
                           base=c["ref"].setdefault("base", {}))
    return c["ref"][key]


def make_cond_inputs(d, M, radius, ux, uy, seed, centres=None):
    """plan_reference.make_inputs' (Y, fut, present, plans, ego, info) with the ego slots named for conditioning: the kinds follow, cross, nan and
    gone replace their target slot, far a random slot, ego keeps its slot, same keeps none.  At mno = 1 every plan replaces the one slot, as
    make_inputs has it.  Replacing a slot only takes pairs out of the contact rule, so the margin make_inputs cleared still holds (the tests
    assert it on the float64 pass all the same)."""
    Y, fut, present, plans, ego, info = make_inputs(d, M, radius, ux, uy, seed, centres=centres)
    ego = ego.copy()
    if d.mno > 1:
        rng = np.random.default_rng([seed, 4243])
        for w, row in enumerate(info["plans"]):
            for mi, (kind, i, _, _, _) in enumerate(row):
                if kind in ("follow", "cross", "nan", "gone"):
                    ego[w, mi] = i
                elif kind == "far":
                    ego[w, mi] = int(rng.integers(d.mno))
                elif kind == "same":
                    ego[w, mi] = -1
    return Y, fut, present, plans, ego, info


# ---- the planted inputs of the exact anchors
def planted_identical(c):
    """Every plan replaces slot 0, whose K rows are world 0's: Y, ego."""
    d = c["d"]
    Yk = c["Y"].reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).copy()
    Yk[:, :, 0] = Yk[:, :1, 0]
    return Yk.reshape(c["Y"].shape), np.zeros_like(c["ego"])


def planted_one_hot(c):
    """Plan m of a window = the row of world m % K of a slot that is counted in every frame and finite in every world, replacing that slot:
    (plans, ego, k0 [M], sigma, live [n]).  The other worlds' rows differ from it (the generator's jitter; asserted).  A window without such a
    slot (the generator's empty window) is not live: its plans name slot 0 and are not conditioned."""
    d = c["d"]
    n, K, m, T, M = d.n_scenes, d.K, d.mno, d.T_pred, c["M"]
    Yk = c["Y"].reshape(n, K, m, T, 2)
    counted = (c["fut"][..., 0] != 0).all(1)                                # [n, m]
    plans = np.zeros((n, M, T, 2), np.float32)
    ego = np.zeros((n, M), np.int32)
    k0 = np.arange(M) % K
    low = np.inf
    live = np.zeros(n, bool)
    for w in range(n):
        ok = np.nonzero(counted[w] & np.isfinite(Yk[w]).all((0, 2, 3)))[0]
        if ok.size == 0:
            continue
        live[w] = True
        e = int(ok[0])
        ego[w] = e
        plans[w] = Yk[w, k0, e]
        unit = np.array(c["unit"][:2])
        for mi in range(M):
            dd = (((Yk[w, :, e].astype(np.float64) - plans[w, mi]) * unit) ** 2).sum(-1).mean(-1)      # [K]
            assert dd[k0[mi]] == 0 and (np.delete(dd, k0[mi]) > 0).all()
            if K > 1:
                low = min(low, float(np.delete(dd, k0[mi]).min()))
    assert live.any() and np.isfinite(low)
    return plans, ego, k0, float(np.sqrt(low / (2 * 104.0)) / 4), live


def planted_nan(c, f64):
    """A NaN at a compared frame of one world's row of the ego slot of a conditioned plan: (Y, window, plan, world)."""
    d = c["d"]
    w, mi = (int(v[0]) for v in np.nonzero(f64["conditioned"]))
    e, k1 = int(c["ego"][w, mi]), d.K - 1
    t = int(np.nonzero((c["fut"][w, :, e, 0] != 0) & ~np.isnan(c["plans"][w, mi]).any(-1))[0][0])
    Yk = c["Y"].reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).copy()
    Yk[w, k1, e, t, 1] = np.nan
    return Yk.reshape(c["Y"].shape), w, mi, k1
