"""Numpy statements of the occupancy contract (include/desire_hip.h: desire_occupancy) and the input generator their tests share.
occupancy_f32 is the contract in its order of operations with float32 scalars throughout, occupancy_f64 the same in float64, marginals_brute
a third, brute-force statement of the visits and marginals alone (np.add.at per (agent, horizon), uniform weights).  Agent a = scene * mno +
slot, row r_k = (scene * K + k) * mno + slot.

The cell of a position can only differ between the precisions where a coordinate lies within rounding of a cell edge.  The generator keeps
every coordinate either EXACTLY on an edge at a dyadic value (x = 0.5, x = 1.0, x = -0.25: the product with the grid size is exact in both
precisions) or at least EDGE_MARGIN (normalised units) away from one; edge_margin() measures that on float64 alone."""
import numpy as np

from tests.select_reference import weights

AT, UNTIL = 0, 1
EDGE_MARGIN = 1e-4
# (windows, mno, K, T_pred, (Oh, Ow)) of tests/test_gpu_occupancy.py, with the seed chosen on the CPU so that conditions() holds on each
SHAPES = [(2, 8, 3, 7, (4, 5)), (3, 1, 3, 7, (3, 3)), (2, 32, 20, 40, (64, 64)), (2, 160, 4, 9, (16, 16)), (2, 8, 5, 9, (96, 96)), (1, 8, 130, 7, (8, 8))]
SEEDS = {s: 3 for s in SHAPES}


def band_rows(K, frames, Oh, Ow, until):
    """Grid rows of one band of the kernel's LDS plan (desire_amd/csrc/eval_lds.h: occupancy_geometry); frames = 1 in AT, the largest horizon in UNTIL."""
    fc = min(frames, 512)
    kc = min(K, max(1, 512 // fc))
    kc = -(-K // -(-K // kc))
    fit = (61440 - 20 * kc * fc) // (4 * (4 if until else 3)) // Ow
    r = min(Oh, fit)
    return -(-Oh // -(-Oh // r))


def _counted(fut, present, d):
    n, m, T = d.n_scenes, d.mno, d.T_pred
    if fut is not None:
        return (np.asarray(fut, np.float32)[..., 0] != 0).transpose(0, 2, 1)               # [n, m, T]
    return np.broadcast_to((np.asarray(present).reshape(n, m) != 0)[:, :, None], (n, m, T))


def _cells(x, y, Oh, Ow, dtype):
    """The cell of every position, -1 where it is off frame: one multiply per axis in `dtype`, floor, no clamp; a NaN is off frame."""
    with np.errstate(all="ignore"):
        fx = np.floor(np.asarray(x, np.float32).astype(dtype) * dtype(Ow))
        fy = np.floor(np.asarray(y, np.float32).astype(dtype) * dtype(Oh))
        ok = (fx >= 0) & (fx <= Ow - 1) & (fy >= 0) & (fy <= Oh - 1)
        return np.where(ok, np.where(ok, fy, 0).astype(np.int64) * Ow + np.where(ok, fx, 0).astype(np.int64), -1)


def _occupancy(Y, fut, present, score, horizons, mode, grid, mask, mask_of_scene, d, dtype, want_marg=False):
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Oh, Ow = grid
    hz = [int(h) for h in horizons]
    nh, C = len(hz), Oh * Ow
    Yk = np.asarray(Y, np.float32).reshape(n, K, m, T, 2)
    c = _counted(fut, present, d)
    w = weights(score, d, dtype).reshape(n, m, K)
    cell = _cells(Yk[..., 0], Yk[..., 1], Oh, Ow, dtype)                                   # [n, K, m, T]
    one, zero = dtype(1), dtype(0)
    E = np.zeros((n, nh, C), dtype)
    q = np.ones((n, nh, C), dtype)
    off = np.zeros((n, m, nh), dtype)
    viol = np.zeros((n, m, nh), dtype)
    hit = np.zeros((n, m, nh), dtype)
    marg = np.zeros((n, m, nh, C), dtype) if want_marg else None
    if fut is not None:
        f = np.asarray(fut, np.float32)
        gx = (f[..., 1] * np.float32(d.sx)).astype(np.float32)                              # rounded once in fp32: an input
        gy = (f[..., 2] * np.float32(d.sy)).astype(np.float32)
        gcell = _cells(gx, gy, Oh, Ow, dtype).transpose(0, 2, 1)                            # [n, m, T]
    for s in range(n):
        mk = None
        if mask is not None and int(mask_of_scene[s]) >= 0:
            mk = np.asarray(mask)[int(mask_of_scene[s])].reshape(C)
        for hi, h in enumerate(hz):
            frames = np.arange(h) if mode == UNTIL else np.array([h - 1])
            for i in range(m):
                ct = c[s, i, frames]
                if not ct.any():
                    continue
                p = np.zeros(C, dtype)
                so, sv, sh = zero, zero, zero
                cg = gcell[s, i, h - 1] if (fut is not None and mode == AT and c[s, i, h - 1]) else -1
                for k in range(K):
                    ck = cell[s, k, i, frames][ct]
                    wk = w[s, i, k]
                    if (ck < 0).any():
                        so = so + wk
                    vis = np.unique(ck[ck >= 0])                                            # a cell once, however often the sample returns
                    p[vis] = p[vis] + wk
                    if mk is not None and (mk[vis] == 0).any():
                        sv = sv + wk
                    if cg >= 0 and (vis == cg).any():
                        sh = sh + wk
                E[s, hi] = E[s, hi] + p
                q[s, hi] = q[s, hi] * (one - p)
                off[s, i, hi], viol[s, i, hi], hit[s, i, hi] = so, sv, sh
                if want_marg:
                    marg[s, i, hi] = p
    res = {"occ": (one - q).reshape(n, nh, Oh, Ow), "exp": E.reshape(n, nh, Oh, Ow), "off": off.reshape(n * m, nh),
           "viol": viol.reshape(n * m, nh) if mask is not None else None, "hit": hit.reshape(n * m, nh) if (fut is not None and mode == AT) else None}
    if want_marg:
        res["marg"] = marg.reshape(n * m, nh, C)
    return res


def occupancy_f32(Y, fut, present, score, horizons, mode, grid, mask, mask_of_scene, d, want_marg=False):
    return _occupancy(Y, fut, present, score, horizons, mode, grid, mask, mask_of_scene, d, np.float32, want_marg)


def occupancy_f64(Y, fut, present, score, horizons, mode, grid, mask, mask_of_scene, d, want_marg=False):
    return _occupancy(Y, fut, present, score, horizons, mode, grid, mask, mask_of_scene, d, np.float64, want_marg)


def marginals_brute(Y, fut, present, horizons, mode, grid, d):
    """(visits [A, n_h, K, C] bool, marginals [A, n_h, C] float32) under uniform weights, position by position: a third statement of steps 3 - 5."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Oh, Ow = grid
    C = Oh * Ow
    Yk = np.asarray(Y, np.float32).reshape(n, K, m, T, 2)
    c = _counted(fut, present, d)
    vis = np.zeros((n * m, len(horizons), K, C), bool)
    for s in range(n):
        for i in range(m):
            for hi, h in enumerate(horizons):
                for t in (range(h) if mode == UNTIL else [h - 1]):
                    if not c[s, i, t]:
                        continue
                    for k in range(K):
                        x, y = np.float32(Yk[s, k, i, t, 0]) * np.float32(Ow), np.float32(Yk[s, k, i, t, 1]) * np.float32(Oh)
                        if not (0 <= x < Ow and 0 <= y < Oh):                               # (a NaN fails both)
                            continue
                        vis[s * m + i, hi, k, int(np.floor(y)) * Ow + int(np.floor(x))] = True
    marg = np.zeros((n * m, len(horizons), C), np.float32)
    u = np.float32(1) / np.float32(K)
    for a in range(n * m):
        for hi in range(len(horizons)):
            kk, cc = np.nonzero(vis[a, hi])                                                 # k-major: np.add.at adds in increasing k
            np.add.at(marg[a, hi], cc, np.full(len(cc), u, np.float32))
    return vis, marg


def edge_margin(Y, fut, grid, d):
    """The smallest distance (normalised units) of a coordinate that is not EXACTLY on a cell edge from the nearest edge, over the finite sample
    positions and the scaled targets -- in float64 alone."""
    Oh, Ow = grid
    xs = [np.asarray(Y, np.float32)[..., 0].astype(np.float64).ravel()]
    ys = [np.asarray(Y, np.float32)[..., 1].astype(np.float64).ravel()]
    if fut is not None:
        f = np.asarray(fut, np.float32)
        xs.append((f[..., 1] * np.float32(d.sx)).astype(np.float32).astype(np.float64).ravel())
        ys.append((f[..., 2] * np.float32(d.sy)).astype(np.float32).astype(np.float64).ravel())
    best = np.inf
    for v, G in ((np.concatenate(xs), Ow), (np.concatenate(ys), Oh)):
        v = v[np.isfinite(v)]
        dist = np.abs(v * G - np.rint(v * G)) / G
        dist = dist[dist > 0]
        if dist.size:
            best = min(best, float(dist.min()))
    return best


def _off_edges(v, G):
    """Moves every float32 value of v that is within 2 * EDGE_MARGIN of a multiple of 1 / G, and not exactly on one, further away."""
    v = v.astype(np.float32)
    for _ in range(8):
        u = v.astype(np.float64) * G
        dist = np.abs(u - np.rint(u)) / G
        bad = np.isfinite(dist) & (dist > 0) & (dist < 2 * EDGE_MARGIN)
        if not bad.any():
            break
        v = np.where(bad, v + np.float32(5 * EDGE_MARGIN), v).astype(np.float32)
    return v


def make_inputs(d, grid, seed):
    """Y [R, T, 2], fut [n, T, mno, 3], present [A] uint8, mask [2, Oh, Ow] uint8, mask_of_scene [n] int32, with the cases of the module docstring of
    tests/test_gpu_occupancy.py planted.  The agents of a window walk within a few cells of the frame's centre, so that they share cells (and, on a
    banded grid, lie on both sides of a band's border); an agent's samples scatter by a fraction of a cell around its track."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Oh, Ow = grid
    rng = np.random.default_rng(seed)
    cw = np.array([1.0 / Ow, 1.0 / Oh])
    start = 0.5 + rng.uniform(-1.4, 1.4, (n, 1, m, 1, 2)) * cw
    start[:, :, 1::2, :, 1] -= 1.0 / 6                                                        # the odd slots a sixth of the frame up: a second cluster
    track = start + np.cumsum(rng.normal(0, 0.35, (n, 1, m, T, 2)), 3) * cw
    Yk = track + rng.normal(0, 0.45, (n, K, m, 1, 2)) * cw + rng.normal(0, 0.25, (n, K, m, T, 2)) * cw
    Yk = Yk.astype(np.float32)
    g = (track[:, 0] + rng.normal(0, 0.3, (n, m, T, 2)) * cw).astype(np.float32)             # targets [n, m, T, 2], normalised
    # off frame: some samples leave the frame for a frame or two (x = 1.0 exactly, negatives, far outside)
    gone = rng.random((n, K, m)) < 0.12
    for s, k, i in zip(*np.nonzero(gone)):
        t = int(rng.integers(0, T))
        Yk[s, k, i, t] = [(1.0, 0.5), (-0.25, 0.5), (0.5, 1.75), (-1e-3, -1e-3)][int(rng.integers(0, 4))]
    ids = np.ones((n, T, m), np.float32) * np.arange(1, m + 1, dtype=np.float32)[None, None, :]
    ids[rng.random((n, T, m)) < 0.1] = 0                                                      # frames the object is missing from
    t_mid = T // 2
    # ---- the planted cases (window 0)
    centre = np.array([0.5 + 0.3 / Ow, 0.5 + 0.3 / Oh], np.float32)
    Yk[0, 0, 0, 0] = centre; ids[0, 0, 0] = 1
    if K > 1:
        Yk[0, 1, 0, 0] = centre                                                               # two samples of one agent in one cell
    for i in range(1, min(m, 3)):
        Yk[0, 0, i, 0] = centre; ids[0, 0, i] = i + 1                                         # two and three agents in one cell
    if K > 2 and T > 2:                                                                       # a sample that leaves a cell and returns
        Yk[0, 2, 0, 0] = centre; Yk[0, 2, 0, 1] = centre + np.array([1.0 / Ow, 0], np.float32); Yk[0, 2, 0, 2] = centre
        ids[0, :3, 0] = 1
    Yk[0, 0, 0, T - 1] = (0.5, 0.5)                                                           # on a cell edge of an even grid, exactly
    Yk[0, K - 1, 0, T - 1] = (1.0, 0.25)                                                      # x = 1.0 exactly: off frame
    Yk[0, K - 1, 0, max(T - 2, 0)] = (-0.25, 0.25)
    ids[0, max(T - 2, 0):, 0] = 1
    if n > 1 or m > 1:
        Yk[-1 if n > 1 else 0, K - 1, m - 1 if n == 1 else 0] = np.nan                        # a NaN row
    if T > 2:
        ids[0, t_mid, 0] = 0                                                                  # an uncounted frame in the middle of a track
        ids[0, t_mid - 1, 0] = 1; ids[0, t_mid + 1 if t_mid + 1 < T else t_mid - 1, 0] = 1
    if m > 1:
        ids[0, :, m - 1] = 0                                                                  # an absent slot
    if n > 1:
        ids[n - 1] = 0                                                                        # an empty window
    Yk[..., 0], Yk[..., 1] = _off_edges(Yk[..., 0], Ow), _off_edges(Yk[..., 1], Oh)
    fut = np.zeros((n, T, m, 3), np.float32)
    fut[..., 0] = ids
    sx, sy = np.float32(d.sx), np.float32(d.sy)
    px, py = (g[..., 0] / sx).astype(np.float32), (g[..., 1] / sy).astype(np.float32)
    for _ in range(8):                                                                        # the SCALED target is what must keep off the edges
        gx, gy = (px * sx).astype(np.float32), (py * sy).astype(np.float32)
        px = np.where(_off_edges(gx, Ow) != gx, px + np.float32(5 * EDGE_MARGIN) / sx, px).astype(np.float32)
        py = np.where(_off_edges(gy, Oh) != gy, py + np.float32(5 * EDGE_MARGIN) / sy, py).astype(np.float32)
    fut[..., 1], fut[..., 2] = px.transpose(0, 2, 1), py.transpose(0, 2, 1)
    present = (ids != 0).any(1).reshape(-1).astype(np.uint8)
    # ---- masks: mask 0 forbids a visited cell (the planted one) and one nobody visits, where the grid has one; mask 1 forbids everything
    mask = np.ones((2, Oh, Ow), np.uint8)
    cells = _cells(Yk[..., 0], Yk[..., 1], Oh, Ow, np.float64)
    mask[0].reshape(-1)[int(_cells(centre[0], centre[1], Oh, Ow, np.float64))] = 0
    free = np.setdiff1d(np.arange(Oh * Ow), cells[cells >= 0])
    if free.size:
        mask[0].reshape(-1)[int(free[0])] = 0
    mask[1] = 0
    mos = np.array([(0, -1, 1)[s % 3] for s in range(n)], np.int32)
    Y = np.ascontiguousarray(Yk.reshape(d.R, T, 2))
    return Y, fut, present, mask, mos


def constant_ids(fut):
    """The same targets with every slot's id constant over t (its first frame's): the evaluation form then counts what the prediction form counts."""
    f = fut.copy()
    f[..., 0] = f[:, :1, :, 0]
    return f, (f[:, 0, :, 0] != 0).reshape(-1).astype(np.uint8)


def conditions(Y, fut, horizons, grid, d):
    """The three fractions the generated inputs must reach, on the float64 statement alone: (non-empty (window, horizon, cell) with mass from two or
    more agents, counted (agent, frame) with two samples in one cell, samples off frame somewhere)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Oh, Ow = grid
    r = occupancy_f64(Y, fut, None, None, horizons, UNTIL, grid, None, None, d, want_marg=True)
    agents = (r["marg"].reshape(n, m, len(horizons), -1) > 0).sum(1)
    shared = float((agents >= 2).sum()) / max(1, int((agents >= 1).sum()))
    Yk = np.asarray(Y, np.float32).reshape(n, K, m, T, 2)
    cell = _cells(Yk[..., 0], Yk[..., 1], Oh, Ow, np.float64).transpose(0, 2, 3, 1)          # [n, m, T, K]
    c = _counted(fut, None, d)
    srt = np.sort(cell, -1)
    twice = ((srt[..., 1:] == srt[..., :-1]) & (srt[..., 1:] >= 0)).any(-1) if K > 1 else np.zeros(c.shape, bool)
    double = float((twice & c).sum()) / max(1, int(c.sum()))
    off = ((cell < 0) & c[..., None]).any(2)                                                  # [n, m, K]
    part = c.any(-1)
    away = float((off & part[..., None]).sum()) / max(1, int(part.sum()) * K)
    return shared, double, away
