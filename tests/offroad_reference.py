"""Numpy statements of the off-road contracts (include/desire_hip.h: desire_mask_distance, desire_offroad_loss / desire_set_offroad_loss): the
distance field by brute force in float32 (mask_field_f32) and in the separable form the device uses (mask_field_separable_f32); the penalty in two
forms -- offroad_f32, the contract's fp32 operation sequence, and offroad_f64, the same in float64 --; the masks and inputs their tests share;
mirrors of the LDS plan (desire_amd/csrc/eval_lds.h: OffLds, offroad_geometry); and the float64 autograd reference of the training loss with the
term (offroad_loss_and_grads: the oracle's forward, the loss rebuilt as tests/collision_reference.py rebuilds it).  Agent a = scene * mno + slot,
row r_k = (scene * K + k) * mno + slot.  The integer output (count) and the taps of the two forms can only differ where a coordinate times the
side lies within rounding of a cell line (an integer) or of a cell centre line (an integer + 0.5): make_offroad_inputs keeps every position that
is not planted on one exactly at least MARGIN cells away, and the tests assert it on "margin" of the float64 pass alone."""
import numpy as np

from tests.collision_reference import AGENT, MEAN, MIN, SCENE, SOFTMIN, coll_chunk_frames, coll_lds_bytes  # noqa: F401

LDS_BYTES = 60 * 1024
MARGIN = 1e-3                                   # cells


# ---- the LDS plan -------------------------------------------------------------------------------------------------------------------------------
def off_lds_bytes(mno, tc, cells):
    """OffLds(mno, tc, cells).bytes(): the collision kernel's plan with the staged field behind it."""
    return coll_lds_bytes(mno, tc) + 4 * cells


def offroad_geometry(mno, T, Mh, Mw):
    """(frames per chunk, field staged in LDS) of offroad_geometry in eval_lds.h."""
    tc = coll_chunk_frames(mno, T)
    return tc, off_lds_bytes(mno, tc, Mh * Mw) <= LDS_BYTES


# ---- the distance field ---------------------------------------------------------------------------------------------------------------------------
def mask_field_f32(mask, cell_x, cell_y):
    """The statement itself: per cell the min over every traversable cell of a * a + b * b in float32, then the root.  mask [n, Mh, Mw]."""
    f32 = np.float32
    mask = np.asarray(mask)
    n, Mh, Mw = mask.shape
    cx, cy = f32(cell_x), f32(cell_y)
    out = np.zeros((n, Mh, Mw), f32)
    yy, xx = np.meshgrid(np.arange(Mh), np.arange(Mw), indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    for i in range(n):
        ys, xs = np.nonzero(mask[i])
        if ys.size == 0:
            continue                                                   # no traversable cell: 0.f everywhere
        best = np.empty(Mh * Mw, f32)
        step = max(1, (1 << 22) // ys.size)
        for c0 in range(0, Mh * Mw, step):
            a = (xx[c0:c0 + step, None] - xs[None, :]).astype(f32) * cx
            b = (yy[c0:c0 + step, None] - ys[None, :]).astype(f32) * cy
            best[c0:c0 + step] = (a * a + b * b).min(1)
        out[i] = np.sqrt(best).reshape(Mh, Mw)
    return out


def mask_field_separable_f32(mask, cell_x, cell_y):
    """The device's two passes: g(y, x') = rows to the nearest traversable cell of column x', then per cell the min over the columns that have one."""
    f32 = np.float32
    mask = np.asarray(mask)
    n, Mh, Mw = mask.shape
    cx, cy = f32(cell_x), f32(cell_y)
    NONE = np.iinfo(np.int32).max
    out = np.zeros((n, Mh, Mw), f32)
    for i in range(n):
        g = np.full((Mh, Mw), NONE, np.int64)
        d = np.full(Mw, NONE, np.int64)
        for y in range(Mh):                                            # down
            d = np.where(mask[i, y] != 0, 0, np.where(d == NONE, NONE, d + 1))
            g[y] = d
        d = np.full(Mw, NONE, np.int64)
        for y in range(Mh - 1, -1, -1):                                # up
            d = np.where(mask[i, y] != 0, 0, np.where(d == NONE, NONE, d + 1))
            g[y] = np.minimum(g[y], d)
        cols = np.nonzero(g[0] != NONE)[0]
        if cols.size == 0:
            continue
        a = (np.arange(Mw)[:, None] - cols[None, :]).astype(f32) * cx      # [x, x']
        aa = a * a
        for y in range(Mh):
            b = g[y, cols].astype(f32) * cy
            out[i, y] = np.sqrt((aa + (b * b)[None, :]).min(1))
    return out


# ---- the penalty ----------------------------------------------------------------------------------------------------------------------------------
def _offroad(Y, fut, valid, field, fos, scale, d, dtype):
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    f32 = np.float32
    field = np.asarray(field, f32)
    _, Mh, Mw = field.shape
    fos = np.asarray(fos).reshape(n)
    sc = dtype(f32(scale))
    fMw, fMh, xmax, ymax = dtype(Mw), dtype(Mh), dtype(Mw - 1), dtype(Mh - 1)
    half, two = dtype(0.5), dtype(2)
    f = np.asarray(fut, f32)
    c = (f[..., 0] != 0).transpose(0, 2, 1)                                # [n, m, T]
    nfut = c.sum(-1)
    lmask = (np.asarray(valid).reshape(n, m) != 0) & (nfut > 0)
    has = fos >= 0
    live = lmask & has[:, None]                                            # agents that can cost anything
    cc = c & live[:, :, None]
    nvalid = dtype(max(int(lmask.sum()), 1))                               # (of the loss mask: a window without a field still counts its agents)
    nf = np.maximum(nfut, 1).astype(dtype)
    inv = np.where(live, dtype(1) / nf, dtype(0)).astype(dtype)            # [n, m]
    nk = nvalid * dtype(K)
    Yk = np.asarray(Y).reshape(n, K, m, T, 2).astype(dtype)
    phi = np.zeros((n, K, m, T), dtype)
    G = np.zeros((n, K, m, T, 2), dtype)
    count = np.zeros((n, K), np.int64)
    margin = np.full((n, K, m, T), np.inf)
    with np.errstate(all="ignore"):
        for w in range(n):
            if not has[w]:
                continue
            D = field[fos[w]].astype(dtype)
            x, y = Yk[w, ..., 0], Yk[w, ..., 1]                            # [K, m, T]
            ok = cc[w][None] & ~np.isnan(x) & ~np.isnan(y)
            xs, ys = np.where(ok, x, dtype(0)), np.where(ok, y, dtype(0))
            xm, ym = xs * fMw, ys * fMh                                    # step 1
            u, v = xm - half, ym - half
            uc, vc = np.minimum(np.maximum(u, dtype(0)), xmax), np.minimum(np.maximum(v, dtype(0)), ymax)
            ufl, vfl = np.floor(uc), np.floor(vc)
            x0, y0 = ufl.astype(np.int64), vfl.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, Mw - 1), np.minimum(y0 + 1, Mh - 1)
            fx, fy = uc - ufl, vc - vfl
            D00, D01, D10, D11 = D[y0, x0], D[y0, x1], D[y1, x0], D[y1, x1]      # step 2
            h0, h1 = D01 - D00, D11 - D10
            top, bot = D00 + fx * h0, D10 + fx * h1
            vd = bot - top
            dd = top + fy * vd
            e = dd / sc                                                    # step 3
            phi[w] = np.where(ok, e * e, dtype(0))
            sx = np.where((u >= 0) & (u <= xmax), (h0 + fy * (h1 - h0)) * fMw, dtype(0))     # step 7
            sy = np.where((v >= 0) & (v <= ymax), vd * fMh, dtype(0))
            mm = (two * e) / sc
            coef = (inv[w] / nk)[None, :, None]
            G[w, ..., 0] = np.where(ok, (mm * sx) * coef, dtype(0))
            G[w, ..., 1] = np.where(ok, (mm * sy) * coef, dtype(0))
            cx, cy = np.floor(xm), np.floor(ym)                            # step 5
            inf = (cx >= 0) & (cx <= xmax) & (cy >= 0) & (cy <= ymax)
            cell = D[np.where(inf, cy, 0).astype(np.int64), np.where(inf, cx, 0).astype(np.int64)]
            count[w] = (ok & inf & (cell > 0)).sum((1, 2))
            x64, y64 = xs.astype(np.float64) * Mw, ys.astype(np.float64) * Mh
            gap = np.minimum(np.abs(2 * x64 - np.rint(2 * x64)), np.abs(2 * y64 - np.rint(2 * y64))) / 2
            margin[w] = np.where(ok, gap, np.inf)
        acc = np.zeros((n, K, m), dtype)
        for t in range(T):                                                 # step 4: the counted frames in increasing t
            acc = np.where(cc[:, None, :, t], acc + phi[..., t], acc)
        off = np.where(live[:, None, :], acc / nf[:, None, :], dtype(0)).astype(dtype)
        off = np.ascontiguousarray(off.transpose(0, 2, 1)).reshape(n * m, K)
        ma = np.zeros(n * m, dtype)                                        # step 6
        for k in range(K):
            ma = ma + off[:, k]
        ma = ma / dtype(K)
        S = np.zeros(256, dtype)
        for a0 in range(0, n * m, 256):
            part = ma[a0:a0 + 256]
            S[:part.size] = S[:part.size] + part
        st = 128
        while st > 0:
            S[:st] = S[:st] + S[st:2 * st]
            st //= 2
        term = dtype(S[0] / nvalid)
    return {"off": off, "count": count.astype(np.int32), "dY": G.reshape(n * K * m, T, 2), "term": np.array([term], dtype), "margin": margin,
            "lmask": lmask.reshape(-1), "counted": cc, "phi": phi}


def offroad_f32(Y, fut, valid, field, fos, scale, d):
    """The contract in fp32: off, dY, term and count are the device's bits."""
    return _offroad(Y, fut, valid, field, fos, scale, d, np.float32)


def offroad_f64(Y, fut, valid, field, fos, scale, d):
    """The same sequence in float64 (Y may be float64 itself: the central differences step it)."""
    return _offroad(Y, fut, valid, field, fos, scale, d, np.float64)


def positive_share(res):
    """The share of the counted positions with phi > 0 (between a quarter and three quarters: neither all road nor all wall)."""
    cnt = np.broadcast_to(res["counted"][:, None], res["phi"].shape)
    return float((res["phi"][cnt] > 0).mean()) if cnt.any() else 0.0


# ---- masks and inputs -------------------------------------------------------------------------------------------------------------------------------
def make_masks(n_masks, Mh, Mw, seed):
    """Road masks [n_masks, Mh, Mw] uint8: a wall band along the top with a wavy edge (a phase per mask) and a wall block inside the road."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(Mh), np.arange(Mw), indexing="ij")
    out = np.ones((n_masks, Mh, Mw), np.uint8)
    for i in range(n_masks):
        ph = rng.uniform(0, 2 * np.pi)
        # (a coarse mask is off the road a cell around every wall cell: a narrower band gives it the same share of off-road positions)
        edge = Mh * ((0.22 if Mh < 16 else 0.38) + 0.08 * np.sin(2 * np.pi * xx / max(Mw, 2) + ph))
        out[i][yy + 0.5 < edge] = 0
        bx, by = rng.uniform(0.45, 0.6), rng.uniform(0.5, 0.65)
        out[i][(xx >= bx * Mw) & (xx < (bx + 0.25) * Mw) & (yy >= by * Mh) & (yy < (by + 0.2) * Mh)] = 0
    return out


def cell_sizes(d, Mh, Mw):
    """The cell of a mask over the normalised frame, in pixels (what DESIREModel.set_scene_masks passes)."""
    return float(np.float32((1.0 / d.sx) / Mw)), float(np.float32((1.0 / d.sy) / Mh))


def centre(M):
    """A coordinate exactly on a cell centre of an axis of M cells, exact in fp32 for an odd M or a power of two."""
    return np.float32((M // 2 + 0.5) / M)


def make_offroad_inputs(d, Mh, Mw, seed):
    """(Y [R, T, 2] fp32, fut [n, T, mno, 3] fp32, valid [A] uint8, planted [R, T] bool): positions uniform over [-0.08, 1.08]^2 -- so some are
    clamped on every side and some are negative --, every one at least MARGIN cells from a cell line and a centre line; planted on the first counted
    rows: a position exactly on a cell centre, x = 1.0 exactly, a NaN x and a NaN y.  Slots absent altogether, slots that leave half way, from 8
    slots on one fully present slot taken out of the loss mask by `valid` alone, and from three windows on the last window empty."""
    rng = np.random.default_rng(seed)
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    fut = np.zeros((n, T, m, 3), np.float32)
    fut[..., 0] = np.arange(1, m + 1)
    fut[..., 1:] = rng.uniform(100, 1000, (n, T, m, 2))
    for s in range(m):
        if m >= 5 and s % 5 == 4:
            fut[:, :, s] = 0                                               # absent
        elif m >= 4 and s % 7 == 3:
            fut[:, T // 2:, s] = 0                                         # leaves half way
    if n >= 3:
        fut[-1] = 0                                                        # a window of none
    valid = (fut[:, 0, :, 0] != 0).astype(np.uint8).reshape(-1)
    if m >= 8:
        valid[1] = 0                                                       # present in every frame, not in the loss mask
    P = rng.uniform(-0.08, 1.08, (n, K, m, T, 2))
    for ax, M in ((0, Mw), (1, Mh)):                                       # the margin, in float64 on twice the cell coordinate
        z = 2 * P[..., ax] * M
        near = np.abs(z - np.rint(z)) < 4 * MARGIN
        P[..., ax] = np.where(near, P[..., ax] + 0.01 / M, P[..., ax])
    Y = P.astype(np.float32)
    planted = np.zeros((n, K, m, T), bool)
    s0 = 0                                                                 # slot 0 is counted in every frame of window 0
    Y[0, 0, s0, 0] = (centre(Mw), centre(Mh)); planted[0, 0, s0, 0] = True
    Y[0, 0, s0, 1, 0] = 1.0; planted[0, 0, s0, 1] = True                  # (on the frame's edge: exact in both precisions)
    Y[0, 0, s0, 2, 0] = np.nan; planted[0, 0, s0, 2] = True
    Y[0, K - 1, s0, 3, 1] = np.nan; planted[0, K - 1, s0, 3] = True
    return np.ascontiguousarray(Y.reshape(n * K * m, T, 2)), fut, valid, planted


def default_fos(n):
    """Window -> field for two fields: windows 0 and 1 on different fields; from three windows on window 1 has none (it holds agents: the negative
    entry is what silences it) and the others alternate."""
    fos = np.array([(1, 0)[i % 2] for i in range(n)], np.int32)
    if n >= 3:
        fos[1] = -1
    return fos


# ---- float64 autograd of the training loss with the term ------------------------------------------------------------------------------------------------
def masks_from_positions(Y0, counted, d, Mh, Mw):
    """One mask per window from that window's own counted positions [n, K, m, T, 2]: the cells on one side of a diagonal through the median cell
    of the positions are wall (above and left of it in even windows, below and left of it in odd ones), the rest road -- about half of the
    positions stand off the road wherever the model happens to put them, and the field slopes in x and in y, so that both components of the
    gradient and both clamps are in the step's comparison."""
    n = d.n_scenes
    masks = np.ones((n, Mh, Mw), np.uint8)
    yy, xx = np.meshgrid(np.arange(Mh), np.arange(Mw), indexing="ij")
    for w in range(n):
        sel = np.broadcast_to(counted[w][None], Y0.shape[1:4])
        if not sel.any():
            continue
        mc = int(np.median(np.floor(Y0[w, ..., 0][sel] * Mw)))
        mr = int(np.median(np.floor(Y0[w, ..., 1][sel] * Mh)))
        side = (yy - mr) if w % 2 == 0 else (mr - yy)
        masks[w][(xx - mc) + side < 0] = 0
    return masks


def offroad_loss_and_grads(past, fut, eps, grids, gos, w_np, d, mode, tau, scope, Mh, Mw, scale, boost=1.5, collision=None):
    """Float64 autograd of loss(mode, scope) + weight * L_off (+ cw * L_col with collision = (radius, cw): the collision term as
    tests/collision_reference.collision_loss_and_grads states it): the oracle's forward (oracle.desire_torch.forward_loss, used as it is), the
    reconstruction term rebuilt, the off-road term from out["Y0"] against the fp32 brute-force field of masks_from_positions (cells in pixels).
    past / fut in the oracle layout [T, A, 3].  The weight (rounded to fp32) is `boost` times what makes the term's gradient on head/w as long as
    the rest of the loss's, so that the term carries at least boost / (1 + boost) of the whole.  Returns (vals, grads): vals = masks, field,
    weight, scale, L_off, L_col, loss, counted [A], margin (cells, of the counted positions of Y0 to the nearest cell or centre line), share, Y0
    [R, T, 2], positive (share of the counted positions with phi > 0)."""
    import torch
    from oracle import desire_torch as OT
    w = OT.leaf_weights(w_np)
    out = OT.forward_loss(past, fut, eps, grids, gos, w, d)
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    pres = torch.as_tensor(np.asarray(fut)[:, :, 0] != 0)
    pm = pres.T.reshape(n, 1, m, T).to(OT.DT)
    nf = pres.sum(0).to(OT.DT)
    nfc = torch.clamp(nf, min=1.0)
    valid = torch.as_tensor(np.asarray(past)[d.T_obs - 1, :, 0] != 0)
    v = (valid & (nf > 0)).to(OT.DT)
    n_valid = torch.clamp(v.sum(), min=1.0)
    gt = torch.as_tensor(OT.O.normalise(fut, d, np.float64), dtype=OT.DT).permute(1, 0, 2).reshape(n, 1, m, T, 2)
    Y0 = out["Y0"].reshape(n, K, m, T, 2)
    e0 = torch.sqrt(((Y0 - gt) ** 2).sum(-1) + 1e-300)
    e = (e0 * pm).sum(3) / nfc.reshape(n, 1, m)                              # [n, K, m]
    if scope == SCENE and mode != MEAN:
        vw = v.reshape(n, 1, m)
        E = (e * vw).sum(2) / torch.clamp(vw.sum(2), min=1.0)
        R = E.min(dim=1).values if mode == MIN else -float(tau) * (torch.logsumexp(-E / float(tau), dim=1) - float(np.log(K)))
        recon = R.reshape(n, 1).expand(n, m).reshape(d.A)
    elif mode == MIN:
        recon = e.min(dim=1).values.reshape(d.A)
    elif mode == SOFTMIN:
        recon = (-float(tau) * (torch.logsumexp(-e / float(tau), dim=1) - float(np.log(K)))).reshape(d.A)
    else:
        recon = e.mean(dim=1).reshape(d.A)
    base = ((recon + out["kld"]) * v).sum() / n_valid + out["L_ioc"]
    cc = pm * v.reshape(n, 1, m, 1)                                          # [n, 1, m, T]
    L_col = torch.zeros((), dtype=OT.DT)
    if collision is not None:
        radius, cw = collision
        fx, fy = float(np.float32(1.0 / d.sx)), float(np.float32(1.0 / d.sy))
        pair = cc.unsqueeze(3) * cc.unsqueeze(2) * (1.0 - torch.eye(m, dtype=OT.DT)).reshape(1, 1, m, m, 1)
        a = (Y0[..., 0].unsqueeze(3) - Y0[..., 0].unsqueeze(2)) * fx
        b = (Y0[..., 1].unsqueeze(3) - Y0[..., 1].unsqueeze(2)) * fy
        dist = torch.sqrt(a * a + b * b + 1e-300)
        hinge = torch.clamp(1.0 - dist / float(np.float32(radius)), min=0.0) ** 2 * pair
        L_col = ((hinge.sum((3, 4)) / nfc.reshape(n, 1, m)).mean(1) * v.reshape(n, m)).sum() / n_valid
        base = base + float(np.float32(cw)) * L_col
    # ---- the off-road term on Y0
    counted = (cc.reshape(n, m, T) > 0).numpy()
    Y0n = Y0.detach().numpy()
    masks = masks_from_positions(Y0n, counted, d, Mh, Mw)
    cell_x, cell_y = cell_sizes(d, Mh, Mw)
    field = mask_field_f32(masks, cell_x, cell_y)
    Dt = torch.as_tensor(field.astype(np.float64))
    widx = torch.arange(n).reshape(n, 1, 1, 1).expand(n, K, m, T)
    u = Y0[..., 0] * float(Mw) - 0.5
    vv = Y0[..., 1] * float(Mh) - 0.5
    uc, vc = torch.clamp(u, 0.0, float(Mw - 1)), torch.clamp(vv, 0.0, float(Mh - 1))
    x0, y0 = torch.floor(uc.detach()).long(), torch.floor(vc.detach()).long()
    x1, y1 = torch.clamp(x0 + 1, max=Mw - 1), torch.clamp(y0 + 1, max=Mh - 1)
    fx_, fy_ = uc - x0.to(OT.DT), vc - y0.to(OT.DT)
    D00, D01, D10, D11 = Dt[widx, y0, x0], Dt[widx, y0, x1], Dt[widx, y1, x0], Dt[widx, y1, x1]
    top, bot = D00 + fx_ * (D01 - D00), D10 + fx_ * (D11 - D10)
    dd = top + fy_ * (bot - top)
    sc = float(np.float32(scale))
    phi = (dd / sc) ** 2 * cc
    off = phi.sum(3) / nfc.reshape(n, 1, m)                                  # [n, K, m]
    L_off = (off.mean(1) * v.reshape(n, m)).sum() / n_valid
    hw = w["head/w"]
    g_off = torch.autograd.grad(L_off, hw, retain_graph=True)[0]
    g_base = torch.autograd.grad(base, hw, retain_graph=True)[0]
    weight = float(np.float32(boost * float(g_base.norm()) / float(g_off.norm())))
    loss = base + weight * L_off
    loss.backward()
    grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(t.shape)) for k, t in w.items()}
    sel = np.broadcast_to(counted[:, None], (n, K, m, T))
    z = np.stack([2 * Y0n[..., 0] * Mw, 2 * Y0n[..., 1] * Mh], -1)
    gap = (np.abs(z - np.rint(z)).min(-1) / 2)[sel]
    vals = {"masks": masks, "field": field, "weight": weight, "scale": sc, "L_off": float(L_off.detach()), "L_col": float(L_col.detach()),
            "loss": float(loss.detach()), "kld": out["kld"].detach().numpy(), "ce": out["ce"].detach().numpy(), "reg": out["reg"].detach().numpy(),
            "counted": v.numpy() != 0, "margin": float(gap.min()), "positive": float((phi.detach().numpy()[sel] > 0).mean()),
            "Y0": Y0n.reshape(n * K * m, T, 2), "share": weight * float(g_off.norm()) / float(np.linalg.norm(grads["head/w"]))}
    return vals, grads
