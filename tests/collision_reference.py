"""Numpy statement of the collision-penalty contract (include/desire_hip.h: desire_collision_loss / desire_set_collision_loss) in two forms --
collision_f32, the contract's fp32 operation sequence, and collision_f64, the same in float64 --, the input generator their tests share, and the
float64 autograd reference of the training loss with the term (collision_loss_and_grads: the oracle's forward, the loss rebuilt).  Agent a =
scene * mno + slot, row r_k = (scene * K + k) * mno + slot.  The integer output (touch) of the two forms can only differ where a pair's q lies
within rounding of r2: the generator (tests/joint_reference.make_inputs) keeps every (pair, frame) further than MARGIN * r2 from r2 in float64,
and the tests assert it on "margin" of the float64 pass alone."""
import numpy as np

from tests.joint_reference import MARGIN, make_inputs

MEAN, MIN, SOFTMIN = 0, 1, 2
AGENT, SCENE = 0, 1
LDS_BYTES = 60 * 1024


def coll_lds_bytes(mno, tc):
    """CollLds(mno, tc).bytes() of desire_amd/csrc/eval_lds.h (tests/test_collision_cpu.py holds the two together)."""
    stride = mno + 1 if mno >= 32 else mno
    park = tc | 1
    return (tc * stride + mno * park) * 8 + 4 * (mno * park + 2 * mno + 1)


def coll_chunk_frames(mno, T):
    """Frames of a (window, k) unit one pass of the kernel's LDS plan holds: T when the unit fits, else the most that do."""
    if coll_lds_bytes(mno, T) <= LDS_BYTES:
        return T
    tc = 1
    while tc < T and coll_lds_bytes(mno, tc + 1) <= LDS_BYTES:
        tc += 1
    return tc


def coll_chunk_centres(mno, T):
    """Centre frames of the crossings for a chunked shape: contacts in the first chunk, straddling the first chunk border, and in the last chunk."""
    tc = coll_chunk_frames(mno, T)
    if tc >= T:
        return None
    last0 = ((T - 1) // tc) * tc
    return [tc // 2, tc - 1, tc, min(T - 2, last0 + (T - last0) // 2)]


def _collision(Y, fut, valid, radius, ux, uy, d, dtype):
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    f32 = np.float32
    ux, uy, r = dtype(f32(ux)), dtype(f32(uy)), dtype(f32(radius))
    r2 = r * r
    f = np.asarray(fut, f32)
    c = (f[..., 0] != 0).transpose(0, 2, 1)                                # [n, m, T]
    nfut = c.sum(-1)
    lmask = (np.asarray(valid).reshape(n, m) != 0) & (nfut > 0)
    cc = c & lmask[:, :, None]                                             # step 1
    nvalid = dtype(max(int(lmask.sum()), 1))
    nf = np.maximum(nfut, 1).astype(dtype)
    inv = np.where(lmask, dtype(1) / nf, dtype(0)).astype(dtype)           # [n, m]
    Yk = np.asarray(Y, f32).reshape(n, K, m, T, 2).astype(dtype)
    x, y = Yk[..., 0], Yk[..., 1]                                          # [n, K, m, T]
    s = np.zeros((n, K, m, T), dtype)
    gx, gy = np.zeros((n, K, m, T), dtype), np.zeros((n, K, m, T), dtype)
    touch = np.zeros((n, K), np.int64)
    margin = np.inf
    ci = cc[:, None]                                                       # [n, 1, m, T]
    with np.errstate(all="ignore"):
        for j in range(m):                                                 # the partners in increasing j, every operation rounded once
            a = (x - x[:, :, j:j + 1]) * ux
            b = (y - y[:, :, j:j + 1]) * uy
            q = a * a + b * b
            both = np.broadcast_to(ci & ci[:, :, j:j + 1], q.shape).copy()
            both[:, :, j] = False
            hit = both & (q < r2)                                          # step 2: strict, false for a NaN
            if r2 > 0:
                sel = np.isfinite(q)
                sel[:, :, j] = False
                if sel.any():
                    margin = min(margin, float(np.min(np.abs(q[sel].astype(np.float64) - float(r2)))) / float(r2))
            dist = np.sqrt(np.where(hit, q, dtype(1)))
            u = dtype(1) - dist / (r if r > 0 else dtype(1))
            s = np.where(hit, s + u * u, s)                                # steps 3, 4
            touch += hit[:, :, j + 1:].sum((2, 3))                         # step 5: the pairs i > j, once each
            push = hit & (dist > 0)
            cij = (inv[:, None, :, None] + inv[:, None, j, None, None]) * (u / (r * np.where(push, dist, dtype(1))))
            gx = np.where(push, gx + cij * a, gx)                          # step 7
            gy = np.where(push, gy + cij * b, gy)
        acc = np.zeros((n, K, m), dtype)
        for t in range(T):                                                 # the counted frames in increasing t
            acc = np.where(ci[..., t], acc + s[..., t], acc)
        col = np.where(lmask[:, None, :], acc / nf[:, None, :], dtype(0)).astype(dtype)
        col = np.ascontiguousarray(col.transpose(0, 2, 1)).reshape(n * m, K)
        scale = dtype(-2) / (nvalid * dtype(K))
        G = np.stack([(gx * ux) * scale, (gy * uy) * scale], -1).astype(dtype).reshape(n * K * m, T, 2)
        ma = np.zeros(n * m, dtype)                                        # step 6
        for k in range(K):
            ma = ma + col[:, k]
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
    return {"col": col, "touch": touch.astype(np.int32), "dY": G, "term": np.array([term], dtype), "margin": margin, "lmask": lmask.reshape(-1),
            "counted": cc}


def collision_f32(Y, fut, valid, radius, ux, uy, d):
    """The contract in fp32: col, dY, term and touch are the device's bits."""
    return _collision(Y, fut, valid, radius, ux, uy, d, np.float32)


def collision_f64(Y, fut, valid, radius, ux, uy, d):
    return _collision(Y, fut, valid, radius, ux, uy, d, np.float64)


def make_collision_inputs(d, radius, ux, uy, seed):
    """(Y [R, T, 2] fp32, fut [n, T, mno, 3] fp32, valid [A] uint8) from tests/joint_reference.make_inputs -- lattice slots with planted crossings
    (centred in the first chunk, on the chunk border and in the last chunk where the shape is walked in frame chunks), followers and coincident
    pairs, absent slots, slots that leave half way, a NaN row, the last of two or more windows empty; every (pair, frame) keeps the margin.  valid
    is presence in the first target frame, and from 8 slots on one fully present slot of window 0 is taken out of the loss mask by it alone."""
    Y, fut, present, _ = make_inputs(d, radius, ux, uy, seed, centres=coll_chunk_centres(d.mno, d.T_pred))
    valid = present.copy()
    if d.mno >= 8:
        full = np.nonzero((fut[0, :, :, 0] != 0).all(0))[0]
        valid[full[len(full) // 2]] = 0
    return Y, fut, valid


def past_with_valid(d, valid, seed=3):
    """A past tensor [n, T_obs, mno, 3] whose last observed frame carries `valid`: the way the mask reaches a handle (desire_encode)."""
    past = np.zeros((d.n_scenes, d.T_obs, d.mno, 3), np.float32)
    past[..., 0] = np.asarray(valid).reshape(d.n_scenes, 1, d.mno)
    past[..., 1:] = np.random.default_rng(seed).uniform(200, 900, past[..., 1:].shape) * (past[..., :1] != 0)
    return past


def collision_loss_and_grads(past, fut, eps, grids, gos, w_np, d, mode, tau, scope, ux, uy, quantile=0.25):
    """Float64 autograd of loss(mode, scope) + weight * L_col: the oracle's forward (oracle.desire_torch.forward_loss, used as it is), the
    reconstruction term rebuilt as tests/recon_reference.bom_loss_and_grads and tests/recon_scene_reference.scene_loss_and_grads rebuild it, the
    collision term from out["Y0"] with sqrt(q + 1e-300) for the root.  past / fut in the oracle layout [T, A, 3].  Radius and weight come from
    the float64 Y0 alone: the radius (rounded to fp32) is the distance below which `quantile` of the counted (pair, frame)s fall, the weight
    (rounded to fp32) makes the term's gradient on head/w as long as the rest of the loss's.  Returns (vals, grads): vals = radius, weight,
    L_col, loss, kld / ce / reg per agent, counted [A], touching (the number of touching ordered (pair, frame, k)), share (|d weight L_col / d
    head/w| over |d loss / d head/w|), Y0 [R, T, 2] and near (L_col's reduction of the number of partners within 1.01 radius per (agent, k,
    frame): phi is Lipschitz in the distance with constant 2 / radius, so L_col moves by at most (2 / radius) * near * the largest change
    of a pair's distance)."""
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
    # ---- the collision term on Y0
    fx, fy = float(np.float32(ux)), float(np.float32(uy))
    cc = pm * v.reshape(n, 1, m, 1)                                          # [n, 1, m, T]
    pair = cc.unsqueeze(3) * cc.unsqueeze(2) * (1.0 - torch.eye(m, dtype=OT.DT)).reshape(1, 1, m, m, 1)      # [n, 1, i, j, T]
    a = (Y0[..., 0].unsqueeze(3) - Y0[..., 0].unsqueeze(2)) * fx             # [n, K, i, j, T]
    b = (Y0[..., 1].unsqueeze(3) - Y0[..., 1].unsqueeze(2)) * fy
    dist = torch.sqrt(a * a + b * b + 1e-300)
    on = (pair > 0).expand_as(dist)
    radius = float(np.float32(np.quantile(dist.detach()[on].numpy(), quantile)))
    hinge = torch.clamp(1.0 - dist / radius, min=0.0) ** 2 * pair
    col = hinge.sum((3, 4)) / nfc.reshape(n, 1, m)                           # [n, K, i]
    L_col = (col.mean(1) * v.reshape(n, m)).sum() / n_valid
    near = ((dist.detach() < 1.01 * radius).to(OT.DT) * pair).sum((3, 4)) / nfc.reshape(n, 1, m)
    near = float((near.mean(1) * v.reshape(n, m)).sum() / n_valid)
    hw = w["head/w"]
    g_col = torch.autograd.grad(L_col, hw, retain_graph=True)[0]
    g_base = torch.autograd.grad(base, hw, retain_graph=True)[0]
    weight = float(np.float32(float(g_base.norm()) / float(g_col.norm())))
    loss = base + weight * L_col
    loss.backward()
    grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(t.shape)) for k, t in w.items()}
    vals = {"radius": radius, "weight": weight, "L_col": float(L_col.detach()), "loss": float(loss.detach()), "kld": out["kld"].detach().numpy(),
            "ce": out["ce"].detach().numpy(), "reg": out["reg"].detach().numpy(), "counted": v.numpy() != 0,
            "touching": int(((dist.detach() < radius) & on).sum()), "near": near,
            "Y0": out["Y0"].detach().numpy().reshape(n * K * m, T, 2), "share": weight * float(g_col.norm()) / float(np.linalg.norm(grads["head/w"]))}
    return vals, grads
