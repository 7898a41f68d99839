"""Numpy statement of the reconstruction-weight contract (include/desire_hip.h: desire_recon_weights / desire_set_recon_loss) in two forms --
recon_f32, the contract's fp32 operation sequence, and recon_f64, the same in float64 --, the input generator their tests share, and the float64
autograd reference of the training loss under a mode (bom_loss_and_grads: the oracle's forward, its reconstruction term rebuilt).  Agent a =
scene * mno + slot, row r_k = (scene * K + k) * mno + slot.  The winner of the two forms can only differ where the two smallest errors of an
agent lie within rounding of each other: the generator keeps them further apart than GAP * e in float64 (asserted on the float64 pass alone),
except for the agents it gives two bit-identical rows -- there the tie goes to the lower k in either precision."""
import numpy as np

MEAN, MIN, SOFTMIN = 0, 1, 2
# fp32 rounding of e (T_pred additions of correctly rounded terms, one division) stays below (T_pred + 4) * 2^-24 relative, 2.7e-6 at T_pred = 40
GAP = 1e-3


def _recon(Y, fut, valid, d, mode, tau, dtype):
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    f32 = np.float32
    f = np.asarray(fut, f32)
    c = (f[..., 0] != 0).transpose(0, 2, 1)                                                       # [n, m, T]
    g = np.stack([f[..., 1] * f32(d.sx), f[..., 2] * f32(d.sy)], -1).astype(f32).transpose(0, 2, 1, 3).astype(dtype)   # rounded once in fp32: an input
    nfut = c.sum(-1)
    lmask = (np.asarray(valid).reshape(n, m) != 0) & (nfut > 0)
    Yk = np.asarray(Y, f32).reshape(n, K, m, T, 2).astype(dtype)
    s = np.zeros((n, K, m), dtype)
    with np.errstate(all="ignore"):
        for t in range(T):                                                                        # increasing t from 0.f, every operation rounded once
            dx = Yk[:, :, :, t, 0] - g[:, None, :, t, 0]
            dy = Yk[:, :, :, t, 1] - g[:, None, :, t, 1]
            term = np.sqrt(dx * dx + dy * dy)
            s = np.where(c[:, None, :, t], s + term, s)
        e = np.where(lmask[:, None, :], s / np.maximum(nfut, 1).astype(dtype)[:, None, :], dtype(0))
        e = np.ascontiguousarray(e.transpose(0, 2, 1)).reshape(n * m, K).astype(dtype)            # [A, K]
        win = np.zeros(n * m, np.int32)
        mval = e[:, 0].copy()
        for k in range(1, K):                                                                     # strict: a tie stays with the lower k; a NaN gives way
            take = (e[:, k] < mval) | (np.isnan(mval) & ~np.isnan(e[:, k]))
            win = np.where(take, k, win).astype(np.int32)
            mval = np.where(take, e[:, k], mval)
        if mode == MIN:
            w = (np.arange(K)[None, :] == win[:, None]).astype(dtype)
            recon = mval
        elif mode == SOFTMIN:
            tau = dtype(f32(tau))
            x = np.exp(-(e - mval[:, None]) / tau).astype(dtype)
            S = np.zeros(n * m, dtype)
            for k in range(K):
                S = S + x[:, k]
            w = x / S[:, None]
            recon = mval - tau * np.log(S / dtype(K))
        else:
            S = np.zeros(n * m, dtype)
            for k in range(K):
                S = S + e[:, k]
            w = np.full((n * m, K), dtype(1) / dtype(K), dtype)
            recon = S / dtype(K)
    srt = np.sort(np.where(np.isnan(e), np.inf, e), axis=1)
    gap = (srt[:, 1] - srt[:, 0]) if K > 1 else np.full(n * m, np.inf)
    return {"e": e, "w": w.astype(dtype), "winner": win, "recon": recon.astype(dtype), "lmask": lmask.reshape(-1), "gap": gap}


def recon_f32(Y, fut, valid, d, mode, tau=0.0):
    """The contract in fp32: e, recon (MIN, MEAN) and winner are the device's bits; w and recon of SOFTMIN up to the device's expf / logf."""
    return _recon(Y, fut, valid, d, mode, tau, np.float32)


def recon_f64(Y, fut, valid, d, mode, tau=0.0):
    return _recon(Y, fut, valid, d, mode, tau, np.float64)


def make_recon_case(d, seed):
    """(Y [R, T, 2] fp32, fut [n, T, mno, 3] fp32 in pixels, valid [A] uint8, ties [A] bool): samples scattered around the target at a
    per-sample scale, with absent agents (valid 0), agents with no counted frame, partly counted rows and -- for K > 1 -- agents whose two best
    rows are bit-identical (ties).  Every other counted agent's two smallest float64 errors differ by at least GAP * e (asserted here)."""
    rng = np.random.default_rng(seed)
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    A = n * m
    fut = np.zeros((n, T, m, 3), np.float32)
    fut[..., 0] = np.arange(1, m + 1)
    fut[..., 1] = np.round(rng.uniform(100, 1300, (n, T, m)) * 2) / 2
    fut[..., 2] = np.round(rng.uniform(100, 1000, (n, T, m)) * 2) / 2
    valid = np.ones(A, np.uint8)
    kind = rng.permutation(A) % 8 if A >= 8 else np.arange(A) + 4         # small cases: partly counted, ties and plain agents only
    absent = kind == 0
    none_counted = kind == 1
    partly = (kind == 2) | (kind == 3) | (kind == 4)
    ties = ((kind == 5) | (kind == 2)) & (K > 1)
    valid[absent] = 0
    fr = fut.transpose(0, 2, 1, 3).reshape(A, T, 3).copy()
    fr[none_counted, :, 0] = 0
    for a in np.nonzero(partly)[0]:
        drop = rng.random(T) < 0.4
        drop[rng.integers(T)] = False                                       # at least one counted frame stays
        fr[a, drop, 0] = 0
    fut = np.ascontiguousarray(fr.reshape(n, m, T, 3).transpose(0, 2, 1, 3))
    g = np.stack([fut[..., 1] * np.float32(d.sx), fut[..., 2] * np.float32(d.sy)], -1).transpose(0, 2, 1, 3)       # [n, m, T, 2]

    def draw(shape_k):
        scale = rng.uniform(0.01, 0.08, shape_k + (1, 1))
        return (scale * rng.normal(0, 1, shape_k + (T, 2))).astype(np.float32)

    Y = (g[:, None] + draw((n, K, m))).astype(np.float32)                    # [n, K, m, T, 2]
    for _ in range(50):
        r = recon_f64(Y.reshape(-1, T, 2), fut, valid, d, MIN)
        bad = r["lmask"] & (r["gap"] < 4 * GAP * r["e"].min(1))
        if not bad.any():
            break
        for a in np.nonzero(bad)[0]:                                        # redraw the agent's K rows
            Y[a // m, :, a % m] = g[a // m, a % m][None] + draw((K,))
    for a in np.nonzero(ties)[0]:                                           # the winner's row once more, at a later (or earlier) k
        r_a = recon_f64(Y.reshape(-1, T, 2), fut, valid, d, MIN)["winner"][a]
        other = (int(r_a) + 1 + int(rng.integers(K - 1))) % K
        Y[a // m, other, a % m] = Y[a // m, r_a, a % m]
    Y = np.ascontiguousarray(Y.reshape(n * K * m, T, 2))
    r = recon_f64(Y, fut, valid, d, MIN)
    plain = r["lmask"] & ~ties
    assert (r["gap"][plain] >= GAP * r["e"].min(1)[plain]).all()
    assert (r["gap"][r["lmask"] & ties] == 0).all()
    return Y, fut, valid, ties


def bom_loss_and_grads(past, fut, eps, grids, gos, w_np, d, mode, tau=0.0):
    """Float64 autograd of the training loss with the mode's reconstruction term: the oracle's forward (oracle.desire_torch.forward_loss, which
    keeps the autograd graph of Y0, kld, ce, reg), the loss rebuilt with recon from out["Y0"], backpropagated.  past / fut in the oracle layout
    [T, A, 3].  Returns (vals, grads): vals = recon / kld / ce / reg per agent, loss, e [A, K], winner [A], gap [A] (second smallest - smallest
    e, absolute), counted [A]."""
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
    e0 = torch.sqrt(((out["Y0"].reshape(n, K, m, T, 2) - gt) ** 2).sum(-1) + 1e-300)
    e = (e0 * pm).sum(3) / nfc.reshape(n, 1, m)                              # [n, K, m]
    if mode == MIN:
        recon = e.min(dim=1).values
    elif mode == SOFTMIN:
        recon = -float(tau) * (torch.logsumexp(-e / float(tau), dim=1) - float(np.log(K)))
    else:
        recon = e.mean(dim=1)
    recon = recon.reshape(d.A)
    loss = ((recon + out["kld"]) * v).sum() / n_valid + out["L_ioc"]
    loss.backward()
    grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(t.shape)) for k, t in w.items()}
    e_np = e.detach().permute(0, 2, 1).reshape(d.A, K).numpy()
    srt = np.sort(e_np, axis=1)
    vals = {"recon": recon.detach().numpy(), "kld": out["kld"].detach().numpy(), "ce": out["ce"].detach().numpy(),
            "reg": out["reg"].detach().numpy(), "loss": float(loss.detach()), "e": e_np, "winner": e_np.argmin(1).astype(np.int32),
            "gap": srt[:, 1] - srt[:, 0] if K > 1 else np.full(d.A, np.inf), "counted": v.numpy() != 0}
    return vals, grads
