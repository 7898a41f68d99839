"""Numpy statement of the scene scope of the reconstruction weights (include/desire_hip.h: desire_recon_weights_scene / desire_set_recon_scope) in
two forms -- scene_f32, the contract's fp32 operation sequence, and scene_f64, the same in float64 --, a generator of windows with a known best
world, and the float64 autograd reference of the training loss under a mode in the scene scope (scene_loss_and_grads: the oracle's forward, its
reconstruction term rebuilt per window).  Built on tests/recon_reference.py's e: step 1 is that file's, unchanged.  Window w = a // mno; a world
is sample k of every agent of a window."""
import numpy as np

from tests.recon_reference import MEAN, MIN, SOFTMIN, _recon, make_recon_case


def _walk(E, dtype):
    """The winner walk of the contract over the last axis of E [n, K]: strict, ties to the lower k, a NaN gives way to any number."""
    n, K = E.shape
    win = np.zeros(n, np.int32)
    m = E[:, 0].copy()
    for k in range(1, K):
        take = (E[:, k] < m) | (np.isnan(m) & ~np.isnan(E[:, k]))
        win = np.where(take, k, win).astype(np.int32)
        m = np.where(take, E[:, k], m)
    return win, m.astype(dtype)


def _scene(Y, fut, valid, d, mode, tau, dtype):
    n, K, m = d.n_scenes, d.K, d.mno
    base = _recon(Y, fut, valid, d, MIN, 0.0, dtype)                         # step 1: e [A, K], lmask [A]
    e, lmask = base["e"], base["lmask"].reshape(n, m)
    count = lmask.sum(1).astype(np.int32)
    with np.errstate(all="ignore"):
        S = np.zeros((n, K), dtype)
        for s in range(m):                                                     # increasing slot from 0.f, the counted slots only
            S = np.where(lmask[:, s, None], S + e.reshape(n, m, K)[:, s], S)
        E = np.where(count[:, None] > 0, S / np.maximum(count, 1).astype(dtype)[:, None], dtype(0)).astype(dtype)
        win, mval = _walk(E, dtype)
        if mode == MIN:
            W = (np.arange(K)[None, :] == win[:, None]).astype(dtype)
            R = mval
        elif mode == SOFTMIN:
            tau = dtype(np.float32(tau))
            x = np.exp(-(E - mval[:, None]) / tau).astype(dtype)
            Ssum = np.zeros(n, dtype)
            for k in range(K):
                Ssum = Ssum + x[:, k]
            W = x / Ssum[:, None]
            R = mval - tau * np.log(Ssum / dtype(K))
        else:
            Ssum = np.zeros(n, dtype)
            for k in range(K):
                Ssum = Ssum + E[:, k]
            W = np.full((n, K), dtype(1) / dtype(K), dtype)
            R = Ssum / dtype(K)
    W, R = W.astype(dtype), R.astype(dtype)
    srt = np.sort(np.where(np.isnan(E), np.inf, E), axis=1)
    with np.errstate(invalid="ignore"):                                        # (inf - inf where fewer than two worlds are numbers)
        gap = (srt[:, 1] - srt[:, 0]) if K > 1 else np.full(n, np.inf)
    return {"e": e, "E": E, "count": count, "W": W, "R": R, "winner_w": win, "gap": gap, "lmask": lmask.reshape(-1),
            "w": np.ascontiguousarray(np.repeat(W, m, axis=0)), "winner": np.repeat(win, m).astype(np.int32), "recon": np.repeat(R, m)}


def scene_f32(Y, fut, valid, d, mode, tau=0.0):
    """The contract in fp32: e, E, count, winner and -- in MEAN and MIN -- w and recon are the device's bits; w and recon of SOFTMIN up to the
    device's expf / logf.  "W" [n, K], "R" [n], "winner_w" [n] are per window; "w" [A, K], "winner" [A], "recon" [A] the same on every slot."""
    return _scene(Y, fut, valid, d, mode, tau, np.float32)


def scene_f64(Y, fut, valid, d, mode, tau=0.0):
    return _scene(Y, fut, valid, d, mode, tau, np.float64)


SCENE_GAP = 1e-3     # relative float64 gap between a window's best and second world the generator keeps: far above the fp32 rounding of E
                     # ((T_pred + mno + 5) * 2^-24 relative: T_pred additions and a division in e, mno additions and a division in E)


def make_scene_case(d, seed, empty_window=None, tie_window=None):
    """make_recon_case's (Y, fut, valid) with window-level conditions: `empty_window` has no counted agent (all absent), in `tie_window` the best
    world's rows are copied into another world (a bit-identical tie: the lower k wins in either precision), and every other window with K > 1
    keeps its two smallest float64 world errors at least SCENE_GAP * E apart (asserted): the worlds are re-drawn at per-world scales, so one
    world is the best for the whole window.  Returns (Y, fut, valid, tied [n] bool)."""
    rng = np.random.default_rng(seed + 7)
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Y, fut, valid, _ = make_recon_case(d, seed)
    valid = valid.copy()
    if empty_window is not None:
        valid[empty_window * m:(empty_window + 1) * m] = 0
    g = np.stack([fut[..., 1] * np.float32(d.sx), fut[..., 2] * np.float32(d.sy)], -1).transpose(0, 2, 1, 3)       # [n, m, T, 2]
    Y = Y.reshape(n, K, m, T, 2).copy()
    for _ in range(50):
        scale = rng.uniform(0.01, 0.08, (n, K, 1, 1, 1)) * rng.uniform(0.8, 1.25, (n, K, m, 1, 1))                  # a world's scale, jittered per agent
        Y = (g[:, None] + scale * rng.normal(0, 1, (n, K, m, T, 2))).astype(np.float32)
        r = scene_f64(Y.reshape(-1, T, 2), fut, valid, d, MIN)
        if K == 1 or not ((r["count"] > 0) & (r["gap"] < 4 * SCENE_GAP * r["E"].min(1))).any():
            break
    tied = np.zeros(n, bool)
    if tie_window is not None and K > 1:
        k0 = int(r["winner_w"][tie_window])
        other = (k0 + 1 + int(rng.integers(K - 1))) % K
        Y[tie_window, other] = Y[tie_window, k0]
        tied[tie_window] = True
    Y = np.ascontiguousarray(Y.reshape(n * K * m, T, 2))
    r = scene_f64(Y, fut, valid, d, MIN)
    plain = (r["count"] > 0) & ~tied
    if K > 1:
        assert (r["gap"][plain] >= SCENE_GAP * r["E"].min(1)[plain]).all()
        assert (r["gap"][tied & (r["count"] > 0)] == 0).all()
    if empty_window is not None:
        assert r["count"][empty_window] == 0
    return Y, fut, valid, tied


def scene_loss_and_grads(past, fut, eps, grids, gos, w_np, d, mode, tau=0.0):
    """tests/recon_reference.py's bom_loss_and_grads in the scene scope: float64 autograd of the training loss whose reconstruction term is, per
    window, the mode's reduction over the K world errors E[w, k] = the mean of e[a, k] over the window's counted agents, and L_recon = (the sum of
    count * R) / (the sum of count).  The oracle's forward (oracle.desire_torch.forward_loss) is used as it is.  past / fut in the oracle layout
    [T, A, 3].  Returns (vals, grads): vals = recon [A] (R of the agent's window), kld / ce / reg per agent, loss, L_recon, E [n, K], winner [A]
    (the window's), winner_w [n], gap [n] (second smallest - smallest E, absolute), count [n], counted [A]."""
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
    vw = v.reshape(n, 1, m)
    count = vw.sum(2)                                                        # [n, 1]
    E = (e * vw).sum(2) / torch.clamp(count, min=1.0)                        # [n, K]
    if mode == MIN:
        R = E.min(dim=1).values
    elif mode == SOFTMIN:
        R = -float(tau) * (torch.logsumexp(-E / float(tau), dim=1) - float(np.log(K)))
    else:
        R = E.mean(dim=1)
    recon = R.reshape(n, 1).expand(n, m).reshape(d.A)
    L_recon = (recon * v).sum() / n_valid                                    # = sum(count * R) / sum(count)
    loss = L_recon + (out["kld"] * v).sum() / n_valid + out["L_ioc"]
    loss.backward()
    grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(t.shape)) for k, t in w.items()}
    E_np = E.detach().numpy()
    srt = np.sort(E_np, axis=1)
    win_w = E_np.argmin(1).astype(np.int32)
    vals = {"recon": recon.detach().numpy(), "kld": out["kld"].detach().numpy(), "ce": out["ce"].detach().numpy(),
            "reg": out["reg"].detach().numpy(), "loss": float(loss.detach()), "L_recon": float(L_recon.detach()), "E": E_np,
            "winner_w": win_w, "winner": np.repeat(win_w, m).astype(np.int32), "gap": srt[:, 1] - srt[:, 0] if K > 1 else np.full(n, np.inf),
            "count": count.reshape(n).numpy().astype(np.int32), "counted": v.numpy() != 0}
    return vals, grads


__all__ = ["MEAN", "MIN", "SOFTMIN", "SCENE_GAP", "scene_f32", "scene_f64", "make_scene_case", "scene_loss_and_grads"]
