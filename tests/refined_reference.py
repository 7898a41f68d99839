"""Float64 autograd of the training loss with the terms of desire_set_refined_loss (include/desire_hip.h): the recon mode,
the collision hinge and the off-road field on the REFINED trajectories Y next to their twins on Y0.  The forward is the oracle's
(oracle.desire_torch.forward_loss, used as it is): its out["Y"] carries the gradient of the refinement and is built on the detached Y0, so a
term on Y reaches ioc/* and, through Hx, enc_x/* -- nothing else.  The three terms are written once, as functions of any [n, K, mno, T, 2]
trajectory tensor, with the statements of tests/recon_reference.py / tests/recon_scene_reference.py (min, soft-min, the scene scope),
tests/collision_reference.py (the hinge, sqrt(q + 1e-300) for the root) and tests/offroad_reference.py (the clamped bilinear read-out, the fp32
brute-force field, masks_from_positions); radius, masks and weights come from the float64 oracle alone, never from a device."""
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from tests.collision_reference import AGENT, MEAN, MIN, SCENE, SOFTMIN  # noqa: F401
from tests.offroad_reference import cell_sizes, mask_field_f32, masks_from_positions


@dataclass(frozen=True)
class Spec:
    """What is on.  A weight / radius of None with its switch on is chosen from the oracle (refined_loss_and_grads); the resolved Spec comes back
    in vals["spec"] and pins every choice (finite differences, a second forward)."""
    mode: int = MEAN
    tau: float = 0.0
    scope: int = AGENT
    recon: bool = False                 # the regression term follows mode / tau / scope, with weights from the refined errors
    rcol: bool = False                  # collision term on Y
    roff: bool = False                  # off-road term on Y
    col: bool = False                   # collision term on Y0
    off: bool = False                   # off-road term on Y0
    radius: Optional[float] = None      # pixels: one radius, one field and one scale per handle, shared by both sides
    quantile: float = 0.25              # the radius is the distance below which this share of the counted (pair, frame)s of Y fall
    Mh: int = 16
    Mw: int = 16
    scale: float = 120.0                # pixels
    masks: Optional[np.ndarray] = None  # [n, Mh, Mw] uint8 (None: tests/offroad_reference.masks_from_positions on Y)
    rcw: Optional[float] = None
    row: Optional[float] = None
    cw: Optional[float] = None
    ow: Optional[float] = None

    def any_on(self):
        return self.mode != MEAN or self.rcol or self.roff or self.col or self.off


def _masks(past, fut, d):
    import torch
    from oracle import desire_torch as OT
    n, m, T = d.n_scenes, d.mno, d.T_pred
    pres = torch.as_tensor(np.asarray(fut)[:, :, 0] != 0)
    pm = pres.T.reshape(n, 1, m, T).to(OT.DT)
    nf = pres.sum(0).to(OT.DT)
    nfc = torch.clamp(nf, min=1.0)
    valid = torch.as_tensor(np.asarray(past)[d.T_obs - 1, :, 0] != 0)
    v = (valid & (nf > 0)).to(OT.DT)
    gt = torch.as_tensor(OT.O.normalise(fut, d, np.float64), dtype=OT.DT).permute(1, 0, 2).reshape(n, 1, m, T, 2)
    return dict(pm=pm, nfc=nfc, v=v, n_valid=torch.clamp(v.sum(), min=1.0), gt=gt, cc=pm * v.reshape(n, 1, m, 1))


def recon_term(Yt, M, d, mode, tau, scope):
    """(term [A], e [n, K, m], E [n, K] or None): the reconstruction term of every agent on the trajectories Yt [n, K, m, T, 2] -- the mean over K,
    the min / soft-min over K per agent, or in the scene scope the window's min / soft-min over its K worlds on every slot of the window."""
    import torch
    n, K, m = d.n_scenes, d.K, d.mno
    e0 = torch.sqrt(((Yt - M["gt"]) ** 2).sum(-1) + 1e-300)
    e = (e0 * M["pm"]).sum(3) / M["nfc"].reshape(n, 1, m)                     # [n, K, m]
    E = None
    if scope == SCENE and mode != MEAN:
        vw = M["v"].reshape(n, 1, m)
        E = (e * vw).sum(2) / torch.clamp(vw.sum(2), min=1.0)
        R = E.min(dim=1).values if mode == MIN else -float(tau) * (torch.logsumexp(-E / float(tau), dim=1) - float(np.log(K)))
        term = R.reshape(n, 1).expand(n, m).reshape(d.A)
    elif mode == MIN:
        term = e.min(dim=1).values.reshape(d.A)
    elif mode == SOFTMIN:
        term = (-float(tau) * (torch.logsumexp(-e / float(tau), dim=1) - float(np.log(K)))).reshape(d.A)
    else:
        term = e.mean(dim=1).reshape(d.A)
    return term, e, E


def pair_distances(Yt, M, d):
    """(dist [n, K, i, j, T] in pixels, pair [n, 1, i, j, T]: the counted ordered pairs)."""
    import torch
    from oracle import desire_torch as OT
    m = d.mno
    fx, fy = float(np.float32(1.0 / d.sx)), float(np.float32(1.0 / d.sy))
    cc = M["cc"]
    pair = cc.unsqueeze(3) * cc.unsqueeze(2) * (1.0 - torch.eye(m, dtype=OT.DT)).reshape(1, 1, m, m, 1)
    a = (Yt[..., 0].unsqueeze(3) - Yt[..., 0].unsqueeze(2)) * fx
    b = (Yt[..., 1].unsqueeze(3) - Yt[..., 1].unsqueeze(2)) * fy
    return torch.sqrt(a * a + b * b + 1e-300), pair


def collision_term(Yt, M, d, radius):
    """L_col of Yt at `radius` pixels: the squared hinge of every counted pair, over nfut, the mean over K, the mean over the counted agents."""
    import torch
    n, m = d.n_scenes, d.mno
    dist, pair = pair_distances(Yt, M, d)
    hinge = torch.clamp(1.0 - dist / float(np.float32(radius)), min=0.0) ** 2 * pair
    col = hinge.sum((3, 4)) / M["nfc"].reshape(n, 1, m)
    return (col.mean(1) * M["v"].reshape(n, m)).sum() / M["n_valid"]


def offroad_term(Yt, M, d, field, scale):
    """(L_off, phi [n, K, m, T]) of Yt against field [n, Mh, Mw] (fp32 values, window w reads field w) at `scale` pixels."""
    import torch
    from oracle import desire_torch as OT
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Mh, Mw = field.shape[1:]
    Dt = torch.as_tensor(field.astype(np.float64))
    widx = torch.arange(n).reshape(n, 1, 1, 1).expand(n, K, m, T)
    u = Yt[..., 0] * float(Mw) - 0.5
    vv = Yt[..., 1] * float(Mh) - 0.5
    uc, vc = torch.clamp(u, 0.0, float(Mw - 1)), torch.clamp(vv, 0.0, float(Mh - 1))
    x0, y0 = torch.floor(uc.detach()).long(), torch.floor(vc.detach()).long()
    x1, y1 = torch.clamp(x0 + 1, max=Mw - 1), torch.clamp(y0 + 1, max=Mh - 1)
    fx_, fy_ = uc - x0.to(OT.DT), vc - y0.to(OT.DT)
    D00, D01, D10, D11 = Dt[widx, y0, x0], Dt[widx, y0, x1], Dt[widx, y1, x0], Dt[widx, y1, x1]
    top, bot = D00 + fx_ * (D01 - D00), D10 + fx_ * (D11 - D10)
    dd = top + fy_ * (bot - top)
    phi = (dd / float(np.float32(scale))) ** 2 * M["cc"]
    off = phi.sum(3) / M["nfc"].reshape(n, 1, m)
    return (off.mean(1) * M["v"].reshape(n, m)).sum() / M["n_valid"], phi


def cell_margin(Ynp, counted, d, Mh, Mw):
    """Cells between the counted positions of Ynp [n, K, m, T, 2] and the nearest cell line or centre line of an Mh x Mw mask."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    sel = np.broadcast_to(counted[:, None], (n, K, m, T))
    z = np.stack([2 * Ynp[..., 0] * Mw, 2 * Ynp[..., 1] * Mh], -1)
    return float((np.abs(z - np.rint(z)).min(-1) / 2)[sel].min()) if sel.any() else float("inf")


def refined_forward(past, fut, eps, grids, gos, w, d, spec, fixed=None):
    """The loss under `spec` on leaf weights w: a dict of torch values (loss, base = the loss without the four penalties, the penalties, Y, Y0, the
    masks M, the per-agent regression term `reg`).  past / fut in the oracle layout [T, A, 3].  With everything off `loss` is forward_loss' own
    expression.  A penalty that is on needs its radius / masks resolved (refined_loss_and_grads does that)."""
    from oracle import desire_torch as OT
    out = OT.forward_loss(past, fut, eps, grids, gos, w, d, fixed=fixed)
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    M = _masks(past, fut, d)
    Y0, Y = out["Y0"].reshape(n, K, m, T, 2), out["Y"].reshape(n, K, m, T, 2)
    v, n_valid = M["v"], M["n_valid"]
    L_sgm, L_ioc, reg, e1, E1 = out["L_sgm"], out["L_ioc"], out["reg"], None, None
    if spec.mode != MEAN:
        recon, _, _ = recon_term(Y0, M, d, spec.mode, spec.tau, spec.scope)
        L_sgm = ((recon + out["kld"]) * v).sum() / n_valid
        if spec.recon:
            reg, e1, E1 = recon_term(Y, M, d, spec.mode, spec.tau, spec.scope)
            L_ioc = ((out["ce"] + reg) * v).sum() / n_valid
    res = dict(out=out, M=M, Y0=Y0, Y=Y, reg=reg, e1=e1, E1=E1, base=L_sgm + L_ioc)
    loss = res["base"]
    field = None
    if spec.off or spec.roff:
        field = mask_field_f32(spec.masks, *cell_sizes(d, spec.Mh, spec.Mw))
    for key, on, Yt, wt in (("L_col_Y0", spec.col, Y0, spec.cw), ("L_col_Y", spec.rcol, Y, spec.rcw)):
        if on:
            res[key] = collision_term(Yt, M, d, spec.radius)
            if wt is not None:
                loss = loss + float(np.float32(wt)) * res[key]
    for key, on, Yt, wt in (("L_off_Y0", spec.off, Y0, spec.ow), ("L_off_Y", spec.roff, Y, spec.row)):
        if on:
            res[key], res[key + "_phi"] = offroad_term(Yt, M, d, field, spec.scale)
            if wt is not None:
                loss = loss + float(np.float32(wt)) * res[key]
    res.update(loss=loss, field=field)
    return res


def refined_loss_and_grads(past, fut, eps, grids, gos, w_np, d, spec=Spec()):
    """(vals, grads) of the loss under `spec`, choosing what spec leaves open from the float64 forward alone: the radius (rounded to fp32) is the
    spec.quantile of the counted pair distances of Y; the masks are masks_from_positions on Y; a refined weight (rounded to fp32) makes its term's
    gradient on ioc/reg/w as long as the rest of the loss's there, a Y0 weight does the same on head/w.  vals: spec (resolved), loss, Y / Y0 [R, T,
    2], counted [A], reg [A] (the per-agent regression term that is trained), kld / ce per agent, L_col_Y / L_off_Y / L_col_Y0 / L_off_Y0,
    share_rcol / share_roff (|weight d L / d ioc/reg/w| over |d loss / d ioc/reg/w|), touching (ordered counted (pair, frame, k) of Y inside the
    radius), hinge_gap (the smallest |dist / radius - 1| of a counted pair of Y and, with col, of Y0), margin (cells, cell_margin of Y and, with
    off, of Y0), positive (share of the counted positions of Y with phi > 0), winner / win_gap with recon in MIN (the argmin of the refined
    errors per agent [A] or per window [n], and the smallest relative lead of a counted winner over its runner-up)."""
    import torch
    from oracle import desire_torch as OT
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    w = OT.leaf_weights(w_np)
    if not spec.any_on():
        res = refined_forward(past, fut, eps, grids, gos, w, d, spec)
    else:
        with torch.no_grad():
            probe = OT.forward_loss(past, fut, eps, grids, gos, w, d)
        M = _masks(past, fut, d)
        Yp = probe["Y"].reshape(n, K, m, T, 2)
        counted = (M["cc"].reshape(n, m, T) > 0).numpy()
        if (spec.rcol or spec.col) and spec.radius is None:
            dist, pair = pair_distances(Yp, M, d)
            spec = replace(spec, radius=float(np.float32(np.quantile(np.unique(dist[(pair > 0).expand_as(dist)].numpy()), spec.quantile, method="midpoint"))))
        if (spec.roff or spec.off) and spec.masks is None:
            spec = replace(spec, masks=masks_from_positions(Yp.numpy(), counted, d, spec.Mh, spec.Mw))
        res = refined_forward(past, fut, eps, grids, gos, w, d, spec)
        loss = res["loss"]                                                    # (the terms with a given weight are in it already)
        for key, on, name, leaf in (("L_col_Y0", spec.col, "cw", "head/w"), ("L_off_Y0", spec.off, "ow", "head/w"),
                                    ("L_col_Y", spec.rcol, "rcw", "ioc/reg/w"), ("L_off_Y", spec.roff, "row", "ioc/reg/w")):
            if on and getattr(spec, name) is None:
                g_t = torch.autograd.grad(res[key], w[leaf], retain_graph=True)[0]
                g_b = torch.autograd.grad(res["base"], w[leaf], retain_graph=True)[0]
                wt = float(np.float32(float(g_b.norm()) / float(g_t.norm())))
                spec = replace(spec, **{name: wt})
                loss = loss + wt * res[key]
        res["loss"] = loss
    share = {}
    for key, on, name in (("L_col_Y", spec.rcol, "rcw"), ("L_off_Y", spec.roff, "row")):
        if on:
            share[name] = float(np.float32(getattr(spec, name))) * float(torch.autograd.grad(res[key], w["ioc/reg/w"], retain_graph=True)[0].norm())
    res["loss"].backward()
    grads = {k: (t.grad.numpy() if t.grad is not None else np.zeros(t.shape)) for k, t in w.items()}
    out, M = res["out"], res["M"]
    counted = (M["cc"].reshape(n, m, T) > 0).numpy()
    Yn, Y0n = res["Y"].detach().numpy(), res["Y0"].detach().numpy()
    vals = {"spec": spec, "loss": float(res["loss"].detach()), "Y": Yn.reshape(n * K * m, T, 2), "Y0": Y0n.reshape(n * K * m, T, 2),
            "counted": M["v"].numpy() != 0, "reg": res["reg"].detach().numpy(), "kld": out["kld"].detach().numpy(), "ce": out["ce"].detach().numpy(),
            "field": res["field"]}
    for key in ("L_col_Y", "L_off_Y", "L_col_Y0", "L_off_Y0"):
        if key in res:
            vals[key] = float(res[key].detach())
    total = float(np.linalg.norm(grads["ioc/reg/w"]))
    for name, s in share.items():
        vals[{"rcw": "share_rcol", "row": "share_roff"}[name]] = s / total
    if spec.rcol or spec.col:
        gaps = []
        for side, Yt in [("Y", res["Y"].detach())] + ([("Y0", res["Y0"].detach())] if spec.col else []):
            dist, pair = pair_distances(Yt, M, d)
            on = (pair > 0).expand_as(dist)
            gaps.append(float((dist[on] / spec.radius - 1.0).abs().min()))
            if side == "Y":
                vals["touching"] = int(((dist < spec.radius) & on).sum())
        vals["hinge_gap"] = min(gaps)
    if spec.roff or spec.off:
        vals["margin"] = min([cell_margin(Yn, counted, d, spec.Mh, spec.Mw)] + ([cell_margin(Y0n, counted, d, spec.Mh, spec.Mw)] if spec.off else []))
        if spec.roff:
            sel = np.broadcast_to(counted[:, None], (n, K, m, T))
            vals["positive"] = float((res["L_off_Y_phi"].detach().numpy()[sel] > 0).mean())
    if spec.recon and spec.mode == MIN:
        if spec.scope == SCENE:
            E = res["E1"].detach().numpy()                                    # [n, K]
            keep = counted.any((1, 2))
        else:
            E = res["e1"].detach().numpy().transpose(0, 2, 1).reshape(n * m, K)
            keep = vals["counted"]
        srt = np.sort(E, 1)[keep]
        vals["winner"] = E.argmin(1).astype(np.int32)
        vals["win_keep"] = keep
        vals["win_gap"] = float(((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min()) if K > 1 and keep.any() else float("inf")
    return vals, grads
