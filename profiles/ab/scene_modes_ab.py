"""Same-process timing of the scene-mode fit (desire_fit_scene_modes) on the layout of tests/scene_modes_reference.py's generator (per window 1 - 4
scene modes that diverge along every slot's own direction, a two-number jitter per world, planted world scores, 24 of 32 slots taking part; sixteen
windows generated, tiled to the shape -- a result depends on its window alone), with every output and the likelihood, and the fit alone (no
targets), against a plain torch statement of the same outputs on the same device with the same pass cap, what a user has without the call: per
pass the broadcast [n, K, modes, mno, T] of the assignment and a one-hot contraction for the update, a host read per pass to stop when no label
moved, then the covariances and the joint log-density.  Next to it desire_fit_modes on the same tensors (the per-agent fit of the same K x mno
rows).  Hip events around N back-to-back launches each after a warm-up, three repeats, median (min - max), at the headline shape (512 windows x 32
slots, K = 20, T_pred = 40, n = 6, iters = 8) and at one window.  The call's time is stated against the streaming floor of the bytes it moves at
6.3 TB/s: the taking-part rows of Y, the scores, the order and the targets once, and the outputs.  Each shape runs in a child process under its own
time limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/scene_modes_ab.py [--launches 50] [--reps 3]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_US = 6.3e6                           # 6.3 TB/s achievable
N_MODES, ITERS, MIN_STD_PX, LOG_FLOOR = 6, 8, 0.5, -20.0


def torch_scene_modes(torch, Y, part, order, wscore, fut, n, iters, ux, uy, vf, hz, d):
    """The call's outputs in plain torch: (label, count, prob, mean, cov, passes of the batch, out)."""
    N, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    dev = Y.device
    unit = torch.tensor([ux, uy], device=dev)
    Yw = Y.view(N, K, m, T, 2)
    w = torch.softmax(wscore, 1)
    w = torch.where(torch.isfinite(wscore).all(1, keepdim=True), w, torch.full_like(w, 1.0 / K))
    ar = torch.arange(N, device=dev)[:, None]
    pm = part[:, None, None, :].float()                                                            # [N, 1, 1, m]
    means = Yw[ar, order[:, :n].long()]                                                            # [N, n, m, T, 2]

    def assign(mu):
        diff = (Yw[:, :, None] - mu[:, None]) * unit                                               # [N, K, n, m, T, 2]
        return ((diff * diff).sum((-1, -2)) * pm).sum(-1).argmin(-1)

    def update(label, mu):
        oh = torch.nn.functional.one_hot(label, n).float() * w[..., None]                          # [N, K, n]
        W = oh.sum(1)
        num = torch.einsum("wki,wkmtc->wimtc", oh, Yw)
        return torch.where((W > 0)[..., None, None, None], num / W.clamp(min=1e-38)[..., None, None, None], mu), W, oh

    label = assign(means)
    p = 0
    while True:
        means, W, oh = update(label, means)
        if p == iters:
            break
        p += 1
        new = assign(means)
        same = bool(torch.equal(new, label))                                                       # the host read of a data-dependent stop
        label = new
        if same:
            break
    c = (Yw[:, :, None] - means[:, None]) * unit                                                   # [N, K, n, m, T, 2]
    Wd = W.clamp(min=1e-38)[..., None, None]
    has = (W > 0)[..., None, None]
    zero = torch.zeros((), device=dev)
    cxx = torch.where(has, torch.einsum("wki,wkimt->wimt", oh, c[..., 0] * c[..., 0]) / Wd + vf, zero)
    cyy = torch.where(has, torch.einsum("wki,wkimt->wimt", oh, c[..., 1] * c[..., 1]) / Wd + vf, zero)
    cxy = torch.where(has, torch.einsum("wki,wkimt->wimt", oh, c[..., 0] * c[..., 1]) / Wd, zero)
    pt = part[:, None, :, None]
    means_o = torch.where(pt[..., None], means, torch.zeros_like(means))
    cov = torch.where(pt[..., None], torch.stack([cxx, cyy, cxy], -1), torch.zeros((), device=dev))
    count = torch.nn.functional.one_hot(label, n).sum(1).int()
    counted = (fut[..., 0] != 0).permute(0, 2, 1) & part[:, :, None]                               # [N, m, T]
    ct = counted.sum(1)                                                                            # [N, T]
    g = (fut[..., 1:] * torch.tensor([d.sx, d.sy], device=dev)).permute(0, 2, 1, 3)[:, None]       # [N, 1, m, T, 2]
    dd = (means - g) * unit
    det = cxx * cyy - cxy * cxy
    good = det > 1e-5 * cxx * cyy
    term = (-0.5 * (cyy * dd[..., 0] ** 2 - 2 * cxy * dd[..., 0] * dd[..., 1] + cxx * dd[..., 1] ** 2)) / det - 1.8378770664093453 - 0.5 * torch.log(det)
    cn = counted[:, None]
    li = torch.log(W)[..., None] + torch.where(cn & good, term, torch.zeros_like(term)).sum(2)     # [N, n, T]
    ok = (W > 0)[..., None] & (good | ~cn).all(2)
    li = torch.where(ok, li, torch.full_like(li, float("-inf")))
    l = torch.logsumexp(li, 1) / ct.clamp(min=1)
    frame = torch.where(ct > 0, torch.where(l > LOG_FLOOR, l, torch.full_like(l, LOG_FLOOR)), torch.zeros_like(l))
    out = []
    tt = torch.arange(1, T + 1, device=dev)
    for x in hz:
        cx = ct[:, :x] > 0
        np_ = cx.sum(1)
        last = (cx * tt[:x]).argmax(1)
        mean_ = -(frame[:, :x].sum(1) / np_.clamp(min=1))
        fin = -frame[ar[:, 0], last]
        z = torch.zeros_like(mean_)
        out.append(torch.stack([torch.where(np_ > 0, mean_, z), torch.where(np_ > 0, fin, z)], -1))
    return label.int(), count, W, means_o, cov, p, torch.stack(out, 1)


def child(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims
    from tests.joint_reference import _rank
    from tests.scene_modes_reference import make_inputs, scene_modes_geometry
    kw = dict(mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, sx=1.0 / 1400.0, sy=1.0 / 1100.0,
              iters=1, posterior=0)
    gen = min(n_windows, 16)
    d, dg = Dims(n_scenes=n_windows, **kw), Dims(n_scenes=gen, **kw)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    vf = MIN_STD_PX ** 2
    n, T, K, m, N = N_MODES, d.T_pred, d.K, d.mno, d.n_scenes
    Yg, presg, _, wsg, futg, info = make_inputs(dg, n, T, ux, uy, seed=1)
    # the layout alone: no NaN row, no non-finite score, no BAD order row, and the window with nobody taking part is window 0 once more
    Yg = np.nan_to_num(Yg, nan=0.5).reshape(gen, K * m, T, 2)
    wsg = np.nan_to_num(wsg, nan=0.0, posinf=0.0)
    presg = np.array(presg).reshape(gen, m)
    futg = np.array(futg)
    if info["empty"] >= 0:
        e = info["empty"]
        Yg[e], presg[e], futg[e], wsg[e] = Yg[0], presg[0], futg[0], wsg[0]
    og = _rank(wsg)
    assert (presg.sum(1) == 24).all()
    rep = n_windows // gen
    h = _lib.Handle(d)
    Y = torch.as_tensor(Yg, device="cuda").repeat(rep, 1, 1, 1).reshape(d.R, T, 2).contiguous()
    pres = torch.as_tensor(presg, device="cuda").repeat(rep, 1).contiguous()
    order = torch.as_tensor(og, device="cuda").repeat(rep, 1).contiguous()
    ws = torch.as_tensor(wsg, device="cuda").repeat(rep, 1).contiguous()
    fut = torch.as_tensor(futg, device="cuda").repeat(rep, 1, 1, 1).contiguous()
    i32 = torch.int32
    hz = [10, 20, 30, 40]
    label = torch.zeros((N, K), device="cuda", dtype=i32); count = torch.zeros((N, n), device="cuda", dtype=i32)
    prob = torch.zeros((N, n), device="cuda"); mean = torch.zeros((N, n, m, T, 2), device="cuda"); cov = torch.zeros((N, n, m, T, 3), device="cuda")
    passes = torch.zeros((N,), device="cuda", dtype=i32); out = torch.zeros((N, 4, 2), device="cuda"); frame = torch.zeros((N, T), device="cuda")
    # desire_fit_modes on the same tensors: every agent seeded by its window's order, weighted by its window's scores
    a_order = order[:, None, :].expand(N, m, K).reshape(d.A, K).contiguous()
    a_score = ws[:, :, None].expand(N, K, m).contiguous()
    a_label = torch.zeros((d.A, K), device="cuda", dtype=i32); a_count = torch.zeros((d.A, n), device="cuda", dtype=i32)
    a_prob = torch.zeros((d.A, n), device="cuda"); a_mean = torch.zeros((d.A, n, T, 2), device="cuda"); a_cov = torch.zeros((d.A, n, T, 3), device="cuda")
    a_passes = torch.zeros((d.A,), device="cuda", dtype=i32); a_out = torch.zeros((d.A, 4, 2), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    legs = {"fit_scene_modes": lambda: h.fit_scene_modes(Y.data_ptr(), pres.data_ptr(), order.data_ptr(), ws.data_ptr(), n, T, ITERS, ux, uy, vf,
                                                         count.data_ptr(), prob.data_ptr(), label.data_ptr(), mean.data_ptr(), cov.data_ptr(),
                                                         passes.data_ptr(), fut.data_ptr(), hz, LOG_FLOOR, out.data_ptr(), frame.data_ptr(), s),
            "fit_scene_modes_fit_only": lambda: h.fit_scene_modes(Y.data_ptr(), pres.data_ptr(), order.data_ptr(), ws.data_ptr(), n, T, ITERS, ux, uy, vf,
                                                                  count.data_ptr(), prob.data_ptr(), label.data_ptr(), mean.data_ptr(), cov.data_ptr(),
                                                                  passes.data_ptr(), stream=s),
            "fit_modes": lambda: h.fit_modes(Y.data_ptr(), a_order.data_ptr(), a_score.data_ptr(), n, T, ITERS, ux, uy, vf, a_count.data_ptr(),
                                             a_prob.data_ptr(), a_label.data_ptr(), a_mean.data_ptr(), a_cov.data_ptr(), a_passes.data_ptr(), fut.data_ptr(),
                                             hz, LOG_FLOOR, a_out.data_ptr(), 0, s)}
    r = {"windows": n_windows, "modes": n, "iters": ITERS, "launches": launches}
    legs["fit_scene_modes"]()
    torch.cuda.synchronize()
    part = pres != 0
    t_label, t_count, t_prob, t_mean, t_cov, t_passes, t_out = torch_scene_modes(torch, Y, part, order, ws, fut, n, ITERS, ux, uy, vf, hz, d)
    r["torch_label_agreement"] = float((t_label == label).float().mean())
    r["torch_prob_max_diff"] = float((t_prob - prob).abs().max())
    r["torch_mean_max_diff"] = float((t_mean - mean).abs().max())
    r["torch_cov_max_rel_diff"] = float(((t_cov - cov).abs() / cov.abs().clamp(min=1.0)).max())
    r["torch_out_max_diff"] = float((t_out - out).abs().max())
    r["passes_hist"] = torch.bincount(passes.long()).tolist()
    r["torch_passes"] = t_passes
    del t_label, t_count, t_prob, t_mean, t_cov, t_out
    for f in legs.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(reps):                          # interleaved
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1000.0 / launches)
    ts = []
    for _ in range(reps):                          # the torch statement: the whole thing, a few times (it is milliseconds)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_scene_modes(torch, Y, part, order, ws, fut, n, ITERS, ux, uy, vf, hz, d)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    us["torch"] = ts
    for k, v in us.items():
        r[k + "_us"] = "%.1f (%.1f - %.1f)" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in us.items()}
    sc = scene_modes_geometry(m, K, T, n)
    in_bytes = int(part.sum()) * K * T * 8 + ws.numel() * 4 + order.numel() * 4 + pres.numel() + fut.numel() * 4
    out_bytes = 4 * (label.numel() + count.numel() + prob.numel() + mean.numel() + cov.numel() + passes.numel() + out.numel() + frame.numel())
    r["slot_chunk"], r["workgroups"] = sc, N
    r["in_MB"], r["out_MB"] = round(in_bytes / 1e6, 2), round(out_bytes / 1e6, 2)
    r["floor_us"] = round((in_bytes + out_bytes) / HBM_BYTES_PER_US, 1)
    r["fit_scene_modes_over_floor"] = round(med["fit_scene_modes"] / max(r["floor_us"], 1e-9), 2)
    r["fit_scene_modes_over_torch"] = round(med["fit_scene_modes"] / med["torch"], 5)
    r["fit_scene_modes_over_fit_modes"] = round(med["fit_scene_modes"] / med["fit_modes"], 3)
    h.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", type=int, default=0, help="run one shape (this many windows) in this process")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.launches, a.reps)), flush=True)
        return
    for n in (512, 1):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--launches", str(a.launches), "--reps", str(a.reps)],
                           cwd=ROOT, timeout=300)
        if p.returncode != 0:
            raise SystemExit("shape %d failed with exit status %d: nothing more is started" % (n, p.returncode))


if __name__ == "__main__":
    main()
