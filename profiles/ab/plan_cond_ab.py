"""Same-process timing of the conditioned plan-risk call (desire_plan_risk_cond) next to desire_plan_risk on the layout of
profiles/ab/plan_risk_ab.py (tests/plan_reference.py's generator, M = 64 plans per window around a 20-pixel radius, sixteen windows generated and
tiled), every plan replacing slot 0, sigma = 40 pixels, every frame compared, every output asked for -- against a plain torch statement of the same
conditioned outputs on the same device, what a user has without the call: plan_risk_ab's broadcast in chunks of plans, with the [n, M, K] distances,
the softmax over k and the per-plan weights in the two sums.  Hip events around N back-to-back launches each after a warm-up, three repeats, median
(min - max), at the headline shape (512 windows x 32 slots, K = 20, T_pred = 40) and at one window.  The cost of conditioning is the conditioned call
minus the plain one; its floor is the plans, the unique ego rows and the [n, M, K] tables once through memory at 6.3 TB/s.  Each shape runs in a
child process under its own time limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/plan_cond_ab.py [--launches 50] [--reps 3]
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
RADIUS_PX, SIGMA_PX = 20.0, 40.0
M_PLANS = 64
TORCH_CHUNK = 8                                    # plans per pass of the torch statement, as plan_risk_ab.py chunks


def torch_plan_cond(torch, Y, fut, score, plans, ego, hz, radius, sigma, ux, uy, d):
    """The call's outputs in plain torch: (first, clear, risk, blame, cw, dist, ess, support)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    dev = Y.device
    unit = torch.tensor([ux, uy], device=dev)
    g = (fut[..., 1:] * torch.tensor([d.sx, d.sy], device=dev)).permute(0, 2, 1, 3)                # [n, m, T, 2]
    c = (fut[..., 0] != 0).permute(0, 2, 1)                                                        # [n, m, T]
    Yk = Y.view(n, K, m, T, 2)
    pos = torch.cat([Yk, g[:, None]], 1) * unit                                                    # [n, K + 1, m, T, 2]
    js = (score.view(n, K, m) * c.any(-1)[:, None].float()).sum(-1)
    fin = torch.isfinite(js).all(1, keepdim=True)
    W = torch.where(fin, torch.softmax(js, 1), torch.full_like(js, 1.0 / K))
    p = torch.where(fin, js, torch.zeros_like(js))
    tt = torch.arange(T, device=dev, dtype=torch.int32)
    hzt = torch.tensor(hz, device=dev, dtype=torch.int32)
    slots = torch.arange(m, device=dev, dtype=torch.int32)
    inf = torch.tensor(float("inf"), device=dev)
    r2, inv = radius * radius, 1.0 / (2.0 * sigma * sigma)
    wi = torch.arange(n, device=dev)[:, None]
    out = [[] for _ in range(8)]
    for m0 in range(0, plans.shape[1], TORCH_CHUNK):
        P = plans[:, m0:m0 + TORCH_CHUNK] * unit                                                   # [n, Mc, T, 2]
        e = ego[:, m0:m0 + TORCH_CHUNK].long()
        has = (e >= 0) & (e < m)
        es = e.clamp(0, m - 1)
        rows = pos[wi, :K, es]                                                                     # [n, Mc, K, T, 2]
        cmp = has[..., None] & c[wi, es] & ~torch.isnan(P).any(-1)                                 # [n, Mc, T]
        n_c = cmp.sum(-1)
        dq = ((P[:, :, None] - rows) ** 2).sum(-1)                                                 # [n, Mc, K, T]
        D = torch.where(cmp[:, :, None], dq, torch.zeros_like(dq)).sum(-1) / n_c.clamp(min=1)[..., None]
        l = p[:, None] - D * inv
        conditioned = has & (n_c >= 1) & torch.isfinite(l).all(-1)
        cw = torch.where(conditioned[..., None], torch.softmax(l, -1), W[:, None].expand_as(l))
        support = torch.where(conditioned, (W[:, None] * torch.exp(-(D * inv))).sum(-1), torch.ones_like(n_c, dtype=torch.float32))
        diff = P[:, :, None, None] - pos[:, None]                                                  # [n, Mc, K + 1, m, T, 2]
        q = (diff * diff).sum(-1)
        ok = c[:, None, None] & (ego[:, m0:m0 + TORCH_CHUNK, None, None, None] != slots[None, None, None, :, None])
        q = torch.where(ok & ~torch.isnan(q), q, inf)
        first_slot = torch.where(q < r2, tt, torch.full_like(tt, T)).amin(-1)                      # [n, Mc, K + 1, m]
        first = first_slot.amin(-1)
        out[0].append(first)
        out[1].append(torch.stack([q[..., :h].amin((-1, -2)) for h in hz], -1))
        out[2].append(((first[:, :, :K, None] < hzt).float() * cw[..., None]).sum(2))
        out[3].append(((first_slot[:, :, :K, None, :] < hzt[None, None, None, :, None]).float() * cw[..., None, None]).sum(2))
        out[4].append(cw)
        out[5].append(D)
        out[6].append(1.0 / (cw * cw).sum(-1))
        out[7].append(support)
    return tuple(torch.cat(x, 1) for x in out)


def child(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims
    from tests.plan_cond_reference import plan_cond_geometry
    from tests.plan_reference import make_inputs
    kw = dict(mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, sx=1.0 / 1400.0, sy=1.0 / 1100.0,
              iters=1, posterior=0)
    gen = min(n_windows, 16)
    d, dg = Dims(n_scenes=n_windows, **kw), Dims(n_scenes=gen, **kw)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    Yg, futg, _, plansg, _, _ = make_inputs(dg, M_PLANS, RADIUS_PX, ux, uy, seed=1)
    Yg = np.nan_to_num(Yg, nan=0.5)
    rep = n_windows // gen
    h = _lib.Handle(d)
    gg = torch.Generator(device="cuda").manual_seed(1)
    Y = torch.as_tensor(Yg, device="cuda").repeat(rep, 1, 1).contiguous()
    fut = torch.as_tensor(futg, device="cuda").repeat(rep, 1, 1, 1).contiguous()
    plans = torch.as_tensor(plansg, device="cuda").repeat(rep, 1, 1, 1).contiguous()
    i32, n, K, m, M, T = torch.int32, d.n_scenes, d.K, d.mno, M_PLANS, d.T_pred
    ego = torch.zeros((n, M), device="cuda", dtype=i32)                    # every plan replaces slot 0
    score = torch.randn((d.R,), generator=gg, device="cuda") * 0.1
    hz = [10, 20, 30, 40]
    first = torch.zeros((n, M, K + 1), device="cuda", dtype=i32); clear = torch.zeros((n, M, K + 1, 4), device="cuda")
    risk = torch.zeros((n, M, 4), device="cuda"); blame = torch.zeros((n, M, 4, m), device="cuda")
    cw = torch.zeros((n, M, K), device="cuda"); dist = torch.zeros((n, M, K), device="cuda")
    ess = torch.zeros((n, M), device="cuda"); support = torch.zeros((n, M), device="cuda"); cond = torch.zeros((n, M), device="cuda", dtype=i32)
    s = torch.cuda.current_stream().cuda_stream
    legs = {"plan_risk_cond": lambda: h.plan_risk_cond(Y.data_ptr(), fut.data_ptr(), 0, score.data_ptr(), plans.data_ptr(), ego.data_ptr(), M, hz,
                                                       RADIUS_PX, ux, uy, SIGMA_PX, T, risk.data_ptr(), cw.data_ptr(), first.data_ptr(),
                                                       clear.data_ptr(), blame.data_ptr(), dist.data_ptr(), ess.data_ptr(), support.data_ptr(),
                                                       cond.data_ptr(), s),
            "plan_risk": lambda: h.plan_risk(Y.data_ptr(), fut.data_ptr(), 0, score.data_ptr(), plans.data_ptr(), ego.data_ptr(), M, hz, RADIUS_PX, ux, uy,
                                             risk.data_ptr(), first.data_ptr(), clear.data_ptr(), blame.data_ptr(), s)}
    r = {"windows": n_windows, "plans": M, "launches": launches}
    legs["plan_risk_cond"]()
    torch.cuda.synchronize()
    t = torch_plan_cond(torch, Y, fut, score, plans, ego, hz, RADIUS_PX, SIGMA_PX, ux, uy, d)
    r["torch_agrees_first"] = bool(torch.equal(t[0], first))               # (no plan of this layout sits on the radius)
    for name, a, b in (("risk", t[2], risk), ("blame", t[3], blame), ("cw", t[4], cw), ("ess", t[6], ess), ("support", t[7], support)):
        r["torch_%s_max_diff" % name] = float((a - b).abs().max())
    r["torch_dist_max_rel_diff"] = float(((t[5] - dist).abs() / dist.clamp(min=1e-30)).max())
    r["conditioned_plans"] = round(float((cond > 0).float().mean()), 4)
    r["mean_ess"] = round(float(ess.mean()), 3)
    r["mean_risk_given"] = [round(float(v), 4) for v in risk.mean((0, 1))]
    legs["plan_risk"]()
    torch.cuda.synchronize()
    r["mean_risk_prior"] = [round(float(v), 4) for v in risk.mean((0, 1))]
    del t
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
        torch_plan_cond(torch, Y, fut, score, plans, ego, hz, RADIUS_PX, SIGMA_PX, ux, uy, d)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    us["torch"] = ts
    for k, v in us.items():
        r[k + "_us"] = "%.1f (%.1f - %.1f)" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in us.items()}
    pc, tc, rows = plan_cond_geometry(K, T, M)
    r["plan_chunk"], r["frames_per_pass"], r["ego_rows_in_lds"], r["workgroups"] = pc, tc, rows, n * -(-M // pc)
    floor_bytes = n * M * T * 8 + n * K * T * 8 + 2 * 4 * cw.numel() + 4 * (ess.numel() + support.numel() + cond.numel())
    r["conditioning_us"] = round(med["plan_risk_cond"] - med["plan_risk"], 1)
    r["conditioning_MB"] = round(floor_bytes / 1e6, 1)
    r["floor_conditioning_us"] = round(floor_bytes / HBM_BYTES_PER_US, 1)
    r["cond_over_plain"] = round(med["plan_risk_cond"] / med["plan_risk"], 3)
    r["cond_over_torch"] = round(med["plan_risk_cond"] / med["torch"], 5)
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
