"""Same-process timing of the plan-risk call (desire_plan_risk) on the layout of tests/plan_reference.py's generator (joint_reference's lattice of
slots with M = 64 candidate plans per window cycling through crossing, following, coincident, replaced, far, NaN and left-slot plans around a
20-pixel radius; sixteen windows generated, tiled to the shape -- a result depends on its window alone), in the evaluation form with every output
and in the prediction form with the risk alone, against a plain torch statement of the same outputs on the same device, what a user has without
the call: the broadcast [n, Mc, K + 1, mno, T] in chunks of Mc plans, masks and the reductions.  Hip events around N back-to-back launches each
after a warm-up, three repeats, median (min - max), at the headline shape (512 windows x 32 slots, K = 20, T_pred = 40) and at one window.  The
call's time is stated against the streaming floor of the bytes it moves at 6.3 TB/s: Y once per plan chunk, the plans and the outputs.  Each shape
runs in a child process under its own time limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/plan_risk_ab.py [--launches 50] [--reps 3]
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
RADIUS_PX = 20.0
M_PLANS = 64
TORCH_CHUNK = 8                                    # plans per pass of the torch statement: 0.44 GB per intermediate at the headline shape


def torch_plan(torch, Y, fut, score, plans, ego, hz, radius, ux, uy, d):
    """The call's outputs in plain torch: (first, clear, risk, blame)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    dev = Y.device
    unit = torch.tensor([ux, uy], device=dev)
    g = (fut[..., 1:] * torch.tensor([d.sx, d.sy], device=dev)).permute(0, 2, 1, 3)                # [n, m, T, 2]
    c = (fut[..., 0] != 0).permute(0, 2, 1)                                                        # [n, m, T]
    pos = torch.cat([Y.view(n, K, m, T, 2), g[:, None]], 1) * unit                                 # [n, K + 1, m, T, 2]
    js = (score.view(n, K, m) * c.any(-1)[:, None].float()).sum(-1)
    W = torch.softmax(js, 1)
    W = torch.where(torch.isfinite(js).all(1, keepdim=True), W, torch.full_like(W, 1.0 / K))
    tt = torch.arange(T, device=dev, dtype=torch.int32)
    hzt = torch.tensor(hz, device=dev, dtype=torch.int32)
    slots = torch.arange(m, device=dev, dtype=torch.int32)
    inf = torch.tensor(float("inf"), device=dev)
    r2 = radius * radius
    out = [[], [], [], []]
    for m0 in range(0, plans.shape[1], TORCH_CHUNK):
        P = plans[:, m0:m0 + TORCH_CHUNK] * unit                                                   # [n, Mc, T, 2]
        diff = P[:, :, None, None] - pos[:, None]                                                  # [n, Mc, K + 1, m, T, 2]
        q = (diff * diff).sum(-1)
        ok = c[:, None, None] & (ego[:, m0:m0 + TORCH_CHUNK, None, None, None] != slots[None, None, None, :, None])
        q = torch.where(ok & ~torch.isnan(q), q, inf)
        first_slot = torch.where(q < r2, tt, torch.full_like(tt, T)).amin(-1)                      # [n, Mc, K + 1, m]
        first = first_slot.amin(-1)
        out[0].append(first)
        out[1].append(torch.stack([q[..., :h].amin((-1, -2)) for h in hz], -1))
        out[2].append(((first[:, :, :K, None] < hzt).float() * W[:, None, :, None]).sum(2))
        out[3].append(((first_slot[:, :, :K, None, :] < hzt[None, None, None, :, None]).float() * W[:, None, :, None, None]).sum(2))
    return tuple(torch.cat(x, 1) for x in out)


def child(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims
    from tests.plan_reference import make_inputs, plan_geometry
    kw = dict(mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, sx=1.0 / 1400.0, sy=1.0 / 1100.0,
              iters=1, posterior=0)
    gen = min(n_windows, 16)
    d, dg = Dims(n_scenes=n_windows, **kw), Dims(n_scenes=gen, **kw)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    Yg, futg, presg, plansg, egog, _ = make_inputs(dg, M_PLANS, RADIUS_PX, ux, uy, seed=1)
    Yg = np.nan_to_num(Yg, nan=0.5)
    rep = n_windows // gen
    h = _lib.Handle(d)
    gg = torch.Generator(device="cuda").manual_seed(1)
    Y = torch.as_tensor(Yg, device="cuda").repeat(rep, 1, 1).contiguous()
    fut = torch.as_tensor(futg, device="cuda").repeat(rep, 1, 1, 1).contiguous()
    pres = torch.as_tensor(presg, device="cuda").repeat(rep).contiguous()
    plans = torch.as_tensor(plansg, device="cuda").repeat(rep, 1, 1, 1).contiguous()
    ego = torch.as_tensor(egog, device="cuda").repeat(rep, 1).contiguous()
    score = torch.randn((d.R,), generator=gg, device="cuda") * 0.1
    i32, n, K, m, M = torch.int32, d.n_scenes, d.K, d.mno, M_PLANS
    hz = [10, 20, 30, 40]
    first = torch.zeros((n, M, K + 1), device="cuda", dtype=i32); clear = torch.zeros((n, M, K + 1, 4), device="cuda")
    risk = torch.zeros((n, M, 4), device="cuda"); blame = torch.zeros((n, M, 4, m), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    legs = {"plan_risk": lambda: h.plan_risk(Y.data_ptr(), fut.data_ptr(), 0, score.data_ptr(), plans.data_ptr(), ego.data_ptr(), M, hz, RADIUS_PX, ux, uy,
                                             risk.data_ptr(), first.data_ptr(), clear.data_ptr(), blame.data_ptr(), s),
            "plan_risk_present_risk_only": lambda: h.plan_risk(Y.data_ptr(), 0, pres.data_ptr(), score.data_ptr(), plans.data_ptr(), ego.data_ptr(), M, hz,
                                                               RADIUS_PX, ux, uy, risk.data_ptr(), 0, 0, 0, s)}
    r = {"windows": n_windows, "plans": M, "launches": launches}
    legs["plan_risk"]()
    torch.cuda.synchronize()
    t_first, t_clear, t_risk, t_blame = torch_plan(torch, Y, fut, score, plans, ego, hz, RADIUS_PX, ux, uy, d)
    r["torch_agrees_first"] = bool(torch.equal(t_first, first))            # (no plan of this layout sits on the radius)
    r["torch_risk_max_diff"] = float((t_risk - risk).abs().max())
    r["torch_blame_max_diff"] = float((t_blame - blame).abs().max())
    fin = torch.isfinite(clear)
    r["torch_clear_max_rel_diff"] = float(((t_clear - clear).abs() / clear.clamp(min=1e-30))[fin].max()) if bool(fin.any()) else 0.0
    r["mean_risk"] = [round(float(v), 4) for v in risk.mean((0, 1))]
    del t_first, t_clear, t_risk, t_blame
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
        torch_plan(torch, Y, fut, score, plans, ego, hz, RADIUS_PX, ux, uy, d)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    us["torch"] = ts
    for k, v in us.items():
        r[k + "_us"] = "%.1f (%.1f - %.1f)" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in us.items()}
    pc, tc = plan_geometry(m, d.T_pred, M)
    chunks = -(-M // pc)
    y_bytes, plan_bytes = d.R * d.T_pred * 8, n * M * d.T_pred * 8
    out_bytes = 4 * (first.numel() + clear.numel() + risk.numel() + blame.numel())
    r["plan_chunk"], r["frames_per_pass"], r["workgroups"] = pc, tc, n * chunks
    r["Y_MB"], r["out_MB"] = round(y_bytes / 1e6, 1), round(out_bytes / 1e6, 1)
    r["pair_frames_M"] = round(n * M * (K + 1) * m * d.T_pred / 1e6, 1)
    r["floor_plan_risk_us"] = round((chunks * y_bytes + plan_bytes + out_bytes) / HBM_BYTES_PER_US, 1)
    r["floor_risk_only_us"] = round((chunks * y_bytes + plan_bytes + 4 * risk.numel()) / HBM_BYTES_PER_US, 1)
    r["plan_risk_over_floor"] = round(med["plan_risk"] / max(r["floor_plan_risk_us"], 1e-9), 2)
    r["pair_frames_per_us"] = round(n * M * (K + 1) * m * d.T_pred / med["plan_risk"], 1)
    r["plan_risk_over_torch"] = round(med["plan_risk"] / med["torch"], 5)
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
