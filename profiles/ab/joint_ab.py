"""Same-process timing of the joint (scene-level) metrics (desire_joint_metrics) on the layout of tests/joint_reference.py's generator (a lattice of
slots with planted crossings, followers and coincident pairs around a 20-pixel radius; sixteen windows generated, tiled to the shape -- a result
depends on its window alone), in the evaluation form with every output and in the prediction form, against two yardsticks measured in the same
process, neither of them the code under test: (a) desire_ranked_errors with four horizons -- the parent's code, streaming the same Y once -- and
(b) a plain torch statement of the same outputs on the same device, what a user has without the call: per-frame cdist + masks + the reductions.
Hip events around N back-to-back launches each after a warm-up, three repeats, median (min - max), at the headline shape (512 windows x 32 slots,
K = 20, T_pred = 40) and at the training shape (128 windows).  Each time is stated against the streaming floor of the bytes the call moves at
6.3 TB/s.  Each shape runs in a child process under its own time limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/joint_ab.py [--launches 200] [--reps 3]
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


def torch_joint(torch, Y, fut, score, hz, top, radius, ux, uy, d):
    """The call's outputs in plain torch: (first, cnt, jerr, jscore, order, out)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    unit = torch.tensor([ux, uy], device=Y.device)
    g = (fut[..., 1:] * torch.tensor([d.sx, d.sy], device=Y.device)).permute(0, 2, 1, 3)           # [n, m, T, 2]
    c = (fut[..., 0] != 0).permute(0, 2, 1)                                                        # [n, m, T]
    Yk = Y.view(n, K, m, T, 2)
    pos = torch.cat([Yk, g[:, None]], 1) * unit                                                    # [n, K + 1, m, T, 2]
    eye = torch.eye(m, dtype=torch.bool, device=Y.device)
    first = torch.full((n, K + 1, m), T, device=Y.device, dtype=torch.int32)
    for t in range(T - 1, -1, -1):
        p = pos[:, :, :, t].reshape(n * (K + 1), m, 2)
        near = (torch.cdist(p, p, compute_mode="donot_use_mm_for_euclid_dist") < radius).view(n, K + 1, m, m)
        ok = (c[:, None, :, None, t] & c[:, None, None, :, t]) & ~eye
        first = torch.where((near & ok).any(-1), torch.full_like(first, t), first)
    part = torch.stack([c[:, :, :h].any(-1) for h in hz], 1)                                       # [n, n_h, m]
    cnt = torch.stack([torch.stack([(first < h).sum(-1) for h in hz], -1),
                       part.sum(-1)[:, None, :].expand(n, K + 1, len(hz))], -1).int()
    e = ((Yk - g[:, None]) * unit).norm(dim=-1) * c[:, None]                                       # [n, K, m, T]
    csum, ccnt = e.cumsum(-1), c.cumsum(-1)
    last = torch.cummax(torch.where(c, torch.arange(T, device=Y.device), torch.zeros((), device=Y.device, dtype=torch.long)), -1).values
    jerr = torch.zeros((n, K, len(hz), 2), device=Y.device)
    for hi, h in enumerate(hz):
        ade = csum[..., h - 1] / ccnt[:, None, :, h - 1].clamp(min=1)
        fde = torch.gather(e, 3, last[:, None, :, h - 1, None].expand(n, K, m, 1))[..., 0]
        w = part[:, None, hi].float()
        nt = part[:, hi].sum(-1).clamp(min=1)[:, None]
        jerr[:, :, hi, 0] = (ade * w).sum(-1) / nt
        jerr[:, :, hi, 1] = (fde * w).sum(-1) / nt
    jscore = (score.view(n, K, m) * c.any(-1)[:, None].float()).sum(-1)
    order = torch.sort(jscore, dim=1, descending=True, stable=True).indices.int()
    picked = torch.gather(jerr, 1, order[:, :top].long()[:, :, None, None].expand(n, top, len(hz), 2))
    out = torch.cat([picked[:, 0], picked.amin(1)], -1) * part.any(-1)[:, :, None].float()
    return first, cnt, jerr, jscore, order, out


def child(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims
    from tests.joint_reference import make_inputs
    kw = dict(mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, sx=1.0 / 1400.0, sy=1.0 / 1100.0,
              iters=1, posterior=0)
    d, d16 = Dims(n_scenes=n_windows, **kw), Dims(n_scenes=16, **kw)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    Y16, fut16, pres16, _ = make_inputs(d16, RADIUS_PX, ux, uy, seed=1)
    Y16 = np.nan_to_num(Y16, nan=0.5)
    rep = n_windows // 16
    h = _lib.Handle(d)
    g = torch.Generator(device="cuda").manual_seed(1)
    Y = torch.as_tensor(Y16, device="cuda").repeat(rep, 1, 1).contiguous()
    fut = torch.as_tensor(fut16, device="cuda").repeat(rep, 1, 1, 1).contiguous()
    pres = torch.as_tensor(pres16, device="cuda").repeat(rep).contiguous()
    score = torch.randn((d.R,), generator=g, device="cuda")
    i32, n, K, m = torch.int32, d.n_scenes, d.K, d.mno
    hz, top = [10, 20, 30, 40], 2
    order = torch.zeros((d.A, K), device="cuda", dtype=i32); out4 = torch.zeros((d.A, 4, 4), device="cuda")
    first = torch.zeros((n, K + 1, m), device="cuda", dtype=i32); cnt = torch.zeros((n, K + 1, 4, 2), device="cuda", dtype=i32)
    jerr = torch.zeros((n, K, 4, 2), device="cuda"); js = torch.zeros((n, K), device="cuda")
    jo = torch.zeros((n, K), device="cuda", dtype=i32); out = torch.zeros((n, 4, 4), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    h.rank_samples(score.data_ptr(), 0, top, order.data_ptr(), 0, 0, s)
    legs = {"ranked_errors": lambda: h.ranked_errors(Y.data_ptr(), fut.data_ptr(), order.data_ptr(), top, hz, ux, uy, out4.data_ptr(), s),
            "joint": lambda: h.joint_metrics(Y.data_ptr(), fut.data_ptr(), 0, score.data_ptr(), hz, top, RADIUS_PX, ux, uy, cnt.data_ptr(), jo.data_ptr(),
                                             first.data_ptr(), jerr.data_ptr(), js.data_ptr(), out.data_ptr(), s),
            "joint_no_errors": lambda: h.joint_metrics(Y.data_ptr(), fut.data_ptr(), 0, score.data_ptr(), hz, top, RADIUS_PX, ux, uy, cnt.data_ptr(),
                                                       jo.data_ptr(), first.data_ptr(), 0, js.data_ptr(), 0, s),
            "joint_present": lambda: h.joint_metrics(Y.data_ptr(), 0, pres.data_ptr(), score.data_ptr(), hz, top, RADIUS_PX, ux, uy, cnt.data_ptr(),
                                                     jo.data_ptr(), first.data_ptr(), 0, js.data_ptr(), 0, s)}
    r = {"windows": n_windows, "launches": launches}
    legs["joint"]()
    torch.cuda.synchronize()
    t_first, t_cnt, t_jerr, _, _, _ = torch_joint(torch, Y, fut, score, hz, top, RADIUS_PX, ux, uy, d)
    r["torch_agrees_first_cnt"] = bool(torch.equal(t_first, first)) and bool(torch.equal(t_cnt, cnt))     # (no pair of this layout sits on the radius)
    r["torch_jerr_max_diff_px"] = round(float((t_jerr - jerr).abs().max()), 6)
    r["touching_share"] = round(float(cnt[:, :K, -1, 0].sum()) / max(float(cnt[:, :K, -1, 1].sum()), 1.0), 3)
    for f in legs.values():
        for _ in range(10):
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
        torch_joint(torch, Y, fut, score, hz, top, RADIUS_PX, ux, uy, d)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    us["torch"] = ts
    for k, v in us.items():
        r[k + "_us"] = "%.1f (%.1f - %.1f)" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in us.items()}
    y_bytes, fut_bytes, tab_bytes = d.R * d.T_pred * 8, n * d.T_pred * m * 12, d.R * 4 * 8
    r["Y_MB"] = round(y_bytes / 1e6, 1)
    r["pair_tests_M"] = round(n * (K + 1) * m * (m - 1) * d.T_pred / 1e6, 1)
    # evaluation form: Y twice (the table's pass and the pair pass), the targets twice, the table written and read; without errors: Y and the targets once
    r["floor_joint_us"] = round((2 * y_bytes + 2 * fut_bytes + 2 * tab_bytes) / HBM_BYTES_PER_US, 1)
    r["floor_joint_no_errors_us"] = round((y_bytes + fut_bytes) / HBM_BYTES_PER_US, 1)
    r["joint_over_ranked_errors"] = round(med["joint"] / med["ranked_errors"], 3)
    r["joint_over_torch"] = round(med["joint"] / med["torch"], 4)
    h.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", type=int, default=0, help="run one shape (this many windows) in this process")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.launches, a.reps)), flush=True)
        return
    for n in (512, 128):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--launches", str(a.launches), "--reps", str(a.reps)],
                           cwd=ROOT, timeout=300)
        if p.returncode != 0:
            raise SystemExit("shape %d failed with exit status %d: nothing more is started" % (n, p.returncode))


if __name__ == "__main__":
    main()
