"""Same-process timing of the selection of distinct joint futures (desire_select_worlds) on the layout of tests/worlds_reference.py's generator
(scene modes 4 radii apart, worlds = a mode plus jitter, a chain, absent slots; sixteen windows generated, the empty one and the NaN row replaced,
tiled to the shape -- a result depends on its window alone), in two layouts -- 2 modes per window (about 3 worlds kept) and 11 (about 12) --, all
three metrics and both reduces, against two yardsticks measured in the same process, neither of them the code under test: (a)
desire_joint_metrics in its prediction form on the same tensors -- the parent's code, one pass over Y -- and (b) a plain torch statement of the
same outputs on the same device, what a user has without the call: chunked pairwise world distances, then the K-step greedy loop over all
windows at once.  Hip events around N back-to-back launches each after a warm-up, three repeats, median (min - max), at the headline shape (512
windows x 32 slots, K = 20, T_pred = 40) and at the training shape (128 windows).  Next to each time: the bytes of Y the greedy form reads (the kept
world and every live candidate, once per kept world) and their streaming floor at 6.3 TB/s.  Each shape runs in a child process under its own
time limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/worlds_ab.py [--launches 100] [--reps 3]
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
NAMES = {0: "final", 1: "mean", 2: "max"}


def torch_worlds(torch, Y, pres, ws, metric, reduce, t_end, radius, ux, uy, d, chunk=32):
    """The call's outputs in plain torch: (worder, wcount, wmass, wlabel)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    dev = Y.device
    unit = torch.tensor([ux, uy], device=dev)
    t_lo = t_end - 1 if metric == 0 else 0
    Yk = Y.view(n, K, m, T, 2)[:, :, :, t_lo:t_end] * unit
    part = (pres.view(n, m) != 0)
    num = part.sum(1)
    near = torch.empty((n, K, K), device=dev, dtype=torch.bool)
    for w0 in range(0, n, chunk):
        P = Yk[w0:w0 + chunk]
        q = ((P[:, :, None] - P[:, None]) ** 2).sum(-1)                                  # [c, K, K, m, t]
        v = q[..., -1] if metric == 0 else (q.amax(-1) if metric == 2 else q.sqrt().mean(-1))
        pw = part[w0:w0 + chunk, None, None, :]
        if reduce == 0:
            near[w0:w0 + chunk] = ((v < (radius if metric == 1 else radius * radius)) | ~pw).all(-1)
        else:
            di = v if metric == 1 else v.sqrt()
            near[w0:w0 + chunk] = (di * pw).sum(-1) / num[w0:w0 + chunk, None, None].clamp(min=1) < radius
    near = torch.where((num == 0)[:, None, None], torch.full_like(near, radius > 0), near)
    order = torch.sort(ws, dim=1, descending=True, stable=True).indices
    W = torch.softmax(ws, 1)
    rows = torch.arange(n, device=dev)
    kept_idx = torch.full((n, K), K, device=dev, dtype=torch.long)
    count = torch.zeros((n,), device=dev, dtype=torch.long)
    owner = torch.zeros((n, K), device=dev, dtype=torch.long)
    is_kept = torch.zeros((n, K), device=dev, dtype=torch.bool)
    mass = torch.zeros((n, K), device=dev)
    label = torch.zeros((n, K), device=dev, dtype=torch.long)
    for j in range(K):                                                                   # the K-step loop
        k = order[:, j]
        first = torch.where(near[rows, k], kept_idx, torch.full_like(kept_idx, K)).min(1).values
        keep = first == K
        own = torch.where(keep, count, first)
        kept_idx[rows, k] = torch.where(keep, count, kept_idx[rows, k])
        owner[:, j], is_kept[:, j] = own, keep
        mass[rows, own] += W[rows, k]
        label[rows, k] = own
        count = count + keep
    key = torch.where(is_kept, owner, K + torch.arange(K, device=dev)[None])
    worder = torch.gather(order, 1, torch.sort(key, dim=1, stable=True).indices)
    return worder.int(), count.int(), mass, label.int()


def child(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims
    from tests.worlds_reference import make_inputs
    kw = dict(mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, sx=1.0 / 1400.0, sy=1.0 / 1100.0,
              iters=1, posterior=0)
    d, d16 = Dims(n_scenes=n_windows, **kw), Dims(n_scenes=16, **kw)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    rep = n_windows // 16
    h = _lib.Handle(d)
    g = torch.Generator(device="cuda").manual_seed(1)
    i32, n, K, m, T = torch.int32, d.n_scenes, d.K, d.mno, d.T_pred
    score = torch.randn((d.R,), generator=g, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    wo, wl = torch.zeros((n, K), device="cuda", dtype=i32), torch.zeros((n, K), device="cuda", dtype=i32)
    wc, wm = torch.zeros((n,), device="cuda", dtype=i32), torch.zeros((n, K), device="cuda")
    cnt = torch.zeros((n, K + 1, 1, 2), device="cuda", dtype=i32); js = torch.zeros((n, K), device="cuda"); jo = torch.zeros((n, K), device="cuda", dtype=i32)
    r = {"windows": n_windows, "launches": launches, "Y_MB": round(d.R * T * 8 / 1e6, 1), "rows": []}
    for modes in (2, 11):
        Y16, pres16, _ = make_inputs(d16, RADIUS_PX, ux, uy, seed=1, modes=modes)
        Y16 = np.nan_to_num(Y16, nan=0.5).reshape(16, -1, T, 2)
        pres16 = pres16.reshape(16, m).copy()
        Y16[15], pres16[15] = Y16[0], pres16[0]                                          # (the generator's empty window: a copy of the first)
        Y = torch.as_tensor(Y16.reshape(-1, T, 2), device="cuda").repeat(rep, 1, 1).contiguous()
        pres = torch.as_tensor(pres16.reshape(-1), device="cuda").repeat(rep).contiguous()
        joint = lambda: h.joint_metrics(Y.data_ptr(), 0, pres.data_ptr(), score.data_ptr(), [T], 1, RADIUS_PX, ux, uy, cnt.data_ptr(), jo.data_ptr(),
                                        0, 0, js.data_ptr(), 0, s)
        joint()
        torch.cuda.synchronize()
        for metric in (0, 1, 2):
            for reduce in (0, 1):
                call = lambda: h.select_worlds(Y.data_ptr(), pres.data_ptr(), js.data_ptr(), metric, reduce, T, RADIUS_PX, ux, uy, wo.data_ptr(),
                                               wc.data_ptr(), wm.data_ptr(), wl.data_ptr(), s)
                call()
                torch.cuda.synchronize()
                t_o, t_c, t_m, t_l = torch_worlds(torch, Y, pres, js, metric, reduce, T, RADIUS_PX, ux, uy, d)
                agrees = bool(torch.equal(t_o, wo)) and bool(torch.equal(t_c, wc)) and bool(torch.equal(t_l, wl))      # (no pair of this layout sits on the radius)
                us = {"worlds": [], "joint": [], "torch": []}
                for f in (call, joint):
                    for _ in range(10):
                        f()
                torch.cuda.synchronize()
                for _ in range(reps):                                                    # interleaved
                    for k, f in (("worlds", call), ("joint", joint)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(launches):
                            f()
                        e1.record()
                        torch.cuda.synchronize()
                        us[k].append(e0.elapsed_time(e1) * 1000.0 / launches)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()                                                          # the torch statement: the whole thing once (it is milliseconds)
                    torch_worlds(torch, Y, pres, js, metric, reduce, T, RADIUS_PX, ux, uy, d)
                    e1.record()
                    torch.cuda.synchronize()
                    us["torch"].append(e0.elapsed_time(e1) * 1000.0)
                med = {k: float(np.median(v)) for k, v in us.items()}
                # rows read: per kept world i the kept world and every world still live, = the worlds whose label is >= i
                lab, kept = wl.long(), wc.long()
                steps = torch.arange(K, device="cuda")[None, :, None]
                worlds_read = ((lab[:, None, :] >= steps) & (steps < kept[:, None, None])).sum((1, 2))
                nt = 1 if metric == 0 else T
                bytes_read = float((worlds_read * (pres.view(n, m) != 0).sum(1)).sum()) * nt * 8
                row = {"modes": modes, "metric": NAMES[metric], "reduce": "all" if reduce == 0 else "mean", "mean_kept": round(float(wc.float().mean()), 2),
                       "torch_agrees": agrees, "torch_mass_max_diff": round(float((t_m - wm).abs().max()), 8), "MB_read": round(bytes_read / 1e6, 1),
                       "floor_us": round(bytes_read / HBM_BYTES_PER_US, 1), "worlds_over_torch": round(med["worlds"] / med["torch"], 4),
                       "worlds_over_joint": round(med["worlds"] / med["joint"], 3)}
                for k, v in us.items():
                    row[k + "_us"] = "%.1f (%.1f - %.1f)" % (float(np.median(v)), min(v), max(v))
                r["rows"].append(row)
    h.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
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
