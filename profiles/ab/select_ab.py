"""Same-process timing of the score-ordered non-maximum suppression (desire_select_diverse) on the layout of tests/select_reference.py's
generator (modes, chains and scatter around a 20-pixel radius; sixteen windows generated, tiled to the shape -- a result depends on its agent
alone), called at the radius that leaves about three samples kept per agent (eight times the layout's) and at the layout's own radius (about
twelve kept), against (a) desire_ranked_errors with four horizons -- the like-for-like neighbour: it streams the same Y once -- and (b) a plain
torch formulation on the same device, what a user has without the call: pairwise distances in chunks of windows plus the K-step greedy loop.
Alternating, hip events around N back-to-back launches each after a warm-up, three repeats, at the headline shape (512 windows x 32 slots,
K = 20, T_pred = 40) and at the training shape (128 windows).  Each time is stated against the streaming floor of what the call stages: the bytes
of Y it reads / 6.3 TB/s.  Each shape runs in a child process under its own time limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/select_ab.py [--launches 200] [--reps 3]
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
METRICS = (("final", 0), ("mean", 1), ("max", 2))


def torch_select(torch, Y, order, metric, radius, ux, uy, d, chunk=32):
    """The selection in plain torch: [n, mno, K, K] distances per chunk of windows, then K dependent steps.  Returns (order out, count)."""
    K = d.K
    Yk = Y.view(d.n_scenes, K, d.mno, d.T_pred, 2).permute(0, 2, 1, 3, 4)                     # [n, mno, K, T, 2]
    unit = torch.tensor([ux, uy], device=Y.device)
    out = torch.empty_like(order)
    count = torch.empty((d.A,), device=Y.device, dtype=torch.int32)
    for w0 in range(0, d.n_scenes, chunk):
        y = Yk[w0:w0 + chunk].reshape(-1, K, d.T_pred, 2)
        o = order[w0 * d.mno:(w0 + chunk) * d.mno].long()
        y = torch.gather(y, 1, o[:, :, None, None].expand(-1, -1, d.T_pred, 2))              # rows in processing order
        if metric == 0:
            df = (y[:, :, None, -1] - y[:, None, :, -1]) * unit
            near = (df * df).sum(-1) < radius * radius
        else:
            df = (y[:, :, None] - y[:, None, :]) * unit                                        # [a, K, K, T, 2]
            q = (df * df).sum(-1)
            near = (q.sqrt().mean(-1) < radius) if metric == 1 else (q.amax(-1) < radius * radius)
        kept = torch.zeros(near.shape[:2], dtype=torch.bool, device=Y.device)
        for j in range(K):                                                                     # the greedy pass: K dependent steps
            kept[:, j] = ~(near[:, j] & kept).any(1)
        key = (~kept).long() * K + torch.arange(K, device=Y.device)                            # the kept first, both parts in processing order
        out[w0 * d.mno:(w0 + chunk) * d.mno] = torch.gather(o, 1, key.argsort(1)).int()
        count[w0 * d.mno:(w0 + chunk) * d.mno] = kept.sum(1).int()
    return out, count


def child(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims
    from tests.select_reference import make_inputs
    kw = dict(mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, sx=1.0 / 1400.0, sy=1.0 / 1100.0,
              iters=1, posterior=0)
    d, d16 = Dims(n_scenes=n_windows, **kw), Dims(n_scenes=16, **kw)
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    Y16, _ = make_inputs(d16, RADIUS_PX, ux, uy, seed=1, cases=[], absent=False)
    h = _lib.Handle(d)
    g = torch.Generator(device="cuda").manual_seed(1)
    Y = torch.as_tensor(Y16, device="cuda").repeat(n_windows // 16, 1, 1).contiguous()
    fut = torch.rand((d.n_scenes, d.T_pred, d.mno, 3), generator=g, device="cuda") * 1000.0 + 1.0
    score = torch.randn((d.R,), generator=g, device="cuda")
    order = torch.zeros((d.A, d.K), device="cuda", dtype=torch.int32); div = torch.zeros_like(order)
    count = torch.zeros((d.A,), device="cuda", dtype=torch.int32); mass = torch.zeros((d.A, d.K), device="cuda")
    top = 2
    top_Y = torch.zeros((d.A, top, d.T_pred, 2), device="cuda"); top_s = torch.zeros((d.A, top), device="cuda")
    out4 = torch.zeros((d.A, 4, 4), device="cuda")
    hz = [10, 20, 30, 40]
    s = torch.cuda.current_stream().cuda_stream
    h.rank_samples(score.data_ptr(), 0, top, order.data_ptr(), 0, 0, s)

    def sel(metric, radius):
        return lambda: h.select_diverse(Y.data_ptr(), order.data_ptr(), score.data_ptr(), metric, d.T_pred, radius, ux, uy, top, div.data_ptr(),
                                        count.data_ptr(), mass.data_ptr(), top_Y.data_ptr(), top_s.data_ptr(), s)

    legs = {"ranked_errors": lambda: h.ranked_errors(Y.data_ptr(), fut.data_ptr(), order.data_ptr(), top, hz, ux, uy, out4.data_ptr(), s)}
    r = {"windows": n_windows, "launches": launches}
    for name, metric in METRICS:
        for tag, mult in (("r8", 8.0), ("r1", 1.0)):
            legs["select_%s_%s" % (name, tag)] = sel(metric, RADIUS_PX * mult)
            legs["select_%s_%s" % (name, tag)]()
            torch.cuda.synchronize()
            r["kept_%s_%s" % (name, tag)] = round(float(count.float().mean()), 2)
            if tag == "r8":                        # the torch formulation selects the same samples (no pair of this layout sits on the radius)
                t_order, t_count = torch_select(torch, Y, order, metric, RADIUS_PX * mult, ux, uy, d)
                r["torch_agrees_%s" % name] = bool(torch.equal(t_count, count)) and bool(torch.equal(t_order, div))
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
    r.update({k + "_us": round(float(np.median(v)), 2) for k, v in us.items()})
    for name, metric in METRICS:                   # the torch formulation: a few repeats of the whole thing (it is milliseconds)
        ts = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch_select(torch, Y, order, metric, RADIUS_PX * 8.0, ux, uy, d)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1000.0)
        r["torch_%s_us" % name] = round(float(np.median(ts)), 1)
    y_bytes = d.R * d.T_pred * 8
    r["Y_MB"] = round(y_bytes / 1e6, 1)
    for name, metric in METRICS:                   # staged: every frame, or the last one of every row (FINAL); plus the gathered rows
        staged = (d.R * 8 if metric == 0 else y_bytes) + d.A * top * d.T_pred * 8
        r["floor_%s_us" % name] = round(staged / HBM_BYTES_PER_US, 2)
        r["select_%s_r8_over_ranked_errors" % name] = round(r["select_%s_r8_us" % name] / r["ranked_errors_us"], 3)
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
