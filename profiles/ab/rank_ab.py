"""Same-process timing of the ranking calls against the ADE / FDE harness they sit next to, on seeded synthetic buffers (the calls need the
handle's dims only: no weights, no forward): (a) desire_ade_fde, (b) desire_ranked_errors with four horizons, (c) desire_rank_samples with
n_top = 2 and the gather -- alternating, hip events around N back-to-back launches each after a warm-up (one launch is tens of microseconds:
a single launch measures the clock), at the headline shape (512 windows x 32 slots, K = 20, T_pred = 40) and at the training shape (128
windows).  (b) is also stated against the streaming floor: the bytes of Y / 6.3 TB/s.  Each shape runs in a child process under its own time
limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/rank_ab.py [--launches 200] [--reps 5]
    rocprofv3 --kernel-trace --stats -d out -- python profiles/ab/rank_ab.py --child 512 --launches 50 --reps 1      # per-kernel times
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


def child(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims
    d = Dims(n_scenes=n_windows, mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15,
             sx=1.0 / 1400.0, sy=1.0 / 1100.0, iters=1, posterior=0)
    h = _lib.Handle(d)
    g = torch.Generator(device="cuda").manual_seed(1)
    Y = torch.rand((d.R, d.T_pred, 2), generator=g, device="cuda")
    score = torch.randn((d.R,), generator=g, device="cuda")
    fut = torch.rand((d.n_scenes, d.T_pred, d.mno, 3), generator=g, device="cuda") * 1000.0 + 1.0      # every id != 0: every frame counts
    af = torch.zeros((d.A, 4), device="cuda")
    order = torch.zeros((d.A, d.K), device="cuda", dtype=torch.int32)
    top_Y = torch.zeros((d.A, 2, d.T_pred, 2), device="cuda"); top_s = torch.zeros((d.A, 2), device="cuda")
    out = torch.zeros((d.A, 4, 4), device="cuda")
    hz = [10, 20, 30, 40]
    s = torch.cuda.current_stream().cuda_stream
    legs = {"ade_fde": lambda: h.ade_fde(Y.data_ptr(), fut.data_ptr(), af.data_ptr(), s),
            "ranked_errors": lambda: h.ranked_errors(Y.data_ptr(), fut.data_ptr(), order.data_ptr(), 2, hz, 1.0 / d.sx, 1.0 / d.sy, out.data_ptr(), s),
            "rank_samples": lambda: h.rank_samples(score.data_ptr(), Y.data_ptr(), 2, order.data_ptr(), top_Y.data_ptr(), top_s.data_ptr(), s)}
    legs["rank_samples"]()                         # a real order for the error selection
    for f in legs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(reps):                          # interleaved: a, b, c, a, b, c, ...
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1000.0 / launches)
    r = {"windows": n_windows, "launches": launches}
    r.update({k + "_us": round(float(np.median(v)), 2) for k, v in us.items()})
    floor = d.R * d.T_pred * 8 / HBM_BYTES_PER_US
    r["Y_MB"] = round(d.R * d.T_pred * 8 / 1e6, 1)
    r["floor_us"] = round(floor, 2)
    r["ranked_errors_over_floor"] = round(r["ranked_errors_us"] / floor, 2)
    r["ranked_errors_over_ade_fde"] = round(r["ranked_errors_us"] / r["ade_fde_us"], 3)
    h.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
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
