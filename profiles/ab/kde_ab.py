"""Same-process timing of the KDE log-likelihood against the call it sits next to, on seeded synthetic buffers (the calls need the handle's dims
only: no weights, no forward): (a) desire_ranked_errors with four horizons -- the yardstick: it streams the same Y and the same targets --
(b) desire_kde_nll with equal weights, (c) desire_kde_nll with softmax(score) weights; alternating, hip events around N back-to-back launches
each after a warm-up (one launch is tens of microseconds: a single launch measures the clock), three repeats, at the headline shape (512 windows
x 32 slots, K = 20, T_pred = 40) and at the training shape (128 windows).  The bytes a KDE call moves: Y once, the targets, the scores and
weights, the outputs; effective TB/s = those bytes / the median.  Each shape runs in a child process under its own time limit; the first failure
ends the run.  Not part of bench.py.

    python profiles/ab/kde_ab.py [--launches 200] [--reps 3]
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
    fut = torch.rand((d.n_scenes, d.T_pred, d.mno, 3), generator=g, device="cuda") * 1000.0 + 1.0      # every id != 0: every frame counts
    # samples scattered around the scaled ground truth: no frame is degenerate, every lane takes the whole density path
    gt = (fut[..., 1:] * torch.tensor([d.sx, d.sy], device="cuda")).permute(0, 2, 1, 3)                 # [n, mno, T, 2]
    Y = (gt[:, None] + 0.01 * torch.randn((d.n_scenes, d.K, d.mno, d.T_pred, 2), generator=g, device="cuda")).reshape(d.R, d.T_pred, 2).contiguous()
    score = torch.randn((d.R,), generator=g, device="cuda")
    order = torch.zeros((d.A, d.K), device="cuda", dtype=torch.int32)
    out4 = torch.zeros((d.A, 4, 4), device="cuda")
    out2 = torch.zeros((d.A, 4, 2), device="cuda")
    frame = torch.zeros((d.A, d.T_pred), device="cuda")
    hz = [10, 20, 30, 40]
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    s = torch.cuda.current_stream().cuda_stream
    h.rank_samples(score.data_ptr(), 0, 2, order.data_ptr(), 0, 0, s)       # a real order for the error selection
    legs = {"ranked_errors": lambda: h.ranked_errors(Y.data_ptr(), fut.data_ptr(), order.data_ptr(), 2, hz, ux, uy, out4.data_ptr(), s),
            "kde_uniform": lambda: h.kde_nll(Y.data_ptr(), fut.data_ptr(), 0, hz, ux, uy, _lib.KDE_LOG_FLOOR, out2.data_ptr(), frame.data_ptr(), s),
            "kde_weighted": lambda: h.kde_nll(Y.data_ptr(), fut.data_ptr(), score.data_ptr(), hz, ux, uy, _lib.KDE_LOG_FLOOR, out2.data_ptr(),
                                              frame.data_ptr(), s)}
    for f in legs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    floored = int((frame <= _lib.KDE_LOG_FLOOR).sum())
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
    r = {"windows": n_windows, "launches": launches, "floored_frames": floored, "frames": int(frame.numel())}
    r.update({k + "_us": round(float(np.median(v)), 2) for k, v in us.items()})
    y_bytes = d.R * d.T_pred * 8
    kde_bytes = y_bytes + fut.numel() * 4 + 3 * d.R * 4 + out2.numel() * 4 + frame.numel() * 4 + d.A * 16      # (scores read, weights written and read)
    r["Y_MB"] = round(y_bytes / 1e6, 1)
    r["kde_MB"] = round(kde_bytes / 1e6, 1)
    r["floor_us"] = round(kde_bytes / HBM_BYTES_PER_US, 2)
    for k in ("kde_uniform", "kde_weighted"):
        r[k + "_over_ranked_errors"] = round(r[k + "_us"] / r["ranked_errors_us"], 3)
        r[k + "_TBps"] = round(kde_bytes / r[k + "_us"] / 1e6, 2)
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
