"""Same-process A/B of the Gaussian-head rollout: K calls of desire_rollout(num = T_pred) -- one trajectory per agent and call, K warm-ups, the head
on 32 threads of each workgroup -- against ONE desire_rollout_samples -- K rollouts per agent in the sample layout, one warm-up, the head on the whole
workgroup -- on the same handle, at 1 and at 512 windows of the headline dims (32 slots, K = 20, T 8 / 40, H = 128, fp32).  Legs, alternating:
  old        K back-to-back desire_rollout calls on normals [T_pred, A, 2] each;
  new        one desire_rollout_samples on explicit normals [R, T_pred, 2];
  new_rng    one desire_rollout_samples with NULL normals (drawn in the kernel; no noise tensor).
hip events around N back-to-back units after a warm-up; per leg the median and (min, max) over the repeats, so that a difference can be read against
the old leg's own spread.  Both legs do the same arithmetic per (row, step); the condition DESIGN.md 7c records is new <= old.  One process; a shape
that fails ends the run.  Not part of bench.py.

    python profiles/ab/rollout_ab.py [--launches 20] [--reps 3] [--windows 1,512]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def shape(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims, init_weights
    from desire_amd.synth import make_case
    d = Dims(n_scenes=n_windows, mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15,
             sx=1.0 / 1400.0, sy=1.0 / 1100.0, iters=1, posterior=0)
    w = init_weights(d, 0)
    w["gauss_head/b"] = np.array([0.45, 0.5, -3.0, -3.5, 0.3], np.float32)
    past, _, _, _, _ = make_case(d, seed=1, n_absent=0)
    p_t = torch.as_tensor(np.ascontiguousarray(past), device="cuda")
    h = _lib.Handle(d)
    h.set_weights(w)
    s = torch.cuda.current_stream().cuda_stream
    h.set_rng(1234, 0, s)
    n_new = torch.empty((d.R, d.T_pred, 2), device="cuda")
    h.rng_fill(1234, 0, 0, _lib.RNG_ROLLOUT, n_new.data_ptr(), n_new.numel(), s)
    n_old = torch.empty((d.K, d.T_pred, d.A, 2), device="cuda")
    h.rng_fill(1234, 1, 0, _lib.RNG_NORMAL, n_old.data_ptr(), n_old.numel(), s)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda")
    out = torch.zeros((d.K, d.T_pred, d.A, 2), device="cuda")

    def old():
        for k in range(d.K):
            h.rollout(p_t.data_ptr(), n_old[k].data_ptr(), d.T_pred, out[k].data_ptr(), s)

    legs = {"old": old,
            "new": lambda: h.rollout_samples(p_t.data_ptr(), n_new.data_ptr(), Y.data_ptr(), s),
            "new_rng": lambda: h.rollout_samples(p_t.data_ptr(), 0, Y.data_ptr(), s)}
    for f in legs.values():
        f(); f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / launches)
            print("%d windows, %s: %.4f ms" % (n_windows, k, ms[k][-1]), file=sys.stderr, flush=True)
    r = {"windows": n_windows, "K": d.K, "rows": d.R, "launches": launches, "reps": reps, "normals_MB": round(d.R * d.T_pred * 8 / 1e6, 1)}
    for k in legs:
        r[k + "_ms"] = stats(ms[k])
    r["old_spread_ms"] = round(r["old_ms"]["max"] - r["old_ms"]["min"], 4)
    r["new_over_old"] = round(r["new_ms"]["median"] / r["old_ms"]["median"], 4)
    r["new_rng_over_old"] = round(r["new_rng_ms"]["median"] / r["old_ms"]["median"], 4)
    r["new_not_slower"] = bool(r["new_ms"]["median"] <= r["old_ms"]["median"])
    # the warm-up and the rollout kernel alone: the handle's own event pairs
    h.set_profiling(True)
    h.rollout_samples(p_t.data_ptr(), n_new.data_ptr(), Y.data_ptr(), s)
    torch.cuda.synchronize()
    for name, v in h.get_profile():
        r[name + "_us"] = round(v * 1000.0, 1)
    h.set_profiling(False)
    h.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=str, default="1,512")
    a = ap.parse_args()
    for n in (int(x) for x in a.windows.split(",")):
        print(json.dumps(shape(n, a.launches, a.reps)), flush=True)


if __name__ == "__main__":
    main()
