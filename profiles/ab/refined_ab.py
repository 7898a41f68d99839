"""A/B timing of the terms on the refined trajectories (desire_set_refined_loss) on the training step of `bench.py --train`, by offroad_ab.py's
method: BASELINE configs[4] per-GPU shape at 128 windows (32 slots, K = 20, T_pred = 40, H = 128; forward, backward, clip, Adam), one process
per configuration, each under its own time limit, the first failure ends the run; hip events around the timed steps after a warm-up, three
repeats, median (min - max).  Legs: `default` (an untouched handle), `off` (radius, field and scale set at weight 0, then
desire_set_refined_loss(h, 0, 0, 0): the launches of the default), `rcol`, `roff`, `recon` (soft-min, the regression term weighted from the
refined errors; next to `softmin`, the same mode with the flag off) and `all`; with `--parent_root DIR`, a checkout of the parent commit with
its library built, run by the same child code (which then never touches the new call), the parent alternates with the others so that its own
process-to-process spread is the yardstick.  `--control`: only `touched` -- radius, field and scale at weight 0 and NO call of the new setter,
which both trees can run -- alternating between the two trees with `off`: what attaching a field costs a process on either tree.  Not part of
bench.py.

    python profiles/ab/refined_ab.py [--steps 10] [--reps 3] [--parent_root DIR] [--control]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SCALE_PX, WEIGHT, RADIUS_PX, SIDE, TAU = 100.0, 0.5, 60.0, 64, 0.01
# leg -> (recon mode of the handle, refined recon flag, refined collision weight, refined off-road weight); None: nothing is touched
# (a flag of None: the new setter is not called)
STEP_LEGS = {"parent": None, "default": None, "touched": (0, None, 0.0, 0.0), "parent_touched": (0, None, 0.0, 0.0), "off": (0, 0, 0.0, 0.0),
             "rcol": (0, 0, WEIGHT, 0.0), "roff": (0, 0, 0.0, WEIGHT), "softmin": (2, 0, 0.0, 0.0), "recon": (2, 1, 0.0, 0.0),
             "all": (2, 1, WEIGHT, WEIGHT)}


def _fmt(v, prec=3):
    return "%.*f (%.*f - %.*f)" % (prec, float(np.median(v)), prec, min(v), prec, max(v))


def _dims(n_windows):
    from desire_amd.spec import Dims
    return Dims(n_scenes=n_windows, mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, sx=1.0 / 1400.0,
                sy=1.0 / 1100.0, iters=1, posterior=1)


def _masks(n_masks):
    """Road masks: a wall band along the top with a wavy edge and a wall block inside the road (about 45 % wall)."""
    yy, xx = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    out = np.ones((n_masks, SIDE, SIDE), np.uint8)
    for i in range(n_masks):
        out[i][yy + 0.5 < SIDE * (0.38 + 0.08 * np.sin(2 * np.pi * xx / SIDE + i))] = 0
        out[i][(xx >= 0.5 * SIDE) & (xx < 0.75 * SIDE) & (yy >= 0.55 * SIDE) & (yy < 0.75 * SIDE)] = 0
    return out


def child_step(leg: str, steps: int, reps: int) -> dict:
    """The training step of bench.py --train under one leg of STEP_LEGS (parent: the package on sys.path is the parent's, nothing is set)."""
    import torch
    from desire_amd import _lib
    from desire_amd.spec import init_weights
    from desire_amd.synth import make_case
    d = _dims(128)
    past, fut, eps, grids, gos = make_case(d, seed=1, n_absent=0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    past_t, fut_t, eps_t, grids_t = t(past), t(fut), t(eps), t(grids)
    h = _lib.Handle(d)
    h.set_weights(init_weights(d, 0))
    h.set_scene_grids(grids_t.data_ptr(), gos)
    h.set_training(True)
    cfg = STEP_LEGS[leg]
    if cfg is not None:
        mode, recon, rcw, row = cfg
        m = torch.as_tensor(_masks(4), device="cuda")
        field = torch.empty((4, SIDE, SIDE), device="cuda", dtype=torch.float32)
        h.mask_distance(m.data_ptr(), 4, SIDE, SIDE, (1.0 / d.sx) / SIDE, (1.0 / d.sy) / SIDE, field.data_ptr())
        torch.cuda.synchronize()
        h.set_offroad_field(field.data_ptr(), 4, SIDE, SIDE, np.arange(d.n_scenes, dtype=np.int32) % 4)
        h.set_offroad_loss(0.0, SCALE_PX)
        h.set_collision_loss(0.0, RADIUS_PX, 1.0 / d.sx, 1.0 / d.sy)
        if mode:
            h.set_recon_loss(mode, TAU)
        if recon is not None:
            h.set_refined_loss(recon, rcw, row)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda")
    score = torch.zeros((d.R,), device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def step():
        h.forward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr(), Y.data_ptr(), score.data_ptr(), s)
        h.backward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr(), s)
        h.clip_grads(10.0, stream=s)
        h.adam_step(1e-4, stream=s)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    loss = h.train_loss(fut_t.data_ptr())
    r = {"leg": "step", "mode": leg, "steps": steps, "step_ms": _fmt(ms), "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3),
         "max_ms": round(max(ms), 3), "loss": round(loss["loss"], 6), "reg": round(loss["reg"], 6)}
    if cfg is not None and cfg[2] > 0:
        r["L_col_Y"] = round(float(h.device_tensor("rcol_term")[0]), 6)
        r["touch"] = int(h.device_tensor("rcol_touch", "<i4")[: d.n_scenes * d.K].sum())
    if cfg is not None and cfg[3] > 0:
        r["L_off_Y"] = round(float(h.device_tensor("roff_term")[0]), 6)
        r["count"] = int(h.device_tensor("roff_count", "<i4")[: d.n_scenes * d.K].sum())
    h.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent_root", type=str, default=None, help="a checkout of the parent commit with libdesire_hip.so built: adds the `parent` leg")
    ap.add_argument("--control", action="store_true", help="only the `touched` control on both trees, alternating with `off` (needs --parent_root)")
    ap.add_argument("--child", type=str, default=None, help="run one configuration in this process: a leg of STEP_LEGS")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.getcwd())                # the tree this child was started in: this one, or the parent's
        print(json.dumps(child_step(a.child, a.steps, a.reps)), flush=True)
        return
    order = ["default", "off", "rcol", "roff", "softmin", "recon", "all"]
    if a.parent_root:                                  # the parent alternates with the others; default and off, which carry the only bar, run twice
        order = ["parent", "default", "parent", "off", "parent", "rcol", "roff", "parent", "softmin", "recon", "parent", "all", "parent", "default",
                 "off", "parent"]
    if a.control:
        if not a.parent_root:
            raise SystemExit("--control needs --parent_root")
        order = ["parent_touched", "off", "touched", "parent_touched", "off", "touched", "parent_touched"]
    legs = [(leg, os.path.abspath(a.parent_root) if leg.startswith("parent") else ROOT) for leg in order]
    for leg, cwd in legs:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps), "--reps", str(a.reps)], cwd=cwd, timeout=300)
        if p.returncode != 0:
            raise SystemExit("%s failed with exit status %d: nothing more is started" % (leg, p.returncode))


if __name__ == "__main__":
    main()
