"""A/B timing of the off-road term of the training loss (desire_set_offroad_loss) on the training step of `bench.py --train`, by collision_ab.py's
method: BASELINE configs[4] per-GPU shape at 128 windows (32 slots, K = 20, T_pred = 40, H = 128; forward, backward, clip, Adam), one process
per configuration, each under its own time limit, the first failure ends the run; hip events around the timed steps after a warm-up, three
repeats, median (min - max).  Legs: weight 0 (a 64 x 64 field attached, the handle touched by desire_set_offroad_loss(h, 0, ..)), weight > 0 and
-- with `--parent_root DIR`, a checkout of the parent commit with its library built, run by the same child code (which then never touches the
new calls) -- the parent, alternating with the others so that its own process-to-process spread is the yardstick.  Then the stand-alone op
(desire_offroad_loss) next to desire_collision_loss on the same rows, interleaved launches, at 128 and 512 windows, and desire_mask_distance on
the masks.  Not part of bench.py.

    python profiles/ab/offroad_ab.py [--steps 10] [--reps 3] [--launches 200] [--parent_root DIR]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SCALE_PX, WEIGHT, RADIUS_PX, SIDE = 100.0, 0.5, 60.0, 64
STEP_LEGS = {"parent": None, "w0": 0.0, "w_on": WEIGHT}


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


def _field(h, d, n_masks, torch):
    m = torch.as_tensor(_masks(n_masks), device="cuda")
    f = torch.empty((n_masks, SIDE, SIDE), device="cuda", dtype=torch.float32)
    h.mask_distance(m.data_ptr(), n_masks, SIDE, SIDE, (1.0 / d.sx) / SIDE, (1.0 / d.sy) / SIDE, f.data_ptr())
    torch.cuda.synchronize()
    return m, f


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
    if STEP_LEGS[leg] is not None:
        _, field = _field(h, d, 4, torch)
        h.set_offroad_field(field.data_ptr(), 4, SIDE, SIDE, np.arange(d.n_scenes, dtype=np.int32) % 4)
        h.set_offroad_loss(STEP_LEGS[leg], SCALE_PX)
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
         "max_ms": round(max(ms), 3), "loss": round(loss["loss"], 6)}
    if STEP_LEGS[leg]:
        r["L_off"] = round(float(h.device_tensor("off_term")[0]), 6)
        r["count"] = int(h.device_tensor("off_count", "<i4")[: d.n_scenes * d.K].sum())
    h.close()
    return r


def child_op(n_windows: int, launches: int, reps: int) -> dict:
    """desire_offroad_loss and desire_collision_loss, interleaved, on the same Y; desire_mask_distance on the op's masks."""
    import torch
    from desire_amd import _lib
    from desire_amd.spec import init_weights
    from desire_amd.synth import make_case
    d = _dims(n_windows)
    past, fut, _, _, _ = make_case(d, seed=1, n_absent=3)
    h = _lib.Handle(d)
    h.set_weights(init_weights(d, 0))
    past_t = torch.as_tensor(past, device="cuda"); fut_t = torch.as_tensor(fut, device="cuda")
    h.encode(past_t.data_ptr(), fut_t.data_ptr())          # leaves the handle's presence flags
    g = torch.Generator(device="cuda").manual_seed(1)
    gt = (fut_t[..., 1:] * torch.tensor([d.sx, d.sy], device="cuda")).permute(0, 2, 1, 3)             # [n, m, T, 2]
    Y = (gt[:, None] + 0.03 * torch.randn((d.n_scenes, d.K, d.mno, d.T_pred, 2), generator=g, device="cuda")).reshape(d.R, d.T_pred, 2).contiguous()
    A, K, n = d.A, d.K, d.n_scenes
    masks, field = _field(h, d, 4, torch)
    h.set_offroad_field(field.data_ptr(), 4, SIDE, SIDE, np.arange(n, dtype=np.int32) % 4)
    off = torch.zeros((A, K), device="cuda"); count = torch.zeros((n, K), device="cuda", dtype=torch.int32)
    col = torch.zeros((A, K), device="cuda"); touch = torch.zeros((n, K), device="cuda", dtype=torch.int32)
    dY = torch.zeros_like(Y); term = torch.zeros((1,), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    legs = {"offroad_loss": lambda: h.offroad_loss(fut_t.data_ptr(), Y.data_ptr(), SCALE_PX, off.data_ptr(), count.data_ptr(), dY.data_ptr(), term.data_ptr(), s),
            "collision_loss": lambda: h.collision_loss(fut_t.data_ptr(), Y.data_ptr(), RADIUS_PX, ux, uy, col.data_ptr(), touch.data_ptr(), dY.data_ptr(),
                                                       term.data_ptr(), s),
            "mask_distance": lambda: h.mask_distance(masks.data_ptr(), 4, SIDE, SIDE, ux / SIDE, uy / SIDE, field.data_ptr(), s)}
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
    legs["offroad_loss"]()
    torch.cuda.synchronize()
    r = {"leg": "op", "windows": n_windows, "launches": launches}
    for k, v in us.items():
        r[k + "_us"] = _fmt(v, 1)
    r["Y_MB"] = round(d.R * d.T_pred * 8 / 1e6, 1)
    r["off_road_rate"] = round(float(count.float().sum()) / max(float((fut_t[..., 0] != 0).sum()) * K, 1.0), 3)
    r["L_off"] = round(float(term[0]), 6)
    h.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent_root", type=str, default=None, help="a checkout of the parent commit with libdesire_hip.so built: adds the `parent` leg")
    ap.add_argument("--child", type=str, default=None, help="run one configuration in this process: step:<leg> or op:<windows>")
    a = ap.parse_args()
    if a.child:
        kind, _, arg = a.child.partition(":")
        sys.path.insert(0, os.getcwd())                # the tree this child was started in: this one, or the parent's
        print(json.dumps(child_step(arg, a.steps, a.reps) if kind == "step" else child_op(int(arg), a.launches, a.reps)), flush=True)
        return
    here = [("step:w0", ROOT), ("step:w_on", ROOT)]
    legs = list(here)
    if a.parent_root:                                  # the parent alternates with the others
        par = ("step:parent", os.path.abspath(a.parent_root))
        legs = [par, here[0], par, here[1], par, here[0], par, here[1], par]
    legs += [("op:128", ROOT), ("op:512", ROOT)]
    for leg, cwd in legs:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps), "--launches", str(a.launches),
                            "--reps", str(a.reps)], cwd=cwd, timeout=300)
        if p.returncode != 0:
            raise SystemExit("%s failed with exit status %d: nothing more is started" % (leg, p.returncode))


if __name__ == "__main__":
    main()
