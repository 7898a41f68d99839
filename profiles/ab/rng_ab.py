"""Same-process A/B of the latent noise: eps GIVEN by the caller (a [R, L] tensor the reparameterisation reads: 168 MB at 512 headline windows) against
eps GENERATED on the device (desire_set_rng, NULL eps: Philox4x32-10 + Box-Muller inside the kernel, about 100 vector operations per four normals).
ONE handle per shape serves both legs -- the argument alone differs -- alternating given, generated, given, ...; hip events around N back-to-back calls
after a warm-up:
  * inference, 512 windows of the headline dims (32 slots, K = 20, T 8 / 40, H = 128, L = 128, fp32): the whole desire_forward, and the `reparam` stage
    alone -- the stage has no entry point of its own, so its time is the handle's own event pair around that one launch (desire_set_profiling) over
    --stage-calls forwards per leg;
  * training, the BASELINE configs[4] step at 128 windows (forward with saves + backward + clip + Adam): the generated leg also regenerates eps in
    the backward and holds no eps tensor (R * L * 4 bytes).
Per leg: median and (min, max) over the repeats, so that a difference can be read against the given leg's own spread.  Each shape runs in a child
process under its own time limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/rng_ab.py [--launches 200] [--reps 3]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def child(n_windows: int, train: bool, launches: int, reps: int, stage_calls: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims, init_weights
    from desire_amd.synth import make_case
    d = Dims(n_scenes=n_windows, mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15,
             sx=1.0 / 1400.0, sy=1.0 / 1100.0, iters=1, posterior=1)
    w = init_weights(d, 0)
    past, fut, _, grids, gos = make_case(d, seed=1, n_absent=0)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    p_t, f_t, g_t = t(past), t(fut), t(grids)
    h = _lib.Handle(d)
    h.set_weights(w)
    h.set_scene_grids(g_t.data_ptr(), gos)
    if train:
        h.set_training(True)
    s = torch.cuda.current_stream().cuda_stream
    h.set_rng(1234, 0, s)
    e_t = torch.empty((d.R, d.L), device="cuda")
    h.rng_fill(1234, 0, 0, _lib.RNG_LATENT, e_t.data_ptr(), e_t.numel(), s)          # the given leg reads normals of the same generator (draw 0)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")

    def one(eps_ptr):
        h.forward(p_t.data_ptr(), f_t.data_ptr(), eps_ptr, Y.data_ptr(), sc.data_ptr(), s)
        if train:
            h.backward(p_t.data_ptr(), f_t.data_ptr(), eps_ptr, s)
            h.clip_grads(10.0, stream=s)
            h.adam_step(1e-4, stream=s)

    legs = {"given": e_t.data_ptr(), "generated": 0}
    for ptr in legs.values():
        one(ptr); one(ptr)
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, ptr in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                one(ptr)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / launches)
            print("%s: %.4f ms" % (k, ms[k][-1]), file=sys.stderr, flush=True)
    r = {"windows": n_windows, "mode": "train_step" if train else "forward", "launches": launches, "reps": reps,
         "eps_MB": round(d.R * d.L * 4 / 1e6, 1)}
    for k in legs:
        r[k + "_ms"] = stats(ms[k])
    r["generated_minus_given_ms"] = round(r["generated_ms"]["median"] - r["given_ms"]["median"], 4)
    r["given_spread_ms"] = round(r["given_ms"]["max"] - r["given_ms"]["min"], 4)
    # the stage alone: the handle's own event pair around the reparam launch (and, training, the backward stage that holds k_reparam_bwd)
    stage = {k: {} for k in legs}
    h.set_profiling(True)
    for _ in range(stage_calls):
        for k, ptr in legs.items():
            one(ptr)
            torch.cuda.synchronize()
            for name, v in h.get_profile():
                if name in ("reparam", "bwd_cvae_enc"):
                    stage[k].setdefault(name, []).append(v)
    h.set_profiling(False)
    for k in legs:
        for name, v in stage[k].items():
            r["%s_%s_us" % (k, name)] = {a: round(b * 1000.0, 1) for a, b in stats(v).items()}
    h.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stage-calls", type=int, default=20)
    ap.add_argument("--child", type=int, default=0, help="run one shape (this many windows) in this process")
    ap.add_argument("--train", action="store_true", help="with --child: the training step instead of the forward")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.train, a.launches, a.reps, a.stage_calls)), flush=True)
        return
    for n, train in ((512, False), (128, True)):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--launches", str(a.launches), "--reps", str(a.reps),
               "--stage-calls", str(a.stage_calls)] + (["--train"] if train else [])
        p = subprocess.run(cmd, cwd=ROOT, timeout=900)
        if p.returncode != 0:
            raise SystemExit("shape %d failed with exit status %d: nothing more is started" % (n, p.returncode))


if __name__ == "__main__":
    main()
