"""Same-process A/B of scene training: the BASELINE configs[4] training step (128 windows x 32 slots x K = 20 = 81 920 samples, T 8 / 40, H = 128,
forward with saves + backward + clip + Adam) with precomputed grids (off), with desire_set_option(h, "scene_grad", 1) (on), and with scene images
attached (images: the scene CNN forward and backward every step), fp32 and split-bf16
operands on synthetic windows, and the compacted (COMPACT_ROWS | COMPACT_IOC) split step on real SDD bookstore windows.  Step times from hip
events around N steps; with --profile, the per-entry split of desire_set_profiling for one step of each variant.  Not part of bench.py.

    python profiles/ab/scene_train_ab.py [--steps 6] [--profile]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    from benchlib.common import sdd_windows
    from desire_amd import _lib
    from desire_amd.spec import Dims, init_weights
    from desire_amd.synth import make_case
    d = Dims(n_scenes=128, mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15,
             sx=1.0 / 1400.0, sy=1.0 / 1100.0, iters=1, posterior=1)
    w = init_weights(d, 0)
    past, fut, eps, grids, gos = make_case(d, seed=1, n_absent=0)
    W_IMG, H_IMG = 1424.0, 1088.0
    ds = d.replace(nb_w=32.0 / W_IMG, nb_h=32.0 / H_IMG, sx=1.0 / W_IMG, sy=1.0 / H_IMG)
    p_sdd, f_sdd, _ = sdd_windows(ds.n_scenes, ds.mno)
    dev = torch.device("cuda")
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    e_t, g_t = t(eps), t(grids)
    img_t = t(np.random.default_rng(2).uniform(0, 1, (d.n_grids, 4 * d.Gh, 4 * d.Gw, 3)).astype(np.float32))
    stream = torch.cuda.current_stream().cuda_stream
    Y = torch.zeros((d.R, d.T_pred, 2), device=dev)
    sc = torch.zeros((d.R,), device=dev)
    legs = [("fp32", d, 0, 0, t(past), t(fut)), ("split", d, 2, 0, t(past), t(fut)), ("split_sdd_compact", ds, 2, 12, t(p_sdd), t(f_sdd))]
    res = {}
    for tag, dd, mode, flags, p_t, f_t in legs:
        handles = {}
        for sg in (0, 1, 2):
            h = _lib.Handle(dd.replace(bf16=mode, flags=flags))
            h.set_weights(w)
            if sg == 2:
                h.set_scene_images(img_t.data_ptr(), 4 * dd.Gh, 4 * dd.Gw, gos)
            else:
                h.set_scene_grids(g_t.data_ptr(), gos)
                h.set_option("scene_grad", sg)
            h.set_training(True)
            handles[sg] = h

        def one(h):
            h.forward(p_t.data_ptr(), f_t.data_ptr(), e_t.data_ptr(), Y.data_ptr(), sc.data_ptr(), stream)
            h.backward(p_t.data_ptr(), f_t.data_ptr(), e_t.data_ptr(), stream)
            h.clip_grads(10.0, stream=stream)
            h.adam_step(1e-4, stream=stream)

        ms = {0: [], 1: [], 2: []}
        for h in handles.values():
            one(h); one(h)
        torch.cuda.synchronize()
        for rep in range(3):                     # interleaved: off, on, off, on, ...
            for sg, h in handles.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    one(h)
                e1.record()
                torch.cuda.synchronize()
                ms[sg].append(e0.elapsed_time(e1) / a.steps)
        r = {"ms_off": float(np.median(ms[0])), "ms_on": float(np.median(ms[1])), "ms_images": float(np.median(ms[2]))}
        r["ratio"] = r["ms_on"] / r["ms_off"]
        r["ratio_images"] = r["ms_images"] / r["ms_off"]
        if a.profile:
            for sg, h in handles.items():
                h.set_profiling(True)
                one(h)
                torch.cuda.synchronize()
                prof = {}
                for name, v in h.get_profile():
                    prof[name] = prof.get(name, 0.0) + v
                h.set_profiling(False)
                r[("profile_off", "profile_on", "profile_images")[sg]] = {k: round(v, 3) for k, v in prof.items()}
        res[tag] = r
        print(tag, json.dumps(r), flush=True)
        for h in handles.values():
            h.close()
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
