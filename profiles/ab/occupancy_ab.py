"""Same-process timing of the predicted occupancy maps (desire_occupancy) on the layout of tests/occupancy_reference.py's generator (sixteen windows
generated, tiled to the shape -- a result depends on its window alone) at the headline shape (32 slots, K = 20, T_pred = 40, four horizons, a
64 x 64 grid), in both modes, with the maps alone and with every optional output, against a plain torch statement of the same outputs on the same
device -- what a user has without the call, not the code under test: the cells, a scatter of the weights (mode AT: scatter_add, float atomics)
or of visit flags (mode UNTIL: one flag per (sample, cell), then the weighted sum over k), the sum and the product over the agents.
Hip events around N back-to-back launches each after a warm-up, three repeats, median (min - max), at 512 and at 128 windows.  Each time is
stated next to the streaming floor of the bytes the call has to move at 6.3 TB/s: Y once per horizon, the maps written.  Each shape runs in a
child process under its own time limit; the first failure ends the run.  Not part of bench.py.

    python profiles/ab/occupancy_ab.py [--launches 200] [--reps 3]
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
GRID = (64, 64)


def torch_occupancy(torch, Y, present, score, hz, until, d):
    """The call's outputs in plain torch, prediction form: (occ, expected, off)."""
    n, K, m, T = d.n_scenes, d.K, d.mno, d.T_pred
    Oh, Ow = GRID
    C = Oh * Ow
    Yk = Y.view(n, K, m, T, 2).permute(0, 2, 1, 3, 4)                                              # [n, m, K, T, 2]
    fx, fy = torch.floor(Yk[..., 0] * Ow), torch.floor(Yk[..., 1] * Oh)
    inside = (fx >= 0) & (fx <= Ow - 1) & (fy >= 0) & (fy <= Oh - 1)
    cell = torch.where(inside, fy * Ow + fx, torch.full_like(fx, C)).long().reshape(n * m, K, T)    # cell C: off frame
    w = torch.softmax(score.view(n, K, m).permute(0, 2, 1), -1).reshape(n * m, K) * present.view(n * m, 1).float()
    occ, exp, off = [], [], []
    visit = torch.zeros((n * m, K, C + 1), device=Y.device, dtype=torch.bool) if until else None
    t0 = 0
    for h in hz:
        if until:
            visit.scatter_(2, cell[:, :, t0:h], True)
            p = torch.bmm(w[:, None, :], visit.float())[:, 0]                                       # [n m, C + 1]
            off.append(torch.bmm(w[:, None, :], visit[:, :, C:].float())[:, 0, 0])
            t0 = h
        else:
            p = torch.zeros((n * m, C + 1), device=Y.device).scatter_add_(1, cell[:, :, h - 1], w)
            off.append(p[:, C])
        p = p[:, :C].view(n, m, C)
        exp.append(p.sum(1))
        occ.append(1.0 - (1.0 - p).prod(1))
    return torch.stack(occ, 1).view(n, len(hz), Oh, Ow), torch.stack(exp, 1).view(n, len(hz), Oh, Ow), torch.stack(off, 1).view(n, m, len(hz))


def child(n_windows: int, launches: int, reps: int) -> dict:
    import torch
    from desire_amd import _lib
    from desire_amd.spec import Dims
    from tests.occupancy_reference import make_inputs
    kw = dict(mno=32, K=20, T_obs=8, T_pred=40, H=128, L=128, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, sx=1.0 / 1400.0, sy=1.0 / 1100.0,
              iters=1, posterior=0)
    d, d16 = Dims(n_scenes=n_windows, **kw), Dims(n_scenes=16, **kw)
    Y16, fut16, pres16, mask, _ = make_inputs(d16, GRID, seed=1)
    Y16 = np.nan_to_num(Y16, nan=0.5)
    rep = n_windows // 16
    h = _lib.Handle(d)
    g = torch.Generator(device="cuda").manual_seed(1)
    Y = torch.as_tensor(Y16, device="cuda").repeat(rep, 1, 1).contiguous()
    fut = torch.as_tensor(fut16, device="cuda").repeat(rep, 1, 1, 1).contiguous()
    pres = torch.as_tensor(pres16, device="cuda").repeat(rep).contiguous()
    mk = torch.as_tensor(mask, device="cuda")
    mos = torch.zeros((n_windows,), device="cuda", dtype=torch.int32)
    score = torch.randn((d.R,), generator=g, device="cuda")
    n, m = d.n_scenes, d.mno
    hz = [10, 20, 30, 40]
    occ = torch.zeros((n, 4) + GRID, device="cuda"); ex = torch.zeros_like(occ)
    hit = torch.zeros((n, m, 4), device="cuda"); viol = torch.zeros_like(hit); off = torch.zeros_like(hit)
    s = torch.cuda.current_stream().cuda_stream
    AT, UNTIL = _lib.OCC_AT, _lib.OCC_UNTIL

    def call(mode, full, form="present"):
        f, p = (fut.data_ptr(), 0) if form == "fut" else (0, pres.data_ptr())
        if not full:
            return lambda: h.occupancy(Y.data_ptr(), f, p, score.data_ptr(), hz, mode, GRID[0], GRID[1], occ.data_ptr(), stream=s)
        return lambda: h.occupancy(Y.data_ptr(), f, p, score.data_ptr(), hz, mode, GRID[0], GRID[1], occ.data_ptr(), ex.data_ptr(),
                                   hit.data_ptr() if (form == "fut" and mode == AT) else 0, viol.data_ptr(), off.data_ptr(), mk.data_ptr(), mos.data_ptr(), s)

    legs = {"at_maps": call(AT, False), "at_all": call(AT, True), "at_all_eval": call(AT, True, "fut"),
            "until_maps": call(UNTIL, False), "until_all": call(UNTIL, True), "until_all_eval": call(UNTIL, True, "fut")}
    r = {"windows": n_windows, "launches": launches}
    for name, mode in (("at", AT), ("until", UNTIL)):
        legs[name + "_all"]()
        torch.cuda.synchronize()
        t_occ, t_exp, t_off = torch_occupancy(torch, Y, pres, score, hz, mode == UNTIL, d)
        r["torch_%s_max_diff" % name] = [round(float((a - b).abs().max()), 7) for a, b in ((t_occ, occ), (t_exp, ex), (t_off, off))]
    r["expected_per_window"] = round(float(ex.sum()) / (n * 4), 2)
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
    for name, until in (("torch_at", False), ("torch_until", True)):      # the torch statement: the whole thing, a few times (it is milliseconds)
        torch_occupancy(torch, Y, pres, score, hz, until, d)
        torch.cuda.synchronize()
        us[name] = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch_occupancy(torch, Y, pres, score, hz, until, d)
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1000.0)
    for k, v in us.items():
        r[k + "_us"] = "%.1f (%.1f - %.1f)" % (float(np.median(v)), min(v), max(v))
    med = {k: float(np.median(v)) for k, v in us.items()}
    y_bytes, map_bytes = d.R * d.T_pred * 8, n * 4 * GRID[0] * GRID[1] * 4
    r["Y_MB"] = round(y_bytes / 1e6, 1)
    # mode AT reads one frame of every row per horizon (a 64-byte sector each), UNTIL the frames before the horizon; the floor counts Y once per horizon
    r["floor_maps_us"] = round((4 * y_bytes + map_bytes) / HBM_BYTES_PER_US, 1)
    r["floor_all_us"] = round((4 * y_bytes + 2 * map_bytes) / HBM_BYTES_PER_US, 1)
    r["at_all_over_torch"] = round(med["at_all"] / med["torch_at"], 4)
    r["until_all_over_torch"] = round(med["until_all"] / med["torch_until"], 4)
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
