"""Evaluation of a checkpoint in the paper's protocol: prior samples of every window of a data set, ranked by IOC score on the
device, errors per horizon of the best-scored sample (top-1), of the best among the top N by score and of the best of all K.

    python -m desire_amd.evaluate --checkpoint save/social_model-400.npz --data_dir data/ --max_num_obj 32 --d_dim 128 \\
        --pred_length 12 [--eval_top 2] [--eval_horizons 3,6,9,12] [--units px|norm|0.2] [--max_windows 500] [--out result.json] \\
        [--generator cvae|rollout] [--nll] [--select nms --nms_radius 20 [--nms_metric final|mean|max] [--nms_horizon 12]] \\
        [--joint [--collision_radius 10]] [--occupancy 64x64 [--occupancy_mode at|until]] [--plan_risk [--collision_radius 10]] \\
        [--modes 6 [--modes_iters 8] [--modes_min_std 1.0] [--modes_seeds nms|score]]

The model flags are train.py's and must be the ones the checkpoint was trained with.  Every video is walked once from its first frame in
steps of one window (no random pointer jumps); the windows are cut and slot-assigned like DataLoader.next_batch does.  Means are taken in
float64 on the host over the agents the loss counts (present at the last observed frame and in at least one target frame); a horizon's
mean runs over those of them with a target frame before it, so every horizon carries its own agent count.
"""
from __future__ import annotations

import argparse
import json
import sys
from typing import Iterator, List, Optional, Tuple

import numpy as np

from .train import build_parser as _train_parser, parse_horizons, split_windows


def build_parser() -> argparse.ArgumentParser:
    p = _train_parser()
    p.description = "DESIRE evaluation on MI355X: ranked ADE / FDE per horizon of a checkpoint (model flags of desire_amd.train)"
    p.add_argument("--checkpoint", type=str, required=True, help="weights archive written by desire_amd.train (social_model-N.npz)")
    p.add_argument("--units", type=str, default="px",
                   help="px (pixels), norm (normalised units) or a factor on pixels, e.g. 0.2 for the paper's 1/5 resolution")
    p.add_argument("--max_windows", type=int, default=0, help="stop after this many windows (0 = all)")
    p.add_argument("--generator", type=str, default="cvae", choices=("cvae", "rollout"),
                   help="what draws the K samples that the IOC stage scores: cvae (the CVAE decoder) or rollout (K rollouts of the reference's Gaussian head "
                        "per agent, desire_rollout_samples; needs a checkpoint trained with --head_loss_weight > 0)")
    p.add_argument("--nll", action="store_true",
                   help="also report the KDE negative log-likelihood of the ground truth under the K samples per horizon (mean over the frames "
                        "and final frame; density per unit^2 of --units, log clipped at -20), with equal weights and with weights softmax(IOC score)")
    p.add_argument("--select", type=str, default="score", choices=("score", "nms"),
                   help="score: the top N by IOC score (default).  nms: also report the best of the N most plausible MUTUALLY DISTINCT futures -- "
                        "score-ordered non-maximum suppression on the device (desire_select_diverse), see --nms_radius")
    p.add_argument("--nms_radius", type=float, default=None, help="--select nms: two futures closer than this many pixels are one (required then)")
    p.add_argument("--nms_metric", type=str, default="final", choices=("final", "mean", "max"),
                   help="--select nms: the distance of two futures -- at the last frame, the mean over the frames, or the largest over the frames")
    p.add_argument("--nms_horizon", type=int, default=None, help="--select nms: frames the distance looks at (default: all of --pred_length)")
    p.add_argument("--joint", action="store_true",
                   help="also report the K samples of a window as K JOINT futures of the scene (desire_joint_metrics): JADE / JFDE per horizon of the "
                        "joint sample with the best summed score and of the best among the top N, and the collision rate of the predicted joint futures "
                        "next to the ground truth's under the same rule, see --collision_radius")
    p.add_argument("--collision_radius", type=float, default=None,
                   help="--joint, --plan_risk: two agents closer than this many pixels in a frame touch (default: 0, nothing touches)")
    p.add_argument("--plan_risk", action="store_true",
                   help="also report the leave-one-out plan risk (desire_plan_risk): per horizon the mean predicted risk of what each agent actually "
                        "did, held against the K joint futures of the others, next to the rate at which it actually came within --collision_radius of "
                        "somebody; a predictor that is calibrated about interactions brings the two close")
    p.add_argument("--occupancy", type=str, default=None, metavar="OHxOW",
                   help="also report the predicted occupancy maps of the score-weighted samples on a grid of OH x OW cells over the frame "
                        "(desire_occupancy): per horizon the mean of -log(max(mass on the ground truth's cell, 1e-6)), the mean mass off the frame and "
                        "the mean expected number of agents in the frame per window")
    p.add_argument("--occupancy_mode", type=str, default="at", choices=("at", "until"),
                   help="--occupancy: the maps at the frame of the horizon (at) or swept over every frame before it (until); the mass on the ground "
                        "truth's cell is always the frame's")
    p.add_argument("--modes", type=int, default=0, metavar="N",
                   help="also report the mixture of N modes per agent that predict_modes hands out (desire_fit_modes): per horizon its negative "
                        "log-likelihood of the ground truth (mean over the frames and final frame; density per unit^2 of --units, log clipped at -20) and "
                        "the ADE / FDE of the most probable mode's mean and of the best mode's mean")
    p.add_argument("--modes_iters", type=int, default=8, help="--modes: the most Lloyd passes (0..32)")
    p.add_argument("--modes_min_std", type=float, default=1.0, help="--modes: the standard deviation in pixels whose square is added to every variance")
    p.add_argument("--modes_seeds", type=str, default="nms", choices=("nms", "score"),
                   help="--modes: the seeds -- nms: the mutually distinct samples first (needs --nms_radius; --nms_metric applies), score: the best-scored")
    p.add_argument("--out", type=str, default=None, help="write the result JSON here (default: standard output only)")
    return p


def iter_batches(data_loader, batch_size: int, max_windows: int = 0) -> Iterator[Tuple[List[np.ndarray], List[int]]]:
    """Every window of every video of the loader once, in order, in batches of batch_size (the last one may be shorter): video v from frame
    0 in steps of seq_length while a window plus the loader's look-ahead frame fits (utils/data_loader.py:190-205 without the random jump).
    Yields (windows [seq_length, max_num_obj, 3], video index of each)."""
    from .data_loader import window_to_slots
    T, xs, ds, n = data_loader.seq_length, [], [], 0
    for v, video in enumerate(data_loader.data):
        idx = 0
        while idx + T < video.shape[0] and not (max_windows and n >= max_windows):
            xs.append(window_to_slots(video[idx:idx + T + 1], T, data_loader.max_num_obj)[0])
            ds.append(v)
            idx += T
            n += 1
            if len(xs) == batch_size:
                yield xs, ds
                xs, ds = [], []
    if xs:
        yield xs, ds


def evaluate(args, data_loader=None, model=None) -> dict:
    """Runs the walk; returns the result dict main() prints.  `data_loader` / `model` may be injected (tests)."""
    from .data_loader import DataLoader
    from .model import DESIREModel, default_top
    from ._lib import KDE_LOG_FLOOR
    if args.pred_length is None:
        args.pred_length = args.seq_length
    t_obs, t_pred = int(args.seq_length), int(args.pred_length)
    if data_loader is None:
        data_loader = DataLoader(args.batch_size, t_obs + t_pred, args.max_num_obj, args.leave_dataset, preprocess=False,
                                 data_dir=args.data_dir, traj_bin=args.traj_bin, fix_id0=args.fix_id0)
    if model is None:
        model = DESIREModel.restore(args, args.checkpoint)
    K = int(args.num_samples)
    generator = str(getattr(args, "generator", "cvae") or "cvae")
    top = int(args.eval_top or default_top(K))
    hz = parse_horizons(args.eval_horizons, t_pred)
    units = args.units if args.units in ("px", "norm") else float(args.units)
    names = ("top1", "best_of_top", "best_of_K")
    sums = {k: np.zeros((len(hz), 2), np.float64) for k in names}
    agents = np.zeros(len(hz), np.int64)
    mean_k, n_all, n_windows = np.zeros(2, np.float64), 0, 0
    nll = bool(getattr(args, "nll", False))
    nll_sums = {k: np.zeros((len(hz), 2), np.float64) for k in ("uniform", "score_weighted")}
    nll_floored, nll_frames = 0, 0
    nms = str(getattr(args, "select", "score") or "score") == "nms"
    if nms and getattr(args, "nms_radius", None) is None:
        raise ValueError("--select nms needs --nms_radius (pixels)")
    nms_kw = dict(select="nms", nms_radius=args.nms_radius, nms_metric=args.nms_metric, nms_horizon=args.nms_horizon) if nms else {}
    nms_sums, nms_count, nms_present = np.zeros((len(hz), 2), np.float64), 0, 0
    joint = bool(getattr(args, "joint", False))
    j_sums, j_windows = np.zeros((len(hz), 4), np.float64), np.zeros(len(hz), np.int64)
    j_cnt = {k: np.zeros((len(hz), 2), np.int64) for k in ("top1", "all_K", "ground_truth")}      # (touching, taking part)
    occ_grid = parse_grid(getattr(args, "occupancy", None))
    occ_mode = str(getattr(args, "occupancy_mode", "at") or "at")
    o_nll, o_off, o_exp = np.zeros(len(hz), np.float64), np.zeros(len(hz), np.float64), np.zeros(len(hz), np.float64)
    o_at = np.zeros(len(hz), np.int64)                                                           # agents counted at the horizon's own frame
    plan_risk = bool(getattr(args, "plan_risk", False))
    p_pred, p_act, p_agents = np.zeros(len(hz), np.float64), np.zeros(len(hz), np.float64), np.zeros(len(hz), np.int64)
    n_modes = int(getattr(args, "modes", 0) or 0)
    if n_modes and str(getattr(args, "modes_seeds", "nms")) == "nms" and getattr(args, "nms_radius", None) is None:
        raise ValueError("--modes with --modes_seeds nms needs --nms_radius (pixels)")
    m_sums = {k: np.zeros((len(hz), 2), np.float64) for k in ("nll", "top1", "best")}
    m_passes, m_present = 0, 0
    for xs, _ in iter_batches(data_loader, int(args.batch_size), int(args.max_windows or 0)):
        past, fut = split_windows(xs, t_obs)
        # --device_rng: a window's noise is a function of its running index, so the result does not depend on --batch_size
        gen = {} if generator == "cvae" else {"generator": generator}
        model.predict(past, top=top, seed=args.seed, device_rng=bool(getattr(args, "device_rng", False)), window_base=n_windows, **gen)
        Y, score = model.final_output, model.final_states
        ranked = model.evaluate_ranked(Y, score, fut, top=top, horizons=hz, units=units).astype(np.float64)
        best = model.evaluate_ranked(Y, score, fut, top=K, horizons=hz, units=units).astype(np.float64)
        ev = model.evaluate(Y, fut).astype(np.float64)
        if nms:
            distinct, kept = model.evaluate_ranked(Y, score, fut, top=top, horizons=hz, units=units, return_count=True, **nms_kw)
            distinct = distinct.astype(np.float64)
        if nll:
            nll_u, fr = model.evaluate_nll(Y, score, fut, horizons=hz, units=units, log_floor=KDE_LOG_FLOOR, return_frames=True)
            nll_w = model.evaluate_nll(Y, score, fut, horizons=hz, units=units, weighted=True, log_floor=KDE_LOG_FLOOR)
        if joint:                                    # per window: the call counts by the targets' ids alone
            jm = model.evaluate_joint(Y, score, fut, top=top, horizons=hz, units=units, collision_radius=getattr(args, "collision_radius", None))
            cnt = jm["cnt"].astype(np.int64)
            takes = cnt[:, 0, :, 1] > 0                                                          # [n, n_h]
            j_sums += np.where(takes[:, :, None], jm["out"].astype(np.float64), 0.0).sum(0)
            j_windows += takes.sum(0)
            j_cnt["top1"] += cnt[np.arange(cnt.shape[0]), jm["order"][:, 0]].sum(0)
            j_cnt["all_K"] += cnt[:, :K].sum((0, 1))
            j_cnt["ground_truth"] += cnt[:, K].sum(0)
        if plan_risk:                                # sums over the agents taking part, so that the batches weigh as their agents do
            pm = model.evaluate_plan_risk(Y, score, fut, float(getattr(args, "collision_radius", None) or 0.0), horizons=hz)
            p_pred += pm["predicted"] * pm["agents"]
            p_act += pm["actual"] * pm["agents"]
            p_agents += pm["agents"]
        if occ_grid:
            om = model.evaluate_occupancy(Y, score, fut, occ_grid, horizons=hz, mode=occ_mode)
            o_hit = om["hit"] if occ_mode == "at" else model.evaluate_occupancy(Y, score, fut, occ_grid, horizons=hz, mode="at")["hit"]
            o_exp += om["expected"].astype(np.float64).sum((0, 2, 3))
        if n_modes:
            mm = model.evaluate_modes(Y, score, fut, modes=n_modes, seeds=str(getattr(args, "modes_seeds", "nms")), nms_radius=getattr(args, "nms_radius", None),
                                      nms_metric=str(getattr(args, "nms_metric", "final")), iters=int(getattr(args, "modes_iters", 8)),
                                      min_std=float(getattr(args, "modes_min_std", 1.0)), horizons=hz, units=units, log_floor=KDE_LOG_FLOOR)
        pw, fw = np.stack(past), np.stack(fut)
        mno = ranked.shape[0] // pw.shape[0]
        valid = np.zeros((pw.shape[0], mno), bool)
        valid[:, :pw.shape[2]] = pw[:, -1, :, 0] != 0
        seen = np.zeros((pw.shape[0], t_pred, mno), bool)
        seen[:, :, :pw.shape[2]] = fw[:, :, :, 0] != 0
        for i, h in enumerate(hz):
            c = (valid & seen[:, :h].any(1)).reshape(-1)
            agents[i] += int(c.sum())
            sums["top1"][i] += ranked[c, i, 0:2].sum(0)
            sums["best_of_top"][i] += ranked[c, i, 2:4].sum(0)
            sums["best_of_K"][i] += best[c, i, 2:4].sum(0)
            if nms:
                nms_sums[i] += distinct[c, i, 2:4].sum(0)
            if occ_grid:
                at = (valid & seen[:, h - 1]).reshape(-1)
                o_at[i] += int(at.sum())
                o_nll[i] += float(-np.log(np.maximum(o_hit.reshape(-1, len(hz))[at, i].astype(np.float64), 1e-6)).sum())
                o_off[i] += float(om["off"].reshape(-1, len(hz))[c, i].astype(np.float64).sum())
            if n_modes:
                for k in m_sums:
                    m_sums[k][i] += mm[k][c, i].astype(np.float64).sum(0)
            if nll:
                nll_sums["uniform"][i] += nll_u[c, i].astype(np.float64).sum(0)
                nll_sums["score_weighted"][i] += nll_w[c, i].astype(np.float64).sum(0)
        c = (valid & seen.any(1)).reshape(-1)
        mean_k += ev[c, 0:2].sum(0)
        if nms:                                      # samples kept per agent present at the last observed frame
            nms_count += int(kept[valid.reshape(-1)].sum())
            nms_present += int(valid.sum())
        n_all += int(c.sum())
        if n_modes:                                  # passes per agent present at the last observed frame
            m_passes += int(mm["passes"][valid.reshape(-1)].sum())
            m_present += int(valid.sum())
        if nll:                                      # the counted frames of those agents, and how many of them sit on the floor (equal weights)
            cf = (valid[:, None, :] & seen).transpose(0, 2, 1).reshape(fr.shape)
            nll_frames += int(cf.sum())
            nll_floored += int((cf & (fr <= np.float32(KDE_LOG_FLOOR))).sum())
        n_windows += len(xs)
    res = {"checkpoint": args.checkpoint, "generator": generator, "units": args.units, "seed": int(args.seed), "K": K, "top": top, "horizons": hz,
           "windows": n_windows, "agents": [int(a) for a in agents]}
    for k in names:
        m = sums[k] / np.maximum(agents, 1)[:, None]
        res[k] = {"ade": [float(v) for v in m[:, 0]], "fde": [float(v) for v in m[:, 1]]}
    # mean-of-K comes from the ADE / FDE harness: normalised units, the whole prediction
    res["mean_of_K"] = {"ade": float(mean_k[0] / max(n_all, 1)), "fde": float(mean_k[1] / max(n_all, 1)), "units": "norm", "horizon": t_pred,
                        "agents": n_all}
    if nms:
        m = nms_sums / np.maximum(agents, 1)[:, None]
        res["select"] = {"mode": "nms", "radius_px": float(args.nms_radius), "metric": str(args.nms_metric),
                         "horizon": int(args.nms_horizon or t_pred), "mean_count": float(nms_count / max(nms_present, 1)), "present_agents": nms_present,
                         "best_of_top_distinct": {"ade": [float(v) for v in m[:, 0]], "fde": [float(v) for v in m[:, 1]]}}
    if nll:
        res["kde_nll"] = {"log_floor": KDE_LOG_FLOOR}
        for k in ("uniform", "score_weighted"):
            m = nll_sums[k] / np.maximum(agents, 1)[:, None]
            res["kde_nll"][k] = {"mean": [float(v) for v in m[:, 0]], "final": [float(v) for v in m[:, 1]]}
        res["kde_nll"].update({"floored_frames": nll_floored, "frames": nll_frames})
    if joint:
        m = j_sums / np.maximum(j_windows, 1)[:, None]
        rate = {k: [float(v[i, 0] / max(int(v[i, 1]), 1)) for i in range(len(hz))] for k, v in j_cnt.items()}
        res["joint"] = {"collision_radius_px": float(getattr(args, "collision_radius", None) or 0.0), "windows": [int(v) for v in j_windows],
                        "top1": {"jade": [float(v) for v in m[:, 0]], "jfde": [float(v) for v in m[:, 1]]},
                        "best_of_top": {"jade": [float(v) for v in m[:, 2]], "jfde": [float(v) for v in m[:, 3]]},
                        "collision_rate": rate, "slots": [int(v) for v in j_cnt["ground_truth"][:, 1]]}
    if plan_risk:
        res["plan_risk"] = {"collision_radius_px": float(getattr(args, "collision_radius", None) or 0.0), "agents": [int(v) for v in p_agents],
                            "predicted_risk": [float(p_pred[i] / max(int(p_agents[i]), 1)) for i in range(len(hz))],
                            "actual_rate": [float(p_act[i] / max(int(p_agents[i]), 1)) for i in range(len(hz))]}
    if occ_grid:
        res["occupancy"] = {"grid": [int(occ_grid[0]), int(occ_grid[1])], "mode": occ_mode, "weights": "score", "hit_floor": 1e-6,
                            "agents_at_frame": [int(v) for v in o_at],
                            "hit_nll": [float(o_nll[i] / max(int(o_at[i]), 1)) for i in range(len(hz))],
                            "off_mass": [float(o_off[i] / max(int(agents[i]), 1)) for i in range(len(hz))],
                            "expected_in_frame": [float(o_exp[i] / max(n_windows, 1)) for i in range(len(hz))]}
    if n_modes:
        m = {k: v / np.maximum(agents, 1)[:, None] for k, v in m_sums.items()}
        res["modes"] = {"n": n_modes, "seeds": str(getattr(args, "modes_seeds", "nms")), "iters": int(getattr(args, "modes_iters", 8)),
                        "min_std_px": float(getattr(args, "modes_min_std", 1.0)), "log_floor": KDE_LOG_FLOOR,
                        "mean_passes": float(m_passes / max(m_present, 1)),
                        "nll": {"mean": [float(v) for v in m["nll"][:, 0]], "final": [float(v) for v in m["nll"][:, 1]]},
                        "top1": {"ade": [float(v) for v in m["top1"][:, 0]], "fde": [float(v) for v in m["top1"][:, 1]]},
                        "best": {"ade": [float(v) for v in m["best"][:, 0]], "fde": [float(v) for v in m["best"][:, 1]]}}
    return res


def parse_grid(text) -> Optional[Tuple[int, int]]:
    """--occupancy OHxOW -> (OH, OW); None without the flag."""
    if not text:
        return None
    parts = str(text).lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts) or not all(1 <= int(p) <= 1024 for p in parts):
        raise ValueError("--occupancy takes OHxOW with both sides in 1..1024, e.g. 64x64, got %r" % (text,))
    return int(parts[0]), int(parts[1])


def main(argv: Optional[List[str]] = None) -> None:
    args = build_parser().parse_args(argv)
    res = evaluate(args)
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    sys.stdout.flush()


if __name__ == "__main__":
    main()
