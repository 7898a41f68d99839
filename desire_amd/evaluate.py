"""Evaluation of a checkpoint in the paper's protocol: prior samples of every window of a data set, ranked by IOC score on the
device, errors per horizon of the best-scored sample (top-1), of the best among the top N by score and of the best of all K.

    python -m desire_amd.evaluate --checkpoint save/social_model-400.npz --data_dir data/ --max_num_obj 32 --d_dim 128 \\
        --pred_length 12 [--eval_top 2] [--eval_horizons 3,6,9,12] [--units px|norm|0.2] [--max_windows 500] [--out result.json] \\
        [--generator cvae|rollout] [--nll] [--select nms --nms_radius 20 [--nms_metric final|mean|max] [--nms_horizon 12]] \\
        [--joint [--collision_radius 10]] [--occupancy 64x64 [--occupancy_mode at|until]] [--plan_risk [--collision_radius 10]] \\
        [--modes 6 [--modes_iters 8] [--modes_min_std 1.0] [--modes_seeds nms|score]] \\
        [--joint_modes 6 [--joint_modes_iters 8] [--joint_modes_min_std 1.0] [--joint_modes_seeds nms|score] [--joint_radius 20]]

The model flags are train.py's and must be the ones the checkpoint was trained with.  Every video is walked once from its first frame in
steps of one window (no random pointer jumps); the windows are cut and slot-assigned like DataLoader.next_batch does.  Means are taken in
float64 on the host over the agents the loss counts (present at the last observed frame and in at least one target frame); a horizon's
mean runs over those of them with a target frame before it, so every horizon carries its own agent count.

Every report is one block below (_Ranked and one class per optional flag): __init__(args, hz, run) reads its flags, update(model, Y, score, fut,
masks) makes its model calls for a batch and adds to its float64 / int64 sums, result() returns its part of the result.  evaluate() only walks the
batches, computes the agent masks they share (_masks) and asks the enabled blocks in the order of the result's keys.
"""
from __future__ import annotations

import argparse
import json
import sys
from types import SimpleNamespace
from typing import Iterator, List, Optional, Tuple

import numpy as np

from ._lib import KDE_LOG_FLOOR
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
    # (--collision_radius comes with the training flags, where --report_joint reads it: here it serves --joint and --plan_risk)
    p.add_argument("--joint_select", type=str, default=None, choices=("nms",),
                   help="--joint: also report the best of the N most plausible MUTUALLY DISTINCT joint futures -- score-ordered non-maximum suppression "
                        "of the K joint samples of a window on the device (desire_select_worlds), see --joint_radius")
    p.add_argument("--joint_radius", type=float, default=None, help="--joint_select nms: two joint futures closer than this many pixels are one (required then)")
    p.add_argument("--joint_metric", type=str, default="final", choices=("final", "mean", "max"),
                   help="--joint_select nms: the distance of an agent's two futures, as --nms_metric")
    p.add_argument("--joint_reduce", type=str, default="mean", choices=("mean", "all"),
                   help="--joint_select nms: two joint futures are one when the mean over the agents of that distance is below the radius (mean), or when "
                        "every agent's is (all)")
    p.add_argument("--joint_horizon", type=int, default=None, help="--joint_select nms: frames the distance looks at (default: all of --pred_length)")
    p.add_argument("--collision_penalty", type=float, default=0.0,
                   help="--joint_select nms: rank the joint futures by joint score minus this much per agent that collides (--collision_radius) before "
                        "the last horizon")
    p.add_argument("--plan_risk", action="store_true",
                   help="also report the leave-one-out plan risk (desire_plan_risk): per horizon the mean predicted risk of what each agent actually "
                        "did, held against the K joint futures of the others, next to the rate at which it actually came within --collision_radius of "
                        "somebody; a predictor that is calibrated about interactions brings the two close")
    p.add_argument("--plan_risk_sigma", type=float, default=None, metavar="PX",
                   help="--plan_risk: also report the risk GIVEN what the agent did (desire_plan_risk_cond): the K joint futures reweighted by how close "
                        "their own sample of the agent came to its recorded future, a Gaussian kernel of this many pixels RMS per frame; next to it the "
                        "mean effective number of joint futures that carry the answer")
    p.add_argument("--plan_risk_cond_horizon", type=int, default=None, metavar="T",
                   help="--plan_risk_sigma: frames the reweighting compares (default: all of --pred_length)")
    p.add_argument("--occupancy", type=str, default=None, metavar="OHxOW",
                   help="also report the predicted occupancy maps of the score-weighted samples on a grid of OH x OW cells over the frame "
                        "(desire_occupancy): per horizon the mean of -log(max(mass on the ground truth's cell, 1e-6)), the mean mass off the frame and "
                        "the mean expected number of agents in the frame per window")
    p.add_argument("--occupancy_mode", type=str, default="at", choices=("at", "until"),
                   help="--occupancy: the maps at the frame of the horizon (at) or swept over every frame before it (until); the mass on the ground "
                        "truth's cell is always the frame's")
    p.add_argument("--offroad", type=str, default=None, metavar="MASKFILE",
                   help="also report how far the K joint futures leave the road (desire_offroad_loss): MASKFILE is the .npz of train.py's "
                        "--scene_masks (one [Mh, Mw] uint8 traversability mask per video, keyed by the video directory relative to --data_dir); the "
                        "share of predicted positions on a cell off the road per joint future, the same of the ground truth, and the mean penalty "
                        "at --offroad_scale pixels (the training flag; default here: one cell of the mask, the wider side)")
    p.add_argument("--modes", type=int, default=0, metavar="N",
                   help="also report the mixture of N modes per agent that predict_modes hands out (desire_fit_modes): per horizon its negative "
                        "log-likelihood of the ground truth (mean over the frames and final frame; density per unit^2 of --units, log clipped at -20) and "
                        "the ADE / FDE of the most probable mode's mean and of the best mode's mean")
    p.add_argument("--modes_iters", type=int, default=8, help="--modes: the most Lloyd passes (0..32)")
    p.add_argument("--modes_min_std", type=float, default=1.0, help="--modes: the standard deviation in pixels whose square is added to every variance")
    p.add_argument("--modes_seeds", type=str, default="nms", choices=("nms", "score"),
                   help="--modes: the seeds -- nms: the mutually distinct samples first (needs --nms_radius; --nms_metric applies), score: the best-scored")
    p.add_argument("--joint_modes", type=int, default=0, metavar="N",
                   help="also report the mixture of N SCENE modes per window that predict_scene_modes hands out (desire_fit_scene_modes): per horizon "
                        "its negative joint log-likelihood of the ground truth per agent (mean over the frames and final frame; density per unit^2 of "
                        "--units, log clipped at -20) and the JADE / JFDE of the most probable mode's means and of the best mode's means")
    p.add_argument("--joint_modes_iters", type=int, default=8, help="--joint_modes: the most Lloyd passes (0..32)")
    p.add_argument("--joint_modes_min_std", type=float, default=1.0,
                   help="--joint_modes: the standard deviation in pixels whose square is added to every variance")
    p.add_argument("--joint_modes_seeds", type=str, default="nms", choices=("nms", "score"),
                   help="--joint_modes: the seeds -- nms: the mutually distinct joint futures first (needs --joint_radius; --joint_metric, --joint_reduce, "
                        "--joint_horizon, --collision_radius and --collision_penalty apply), score: the joint futures with the best summed score")
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


def _per_horizon(m, a: str, b: str) -> dict:
    """{a: column 0, b: column 1} of a [n_h, >= 2] array of means, as the result's lists of floats."""
    return {a: [float(v) for v in m[:, 0]], b: [float(v) for v in m[:, 1]]}


class _Run:
    """The settings every block reads and the counts they divide by: windows walked, and per horizon the agents the loss counts (present at the
    last observed frame and in a target frame before the horizon).  Its result is the head of the result dict."""

    def __init__(self, args, hz, generator: str, K: int, top: int, t_pred: int):
        self.args, self.hz, self.generator, self.K, self.top, self.t_pred = args, hz, generator, K, top, t_pred
        self.units = args.units if args.units in ("px", "norm") else float(args.units)
        self.agents, self.windows = np.zeros(len(hz), np.int64), 0

    def update(self, model, Y, score, fut, masks):
        for i, c in enumerate(masks.c):
            self.agents[i] += int(c.sum())
        self.windows += masks.valid.shape[0]

    def mean(self, sums):
        """Per-horizon sums [n_h, ...] over the counted agents -> their means."""
        return sums / np.maximum(self.agents, 1)[:, None]

    def result(self) -> dict:
        return {"checkpoint": self.args.checkpoint, "generator": self.generator, "units": self.args.units, "seed": int(self.args.seed), "K": self.K,
                "top": self.top, "horizons": self.hz, "windows": self.windows, "agents": [int(a) for a in self.agents]}


class _Ranked:
    """top1 / best_of_top / best_of_K: the errors of the best-scored sample, of the best among the top N by score and of the best of all K; and
    mean_of_K from the ADE / FDE harness (normalised units, the whole prediction)."""
    on = True

    def __init__(self, args, hz, run):
        self.run = run
        self.sums = {k: np.zeros((len(hz), 2), np.float64) for k in ("top1", "best_of_top", "best_of_K")}
        self.mean_k, self.n_all = np.zeros(2, np.float64), 0

    def update(self, model, Y, score, fut, masks):
        r = self.run
        ranked = model.evaluate_ranked(Y, score, fut, top=r.top, horizons=r.hz, units=r.units).astype(np.float64)
        best = model.evaluate_ranked(Y, score, fut, top=r.K, horizons=r.hz, units=r.units).astype(np.float64)
        ev = model.evaluate(Y, fut).astype(np.float64)
        for i, c in enumerate(masks.c):
            self.sums["top1"][i] += ranked[c, i, 0:2].sum(0)
            self.sums["best_of_top"][i] += ranked[c, i, 2:4].sum(0)
            self.sums["best_of_K"][i] += best[c, i, 2:4].sum(0)
        self.mean_k += ev[masks.all, 0:2].sum(0)
        self.n_all += int(masks.all.sum())

    def result(self) -> dict:
        res = {k: _per_horizon(self.run.mean(v), "ade", "fde") for k, v in self.sums.items()}
        res["mean_of_K"] = {"ade": float(self.mean_k[0] / max(self.n_all, 1)), "fde": float(self.mean_k[1] / max(self.n_all, 1)), "units": "norm",
                            "horizon": self.run.t_pred, "agents": self.n_all}
        return res


class _Select:
    """--select nms: the best of the N most plausible mutually distinct futures, and the samples kept per agent present at the last observed frame."""

    def __init__(self, args, hz, run):
        self.on = str(getattr(args, "select", "score") or "score") == "nms"
        if self.on and getattr(args, "nms_radius", None) is None:
            raise ValueError("--select nms needs --nms_radius (pixels)")
        self.args, self.run = args, run
        self.sums, self.count, self.present = np.zeros((len(hz), 2), np.float64), 0, 0

    def update(self, model, Y, score, fut, masks):
        a, r = self.args, self.run
        distinct, kept = model.evaluate_ranked(Y, score, fut, top=r.top, horizons=r.hz, units=r.units, return_count=True, select="nms",
                                               nms_radius=a.nms_radius, nms_metric=a.nms_metric, nms_horizon=a.nms_horizon)
        distinct = distinct.astype(np.float64)
        for i, c in enumerate(masks.c):
            self.sums[i] += distinct[c, i, 2:4].sum(0)
        self.count += int(kept[masks.valid.reshape(-1)].sum())
        self.present += int(masks.valid.sum())

    def result(self) -> dict:
        a = self.args
        return {"select": {"mode": "nms", "radius_px": float(a.nms_radius), "metric": str(a.nms_metric), "horizon": int(a.nms_horizon or self.run.t_pred),
                           "mean_count": float(self.count / max(self.present, 1)), "present_agents": self.present,
                           "best_of_top_distinct": _per_horizon(self.run.mean(self.sums), "ade", "fde")}}


class _KdeNll:
    """--nll: the KDE negative log-likelihood of the ground truth with equal weights and with weights softmax(score), and of the counted frames of
    the counted agents how many sit on the floor (equal weights)."""

    def __init__(self, args, hz, run):
        self.on = bool(getattr(args, "nll", False))
        self.run = run
        self.sums = {k: np.zeros((len(hz), 2), np.float64) for k in ("uniform", "score_weighted")}
        self.floored, self.frames = 0, 0

    def update(self, model, Y, score, fut, masks):
        r = self.run
        by = {}
        by["uniform"], fr = model.evaluate_nll(Y, score, fut, horizons=r.hz, units=r.units, log_floor=KDE_LOG_FLOOR, return_frames=True)
        by["score_weighted"] = model.evaluate_nll(Y, score, fut, horizons=r.hz, units=r.units, weighted=True, log_floor=KDE_LOG_FLOOR)
        for i, c in enumerate(masks.c):
            for k, v in by.items():
                self.sums[k][i] += v[c, i].astype(np.float64).sum(0)
        cf = (masks.valid[:, None, :] & masks.seen).transpose(0, 2, 1).reshape(fr.shape)
        self.frames += int(cf.sum())
        self.floored += int((cf & (fr <= np.float32(KDE_LOG_FLOOR))).sum())

    def result(self) -> dict:
        res = {"log_floor": KDE_LOG_FLOOR}
        for k, v in self.sums.items():
            res[k] = _per_horizon(self.run.mean(v), "mean", "final")
        res.update({"floored_frames": self.floored, "frames": self.frames})
        return {"kde_nll": res}


class _Joint:
    """--joint: the K samples of a window as K joint futures -- JADE / JFDE over the windows with an agent taking part, and the collision rates.
    Per window: the call counts by the targets' ids alone.  --joint_select nms: the same call also puts the joint samples through the
    non-maximum suppression of worlds, and the block gains its parameters, the worlds kept per window and the best of the top N distinct ones."""

    def __init__(self, args, hz, run):
        self.on = bool(getattr(args, "joint", False))
        self.radius, self.run = getattr(args, "collision_radius", None), run
        self.nms = getattr(args, "joint_select", None) == "nms"
        if self.on and self.nms and getattr(args, "joint_radius", None) is None:
            raise ValueError("--joint_select nms needs --joint_radius (pixels)")
        self.worlds = {}
        if self.nms:
            self.worlds = dict(select="worlds", worlds_radius=args.joint_radius, worlds_metric=str(getattr(args, "joint_metric", "final")),
                               worlds_reduce=str(getattr(args, "joint_reduce", "mean")), worlds_horizon=getattr(args, "joint_horizon", None),
                               collision_penalty=float(getattr(args, "collision_penalty", 0.0) or 0.0))
        self.distinct, self.kept = np.zeros((len(hz), 2), np.float64), 0
        self.sums, self.windows = np.zeros((len(hz), 4), np.float64), np.zeros(len(hz), np.int64)
        self.cnt = {k: np.zeros((len(hz), 2), np.int64) for k in ("top1", "all_K", "ground_truth")}      # (touching, taking part)

    def update(self, model, Y, score, fut, masks):
        r = self.run
        jm = model.evaluate_joint(Y, score, fut, top=r.top, horizons=r.hz, units=r.units, collision_radius=self.radius, **self.worlds)
        cnt = jm["cnt"].astype(np.int64)
        takes = cnt[:, 0, :, 1] > 0                                                              # [n, n_h]
        if self.nms:
            self.distinct += np.where(takes[:, :, None], jm["out_distinct"].astype(np.float64), 0.0).sum(0)
            self.kept += int(jm["wcount"][takes[:, -1]].sum())
        self.sums += np.where(takes[:, :, None], jm["out"].astype(np.float64), 0.0).sum(0)
        self.windows += takes.sum(0)
        self.cnt["top1"] += cnt[np.arange(cnt.shape[0]), jm["order"][:, 0]].sum(0)
        self.cnt["all_K"] += cnt[:, :r.K].sum((0, 1))
        self.cnt["ground_truth"] += cnt[:, r.K].sum(0)

    def result(self) -> dict:
        m = self.sums / np.maximum(self.windows, 1)[:, None]
        rate = {k: [float(v[i, 0] / max(int(v[i, 1]), 1)) for i in range(len(self.run.hz))] for k, v in self.cnt.items()}
        res = {"collision_radius_px": float(self.radius or 0.0), "windows": [int(v) for v in self.windows],
               "top1": _per_horizon(m[:, 0:2], "jade", "jfde"), "best_of_top": _per_horizon(m[:, 2:4], "jade", "jfde"),
               "collision_rate": rate, "slots": [int(v) for v in self.cnt["ground_truth"][:, 1]]}
        if self.nms:
            w = self.worlds
            res["select"] = {"mode": "nms", "radius_px": float(w["worlds_radius"]), "metric": w["worlds_metric"], "reduce": w["worlds_reduce"],
                             "horizon": int(w["worlds_horizon"] or self.run.t_pred), "collision_penalty": w["collision_penalty"],
                             "mean_count": float(self.kept / max(int(self.windows[-1]), 1)),
                             "best_of_top_distinct": _per_horizon(self.distinct / np.maximum(self.windows, 1)[:, None], "jade", "jfde")}
        return {"joint": res}


class _PlanRisk:
    """--plan_risk: the leave-one-out plan risk, summed over the agents taking part so that the batches weigh as their agents do."""

    def __init__(self, args, hz, run):
        self.on = bool(getattr(args, "plan_risk", False))
        self.radius, self.run = float(getattr(args, "collision_radius", None) or 0.0), run
        self.pred, self.act, self.agents = np.zeros(len(hz), np.float64), np.zeros(len(hz), np.float64), np.zeros(len(hz), np.int64)
        self.sigma, self.t_cond = getattr(args, "plan_risk_sigma", None), getattr(args, "plan_risk_cond_horizon", None)
        self.given, self.ess = np.zeros(len(hz), np.float64), np.zeros(len(hz), np.float64)

    def update(self, model, Y, score, fut, masks):
        if self.sigma is None:
            pm = model.evaluate_plan_risk(Y, score, fut, self.radius, horizons=self.run.hz)
        else:
            pm = model.evaluate_plan_risk(Y, score, fut, self.radius, horizons=self.run.hz, condition=True, condition_sigma=self.sigma,
                                          condition_horizon=self.t_cond)
            self.given += pm["predicted_given"] * pm["agents"]
            self.ess += pm["ess_mean"] * pm["agents"]
        self.pred += pm["predicted"] * pm["agents"]
        self.act += pm["actual"] * pm["agents"]
        self.agents += pm["agents"]

    def result(self) -> dict:
        rate = lambda s: [float(s[i] / max(int(self.agents[i]), 1)) for i in range(len(self.run.hz))]
        res = {"collision_radius_px": self.radius, "agents": [int(v) for v in self.agents], "predicted_risk": rate(self.pred), "actual_rate": rate(self.act)}
        if self.sigma is not None:
            res.update({"predicted_risk_given": rate(self.given), "ess": rate(self.ess)})
        return {"plan_risk": res}


class _Occupancy:
    """--occupancy OHxOW: the occupancy maps of the score-weighted samples.  The mass on the ground truth's cell is always the frame's (mode "at"),
    over the agents counted at the horizon's own frame; --occupancy_mode until asks for it in a second call."""

    def __init__(self, args, hz, run):
        self.grid = parse_grid(getattr(args, "occupancy", None))
        self.on = bool(self.grid)
        self.mode, self.run = str(getattr(args, "occupancy_mode", "at") or "at"), run
        self.nll, self.off, self.exp = np.zeros(len(hz), np.float64), np.zeros(len(hz), np.float64), np.zeros(len(hz), np.float64)
        self.at = np.zeros(len(hz), np.int64)

    def update(self, model, Y, score, fut, masks):
        hz = self.run.hz
        om = model.evaluate_occupancy(Y, score, fut, self.grid, horizons=hz, mode=self.mode)
        hit = om["hit"] if self.mode == "at" else model.evaluate_occupancy(Y, score, fut, self.grid, horizons=hz, mode="at")["hit"]
        self.exp += om["expected"].astype(np.float64).sum((0, 2, 3))
        for i, (c, at) in enumerate(zip(masks.c, masks.at)):
            self.at[i] += int(at.sum())
            self.nll[i] += float(-np.log(np.maximum(hit.reshape(-1, len(hz))[at, i].astype(np.float64), 1e-6)).sum())
            self.off[i] += float(om["off"].reshape(-1, len(hz))[c, i].astype(np.float64).sum())

    def result(self) -> dict:
        r, nh = self.run, len(self.run.hz)
        return {"occupancy": {"grid": [int(self.grid[0]), int(self.grid[1])], "mode": self.mode, "weights": "score", "hit_floor": 1e-6,
                              "agents_at_frame": [int(v) for v in self.at],
                              "hit_nll": [float(self.nll[i] / max(int(self.at[i]), 1)) for i in range(nh)],
                              "off_mass": [float(self.off[i] / max(int(r.agents[i]), 1)) for i in range(nh)],
                              "expected_in_frame": [float(self.exp[i] / max(r.windows, 1)) for i in range(nh)]}}


class _Offroad:
    """--offroad MASKFILE: the off-road rate of the K joint futures and of the ground truth against each video's traversability mask, and the mean
    penalty (the training term of --offroad_weight, window by window, weighted by the window's counted frames)."""

    def __init__(self, args, hz, run):
        self.path = getattr(args, "offroad", None)
        self.on = bool(self.path)
        self.scale, self.run, self.args = getattr(args, "offroad_scale", None), run, args
        if self.on and self.scale is not None and not (np.isfinite(float(self.scale)) and float(self.scale) > 0.0):
            raise ValueError("--offroad_scale must be finite and > 0 (pixels), got %r" % (self.scale,))
        self.masks, self.frames, self.count, self.gt, self.best, self.pen, self.gt_pen, self.batches = None, 0, 0, 0, 0.0, 0.0, 0.0, 0

    def update(self, model, Y, score, fut, masks):
        if self.masks is None:
            from .train import load_scene_masks, scene_image_keys
            self.masks, self.of_video = load_scene_masks(self.path, scene_image_keys(masks.loader, self.args.data_dir))
            if self.scale is None:
                d = model._handle(len(fut), False).dims
                self.scale = max((1.0 / d.sx) / self.masks.shape[2], (1.0 / d.sy) / self.masks.shape[1])
        r = model.evaluate_offroad(Y, score, fut, self.masks, self.of_video[np.asarray(masks.video, np.int64)], float(self.scale))
        self.frames += int(r["frames"].sum())
        self.count += int(r["count"].sum())
        self.gt += int(r["gt_count"].sum())
        self.best += float(r["count"].min(1).sum())
        w = int(r["frames"].sum())
        self.pen, self.gt_pen, self.batches = self.pen + r["penalty"] * w, self.gt_pen + r["gt_penalty"] * w, self.batches + w

    def result(self) -> dict:
        f = max(self.frames, 1)
        return {"offroad": {"masks": self.path, "scale_px": float(self.scale) if self.scale is not None else None, "frames": int(self.frames),
                            "rate_mean_of_K": float(self.count / (f * self.run.K)), "rate_best_of_K": float(self.best / f),
                            "rate_ground_truth": float(self.gt / f), "penalty": float(self.pen / max(self.batches, 1)),
                            "penalty_ground_truth": float(self.gt_pen / max(self.batches, 1))}}


class _Modes:
    """--modes N: the mixture of N modes per agent -- its likelihood of the ground truth, the errors of the most probable and of the best mode's
    mean, and the Lloyd passes per agent present at the last observed frame."""

    def __init__(self, args, hz, run):
        self.n = int(getattr(args, "modes", 0) or 0)
        self.on = bool(self.n)
        self.seeds, self.radius = str(getattr(args, "modes_seeds", "nms")), getattr(args, "nms_radius", None)
        if self.on and self.seeds == "nms" and self.radius is None:
            raise ValueError("--modes with --modes_seeds nms needs --nms_radius (pixels)")
        self.metric, self.iters = str(getattr(args, "nms_metric", "final")), int(getattr(args, "modes_iters", 8))
        self.min_std, self.run = float(getattr(args, "modes_min_std", 1.0)), run
        self.sums = {k: np.zeros((len(hz), 2), np.float64) for k in ("nll", "top1", "best")}
        self.passes, self.present = 0, 0

    def update(self, model, Y, score, fut, masks):
        r = self.run
        mm = model.evaluate_modes(Y, score, fut, modes=self.n, seeds=self.seeds, nms_radius=self.radius, nms_metric=self.metric, iters=self.iters,
                                  min_std=self.min_std, horizons=r.hz, units=r.units, log_floor=KDE_LOG_FLOOR)
        for i, c in enumerate(masks.c):
            for k in self.sums:
                self.sums[k][i] += mm[k][c, i].astype(np.float64).sum(0)
        self.passes += int(mm["passes"][masks.valid.reshape(-1)].sum())
        self.present += int(masks.valid.sum())

    def result(self) -> dict:
        m = {k: self.run.mean(v) for k, v in self.sums.items()}
        return {"modes": {"n": self.n, "seeds": self.seeds, "iters": self.iters, "min_std_px": self.min_std, "log_floor": KDE_LOG_FLOOR,
                          "mean_passes": float(self.passes / max(self.present, 1)), "nll": _per_horizon(m["nll"], "mean", "final"),
                          "top1": _per_horizon(m["top1"], "ade", "fde"), "best": _per_horizon(m["best"], "ade", "fde")}}


class _JointModes:
    """--joint_modes N: the mixture of N scene modes per window -- its joint likelihood of the ground truth per agent, the joint errors of the most
    probable and of the best mode's means, over the windows with an agent taking part (by the targets' ids alone, as --joint counts), and the Lloyd
    passes per such window."""

    def __init__(self, args, hz, run):
        self.n = int(getattr(args, "joint_modes", 0) or 0)
        self.on = bool(self.n)
        self.seeds = str(getattr(args, "joint_modes_seeds", "nms"))
        if self.on and self.seeds == "nms" and getattr(args, "joint_radius", None) is None:
            raise ValueError("--joint_modes with --joint_modes_seeds nms needs --joint_radius (pixels)")
        self.iters, self.min_std, self.run = int(getattr(args, "joint_modes_iters", 8)), float(getattr(args, "joint_modes_min_std", 1.0)), run
        self.worlds = {"seeds": "score"}
        if self.seeds == "nms":
            self.worlds = dict(seeds="worlds", worlds_radius=getattr(args, "joint_radius", None), worlds_metric=str(getattr(args, "joint_metric", "final")),
                               worlds_reduce=str(getattr(args, "joint_reduce", "mean")), horizon=getattr(args, "joint_horizon", None),
                               collision_radius=getattr(args, "collision_radius", None),
                               collision_penalty=float(getattr(args, "collision_penalty", 0.0) or 0.0))
        self.sums = {k: np.zeros((len(hz), 2), np.float64) for k in ("nll", "top1", "best")}
        self.windows, self.passes = np.zeros(len(hz), np.int64), 0

    def update(self, model, Y, score, fut, masks):
        r = self.run
        mm = model.evaluate_scene_modes(Y, score, fut, modes=self.n, iters=self.iters, min_std=self.min_std, horizons=r.hz, units=r.units,
                                        log_floor=KDE_LOG_FLOOR, **self.worlds)
        takes = np.stack([masks.seen[:, :h].any((1, 2)) for h in r.hz], 1)                       # [n, n_h]
        for k in self.sums:
            self.sums[k] += np.where(takes[:, :, None], mm[k].astype(np.float64), 0.0).sum(0)
        self.windows += takes.sum(0)
        self.passes += int(mm["passes"][takes[:, -1]].sum())

    def result(self) -> dict:
        m = {k: v / np.maximum(self.windows, 1)[:, None] for k, v in self.sums.items()}
        return {"joint_modes": {"n": self.n, "seeds": self.seeds, "iters": self.iters, "min_std_px": self.min_std, "log_floor": KDE_LOG_FLOOR,
                                "windows": [int(v) for v in self.windows], "mean_passes": float(self.passes / max(int(self.windows[-1]), 1)),
                                "nll": _per_horizon(m["nll"], "mean", "final"), "top1": _per_horizon(m["top1"], "jade", "jfde"),
                                "best": _per_horizon(m["best"], "jade", "jfde")}}


def _masks(past, fut, hz, mno: int) -> SimpleNamespace:
    """The agent masks of a batch, computed once for every block, on the model's slot axis (mno >= the loader's, the padding never counted):
    valid [n, mno] = present at the last observed frame; seen [n, T_pred, mno] = in that target frame; per horizon h, flat over (window, slot),
    c = valid and seen before h and at = valid and seen at frame h - 1; all = valid and seen at all."""
    pw, fw = np.stack(past), np.stack(fut)
    valid = np.zeros((pw.shape[0], mno), bool)
    valid[:, :pw.shape[2]] = pw[:, -1, :, 0] != 0
    seen = np.zeros((pw.shape[0], fw.shape[1], mno), bool)
    seen[:, :, :pw.shape[2]] = fw[:, :, :, 0] != 0
    return SimpleNamespace(valid=valid, seen=seen, c=[(valid & seen[:, :h].any(1)).reshape(-1) for h in hz],
                           at=[(valid & seen[:, h - 1]).reshape(-1) for h in hz], all=(valid & seen.any(1)).reshape(-1))


def evaluate(args, data_loader=None, model=None) -> dict:
    """Runs the walk; returns the result dict main() prints.  `data_loader` / `model` may be injected (tests)."""
    from .data_loader import DataLoader
    from .model import DESIREModel, default_top, dims_from_args
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
    hz = parse_horizons(args.eval_horizons, t_pred)
    run = _Run(args, hz, generator, K, int(args.eval_top or default_top(K)), t_pred)
    # every block reads its flags here -- a bad one is refused before a window is touched --, the enabled ones report in this order
    blocks = [run] + [b for b in [B(args, hz, run) for B in (_Ranked, _Select, _KdeNll, _Joint, _PlanRisk, _Occupancy, _Offroad, _Modes, _JointModes)] if b.on]
    mno = dims_from_args(args, 1, False).mno                             # the model's slot axis: max_num_obj padded up
    for xs, ds in iter_batches(data_loader, int(args.batch_size), int(args.max_windows or 0)):
        past, fut = split_windows(xs, t_obs)
        # --device_rng: a window's noise is a function of its running index, so the result does not depend on --batch_size
        gen = {} if generator == "cvae" else {"generator": generator}
        model.predict(past, top=run.top, seed=args.seed, device_rng=bool(getattr(args, "device_rng", False)), window_base=run.windows, **gen)
        masks = _masks(past, fut, hz, mno)
        masks.video, masks.loader = ds, data_loader                      # (--offroad: the video of every window picks its mask)
        for b in blocks:
            b.update(model, model.final_output, model.final_states, fut, masks)
    res = {}
    for b in blocks:
        res.update(b.result())
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
