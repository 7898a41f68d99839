"""Training loop -- host-side mirror of the reference's train.py:24-207 on top of libdesire_hip.so.

Kept from the reference: the argparse flags and defaults of train.py:28-88, the epoch loop with
`lr = learning_rate * decay_rate ** epoch` (train.py:122-126), `reset_batch_pointer()` per epoch, the save cadence
`(epoch * num_batches + batch) % save_every == 0 and > 0` (train.py:197-206), the per-batch log line
(train.py:185-193) and `save/config.pkl` (train.py:100-101).

Different on purpose: the reference fetches only `cost` (train.py:181, its Adam op is never run) one window at a
time; here every batch is ONE forward + backward + clip + Adam step over all `batch_size` windows
(`DESIREModel.train_step`), the loader window is `seq_length + pred_length` frames split into past / future (the
reference has one length and feeds the window shifted by a frame as "target"), and checkpoints are named fp32 `.npz`
files (formats.save_weights) instead of TF checkpoints.  With torch.distributed initialised every rank takes its block
of the batch's windows and gradients are averaged with one flat all-reduce (dist.allreduce_mean_).

    python -m desire_amd.train --data_dir data/ --batch_size 16 --max_num_obj 32 --d_dim 128 --num_epochs 1
"""
from __future__ import annotations

import argparse
import os
import pickle
import sys
import time
from typing import Callable, List, Sequence, Tuple

import numpy as np

from ._lib import RECON_MODES, RECON_SCOPES


def _noise(args, step: int, rank: int, world: int) -> dict:
    """Where a training step's latent noise comes from: torch.randn seeded per (step, rank), or with --device_rng the device generator seeded per
    step on every rank alike, each rank at the global index of its first window (dist.shard_windows) -- the step's noise is then the one-rank step's."""
    if not getattr(args, "device_rng", False):
        return {"seed": args.seed + step * world + rank}
    from .dist import shard_windows
    return {"seed": args.seed + step, "device_rng": True, "window_base": shard_windows(int(args.batch_size), rank, world)[0]}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="DESIRE training on MI355X (flags of the reference's train.py:28-88)")
    p.add_argument("--rnn_size", type=int, default=512)
    p.add_argument("--num_layers", type=int, default=1)
    p.add_argument("--model", type=str, default="gru")
    p.add_argument("--batch_size", type=int, default=10)
    p.add_argument("--seq_length", type=int, default=8)
    p.add_argument("--num_epochs", type=int, default=100)
    p.add_argument("--save_every", type=int, default=400)
    p.add_argument("--grad_clip", type=float, default=10.0)
    p.add_argument("--learning_rate", type=float, default=0.005)
    p.add_argument("--decay_rate", type=float, default=0.95)
    p.add_argument("--keep_prob", type=float, default=0.8)
    p.add_argument("--embedding_size", type=int, default=64)
    p.add_argument("--neighborhood_size", type=int, default=32)
    p.add_argument("--grid_size", type=int, default=4)
    p.add_argument("--max_num_obj", type=int, default=60)
    p.add_argument("--leave_dataset", type=int, default=5)
    p.add_argument("--latent_size", type=int, default=128)
    p.add_argument("--e_dim", type=int, default=256)
    p.add_argument("--d_dim", type=int, default=16)
    p.add_argument("--stride", type=int, default=1)
    # ---- not in the reference ----
    p.add_argument("--pred_length", type=int, default=None, help="future frames (default: seq_length)")
    p.add_argument("--num_samples", type=int, default=20, help="K futures per agent")
    p.add_argument("--data_dir", type=str, default="data/")
    p.add_argument("--traj_bin", type=str, default=None, help="DSRTRJ1 container instead of CSV/cpkl")
    p.add_argument("--save_dir", type=str, default="save")
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many optimiser steps (0 = all epochs)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device_rng", action="store_true",
                   help="draw the latent noise on the device (counter-based Philox, desire_set_rng) instead of torch.randn: no eps tensor, and a "
                        "window's noise depends on (seed, step, its index in the global batch), not on the rank count or the batch cut")
    p.add_argument("--fix_id0", action="store_true", help="keep SDD track id 0 (the reference drops it)")
    p.add_argument("--ioc_iters", type=int, default=1, help="IOC refinement passes")
    p.add_argument("--bf16", type=str, default="", choices=["", "f32", "x3", "split"],
                   help="matrix operands of the training step: fp32 (default) or x3 = split-bf16 (hi + lo, three bf16 MFMAs per product) in the IOC "
                        "forward / BPTT, the weight-gradient reductions and the large data-gradient convolutions; gradients stay within the fp32 "
                        "path's tolerance of float64 autograd")
    p.add_argument("--two_piece_forward", action="store_true",
                   help="with --bf16 x3: two-piece operands in the forward pass's sample generation too (DESIRE_FLAG_TRAIN_FWD_3P: ~4 %% faster "
                        "steps, gradients within 5e-4 instead of 2e-4 of float64 autograd)")
    p.add_argument("--skip_padding", action="store_true",
                   help="(the default since round 6; kept so that older command lines still parse) DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC: "
                        "run the step on the agents that are present only -- the per-row stages on present rows, the IOC on slot classes "
                        "(include/desire_hip.h).  On SDD windows most of max_num_obj is padding (utils/data_loader.py:209-229): 2.3x faster steps on "
                        "bookstore/video6 at max_num_obj 32; gradients equal the padded step's to fp32 reduction noise")
    p.add_argument("--keep_padding", action="store_true",
                   help="run every one of the max_num_obj slots of every window like the reference does (it masks id-0 objects in the cost only, "
                        "model/model.py:351-366): the opt-out of the default above.  The compacted step reads the present-agent counts back once per "
                        "step (one host wait on an event, include/desire_hip.h)")
    p.add_argument("--head_loss_weight", type=float, default=0.0,
                   help="weight of the reference's own loss for the 5-wide Gaussian output layer (model/model.py:494-550: -log N(next position | "
                        "mux, muy, sx, sy, rho), teacher-forced over the observed frames) added to the training loss; > 0 trains gauss_head/w|b "
                        "(and the X encoder through it), i.e. what sample(mode='rollout') reads")
    p.add_argument("--recon_loss", type=str, default="mean", choices=list(RECON_MODES),
                   help="the reconstruction term over the K samples: mean (the paper's, default), min (best-of-many: only the sample closest to the "
                        "observed future carries the reconstruction gradient) or softmin (a soft-min at temperature --recon_tau); KL and the IOC "
                        "terms keep their mean over K")
    p.add_argument("--recon_tau", type=float, default=None,
                   help="temperature of --recon_loss softmin in normalised units, > 0 (large: the mean, small: the min); required for softmin")
    p.add_argument("--recon_scope", type=str, default="agent", choices=list(RECON_SCOPES),
                   help="who picks among the K samples under --recon_loss min / softmin: agent (every agent its own best sample, default) or scene "
                        "(sample k of every agent of a window is one joint future: the window's best joint future, or a soft-min over them, carries "
                        "the gradient of all its agents -- the scene-level variety loss); ignored with --recon_loss mean")
    p.add_argument("--collision_weight", type=float, default=0.0,
                   help="weight of the collision penalty in the training loss (default 0: off): per joint future -- sample k of every agent of a "
                        "window -- and frame, (1 - dist / radius)^2 of every pair of agents closer than the radius, averaged over the K samples and "
                        "the agents; the column --report_joint prints is the one it pushes down")
    p.add_argument("--collision_loss_radius", type=float, default=None,
                   help="radius of --collision_weight in pixels (default: --collision_radius)")
    p.add_argument("--offroad_weight", type=float, default=0.0,
                   help="weight of the off-road penalty in the training loss (default 0: off): per joint future and frame, (d / scale)^2 with d the "
                        "distance in pixels from the predicted position to the nearest traversable cell of the video's mask (--scene_masks), "
                        "averaged over the K samples and the agents; needs --offroad_scale and --scene_masks")
    p.add_argument("--offroad_scale", type=float, default=None, help="scale of --offroad_weight in pixels: a position this far off the road costs 1")
    p.add_argument("--refine_recon", action="store_true",
                   help="the regression term of the refined trajectories follows --recon_loss / --recon_tau / --recon_scope, with weights from the "
                        "refined errors (default: the plain mean over the K samples, which pulls every refined sample to the observed future); "
                        "changes nothing with --recon_loss mean")
    p.add_argument("--refine_collision_weight", type=float, default=0.0,
                   help="weight of the collision penalty on the REFINED trajectories, the ones the reports read (default 0: off); the radius is "
                        "--collision_loss_radius / --collision_radius, and --collision_weight may stay 0")
    p.add_argument("--refine_offroad_weight", type=float, default=0.0,
                   help="weight of the off-road penalty on the REFINED trajectories (default 0: off); needs --offroad_scale and --scene_masks, and "
                        "--offroad_weight may stay 0")
    p.add_argument("--scene_masks", type=str, default=None,
                   help=".npz with one [Mh, Mw] uint8 traversability mask per video over the whole frame (0 = not traversable), keyed like "
                        "--scene_images by the video directory relative to --data_dir; every mask has the same shape")
    p.add_argument("--prefetch", type=int, default=2,
                   help="batches the loader thread keeps in flight (pinned staging -> copy stream -> device; desire_amd/prefetch.py); 0 = the "
                        "reference's serial loop: next_batch, copy, step, read the loss, every step (train.py:131-183)")
    p.add_argument("--scene_images", type=str, default=None,
                   help=".npz with one [4*scene_grid, 4*scene_grid, 3] float image per video, keyed by the video directory relative to --data_dir "
                        "(e.g. bookstore/video6): the scene CNN runs on them and trains with the model (n_grids = the file's entries)")
    p.add_argument("--report_ade", action="store_true",
                   help="after every epoch: ADE / FDE (mean-of-K and best-of-K, normalised units) of PRIOR samples on the epoch's last batch")
    p.add_argument("--report_ranked", action="store_true",
                   help="after every epoch, on the same batch: errors of the paper's protocol in pixels -- ADE / FDE per horizon of the sample the IOC "
                        "scores best (top-1) and of the best among the --eval_top best-scored samples")
    p.add_argument("--report_nll", action="store_true",
                   help="after every epoch, on the same batch: KDE negative log-likelihood of the ground truth under the K prior samples over the "
                        "whole prediction (per pixel^2, log clipped at -20), with equal weights and with weights softmax(IOC score)")
    p.add_argument("--report_joint", action="store_true",
                   help="after every epoch, on the same batch: the K samples of a window as K joint futures -- JADE / JFDE per horizon in pixels of "
                        "the best-scored joint future and of the best among the --eval_top best-scored, and the collision rate at --collision_radius")
    p.add_argument("--collision_radius", type=float, default=None,
                   help="--report_joint (and the evaluation's --joint, --plan_risk): two agents closer than this many pixels in a frame touch "
                        "(default: 0, nothing touches)")
    p.add_argument("--eval_top", type=int, default=None, help="samples per agent the ranked report keeps (default: 10 %% of --num_samples, at least 1)")
    p.add_argument("--eval_horizons", type=str, default=None,
                   help="horizons of the ranked report in frames, comma separated and increasing, e.g. 3,6,9,12 (default: quarters of --pred_length)")
    return p


def check_recon_args(args) -> None:
    """--recon_loss / --recon_tau: softmin needs a finite temperature > 0; a temperature without softmin is a mistake, not a default.
    --recon_scope: agent or scene (scene with mean is accepted: the mean does not depend on the scope)."""
    mode = getattr(args, "recon_loss", "mean") or "mean"
    scope = getattr(args, "recon_scope", "agent") or "agent"
    if scope not in RECON_SCOPES:
        raise ValueError("--recon_scope must be one of %s, got %r" % (", ".join(RECON_SCOPES), scope))
    tau = getattr(args, "recon_tau", None)
    if mode not in RECON_MODES:
        raise ValueError("--recon_loss must be one of %s, got %r" % (", ".join(RECON_MODES), mode))
    if mode == "softmin":
        if tau is None:
            raise ValueError("--recon_loss softmin needs --recon_tau")
        if not (np.isfinite(float(tau)) and float(tau) > 0.0):
            raise ValueError("--recon_tau must be finite and > 0, got %r" % (tau,))
    elif tau is not None:
        raise ValueError("--recon_tau is the temperature of --recon_loss softmin (got --recon_loss %s)" % mode)
    check_collision_args(args)
    check_offroad_args(args)
    check_refined_args(args)


def check_refined_args(args) -> None:
    """--refine_collision_weight / --refine_offroad_weight: finite and >= 0; > 0 needs what the Y0 term of the same kind needs (a positive radius; a
    positive --offroad_scale and --scene_masks).  --refine_recon is a switch."""
    w = float(getattr(args, "refine_collision_weight", 0.0) or 0.0)
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError("--refine_collision_weight must be finite and >= 0, got %r" % (w,))
    r = collision_loss_radius(args)
    if w > 0.0 and (r is None or not (np.isfinite(float(r)) and float(r) > 0.0)):
        raise ValueError("--refine_collision_weight > 0 needs a radius > 0 in pixels: --collision_loss_radius or --collision_radius (got %r)" % (r,))
    w = float(getattr(args, "refine_offroad_weight", 0.0) or 0.0)
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError("--refine_offroad_weight must be finite and >= 0, got %r" % (w,))
    if w > 0.0:
        s = getattr(args, "offroad_scale", None)
        if s is None or not (np.isfinite(float(s)) and float(s) > 0.0):
            raise ValueError("--refine_offroad_weight > 0 needs --offroad_scale finite and > 0 in pixels (got %r)" % (s,))
        if not getattr(args, "scene_masks", None):
            raise ValueError("--refine_offroad_weight > 0 needs --scene_masks: the masks its distance field is built from")
    if getattr(args, "refine_recon", False) not in (False, True, 0, 1, None):
        raise ValueError("--refine_recon is a switch (got %r)" % (getattr(args, "refine_recon"),))


def check_offroad_args(args) -> None:
    """--offroad_weight: finite and >= 0; > 0 needs --offroad_scale finite and > 0 and --scene_masks."""
    w = float(getattr(args, "offroad_weight", 0.0) or 0.0)
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError("--offroad_weight must be finite and >= 0, got %r" % (w,))
    if w == 0.0:
        return
    s = getattr(args, "offroad_scale", None)
    if s is None or not (np.isfinite(float(s)) and float(s) > 0.0):
        raise ValueError("--offroad_weight > 0 needs --offroad_scale finite and > 0 in pixels (got %r)" % (s,))
    if not getattr(args, "scene_masks", None):
        raise ValueError("--offroad_weight > 0 needs --scene_masks: the masks its distance field is built from")


def collision_loss_radius(args):
    """The radius of the collision term in pixels: --collision_loss_radius, else --collision_radius, else None."""
    r = getattr(args, "collision_loss_radius", None)
    return getattr(args, "collision_radius", None) if r is None else r


def check_collision_args(args) -> None:
    """--collision_weight: finite and >= 0; > 0 needs a positive radius from --collision_loss_radius or --collision_radius."""
    w = float(getattr(args, "collision_weight", 0.0) or 0.0)
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError("--collision_weight must be finite and >= 0, got %r" % (w,))
    r = collision_loss_radius(args)
    if w > 0.0 and (r is None or not (np.isfinite(float(r)) and float(r) > 0.0)):
        raise ValueError("--collision_weight > 0 needs a radius > 0 in pixels: --collision_loss_radius or --collision_radius (got %r)" % (r,))


def step_line(args, step: int, total: int, epoch: int, terms: dict, dt: float) -> str:
    """The per-step log line (train.py:185-190); with --recon_loss min / softmin it also names the mode and prints the term that is trained."""
    line = "{}/{} (epoch {}), train_loss = {:.3f}, time/batch = {:.3f}".format(step, total, epoch, terms["loss"], dt)
    mode = getattr(args, "recon_loss", "mean") or "mean"
    if mode != "mean":
        tag = "softmin tau={:g}".format(float(args.recon_tau)) if mode == "softmin" else mode
        if (getattr(args, "recon_scope", "agent") or "agent") == "scene":
            tag = "scene " + tag
        line += ", recon[{}] = {:.5f}".format(tag, terms["recon"])
    w = float(getattr(args, "collision_weight", 0.0) or 0.0)
    if w > 0.0:
        line += ", col[r={:g} w={:g}] {:.5f}".format(float(collision_loss_radius(args)), w, terms.get("col", float("nan")))
    w = float(getattr(args, "offroad_weight", 0.0) or 0.0)
    if w > 0.0:
        line += ", off[s={:g} w={:g}] {:.5f}".format(float(args.offroad_scale), w, terms.get("off", float("nan")))
    w = float(getattr(args, "refine_collision_weight", 0.0) or 0.0)
    if w > 0.0:
        line += ", rcol[w={:g}] {:.5f}".format(w, terms.get("rcol", float("nan")))
    w = float(getattr(args, "refine_offroad_weight", 0.0) or 0.0)
    if w > 0.0:
        line += ", roff[w={:g}] {:.5f}".format(w, terms.get("roff", float("nan")))
    return line


def parse_horizons(text, t_pred: int) -> List[int]:
    """--eval_horizons: "3,6,9,12" -> [3, 6, 9, 12]; None -> the quarters of the prediction (model.default_horizons)."""
    from .model import default_horizons
    if not text:
        return default_horizons(t_pred)
    hz = [int(x) for x in str(text).split(",") if x.strip()]
    if not hz or len(hz) > 8 or any(b <= a for a, b in zip(hz, hz[1:])) or hz[0] < 1 or hz[-1] > t_pred:
        raise ValueError("--eval_horizons: 1 to 8 strictly increasing frame counts in 1..pred_length (%d), got %r" % (t_pred, text))
    return hz


def _gos(grid_of_video, dval):
    """grid_of_scene of a batch: the scene image of each window's video index (None without --scene_images)."""
    return None if grid_of_video is None else grid_of_video[np.asarray(dval, np.int64)]


def _mos(mask_of_video, dval) -> dict:
    """The mask_of_scene= keyword of a batch: the mask of each window's video index (no keyword at all without --scene_masks)."""
    return {} if mask_of_video is None else {"mask_of_scene": mask_of_video[np.asarray(dval, np.int64)]}


def lr_at_epoch(args, epoch: int) -> float:
    """train.py:122-126."""
    return float(args.learning_rate) * float(args.decay_rate) ** int(epoch)


def should_save(epoch: int, batch: int, num_batches: int, save_every: int) -> bool:
    """train.py:197-199."""
    step = epoch * num_batches + batch
    return step % save_every == 0 and step > 0


def split_windows(xval: Sequence[np.ndarray], t_obs: int) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """Loader windows of seq_length + pred_length frames -> (past [T_obs, MNO, 3], future [T_pred, MNO, 3])."""
    past = [np.asarray(x)[:t_obs] for x in xval]
    fut = [np.asarray(x)[t_obs:] for x in xval]
    return past, fut


def scene_image_keys(data_loader, data_dir: str) -> List[str]:
    """The key of every video the loader reads, in its video index order d: the video directory relative to data_dir."""
    paths = data_loader._csv_paths()[: data_loader.leave_dataset]
    return [os.path.relpath(os.path.dirname(p), data_dir).replace(os.sep, "/") for p in paths]


def load_scene_images(path: str, video_keys: Sequence[str], Gh: int, Gw: int) -> Tuple[np.ndarray, np.ndarray]:
    """--scene_images: (images [n_grids, 4 Gh, 4 Gw, 3] float32, grid of every video index).  n_grids = the entries of the file (sorted by key);
    a video without an entry, or an entry of another shape, raises ValueError naming them."""
    with np.load(path) as z:
        keys = sorted(z.files)
        arrays = {k: np.asarray(z[k]) for k in keys}
    missing = [k for k in video_keys if k not in arrays]
    if missing:
        raise ValueError("--scene_images %s has no image for the video(s) %s (keys: %s)" % (path, ", ".join(missing), ", ".join(keys)))
    want = (4 * Gh, 4 * Gw, 3)
    bad = ["%s %s" % (k, tuple(a.shape)) for k, a in arrays.items() if tuple(a.shape) != want]
    if bad:
        raise ValueError("--scene_images %s: every image must be %s, got %s" % (path, want, ", ".join(bad)))
    images = np.stack([arrays[k].astype(np.float32) for k in keys])
    return images, np.array([keys.index(k) for k in video_keys], np.int32)


def load_scene_masks(path: str, video_keys: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """--scene_masks: (masks [n_masks, Mh, Mw] uint8, mask of every video index).  n_masks = the entries of the file (sorted by key); a video
    without an entry, an entry that is not two-dimensional or of another shape than the first, or a side beyond 1024 raises ValueError."""
    with np.load(path) as z:
        keys = sorted(z.files)
        arrays = {k: np.asarray(z[k]) for k in keys}
    missing = [k for k in video_keys if k not in arrays]
    if missing:
        raise ValueError("--scene_masks %s has no mask for the video(s) %s (keys: %s)" % (path, ", ".join(missing), ", ".join(keys)))
    want = tuple(arrays[keys[0]].shape)
    if len(want) != 2 or not all(1 <= s <= 1024 for s in want):
        raise ValueError("--scene_masks %s: a mask must be [Mh, Mw] with sides 1..1024, got %s %s" % (path, keys[0], want))
    bad = ["%s %s" % (k, tuple(a.shape)) for k, a in arrays.items() if tuple(a.shape) != want]
    if bad:
        raise ValueError("--scene_masks %s: every mask must be %s, got %s" % (path, want, ", ".join(bad)))
    masks = np.stack([(arrays[k] != 0).astype(np.uint8) for k in keys])
    return masks, np.array([keys.index(k) for k in video_keys], np.int32)


def train(args, data_loader=None, model=None, log: Callable[[str], None] = print) -> List[float]:
    """Runs the loop; returns the per-step losses.  `data_loader` / `model` may be injected (tests)."""
    from .data_loader import DataLoader
    from .dist import shard_batch
    from .model import DESIREModel
    import torch.distributed as dist

    check_recon_args(args)
    if args.pred_length is None:
        args.pred_length = args.seq_length
    t_obs, t_pred = int(args.seq_length), int(args.pred_length)
    if data_loader is None:
        data_loader = DataLoader(args.batch_size, t_obs + t_pred, args.max_num_obj, args.leave_dataset, preprocess=False,
                                 data_dir=args.data_dir, traj_bin=args.traj_bin, fix_id0=args.fix_id0)
    if data_loader.seq_length != t_obs + t_pred:
        raise ValueError("the loader window must be seq_length + pred_length frames")
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
    if args.batch_size < world:
        raise ValueError("--batch_size %d is smaller than the %d ranks: every rank needs at least one window per step" % (args.batch_size, world))
    # next_batch advances its pointer by random.randint (utils/data_loader.py:235-238): the SAME seed on every rank, so that all
    # ranks draw the same global batch and shard_batch partitions it (and --seed makes a run reproducible)
    import random
    random.seed(int(args.seed))
    if rank == 0:
        os.makedirs(args.save_dir, exist_ok=True)
        with open(os.path.join(args.save_dir, "config.pkl"), "wb") as fh:
            pickle.dump(args, fh)
    grid_of_video = None
    if getattr(args, "scene_images", None):
        G = int(getattr(args, "scene_grid", 64))
        images, grid_of_video = load_scene_images(args.scene_images, scene_image_keys(data_loader, args.data_dir), G, G)
        args.n_grids = int(images.shape[0])
    mask_of_video = None
    if getattr(args, "scene_masks", None):
        masks, mask_of_video = load_scene_masks(args.scene_masks, scene_image_keys(data_loader, args.data_dir))
    if model is None:
        model = DESIREModel(args, seed=args.seed)
    if grid_of_video is not None:
        model.set_scene_images(images, np.zeros(1, np.int32))
        model._grid_of_video = grid_of_video
    if mask_of_video is not None:
        model.set_scene_masks(masks, np.zeros(1, np.int32))
        model._mask_of_video = mask_of_video
    losses: List[float] = []
    # the overlapped schedule needs the fast loader's next_batch_into; a reference-shaped loader (utils/data_loader.py's API: next_batch only) gets
    # the reference's serial loop instead of an AttributeError from the feeder thread
    if int(getattr(args, "prefetch", 0) or 0) > 0 and hasattr(data_loader, "next_batch_into"):
        return _train_overlapped(args, data_loader, model, log, rank, world, t_obs, t_pred, losses)
    steps = 0
    for epoch in range(args.num_epochs):
        model.learning_rate = lr_at_epoch(args, epoch)
        data_loader.reset_batch_pointer()
        for batch in range(data_loader.num_batches):
            start = time.time()
            xval, _, dval = data_loader.next_batch()
            past, fut = split_windows(shard_batch(xval, rank, world), t_obs)
            terms = model.train_step(past, fut, **_noise(args, steps, rank, world), grid_of_scene=_gos(grid_of_video, shard_batch(dval, rank, world)),
                                     **_mos(mask_of_video, shard_batch(dval, rank, world)))
            losses.append(terms["loss"])
            steps += 1
            if rank == 0:
                log(step_line(args, epoch * data_loader.num_batches + batch, args.num_epochs * data_loader.num_batches, epoch, terms,
                              time.time() - start))
                sys.stdout.flush()
            if rank == 0 and should_save(epoch, batch, data_loader.num_batches, args.save_every):
                path = os.path.join(args.save_dir, "social_model-%d.npz" % (epoch * data_loader.num_batches + batch))
                model.save(path)
                log("model saved to {}".format(path))
            if args.max_steps and steps >= args.max_steps:
                return losses
        if data_loader.num_batches > 0:
            _report(args, model, past, fut, epoch, rank, log)
    return losses


def _report_ade(args, model, past, fut, epoch, rank, log) -> None:
    """The evaluation harness the reference never had: prior sampling (no future given) on this rank's share of the
    epoch's last batch, masked like the loss (present at the last observed frame and in every future frame).  past / fut: lists of
    loader windows or device tensors [n, T, mno, 3]."""
    import torch
    if torch.is_tensor(past):
        Y, _ = model.forward_device(past, None, seed=args.seed)
        pw, fw = past.cpu().numpy(), fut.cpu().numpy()
    else:
        Y, _ = model.forward(past, None, seed=args.seed)
        pw, fw = np.stack([np.asarray(p) for p in past]), np.stack([np.asarray(f) for f in fut])
    ev = model.evaluate(Y, fut)
    there = np.zeros(ev.shape[0], bool)
    m = pw.shape[2]
    there.reshape(pw.shape[0], -1)[:, :m] = (pw[:, -1, :, 0] != 0) & (fw[:, :, :, 0] != 0).all(1)
    if there.any():
        e = ev[there].mean(0)
        log("epoch {} rank {}: ADE/FDE mean-of-K = {:.5f} / {:.5f}, best-of-K = {:.5f} / {:.5f} ({} agents)".format(
            epoch, rank, e[0], e[1], e[2], e[3], int(there.sum())))


def _report_ranked(args, model, past, fut, epoch, rank, log) -> None:
    """--report_ranked: what the ranking module is for.  The batch, the prior samples (same seed) and the agents of _report_ade; the K samples
    of every agent are ranked by IOC score on the device and the errors are those of the paper's protocol, in pixels, per horizon: of the
    best-scored sample and of the best among the top N by score."""
    import torch
    from .model import default_top
    if torch.is_tensor(past):
        Y, score = model.forward_device(past, None, seed=args.seed)
        pw, fw = past.cpu().numpy(), fut.cpu().numpy()
    else:
        Y, score = model.forward(past, None, seed=args.seed)
        pw, fw = np.stack([np.asarray(p) for p in past]), np.stack([np.asarray(f) for f in fut])
    top = int(getattr(args, "eval_top", None) or default_top(int(Y.shape[1])))
    hz = parse_horizons(getattr(args, "eval_horizons", None), int(Y.shape[3]))
    ev = model.evaluate_ranked(Y, score, fut, top=top, horizons=hz, units="px")
    there = np.zeros(ev.shape[0], bool)
    m = pw.shape[2]
    there.reshape(pw.shape[0], -1)[:, :m] = (pw[:, -1, :, 0] != 0) & (fw[:, :, :, 0] != 0).all(1)
    if there.any():
        e = ev[there].astype(np.float64).mean(0)                       # [n_h, 4]
        fmt = lambda col: "[" + ", ".join("%.3f" % v for v in e[:, col]) + "]"
        log("epoch {} rank {}: ranked px @h={}: top-1 ADE/FDE = {} / {}, best-of-top-{} = {} / {} ({} agents)".format(
            epoch, rank, "[" + ", ".join(str(h) for h in hz) + "]", fmt(0), fmt(1), top, fmt(2), fmt(3), int(there.sum())))


def _report_nll(args, model, past, fut, epoch, rank, log) -> None:
    """--report_nll: the proper scoring rule next to the ranked errors.  The batch, the prior samples (same seed) and the agents of _report_ade; a
    Gaussian KDE of every agent's K samples per frame, once with equal weights and once with softmax(IOC score), mean over the whole prediction."""
    import torch
    if torch.is_tensor(past):
        Y, score = model.forward_device(past, None, seed=args.seed)
        pw, fw = past.cpu().numpy(), fut.cpu().numpy()
    else:
        Y, score = model.forward(past, None, seed=args.seed)
        pw, fw = np.stack([np.asarray(p) for p in past]), np.stack([np.asarray(f) for f in fut])
    T = int(Y.shape[3])
    ev = [model.evaluate_nll(Y, score, fut, horizons=[T], units="px", weighted=wt) for wt in (False, True)]
    there = np.zeros(ev[0].shape[0], bool)
    m = pw.shape[2]
    there.reshape(pw.shape[0], -1)[:, :m] = (pw[:, -1, :, 0] != 0) & (fw[:, :, :, 0] != 0).all(1)
    if there.any():
        u, w = (e[there, 0, 0].astype(np.float64).mean() for e in ev)
        log("epoch {} rank {}: KDE NLL px @h={}: uniform = {:.4f}, score-weighted = {:.4f} ({} agents)".format(epoch, rank, T, u, w, int(there.sum())))


def _report_joint(args, model, past, fut, epoch, rank, log) -> None:
    """--report_joint: the number the scene scope of the reconstruction loss is meant to move.  The batch, the prior samples (same seed) of
    _report_ade; sample k of every agent of a window is one joint future, ranked by the summed IOC score on the device: JADE / JFDE per horizon in
    pixels of the best-scored joint future and of the best among the top N, mean over the windows with an agent that takes part, and the share of
    (joint future, agent) pairs that come within --collision_radius of another agent before each horizon."""
    import torch
    from .model import default_top
    Y, score = (model.forward_device if torch.is_tensor(past) else model.forward)(past, None, seed=args.seed)
    top = int(getattr(args, "eval_top", None) or default_top(int(Y.shape[1])))
    hz = parse_horizons(getattr(args, "eval_horizons", None), int(Y.shape[3]))
    radius = getattr(args, "collision_radius", None)
    ev = model.evaluate_joint(Y, score, fut, top=top, horizons=hz, units="px", collision_radius=radius)
    K = int(Y.shape[1])
    cnt = ev["cnt"][:, :K].astype(np.float64)                          # [n, K, n_h, 2]: (touching, taking part) of the K joint futures
    there = cnt[:, 0, -1, 1] > 0                                       # windows with an agent that takes part before the last horizon
    if there.any():
        e = np.nanmean(ev["out"][there].astype(np.float64), 0)         # [n_h, 4]
        rate = cnt[there, :, :, 0].sum((0, 1)) / np.maximum(cnt[there, :, :, 1].sum((0, 1)), 1.0)
        fmt = lambda v: "[" + ", ".join("%.3f" % x for x in v) + "]"
        log("epoch {} rank {}: joint px @h={}: top-1 JADE/JFDE = {} / {}, best-of-top-{} = {} / {}, collision rate (r = {:g} px) = {} ({} windows)".format(
            epoch, rank, "[" + ", ".join(str(h) for h in hz) + "]", fmt(e[:, 0]), fmt(e[:, 1]), top, fmt(e[:, 2]), fmt(e[:, 3]),
            0.0 if radius is None else float(radius), "[" + ", ".join("%.4f" % x for x in rate) + "]", int(there.sum())))


def _report(args, model, past, fut, epoch, rank, log) -> None:
    if getattr(args, "report_ade", False):
        _report_ade(args, model, past, fut, epoch, rank, log)
    if getattr(args, "report_ranked", False):
        _report_ranked(args, model, past, fut, epoch, rank, log)
    if getattr(args, "report_nll", False):
        _report_nll(args, model, past, fut, epoch, rank, log)
    if getattr(args, "report_joint", False):
        _report_joint(args, model, past, fut, epoch, rank, log)


def _train_overlapped(args, data_loader, model, log, rank, world, t_obs, t_pred, losses) -> List[float]:
    """The same schedule with the loader off the critical path (desire_amd/prefetch.py): a background thread runs next_batch into pinned
    staging and uploads on a copy stream `--prefetch` batches ahead; the step's loss is read back ONE STEP LATE, so the host enqueues
    step i + 1 while the device still runs step i.  Same batches, same seeds, same optimiser steps as the serial loop -- the log line of
    step i is printed after step i + 1 has been enqueued, nothing else differs (tests/test_gpu_prefetch.py compares the two)."""
    from .model import dims_from_args
    from .prefetch import WindowFeeder
    mno = dims_from_args(model.args, 1, True).mno
    feeder = WindowFeeder(data_loader, t_obs, t_pred, device=model.device, depth=int(args.prefetch), num_epochs=args.num_epochs,
                          shard=(rank, world), mno=mno, max_batches=int(args.max_steps or 0))
    nb = data_loader.num_batches
    pending = None                                        # (PendingLoss, epoch, batch, start time) of the previous step

    def settle(p):
        terms, epoch, batch, start = p[0].get(), p[1], p[2], p[3]
        losses.append(terms["loss"])
        if rank == 0:
            log(step_line(args, epoch * nb + batch, args.num_epochs * nb, epoch, terms, time.time() - start))
            sys.stdout.flush()

    steps = 0
    last = None
    reporting = getattr(args, "report_ade", False) or getattr(args, "report_ranked", False) or getattr(args, "report_nll", False) or \
        getattr(args, "report_joint", False)
    try:
        for bt in feeder:
            start = time.time()
            model.learning_rate = lr_at_epoch(args, bt.epoch)
            if last is not None and bt.epoch != last[2]:
                _report(args, model, last[0], last[1], last[2], rank, log)
            bt.wait()
            pl = model.train_step_device(bt.past, bt.fut, **_noise(args, steps, rank, world), sync=False,
                                         grid_of_scene=_gos(getattr(model, "_grid_of_video", None), bt.d),
                                         **_mos(getattr(model, "_mask_of_video", None), bt.d))
            if reporting:                                 # the epoch's last batch is evaluated after the feeder has moved on: keep a copy
                last = (bt.past.clone(), bt.fut.clone(), bt.epoch)
            bt.release()
            if pending is not None:
                settle(pending)
            pending = (pl, bt.epoch, bt.index, start)
            steps += 1
            if rank == 0 and should_save(bt.epoch, bt.index, nb, args.save_every):
                path = os.path.join(args.save_dir, "social_model-%d.npz" % (bt.epoch * nb + bt.index))
                model.save(path)
                log("model saved to {}".format(path))
    finally:
        feeder.close()
    if pending is not None:
        settle(pending)
    if last is not None:
        _report(args, model, last[0], last[1], last[2], rank, log)
    return losses


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if args.skip_padding and args.keep_padding:
        raise SystemExit("--skip_padding and --keep_padding exclude each other")
    try:
        check_recon_args(args)
    except ValueError as exc:
        raise SystemExit(str(exc))
    # (dims.flags are derived in desire_amd/model.py: _flags_from_args -- padding skipped unless --keep_padding)
    import torch
    import torch.distributed as dist
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        # DESIRE_DIST_BACKEND=gloo + DESIRE_ONE_GPU=1: the multi-rank path on a box with a single GPU (all ranks share cuda:0 and the
        # flat-gradient all-reduce runs over gloo, because RCCL refuses two ranks on one device); a test switch, never a deployment
        backend = os.environ.get("DESIRE_DIST_BACKEND", "nccl")
        local = 0 if os.environ.get("DESIRE_ONE_GPU") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    try:
        from .model import DESIREModel
        model = DESIREModel(args, seed=args.seed)
        train(args, model=model)
        if dist.is_initialized():
            # data-parallel invariant: every rank applied the same averaged gradient, so every rank holds the same weights
            w = model.sync_weights()
            chk = float(sum(float(np.abs(np.asarray(v, np.float64)).sum()) for v in w.values()))
            print("rank {} weights_checksum = {:.9e}".format(dist.get_rank(), chk))
            sys.stdout.flush()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
