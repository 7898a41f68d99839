"""The scored-sample methods of DESIREModel: everything that looks at the K samples of an agent together with their IOC scores -- ranking,
non-maximum suppression, joint metrics, plan risk, mode fitting per agent and per window, occupancy maps, KDE likelihood -- in their prediction form (predict_* /
score_plans: the prior forward first) and their evaluation form (evaluate_*: samples and scores given, held against the futures).

ScoredSamples is a mixin of DESIREModel (desire_amd/model.py) and uses its torch, device, _handle, _handles, _pad_windows and forward_device.  What
the methods share is stated once here: the evaluation context (_evaluation), the prediction context (_prediction), the order of the samples
(_order) and the small checks and defaults above the class.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import _lib


def default_top(K: int) -> int:
    """How many of an agent's K samples "the top 10 % by score" are (the paper's protocol): max(1, K // 10)."""
    return max(1, int(K) // 10)


def default_horizons(T_pred: int):
    """The paper's 1 / 2 / 3 / 4 s of a 4 s prediction in frames of this model: ceil(T_pred * q / 4) for q = 1..4, duplicates collapsed."""
    return sorted({(int(T_pred) * q + 3) // 4 for q in (1, 2, 3, 4)})


def _ptr(x) -> int:
    """The device address of an optional tensor: 0 for None."""
    return 0 if x is None else x.data_ptr()


def _check_weights(weights, scores: str) -> None:
    if weights not in ("score", "uniform"):
        raise ValueError("weights must be 'score' (softmax of the %s scores) or 'uniform', got %r" % (scores, weights))


def _check_radius(collision_radius) -> None:
    if not (np.isfinite(float(collision_radius)) and float(collision_radius) >= 0):
        raise ValueError("collision_radius must be finite and >= 0 (pixels), got %r" % (collision_radius,))


class ScoredSamples(object):
    """The scored-sample surface of DESIREModel (a mixin: see the module's text)."""

    # ---- what the methods share -----------------------------------------------------------------------------
    def _evaluation(self, Y, fut_windows, horizons=None, units="px"):
        """The context of an evaluate_* call on samples Y [n, ...]: (handle, its dims, horizons in frames, (ux, uy, f) of `units`, the futures
        [n, T_pred, mno, 3] on the device, stream).  The handle is the prior one of n windows when a forward has built it, else the posterior one."""
        torch = self.torch
        n = int(Y.shape[0])
        h = self._handles.get((n, 0, 0)) or self._handle(n, True)
        d = h.dims
        fut = fut_windows if torch.is_tensor(fut_windows) else self._pad_windows(fut_windows, d.mno)
        return h, d, self._horizons(d, horizons), self._unit_scale(units, d), fut, torch.cuda.current_stream().cuda_stream

    def _prediction(self, past, u8: bool = False):
        """The context of a predict_* / score_plans call: (`past` on the device -- loader windows are padded --, the prior handle of its n windows,
        "present" [n, mno] bool = id != 0 at the last observed frame, its uint8 copy for the kernels when u8).  Nothing runs yet: the caller checks
        its arguments, then calls forward_device(past, None, ...)."""
        if not self.torch.is_tensor(past):
            past = self._pad_windows(past, self._handle(len(past), False).dims.mno)
        present = past[:, -1, :, 0] != 0
        return past, self._handle(int(past.shape[0]), False), present, present.to(self.torch.uint8).contiguous() if u8 else None

    def _order(self, h, Y, score, top: int, nms=None):
        """(order [A, K] int32, kept [A] int32 or None): the samples of every agent by descending score (desire_rank_samples), and with nms =
        _nms_args' (metric, t_end, radius) that order put through the non-maximum suppression (desire_select_diverse, the order alone)."""
        torch = self.torch
        d = h.dims
        stream = torch.cuda.current_stream().cuda_stream
        order = torch.empty((d.A, d.K), device=self.device, dtype=torch.int32)
        h.rank_samples(score.data_ptr(), 0, top, order.data_ptr(), 0, 0, stream)
        if nms is None:
            return order, None
        diverse, kept = torch.empty_like(order), torch.empty((d.A,), device=self.device, dtype=torch.int32)
        h.select_diverse(Y.data_ptr(), order.data_ptr(), score.data_ptr(), nms[0], nms[1], nms[2], 1.0 / d.sx, 1.0 / d.sy, top, diverse.data_ptr(),
                         kept.data_ptr(), 0, 0, 0, stream)
        return diverse, kept

    @staticmethod
    def _horizons(d, horizons):
        return default_horizons(d.T_pred) if horizons is None else [int(x) for x in horizons]

    def _scale(self, d):
        """(sx, sy) on the device: pixels times it are normalised units."""
        return self.torch.tensor([d.sx, d.sy], device=self.device, dtype=self.torch.float32)

    @staticmethod
    def _nms_args(select: str, nms_radius, nms_metric: str, nms_horizon, T_pred: int):
        """None for select="score"; (metric, t_end, radius in pixels) for select="nms"."""
        if select == "score":
            return None
        if select != "nms":
            raise ValueError("select must be 'score' (the best-scored samples), 'nms' (score-ordered non-maximum suppression) or 'joint' (the best-scored "
                             "joint samples of the window) or 'worlds' (the distinct joint samples of the window), got %r" % (select,))
        if nms_radius is None:
            raise ValueError("select='nms' needs nms_radius (pixels)")
        metrics = {"final": _lib.DIST_FINAL, "mean": _lib.DIST_MEAN, "max": _lib.DIST_MAX}
        if nms_metric not in metrics:
            raise ValueError("nms_metric must be 'final', 'mean' or 'max', got %r" % (nms_metric,))
        t_end = T_pred if nms_horizon is None else int(nms_horizon)
        if not 1 <= t_end <= T_pred:
            raise ValueError("nms_horizon must be 1..pred_length (%d), got %d" % (T_pred, t_end))
        return metrics[nms_metric], t_end, float(nms_radius)

    @staticmethod
    def _worlds_args(select: str, worlds_radius, worlds_metric: str, worlds_reduce: str, worlds_horizon, collision_penalty, T_pred: int):
        """None unless select == "worlds" (the world keywords are then refused); else (metric, reduce, t_end, radius in pixels, penalty)."""
        if select != "worlds":
            if worlds_radius is not None or worlds_metric != "final" or worlds_reduce != "mean" or worlds_horizon is not None or collision_penalty != 0.0:
                raise ValueError("worlds_radius, worlds_metric, worlds_reduce, worlds_horizon and collision_penalty belong to select='worlds'")
            return None
        if worlds_radius is None:
            raise ValueError("select='worlds' needs worlds_radius (pixels)")
        if not (np.isfinite(float(worlds_radius)) and float(worlds_radius) >= 0):
            raise ValueError("worlds_radius must be finite and >= 0 (pixels), got %r" % (worlds_radius,))
        metrics = {"final": _lib.DIST_FINAL, "mean": _lib.DIST_MEAN, "max": _lib.DIST_MAX}
        if worlds_metric not in metrics:
            raise ValueError("worlds_metric must be 'final', 'mean' or 'max', got %r" % (worlds_metric,))
        reduces = {"all": _lib.WORLD_ALL, "mean": _lib.WORLD_MEAN}
        if worlds_reduce not in reduces:
            raise ValueError("worlds_reduce must be 'mean' (the mean distance over the agents) or 'all' (every agent), got %r" % (worlds_reduce,))
        t_end = T_pred if worlds_horizon is None else int(worlds_horizon)
        if not 1 <= t_end <= T_pred:
            raise ValueError("worlds_horizon must be 1..pred_length (%d), got %d" % (T_pred, t_end))
        if not np.isfinite(float(collision_penalty)):
            raise ValueError("collision_penalty must be finite, got %r" % (collision_penalty,))
        return metrics[worlds_metric], reduces[worlds_reduce], t_end, float(worlds_radius), float(collision_penalty)

    def _select_worlds(self, h, Y, pres8, jscore, collided, wargs, radius: float, ux: float, uy: float):
        """One desire_select_worlds call on device tensors: the world score is jscore [n, K], minus penalty times the collisions of the world
        (collided [n, K] int32) when the penalty is not 0 -- two fp32 operations.  Returns (worder [n, K], wcount [n], wmass [n, K], wlabel [n, K])."""
        torch = self.torch
        d = h.dims
        metric, reduce, t_end, _, penalty = wargs
        wscore = jscore if penalty == 0.0 else (jscore - collided.to(torch.float32) * penalty).contiguous()
        worder = torch.empty((d.n_scenes, d.K), device=self.device, dtype=torch.int32)
        wlabel, wcount = torch.empty_like(worder), torch.empty((d.n_scenes,), device=self.device, dtype=torch.int32)
        wmass = torch.empty((d.n_scenes, d.K), device=self.device, dtype=torch.float32)
        h.select_worlds(Y.data_ptr(), _ptr(pres8), wscore.data_ptr(), metric, reduce, t_end, radius, ux, uy, worder.data_ptr(), wcount.data_ptr(),
                        wmass.data_ptr(), wlabel.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return worder, wcount, wmass, wlabel

    def predict(self, x_batch: Sequence[np.ndarray], top: Optional[int] = None, eps=None, seed: int = 0, grid_of_scene=None, device_rng: bool = False,
                window_base: int = 0, generator: str = "cvae", normals=None, select: str = "score", nms_radius=None, nms_metric: str = "final",
                nms_horizon=None, collision_radius=None, worlds_radius=None, worlds_metric: str = "final", worlds_reduce: str = "mean", worlds_horizon=None,
                collision_penalty: float = 0.0):
        """The `top` most plausible futures of every agent of a batch of observed loader windows [T_obs, MNO, 3], ranked by IOC score
        (prior sampling: no future given).  See predict_device for the result."""
        d = self._handle(len(x_batch), False).dims
        out = self.predict_device(self._pad_windows(x_batch, d.mno), top, eps, seed, grid_of_scene=grid_of_scene, device_rng=device_rng,
                                  window_base=window_base, generator=generator, normals=normals, select=select, nms_radius=nms_radius,
                                  nms_metric=nms_metric, nms_horizon=nms_horizon, collision_radius=collision_radius, worlds_radius=worlds_radius,
                                  worlds_metric=worlds_metric, worlds_reduce=worlds_reduce, worlds_horizon=worlds_horizon, collision_penalty=collision_penalty)
        self.input_data, self.target_data = x_batch, None
        return out

    def predict_device(self, past, top: Optional[int] = None, eps=None, seed: int = 0, grid_of_scene=None, device_rng: bool = False, window_base: int = 0,
                       generator: str = "cvae", normals=None, select: str = "score", nms_radius=None, nms_metric: str = "final", nms_horizon=None,
                       collision_radius=None, worlds_radius=None, worlds_metric: str = "final", worlds_reduce: str = "mean", worlds_horizon=None,
                       collision_penalty: float = 0.0):
        """predict() on windows already in HBM (forward_device's layout).  Returns a dict of device tensors: "traj" [n, mno, top, T_pred, 2]
        IN PIXELS, best-scored first; "score" [n, mno, top]; "order" [n, mno, K] int32 (sample indices by descending score, ties to the
        lower index); "present" [n, mno] bool (id != 0 at the last observed frame -- the rows of absent agents are whatever the forward
        left, zeros under the default padding-skipping flags, and their order is the identity).  top=None: default_top(K).  All K samples
        and scores stay available as self.final_output / self.final_states.
        generator "cvae" (default): the K samples of the CVAE decoder (forward_device).  "rollout": K rollouts of the Gaussian head per agent
        (rollout_samples; `normals` [n, K, mno, T_pred, 2] or None as there, `eps` must be None), scored and refined by the same IOC stage -- the
        reference's generator under the same ranking; warns like sample(mode="rollout") while the head is untrained.
        select "score" (default): the `top` best-scored samples.  "nms": the `top` most plausible MUTUALLY DISTINCT futures -- walking the samples
        best-scored first, one is kept unless it lies within nms_radius pixels (required) of one already kept, by nms_metric "final" (distance at
        the last frame), "mean" (mean distance over the frames) or "max" (largest distance) over the first nms_horizon frames (None: all).
        "traj", "score" and "order" then follow the diverse order (the kept samples, then the suppressed ones best-scored first, so there are
        always `top` distinct samples), and the dict gains "count" [n, mno] int32 (samples kept) and "prob" [n, mno, top] (the softmax(score)
        mass each returned sample absorbed; 0 for a suppressed one).
        select "joint": sample k of every agent of a window was scored and refined together, so the K samples are K joint futures of the scene;
        entry j of EVERY agent of a window is then joint sample jorder[j] -- the order of the scores summed over the present agents
        (desire_joint_metrics, prediction form) -- instead of each agent's own best.  "traj", "score" and "order" keep their shapes ("order" is the
        window's joint order repeated for every slot), and the dict gains "joint_score" [n, top] and "collisions" [n, top] int32: the present agents
        of that joint sample that come within collision_radius pixels (None: 0, nothing touches) of another one at some frame.
        select "worlds": as "joint", but the `top` most plausible MUTUALLY DISTINCT joint futures (desire_select_worlds): walking the joint samples
        best-scored first, one is kept unless it lies within worlds_radius pixels (required) of one already kept -- worlds_reduce "mean": the mean
        over the present agents of their distance (worlds_metric "final", "mean" or "max" over the first worlds_horizon frames, as nms_metric);
        "all": every present agent within the radius.  collision_penalty P != 0 ranks the joint samples by joint score - P * (present agents that
        collide), so a world that runs its agents through each other falls behind a clean one.  The dict is "joint"'s, following the distinct
        order (the kept worlds, then the suppressed ones best-scored first), and gains "count" [n] int32 (worlds kept) and "prob" [n, top] (the
        softmax mass of the world scores each returned world absorbed; 0 for a suppressed one)."""
        torch = self.torch
        worlds = select == "worlds"
        joint = select == "joint" or worlds
        if collision_radius is not None and not joint:
            raise ValueError("collision_radius belongs to select='joint' and select='worlds'")
        if collision_radius is not None:
            _check_radius(collision_radius)
        # refuse a bad selection before the forward runs (the nms horizon: below)
        wargs = self._worlds_args(select, worlds_radius, worlds_metric, worlds_reduce, worlds_horizon, collision_penalty,
                                  self._prediction(past)[1].dims.T_pred if worlds else 1)
        nms = None if joint else self._nms_args(select, nms_radius, nms_metric, None, 1)
        if generator == "cvae":
            if normals is not None:
                raise ValueError("`normals` are the head rollout's draws: pass generator='rollout' with them")
            Y, score = self.forward_device(past, None, eps, seed, grid_of_scene=grid_of_scene, device_rng=device_rng, window_base=window_base)
        elif generator == "rollout":
            if eps is not None:
                raise ValueError("`eps` is the CVAE's latent noise: generator='rollout' takes `normals`")
            Y, score = self._rollout_forward_device(past, normals, seed, grid_of_scene, device_rng, window_base)
        else:
            raise ValueError("generator must be 'cvae' (the CVAE decoder's samples) or 'rollout' (the Gaussian head's rollouts), got %r" % (generator,))
        past, h, present, pres8 = self._prediction(past, u8=joint)
        n, d = int(past.shape[0]), h.dims
        top = default_top(d.K) if top is None else int(top)
        if not 1 <= top <= d.K:
            raise ValueError("top must be 1..num_samples (%d), got %d" % (d.K, top))
        order = torch.empty((n, d.mno, d.K), device=self.device, dtype=torch.int32)
        traj = torch.empty((n, d.mno, top, d.T_pred, 2), device=self.device, dtype=torch.float32)
        sc = torch.empty((n, d.mno, top), device=self.device, dtype=torch.float32)
        stream = torch.cuda.current_stream().cuda_stream
        if joint:
            cnt = torch.empty((n, d.K + 1, 1, 2), device=self.device, dtype=torch.int32)
            jscore = torch.empty((n, d.K), device=self.device, dtype=torch.float32)
            jorder = torch.empty((n, d.K), device=self.device, dtype=torch.int32)
            h.joint_metrics(Y.data_ptr(), 0, pres8.data_ptr(), score.data_ptr(), [d.T_pred], top, float(collision_radius or 0.0), 1.0 / d.sx, 1.0 / d.sy,
                            cnt.data_ptr(), jorder.data_ptr(), 0, 0, jscore.data_ptr(), 0, stream)
            if worlds:
                jorder, wcount, wmass, _ = self._select_worlds(h, Y, pres8, jscore, cnt[:, :d.K, 0, 0], wargs, wargs[3], 1.0 / d.sx, 1.0 / d.sy)
            idx = jorder[:, :top].long()                                     # [n, top]: the joint samples, best first
            w = torch.arange(n, device=self.device)[:, None]
            traj = (Y[w, idx].permute(0, 2, 1, 3, 4) / self._scale(d)).contiguous()
            out = {"traj": traj, "score": score[w, idx].permute(0, 2, 1).contiguous(), "order": jorder[:, None, :].expand(n, d.mno, d.K).contiguous(),
                   "present": present, "joint_score": jscore[w, idx], "collisions": cnt[:, :d.K, 0, 0][w, idx]}
            if worlds:
                out.update({"count": wcount, "prob": wmass[:, :top].contiguous()})
            return out
        if nms is None:
            h.rank_samples(score.data_ptr(), Y.data_ptr(), top, order.data_ptr(), traj.data_ptr(), sc.data_ptr(), stream)
            traj /= self._scale(d)
            return {"traj": traj, "score": sc, "order": order, "present": present}
        metric, t_end, radius = self._nms_args(select, nms_radius, nms_metric, nms_horizon, d.T_pred)
        count = torch.empty((n, d.mno), device=self.device, dtype=torch.int32)
        mass = torch.empty((n, d.mno, d.K), device=self.device, dtype=torch.float32)
        by_score, _ = self._order(h, Y, score, top)                          # this suppression also gathers the kept samples and their mass
        h.select_diverse(Y.data_ptr(), by_score.data_ptr(), score.data_ptr(), metric, t_end, radius, 1.0 / d.sx, 1.0 / d.sy, top, order.data_ptr(),
                         count.data_ptr(), mass.data_ptr(), traj.data_ptr(), sc.data_ptr(), stream)
        traj /= self._scale(d)
        return {"traj": traj, "score": sc, "order": order, "present": present, "count": count, "prob": mass[:, :, :top].contiguous()}

    @staticmethod
    def _unit_scale(units, d):
        """(ux, uy, f) of units "px", "norm" or a float: ux, uy turn a normalised difference into the unit, f turns a length in pixels into it
        ("norm": along x)."""
        if units == "norm":
            return 1.0, 1.0, d.sx
        f = 1.0 if units == "px" else float(units)
        return f / d.sx, f / d.sy, f

    def evaluate_ranked(self, Y, score, fut_windows, top: Optional[int] = None, horizons=None, units="px", select: str = "score", nms_radius=None,
                        nms_metric: str = "final", nms_horizon=None, return_count: bool = False) -> np.ndarray:
        """[A, n_h, 4] = per horizon (ADE, FDE of the best-scored sample, best ADE, best FDE among the `top` best-scored samples) over the
        target frames before the horizon the object is present in; zeros where there is none.  horizons in frames (default
        default_horizons(T_pred)), top default default_top(K); units "px" (pixels), "norm" (normalised units, evaluate()'s) or a float f
        = f x pixels (0.2: the paper's 1/5 resolution).  `fut_windows` as in evaluate().
        select="nms" (nms_radius in pixels, nms_metric, nms_horizon as in predict_device): the order by score goes through the non-maximum
        suppression first, so columns 2 and 3 become "best of the `top` most plausible distinct futures" (columns 0 and 1 are unchanged: the
        best-scored sample is always kept first).  return_count=True: also the number of samples kept per agent [A] (select="nms" only)."""
        h, d, hz, (ux, uy, _), fut, stream = self._evaluation(Y, fut_windows, horizons, units)
        nms = self._nms_args(select, nms_radius, nms_metric, nms_horizon, d.T_pred)
        if return_count and nms is None:
            raise ValueError("return_count needs select='nms'")
        top = default_top(d.K) if top is None else int(top)
        out = self.torch.empty((d.A, len(hz), 4), device=self.device, dtype=self.torch.float32)
        order, count = self._order(h, Y, score, top, nms)
        h.ranked_errors(Y.data_ptr(), fut.data_ptr(), order.data_ptr(), top, hz, ux, uy, out.data_ptr(), stream)
        return (out.cpu().numpy(), count.cpu().numpy()) if return_count else out.cpu().numpy()

    def evaluate_joint(self, Y, score, fut_windows, top: Optional[int] = None, horizons=None, units="px", collision_radius=None, select: str = "score",
                       worlds_radius=None, worlds_metric: str = "final", worlds_reduce: str = "mean", worlds_horizon=None,
                       collision_penalty: float = 0.0) -> dict:
        """The K samples of every window as K JOINT futures of the scene (desire_joint_metrics).  Returns numpy arrays: "jerr" [n, K, n_h, 2] =
        (JADE_h, JFDE_h): the mean over the agents that take part before the horizon of each agent's ADE_h / FDE_h under sample k; "jscore" [n, K] the
        scores summed over the agents that take part; "order" [n, K] the joint samples by descending joint score; "out" [n, n_h, 4] = (JADE, JFDE
        of the best-scored joint sample, best JADE, best JFDE among the `top` best-scored); "first" [n, K + 1, mno] int32 the first frame at which an
        agent comes within collision_radius of another agent of the same joint sample (T_pred: never), row K being the ground truth under the same
        rule; "cnt" [n, K + 1, n_h, 2] int32 = (agents touching, agents taking part) before each horizon -- the collision rate is cnt[..., 0] /
        cnt[..., 1].  units, horizons, top and `fut_windows` as in evaluate_ranked; collision_radius in pixels, converted to the call's unit (units
        "norm": along x); None: radius 0, nothing touches.
        select="worlds" (worlds_radius in pixels, worlds_metric, worlds_reduce, worlds_horizon, collision_penalty as in predict_device; an agent takes
        part when it has a counted frame; the penalty counts the collisions before the last horizon): the joint samples also go through
        desire_select_worlds, and the dict gains "worder" [n, K] (the kept worlds, then the suppressed ones), "wcount" [n], "wprob" [n, K] (the mass
        each kept world absorbed), "wlabel" [n, K] (the keeping position of every world's owner) and "out_distinct" [n, n_h, 2] = the best JADE, and
        the best JFDE, among the `top` first worlds of "worder" (a NaN is kept, as in "out")."""
        torch = self.torch
        if select not in ("score", "worlds"):
            raise ValueError("select must be 'score' (the best-scored joint samples) or 'worlds' (the distinct ones too), got %r" % (select,))
        h, d, hz, (ux, uy, f), fut, stream = self._evaluation(Y, fut_windows, horizons, units)
        wargs = self._worlds_args(select, worlds_radius, worlds_metric, worlds_reduce, worlds_horizon, collision_penalty, d.T_pred)
        n = d.n_scenes
        top = default_top(d.K) if top is None else int(top)
        radius = (0.0 if collision_radius is None else float(collision_radius)) * f
        dev, i32 = self.device, torch.int32
        res = {"jerr": torch.empty((n, d.K, len(hz), 2), device=dev), "out": torch.empty((n, len(hz), 4), device=dev),
               "order": torch.empty((n, d.K), device=dev, dtype=i32), "jscore": torch.empty((n, d.K), device=dev),
               "cnt": torch.empty((n, d.K + 1, len(hz), 2), device=dev, dtype=i32), "first": torch.empty((n, d.K + 1, d.mno), device=dev, dtype=i32)}
        h.joint_metrics(Y.data_ptr(), fut.data_ptr(), 0, _ptr(score), hz, top, radius, ux, uy, res["cnt"].data_ptr(),
                        res["order"].data_ptr(), res["first"].data_ptr(), res["jerr"].data_ptr(), res["jscore"].data_ptr(), res["out"].data_ptr(), stream)
        if wargs is not None:
            part8 = (fut[..., 0] != 0).any(1).to(torch.uint8).contiguous()    # [n, mno]: a counted frame before T_pred
            res["worder"], res["wcount"], res["wprob"], res["wlabel"] = self._select_worlds(h, Y, part8, res["jscore"], res["cnt"][:, :d.K, -1, 0], wargs,
                                                                                            wargs[3] * f, ux, uy)
            idx = res["worder"][:, :top].long()
            je = res["jerr"][torch.arange(n, device=dev)[:, None], idx]      # [n, top, n_h, 2]
            low = je.min(1).values
            res["out_distinct"] = torch.where(torch.isnan(je).any(1), torch.full_like(low, float("nan")), low)
        return {k: v.cpu().numpy() for k, v in res.items()}

    def _plan_risk(self, h, Y, fut, present, score, plans, ego, hz, radius, ux, uy):
        """One desire_plan_risk call on device tensors: plans [n, M, T_pred, 2] normalised, ego [n, M] int32 or None.  Device tensors back."""
        torch = self.torch
        d = h.dims
        n, M, nh = d.n_scenes, int(plans.shape[1]), len(hz)
        dev, i32 = self.device, torch.int32
        res = {"risk": torch.empty((n, M, nh), device=dev), "first": torch.empty((n, M, d.K + 1), device=dev, dtype=i32),
               "clear": torch.empty((n, M, d.K + 1, nh), device=dev), "blame": torch.empty((n, M, nh, d.mno), device=dev)}
        h.plan_risk(Y.data_ptr(), _ptr(fut), _ptr(present), _ptr(score), plans.data_ptr(), _ptr(ego), M, hz, radius, ux, uy, res["risk"].data_ptr(),
                    res["first"].data_ptr(), res["clear"].data_ptr(), res["blame"].data_ptr(), torch.cuda.current_stream().cuda_stream)
        return res

    def _plan_risk_cond(self, h, Y, fut, present, score, plans, ego, hz, radius, ux, uy, sigma, t_cond):
        """One desire_plan_risk_cond call on device tensors (_plan_risk's arguments; sigma in the unit of the radius): _plan_risk's tensors, then
        "cw" and "dist" [n, M, K], "ess" and "support" [n, M] and "cond" [n, M] int32."""
        torch = self.torch
        d = h.dims
        n, M, nh = d.n_scenes, int(plans.shape[1]), len(hz)
        dev, i32 = self.device, torch.int32
        res = {"risk": torch.empty((n, M, nh), device=dev), "first": torch.empty((n, M, d.K + 1), device=dev, dtype=i32),
               "clear": torch.empty((n, M, d.K + 1, nh), device=dev), "blame": torch.empty((n, M, nh, d.mno), device=dev),
               "cw": torch.empty((n, M, d.K), device=dev), "dist": torch.empty((n, M, d.K), device=dev), "ess": torch.empty((n, M), device=dev),
               "support": torch.empty((n, M), device=dev), "cond": torch.empty((n, M), device=dev, dtype=i32)}
        h.plan_risk_cond(Y.data_ptr(), _ptr(fut), _ptr(present), _ptr(score), plans.data_ptr(), _ptr(ego), M, hz, radius, ux, uy, sigma, t_cond,
                         res["risk"].data_ptr(), res["cw"].data_ptr(), res["first"].data_ptr(), res["clear"].data_ptr(), res["blame"].data_ptr(),
                         res["dist"].data_ptr(), res["ess"].data_ptr(), res["support"].data_ptr(), res["cond"].data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
        return res

    @staticmethod
    def _condition_args(d, condition_sigma, condition_horizon):
        """(sigma in pixels, t_cond) of a conditioned call, refused here where they are bad (before a forward runs)."""
        if condition_sigma is None or not (np.isfinite(float(condition_sigma)) and float(condition_sigma) > 0):
            raise ValueError("condition=True needs condition_sigma: pixels, finite and > 0 (the RMS deviation per frame), got %r" % (condition_sigma,))
        t_cond = d.T_pred if condition_horizon is None else int(condition_horizon)
        if not 1 <= t_cond <= d.T_pred:
            raise ValueError("condition_horizon must be 1..pred_length, got %r" % (condition_horizon,))
        return float(condition_sigma), t_cond

    def _prior_risk(self, d, first, score, part, hz):
        """desire_plan_risk's risk stated in torch on the small tensors: first [n, M, >= K] int32, score [R] or None, part [n, mno] bool (the slots
        taking part).  [n, M, n_h]."""
        torch = self.torch
        n = d.n_scenes
        W = torch.full((n, d.K), 1.0 / d.K, device=self.device)
        if score is not None:
            s = score.reshape(n, d.K, d.mno)
            js = torch.where(part[:, None, :], s, torch.zeros_like(s)).sum(-1)
            fin = torch.isfinite(js).all(-1, keepdim=True)
            W = torch.where(fin, torch.softmax(torch.where(fin, js, torch.zeros_like(js)), -1), W)
        hit = first[:, :, :d.K, None] < torch.tensor(hz, device=self.device, dtype=torch.int32)[None, None, None]
        return (hit.to(torch.float32) * W[:, None, :, None]).sum(2)

    def score_plans(self, past, plans, collision_radius, horizons=None, ego_slot=None, weights: str = "score", condition: bool = False,
                    condition_sigma=None, condition_horizon=None, **predict_kwargs) -> dict:
        """M candidate trajectories of the planner's own vehicle per window against the K joint futures the model predicts: the forward as
        predict_device runs it (predict_kwargs: eps, seed, grid_of_scene, device_rng, window_base), then one desire_plan_risk call in its
        prediction form (an agent counts when its id is != 0 at the last observed frame).  `past`: loader windows [T_obs, MNO, 3] or
        predict_device's tensor; plans [n, M, T_pred, 2] IN PIXELS (scaled like the observed positions; a NaN frame: the plan is not defined
        there); collision_radius in pixels, finite and >= 0; ego_slot [n, M] (or [n]: one slot for every plan of the window) = the slot the plan
        replaces, negative or None: nobody.  Returns device tensors: "risk" [n, M, n_h] = the weight of the joint futures in which the plan comes
        within the radius of somebody before the horizon (weights "score": softmax of the joint scores; "uniform": 1 / K), "clearance"
        [n, M, K, n_h] = the smallest distance in pixels to anybody before the horizon (inf: nobody there), "first" [n, M, K] int32 = the frame
        of the first contact (T_pred: none), "blame" [n, M, n_h, mno] = the risk by the agent touched, "present" [n, mno] and "best" [n, n_h] =
        per horizon the plan of least risk, ties to the greater clearance (its smallest over the K futures), then to the lower index.
        condition=True (needs ego_slot and condition_sigma, pixels: the RMS deviation per frame a joint future's own sample of the ego may have
        from the plan; condition_horizon: the frames compared, default all): one desire_plan_risk_cond call instead -- "risk", "blame" and
        "best" are then GIVEN that the ego drives the plan (the joint futures reweighted by how well their ego sample agrees with it), and the
        dict also holds "cond_weights" [n, M, K], "plan_distance" [n, M, K] (pixels RMS), "ess" [n, M] (the effective number of joint futures
        behind the answer), "support" [n, M] (how well the predicted ego supports the plan, in (0, 1]), "conditioned" [n, M] bool and
        "risk_prior" [n, M, n_h], the unconditioned risk."""
        torch = self.torch
        _check_weights(weights, "joint")
        _check_radius(collision_radius)
        past, h, present, pres8 = self._prediction(past, u8=True)
        n, d = int(past.shape[0]), h.dims
        hz = self._horizons(d, horizons)
        if condition:
            if ego_slot is None:
                raise ValueError("condition=True needs ego_slot (the slot whose predicted samples are compared with the plan)")
            sigma, t_cond = self._condition_args(d, condition_sigma, condition_horizon)
        P = torch.as_tensor(plans, device=self.device).to(torch.float32)
        if P.dim() != 4 or int(P.shape[0]) != n or int(P.shape[1]) < 1 or tuple(P.shape[2:]) != (d.T_pred, 2):
            raise ValueError("plans must be [n, M, T_pred, 2] in pixels with M >= 1, got %s" % (tuple(P.shape),))
        M = int(P.shape[1])
        P = (P * self._scale(d)).contiguous()
        ego = None
        if ego_slot is not None:
            ego = torch.as_tensor(ego_slot, device=self.device).to(torch.int32)
            ego = (ego[:, None].expand(n, M) if ego.dim() == 1 else ego).contiguous()
            if tuple(ego.shape) != (n, M):
                raise ValueError("ego_slot must be [n, M] or [n], got %s" % (tuple(ego.shape),))
        Y, score = self.forward_device(past, None, **predict_kwargs)
        sc = score if weights == "score" else None
        if condition:
            res = self._plan_risk_cond(h, Y, None, pres8, sc, P, ego, hz, float(collision_radius), 1.0 / d.sx, 1.0 / d.sy, sigma, t_cond)
        else:
            res = self._plan_risk(h, Y, None, pres8, sc, P, ego, hz, float(collision_radius), 1.0 / d.sx, 1.0 / d.sy)
        clearance = res["clear"][:, :, :d.K].sqrt()
        worst = clearance.min(2).values                                        # [n, M, n_h]
        least = res["risk"] == res["risk"].min(1, keepdim=True).values
        room = torch.where(least, worst, torch.full_like(worst, -1.0))
        pick = least & (room == room.max(1, keepdim=True).values)
        idx = torch.arange(M, device=self.device)[None, :, None].expand_as(pick)
        best = torch.where(pick, idx, torch.full_like(idx, M)).min(1).values
        out = {"risk": res["risk"], "clearance": clearance, "first": res["first"][:, :, :d.K].contiguous(), "blame": res["blame"],
               "present": present, "best": best}
        if condition:
            out.update({"cond_weights": res["cw"], "plan_distance": res["dist"].sqrt(), "ess": res["ess"], "support": res["support"],
                        "conditioned": res["cond"] > 0, "risk_prior": self._prior_risk(d, res["first"], sc, pres8.reshape(n, d.mno) != 0, hz)})
        return out

    def evaluate_plan_risk(self, Y, score, fut_windows, collision_radius, horizons=None, weights: str = "score", condition: bool = False,
                           condition_sigma=None, condition_horizon=None) -> dict:
        """Leave-one-out check of the predicted interactions that needs no planner: plan m of a window is what agent m actually did (its
        recorded future, undefined where it is not counted), replacing slot m, held against the K joint futures of the others.  Returns numpy
        arrays: "risk" [n, mno, n_h] = the predicted risk of what each agent did, "first" [n, mno, K + 1] int32 (row K: against the recorded
        futures of the others), "takes_part" [n, mno, n_h] bool, and per horizon over the agents taking part before it "predicted" [n_h] = the
        mean predicted risk, "actual" [n_h] = the rate at which they actually came within collision_radius (pixels) of somebody, "agents" [n_h].
        A predictor that is calibrated about interactions brings the two columns close.  condition=True (condition_sigma in pixels;
        condition_horizon: the frames compared, default all) adds a desire_plan_risk_cond call: "risk_given" [n, mno, n_h] = the risk GIVEN what
        agent m did (the joint futures reweighted by how close their own sample of slot m came to it), "ess" [n, mno], and per horizon over
        the same agents "predicted_given" [n_h] and "ess_mean" [n_h].  A model that captures interactions predicts the contacts of the others
        better once it is told what agent m really did: predicted_given then lies closer to actual than predicted does."""
        torch = self.torch
        _check_weights(weights, "joint")
        h, d, hz, _, fut, _ = self._evaluation(Y, fut_windows, horizons)
        n = d.n_scenes
        if condition:
            sigma, t_cond = self._condition_args(d, condition_sigma, condition_horizon)
        counted = (fut[..., 0] != 0).permute(0, 2, 1)                          # [n, mno, T_pred]
        g = (fut[..., 1:] * self._scale(d)).permute(0, 2, 1, 3)
        plans = torch.where(counted[..., None], g, torch.full_like(g, float("nan"))).contiguous()
        ego = torch.arange(d.mno, device=self.device, dtype=torch.int32)[None].expand(n, d.mno).contiguous()
        res = self._plan_risk(h, Y, fut, None, score if weights == "score" else None, plans, ego, hz, float(collision_radius), 1.0 / d.sx, 1.0 / d.sy)
        takes = torch.stack([counted[:, :, :x].any(-1) for x in hz], -1)       # [n, mno, n_h]
        hit = res["first"][:, :, d.K, None] < torch.tensor(hz, device=self.device, dtype=torch.int32)[None, None]
        agents = takes.sum((0, 1)).to(torch.float64)
        predicted = torch.where(takes, res["risk"], torch.zeros_like(res["risk"])).to(torch.float64).sum((0, 1))
        actual = (takes & hit).sum((0, 1)).to(torch.float64)
        den = agents.clamp(min=1)
        out = {"risk": res["risk"].cpu().numpy(), "first": res["first"].cpu().numpy(), "takes_part": takes.cpu().numpy(),
               "predicted": (predicted / den).cpu().numpy(), "actual": (actual / den).cpu().numpy(), "agents": agents.cpu().numpy().astype(np.int64)}
        if condition:
            cres = self._plan_risk_cond(h, Y, fut, None, score if weights == "score" else None, plans, ego, hz, float(collision_radius), 1.0 / d.sx,
                                        1.0 / d.sy, sigma, t_cond)
            given = torch.where(takes, cres["risk"], torch.zeros_like(cres["risk"])).to(torch.float64).sum((0, 1))
            ess = torch.where(takes, cres["ess"][..., None].expand_as(takes), torch.zeros_like(cres["risk"])).to(torch.float64).sum((0, 1))
            out.update({"risk_given": cres["risk"].cpu().numpy(), "ess": cres["ess"].cpu().numpy(), "predicted_given": (given / den).cpu().numpy(),
                        "ess_mean": (ess / den).cpu().numpy()})
        return out

    @staticmethod
    def _modes_args(d, modes, seeds, nms_radius, iters, min_std, weights):
        """(n_modes, iters) of the mode calls, refused here where they are bad (before a forward runs)."""
        n = int(modes)
        if not 1 <= n <= min(d.K, _lib.MODES_MAX):
            raise ValueError("modes must be 1..min(num_samples, %d), got %d" % (_lib.MODES_MAX, n))
        if seeds not in ("nms", "score"):
            raise ValueError("seeds must be 'nms' (the mutually distinct samples first) or 'score' (the best-scored samples), got %r" % (seeds,))
        if seeds == "nms" and nms_radius is None:
            raise ValueError("seeds='nms' needs nms_radius (pixels)")
        if not 0 <= int(iters) <= _lib.MODES_MAX_ITERS:
            raise ValueError("iters must be 0..%d, got %r" % (_lib.MODES_MAX_ITERS, iters))
        if not (np.isfinite(float(min_std)) and float(min_std) >= 0):
            raise ValueError("min_std must be finite and >= 0 (pixels), got %r" % (min_std,))
        _check_weights(weights, "IOC")
        return n, int(iters)

    def _fit_modes(self, h, Y, score, fut, n, nms, iters, t_end, ux, uy, var_floor, weighted, hz=None, log_floor=_lib.KDE_LOG_FLOOR):
        """Rank (and the non-maximum suppression with seeds "nms": nms given), then one desire_fit_modes call, on device tensors.  Device tensors back, shaped
        per window and slot."""
        torch = self.torch
        d = h.dims
        dev, i32 = self.device, torch.int32
        N, m = d.n_scenes, d.mno
        order, _ = self._order(h, Y, score, n, nms)
        res = {"mean": torch.empty((N, m, n, d.T_pred, 2), device=dev), "cov": torch.empty((N, m, n, d.T_pred, 3), device=dev),
               "prob": torch.empty((N, m, n), device=dev), "label": torch.empty((N, m, d.K), device=dev, dtype=i32),
               "count": torch.empty((N, m, n), device=dev, dtype=i32), "passes": torch.empty((N, m), device=dev, dtype=i32)}
        if fut is not None:
            res["nll"] = torch.empty((N, m, len(hz), 2), device=dev)
        h.fit_modes(Y.data_ptr(), order.data_ptr(), score.data_ptr() if weighted else 0, n, t_end, iters, ux, uy, var_floor, res["count"].data_ptr(),
                    res["prob"].data_ptr(), res["label"].data_ptr(), res["mean"].data_ptr(), res["cov"].data_ptr(), res["passes"].data_ptr(),
                    _ptr(fut), hz, float(log_floor), _ptr(res.get("nll")), 0, torch.cuda.current_stream().cuda_stream)
        return res

    def predict_modes(self, past, modes: int = 6, seeds: str = "nms", nms_radius=None, nms_metric: str = "final", iters: int = 8,
                      min_std: float = 1.0, horizon=None, weights: str = "score", **predict_kwargs) -> dict:
        """A small mixture per agent, the form trackers, planners and the benchmark formats take: the forward as predict_device runs it
        (predict_kwargs: eps, seed, grid_of_scene, device_rng, window_base), the ranking by IOC score (and, with seeds "nms", the score-ordered
        non-maximum suppression at nms_radius pixels by nms_metric, so that the seeds are mutually distinct samples), then one desire_fit_modes
        call: a weighted Lloyd iteration of at most `iters` passes from the first `modes` samples of that order, the assignment looking at the
        first `horizon` frames (None: all).  `past`: loader windows [T_obs, MNO, 3] or predict_device's tensor.  Returns device tensors: "mean"
        [n, mno, modes, T_pred, 2] IN PIXELS, "cov" [n, mno, modes, T_pred, 3] = (Cxx, Cyy, Cxy) in px^2 with min_std^2 (pixels) added to the
        diagonal, "prob" [n, mno, modes] = the weight of a mode's members (weights "score": softmax of the IOC scores; "uniform": 1 / K), "label"
        [n, mno, K] int32 = the mode of every sample, "count" [n, mno, modes] int32, "passes" [n, mno] int32 and "present" [n, mno] bool.  All K
        samples and scores stay available as self.final_output / self.final_states."""
        past, h, present, _ = self._prediction(past)
        d = h.dims
        n, iters = self._modes_args(d, modes, seeds, nms_radius, iters, min_std, weights)     # refused before the forward runs
        nms = self._nms_args("nms", nms_radius, nms_metric, horizon, d.T_pred) if seeds == "nms" else None
        t_end = d.T_pred if horizon is None else int(horizon)
        if not 1 <= t_end <= d.T_pred:
            raise ValueError("horizon must be 1..pred_length (%d), got %d" % (d.T_pred, t_end))
        Y, score = self.forward_device(past, None, **predict_kwargs)
        res = self._fit_modes(h, Y, score, None, n, nms, iters, t_end, 1.0 / d.sx, 1.0 / d.sy, float(min_std) ** 2, weights == "score")
        res["mean"] /= self._scale(d)
        res["present"] = present
        return res

    def evaluate_modes(self, Y, score, fut_windows, modes: int = 6, seeds: str = "nms", nms_radius=None, nms_metric: str = "final", iters: int = 8,
                       min_std: float = 1.0, horizon=None, weights: str = "score", horizons=None, units="px",
                       log_floor: float = _lib.KDE_LOG_FLOOR) -> dict:
        """The mixture predict_modes hands out, held against the ground truth.  Returns numpy arrays per agent a = window * mno + slot: "nll"
        [A, n_h, 2] = per horizon the (mean, final-frame) negative log-likelihood of the ground truth under the agent's mixture (density per
        unit^2, the log clipped below at log_floor, as evaluate_nll reports the KDE's), "top1" [A, n_h, 2] = (ADE, FDE) of the most probable
        mode's mean, "best" [A, n_h, 2] = the minimum over the modes with mass of their means' ADE, and of their FDE; zeros where the agent has no
        counted frame before the horizon; and "prob" [A, modes], "count" [A, modes], "passes" [A].  units, horizons and `fut_windows` as in
        evaluate_ranked; min_std and nms_radius in pixels."""
        torch = self.torch
        h, d, hz, (ux, uy, f), fut, _ = self._evaluation(Y, fut_windows, horizons, units)
        n, iters = self._modes_args(d, modes, seeds, nms_radius, iters, min_std, weights)
        nms = self._nms_args("nms", nms_radius, nms_metric, horizon, d.T_pred) if seeds == "nms" else None
        t_end = d.T_pred if horizon is None else int(horizon)
        res = self._fit_modes(h, Y, score, fut, n, nms, iters, t_end, ux, uy, (float(min_std) * f) ** 2, weights == "score", hz, log_floor)
        # the errors of the means: torch on the small [A, n, T, 2] tensor
        mean = res["mean"].reshape(d.A, n, d.T_pred, 2)
        prob = res["prob"].reshape(d.A, n)
        counted = (fut[..., 0] != 0).permute(0, 2, 1).reshape(d.A, d.T_pred)
        g = (fut[..., 1:] * self._scale(d)).permute(0, 2, 1, 3).reshape(d.A, 1, d.T_pred, 2)
        e = (((mean - g) * torch.tensor([ux, uy], device=self.device, dtype=torch.float32)) ** 2).sum(-1).sqrt()      # [A, n, T]
        e = torch.where(counted[:, None], e, torch.zeros_like(e))
        top = prob.argmax(1)
        alive = prob > 0
        inf = torch.full((), float("inf"), device=self.device)
        top1, best = torch.zeros((d.A, len(hz), 2), device=self.device), torch.zeros((d.A, len(hz), 2), device=self.device)
        ar = torch.arange(d.A, device=self.device)
        for i, x in enumerate(hz):
            c = counted[:, :x]
            np_ = c.sum(1)
            last = (c * torch.arange(1, x + 1, device=self.device)).argmax(1)                                         # the last counted frame < x
            ade = e[:, :, :x].sum(2) / np_.clamp(min=1)[:, None]
            fde = e[ar, :, last]
            has = (np_ > 0) & alive.any(1)
            both = torch.stack([ade, fde], -1)                                                                        # [A, n, 2]
            top1[:, i] = torch.where(has[:, None], both[ar, top], torch.zeros_like(top1[:, i]))
            low = torch.where(alive[:, :, None], both, inf).min(1).values
            best[:, i] = torch.where(has[:, None], low, torch.zeros_like(low))
        return {"nll": res["nll"].reshape(d.A, len(hz), 2).cpu().numpy(), "top1": top1.cpu().numpy(), "best": best.cpu().numpy(),
                "prob": prob.cpu().numpy(), "count": res["count"].reshape(d.A, n).cpu().numpy(), "passes": res["passes"].reshape(d.A).cpu().numpy()}

    def _scene_modes_args(self, d, modes, seeds, worlds_radius, worlds_metric, worlds_reduce, iters, min_std, horizon, weights, collision_radius,
                          collision_penalty):
        """(n_modes, iters, t_end, _worlds_args' tuple or None) of the scene-mode calls, refused here where they are bad (before a forward runs)."""
        n = int(modes)
        if not 1 <= n <= min(d.K, _lib.MODES_MAX):
            raise ValueError("modes must be 1..min(num_samples, %d), got %d" % (_lib.MODES_MAX, n))
        if seeds not in ("worlds", "score"):
            raise ValueError("seeds must be 'worlds' (the mutually distinct joint samples first) or 'score' (the best-scored joint samples), got %r"
                             % (seeds,))
        if not 0 <= int(iters) <= _lib.MODES_MAX_ITERS:
            raise ValueError("iters must be 0..%d, got %r" % (_lib.MODES_MAX_ITERS, iters))
        if not (np.isfinite(float(min_std)) and float(min_std) >= 0):
            raise ValueError("min_std must be finite and >= 0 (pixels), got %r" % (min_std,))
        _check_weights(weights, "joint")
        t_end = d.T_pred if horizon is None else int(horizon)
        if not 1 <= t_end <= d.T_pred:
            raise ValueError("horizon must be 1..pred_length (%d), got %d" % (d.T_pred, t_end))
        if collision_radius is not None:
            _check_radius(collision_radius)
        if seeds == "score":
            if worlds_radius is not None or worlds_metric != "final" or worlds_reduce != "mean" or collision_penalty != 0.0:
                raise ValueError("worlds_radius, worlds_metric, worlds_reduce and collision_penalty belong to seeds='worlds'")
            return n, int(iters), t_end, None
        if worlds_radius is None:
            raise ValueError("seeds='worlds' needs worlds_radius (pixels)")
        return n, int(iters), t_end, self._worlds_args("worlds", worlds_radius, worlds_metric, worlds_reduce, horizon, collision_penalty, d.T_pred)

    def _fit_scene_modes(self, h, Y, score, fut, part8, n, wargs, iters, t_end, ux, uy, f, var_floor, weighted, collision_radius, hz=None,
                         log_floor=_lib.KDE_LOG_FLOOR):
        """The joint scores and their order (desire_joint_metrics), with wargs the non-maximum suppression of the worlds (desire_select_worlds), then
        one desire_fit_scene_modes call, on device tensors; f turns a length in pixels into the call's unit.  Device tensors back, per window."""
        torch = self.torch
        d = h.dims
        dev, i32 = self.device, torch.int32
        N, stream = d.n_scenes, torch.cuda.current_stream().cuda_stream
        nh = 1 if fut is None else len(hz)
        cnt = torch.empty((N, d.K + 1, nh, 2), device=dev, dtype=i32)
        wscore, order = torch.empty((N, d.K), device=dev), torch.empty((N, d.K), device=dev, dtype=i32)
        h.joint_metrics(Y.data_ptr(), _ptr(fut), 0 if fut is not None else part8.data_ptr(), score.data_ptr(), [d.T_pred] if fut is None else hz, n,
                        float(collision_radius or 0.0) * f, ux, uy, cnt.data_ptr(), order.data_ptr(), 0, 0, wscore.data_ptr(), 0, stream)
        if wargs is not None:
            if wargs[4] != 0.0:                                             # the penalty per colliding agent, as _select_worlds forms it
                wscore = (wscore - cnt[:, :d.K, -1, 0].to(torch.float32) * wargs[4]).contiguous()
            order = self._select_worlds(h, Y, part8, wscore, None, wargs[:4] + (0.0,), wargs[3] * f, ux, uy)[0]
        res = {"mean": torch.empty((N, n, d.mno, d.T_pred, 2), device=dev), "cov": torch.empty((N, n, d.mno, d.T_pred, 3), device=dev),
               "prob": torch.empty((N, n), device=dev), "label": torch.empty((N, d.K), device=dev, dtype=i32),
               "count": torch.empty((N, n), device=dev, dtype=i32), "passes": torch.empty((N,), device=dev, dtype=i32)}
        if fut is not None:
            res["nll"] = torch.empty((N, nh, 2), device=dev)
        h.fit_scene_modes(Y.data_ptr(), part8.data_ptr(), order.data_ptr(), wscore.data_ptr() if weighted else 0, n, t_end, iters, ux, uy, var_floor,
                          res["count"].data_ptr(), res["prob"].data_ptr(), res["label"].data_ptr(), res["mean"].data_ptr(), res["cov"].data_ptr(),
                          res["passes"].data_ptr(), _ptr(fut), hz, float(log_floor), _ptr(res.get("nll")), 0, stream)
        return res

    def predict_scene_modes(self, past, modes: int = 6, seeds: str = "worlds", worlds_radius=None, worlds_metric: str = "final",
                            worlds_reduce: str = "mean", iters: int = 8, min_std: float = 1.0, horizon=None, weights: str = "score",
                            collision_radius=None, collision_penalty: float = 0.0, **predict_kwargs) -> dict:
        """A small mixture per WINDOW, the form joint consumers take: `modes` scene modes, one probability per mode and, for every agent of that
        mode, a mean trajectory and a covariance per frame, consistent across the agents -- a mode is a set of joint samples (sample k of every
        agent together), never agent A's left turn next to agent B's incompatible one.  The forward as predict_device runs it (predict_kwargs:
        eps, seed, grid_of_scene, device_rng, window_base), the joint scores and their order (desire_joint_metrics), with seeds "worlds" the
        score-ordered non-maximum suppression of the joint samples (desire_select_worlds at worlds_radius pixels by worlds_metric / worlds_reduce,
        as predict_device's select="worlds"; collision_penalty P ranks by joint score - P * agents that collide within collision_radius pixels),
        then one desire_fit_scene_modes call: a weighted Lloyd iteration on whole joint samples of at most `iters` passes from the first `modes`
        of that order, the assignment looking at the first `horizon` frames (None: all) of the agents present at the last observed frame.
        Returns device tensors: "mean" [n, modes, mno, T_pred, 2] IN PIXELS, "cov" [n, modes, mno, T_pred, 3] = (Cxx, Cyy, Cxy) in px^2 with
        min_std^2 added to the diagonal (zeros for an absent agent), "prob" [n, modes] = the weight of a mode's joint samples (weights "score":
        softmax of the joint scores; "uniform": 1 / K), "label" [n, K] int32 = the mode of every joint sample, "count" [n, modes] int32, "passes"
        [n] int32 and "present" [n, mno] bool.  All K samples and scores stay available as self.final_output / self.final_states."""
        past, h, present, pres8 = self._prediction(past, u8=True)
        d = h.dims
        n, iters, t_end, wargs = self._scene_modes_args(d, modes, seeds, worlds_radius, worlds_metric, worlds_reduce, iters, min_std, horizon, weights,
                                                        collision_radius, collision_penalty)       # refused before the forward runs
        Y, score = self.forward_device(past, None, **predict_kwargs)
        res = self._fit_scene_modes(h, Y, score, None, pres8, n, wargs, iters, t_end, 1.0 / d.sx, 1.0 / d.sy, 1.0, float(min_std) ** 2,
                                    weights == "score", collision_radius)
        res["mean"] /= self._scale(d)
        res["present"] = present
        return res

    def evaluate_scene_modes(self, Y, score, fut_windows, modes: int = 6, seeds: str = "worlds", worlds_radius=None, worlds_metric: str = "final",
                             worlds_reduce: str = "mean", iters: int = 8, min_std: float = 1.0, horizon=None, weights: str = "score",
                             collision_radius=None, collision_penalty: float = 0.0, horizons=None, units="px",
                             log_floor: float = _lib.KDE_LOG_FLOOR) -> dict:
        """The mixture predict_scene_modes hands out, held against the ground truth (an agent takes part when it has a counted frame).  Returns
        numpy arrays per window: "nll" [n, n_h, 2] = per horizon the (mean over the frames, final-frame) negative JOINT log-likelihood of the
        ground truth under the window's mixture -- log sum_modes p_m prod_agents N(g | mean, cov) -- PER AGENT counted in the frame (density per
        unit^2, the per-agent log clipped below at log_floor): comparable with evaluate_modes' "nll", and below the agents' mean of it exactly
        when the mixture captures their interaction; "top1" [n, n_h, 2] = (JADE, JFDE) of the most probable mode's means (the mean over the
        agents taking part before the horizon of each agent's ADE / FDE, as evaluate_joint's), "best" [n, n_h, 2] = the minimum over the modes
        with mass of their JADE, and of their JFDE; zeros where nobody takes part before the horizon; and "prob" [n, modes], "count" [n, modes],
        "passes" [n].  units, horizons and `fut_windows` as in evaluate_ranked; min_std, worlds_radius and collision_radius in pixels."""
        torch = self.torch
        h, d, hz, (ux, uy, f), fut, _ = self._evaluation(Y, fut_windows, horizons, units)
        n, iters, t_end, wargs = self._scene_modes_args(d, modes, seeds, worlds_radius, worlds_metric, worlds_reduce, iters, min_std, horizon, weights,
                                                        collision_radius, collision_penalty)
        counted = (fut[..., 0] != 0).permute(0, 2, 1)                          # [n, mno, T_pred]
        part8 = counted.any(2).to(torch.uint8).contiguous()
        res = self._fit_scene_modes(h, Y, score, fut, part8, n, wargs, iters, t_end, ux, uy, f, (float(min_std) * f) ** 2, weights == "score",
                                    collision_radius, hz, log_floor)
        # the errors of the means: torch on the small [n, modes, mno, T, 2] tensor
        N, dev = d.n_scenes, self.device
        g = (fut[..., 1:] * self._scale(d)).permute(0, 2, 1, 3)[:, None]       # [n, 1, mno, T, 2]
        e = (((res["mean"] - g) * torch.tensor([ux, uy], device=dev, dtype=torch.float32)) ** 2).sum(-1).sqrt()      # [n, modes, mno, T]
        e = torch.where(counted[:, None], e, torch.zeros_like(e))
        top = res["prob"].argmax(1)
        alive = res["prob"] > 0
        inf = torch.full((), float("inf"), device=dev)
        top1, best = torch.zeros((N, len(hz), 2), device=dev), torch.zeros((N, len(hz), 2), device=dev)
        ar = torch.arange(N, device=dev)
        for i, x in enumerate(hz):
            c = counted[:, :, :x]
            np_ = c.sum(2)                                                      # [n, mno] counted frames before the horizon
            takes = np_ > 0
            last = (c * torch.arange(1, x + 1, device=dev)).argmax(2)           # the last counted frame < x
            ade = e[..., :x].sum(3) / np_.clamp(min=1)[:, None]                 # [n, modes, mno]
            fde = e.gather(3, last[:, None, :, None].expand(N, n, d.mno, 1))[..., 0]
            agents = takes.sum(1).clamp(min=1)[:, None]
            both = torch.stack([torch.where(takes[:, None], ade, torch.zeros_like(ade)).sum(2) / agents,
                                torch.where(takes[:, None], fde, torch.zeros_like(fde)).sum(2) / agents], -1)      # [n, modes, 2] = (JADE, JFDE)
            has = takes.any(1) & alive.any(1)
            top1[:, i] = torch.where(has[:, None], both[ar, top], torch.zeros_like(top1[:, i]))
            low = torch.where(alive[:, :, None], both, inf).min(1).values
            best[:, i] = torch.where(has[:, None], low, torch.zeros_like(low))
        return {"nll": res["nll"].cpu().numpy(), "top1": top1.cpu().numpy(), "best": best.cpu().numpy(), "prob": res["prob"].cpu().numpy(),
                "count": res["count"].cpu().numpy(), "passes": res["passes"].cpu().numpy()}

    def _occupancy_args(self, d, grid, horizons, mode, weights, mask, mask_of_window, n):
        """(Oh, Ow, horizons, mode id, mask tensor or None, mask_of_window tensor or None) of the occupancy calls, refused here where they are bad."""
        torch = self.torch
        Oh, Ow = (int(x) for x in grid)
        if mode not in _lib.OCC_MODES:
            raise ValueError("mode must be 'at' (the frame h - 1) or 'until' (any frame before h), got %r" % (mode,))
        _check_weights(weights, "IOC")
        hz = self._horizons(d, horizons)
        if mask is None:
            if mask_of_window is not None:
                raise ValueError("mask_of_window needs mask")
            return Oh, Ow, hz, _lib.OCC_MODES[mode], None, None
        mask = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if mask.dim() == 2:
            mask = mask[None]
        if mask.dim() != 3 or tuple(mask.shape[1:]) != (Oh, Ow):
            raise ValueError("mask must be [n_masks, Oh, Ow] (or [Oh, Ow]) on the occupancy grid, got %s" % (tuple(mask.shape),))
        mow = np.zeros(n, np.int32) if mask_of_window is None else np.asarray(mask_of_window, np.int64).reshape(-1)
        if mow.size != n or (mow >= int(mask.shape[0])).any():
            raise ValueError("mask_of_window must hold one index below n_masks (negative: no mask) per window")
        return Oh, Ow, hz, _lib.OCC_MODES[mode], mask, torch.as_tensor(mow.astype(np.int32), device=self.device)

    def _occupancy(self, h, Y, fut, present, score, args, want_hit):
        torch = self.torch
        d = h.dims
        Oh, Ow, hz, mode, mask, mow = args
        n, nh = d.n_scenes, len(hz)
        res = {"occ": torch.empty((n, nh, Oh, Ow), device=self.device), "expected": torch.empty((n, nh, Oh, Ow), device=self.device),
               "off": torch.empty((n, d.mno, nh), device=self.device)}
        if mask is not None:
            res["violation"] = torch.empty((n, d.mno, nh), device=self.device)
        if want_hit:
            res["hit"] = torch.empty((n, d.mno, nh), device=self.device)
        h.occupancy(Y.data_ptr(), _ptr(fut), _ptr(present), _ptr(score), hz, mode, Oh, Ow, res["occ"].data_ptr(), res["expected"].data_ptr(),
                    _ptr(res.get("hit")), _ptr(res.get("violation")), res["off"].data_ptr(), _ptr(mask), _ptr(mow), torch.cuda.current_stream().cuda_stream)
        return res

    def predict_occupancy(self, past, grid, horizons=None, mode: str = "at", weights: str = "score", mask=None, mask_of_window=None, eps=None,
                          seed: int = 0, grid_of_scene=None, device_rng: bool = False, window_base: int = 0) -> dict:
        """Predicted occupancy maps of windows already in HBM (predict_device's `past`): the forward as predict_device runs it, then one
        desire_occupancy call in its prediction form (an agent counts when its id is != 0 at the last observed frame).  grid = (Oh, Ow) cells over
        the normalised frame.  Returns device tensors: "occ" [n, n_h, Oh, Ow] = the probability that at least one agent is in the cell at frame
        h - 1 (mode "at") or at any frame before h ("until"), "expected" (same shape) = the expected number of agents there, "off" [n, mno, n_h] =
        the weight of an agent's samples that are off the frame, "present" [n, mno] bool and, with mask [n_masks, Oh, Ow] (nonzero: traversable;
        mask_of_window [n]: its mask per window, negative: none; default mask 0 for every window), "violation" [n, mno, n_h] = the weight of the
        samples that enter a cell the mask forbids.  weights "score": softmax of the IOC scores per agent; "uniform": 1 / K.  horizons in frames
        (default default_horizons(T_pred)).  All K samples and scores stay available as self.final_output / self.final_states."""
        past, h, present, pres8 = self._prediction(past, u8=True)
        args = self._occupancy_args(h.dims, grid, horizons, mode, weights, mask, mask_of_window, int(past.shape[0]))      # refused before the forward runs
        Y, score = self.forward_device(past, None, eps, seed, grid_of_scene=grid_of_scene, device_rng=device_rng, window_base=window_base)
        res = self._occupancy(h, Y, None, pres8, score if weights == "score" else None, args, False)
        res["present"] = present
        return res

    def evaluate_occupancy(self, Y, score, fut_windows, grid, horizons=None, mode: str = "at", weights: str = "score", mask=None,
                           mask_of_window=None) -> dict:
        """The occupancy maps of samples Y [n, K, mno, T_pred, 2] (and scores) against their futures: desire_occupancy in its evaluation form (a frame
        counts when the object is in it).  Returns numpy arrays: "occ", "expected", "off" and "violation" as predict_occupancy, and in mode "at"
        "hit" [n, mno, n_h] = the weight of the agent's samples in the cell the ground truth is in at frame h - 1 (0 where it is not counted or off
        the frame).  `fut_windows`, horizons as in evaluate_ranked; weights "score" needs `score`."""
        h, d, _, _, fut, _ = self._evaluation(Y, fut_windows)
        args = self._occupancy_args(d, grid, horizons, mode, weights, mask, mask_of_window, d.n_scenes)
        if weights == "score" and score is None:
            raise ValueError("weights='score' needs the IOC scores")
        res = self._occupancy(h, Y, fut, None, score if weights == "score" else None, args, mode == "at")
        return {k: v.cpu().numpy() for k, v in res.items()}

    def evaluate_offroad(self, Y, score, fut_windows, mask, mask_of_window=None, scale: float = 1.0) -> dict:
        """The off-road read-out of samples Y [n, K, mno, T_pred, 2] read as K joint futures per window, against traversability masks [n_masks, Mh,
        Mw] (or [Mh, Mw]; nonzero: traversable; mask_of_window [n]: its mask per window, negative: none; default mask 0 for every window):
        desire_offroad_loss on the masks' distance field in pixels, the quantities the training term (args.offroad_weight) pushes down.  Returns
        numpy values: "count" [n, K] = the counted (slot, frame)s of world k on a cell off the road, "frames" [n] = the counted (slot, frame)s of
        the window, "rate" [n, K] = count / frames (0 where there are none), "penalty" = the term L_off at `scale` pixels, and the same of the
        ground truth by the same rule -- the op run on the futures laid out as K identical worlds --: "gt_count" [n], "gt_rate" [n],
        "gt_penalty".  `score` is not read (every world counts alike); `fut_windows` as in evaluate_ranked."""
        torch = self.torch
        h, d, _, _, fut, stream = self._evaluation(Y, fut_windows)
        if not (np.isfinite(float(scale)) and float(scale) > 0.0):
            raise ValueError("scale must be finite and > 0 (pixels), got %r" % (scale,))
        mask = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if mask.dim() == 2:
            mask = mask[None]
        if mask.dim() != 3:
            raise ValueError("mask must be [n_masks, Mh, Mw] (or [Mh, Mw]), got %s" % (tuple(mask.shape),))
        nm, Mh, Mw = (int(v) for v in mask.shape)
        mow = np.zeros(d.n_scenes, np.int32) if mask_of_window is None else np.asarray(mask_of_window, np.int64).reshape(-1).astype(np.int32)
        if mow.size != d.n_scenes or (mow >= nm).any():
            raise ValueError("mask_of_window must hold one index below n_masks (negative: no mask) per window")
        field = torch.empty((nm, Mh, Mw), device=self.device, dtype=torch.float32)
        h.mask_distance(mask.data_ptr(), nm, Mh, Mw, (1.0 / d.sx) / Mw, (1.0 / d.sy) / Mh, field.data_ptr(), stream)
        h.set_offroad_field(field.data_ptr(), nm, Mh, Mw, mow)
        h._mask_src = None                                     # (a training step on this handle attaches its own field again)
        gt = (fut[..., 1:].to(torch.float32) * self._scale(d)).permute(0, 2, 1, 3)                      # [n, mno, T_pred, 2], normalised
        worlds = {"": Y.reshape(d.R, d.T_pred, 2).contiguous(),
                  "gt_": gt[:, None].expand(d.n_scenes, d.K, d.mno, d.T_pred, 2).reshape(d.R, d.T_pred, 2).contiguous()}
        res = {}
        for tag, rows in worlds.items():
            count = torch.empty((d.n_scenes, d.K), device=self.device, dtype=torch.int32)
            term = torch.empty((1,), device=self.device, dtype=torch.float32)
            h.offroad_loss(fut.data_ptr(), rows.data_ptr(), float(scale), 0, count.data_ptr(), 0, term.data_ptr(), stream)
            res[tag + "count"], res[tag + "penalty"] = count.cpu().numpy(), float(term[0])
        lmask = h.device_tensor("lmask", "|u1")[: d.A].reshape(d.n_scenes, d.mno) != 0
        seen = (fut[..., 0] != 0).sum(1)                                                                # [n, mno] counted frames per slot
        frames = (seen * lmask * torch.as_tensor(mow >= 0, device=self.device)[:, None]).sum(1).cpu().numpy().astype(np.int64)
        res["frames"] = frames
        res["rate"] = res["count"] / np.maximum(frames, 1)[:, None]
        res["gt_count"] = res["gt_count"][:, 0]
        res["gt_rate"] = res["gt_count"] / np.maximum(frames, 1)
        torch.cuda.synchronize()                               # `field` is referenced by the handle until the next set_offroad_field: keep it
        self._eval_field = field
        return res

    def evaluate_nll(self, Y, score, fut_windows, horizons=None, units="px", weighted: bool = False, log_floor: float = _lib.KDE_LOG_FLOOR,
                     return_frames: bool = False):
        """[A, n_h, 2] = per horizon (mean, final) KDE negative log-likelihood of the ground truth under the agent's K samples: at every counted
        frame a Gaussian kernel density (Scott's bandwidth, scipy.stats.gaussian_kde's fit) over the K sampled positions, its log at the ground
        truth clipped below at log_floor, averaged over the counted frames before the horizon / taken at the last of them; zeros where there is
        none.  weighted=False: equal weights; True: the weights softmax(score) that the ranking loss trains the IOC scores as.  The density is
        per unit^2: units, horizons and `fut_windows` as in evaluate_ranked.  return_frames=True: also the per-frame log-densities [A, T_pred]
        (0 where a frame is not counted)."""
        torch = self.torch
        h, d, hz, (ux, uy, _), fut, stream = self._evaluation(Y, fut_windows, horizons, units)
        if weighted and score is None:
            raise ValueError("weighted=True needs the IOC scores")
        out = torch.empty((d.A, len(hz), 2), device=self.device, dtype=torch.float32)
        frames = torch.empty((d.A, d.T_pred), device=self.device, dtype=torch.float32) if return_frames else None
        h.kde_nll(Y.data_ptr(), fut.data_ptr(), score.data_ptr() if weighted else 0, hz, ux, uy, float(log_floor), out.data_ptr(), _ptr(frames), stream)
        return (out.cpu().numpy(), frames.cpu().numpy()) if return_frames else out.cpu().numpy()
