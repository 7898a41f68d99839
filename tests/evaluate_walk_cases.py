"""The inputs of tests/test_evaluate_walk_cpu.py and tests/golden/make_evaluate_walk_golden.py: a stub model that answers desire_amd.evaluate's walk
on the CPU, two videos whose agents appear late, leave inside a target window and have a gap, and the four command lines.  What the stub hands back is
a pure function of (method, window_base of the batch, the call's arguments) -- a generator seeded from their hash, never the next draw of one stream --
so the order in which the walk calls the model is free while what it calls it with is not; every call is recorded with its arguments."""
import hashlib
import json

import numpy as np

K, MNO, T_OBS, T = 5, 8, 4, 6
FLAGS = ["--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--num_samples", "5", "--batch_size", "3", "--eval_horizons", "2,4,6",
         "--seed", "3", "--checkpoint", "none.npz"]
EVERY = ["--nll", "--select", "nms", "--nms_radius", "20", "--nms_metric", "mean", "--nms_horizon", "5", "--joint", "--collision_radius", "12.5",
         "--plan_risk", "--occupancy", "6x9", "--occupancy_mode", "until", "--modes", "3", "--modes_iters", "5", "--modes_min_std", "0.5",
         "--units", "0.2", "--max_windows", "7", "--device_rng", "--eval_top", "2"]
CASES = {"plain": [], "every_flag": EVERY, "occupancy_at": ["--occupancy", "6x9", "--occupancy_mode", "at"],
         "modes_by_score": ["--modes", "2", "--modes_seeds", "score"]}


def videos():
    """Two videos of 45 frames [F, 8, 3] = (id, x, y): four windows of 10 frames each (4 observed, 6 targets), so 8 windows in batches of 3, 3, 2."""
    out = []
    for v in range(2):
        t = np.arange(45, dtype=np.float64)
        video = np.zeros((45, MNO, 3))
        for i in range(6):
            video[:, i, 0] = 10 * v + i + 1
            video[:, i, 1] = 150 + 120 * i + (3 + v) * t
            video[:, i, 2] = 100 + 90 * i + 2 * t
        video[:12 + v, 1] = 0              # appears late: inside the observed frames of the second window
        video[:25, 2] = 0                  # ... and inside the targets of the third (not there at its last observed frame)
        video[16 + v:, 3] = 0              # leaves inside the targets of the second window
        video[14:16, 4] = 0                # a gap over the first two targets of the second window: counted from the second horizon on
        video[34:36 + v, 4] = 0            # ... and again in the fourth
        video[27:29, 5] = 0                # a gap in the middle of the third window's targets
        out.append(video)
    return out


def _plain(x):
    """A call's argument as JSON holds it."""
    if isinstance(x, (np.floating, np.integer, np.bool_)):
        return x.item()
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


class Stub:
    """Answers the walk with arrays of the shapes and dtypes DESIREModel hands back."""

    def __init__(self):
        self.calls = []
        self.final_output = self.final_states = None

    def _rng(self, method, Y, score, fut, **kw):
        """Records the call; the generator of its answer."""
        assert Y == ("Y", self.base) and score == ("score", self.base)          # the batch's own samples and scores were passed on
        futs = None if fut is None else hashlib.sha256(np.stack(fut).astype(np.float64).tobytes()).hexdigest()[:16]
        rec = [method, self.base, {k: _plain(v) for k, v in sorted(kw.items())}, futs]
        self.calls.append(rec)
        return np.random.default_rng(int.from_bytes(hashlib.sha256(json.dumps(rec).encode()).digest()[:8], "little"))

    def predict(self, past, **kw):
        self.n, self.base = len(past), int(kw.get("window_base", 0))
        self.final_output, self.final_states = ("Y", self.base), ("score", self.base)
        self._rng("predict", self.final_output, self.final_states, past, **kw)

    def evaluate(self, Y, fut):
        return self._rng("evaluate", Y, self.final_states, fut).uniform(0, 0.1, (self.n * MNO, 4)).astype(np.float32)

    def evaluate_ranked(self, Y, score, fut, top=None, horizons=None, units="px", return_count=False, **kw):
        g = self._rng("evaluate_ranked", Y, score, fut, top=top, horizons=horizons, units=units, return_count=return_count, **kw)
        out = g.uniform(0.5, 30.0, (self.n * MNO, len(horizons), 4)).astype(np.float32)
        return (out, g.integers(1, K + 1, self.n * MNO).astype(np.int32)) if return_count else out

    def evaluate_nll(self, Y, score, fut, horizons=None, units="px", weighted=False, log_floor=None, return_frames=False):
        g = self._rng("evaluate_nll", Y, score, fut, horizons=horizons, units=units, weighted=weighted, log_floor=log_floor, return_frames=return_frames)
        out = g.uniform(-2.0, 20.0, (self.n * MNO, len(horizons), 2)).astype(np.float32)
        frames = np.maximum(g.uniform(-30.0, 2.0, (self.n * MNO, T)), log_floor).astype(np.float32)     # a third of them on the floor
        return (out, frames) if return_frames else out

    def evaluate_joint(self, Y, score, fut, top=None, horizons=None, units="px", collision_radius=None):
        g = self._rng("evaluate_joint", Y, score, fut, top=top, horizons=horizons, units=units, collision_radius=collision_radius)
        n, nh = self.n, len(horizons)
        cnt = np.zeros((n, K + 1, nh, 2), np.int32)
        cnt[..., 1] = np.sort(g.integers(0, 5, (n, 1, nh)), -1)                 # agents taking part: grows with the horizon, none in some windows
        cnt[..., 0] = g.integers(0, 5, (n, K + 1, nh)) % (cnt[..., 1] + 1)
        return {"jerr": g.uniform(0, 9, (n, K, nh, 2)).astype(np.float32), "out": g.uniform(0.5, 9, (n, nh, 4)).astype(np.float32),
                "order": np.stack([g.permutation(K) for _ in range(n)]).astype(np.int32), "jscore": g.standard_normal((n, K)).astype(np.float32),
                "cnt": cnt, "first": g.integers(0, T + 1, (n, K + 1, MNO)).astype(np.int32)}

    def evaluate_plan_risk(self, Y, score, fut, collision_radius, horizons=None, weights="score"):
        g = self._rng("evaluate_plan_risk", Y, score, fut, collision_radius=collision_radius, horizons=horizons, weights=weights)
        n, nh = self.n, len(horizons)
        return {"risk": g.uniform(0, 1, (n, MNO, nh)).astype(np.float32), "first": g.integers(0, T + 1, (n, MNO, K + 1)).astype(np.int32),
                "takes_part": g.uniform(0, 1, (n, MNO, nh)) < 0.6, "predicted": g.uniform(0, 1, nh), "actual": g.uniform(0, 1, nh),
                "agents": np.sort(g.integers(0, n * MNO, nh)).astype(np.int64)}

    def evaluate_occupancy(self, Y, score, fut, grid, horizons=None, mode="at", weights="score", mask=None, mask_of_window=None):
        g = self._rng("evaluate_occupancy", Y, score, fut, grid=grid, horizons=horizons, mode=mode, weights=weights)
        assert mask is None and mask_of_window is None
        n, nh = self.n, len(horizons)
        res = {"occ": g.uniform(0, 1, (n, nh) + tuple(grid)).astype(np.float32), "expected": g.uniform(0, 0.2, (n, nh) + tuple(grid)).astype(np.float32),
               "off": g.uniform(0, 0.3, (n, MNO, nh)).astype(np.float32)}
        if mode == "at":
            res["hit"] = np.maximum(g.uniform(-0.3, 1, (n, MNO, nh)), 0).astype(np.float32)          # a quarter of them zero: the floor of the log
        return res

    def evaluate_modes(self, Y, score, fut, modes=6, horizons=None, units="px", **kw):
        g = self._rng("evaluate_modes", Y, score, fut, modes=modes, horizons=horizons, units=units, **kw)
        A, nh = self.n * MNO, len(horizons)
        return {"nll": g.uniform(-2, 20, (A, nh, 2)).astype(np.float32), "top1": g.uniform(0.5, 30, (A, nh, 2)).astype(np.float32),
                "best": g.uniform(0.5, 30, (A, nh, 2)).astype(np.float32), "prob": g.uniform(0, 1, (A, modes)).astype(np.float32),
                "count": g.integers(0, K + 1, (A, modes)).astype(np.int32), "passes": g.integers(0, 9, A).astype(np.int32)}


def walk(extra):
    """(the text main() would print, the sorted call log) of one command line."""
    from desire_amd import evaluate as E
    from desire_amd.data_loader import DataLoader
    a = E.build_parser().parse_args(FLAGS + list(extra))
    dl = DataLoader(int(a.batch_size), a.seq_length + a.pred_length, a.max_num_obj, a.leave_dataset, frames=videos())
    stub = Stub()
    res = E.evaluate(a, data_loader=dl, model=stub)
    return json.dumps(res, indent=1), sorted(json.dumps(c) for c in stub.calls)
