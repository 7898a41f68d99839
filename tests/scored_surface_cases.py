"""The calls of tests/test_gpu_scored_surface.py and tests/golden/make_scored_surface_digests.py: every public scored-sample method of DESIREModel
once or twice on one small planted case (2 windows of the shared EVAL_FLAGS model: 8 slots, 5 samples, 6 target frames), the forward replaced by
the planted (Y, score).  run() returns per call the arrays it handed back and how often each _lib.Handle method ran; digest() turns the arrays
into (dtype, shape, SHA-256 of the bytes)."""
import collections
import hashlib
import inspect

import numpy as np

from tests.helpers import EVAL_FLAGS

N, K, MNO, T_OBS, T = 2, 5, 8, 4, 6
HZ = [2, 4, 6]
W_IMG = 2048.0                          # train.py's default frame, both sides
ABSENT, LEAVER, GAP, TWIN = 5, 6, 7, 1   # slots: never there; leaves after target frame 3; misses target frame 2; samples 0 and 1 coincide
RADIUS = 20.0                           # pixels: the two tracks of an agent are ~100 px apart, the samples on one track within ~5 px


def planted():
    """(past [N, T_OBS, MNO, 3], fut [N, T, MNO, 3] loader windows in pixels, Y [N, K, MNO, T, 2] normalised, score [N, K, MNO], plans, mask)."""
    rng = np.random.default_rng(20)
    t = np.arange(1, T + 1, dtype=np.float32)
    start = np.zeros((N, MNO, 2), np.float32)
    for w in range(N):
        for s in range(MNO):
            start[w, s] = (300 + 170 * s + 40 * w, 400 + 110 * s - 25 * w)
        start[w, 3] = start[w, 2] + np.array([28.0, -9.0], np.float32)         # two agents side by side: contacts
    steps = np.array([[[9.0, 2.0]], [[-4.0, 17.0]]], np.float32)              # two tracks per agent: samples 0..2 on the first, 3 and 4 on the second
    of_track = [0, 0, 0, 1, 1]
    Ypx = np.empty((N, K, MNO, T, 2), np.float32)
    for k in range(K):
        Ypx[:, k] = start[:, :, None, :] + steps[of_track[k]] * t[None, None, :, None] + rng.uniform(-2.5, 2.5, (N, MNO, 1, 2)).astype(np.float32)
    Ypx[:, 2, TWIN] = Ypx[:, 3, TWIN] + np.float32(1.5)
    Ypx[:, 1, TWIN] = Ypx[:, 0, TWIN]                                          # an exact twin, alone on its track: the mode it seeds ends empty
    assert Ypx.min() > 0 and Ypx.max() < W_IMG                                 # inside the frame
    score = rng.standard_normal((N, K, MNO)).astype(np.float32)
    score[:, 0, TWIN], score[:, 1, TWIN] = 5.0, 4.0                            # the twins are that agent's two best
    score[0, 1, 2] = score[0, 3, 2]                                            # a tie across the tracks
    score[1, 4, LEAVER] = -np.inf                                              # one non-finite score
    ids = np.arange(1, MNO + 1, dtype=np.float32)
    past = np.zeros((N, T_OBS, MNO, 3), np.float32)
    fut = np.zeros((N, T, MNO, 3), np.float32)
    back = np.arange(-T_OBS + 1, 1, dtype=np.float32)
    for w in range(N):
        past[w, :, :, 0] = ids
        past[w, :, :, 1:] = start[w][None] + steps[0] * back[:, None, None]
        fut[w, :, :, 0] = ids
        fut[w, :, :, 1:] = start[w][None] + (0.7 * steps[0] + 0.3 * steps[1]) * t[:, None, None] + rng.uniform(-3, 3, (T, MNO, 2)).astype(np.float32)
    past[:, :, ABSENT] = 0
    fut[:, :, ABSENT] = 0
    fut[:, 4:, LEAVER] = 0
    fut[:, 2, GAP] = 0
    plans = np.empty((N, 3, T, 2), np.float32)                                 # pixels: along agent 0's first track, across agent 2's, far away
    for w in range(N):
        plans[w, 0] = start[w, 0] + steps[0][0] * t[:, None] + 6.0
        plans[w, 1] = start[w, 2] + np.array([-30.0, 0.0], np.float32) + np.array([12.0, 3.0], np.float32) * t[:, None]
        plans[w, 2] = np.array([1900.0, 100.0], np.float32) + t[:, None]
    plans[1, 1, 4:] = np.nan                                                   # a plan that ends early
    mask = np.ones((2, 8, 12), np.uint8)
    mask[0, 2:5, 3:9] = 0
    mask[1, :, :2] = 0
    return past, fut, (Ypx / W_IMG).astype(np.float32), score, plans, mask


def _calls(m, torch, past, fut, Y, score, plans, mask):
    """(name, thunk) of every call; past / fut as loader windows (lists) and as device tensors, so both entries are walked."""
    past_l, fut_l = list(past), list(fut)
    past_t, fut_t = torch.as_tensor(past, device="cuda"), torch.as_tensor(fut, device="cuda")
    nms = dict(select="nms", nms_radius=RADIUS)
    return [
        ("predict_device score", lambda: m.predict_device(past_t, top=2)),
        ("predict_device nms", lambda: m.predict_device(past_t, top=3, nms_metric="mean", nms_horizon=4, **nms)),
        ("predict_device joint", lambda: m.predict_device(past_t, top=2, select="joint", collision_radius=30.0)),
        ("predict", lambda: m.predict(past_l, top=1)),
        ("evaluate_ranked", lambda: m.evaluate_ranked(Y, score, fut_l, top=2, horizons=HZ, units=0.2)),
        ("evaluate_ranked nms", lambda: m.evaluate_ranked(Y, score, fut_t, top=3, return_count=True, **nms)),
        ("evaluate_nll uniform", lambda: m.evaluate_nll(Y, score, fut_l, horizons=HZ, return_frames=True)),
        ("evaluate_nll weighted", lambda: m.evaluate_nll(Y, score, fut_t, units="norm", weighted=True, return_frames=True)),
        ("evaluate_joint", lambda: m.evaluate_joint(Y, score, fut_l, top=2, horizons=HZ, collision_radius=30.0)),
        ("score_plans n", lambda: m.score_plans(past_l, plans, 30.0, horizons=HZ, ego_slot=[0, -1])),
        ("score_plans nM", lambda: m.score_plans(past_t, plans, 30.0, ego_slot=[[0, 2, -1], [-1, 2, 0]], weights="uniform")),
        ("evaluate_plan_risk", lambda: m.evaluate_plan_risk(Y, score, fut_l, 30.0, horizons=HZ)),
        ("predict_modes nms", lambda: m.predict_modes(past_l, modes=3, seeds="nms", nms_radius=RADIUS, iters=4)),
        ("predict_modes score", lambda: m.predict_modes(past_t, modes=3, seeds="score", min_std=0.5, horizon=4, weights="uniform")),
        ("evaluate_modes nms", lambda: m.evaluate_modes(Y, score, fut_l, modes=3, seeds="nms", nms_radius=RADIUS, horizons=HZ, units=0.2)),
        ("evaluate_modes score", lambda: m.evaluate_modes(Y, score, fut_t, modes=3, seeds="score", iters=4, weights="uniform")),
        ("predict_occupancy at", lambda: m.predict_occupancy(past_t, (8, 12), horizons=HZ)),
        ("predict_occupancy until mask", lambda: m.predict_occupancy(past_t, (8, 12), mode="until", weights="uniform", mask=mask, mask_of_window=[1, -1])),
        ("evaluate_occupancy at mask", lambda: m.evaluate_occupancy(Y, score, fut_l, (8, 12), horizons=HZ, mask=mask[0])),
        ("evaluate_occupancy until", lambda: m.evaluate_occupancy(Y, score, fut_t, (8, 12), mode="until", weights="uniform")),
    ]


def _arrays(torch, out):
    """A call's result as {name: numpy array}: a dict as it is, a tuple by position, one array as "out"."""
    if isinstance(out, dict):
        items = list(out.items())
    elif isinstance(out, tuple):
        items = [(str(i), v) for i, v in enumerate(out)]
    else:
        items = [("out", out)]
    return {k: np.ascontiguousarray(v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in items}


def run(torch, monkeypatch):
    """{call: {"keys": the result's keys in order, "arrays": {...}, "handle_calls": {Handle method: times it ran}}}."""
    from desire_amd import _lib, evaluate as E
    from desire_amd.model import DESIREModel
    past, fut, Y, score, plans, mask = planted()
    m = DESIREModel(E.build_parser().parse_args(EVAL_FLAGS), seed=4)
    m._handle(N, False)                                                        # built (and given its weights) before anything is counted
    Yt, st = torch.as_tensor(Y, device="cuda"), torch.as_tensor(score, device="cuda")
    monkeypatch.setattr(m, "forward_device", lambda *a, **kw: (Yt, st))
    ran = collections.Counter()

    def counted(name, fn):
        def call(self, *a, **kw):
            ran[name] += 1
            return fn(self, *a, **kw)
        return call

    for name, fn in list(vars(_lib.Handle).items()):
        if inspect.isfunction(fn) and not name.startswith("_") and name != "close":
            monkeypatch.setattr(_lib.Handle, name, counted(name, fn))
    res = {}
    for name, thunk in _calls(m, torch, past, fut, Yt, st, plans, mask):
        ran.clear()
        arrays = _arrays(torch, thunk())
        torch.cuda.synchronize()
        res[name] = {"keys": list(arrays), "arrays": arrays, "handle_calls": dict(sorted(ran.items()))}
    return res


def digest(res):
    """run()'s record with every array replaced by its dtype, shape and SHA-256: what the golden file holds."""
    return {name: {"keys": r["keys"], "handle_calls": r["handle_calls"],
                   "arrays": {k: {"dtype": str(v.dtype), "shape": list(v.shape), "sha256": hashlib.sha256(v.tobytes()).hexdigest()}
                              for k, v in r["arrays"].items()}} for name, r in res.items()}


def check_paths(res):
    """The paths the case is there to take: the suppression keeps fewer than K, a joint order differs from an agent's own, a mode ends empty."""
    kept = res["evaluate_ranked nms"]["arrays"]["1"].reshape(N, MNO)
    assert (kept[:, :ABSENT] < K).all() and (kept[:, :ABSENT] >= 2).all(), kept
    own = res["predict_device score"]["arrays"]["order"]
    joint = res["predict_device joint"]["arrays"]["order"]
    assert (own[:, :ABSENT] != joint[:, :ABSENT]).any()
    for call in ("predict_modes score", "evaluate_modes score"):
        count = res[call]["arrays"]["count"].reshape(N, MNO, 3)
        assert (count[:, TWIN] == 0).any() and (count[:, TWIN].sum(-1) == K).all(), count[:, TWIN]
