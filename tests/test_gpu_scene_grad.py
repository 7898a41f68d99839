"""d(loss)/d(scene grids) of a training step (desire_set_option(h, "scene_grad", 1), csrc/kernels_scene.hip) against float64 autograd of the
torch oracle, fed a grid tensor that requires grad; bitwise reproducibility; every other gradient unchanged by the option; refusals."""
import numpy as np
import pytest

from desire_amd.spec import init_weights
from tests.helpers import make_case, small_dims, to_oracle_layout

pytestmark = pytest.mark.gpu

FLAG_COMPACT = 12                       # DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


def _spread(w):
    # as tests/test_gpu_train.py: K distinct futures, so the ranking gradients do not vanish
    for k in w:
        if k.startswith("vae_dec/") and k.endswith("/w"):
            w[k] = w[k] * 3
    w["mask_fc/w"] = w["mask_fc/w"] * 20
    w["head/w"] = w["head/w"] * 4
    w["ioc/score/w"] = w["ioc/score/w"] * 3
    return w


OFF_FRAME_PX = np.float32([(0, 0), (-1260, 0), (1260, 0), (0, -990), (0, 990)])     # 0.9 of the 1400 x 1100 frame, by slot % 5


def _case(kw, n_absent=4, seed=42):
    base = dict(n_scenes=2, mno=32, K=3, T_obs=6, T_pred=7, n_grids=2)
    base.update(kw)
    off_frame = base.pop("off_frame", False)
    d = small_dims(**base)
    w = _spread(init_weights(d, 41))
    if isinstance(n_absent, (list, tuple)):           # a different number of absent slots per scene: the windows fall into several slot classes
        past, fut, eps, grids, _ = make_case(d, seed=seed, n_absent=0)
        for sc, na in enumerate(n_absent):
            if na:
                past[sc, :, d.mno - na:] = 0
                fut[sc, :, d.mno - na:] = 0
    else:
        past, fut, eps, grids, _ = make_case(d, seed=seed, n_absent=n_absent)
    if off_frame:                                      # whole tracks moved off the frame by slot: the agents of one class keep their relative positions
        for win in (past, fut):                        # (and their social neighbours), and the sort key of k_scene_ds meets the clamp on every side
            win[..., 1:] += np.where(win[..., :1] != 0, OFF_FRAME_PX[np.arange(d.mno) % 5], 0).astype(np.float32)
    gos = ((np.arange(d.n_scenes) + 1) % d.n_grids).astype(np.int32)          # mixed: scene 0 -> grid 1, scene 1 -> grid 0, ...
    return d, w, past, fut, eps, grids, gos


def pinned_to_kernel(d, past, fut, eps, grids, gos, w, Y0_gpu):
    """The stop-gradient quantities of the reference with the KERNEL's trajectories in place of its own (as tests/fuzz_train.py does): the float64
    reference and the fp32 kernels look cells and bins up at positions that differ by rounding, and on the rectangular grids a present position
    lies within 1e-6 of a cell edge.  With Yd pinned, cells and bins are equal by construction; dmax comes from an unpinned evaluation.  Rows of
    absent agents (not computed on a compacted handle; masked out of the loss) keep the reference's own positions."""
    import torch
    from oracle import desire_torch as OT
    with torch.no_grad():
        o1 = OT.forward_loss(to_oracle_layout(past), to_oracle_layout(fut), eps, grids, gos, OT.leaf_weights(w), d)
    present = np.repeat((past[:, d.T_obs - 1, :, 0] != 0)[:, None, :], d.K, 1).reshape(d.R)
    Yd = np.where(present[:, None, None], Y0_gpu.astype(np.float64), o1["Yd"].numpy())
    return {"Yd": Yd, "dmax": o1["dmax"].numpy()}


def _autograd_grid_grad(monkeypatch, d, w, past, fut, eps, grids, gos, fixed=None):
    import torch
    from oracle import desire_torch as OT
    orig = OT._t
    monkeypatch.setattr(OT, "_t", lambda x: x if torch.is_tensor(x) else orig(x))
    G = torch.as_tensor(grids, dtype=torch.float64).clone().requires_grad_(True)
    out = OT.forward_loss(to_oracle_layout(past), to_oracle_layout(fut), eps, G, gos, OT.leaf_weights(w), d, fixed=fixed)
    out["loss"].backward()
    return G.grad.numpy()


def _step(d, w, past, fut, eps, grids, gos, scene_grad=True, option_first=True, n_backward=1):
    import torch
    from desire_amd import _lib
    h = _lib.Handle(d)
    h.set_weights(w)
    if d.flags:
        h.set_option("compact_min_rows", 0)          # every slot class runs on its own
    if scene_grad and option_first:
        h.set_option("scene_grad", 1)
    h.set_training(True)
    if scene_grad and not option_first:
        h.set_option("scene_grad", 1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    past_t, fut_t, eps_t, grids_t = t(past), t(fut), t(eps), t(grids)
    h.set_scene_grids(grids_t.data_ptr(), gos)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda")
    score = torch.zeros((d.R,), device="cuda")
    h.encode(past_t.data_ptr(), fut_t.data_ptr())                          # desire_forward, with the decoded Y0 kept in the caller's row layout
    h.sample(eps_t.data_ptr(), Y.data_ptr())
    Y0 = Y.cpu().numpy().copy()
    h.ioc_refine(Y.data_ptr(), score.data_ptr())
    outs = []
    for _ in range(n_backward):
        h.backward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr())
        torch.cuda.synchronize()
        outs.append((h.scene_grid_grad().cpu().numpy().copy() if scene_grad else None, h.grad_tensor().cpu().numpy().copy()))
    return h, outs, Y0


# (name, dims, absent slots per scene, seed, tolerance).  iters = 2: the second pass looks its cells and bins up at positions the first one
# computed, in fp32 here and in float64 in the reference; seed 45 on a 16 x 16 grid keeps every one of them more than 3e-6 from a cell or
# bin edge (at seed 42 on 64 x 64 one row changes cell, and the weight gradients of the IOC miss autograd by 5 % as well)
CASES = [
    ("fp32", dict(), 4, 42, 2e-4),
    ("compact12", dict(flags=FLAG_COMPACT), 22, 42, 2e-4),          # 10 present of 32: the padded three-groups-per-tile class
    ("compact12_mixed", dict(flags=FLAG_COMPACT, n_scenes=4), [22, 4, 26, 14], 42, 2e-4),   # 10 / 28 / 6 / 18 present: several classes, mixed grids
    ("iters2", dict(iters=2, Gh=16, Gw=16), 4, 45, 2e-4),
    ("cluster_fwd_mno64", dict(mno=64, n_scenes=1, K=3, H=64, L=64, ioc_form=4), 7, 42, 2e-4),      # cluster forward, 64-row tile BPTT
    ("cluster_bwd_mno96", dict(mno=96, n_scenes=1, K=2, H=128), 7, 42, 2e-4),
    ("cluster_bwd_mno128", dict(mno=128, n_scenes=2, K=2, H=64, L=64), 7, 42, 2e-4),
    ("split_bf16", dict(bf16=2), 4, 42, 2e-4),
    # rectangular grids (reference pinned to the kernel's trajectories, see pinned_to_kernel).  No split-operand case here: k_scene_ds and the struct
    # it is launched with do not depend on dims.bf16, and at this fixture's seeds 40 .. 79 the float64 reference has an e_r pre-activation within
    # 5.3e-6 of the ReLU kink (4.9e-7 at seed 42, 40 x 24), inside the split forward's own error, where the gradient differs by a whole term
    # (tests/test_gpu_split.py describes it); tests/test_gpu_scene_train.py runs split operands on 12 x 20 and 20 x 12
    ("fp32_44x56", dict(Gh=44, Gw=56), 4, 42, 2e-4),
    ("compact12_mixed_44x56", dict(flags=FLAG_COMPACT, n_scenes=4, Gh=44, Gw=56), [22, 4, 26, 14], 42, 2e-4),
    ("cluster_bwd_mno96_40x24", dict(mno=96, n_scenes=2, K=2, H=128, Gh=40, Gw=24), 7, 42, 2e-4),
    ("fp32_off_frame_44x56", dict(Gh=44, Gw=56, off_frame=True), 4, 42, 2e-4),
]


@pytest.mark.parametrize("name,kw,n_absent,seed,tol", CASES, ids=[c[0] for c in CASES])
def test_scene_grid_grad_matches_autograd(monkeypatch, name, kw, n_absent, seed, tol):
    d, w, past, fut, eps, grids, gos = _case(kw, n_absent, seed)
    _, outs, Y0 = _step(d, w, past, fut, eps, grids, gos, option_first=(name != "iters2"))
    fixed = pinned_to_kernel(d, past, fut, eps, grids, gos, w, Y0) if d.Gh != d.Gw else None
    ref = _autograd_grid_grad(monkeypatch, d, w, past, fut, eps, grids, gos, fixed=fixed)
    got = outs[0][0]
    assert got.shape == (d.n_grids, d.Gh, d.Gw, d.C)
    assert np.isfinite(got).all()
    hit = np.abs(ref).reshape(-1, d.C).max(1) > 0
    assert hit.any()
    e = rel_err(got, ref)
    print("%s: %d of %d cells reached, rel err %.2e" % (name, int(hit.sum()), hit.size, e))
    assert e < tol, (name, e)


def test_scene_grid_grad_is_bitwise_reproducible_and_leaves_other_gradients_alone():
    d, w, past, fut, eps, grids, gos = _case(dict(iters=2))
    _, outs, _ = _step(d, w, past, fut, eps, grids, gos, n_backward=2)
    (g1, flat1), (g2, flat2) = outs
    assert np.array_equal(g1, g2)
    assert np.array_equal(flat1, flat2)
    _, base, _ = _step(d, w, past, fut, eps, grids, gos, scene_grad=False)
    assert np.array_equal(base[0][1], flat1)                 # the option adds an output, it changes no weight gradient


def test_scene_grid_grad_is_refused_without_the_option():
    from desire_amd import _lib
    d, w, past, fut, eps, grids, gos = _case(dict())
    h, _, _ = _step(d, w, past, fut, eps, grids, gos, scene_grad=False)
    with pytest.raises(_lib.DesireError, match="scene_grad"):
        h.scene_grid_grad()
    with pytest.raises(_lib.DesireError, match="scene_grad must be 0 or 1"):
        h.set_option("scene_grad", 2)
    h.set_option("scene_grad", 1)
    h.set_training(False)
    with pytest.raises(_lib.DesireError, match="training mode"):
        h.scene_grid_grad()
