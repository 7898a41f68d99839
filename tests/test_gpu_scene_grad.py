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


def _case(kw, n_absent=4, seed=42):
    base = dict(n_scenes=2, mno=32, K=3, T_obs=6, T_pred=7, n_grids=2)
    base.update(kw)
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
    gos = ((np.arange(d.n_scenes) + 1) % d.n_grids).astype(np.int32)          # mixed: scene 0 -> grid 1, scene 1 -> grid 0, ...
    return d, w, past, fut, eps, grids, gos


def _autograd_grid_grad(monkeypatch, d, w, past, fut, eps, grids, gos):
    import torch
    from oracle import desire_torch as OT
    orig = OT._t
    monkeypatch.setattr(OT, "_t", lambda x: x if torch.is_tensor(x) else orig(x))
    G = torch.as_tensor(grids, dtype=torch.float64).clone().requires_grad_(True)
    out = OT.forward_loss(to_oracle_layout(past), to_oracle_layout(fut), eps, G, gos, OT.leaf_weights(w), d)
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
    h.forward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr(), Y.data_ptr(), score.data_ptr())
    outs = []
    for _ in range(n_backward):
        h.backward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr())
        torch.cuda.synchronize()
        outs.append((h.scene_grid_grad().cpu().numpy().copy() if scene_grad else None, h.grad_tensor().cpu().numpy().copy()))
    return h, outs


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
]


@pytest.mark.parametrize("name,kw,n_absent,seed,tol", CASES, ids=[c[0] for c in CASES])
def test_scene_grid_grad_matches_autograd(monkeypatch, name, kw, n_absent, seed, tol):
    d, w, past, fut, eps, grids, gos = _case(kw, n_absent, seed)
    ref = _autograd_grid_grad(monkeypatch, d, w, past, fut, eps, grids, gos)
    _, outs = _step(d, w, past, fut, eps, grids, gos, option_first=(name != "iters2"))
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
    _, outs = _step(d, w, past, fut, eps, grids, gos, n_backward=2)
    (g1, flat1), (g2, flat2) = outs
    assert np.array_equal(g1, g2)
    assert np.array_equal(flat1, flat2)
    _, base = _step(d, w, past, fut, eps, grids, gos, scene_grad=False)
    assert np.array_equal(base[0][1], flat1)                 # the option adds an output, it changes no weight gradient


def test_scene_grid_grad_is_refused_without_the_option():
    from desire_amd import _lib
    d, w, past, fut, eps, grids, gos = _case(dict())
    h, _ = _step(d, w, past, fut, eps, grids, gos, scene_grad=False)
    with pytest.raises(_lib.DesireError, match="scene_grad"):
        h.scene_grid_grad()
    with pytest.raises(_lib.DesireError, match="scene_grad must be 0 or 1"):
        h.set_option("scene_grad", 2)
    h.set_option("scene_grad", 1)
    h.set_training(False)
    with pytest.raises(_lib.DesireError, match="training mode"):
        h.scene_grid_grad()
