"""The scene CNN trained end to end through the IOC backward (desire_set_scene_images): scene_cnn/* gradients against float64 autograd of the
torch oracle fed the torch scene CNN's grid; every other gradient and the forward bit-identical to a run given desire_scene_cnn's grid; the stale
check; reproducibility; Adam; refusals; DESIREModel.set_scene_images and train.py --scene_images."""
import os

import numpy as np
import pytest

from desire_amd.spec import init_weights
from tests.helpers import make_case, small_dims, to_oracle_layout

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CNN = ["scene_cnn/conv1/w", "scene_cnn/conv1/b", "scene_cnn/conv2/w", "scene_cnn/conv2/b", "scene_cnn/conv3/w", "scene_cnn/conv3/b"]


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


def _case(kw=None, seed=42, n_absent=4):
    base = dict(n_scenes=2, mno=32, K=3, T_obs=6, T_pred=7, n_grids=2, Gh=16, Gw=16)
    base.update(kw or {})
    d = small_dims(**base)
    w = init_weights(d, 41)
    for k in w:
        if k.startswith("vae_dec/") and k.endswith("/w"):
            w[k] = w[k] * 3
    w["mask_fc/w"] = w["mask_fc/w"] * 20
    w["head/w"] = w["head/w"] * 4
    w["ioc/score/w"] = w["ioc/score/w"] * 3
    past, fut, eps, _, _ = make_case(d, seed=seed, n_absent=n_absent)
    images = np.random.default_rng(seed).uniform(0, 1, (d.n_grids, 4 * d.Gh, 4 * d.Gw, 3)).astype(np.float32)
    gos = ((np.arange(d.n_scenes) + 1) % d.n_grids).astype(np.int32)
    return d, w, past, fut, eps, images, gos


def _autograd(monkeypatch, d, w, past, fut, eps, images, gos, Y0_gpu=None):
    """Y0_gpu given (the rectangular cases): the reference's stop-gradient quantities are pinned to the kernel's trajectories, as
    tests/test_gpu_scene_grad.py::pinned_to_kernel does and for its reason -- a present position of these cases lies within 1e-6 of a cell edge."""
    import torch
    import torch.nn.functional as F
    from oracle import desire_torch as OT
    orig = OT._t
    monkeypatch.setattr(OT, "_t", lambda x: x if torch.is_tensor(x) else orig(x))
    wl = OT.leaf_weights(w)
    x = torch.as_tensor(images, dtype=torch.float64)
    x = F.relu(OT.conv2d_tf(x, wl["scene_cnn/conv1/w"], 2, "SAME") + wl["scene_cnn/conv1/b"])
    x = F.relu(OT.conv2d_tf(x, wl["scene_cnn/conv2/w"], 2, "SAME") + wl["scene_cnn/conv2/b"])
    g = OT.conv2d_tf(x, wl["scene_cnn/conv3/w"], 1, "SAME") + wl["scene_cnn/conv3/b"]
    assert tuple(g.shape) == (d.n_grids, d.Gh, d.Gw, d.C)
    fixed = None
    if Y0_gpu is not None:
        with torch.no_grad():
            o1 = OT.forward_loss(to_oracle_layout(past), to_oracle_layout(fut), eps, g, gos, wl, d)
        present = np.repeat((past[:, d.T_obs - 1, :, 0] != 0)[:, None, :], d.K, 1).reshape(d.R)
        fixed = {"Yd": np.where(present[:, None, None], Y0_gpu.astype(np.float64), o1["Yd"].numpy()), "dmax": o1["dmax"].numpy()}
    out = OT.forward_loss(to_oracle_layout(past), to_oracle_layout(fut), eps, g, gos, wl, d, fixed=fixed)
    out["loss"].backward()
    return {k: v.grad.numpy() for k, v in wl.items() if v.grad is not None}


class Run:
    """One training handle; scene = "images" (desire_set_scene_images) or "grid" (desire_scene_cnn's output through desire_set_scene_grids)."""

    def __init__(self, d, w, past, fut, eps, images, gos, scene="images", training=True):
        import torch
        from desire_amd import _lib
        self.d, self.gos = d, gos
        self.h = _lib.Handle(d)
        self.h.set_weights(w)
        if d.flags:
            self.h.set_option("compact_min_rows", 0)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
        self.past, self.fut, self.eps, self.img = t(past), t(fut), t(eps), t(images)
        if training:
            self.h.set_training(True)
        self.grid = torch.zeros((d.n_grids, d.Gh, d.Gw, d.C), device="cuda")
        if scene == "images":
            self.h.set_scene_images(self.img.data_ptr(), 4 * d.Gh, 4 * d.Gw, gos)
        else:
            self.h.scene_cnn(self.img.data_ptr(), 4 * d.Gh, 4 * d.Gw, self.grid.data_ptr())
            self.h.set_scene_grids(self.grid.data_ptr(), gos)
        self.Y = torch.zeros((d.R, d.T_pred, 2), device="cuda")
        self.score = torch.zeros((d.R,), device="cuda")

    def fwd(self):
        import torch
        self.h.encode(self.past.data_ptr(), self.fut.data_ptr())               # desire_forward, with the decoded Y0 kept in the caller's row layout
        self.h.sample(self.eps.data_ptr(), self.Y.data_ptr())
        self.Y0 = self.Y.cpu().numpy().copy()
        self.h.ioc_refine(self.Y.data_ptr(), self.score.data_ptr())
        torch.cuda.synchronize()
        return self.Y.cpu().numpy().copy(), self.score.cpu().numpy().copy()

    def bwd(self):
        import torch
        self.h.backward(self.past.data_ptr(), self.fut.data_ptr(), self.eps.data_ptr())
        torch.cuda.synchronize()

    def grads(self, w):
        return {k: self.h.get_grad(k, w[k].shape) for k in w}

    def img_grid(self):
        d = self.d
        return self.h.read_buffer("scene_img_grid", (d.n_grids, d.Gh, d.Gw, d.C))


CFG = [("fp32", dict(), 4), ("compact12", dict(flags=12), 22), ("iters2", dict(iters=2), 4), ("split_bf16", dict(bf16=2), 4),
       ("cluster_bwd_mno96", dict(mno=96, n_scenes=1, K=2, H=128), 7),
       # rectangular grids: images 48 x 80 and 80 x 48
       ("fp32_12x20", dict(Gh=12, Gw=20), 4), ("fp32_20x12", dict(Gh=20, Gw=12), 4),
       ("compact12_12x20", dict(flags=12, Gh=12, Gw=20), 22), ("compact12_20x12", dict(flags=12, Gh=20, Gw=12), 22),
       ("split_bf16_12x20", dict(bf16=2, Gh=12, Gw=20), 4), ("split_bf16_20x12", dict(bf16=2, Gh=20, Gw=12), 4)]


@pytest.mark.parametrize("name,kw,n_absent", CFG, ids=[c[0] for c in CFG])
def test_scene_cnn_gradients_match_autograd_and_nothing_else_moves(monkeypatch, name, kw, n_absent):
    d, w, past, fut, eps, images, gos = _case(kw, seed=45 if name == "iters2" else 42, n_absent=n_absent)
    a = Run(d, w, past, fut, eps, images, gos, "images")
    b = Run(d, w, past, fut, eps, images, gos, "grid")
    ya, yb = a.fwd(), b.fwd()
    ref = _autograd(monkeypatch, d, w, past, fut, eps, images, gos, Y0_gpu=a.Y0 if d.Gh != d.Gw else None)
    assert np.array_equal(ya[0], yb[0]) and np.array_equal(ya[1], yb[1])         # training-mode forward: the same grid, bit for bit
    assert np.array_equal(a.img_grid(), b.grid.cpu().numpy())
    a.bwd(); b.bwd()
    ga, gb = a.grads(w), b.grads(w)
    for k in CNN:
        assert np.abs(ref[k]).max() > 0, k
        e = rel_err(ga[k], ref[k])
        print("%s %s rel err %.2e" % (name, k, e))
        assert e < 2e-4, (name, k, e)
        assert not np.any(gb[k]), k                                                # precomputed grids: the CNN gets no gradient
    for k in w:
        if k not in CNN:
            assert np.array_equal(ga[k], gb[k]), k


def test_inference_forward_equals_the_precomputed_grid_and_follows_adam():
    d, w, past, fut, eps, images, gos = _case()
    a = Run(d, w, past, fut, eps, images, gos, "images", training=False)
    b = Run(d, w, past, fut, eps, images, gos, "grid", training=False)
    ya, yb = a.fwd(), b.fwd()
    assert np.array_equal(ya[0], yb[0]) and np.array_equal(ya[1], yb[1])
    t = Run(d, w, past, fut, eps, images, gos, "images")
    t.fwd(); t.bwd()
    g0 = t.grads(w)
    t.bwd()
    g1 = t.grads(w)
    for k in CNN:                                                                   # two backward calls: bitwise equal
        assert np.array_equal(g0[k], g1[k]), k
    assert np.array_equal(t.h.scene_grid_grad().cpu().numpy(), t.h.scene_grid_grad().cpu().numpy())
    t.h.adam_step(lr=0.005)
    from oracle import desire_torch as OT
    w2 = {k: t.h.get_weight(k, w[k].shape) for k in w}
    for k in CNN:                                                                   # Adam moved scene_cnn/* as the TF formula predicts
        want, _, _ = OT.adam_step(w[k].astype(np.float64), g0[k].astype(np.float64), 0.0, 0.0, 1)
        assert np.abs(w2[k] - want).max() <= 1e-6, k
        assert not np.array_equal(w2[k], w[k]), k
    t.h.set_training(False)
    t.fwd()                                                                         # inference: the grid is stale after Adam and rebuilt
    c = Run(d, w2, past, fut, eps, images, gos, "grid", training=False)            # a fresh handle from get_weight builds the same grid
    assert np.array_equal(t.img_grid(), c.grid.cpu().numpy())
    assert not np.array_equal(c.grid.cpu().numpy(), b.grid.cpu().numpy())


def test_refusals_and_setter_precedence():
    from desire_amd import _lib
    d, w, past, fut, eps, images, gos = _case()
    b = Run(d, w, past, fut, eps, images, gos, "grid")
    b.fwd(); b.bwd()
    for k in CNN:
        assert not np.any(b.h.get_grad(k, w[k].shape)), k
    with pytest.raises(_lib.DesireError, match="scene_grad"):
        b.h.scene_grid_grad()
    with pytest.raises(_lib.DesireError, match=r"4\*Gh, 4\*Gw"):
        b.h.set_scene_images(b.img.data_ptr(), 4 * d.Gh + 2, 4 * d.Gw, gos)
    with pytest.raises(_lib.DesireError, match="out of range"):
        b.h.set_scene_images(b.img.data_ptr(), 4 * d.Gh, 4 * d.Gw, np.full(d.n_scenes, d.n_grids, np.int32))
    a = Run(d, w, past, fut, eps, images, gos, "images")
    a.h.set_scene_grids(b.grid.data_ptr(), gos)                                     # the last setter wins: images detached
    a.fwd(); a.bwd()
    for k in CNN:
        assert not np.any(a.h.get_grad(k, w[k].shape)), k


def test_model_set_scene_images_trains_the_cnn():
    from types import SimpleNamespace
    from desire_amd.model import DESIREModel
    args = SimpleNamespace(seq_length=6, pred_length=7, d_dim=64, rnn_size=512, latent_size=64, max_num_obj=8, learning_rate=0.0005,
                           grad_clip=10.0, neighborhood_size=256, grid_size=4, num_samples=3, batch_size=2, scene_grid=16, n_grids=2)
    m = DESIREModel(args, seed=3)
    rng = np.random.default_rng(0)
    x = [np.concatenate([np.arange(1, 9, dtype=np.float32)[None, :, None].repeat(6, 0), rng.uniform(200, 1800, (6, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    y = [np.concatenate([np.arange(1, 9, dtype=np.float32)[None, :, None].repeat(7, 0), rng.uniform(200, 1800, (7, 8, 2)).astype(np.float32)], -1) for _ in range(2)]
    m.set_scene_images(rng.uniform(0, 1, (2, 64, 64, 3)).astype(np.float32), [0, 1])
    ls = [m.train_step(x, y, seed=1, grid_of_scene=[1, 0])["loss"]]
    w0 = {k: np.array(v) for k, v in m.sync_weights().items() if k.startswith("scene_cnn")}
    ls += [m.train_step(x, y, seed=1, grid_of_scene=[1, 0])["loss"] for _ in range(2)]
    assert all(np.isfinite(ls)), ls
    w1 = m.sync_weights()
    for k in w0:
        assert not np.array_equal(np.array(w1[k]), w0[k]), k
    Y, _ = m.forward(x, y, seed=1)
    assert np.isfinite(Y.cpu().numpy()).all()


def test_train_py_scene_images_on_a_real_sdd_slice(tmp_path):
    import desire_amd.train as T
    from desire_amd.data_loader import DataLoader
    from desire_amd.model import DESIREModel
    frames = [np.load(os.path.join(HERE, "loader_bookstore6_T48.npz"))["data0"]]
    root = tmp_path / "data"
    (root / "bookstore" / "video6").mkdir(parents=True)
    (root / "bookstore" / "video6" / "annotations_processed.csv").write_text("")
    npz = str(tmp_path / "imgs.npz")
    np.savez(npz, **{"bookstore/video6": np.random.default_rng(1).uniform(0, 1, (64, 64, 3)).astype(np.float32)})
    a = T.build_parser().parse_args(["--batch_size", "2", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "32", "--d_dim", "64",
                                     "--latent_size", "64", "--num_samples", "2", "--max_steps", "3", "--prefetch", "0", "--data_dir", str(root),
                                     "--scene_images", npz, "--save_dir", str(tmp_path / "save"), "--save_every", "1000"])
    a.scene_grid = 16
    dl = DataLoader(a.batch_size, a.seq_length + a.pred_length, a.max_num_obj, frames=frames)
    dl.data_dir, dl.leave_dataset = str(root), 1
    a.n_grids = 1
    model = None
    losses = T.train(a, data_loader=dl, model=model, log=lambda s: None)
    assert len(losses) == 3 and all(np.isfinite(losses)), losses
