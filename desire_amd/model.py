"""DESIREModel -- host-side mirror of the reference's model/model.py:29-688 public surface, backed
by libdesire_hip.so.

Kept from the reference:
  * constructor takes the argparse Namespace of train.py:30-88 (seq_length, d_dim, rnn_size,
    latent_size, max_num_obj, learning_rate, grad_clip, neighborhood_size, grid_size, ...);
  * attribute names input_data / target_data / cost / learning_rate / gru_states / final_states /
    final_output exist (here: the last fed arrays / last results, not TF tensors);
  * sample(sess, traj, grid, dimensions, true_traj, num) -> ndarray [obs+num, max_num_obj, 3]
    (model/model.py:613-688).

New (the reference has one seq_length, K hard-coded to 7, no IOC): args.pred_length, args.num_samples,
args.ioc_iters, args.img_width/img_height, args.bf16 (True/1: bf16 matrix operands, inference only; 2 or "x3": split-bf16 operands, fp32-equivalent), and forward() that returns
all K refined samples + scores.

PyTorch is used for device memory and streams only.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import RECON_MODES
from .spec import Dims, init_weights, weight_shapes


def default_top(K: int) -> int:
    """How many of an agent's K samples "the top 10 % by score" are (the paper's protocol): max(1, K // 10)."""
    return max(1, int(K) // 10)


def default_horizons(T_pred: int):
    """The paper's 1 / 2 / 3 / 4 s of a 4 s prediction in frames of this model: ceil(T_pred * q / 4) for q = 1..4, duplicates collapsed."""
    return sorted({(int(T_pred) * q + 3) // 4 for q in (1, 2, 3, 4)})


def _next_divisor_of_64(n: int) -> int:
    """Pad max_num_obj up to a slot count the IOC tiling accepts: a divisor of 32, or a multiple of 32 up to 256 (above 128 the IOC pass
    runs step-wise and training is refused)."""
    for m in (1, 2, 4, 8, 16, 32, 64, 96, 128, 160, 192, 224, 256):
        if m >= n:
            return m
    raise ValueError("max_num_obj > 256 is not supported")


def dims_from_args(args, n_scenes: int, posterior: bool = True, ref_compat: bool = False) -> Dims:
    S = int(np.sqrt(2 * args.rnn_size))                       # model/model.py:57-58
    mno = _next_divisor_of_64(int(args.max_num_obj))
    if ref_compat:
        # the reference graph as written (model/model.py:116-311): raw pixels (:216-231), one eps per object (:262-263), 7 decoder
        # states re-read as seq_length points (:280-289), batch-norm in train phase on a batch of one object (:453,471)
        return Dims(n_scenes=n_scenes, mno=mno, K=1, T_obs=int(args.seq_length), T_pred=int(args.seq_length), H=int(args.d_dim),
                    L=int(args.latent_size), S=S, grid_size=int(getattr(args, "grid_size", 4)), posterior=1, sx=1.0, sy=1.0,
                    bn_mode=1, ref_compat=1, n_dec=int(getattr(args, "n_dec", 7)))
    w_img = float(getattr(args, "img_width", 2048.0))
    h_img = float(getattr(args, "img_height", 2048.0))
    nb = float(getattr(args, "neighborhood_size", 32))
    return Dims(
        n_scenes=n_scenes, mno=mno, K=int(getattr(args, "num_samples", 20)),
        T_obs=int(args.seq_length), T_pred=int(getattr(args, "pred_length", None) or args.seq_length),
        H=int(args.d_dim), L=int(args.latent_size), S=S,
        C=int(getattr(args, "scene_channels", 32)), Gh=int(getattr(args, "scene_grid", 64)),
        Gw=int(getattr(args, "scene_grid", 64)), n_grids=int(getattr(args, "n_grids", 1)),
        grid_size=int(getattr(args, "grid_size", 4)), E_v=16, iters=int(getattr(args, "ioc_iters", 1)),
        posterior=int(posterior), nb_w=nb / w_img, nb_h=nb / h_img, sx=1.0 / w_img, sy=1.0 / h_img,
        bin_mode=int(getattr(args, "social_layout", "rect") == "logpolar"),
        bn_mode={"frozen": 0, "per_object": 1, "batch": 2}[getattr(args, "batch_norm", "frozen")],
        bf16=_operand_mode(getattr(args, "bf16", False)),
        flags=_flags_from_args(args, {"frozen": 0, "per_object": 1, "batch": 2}[getattr(args, "batch_norm", "frozen")]))                          # DESIRE_FLAG_* bits: padding skipped unless --keep_padding / an explicit args.dims_flags


def _flags_from_args(args, bn_mode: int = 0) -> int:
    """desire_dims.flags from the argparse Namespace.  PADDING IS SKIPPED BY DEFAULT (round 6): the loader pads every window to max_num_obj slots
    (utils/data_loader.py:209-229; train.py:74 default 60, SDD frames hold ~8 objects) and the reference masks id-0 objects in the cost only
    (model/model.py:351-366), so DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC -- present rows bit-identical, absent rows zeros -- is on unless
      * args.keep_padding is set (train.py --keep_padding), or
      * args.dims_flags is given (an int: taken literally, plus train.py's --two_piece_forward / --skip_padding bits), or
      * the batch-norm mode is 'batch' (whole-batch statistics depend on the padding rows: the library refuses the combination)."""
    from .spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, FLAG_TRAIN_FWD_3P
    given = getattr(args, "dims_flags", None)
    f = int(given or 0)
    if getattr(args, "two_piece_forward", False):
        f |= FLAG_TRAIN_FWD_3P
    if getattr(args, "skip_padding", False) or (given is None and not getattr(args, "keep_padding", False) and bn_mode != 2):
        f |= FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC
    if getattr(args, "keep_padding", False):
        f &= ~(FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC)
    return f


def _operand_mode(v) -> int:
    """args.bf16 -> dims.bf16: False/0 fp32 operands, True/1 bf16 operands, 2 / "x3" / "split" split-bf16 operands (three products),
    3 / "x6" three bf16 pieces (six products, fp32-class accuracy)."""
    if isinstance(v, str):
        return {"": 0, "0": 0, "f32": 0, "1": 1, "bf16": 1, "2": 2, "x3": 2, "split": 2, "3": 3, "x6": 3}[v.lower()]
    return int(v) if int(v) in (0, 1, 2, 3) else 1


class PendingLoss(object):
    """Loss terms of a training step that has been ENQUEUED, not waited for.  get() blocks on the step's event (at most once) and returns
    the same dict train_step(sync=True) returns."""

    def __init__(self, host8, event, dev8):
        self._host8, self._event, self._dev8, self._terms = host8, event, dev8, None

    def done(self) -> bool:
        return self._terms is not None or self._event.query()

    def get(self) -> Dict[str, float]:
        if self._terms is None:
            self._event.synchronize()
            self._terms = _lib.Handle.loss_terms(self._host8.tolist())
            self._dev8 = None
        return self._terms


class DESIREModel(object):
    """Drop-in for model/model.py:29 DESIREModel(args)."""

    def __init__(self, args, weights: Optional[Dict[str, np.ndarray]] = None, seed: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise _lib.DesireError("DESIREModel needs an MI355X: there is no CPU path (oracle/ is test-only)")
        self.args = args
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.learning_rate = float(args.learning_rate)
        self.max_num_obj = int(args.max_num_obj)
        self.seq_length = int(args.seq_length)
        self.batch_size = int(getattr(args, "batch_size", 1))
        self._weights = weights
        self._head_given = bool(weights) and "gauss_head/w" in weights      # (restore() clears it when it had to fill the head in)
        self._seed = seed
        self._handles: Dict[Tuple[int, int, int], _lib.Handle] = {}
        self._trained = None                 # the handle train_step updates (weights + Adam moments live on the device)
        self._version = 0                    # bumped by every optimiser step
        self._weights_ver = 0                # version self._weights (host copy) corresponds to
        self._grids = None
        self._grid_of_scene = None
        self._images = None                  # set_scene_images: the library runs (and trains) the scene CNN
        # reference attribute names (model/model.py:62-75)
        self.input_data = None
        self.target_data = None
        self.cost = None
        self.gru_states = None
        self.final_states = None
        self.final_output = None

    # ---- plumbing -------------------------------------------------------------------------------
    def _weights_for(self, d: Dims) -> Dict[str, np.ndarray]:
        """self._weights in the shapes `d` wants.  Only ref_compat handles can differ from the model's own dims (they force K = 1 and
        T_pred = T_obs, so the IOC regression head [H, 2*T_pred] -- which ref_compat never runs -- is cut / zero-padded)."""
        want = weight_shapes(d)
        out = {}
        for k, v in self._weights.items():
            shp = want.get(k)
            v = np.asarray(v)
            if shp is None or tuple(v.shape) == tuple(shp):
                out[k] = v
                continue
            if not d.ref_compat or v.ndim != len(shp):
                raise ValueError("weight %s has shape %s, this call needs %s" % (k, v.shape, shp))
            fit = np.zeros(shp, np.float32)
            sl = tuple(slice(0, min(a, b)) for a, b in zip(v.shape, shp))
            fit[sl] = v[sl]
            out[k] = fit
        return out

    def _handle(self, n_scenes: int, posterior: bool, ref_compat: bool = False) -> _lib.Handle:
        key = (n_scenes, int(posterior), int(ref_compat))
        if key not in self._handles:
            d = dims_from_args(self.args, n_scenes, posterior, ref_compat)
            h = _lib.Handle(d)
            if self._weights is None:
                # always drawn for the model's OWN dims (a first call through forward_ref_compat must not size them for its T_pred = T_obs)
                self._weights = init_weights(dims_from_args(self.args, n_scenes, posterior, False), self._seed)
            h.set_weights(self._weights_for(d) if ref_compat else self._weights)
            h._wver = getattr(self, "_version", 0) if getattr(self, "_weights_ver", 0) == getattr(self, "_version", 0) else -1
            self._handles[key] = h
        h = self._handles[key]
        trained = getattr(self, "_trained", None)
        if trained is not None and h is not trained and getattr(h, "_wver", 0) != self._version:
            # the optimiser updates the weights inside the handle it trains on; any other handle (another batch size, the
            # prior path) gets the current values before it runs
            h.set_weights(self._weights_for(h.dims) if h.dims.ref_compat else self.sync_weights())
            h._wver = self._version
        return h

    def set_scene_grids(self, grids: np.ndarray, grid_of_scene: Sequence[int]) -> None:
        """grids [n_grids, Gh, Gw, C] scene features rho(I); grid_of_scene[i] = grid index of window i.  Detaches scene images."""
        self._grids = self.torch.as_tensor(np.ascontiguousarray(grids, np.float32), device=self.device)
        self._grid_of_scene = np.asarray(grid_of_scene, np.int32)
        self._images = None

    def set_scene_images(self, images, grid_of_scene: Sequence[int]) -> None:
        """images [n_grids, 4 Gh, 4 Gw, 3] (host array or device tensor): the library runs the scene CNN rho(I) on every forward that needs it,
        and train_step trains its weights scene_cnn/* through the IOC backward.  grid_of_scene[i] = image index of window i (replaced per batch by
        the grid_of_scene= argument of forward / train_step).  Detaches scene grids."""
        torch = self.torch
        img = images if torch.is_tensor(images) else torch.as_tensor(np.ascontiguousarray(images, np.float32))
        img = img.to(device=self.device, dtype=torch.float32).contiguous()
        if img.dim() != 4 or img.shape[-1] != 3:
            raise ValueError("scene images must be [n_grids, 4*Gh, 4*Gw, 3], got %s" % (tuple(img.shape),))
        self._images = img
        self._grids = None
        self._grid_of_scene = np.asarray(grid_of_scene, np.int32)

    def _attach_scene(self, h, n: int, grid_of_scene=None) -> None:
        """Gives handle h this batch's scene input -- the images (the handle runs the CNN) or the grids -- with the batch's grid_of_scene when
        given, else the stored mapping resized to n windows."""
        d = h.dims
        if grid_of_scene is not None:
            gos = np.ascontiguousarray(grid_of_scene, np.int32).reshape(-1)
            if gos.size != n:
                raise ValueError("grid_of_scene has %d entries for %d windows" % (gos.size, n))
        elif self._grid_of_scene is not None:
            gos = self._grid_of_scene if len(self._grid_of_scene) == n else np.resize(self._grid_of_scene, n)
        else:
            gos = np.zeros(n, np.int32)
        if getattr(self, "_images", None) is not None:
            img = self._images
            src = (img.data_ptr(), tuple(img.shape), gos.tobytes())
            if getattr(h, "_scene_src", None) != src:          # same images and mapping: the handle keeps its grid (no needless CNN rerun)
                h.set_scene_images(img.data_ptr(), int(img.shape[1]), int(img.shape[2]), gos)
                h._scene_src = src
            return
        if self._grids is None:
            self._grids = self.torch.zeros((d.n_grids, d.Gh, d.Gw, d.C), device=self.device)
            self._grid_of_scene = np.zeros(n, np.int32)
        h.set_scene_grids(self._grids.data_ptr(), gos)
        h._scene_src = None

    def _pad_windows(self, batch: Sequence[np.ndarray], mno: int):
        x = np.stack([np.asarray(b) for b in batch]).astype(np.float32)      # [n, T, MNO, 3]
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("windows must be [T, MNO, 3] arrays (id, x, y), got %s" % (x.shape[1:],))
        if x.shape[2] > mno:
            raise ValueError("windows hold %d object slots, the model was built for max_num_obj=%d" % (x.shape[2], self.max_num_obj))
        if x.shape[2] < mno:
            x = np.concatenate([x, np.zeros(x.shape[:2] + (mno - x.shape[2], 3), np.float32)], axis=2)
        return self.torch.as_tensor(np.ascontiguousarray(x), device=self.device)

    # ---- the hot path ---------------------------------------------------------------------------
    def forward(self, x_batch: Sequence[np.ndarray], y_batch: Optional[Sequence[np.ndarray]] = None,
                eps: Optional[np.ndarray] = None, seed: int = 0, grid_of_scene=None, device_rng: bool = False, window_base: int = 0):
        """x_batch: loader windows [T_obs, MNO, 3] (DataLoader.next_batch x); y_batch: future windows
        [T_pred, MNO, 3] or None (prior sampling).  Returns (Yhat [n, K, mno, T_pred, 2] normalised,
        score [n, K, mno]) as torch tensors on the GPU.  device_rng / window_base: see forward_device."""
        posterior = y_batch is not None
        d = self._handle(len(x_batch), posterior).dims
        past = self._pad_windows(x_batch, d.mno)
        fut = self._pad_windows(y_batch, d.mno) if posterior else None
        out = self.forward_device(past, fut, eps, seed, grid_of_scene=grid_of_scene, device_rng=device_rng, window_base=window_base)
        self.input_data, self.target_data = x_batch, y_batch
        return out

    def _eps(self, h, shape, eps, seed: int, device_rng: bool, window_base: int):
        """The eps tensor of a call, or None when the handle draws it itself (device_rng: the counter-based generator of desire_set_rng, seeded
        with `seed` at draw 0 and window origin `window_base` -- a window's noise then depends on its GLOBAL index, not on how the batch was cut)."""
        torch = self.torch
        if device_rng:
            if eps is not None:
                raise ValueError("device_rng draws eps on the device: eps must be None")
            h.set_rng(seed, 0, torch.cuda.current_stream().cuda_stream)
            h.set_rng_origin(window_base, 0)
            return None
        if eps is None:
            g = torch.Generator(device=self.device).manual_seed(seed)
            return torch.randn(shape, generator=g, device=self.device, dtype=torch.float32)
        if torch.is_tensor(eps):
            return eps.reshape(shape)
        return torch.as_tensor(np.ascontiguousarray(eps, np.float32), device=self.device).reshape(shape)

    def forward_device(self, past, fut=None, eps=None, seed: int = 0, grid_of_scene=None, device_rng: bool = False, window_base: int = 0):
        """forward() on windows that are already in HBM: past [n, T_obs, mno, 3], fut [n, T_pred, mno, 3] or None -- float32 device
        tensors in the loader's layout with the slot axis padded to the model's mno (what desire_amd.prefetch's feeders and
        forward_from_video produce).  Nothing here touches the host except the launches themselves.  device_rng=True: no eps tensor exists;
        the kernels draw the latent noise from (seed, draw 0, window_base + window, k, slot, latent) where they consume it."""
        torch = self.torch
        n = int(past.shape[0])
        posterior = fut is not None
        h = self._handle(n, posterior)
        d = h.dims
        if tuple(past.shape[1:]) != (d.T_obs, d.mno, 3) or (posterior and tuple(fut.shape[1:]) != (d.T_pred, d.mno, 3)):
            raise ValueError("window lengths must be (seq_length, pred_length) and the slot axis max_num_obj padded to %d" % d.mno)
        eps_t = self._eps(h, (d.R, d.L), eps, seed, device_rng, window_base)
        self._attach_scene(h, n, grid_of_scene)
        Y = torch.empty((n, d.K, d.mno, d.T_pred, 2), device=self.device, dtype=torch.float32)
        score = torch.empty((n, d.K, d.mno), device=self.device, dtype=torch.float32)
        stream = torch.cuda.current_stream().cuda_stream
        h.forward(past.data_ptr(), fut.data_ptr() if posterior else 0, 0 if eps_t is None else eps_t.data_ptr(), Y.data_ptr(),
                  score.data_ptr(), stream)
        self._keep = (past, fut, eps_t)            # keep inputs alive until the stream has consumed them
        self.final_output, self.final_states = Y, score
        if posterior:                              # train-path scalars (model/model.py:339-376): cost = mean(recon + kld)
            self._kld = torch.empty(d.A, device=self.device)
            self._recon = torch.empty(d.A, device=self.device)
            self._cost = torch.empty(2, device=self.device)
            h.losses(fut.data_ptr(), Y.data_ptr(), self._kld.data_ptr(), self._recon.data_ptr(), self._cost.data_ptr(), stream)
            self.cost = self._cost[0]              # 0-dim device tensor; float(model.cost) synchronises
        else:
            self.cost = None
        return Y, score

    def forward_ref_compat(self, x_batch: Sequence[np.ndarray], y_batch: Sequence[np.ndarray],
                           eps: Optional[np.ndarray] = None, seed: int = 0) -> Dict[str, "object"]:
        """The reference graph AS WRITTEN (model/model.py:116-311; dims.ref_compat) on loader batches: x_batch / y_batch are
        DataLoader.next_batch's x and y (y = x shifted one frame, utils/data_loader.py:206-207), [seq_length, MNO, 3] each, raw
        pixels.  Needs d_dim == 2*seq_length (:286-289).  eps [n, mno, L]: ONE draw per object (:262-263).  Returns device
        tensors: rho [n, mno, 200] (O1, :116-133), Hx / Hy [n, mno, H], output_states [n, mno, n_dec, seq_length, 2] (:280-289)
        and feature_pooling [n, mno, n_dec, seq_length, 200] (O11, :291-311).  The reference's graph stops there (:312-313)."""
        torch = self.torch
        n = len(x_batch)
        h = self._handle(n, True, ref_compat=True)
        d = h.dims
        past, fut = self._pad_windows(x_batch, d.mno), self._pad_windows(y_batch, d.mno)
        if past.shape[1] != d.T_obs or fut.shape[1] != d.T_obs:
            raise ValueError("ref_compat windows are seq_length frames each")
        if eps is None:
            g = torch.Generator(device=self.device).manual_seed(seed)
            eps_t = torch.randn((d.A, d.L), generator=g, device=self.device, dtype=torch.float32)
        else:
            eps_t = torch.as_tensor(np.ascontiguousarray(eps, np.float32), device=self.device).reshape(d.A, d.L)
        stream = torch.cuda.current_stream().cuda_stream
        states = torch.empty((n, d.mno, d.n_dec, d.T_obs, 2), device=self.device)
        rho = torch.empty((n, d.mno, 200), device=self.device)
        fp = torch.empty((n, d.mno, d.n_dec, d.T_obs, 200), device=self.device)
        h.forward(past.data_ptr(), fut.data_ptr(), eps_t.data_ptr(), states.data_ptr(), 0, stream)
        h.temporal_conv(past.data_ptr(), rho.data_ptr(), stream)
        h.feature_pooling(states.data_ptr(), rho.data_ptr(), fp.data_ptr(), stream)
        self._keep = (past, fut, eps_t)
        self.input_data, self.target_data = x_batch, y_batch
        HxHy = h.device_tensor("HxHy").view(n, d.mno, 2, -1)[..., : d.H]
        self.final_output = states
        return {"rho": rho, "Hx": HxHy[:, :, 0], "Hy": HxHy[:, :, 1], "output_states": states, "feature_pooling": fp}

    # ---- training (train.py:140-181 runs only `cost`; the Adam op of model/model.py:386-403 is never applied) ----
    def train_step(self, x_batch: Sequence[np.ndarray], y_batch: Sequence[np.ndarray], eps: Optional[np.ndarray] = None,
                   seed: int = 0, group=None, sync: bool = True, grid_of_scene=None, device_rng: bool = False, window_base: int = 0):
        """One optimiser step on a batch of loader windows: forward (posterior path), backward, gradient mean over
        the data-parallel ranks (RCCL all-reduce of ONE flat buffer when torch.distributed is initialised),
        clip_by_global_norm(args.grad_clip), Adam(args.learning_rate).  Returns the loss terms of DESIGN.md section 8
        evaluated BEFORE the update (what `sess.run([cost, train_op])` would have returned); with sync=False a PendingLoss
        whose .get() returns them later (see train_step_device)."""
        d = self._handle(len(x_batch), True).dims
        out = self.train_step_device(self._pad_windows(x_batch, d.mno), self._pad_windows(y_batch, d.mno), eps, seed, group, sync,
                                     grid_of_scene=grid_of_scene, device_rng=device_rng, window_base=window_base)
        self.input_data, self.target_data = x_batch, y_batch
        return out

    def train_step_device(self, past, fut, eps=None, seed: int = 0, group=None, sync: bool = True, grid_of_scene=None, device_rng: bool = False,
                          window_base: int = 0):
        """train_step on windows already in HBM (forward_device's layout).  device_rng=True: the step holds no eps tensor -- the forward draws
        it and the backward regenerates the same draw.  sync=False: nothing waits for the GPU -- the loss terms
        go to a device buffer (desire_train_loss_async), a pinned copy is enqueued, and the returned PendingLoss reads them when asked,
        normally one step later (desire_amd/train.py): the host runs ahead of the device and the loader thread is never starved by a
        read-back in the middle of every step."""
        from .dist import allreduce_mean_
        torch = self.torch
        h = self._handle(int(past.shape[0]), True)
        prev = getattr(self, "_trained", None)
        if prev is not None and prev is not h:
            raise ValueError("train_step was called with %d windows after training with %d: the Adam moments live in the handle "
                             "of one batch size (keep the batch size fixed, as DataLoader.next_batch does)"
                             % (int(past.shape[0]), prev.dims.n_scenes))
        if not getattr(h, "_training_on", False):
            h.set_training(True)
            h._training_on = True
            pending = self.__dict__.pop("_opt_pending", None)
            if pending is not None:                   # resumed run: Adam moments and step counter of the checkpoint
                h.set_opt_state(pending)
            self._configure_head_loss(h)
            self._configure_recon_loss(h)
        self.forward_device(past, fut, eps, seed, grid_of_scene=grid_of_scene, device_rng=device_rng, window_base=window_base)
        past, fut, eps_t = self._keep
        stream = torch.cuda.current_stream().cuda_stream
        h.backward(past.data_ptr(), fut.data_ptr(), 0 if eps_t is None else eps_t.data_ptr(), stream)
        allreduce_mean_(h.grad_tensor(), group)
        clip = float(getattr(self.args, "grad_clip", 0.0) or 0.0)
        if clip > 0:
            h.clip_grads(clip, stream=stream)
        if sync:
            terms = h.train_loss(fut.data_ptr(), stream)
        else:
            dev8 = torch.empty(8, device=self.device, dtype=torch.float32)
            h.train_loss_async(fut.data_ptr(), dev8.data_ptr(), stream)
            host8 = torch.empty(8, dtype=torch.float32).pin_memory()
            host8.copy_(dev8, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            terms = PendingLoss(host8, ev, dev8)
        h.adam_step(self.learning_rate, stream=stream)
        self._trained = h
        self._version = getattr(self, "_version", 0) + 1
        h._wver = self._version
        return terms

    def _configure_head_loss(self, h) -> None:
        """Hook of the Gaussian-head term (args.head_loss_weight; see train_step / DESIGN.md section 12)."""
        lam = float(getattr(self.args, "head_loss_weight", 0.0) or 0.0)
        if lam > 0.0 and hasattr(h, "set_head_loss"):
            h.set_head_loss(lam)
            self._head_given = True                   # the head is trained from now on: sample(mode="rollout") reads learned weights

    def _configure_recon_loss(self, h) -> None:
        """Hook of the reconstruction term over the K samples (args.recon_loss = "mean" | "min" | "softmin", args.recon_tau)."""
        mode = str(getattr(self.args, "recon_loss", None) or "mean")
        if mode not in RECON_MODES:
            raise ValueError("args.recon_loss must be one of %s, got %r" % (", ".join(RECON_MODES), mode))
        if mode != "mean":
            tau = getattr(self.args, "recon_tau", None)
            if mode == "softmin" and tau is None:
                raise ValueError("args.recon_loss = 'softmin' needs args.recon_tau > 0")
            h.set_recon_loss(RECON_MODES[mode], float(tau) if mode == "softmin" else 0.0)

    def sync_weights(self) -> Dict[str, np.ndarray]:
        """Pull the trained weights back from the device; other handles (batch sizes / prior path) are rebuilt lazily."""
        h = getattr(self, "_trained", None)
        if h is not None and getattr(self, "_weights_ver", 0) != self._version:
            self._weights = {k: h.get_weight(k, np.shape(v)) for k, v in self._weights.items()}
            self._weights_ver = self._version
        return self._weights

    def forward_from_video(self, frames, starts: Sequence[int], posterior: bool = True, eps=None, seed: int = 0, device_rng: bool = False,
                           window_base: int = 0):
        """Device-side batching: `frames` [F, max_num_obj, 3] is one preprocessed video
        (DataLoader.data[i]); the windows starting at `starts` are cut and slot-assigned on the GPU exactly like the x of
        DataLoader(seq_length = seq_length + pred_length).next_batch (slots ranked over the window plus the loader's one
        look-ahead frame), then run through the hot path without touching the host again."""
        torch = self.torch
        n = len(starts)
        h = self._handle(n, posterior)
        d = h.dims
        fr = torch.as_tensor(np.ascontiguousarray(np.asarray(frames), np.float32), device=self.device)
        past = torch.empty((n, d.T_obs, d.mno, 3), device=self.device)
        fut = torch.empty((n, d.T_pred, d.mno, 3), device=self.device)
        stream = torch.cuda.current_stream().cuda_stream
        h.build_windows(fr.data_ptr(), fr.shape[0], fr.shape[1], starts, past.data_ptr(), fut.data_ptr(), stream, lookahead=1)
        eps_t = self._eps(h, (d.R, d.L), eps, seed, device_rng, window_base)
        self._attach_scene(h, n)
        Y = torch.empty((n, d.K, d.mno, d.T_pred, 2), device=self.device, dtype=torch.float32)
        score = torch.empty((n, d.K, d.mno), device=self.device, dtype=torch.float32)
        h.forward(past.data_ptr(), fut.data_ptr() if posterior else 0, 0 if eps_t is None else eps_t.data_ptr(), Y.data_ptr(), score.data_ptr(), stream)
        self._keep = (fr, past, fut, eps_t)
        self.final_output, self.final_states = Y, score
        return Y, score, past, fut

    def evaluate(self, Y, fut_windows) -> np.ndarray:
        """[A, 4] = (ADE mean-of-K, FDE mean-of-K, ADE best-of-K, FDE best-of-K), normalised units (N4 harness).
        `fut_windows`: list of loader windows [T_pred, MNO, 3] or a device tensor [n, T_pred, mno, 3]."""
        torch = self.torch
        n = Y.shape[0]
        h = self._handle(n, True)
        d = h.dims
        fut = fut_windows if torch.is_tensor(fut_windows) else self._pad_windows(fut_windows, d.mno)
        out = torch.empty((d.A, 4), device=self.device)
        h.ade_fde(Y.data_ptr(), fut.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return out.cpu().numpy()

    # ---- ranking by IOC score (desire_rank_samples / desire_ranked_errors) ---------------------------------
    def rollout_samples(self, x_batch: Sequence[np.ndarray], normals=None, seed: int = 0, device_rng: bool = False, window_base: int = 0):
        """K rollouts of the Gaussian head per agent of a batch of observed loader windows [T_obs, MNO, 3], in ONE launch and in the sample layout:
        returns Y [n, K, mno, T_pred, 2] (normalised units, clipped to <= 1.0) on the GPU -- what forward() returns as Yhat, from the reference's
        own generator (sample(mode="rollout") K times).  normals [n, K, mno, T_pred, 2] ~ N(0,1) (array or device tensor), or None: torch's
        generator seeded with `seed`, or with device_rng=True drawn in the kernel from (seed, draw 0, window_base + window, k, slot, step) -- no
        noise tensor exists then.  Objects with id 0 are stepped like any other."""
        d = self._handle(len(x_batch), False).dims
        out = self.rollout_samples_device(self._pad_windows(x_batch, d.mno), normals, seed, device_rng=device_rng, window_base=window_base)
        self.input_data, self.target_data = x_batch, None
        return out

    def rollout_samples_device(self, past, normals=None, seed: int = 0, device_rng: bool = False, window_base: int = 0):
        """rollout_samples() on windows already in HBM (forward_device's layout)."""
        torch = self.torch
        n = int(past.shape[0])
        h = self._handle(n, False)
        d = h.dims
        if tuple(past.shape[1:]) != (d.T_obs, d.mno, 3):
            raise ValueError("windows must be seq_length frames with the slot axis max_num_obj padded to %d" % d.mno)
        stream = torch.cuda.current_stream().cuda_stream
        shape = (d.R, d.T_pred, 2)
        if device_rng:
            if normals is not None:
                raise ValueError("device_rng draws the rollout's normals on the device: normals must be None")
            h.set_rng(seed, 0, stream)
            h.set_rng_origin(window_base, 0)
            nrm = None
        elif normals is None:
            g = torch.Generator(device=self.device).manual_seed(seed)
            nrm = torch.randn(shape, generator=g, device=self.device, dtype=torch.float32)
        elif torch.is_tensor(normals):
            nrm = normals.to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()
        else:
            nrm = torch.as_tensor(np.ascontiguousarray(normals, np.float32), device=self.device).reshape(shape)
        Y = torch.empty((n, d.K, d.mno, d.T_pred, 2), device=self.device, dtype=torch.float32)
        h.rollout_samples(past.data_ptr(), 0 if nrm is None else nrm.data_ptr(), Y.data_ptr(), stream)
        self._keep = (past, nrm)                   # keep inputs alive until the stream has consumed them
        return Y

    def _rollout_forward_device(self, past, normals, seed: int, grid_of_scene, device_rng: bool, window_base: int):
        """forward_device() with the head rollout as the generator: encode (the IOC stage reads its Hx, last positions and presence flags), K
        rollouts per agent, IOC scoring + refinement.  Returns (Y, score) like forward_device."""
        torch = self.torch
        if not getattr(self, "_head_given", False):
            import warnings
            warnings.warn("generator='rollout' reads gauss_head/w|b, which train_step trains only with args.head_loss_weight > 0; this "
                          "model's head holds its random initial values (train it, pass weights= with a trained head, or use generator='cvae')",
                          stacklevel=3)
        n = int(past.shape[0])
        h = self._handle(n, False)
        d = h.dims
        if tuple(past.shape[1:]) != (d.T_obs, d.mno, 3):
            raise ValueError("windows must be seq_length frames with the slot axis max_num_obj padded to %d" % d.mno)
        self._attach_scene(h, n, grid_of_scene)
        stream = torch.cuda.current_stream().cuda_stream
        h.encode(past.data_ptr(), 0, stream)
        Y = self.rollout_samples_device(past, normals, seed, device_rng=device_rng, window_base=window_base)
        score = torch.empty((n, d.K, d.mno), device=self.device, dtype=torch.float32)
        h.ioc_refine(Y.data_ptr(), score.data_ptr(), stream)
        self.final_output, self.final_states, self.cost = Y, score, None
        return Y, score

    @staticmethod
    def _nms_args(select: str, nms_radius, nms_metric: str, nms_horizon, T_pred: int):
        """None for select="score"; (metric, t_end, radius in pixels) for select="nms"."""
        if select == "score":
            return None
        if select != "nms":
            raise ValueError("select must be 'score' (the best-scored samples), 'nms' (score-ordered non-maximum suppression) or 'joint' (the best-scored "
                             "joint samples of the window), got %r" % (select,))
        if nms_radius is None:
            raise ValueError("select='nms' needs nms_radius (pixels)")
        metrics = {"final": _lib.DIST_FINAL, "mean": _lib.DIST_MEAN, "max": _lib.DIST_MAX}
        if nms_metric not in metrics:
            raise ValueError("nms_metric must be 'final', 'mean' or 'max', got %r" % (nms_metric,))
        t_end = T_pred if nms_horizon is None else int(nms_horizon)
        if not 1 <= t_end <= T_pred:
            raise ValueError("nms_horizon must be 1..pred_length (%d), got %d" % (T_pred, t_end))
        return metrics[nms_metric], t_end, float(nms_radius)

    def predict(self, x_batch: Sequence[np.ndarray], top: Optional[int] = None, eps=None, seed: int = 0, grid_of_scene=None, device_rng: bool = False,
                window_base: int = 0, generator: str = "cvae", normals=None, select: str = "score", nms_radius=None, nms_metric: str = "final",
                nms_horizon=None, collision_radius=None):
        """The `top` most plausible futures of every agent of a batch of observed loader windows [T_obs, MNO, 3], ranked by IOC score
        (prior sampling: no future given).  See predict_device for the result."""
        d = self._handle(len(x_batch), False).dims
        out = self.predict_device(self._pad_windows(x_batch, d.mno), top, eps, seed, grid_of_scene=grid_of_scene, device_rng=device_rng,
                                  window_base=window_base, generator=generator, normals=normals, select=select, nms_radius=nms_radius,
                                  nms_metric=nms_metric, nms_horizon=nms_horizon, collision_radius=collision_radius)
        self.input_data, self.target_data = x_batch, None
        return out

    def predict_device(self, past, top: Optional[int] = None, eps=None, seed: int = 0, grid_of_scene=None, device_rng: bool = False, window_base: int = 0,
                       generator: str = "cvae", normals=None, select: str = "score", nms_radius=None, nms_metric: str = "final", nms_horizon=None,
                       collision_radius=None):
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
        of that joint sample that come within collision_radius pixels (None: 0, nothing touches) of another one at some frame."""
        torch = self.torch
        joint = select == "joint"
        if collision_radius is not None and not joint:
            raise ValueError("collision_radius belongs to select='joint'")
        if joint and collision_radius is not None and not (np.isfinite(float(collision_radius)) and float(collision_radius) >= 0):
            raise ValueError("collision_radius must be finite and >= 0 (pixels), got %r" % (collision_radius,))
        nms = None if joint else self._nms_args(select, nms_radius, nms_metric, None, 1)      # refuse a bad selection before the forward runs (the horizon: below)
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
        n = int(past.shape[0])
        h = self._handle(n, False)
        d = h.dims
        top = default_top(d.K) if top is None else int(top)
        if not 1 <= top <= d.K:
            raise ValueError("top must be 1..num_samples (%d), got %d" % (d.K, top))
        order = torch.empty((n, d.mno, d.K), device=self.device, dtype=torch.int32)
        traj = torch.empty((n, d.mno, top, d.T_pred, 2), device=self.device, dtype=torch.float32)
        sc = torch.empty((n, d.mno, top), device=self.device, dtype=torch.float32)
        stream = torch.cuda.current_stream().cuda_stream
        if joint:
            present = past[:, -1, :, 0] != 0
            pres8 = present.to(torch.uint8).contiguous()
            cnt = torch.empty((n, d.K + 1, 1, 2), device=self.device, dtype=torch.int32)
            jscore = torch.empty((n, d.K), device=self.device, dtype=torch.float32)
            jorder = torch.empty((n, d.K), device=self.device, dtype=torch.int32)
            h.joint_metrics(Y.data_ptr(), 0, pres8.data_ptr(), score.data_ptr(), [d.T_pred], top, float(collision_radius or 0.0), 1.0 / d.sx, 1.0 / d.sy,
                            cnt.data_ptr(), jorder.data_ptr(), 0, 0, jscore.data_ptr(), 0, stream)
            idx = jorder[:, :top].long()                                     # [n, top]: the joint samples, best first
            w = torch.arange(n, device=self.device)[:, None]
            traj = (Y[w, idx].permute(0, 2, 1, 3, 4) / torch.tensor([d.sx, d.sy], device=self.device, dtype=torch.float32)).contiguous()
            return {"traj": traj, "score": score[w, idx].permute(0, 2, 1).contiguous(), "order": jorder[:, None, :].expand(n, d.mno, d.K).contiguous(),
                    "present": present, "joint_score": jscore[w, idx], "collisions": cnt[:, :d.K, 0, 0][w, idx]}
        if nms is None:
            h.rank_samples(score.data_ptr(), Y.data_ptr(), top, order.data_ptr(), traj.data_ptr(), sc.data_ptr(), stream)
            traj /= torch.tensor([d.sx, d.sy], device=self.device, dtype=torch.float32)
            return {"traj": traj, "score": sc, "order": order, "present": past[:, -1, :, 0] != 0}
        metric, t_end, radius = self._nms_args(select, nms_radius, nms_metric, nms_horizon, d.T_pred)
        by_score = torch.empty((n, d.mno, d.K), device=self.device, dtype=torch.int32)
        count = torch.empty((n, d.mno), device=self.device, dtype=torch.int32)
        mass = torch.empty((n, d.mno, d.K), device=self.device, dtype=torch.float32)
        h.rank_samples(score.data_ptr(), 0, top, by_score.data_ptr(), 0, 0, stream)
        h.select_diverse(Y.data_ptr(), by_score.data_ptr(), score.data_ptr(), metric, t_end, radius, 1.0 / d.sx, 1.0 / d.sy, top, order.data_ptr(),
                         count.data_ptr(), mass.data_ptr(), traj.data_ptr(), sc.data_ptr(), stream)
        traj /= torch.tensor([d.sx, d.sy], device=self.device, dtype=torch.float32)
        return {"traj": traj, "score": sc, "order": order, "present": past[:, -1, :, 0] != 0, "count": count,
                "prob": mass[:, :, :top].contiguous()}

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
        torch = self.torch
        n = int(Y.shape[0])
        h = self._handles.get((n, 0, 0)) or self._handle(n, True)
        d = h.dims
        nms = self._nms_args(select, nms_radius, nms_metric, nms_horizon, d.T_pred)
        if return_count and nms is None:
            raise ValueError("return_count needs select='nms'")
        top = default_top(d.K) if top is None else int(top)
        hz = default_horizons(d.T_pred) if horizons is None else [int(x) for x in horizons]
        ux, uy, _ = self._unit_scale(units, d)
        fut = fut_windows if torch.is_tensor(fut_windows) else self._pad_windows(fut_windows, d.mno)
        stream = torch.cuda.current_stream().cuda_stream
        order = torch.empty((d.A, d.K), device=self.device, dtype=torch.int32)
        out = torch.empty((d.A, len(hz), 4), device=self.device, dtype=torch.float32)
        h.rank_samples(score.data_ptr(), 0, top, order.data_ptr(), 0, 0, stream)
        if nms is not None:
            diverse = torch.empty_like(order)
            count = torch.empty((d.A,), device=self.device, dtype=torch.int32)
            h.select_diverse(Y.data_ptr(), order.data_ptr(), score.data_ptr(), nms[0], nms[1], nms[2], 1.0 / d.sx, 1.0 / d.sy, top,
                             diverse.data_ptr(), count.data_ptr(), 0, 0, 0, stream)
            order = diverse
        h.ranked_errors(Y.data_ptr(), fut.data_ptr(), order.data_ptr(), top, hz, ux, uy, out.data_ptr(), stream)
        return (out.cpu().numpy(), count.cpu().numpy()) if return_count else out.cpu().numpy()

    def evaluate_joint(self, Y, score, fut_windows, top: Optional[int] = None, horizons=None, units="px", collision_radius=None) -> dict:
        """The K samples of every window as K JOINT futures of the scene (desire_joint_metrics).  Returns numpy arrays: "jerr" [n, K, n_h, 2] =
        (JADE_h, JFDE_h): the mean over the agents that take part before the horizon of each agent's ADE_h / FDE_h under sample k; "jscore" [n, K] the
        scores summed over the agents that take part; "order" [n, K] the joint samples by descending joint score; "out" [n, n_h, 4] = (JADE, JFDE
        of the best-scored joint sample, best JADE, best JFDE among the `top` best-scored); "first" [n, K + 1, mno] int32 the first frame at which an
        agent comes within collision_radius of another agent of the same joint sample (T_pred: never), row K being the ground truth under the same
        rule; "cnt" [n, K + 1, n_h, 2] int32 = (agents touching, agents taking part) before each horizon -- the collision rate is cnt[..., 0] /
        cnt[..., 1].  units, horizons, top and `fut_windows` as in evaluate_ranked; collision_radius in pixels, converted to the call's unit (units
        "norm": along x); None: radius 0, nothing touches."""
        torch = self.torch
        n = int(Y.shape[0])
        h = self._handles.get((n, 0, 0)) or self._handle(n, True)
        d = h.dims
        top = default_top(d.K) if top is None else int(top)
        hz = default_horizons(d.T_pred) if horizons is None else [int(x) for x in horizons]
        r_px = 0.0 if collision_radius is None else float(collision_radius)
        ux, uy, f = self._unit_scale(units, d)
        radius = r_px * f
        fut = fut_windows if torch.is_tensor(fut_windows) else self._pad_windows(fut_windows, d.mno)
        stream = torch.cuda.current_stream().cuda_stream
        dev, i32 = self.device, torch.int32
        res = {"jerr": torch.empty((n, d.K, len(hz), 2), device=dev), "out": torch.empty((n, len(hz), 4), device=dev),
               "order": torch.empty((n, d.K), device=dev, dtype=i32), "jscore": torch.empty((n, d.K), device=dev),
               "cnt": torch.empty((n, d.K + 1, len(hz), 2), device=dev, dtype=i32), "first": torch.empty((n, d.K + 1, d.mno), device=dev, dtype=i32)}
        h.joint_metrics(Y.data_ptr(), fut.data_ptr(), 0, 0 if score is None else score.data_ptr(), hz, top, radius, ux, uy, res["cnt"].data_ptr(),
                        res["order"].data_ptr(), res["first"].data_ptr(), res["jerr"].data_ptr(), res["jscore"].data_ptr(), res["out"].data_ptr(), stream)
        return {k: v.cpu().numpy() for k, v in res.items()}

    def _plan_risk(self, h, Y, fut, present, score, plans, ego, hz, radius, ux, uy):
        """One desire_plan_risk call on device tensors: plans [n, M, T_pred, 2] normalised, ego [n, M] int32 or None.  Device tensors back."""
        torch = self.torch
        d = h.dims
        n, M, nh = d.n_scenes, int(plans.shape[1]), len(hz)
        dev, i32 = self.device, torch.int32
        res = {"risk": torch.empty((n, M, nh), device=dev), "first": torch.empty((n, M, d.K + 1), device=dev, dtype=i32),
               "clear": torch.empty((n, M, d.K + 1, nh), device=dev), "blame": torch.empty((n, M, nh, d.mno), device=dev)}
        ptr = lambda x: 0 if x is None else x.data_ptr()
        h.plan_risk(Y.data_ptr(), ptr(fut), ptr(present), ptr(score), plans.data_ptr(), ptr(ego), M, hz, radius, ux, uy, res["risk"].data_ptr(),
                    res["first"].data_ptr(), res["clear"].data_ptr(), res["blame"].data_ptr(), torch.cuda.current_stream().cuda_stream)
        return res

    def score_plans(self, past, plans, collision_radius, horizons=None, ego_slot=None, weights: str = "score", **predict_kwargs) -> dict:
        """M candidate trajectories of the planner's own vehicle per window against the K joint futures the model predicts: the forward as
        predict_device runs it (predict_kwargs: eps, seed, grid_of_scene, device_rng, window_base), then one desire_plan_risk call in its
        prediction form (an agent counts when its id is != 0 at the last observed frame).  `past`: loader windows [T_obs, MNO, 3] or
        predict_device's tensor; plans [n, M, T_pred, 2] IN PIXELS (scaled like the observed positions; a NaN frame: the plan is not defined
        there); collision_radius in pixels, finite and >= 0; ego_slot [n, M] (or [n]: one slot for every plan of the window) = the slot the plan
        replaces, negative or None: nobody.  Returns device tensors: "risk" [n, M, n_h] = the weight of the joint futures in which the plan comes
        within the radius of somebody before the horizon (weights "score": softmax of the joint scores; "uniform": 1 / K), "clearance"
        [n, M, K, n_h] = the smallest distance in pixels to anybody before the horizon (inf: nobody there), "first" [n, M, K] int32 = the frame
        of the first contact (T_pred: none), "blame" [n, M, n_h, mno] = the risk by the agent touched, "present" [n, mno] and "best" [n, n_h] =
        per horizon the plan of least risk, ties to the greater clearance (its smallest over the K futures), then to the lower index."""
        torch = self.torch
        if weights not in ("score", "uniform"):
            raise ValueError("weights must be 'score' (softmax of the joint scores) or 'uniform', got %r" % (weights,))
        if not (np.isfinite(float(collision_radius)) and float(collision_radius) >= 0):
            raise ValueError("collision_radius must be finite and >= 0 (pixels), got %r" % (collision_radius,))
        if not torch.is_tensor(past):
            past = self._pad_windows(past, self._handle(len(past), False).dims.mno)
        n = int(past.shape[0])
        d = self._handle(n, False).dims
        hz = default_horizons(d.T_pred) if horizons is None else [int(x) for x in horizons]
        P = torch.as_tensor(plans, device=self.device).to(torch.float32)
        if P.dim() != 4 or int(P.shape[0]) != n or int(P.shape[1]) < 1 or tuple(P.shape[2:]) != (d.T_pred, 2):
            raise ValueError("plans must be [n, M, T_pred, 2] in pixels with M >= 1, got %s" % (tuple(P.shape),))
        M = int(P.shape[1])
        P = (P * torch.tensor([d.sx, d.sy], device=self.device, dtype=torch.float32)).contiguous()
        ego = None
        if ego_slot is not None:
            ego = torch.as_tensor(ego_slot, device=self.device).to(torch.int32)
            ego = (ego[:, None].expand(n, M) if ego.dim() == 1 else ego).contiguous()
            if tuple(ego.shape) != (n, M):
                raise ValueError("ego_slot must be [n, M] or [n], got %s" % (tuple(ego.shape),))
        Y, score = self.forward_device(past, None, **predict_kwargs)
        h = self._handle(n, False)
        present = past[:, -1, :, 0] != 0
        res = self._plan_risk(h, Y, None, present.to(torch.uint8).contiguous(), score if weights == "score" else None, P, ego, hz,
                              float(collision_radius), 1.0 / d.sx, 1.0 / d.sy)
        clearance = res["clear"][:, :, :d.K].sqrt()
        worst = clearance.min(2).values                                        # [n, M, n_h]
        least = res["risk"] == res["risk"].min(1, keepdim=True).values
        room = torch.where(least, worst, torch.full_like(worst, -1.0))
        pick = least & (room == room.max(1, keepdim=True).values)
        idx = torch.arange(M, device=self.device)[None, :, None].expand_as(pick)
        best = torch.where(pick, idx, torch.full_like(idx, M)).min(1).values
        return {"risk": res["risk"], "clearance": clearance, "first": res["first"][:, :, :d.K].contiguous(), "blame": res["blame"],
                "present": present, "best": best}

    def evaluate_plan_risk(self, Y, score, fut_windows, collision_radius, horizons=None, weights: str = "score") -> dict:
        """Leave-one-out check of the predicted interactions that needs no planner: plan m of a window is what agent m actually did (its
        recorded future, undefined where it is not counted), replacing slot m, held against the K joint futures of the others.  Returns numpy
        arrays: "risk" [n, mno, n_h] = the predicted risk of what each agent did, "first" [n, mno, K + 1] int32 (row K: against the recorded
        futures of the others), "takes_part" [n, mno, n_h] bool, and per horizon over the agents taking part before it "predicted" [n_h] = the
        mean predicted risk, "actual" [n_h] = the rate at which they actually came within collision_radius (pixels) of somebody, "agents" [n_h].
        A predictor that is calibrated about interactions brings the two columns close."""
        torch = self.torch
        if weights not in ("score", "uniform"):
            raise ValueError("weights must be 'score' (softmax of the joint scores) or 'uniform', got %r" % (weights,))
        n = int(Y.shape[0])
        h = self._handles.get((n, 0, 0)) or self._handle(n, True)
        d = h.dims
        hz = default_horizons(d.T_pred) if horizons is None else [int(x) for x in horizons]
        fut = fut_windows if torch.is_tensor(fut_windows) else self._pad_windows(fut_windows, d.mno)
        counted = (fut[..., 0] != 0).permute(0, 2, 1)                          # [n, mno, T_pred]
        g = (fut[..., 1:] * torch.tensor([d.sx, d.sy], device=self.device, dtype=torch.float32)).permute(0, 2, 1, 3)
        plans = torch.where(counted[..., None], g, torch.full_like(g, float("nan"))).contiguous()
        ego = torch.arange(d.mno, device=self.device, dtype=torch.int32)[None].expand(n, d.mno).contiguous()
        res = self._plan_risk(h, Y, fut, None, score if weights == "score" else None, plans, ego, hz, float(collision_radius), 1.0 / d.sx, 1.0 / d.sy)
        takes = torch.stack([counted[:, :, :x].any(-1) for x in hz], -1)       # [n, mno, n_h]
        hit = res["first"][:, :, d.K, None] < torch.tensor(hz, device=self.device, dtype=torch.int32)[None, None]
        agents = takes.sum((0, 1)).to(torch.float64)
        predicted = torch.where(takes, res["risk"], torch.zeros_like(res["risk"])).to(torch.float64).sum((0, 1))
        actual = (takes & hit).sum((0, 1)).to(torch.float64)
        den = agents.clamp(min=1)
        return {"risk": res["risk"].cpu().numpy(), "first": res["first"].cpu().numpy(), "takes_part": takes.cpu().numpy(),
                "predicted": (predicted / den).cpu().numpy(), "actual": (actual / den).cpu().numpy(), "agents": agents.cpu().numpy().astype(np.int64)}

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
        if weights not in ("score", "uniform"):
            raise ValueError("weights must be 'score' (softmax of the IOC scores) or 'uniform', got %r" % (weights,))
        return n, int(iters)

    def _fit_modes(self, h, Y, score, fut, n, seeds, nms, iters, t_end, ux, uy, var_floor, weighted, hz=None, log_floor=_lib.KDE_LOG_FLOOR):
        """Rank (and the non-maximum suppression with seeds "nms"), then one desire_fit_modes call, on device tensors.  Device tensors back, shaped
        per window and slot."""
        torch = self.torch
        d = h.dims
        dev, i32 = self.device, torch.int32
        N, m = d.n_scenes, d.mno
        stream = torch.cuda.current_stream().cuda_stream
        order = torch.empty((d.A, d.K), device=dev, dtype=i32)
        h.rank_samples(score.data_ptr(), 0, n, order.data_ptr(), 0, 0, stream)
        if seeds == "nms":
            diverse, kept = torch.empty_like(order), torch.empty((d.A,), device=dev, dtype=i32)
            h.select_diverse(Y.data_ptr(), order.data_ptr(), score.data_ptr(), nms[0], nms[1], nms[2], 1.0 / d.sx, 1.0 / d.sy, n, diverse.data_ptr(),
                             kept.data_ptr(), 0, 0, 0, stream)
            order = diverse
        res = {"mean": torch.empty((N, m, n, d.T_pred, 2), device=dev), "cov": torch.empty((N, m, n, d.T_pred, 3), device=dev),
               "prob": torch.empty((N, m, n), device=dev), "label": torch.empty((N, m, d.K), device=dev, dtype=i32),
               "count": torch.empty((N, m, n), device=dev, dtype=i32), "passes": torch.empty((N, m), device=dev, dtype=i32)}
        if fut is not None:
            res["nll"] = torch.empty((N, m, len(hz), 2), device=dev)
        h.fit_modes(Y.data_ptr(), order.data_ptr(), score.data_ptr() if weighted else 0, n, t_end, iters, ux, uy, var_floor, res["count"].data_ptr(),
                    res["prob"].data_ptr(), res["label"].data_ptr(), res["mean"].data_ptr(), res["cov"].data_ptr(), res["passes"].data_ptr(),
                    0 if fut is None else fut.data_ptr(), hz, float(log_floor), res["nll"].data_ptr() if fut is not None else 0, 0, stream)
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
        torch = self.torch
        if not torch.is_tensor(past):
            past = self._pad_windows(past, self._handle(len(past), False).dims.mno)
        n_w = int(past.shape[0])
        d = self._handle(n_w, False).dims
        n, iters = self._modes_args(d, modes, seeds, nms_radius, iters, min_std, weights)     # refused before the forward runs
        nms = self._nms_args("nms", nms_radius, nms_metric, horizon, d.T_pred) if seeds == "nms" else None
        t_end = d.T_pred if horizon is None else int(horizon)
        if not 1 <= t_end <= d.T_pred:
            raise ValueError("horizon must be 1..pred_length (%d), got %d" % (d.T_pred, t_end))
        Y, score = self.forward_device(past, None, **predict_kwargs)
        h = self._handle(n_w, False)
        res = self._fit_modes(h, Y, score, None, n, seeds, nms, iters, t_end, 1.0 / d.sx, 1.0 / d.sy, float(min_std) ** 2, weights == "score")
        res["mean"] /= torch.tensor([d.sx, d.sy], device=self.device, dtype=torch.float32)
        res["present"] = past[:, -1, :, 0] != 0
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
        N = int(Y.shape[0])
        h = self._handles.get((N, 0, 0)) or self._handle(N, True)
        d = h.dims
        n, iters = self._modes_args(d, modes, seeds, nms_radius, iters, min_std, weights)
        nms = self._nms_args("nms", nms_radius, nms_metric, horizon, d.T_pred) if seeds == "nms" else None
        t_end = d.T_pred if horizon is None else int(horizon)
        hz = default_horizons(d.T_pred) if horizons is None else [int(x) for x in horizons]
        ux, uy, f = self._unit_scale(units, d)
        fut = fut_windows if torch.is_tensor(fut_windows) else self._pad_windows(fut_windows, d.mno)
        res = self._fit_modes(h, Y, score, fut, n, seeds, nms, iters, t_end, ux, uy, (float(min_std) * f) ** 2, weights == "score", hz, log_floor)
        # the errors of the means: torch on the small [A, n, T, 2] tensor
        mean = res["mean"].reshape(d.A, n, d.T_pred, 2)
        prob = res["prob"].reshape(d.A, n)
        counted = (fut[..., 0] != 0).permute(0, 2, 1).reshape(d.A, d.T_pred)
        g = (fut[..., 1:] * torch.tensor([d.sx, d.sy], device=self.device, dtype=torch.float32)).permute(0, 2, 1, 3).reshape(d.A, 1, d.T_pred, 2)
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

    def _occupancy_args(self, d, grid, horizons, mode, weights, mask, mask_of_window, n):
        """(Oh, Ow, horizons, mode id, mask tensor or None, mask_of_window tensor or None) of the occupancy calls, refused here where they are bad."""
        torch = self.torch
        Oh, Ow = (int(x) for x in grid)
        if mode not in _lib.OCC_MODES:
            raise ValueError("mode must be 'at' (the frame h - 1) or 'until' (any frame before h), got %r" % (mode,))
        if weights not in ("score", "uniform"):
            raise ValueError("weights must be 'score' (softmax of the IOC scores) or 'uniform', got %r" % (weights,))
        hz = default_horizons(d.T_pred) if horizons is None else [int(x) for x in horizons]
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
        ptr = lambda x: 0 if x is None else x.data_ptr()
        h.occupancy(Y.data_ptr(), ptr(fut), ptr(present), ptr(score), hz, mode, Oh, Ow, res["occ"].data_ptr(), res["expected"].data_ptr(),
                    ptr(res.get("hit")), ptr(res.get("violation")), res["off"].data_ptr(), ptr(mask), ptr(mow), torch.cuda.current_stream().cuda_stream)
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
        n = int(past.shape[0])
        args = self._occupancy_args(self._handle(n, False).dims, grid, horizons, mode, weights, mask, mask_of_window, n)      # refused before the forward runs
        Y, score = self.forward_device(past, None, eps, seed, grid_of_scene=grid_of_scene, device_rng=device_rng, window_base=window_base)
        h = self._handle(n, False)
        present = past[:, -1, :, 0] != 0
        res = self._occupancy(h, Y, None, present.to(self.torch.uint8).contiguous(), score if weights == "score" else None, args, False)
        res["present"] = present
        return res

    def evaluate_occupancy(self, Y, score, fut_windows, grid, horizons=None, mode: str = "at", weights: str = "score", mask=None,
                           mask_of_window=None) -> dict:
        """The occupancy maps of samples Y [n, K, mno, T_pred, 2] (and scores) against their futures: desire_occupancy in its evaluation form (a frame
        counts when the object is in it).  Returns numpy arrays: "occ", "expected", "off" and "violation" as predict_occupancy, and in mode "at"
        "hit" [n, mno, n_h] = the weight of the agent's samples in the cell the ground truth is in at frame h - 1 (0 where it is not counted or off
        the frame).  `fut_windows`, horizons as in evaluate_ranked; weights "score" needs `score`."""
        torch = self.torch
        n = int(Y.shape[0])
        h = self._handles.get((n, 0, 0)) or self._handle(n, True)
        d = h.dims
        args = self._occupancy_args(d, grid, horizons, mode, weights, mask, mask_of_window, n)
        if weights == "score" and score is None:
            raise ValueError("weights='score' needs the IOC scores")
        fut = fut_windows if torch.is_tensor(fut_windows) else self._pad_windows(fut_windows, d.mno)
        res = self._occupancy(h, Y, fut, None, score if weights == "score" else None, args, mode == "at")
        return {k: v.cpu().numpy() for k, v in res.items()}

    def evaluate_nll(self, Y, score, fut_windows, horizons=None, units="px", weighted: bool = False, log_floor: float = _lib.KDE_LOG_FLOOR,
                     return_frames: bool = False):
        """[A, n_h, 2] = per horizon (mean, final) KDE negative log-likelihood of the ground truth under the agent's K samples: at every counted
        frame a Gaussian kernel density (Scott's bandwidth, scipy.stats.gaussian_kde's fit) over the K sampled positions, its log at the ground
        truth clipped below at log_floor, averaged over the counted frames before the horizon / taken at the last of them; zeros where there is
        none.  weighted=False: equal weights; True: the weights softmax(score) that the ranking loss trains the IOC scores as.  The density is
        per unit^2: units, horizons and `fut_windows` as in evaluate_ranked.  return_frames=True: also the per-frame log-densities [A, T_pred]
        (0 where a frame is not counted)."""
        torch = self.torch
        n = int(Y.shape[0])
        h = self._handles.get((n, 0, 0)) or self._handle(n, True)
        d = h.dims
        hz = default_horizons(d.T_pred) if horizons is None else [int(x) for x in horizons]
        ux, uy, _ = self._unit_scale(units, d)
        if weighted and score is None:
            raise ValueError("weighted=True needs the IOC scores")
        fut = fut_windows if torch.is_tensor(fut_windows) else self._pad_windows(fut_windows, d.mno)
        stream = torch.cuda.current_stream().cuda_stream
        out = torch.empty((d.A, len(hz), 2), device=self.device, dtype=torch.float32)
        frames = torch.empty((d.A, d.T_pred), device=self.device, dtype=torch.float32) if return_frames else None
        h.kde_nll(Y.data_ptr(), fut.data_ptr(), score.data_ptr() if weighted else 0, hz, ux, uy, float(log_floor), out.data_ptr(),
                  frames.data_ptr() if return_frames else 0, stream)
        return (out.cpu().numpy(), frames.cpu().numpy()) if return_frames else out.cpu().numpy()

    # ---- checkpoints (train.py:114,197-206 saves TF checkpoints; here: a named fp32 archive) -----------------
    def save(self, path: str) -> None:
        from .formats import save_weights
        if self._weights is None:
            raise ValueError("no weights yet: run forward() once or pass weights=")
        blob = dict(self.sync_weights())
        # whether gauss_head/* holds trained (or caller-supplied) values rather than the random init: an archive always carries the head, so
        # key presence says nothing -- restore() reads this marker to pick sample()'s default mode
        blob["meta/head_trained"] = np.asarray([1.0 if getattr(self, "_head_given", False) else 0.0], np.float32)
        h = getattr(self, "_trained", None)
        if h is not None:                             # the reference's Saver keeps the optimiser slots too (train.py:114)
            for k, v in h.opt_state().items():
                blob["opt/" + k] = v
        save_weights(path, blob)

    @classmethod
    def restore(cls, args, path: str) -> "DESIREModel":
        from .formats import load_weights
        blob = load_weights(path)
        opt = {k[4:]: blob.pop(k) for k in list(blob) if k.startswith("opt/")}
        meta = {k[5:]: blob.pop(k) for k in list(blob) if k.startswith("meta/")}
        # archives of rounds 2-4 carry no marker: the rule they were written under applies (a head that is in the archive counts as given), so a
        # checkpoint trained with --head_loss_weight > 0 keeps sample()'s default mode 'rollout' (INTEGRATION.md "Checkpoints")
        head_trained = bool(float(np.asarray(meta["head_trained"]).reshape(-1)[0])) if "head_trained" in meta else ("gauss_head/w" in blob)
        # archives written before an auxiliary weight existed (the sample() head "gauss_head/*" came with round 2): complete them
        # with the values init_weights draws, so an older checkpoint still loads
        d0 = dims_from_args(args, 1, True)
        missing = [k for k in weight_shapes(d0) if k not in blob]
        if missing:
            fresh = init_weights(d0, 0)
            unknown = [k for k in missing if not k.startswith("gauss_head/")]
            if unknown:
                raise ValueError("checkpoint %s lacks weights %s" % (path, unknown))
            for k in missing:
                blob[k] = fresh[k]
            if opt:                                   # moments of the flat buffer no longer line up: Adam restarts from zero
                opt = {}
        m = cls(args, weights=blob)
        m._head_given = head_trained and not missing      # NOT key presence: save() writes the head whether or not anything ever trained it
        if opt:
            m._opt_pending = opt                      # applied when training starts (the moments live in the training handle)
        return m

    # ---- reference-shaped sampling API (model/model.py:613-688) ------------------------------------
    def _sample_model(self, obs_len: int, dimensions) -> "DESIREModel":
        """The model sample() runs on: same weights, observation length = the trajectory's, frame size = `dimensions`.
        Cached per (obs_len, dimensions); refreshed when the optimiser has moved the weights since (train_step keeps them on
        the device: sync_weights pulls them back)."""
        key = (int(obs_len), None if dimensions is None else (float(dimensions[0]), float(dimensions[1])))
        cache = self.__dict__.setdefault("_sample_models", {})
        wts = self.sync_weights()
        if wts is None:
            self._handle(1, False)                       # first use: draws the initial weights
            wts = self._weights
        sub, ver = cache.get(key, (None, -1))
        if sub is None or ver != self._version:
            args = SimpleNamespace(**vars(self.args))
            args.seq_length = int(obs_len)
            args.pred_length = int(getattr(self.args, "pred_length", None) or self.args.seq_length)
            if key[1] is not None:
                args.img_width, args.img_height = key[1]
            w = dict(wts)
            tw = np.asarray(w["temporal/w"])
            if tw.shape[1] != obs_len:                   # O1's window is seq_length wide; sample() does not use it
                fit = np.zeros((1, obs_len, 2, 100), np.float32)
                n = min(obs_len, tw.shape[1])
                fit[:, :n] = tw[:, :n]
                w["temporal/w"] = fit
            if sub is None:
                sub = DESIREModel(args, w, self._seed)
            else:
                sub._weights = w
                for hd in sub._handles.values():
                    hd.set_weights(w)
            cache[key] = (sub, self._version)
        return sub

    def sample(self, sess, traj, grid, dimensions, true_traj, num=10, mode: Optional[str] = None, normals=None, seed: int = 0,
               device_rng: bool = False):
        """traj [obs, MNO, 3] observed frames; returns [obs+num, MNO, 3]: the observed frames followed by `num` predicted
        frames in pixel units, ids carried over from the last observed frame (model/model.py:680-688).  `sess` is ignored;
        `dimensions` = (width, height) of the frame in pixels (default: args.img_width / img_height).

        mode None (default): "rollout" -- the reference's own sample() semantics -- whenever the 5-wide head "gauss_head/w|b" it reads
        is TRAINED (args.head_loss_weight > 0 adds the reference's Gaussian NLL, model/model.py:494-550, to train_step's loss) or was
        supplied (weights= / a checkpoint that holds it); otherwise "ioc", the path the default loss trains, with a one-time warning
        that says so.  The mode is never inferred from `normals`: they belong to the rollout, and passing them to "ioc" is an error.

        mode "rollout" is the reference's loop (:623-688) on the device in one launch: warm-up over the observed
        frames, then per step the 5-wide Gaussian head "gauss_head/w|b" -> a draw (`normals` [num, MNO, 2] ~ N(0,1), or
        torch's generator seeded with `seed`, or with device_rng=True the library's own desire_rng_fill stream (seed, stream 0)) -> clip to <= 1.0 in normalised units (:666-669) -> fed back as the next input.
        Like the reference, objects with id 0 are stepped too and keep id 0.  `true_traj` only feeds the reference's cost
        print-outs (:649,684-685) and is unused.
        mode "ioc": the top-scored IOC-refined sample of the frozen-spec forward (prior path); `grid` may be a [Gh,Gw,C]
        scene feature grid; num <= pred_length."""
        torch = self.torch
        traj = np.asarray(traj, np.float64)
        sub = self._sample_model(traj.shape[0], dimensions)
        out = np.zeros((traj.shape[0] + num, traj.shape[1], 3))
        out[: traj.shape[0]] = traj
        m = traj.shape[1]
        out[traj.shape[0]:, :, 0] = traj[-1, :, 0]
        if mode is None:
            mode = "rollout" if getattr(self, "_head_given", False) else "ioc"
            if mode == "ioc" and not getattr(self, "_warned_default_mode", False):
                import warnings
                self._warned_default_mode = True
                warnings.warn("sample(): the reference's rollout reads the Gaussian output layer gauss_head/w|b, which this model has neither "
                              "been given nor trained (train with args.head_loss_weight > 0); the default therefore returns the top-scored "
                              "IOC-refined sample (mode='ioc').  Pass mode='rollout' to run the reference's loop on the untrained head.",
                              stacklevel=2)
        if normals is not None and mode != "rollout":
            raise ValueError("`normals` are the rollout's Gaussian draws: pass mode='rollout' with them (the mode is not inferred)")
        if mode == "rollout":
            if not getattr(self, "_head_given", False):
                import warnings
                warnings.warn("sample(mode='rollout') reads gauss_head/w|b, which train_step trains only with args.head_loss_weight > 0; this "
                              "model's head holds its random initial values (train it, pass weights= with a trained head, or use mode='ioc')",
                              stacklevel=2)
            h = sub._handle(1, False)
            d = h.dims
            past = sub._pad_windows([traj], d.mno)
            if device_rng:
                if normals is not None:
                    raise ValueError("device_rng fills the rollout's normals on the device: normals must be None")
                nrm = torch.empty((num, d.A, 2), device=self.device, dtype=torch.float32)
                h.rng_fill(seed, 0, 0, _lib.RNG_NORMAL, nrm.data_ptr(), nrm.numel(), torch.cuda.current_stream().cuda_stream)
            elif normals is None:
                g = torch.Generator(device=self.device).manual_seed(seed)
                nrm = torch.randn((num, d.A, 2), generator=g, device=self.device, dtype=torch.float32)
            else:
                nrm = torch.zeros((num, d.A, 2), device=self.device)
                nrm[:, :m] = torch.as_tensor(np.asarray(normals, np.float32), device=self.device)
            pos = torch.empty((num, d.A, 2), device=self.device)
            h.rollout(past.data_ptr(), nrm.data_ptr(), int(num), pos.data_ptr(), torch.cuda.current_stream().cuda_stream)
            p = pos.cpu().numpy()[:, :m]
            out[traj.shape[0]:, :, 1] = p[..., 0] / d.sx
            out[traj.shape[0]:, :, 2] = p[..., 1] / d.sy
            return out
        if mode != "ioc":
            raise ValueError("sample(mode=...): 'rollout' (the reference's loop) or 'ioc' (top-scored refined sample)")
        t_pred = int(getattr(self.args, "pred_length", None) or self.args.seq_length)
        if num > t_pred:
            raise ValueError("num=%d exceeds the model's pred_length=%d (the IOC regression head is sized by it)"
                             % (num, t_pred))
        if grid is not None and np.ndim(grid) == 3:
            sub.set_scene_grids(np.asarray(grid, np.float32)[None], [0])
        Y, score = sub.forward([traj], None, seed=seed, device_rng=device_rng)
        d = sub._handle(1, False).dims
        best = score[0].argmax(dim=0)                                        # [mno]
        idx = best.view(1, -1, 1, 1).expand(1, d.mno, d.T_pred, 2)
        top = torch.gather(Y[0], 0, idx)[0].cpu().numpy()[:, :num]           # [mno, num, 2]
        out[traj.shape[0]:, :, 1] = (top[:m, :, 0] / d.sx).T
        out[traj.shape[0]:, :, 2] = (top[:m, :, 1] / d.sy).T
        out[traj.shape[0]:][:, traj[-1, :, 0] == 0] = 0
        return out
