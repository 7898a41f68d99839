"""ctypes binding of libdesire_hip.so (include/desire_hip.h).  This is the ONLY compute path of
the package: if the library is missing or no gfx950 device is present, calls raise -- there is
no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Tuple

import numpy as np

from .spec import Dims

LIB_PATH = os.environ.get("DESIRE_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdesire_hip.so")

EXPORTS = [
    "desire_last_error", "desire_version", "desire_dims_size", "desire_build_hash", "desire_create", "desire_destroy", "desire_set_weight",
    "desire_finalize_weights", "desire_set_scene_grids", "desire_set_scene_images", "desire_encode", "desire_sample",
    "desire_ioc_refine", "desire_forward", "desire_read_buffer", "desire_neighbor_bins",
    "desire_scene_cells", "desire_set_profiling", "desire_get_profile", "desire_scene_cnn", "desire_losses",
    "desire_temporal_conv", "desire_feature_pooling", "desire_build_windows", "desire_gaussian_sample", "desire_ade_fde",
    "desire_set_training", "desire_backward", "desire_get_grad", "desire_grad_buffer",
    "desire_train_loss", "desire_adam_step", "desire_get_weight", "desire_clip_grads",
    "desire_device_buffer", "desire_ioc_step", "desire_ioc_finish", "desire_get_bin_table",
    "desire_graph_begin", "desire_graph_end", "desire_graph_launch", "desire_rollout", "desire_build_windows_la", "desire_adam_state",
    "desire_set_option", "desire_train_loss_async", "desire_set_head_loss",
    "desire_peer_export", "desire_peer_open", "desire_ioc_peer_pass", "desire_peer_close", "desire_peer_region", "desire_peer_open_ptr", "desire_peer_status",
    "desire_rank_samples", "desire_ranked_errors", "desire_kde_nll", "desire_select_diverse", "desire_joint_metrics",
    "desire_set_rng", "desire_set_rng_origin", "desire_rng_state", "desire_rng_fill", "desire_rollout_samples",
    "desire_set_recon_loss", "desire_recon_weights", "desire_occupancy", "desire_plan_risk", "desire_fit_modes",
    "desire_select_worlds", "desire_fit_scene_modes", "desire_plan_risk_cond",
    "desire_set_recon_scope", "desire_recon_weights_scene",
    "desire_set_collision_loss", "desire_collision_loss",
    "desire_mask_distance", "desire_set_offroad_field", "desire_set_offroad_loss", "desire_offroad_loss",
    "desire_set_refined_loss",
]
OCC_AT, OCC_UNTIL = 0, 1                                            # desire_occupancy modes (DESIRE_OCC_*)
OCC_MODES = {"at": OCC_AT, "until": OCC_UNTIL}                      # their names on the Python surface (mode=, --occupancy_mode)
RNG_BITS, RNG_NORMAL, RNG_LATENT, RNG_ROLLOUT = 0, 1, 2, 3          # desire_rng_fill kinds (DESIRE_RNG_*)
DIST_FINAL, DIST_MEAN, DIST_MAX = 0, 1, 2                           # desire_select_diverse metrics (DESIRE_DIST_*)
WORLD_ALL, WORLD_MEAN = 0, 1                                        # desire_select_worlds reduces over the slots (DESIRE_WORLD_*)
RECON_MEAN, RECON_MIN, RECON_SOFTMIN = 0, 1, 2                      # desire_set_recon_loss / desire_recon_weights modes (DESIRE_RECON_*)
RECON_MODES = {"mean": RECON_MEAN, "min": RECON_MIN, "softmin": RECON_SOFTMIN}      # their names on the Python surface (args.recon_loss, --recon_loss)
RECON_SCOPE_AGENT, RECON_SCOPE_SCENE = 0, 1                         # desire_set_recon_scope: per agent, or per window over its K worlds (DESIRE_RECON_SCOPE_*)
RECON_SCOPES = {"agent": RECON_SCOPE_AGENT, "scene": RECON_SCOPE_SCENE}             # their names on the Python surface (args.recon_scope, --recon_scope)
MODES_MAX, MODES_MAX_ITERS = 16, 32                                 # desire_fit_modes: the most modes and passes (DESIRE_MODES_MAX, _MAX_ITERS)
KDE_LOG_FLOOR = -20.0                                               # desire_kde_nll: the clip of a frame's log-density (Trajectron++'s)


class DesireDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_scenes", "mno", "K", "T_obs", "T_pred", "H", "L", "S", "C", "Gh", "Gw", "n_grids",
                 "grid_size", "E_v", "iters", "posterior")] + \
               [(n, C.c_float) for n in ("nb_w", "nb_h", "sx", "sy")] + [(n, C.c_int32) for n in ("bin_mode", "bn_mode", "bf16", "ref_compat", "n_dec", "ioc_form", "ioc_split", "train_fp32_mask", "flags")]

    @classmethod
    def from_dims(cls, d: Dims) -> "DesireDims":
        return cls(d.n_scenes, d.mno, d.K, d.T_obs, d.T_pred, d.H, d.L, d.S, d.C, d.Gh, d.Gw, d.n_grids,
                   d.grid_size, d.E_v, d.iters, d.posterior, d.nb_w, d.nb_h, d.sx, d.sy, int(getattr(d, "bin_mode", 0)),
                   int(getattr(d, "bn_mode", 0)), int(getattr(d, "bf16", 0)), int(getattr(d, "ref_compat", 0)), int(getattr(d, "n_dec", 0)),
                   int(getattr(d, "ioc_form", 0)), int(getattr(d, "ioc_split", 0)), int(getattr(d, "train_fp32_mask", 0)), int(getattr(d, "flags", 0)))


class DesireError(RuntimeError):
    pass


_lib = None


def load() -> C.CDLL:
    """Load the shared library (building is __graft_entry__.build()'s job, never done here)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own HIP / HSA runtime libraries.  The process must end up with ONE runtime: importing torch first
    # makes the dynamic loader resolve this library's libamdhip64 / libhsa-runtime64 against what torch already mapped; the other
    # load order leaves two runtimes in the process and the second one to initialise sees no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise DesireError(
            "libdesire_hip.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'`; "
            "desire_amd has no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i32, f32p = C.c_void_p, C.c_int32, C.c_void_p
    lib.desire_last_error.restype = C.c_char_p
    lib.desire_build_hash.restype = C.c_char_p
    lib.desire_create.argtypes = [C.POINTER(DesireDims), C.POINTER(vp)]
    lib.desire_destroy.argtypes = [vp]
    lib.desire_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.desire_set_weight.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_size_t]
    lib.desire_finalize_weights.argtypes = [vp]
    lib.desire_set_scene_grids.argtypes = [vp, f32p, C.POINTER(C.c_int32)]
    lib.desire_set_scene_images.argtypes = [vp, f32p, i32, i32, C.POINTER(C.c_int32)]
    lib.desire_encode.argtypes = [vp, f32p, f32p, vp]
    lib.desire_sample.argtypes = [vp, f32p, f32p, vp]
    lib.desire_ioc_refine.argtypes = [vp, f32p, f32p, vp]
    lib.desire_forward.argtypes = [vp, f32p, f32p, f32p, f32p, f32p, vp]
    lib.desire_read_buffer.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_size_t, vp]
    lib.desire_neighbor_bins.argtypes = [vp, f32p, vp, vp, i32, vp]
    lib.desire_scene_cells.argtypes = [vp, f32p, vp, i32, vp]
    lib.desire_scene_cnn.argtypes = [vp, f32p, i32, i32, f32p, vp]
    lib.desire_losses.argtypes = [vp, f32p, f32p, f32p, f32p, f32p, vp]
    lib.desire_temporal_conv.argtypes = [vp, f32p, f32p, vp]
    lib.desire_feature_pooling.argtypes = [vp, f32p, f32p, f32p, vp]
    lib.desire_build_windows.argtypes = [vp, f32p, i32, i32, C.POINTER(C.c_int32), i32, f32p, f32p, vp]
    lib.desire_build_windows_la.argtypes = [vp, f32p, i32, i32, C.POINTER(C.c_int32), i32, i32, f32p, f32p, vp]
    lib.desire_gaussian_sample.argtypes = [vp, f32p, f32p, f32p, i32, vp]
    lib.desire_ade_fde.argtypes = [vp, f32p, f32p, f32p, vp]
    lib.desire_rank_samples.argtypes = [vp, f32p, f32p, i32, vp, f32p, f32p, vp]
    lib.desire_ranked_errors.argtypes = [vp, f32p, f32p, vp, i32, C.POINTER(C.c_int32), i32, C.c_float, C.c_float, f32p, vp]
    lib.desire_kde_nll.argtypes = [vp, f32p, f32p, f32p, C.POINTER(C.c_int32), i32, C.c_float, C.c_float, C.c_float, f32p, f32p, vp]
    lib.desire_select_diverse.argtypes = [vp, f32p, vp, f32p, i32, i32, C.c_float, C.c_float, C.c_float, i32, vp, vp, f32p, f32p, f32p, vp]
    lib.desire_joint_metrics.argtypes = [vp, f32p, f32p, vp, f32p, C.POINTER(C.c_int32), i32, i32, C.c_float, C.c_float, C.c_float, vp, vp, f32p, f32p,
                                         vp, f32p, vp]
    lib.desire_select_worlds.argtypes = [vp, f32p, vp, f32p, i32, i32, i32, C.c_float, C.c_float, C.c_float, vp, vp, f32p, vp, vp]
    lib.desire_occupancy.argtypes = [vp, f32p, f32p, vp, f32p, C.POINTER(C.c_int32), i32, i32, i32, i32, vp, vp, f32p, f32p, f32p, f32p, f32p, vp]
    lib.desire_plan_risk.argtypes = [vp, f32p, f32p, vp, f32p, f32p, vp, i32, C.POINTER(C.c_int32), i32, C.c_float, C.c_float, C.c_float, vp, f32p, f32p, f32p, vp]
    lib.desire_plan_risk_cond.argtypes = [vp, f32p, f32p, vp, f32p, f32p, vp, i32, C.POINTER(C.c_int32), i32, C.c_float, C.c_float, C.c_float, C.c_float, i32,
                                          vp, f32p, f32p, f32p, f32p, f32p, f32p, f32p, vp, vp]
    lib.desire_fit_modes.argtypes = [vp, f32p, vp, f32p, f32p, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int32), i32, C.c_float,
                                     vp, vp, f32p, f32p, f32p, vp, f32p, f32p, vp]
    lib.desire_fit_scene_modes.argtypes = [vp, f32p, vp, vp, f32p, f32p, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int32), i32,
                                           C.c_float, vp, vp, f32p, f32p, f32p, vp, f32p, f32p, vp]
    lib.desire_rollout.argtypes = [vp, f32p, f32p, i32, f32p, vp]
    lib.desire_rollout_samples.argtypes = [vp, f32p, f32p, f32p, vp]
    lib.desire_set_training.argtypes = [vp, C.c_int]
    lib.desire_backward.argtypes = [vp, f32p, f32p, f32p, vp]
    lib.desire_get_grad.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_size_t, vp]
    lib.desire_grad_buffer.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.desire_train_loss.argtypes = [vp, f32p, C.POINTER(C.c_float), vp]
    lib.desire_train_loss_async.argtypes = [vp, f32p, f32p, vp]
    lib.desire_set_head_loss.argtypes = [vp, C.c_float]
    lib.desire_set_recon_loss.argtypes = [vp, i32, C.c_float]
    lib.desire_recon_weights.argtypes = [vp, f32p, f32p, i32, C.c_float, f32p, f32p, vp, f32p, vp]
    lib.desire_set_recon_scope.argtypes = [vp, i32]
    lib.desire_recon_weights_scene.argtypes = [vp, f32p, f32p, i32, C.c_float, f32p, f32p, vp, f32p, vp, f32p, vp]
    lib.desire_set_collision_loss.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.desire_collision_loss.argtypes = [vp, f32p, f32p, C.c_float, C.c_float, C.c_float, f32p, vp, f32p, f32p, vp]
    lib.desire_mask_distance.argtypes = [vp, vp, i32, i32, i32, C.c_float, C.c_float, f32p, vp]
    lib.desire_set_offroad_field.argtypes = [vp, f32p, i32, i32, i32, C.POINTER(i32)]
    lib.desire_set_offroad_loss.argtypes = [vp, C.c_float, C.c_float]
    lib.desire_offroad_loss.argtypes = [vp, f32p, f32p, C.c_float, f32p, vp, f32p, f32p, vp]
    lib.desire_set_refined_loss.argtypes = [vp, i32, C.c_float, C.c_float]
    lib.desire_peer_export.argtypes = [vp, C.c_char_p, C.POINTER(C.c_size_t)]
    lib.desire_peer_open.argtypes = [vp, i32, i32, i32, C.c_char_p]
    lib.desire_ioc_peer_pass.argtypes = [vp, f32p, f32p, vp]
    lib.desire_peer_close.argtypes = [vp]
    lib.desire_peer_status.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.desire_peer_region.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.desire_peer_open_ptr.argtypes = [vp, i32, i32, i32, vp]
    lib.desire_adam_step.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float, vp]
    lib.desire_adam_state.argtypes = [vp, C.POINTER(C.c_int32), C.c_int]
    lib.desire_get_weight.argtypes = [vp, C.c_char_p, C.POINTER(C.c_float), C.c_size_t, vp]
    lib.desire_clip_grads.argtypes = [vp, C.c_float, C.POINTER(C.c_float), vp]
    lib.desire_get_bin_table.argtypes = [vp, C.POINTER(C.c_float)]
    lib.desire_graph_begin.argtypes = [vp, vp]
    lib.desire_graph_end.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    lib.desire_graph_launch.argtypes = [vp, i32, vp]
    lib.desire_device_buffer.argtypes = [vp, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.desire_ioc_step.argtypes = [vp, i32, i32, i32, f32p, f32p, vp, f32p, f32p, f32p, vp]
    lib.desire_ioc_finish.argtypes = [vp, f32p, f32p, f32p, f32p, vp]
    lib.desire_set_rng.argtypes = [vp, C.c_uint64, C.c_uint32, vp]
    lib.desire_set_rng_origin.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.desire_rng_state.argtypes = [vp, C.POINTER(C.c_uint32), vp]
    lib.desire_rng_fill.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, i32, vp, C.c_size_t, vp]
    lib.desire_set_profiling.argtypes = [vp, C.c_int]
    lib.desire_get_profile.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.POINTER(C.c_int32)]
    for n in EXPORTS:
        if n not in ("desire_last_error", "desire_build_hash"):
            getattr(lib, n).restype = C.c_int
    if lib.desire_dims_size() != C.sizeof(DesireDims):          # this binding and the library disagree about desire_dims: refuse to run
        raise DesireError("libdesire_hip.so was built with sizeof(desire_dims) = %d, this binding has %d: rebuild (python -c 'import "
                          "__graft_entry__ as g; g.build()')" % (lib.desire_dims_size(), C.sizeof(DesireDims)))
    _lib = lib
    return lib


def _chk(rc: int) -> None:
    if rc != 0:
        raise DesireError("libdesire_hip error %d: %s" % (rc, load().desire_last_error().decode()))


def _horizons(horizons, optional: bool = False):
    """(the horizons as a flat int32 array, its const int32_t* for a call); with optional, None gives an empty array and a NULL pointer."""
    if optional and horizons is None:
        return np.zeros(0, np.int32), None
    hz = np.ascontiguousarray(horizons, dtype=np.int32).reshape(-1)
    return hz, hz.ctypes.data_as(C.POINTER(C.c_int32))


class Handle:
    """Thin owner of one desire_handle*.  All device pointers are raw integers (torch .data_ptr())."""

    def __init__(self, dims: Dims):
        dims.validate()
        self.dims = dims
        self.lib = load()
        self._h = C.c_void_p()
        cd = DesireDims.from_dims(dims)
        _chk(self.lib.desire_create(C.byref(cd), C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.desire_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int) -> None:
        """One of the behavioural switches of desire_dims ("ioc_form", "ioc_split", "train_fp32_mask", "flags") or a handle option
        ("compact_min_rows", "compact_host_counts", "scene_grad", "scene_modes_chunk") on the live handle."""
        _chk(self.lib.desire_set_option(self._h, name.encode(), int(value)))
        if hasattr(self.dims, name):                      # ("compact_min_rows" is a handle option, not a desire_dims field)
            self.dims = self.dims.replace(**{name: int(value)})

    def set_weights(self, weights: Dict[str, np.ndarray]) -> None:
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            _chk(self.lib.desire_set_weight(self._h, name.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.size))
        _chk(self.lib.desire_finalize_weights(self._h))

    def set_scene_grids(self, dev_grids_ptr: int, grid_of_scene) -> None:
        g = np.ascontiguousarray(grid_of_scene, dtype=np.int32)
        if g.size != self.dims.n_scenes:
            raise DesireError("grid_of_scene must have n_scenes entries")
        _chk(self.lib.desire_set_scene_grids(self._h, dev_grids_ptr, g.ctypes.data_as(C.POINTER(C.c_int32))))

    def set_scene_images(self, dev_images_ptr: int, Hi: int, Wi: int, grid_of_scene) -> None:
        """Scene images [n_grids, Hi = 4 Gh, Wi = 4 Gw, 3] on the device: the handle runs (and in training, trains) the scene CNN itself."""
        g = np.ascontiguousarray(grid_of_scene, dtype=np.int32)
        if g.size != self.dims.n_scenes:
            raise DesireError("grid_of_scene must have n_scenes entries")
        _chk(self.lib.desire_set_scene_images(self._h, dev_images_ptr, int(Hi), int(Wi), g.ctypes.data_as(C.POINTER(C.c_int32))))

    def encode(self, past_ptr: int, fut_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_encode(self._h, past_ptr, fut_ptr or None, stream or None))

    def sample(self, eps_ptr: int, yhat_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_sample(self._h, eps_ptr, yhat_ptr, stream or None))

    def set_rng(self, seed: int, draw: int = 0, stream: int = 0) -> None:
        """Switches the device generator on (or re-seeds it): afterwards eps_ptr = 0 is legal in sample / forward / backward, one draw per call."""
        _chk(self.lib.desire_set_rng(self._h, int(seed) & (2 ** 64 - 1), int(draw) & 0xFFFFFFFF, stream or None))

    def set_rng_origin(self, scene_base: int = 0, slot_base: int = 0) -> None:
        """Global index of the call's first window and of the handle's first slot (host values: baked into a captured graph)."""
        _chk(self.lib.desire_set_rng_origin(self._h, int(scene_base) & 0xFFFFFFFF, int(slot_base) & 0xFFFFFFFF))

    def rng_state(self, stream: int = 0) -> Tuple[int, int]:
        """(next, used) draw counters; synchronises the stream."""
        out = (C.c_uint32 * 2)()
        _chk(self.lib.desire_rng_state(self._h, out, stream or None))
        return int(out[0]), int(out[1])

    def rng_fill(self, seed: int, stream_id: int, first: int, kind: int, out_ptr: int, n: int, stream: int = 0) -> None:
        """n elements of the fill stream (seed, stream_id) from element `first`: RNG_BITS (uint32) or RNG_NORMAL (fp32); RNG_LATENT writes the eps
        [n_scenes, K, mno, L] of draw `stream_id` at the handle's origin (first = 0, n = R * L), RNG_ROLLOUT the normals [n_scenes, K, mno, T_pred, 2]
        of a generating rollout_samples (first = 0, n = R * T_pred * 2)."""
        _chk(self.lib.desire_rng_fill(self._h, int(seed) & (2 ** 64 - 1), int(stream_id) & 0xFFFFFFFF, int(first), int(kind), out_ptr, int(n), stream or None))

    def ioc_refine(self, yhat_ptr: int, score_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_ioc_refine(self._h, yhat_ptr, score_ptr, stream or None))

    def forward(self, past_ptr: int, fut_ptr: int, eps_ptr: int, yhat_ptr: int, score_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_forward(self._h, past_ptr, fut_ptr or None, eps_ptr, yhat_ptr, score_ptr or None, stream or None))

    def read_buffer(self, name: str, shape: Tuple[int, ...], stream: int = 0) -> np.ndarray:
        out = np.empty(shape, np.float32)
        _chk(self.lib.desire_read_buffer(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size,
                                         stream or None))
        return out

    def neighbor_bins(self, pos_ptr: int, valid_ptr: int, bins_ptr: int, n_groups: int, stream: int = 0) -> None:
        _chk(self.lib.desire_neighbor_bins(self._h, pos_ptr, valid_ptr, bins_ptr, n_groups, stream or None))

    def scene_cells(self, pos_ptr: int, cells_ptr: int, n: int, stream: int = 0) -> None:
        _chk(self.lib.desire_scene_cells(self._h, pos_ptr, cells_ptr, n, stream or None))

    def scene_cnn(self, image_ptr: int, Hi: int, Wi: int, grids_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_scene_cnn(self._h, image_ptr, Hi, Wi, grids_ptr, stream or None))

    def losses(self, fut_ptr: int, yhat_ptr: int, kld_ptr: int, recon_ptr: int, cost_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_losses(self._h, fut_ptr, yhat_ptr, kld_ptr, recon_ptr, cost_ptr, stream or None))

    def temporal_conv(self, past_ptr: int, rho_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_temporal_conv(self._h, past_ptr, rho_ptr, stream or None))

    def feature_pooling(self, yhat_ptr: int, rho_ptr: int, out_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_feature_pooling(self._h, yhat_ptr, rho_ptr, out_ptr, stream or None))

    def build_windows(self, frames_ptr: int, n_frames: int, mno_in: int, starts, past_ptr: int, fut_ptr: int, stream: int = 0,
                      lookahead: int = 0) -> None:
        st = np.ascontiguousarray(starts, dtype=np.int32)
        _chk(self.lib.desire_build_windows_la(self._h, frames_ptr, n_frames, mno_in, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                            st.size, int(lookahead), past_ptr, fut_ptr, stream or None))

    def gaussian_sample(self, params_ptr: int, normals_ptr: int, out_ptr: int, n: int, stream: int = 0) -> None:
        _chk(self.lib.desire_gaussian_sample(self._h, params_ptr, normals_ptr, out_ptr, n, stream or None))

    def rollout(self, past_ptr: int, normals_ptr: int, num: int, out_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_rollout(self._h, past_ptr, normals_ptr, num, out_ptr, stream or None))

    def rollout_samples(self, past_ptr: int, normals_ptr: int, yhat_ptr: int, stream: int = 0) -> None:
        """K head rollouts per agent in the sample layout: yhat [R, T_pred, 2], normals [R, T_pred, 2] or 0 (after set_rng: drawn in the kernel,
        one draw per call)."""
        _chk(self.lib.desire_rollout_samples(self._h, past_ptr or None, normals_ptr or None, yhat_ptr or None, stream or None))

    def ade_fde(self, yhat_ptr: int, fut_ptr: int, out_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_ade_fde(self._h, yhat_ptr, fut_ptr, out_ptr, stream or None))

    def rank_samples(self, score_ptr: int, yhat_ptr: int, n_top: int, order_ptr: int, top_y_ptr: int = 0, top_score_ptr: int = 0,
                     stream: int = 0) -> None:
        """order [A, K] int32 = every agent's samples by descending score (ties to the lower k, NaN last); optionally the n_top best rows of
        Y -> top_y [A, n_top, T_pred, 2] and their scores -> top_score [A, n_top]."""
        _chk(self.lib.desire_rank_samples(self._h, score_ptr, yhat_ptr or None, int(n_top), order_ptr, top_y_ptr or None, top_score_ptr or None,
                                          stream or None))

    def ranked_errors(self, yhat_ptr: int, fut_ptr: int, order_ptr: int, n_top: int, horizons, unit_x: float, unit_y: float, out_ptr: int,
                      stream: int = 0) -> None:
        """out [A, len(horizons), 4] = (ADE_h, FDE_h of the best-scored sample, best ADE_h, FDE_h among the n_top best-scored); errors are
        scaled by (unit_x, unit_y) per axis: (1, 1) normalised units, (1/sx, 1/sy) pixels."""
        hz, hzp = _horizons(horizons)
        _chk(self.lib.desire_ranked_errors(self._h, yhat_ptr, fut_ptr, order_ptr, int(n_top), hzp, hz.size,
                                           C.c_float(unit_x), C.c_float(unit_y), out_ptr, stream or None))

    def kde_nll(self, yhat_ptr: int, fut_ptr: int, score_ptr: int, horizons, unit_x: float, unit_y: float, log_floor: float, out_ptr: int,
                frame_ptr: int = 0, stream: int = 0) -> None:
        """out [A, len(horizons), 2] = (mean, final) negative log-density of the ground truth under a Gaussian KDE of the agent's K samples, per
        frame, clipped below at log_floor, over the counted frames before each horizon; score_ptr = 0: equal weights, else softmax(score).  The
        density is per unit^2 of (unit_x, unit_y), as in ranked_errors.  frame [A, T_pred] (optional): the per-frame log-densities."""
        hz, hzp = _horizons(horizons)
        _chk(self.lib.desire_kde_nll(self._h, yhat_ptr or None, fut_ptr or None, score_ptr or None, hzp, hz.size,
                                     C.c_float(unit_x), C.c_float(unit_y), C.c_float(log_floor), out_ptr or None, frame_ptr or None, stream or None))

    def select_diverse(self, yhat_ptr: int, order_ptr: int, score_ptr: int, metric: int, t_end: int, radius: float, unit_x: float, unit_y: float,
                       n_top: int, order_out_ptr: int, count_ptr: int, mass_ptr: int = 0, top_y_ptr: int = 0, top_score_ptr: int = 0,
                       stream: int = 0) -> None:
        """Score-ordered non-maximum suppression: walking order [A, K] (rank_samples') best first, a sample is kept unless it lies within
        `radius` (metric DIST_FINAL / DIST_MEAN / DIST_MAX over the frames t < t_end, distances scaled by (unit_x, unit_y) as in ranked_errors) of
        one already kept.  order_out [A, K] int32 = the kept samples, then the suppressed ones; count [A] int32 = the number kept; optionally
        mass [A, K] = the softmax(score) weight each kept sample absorbed (score_ptr = 0: equal weights) and the rows / scores of the first
        n_top entries -> top_y [A, n_top, T_pred, 2], top_score [A, n_top]."""
        _chk(self.lib.desire_select_diverse(self._h, yhat_ptr or None, order_ptr or None, score_ptr or None, int(metric), int(t_end), C.c_float(radius),
                                            C.c_float(unit_x), C.c_float(unit_y), int(n_top), order_out_ptr or None, count_ptr or None,
                                            mass_ptr or None, top_y_ptr or None, top_score_ptr or None, stream or None))

    def joint_metrics(self, yhat_ptr: int, fut_ptr: int, present_ptr: int, score_ptr: int, horizons, n_top: int, radius: float, unit_x: float,
                      unit_y: float, cnt_ptr: int, jorder_ptr: int, first_ptr: int = 0, jerr_ptr: int = 0, jscore_ptr: int = 0, out_ptr: int = 0,
                      stream: int = 0) -> None:
        """The K samples of a window as K joint futures: first [n, K + 1, mno] int32 = the first frame at which a slot comes within `radius` of
        another slot of its (window, k) (T_pred: never; row K: the ground truth), cnt [n, K + 1, n_h, 2] int32 = (slots touching, slots taking
        part) before each horizon, jerr [n, K, n_h, 2] = (JADE_h, JFDE_h), jscore [n, K] = the summed score, jorder [n, K] int32 = its order
        (rank_samples' rule), out [n, n_h, 4] = (JADE, JFDE of the best-scored joint sample, best JADE, best JFDE among the n_top best-scored).
        Exactly one of fut_ptr (evaluation) and present_ptr ([A] uint8, prediction time: no jerr / out); distances are scaled by (unit_x, unit_y)
        as in ranked_errors."""
        hz, hzp = _horizons(horizons)
        _chk(self.lib.desire_joint_metrics(self._h, yhat_ptr or None, fut_ptr or None, present_ptr or None, score_ptr or None,
                                           hzp, hz.size, int(n_top), C.c_float(radius), C.c_float(unit_x),
                                           C.c_float(unit_y), first_ptr or None, cnt_ptr or None, jerr_ptr or None, jscore_ptr or None,
                                           jorder_ptr or None, out_ptr or None, stream or None))

    def select_worlds(self, yhat_ptr: int, present_ptr: int, wscore_ptr: int, metric: int, reduce: int, t_end: int, radius: float, unit_x: float,
                      unit_y: float, worder_ptr: int, wcount_ptr: int, wmass_ptr: int = 0, wlabel_ptr: int = 0, stream: int = 0) -> None:
        """Score-ordered non-maximum suppression of a window's K joint futures (world k = sample k of every slot): walking the worlds by
        descending wscore [n, K] (ranked by the call; wscore_ptr = 0: the identity order), a world is kept unless it is near one already kept --
        WORLD_ALL: every taking-part slot (present [A] uint8, present_ptr = 0: all) is within `radius` by `metric` (DIST_* over the frames
        t < t_end, as in select_diverse); WORLD_MEAN: the mean over those slots of the distance is below `radius`.  worder [n, K] int32 = the
        kept worlds, then the suppressed ones; wcount [n] int32 = the number kept; optionally wmass [n, K] = the softmax(wscore) weight each
        kept world absorbed and wlabel [n, K] int32 = for every world the keeping position of the world that owns it."""
        _chk(self.lib.desire_select_worlds(self._h, yhat_ptr or None, present_ptr or None, wscore_ptr or None, int(metric), int(reduce), int(t_end),
                                           C.c_float(radius), C.c_float(unit_x), C.c_float(unit_y), worder_ptr or None, wcount_ptr or None,
                                           wmass_ptr or None, wlabel_ptr or None, stream or None))

    def plan_risk(self, yhat_ptr: int, fut_ptr: int, present_ptr: int, score_ptr: int, plans_ptr: int, ego_ptr: int, M: int, horizons,
                  radius: float, unit_x: float, unit_y: float, risk_ptr: int, first_ptr: int = 0, clear_ptr: int = 0, blame_ptr: int = 0,
                  stream: int = 0) -> None:
        """M candidate ego plans per window (plans [n, M, T_pred, 2], normalised; ego [n, M] int32 = the slot a plan replaces, negative or
        ego_ptr = 0: none) against the K joint futures: risk [n, M, n_h] = the weight of the joint futures in which the plan comes within `radius`
        of a slot before each horizon (softmax of the joint scores; score_ptr = 0: equal weights), first [n, M, K + 1] int32 = the frame of that
        first contact (T_pred: never; row K: the ground truth), clear [n, M, K + 1, n_h] = the smallest SQUARED distance to any slot before each
        horizon (+inf: nobody counted), blame [n, M, n_h, mno] = the risk split by the slot touched.  Exactly one of fut_ptr (evaluation) and
        present_ptr ([A] uint8, prediction time); distances are scaled by (unit_x, unit_y) as in joint_metrics."""
        hz, hzp = _horizons(horizons)
        _chk(self.lib.desire_plan_risk(self._h, yhat_ptr or None, fut_ptr or None, present_ptr or None, score_ptr or None, plans_ptr or None,
                                       ego_ptr or None, int(M), hzp, hz.size, C.c_float(radius),
                                       C.c_float(unit_x), C.c_float(unit_y), first_ptr or None, clear_ptr or None, risk_ptr or None,
                                       blame_ptr or None, stream or None))

    def plan_risk_cond(self, yhat_ptr: int, fut_ptr: int, present_ptr: int, score_ptr: int, plans_ptr: int, ego_ptr: int, M: int, horizons,
                       radius: float, unit_x: float, unit_y: float, sigma: float, t_cond: int, risk_ptr: int, cw_ptr: int, first_ptr: int = 0,
                       clear_ptr: int = 0, blame_ptr: int = 0, dist_ptr: int = 0, ess_ptr: int = 0, support_ptr: int = 0, cond_ptr: int = 0,
                       stream: int = 0) -> None:
        """plan_risk given that the ego drives the plan: the K joint futures of a window are reweighted per plan by how well their own sample of
        the slot the plan replaces (ego) agrees with it -- a Gaussian kernel of bandwidth `sigma` (the unit of the radius: the RMS deviation per
        frame) on the mean squared distance over the counted frames t < t_cond -- times the prior weight.  cw [n, M, K] (required) = those
        weights, the prior's for a plan without an ego slot or a compared frame; risk, first, clear and blame as in plan_risk with cw in place of
        the prior; optionally dist [n, M, K] = the mean squared distances, ess [n, M] = the effective number of worlds 1 / sum cw^2, support
        [n, M] = the kernel density of the plan under the predicted ego in (0, 1], cond [n, M] int32 = the compared frames of a conditioned
        plan, 0 otherwise."""
        hz, hzp = _horizons(horizons)
        _chk(self.lib.desire_plan_risk_cond(self._h, yhat_ptr or None, fut_ptr or None, present_ptr or None, score_ptr or None, plans_ptr or None,
                                            ego_ptr or None, int(M), hzp, hz.size, C.c_float(radius), C.c_float(unit_x), C.c_float(unit_y),
                                            C.c_float(sigma), int(t_cond), first_ptr or None, clear_ptr or None, risk_ptr or None,
                                            blame_ptr or None, cw_ptr or None, dist_ptr or None, ess_ptr or None, support_ptr or None,
                                            cond_ptr or None, stream or None))

    def fit_modes(self, yhat_ptr: int, order_ptr: int, score_ptr: int, n_modes: int, t_end: int, iters: int, unit_x: float, unit_y: float,
                  var_floor: float, count_ptr: int, prob_ptr: int, label_ptr: int = 0, mean_ptr: int = 0, cov_ptr: int = 0, passes_ptr: int = 0,
                  fut_ptr: int = 0, horizons=None, log_floor: float = KDE_LOG_FLOOR, out_ptr: int = 0, frame_ptr: int = 0, stream: int = 0) -> None:
        """n_modes modes per agent fitted to its K weighted samples by a weighted Lloyd iteration seeded with the first n_modes entries of order
        [A, K] (rank_samples' or select_diverse's), at most `iters` passes, the assignment distance over the frames t < t_end scaled by
        (unit_x, unit_y): count [A, n_modes] int32 = the members of each mode, prob [A, n_modes] = their weight (softmax(score); score_ptr = 0:
        1 / K), label [A, K] int32, mean [A, n_modes, T_pred, 2] in Y's coordinates, cov [A, n_modes, T_pred, 3] = (Cxx, Cyy, Cxy) in unit^2 with
        var_floor added to the diagonal, passes [A] int32.  With fut_ptr (and horizons): out [A, n_h, 2] = (mean, final) negative log-density of
        the ground truth under that mixture, clipped below at log_floor, as kde_nll reports it; frame [A, T_pred] the per-frame log-densities."""
        hz, hzp = _horizons(horizons, optional=True)
        _chk(self.lib.desire_fit_modes(self._h, yhat_ptr or None, order_ptr or None, score_ptr or None, fut_ptr or None, int(n_modes), int(t_end),
                                       int(iters), C.c_float(unit_x), C.c_float(unit_y), C.c_float(var_floor), hzp, hz.size, C.c_float(log_floor),
                                       label_ptr or None, count_ptr or None, prob_ptr or None, mean_ptr or None, cov_ptr or None,
                                       passes_ptr or None, out_ptr or None, frame_ptr or None, stream or None))

    def fit_scene_modes(self, yhat_ptr: int, present_ptr: int, worder_ptr: int, wscore_ptr: int, n_modes: int, t_end: int, iters: int, unit_x: float,
                        unit_y: float, var_floor: float, count_ptr: int, prob_ptr: int, label_ptr: int = 0, mean_ptr: int = 0, cov_ptr: int = 0,
                        passes_ptr: int = 0, fut_ptr: int = 0, horizons=None, log_floor: float = KDE_LOG_FLOOR, out_ptr: int = 0, frame_ptr: int = 0,
                        stream: int = 0) -> None:
        """n_modes scene modes per window fitted to its K weighted joint futures (world k = sample k of every slot) by fit_modes' weighted Lloyd
        iteration on whole worlds, seeded with the first n_modes entries of worder [n, K] (joint_metrics' jorder or select_worlds' worder), at most
        `iters` passes; the distance of a world to a mode is the sum over the taking-part slots (present [A] uint8, present_ptr = 0: all) of
        fit_modes' distance over the frames t < t_end: count [n, n_modes] int32 = the member worlds of each mode, prob [n, n_modes] = their weight
        (softmax(wscore [n, K]); wscore_ptr = 0: 1 / K), label [n, K] int32, mean [n, n_modes, mno, T_pred, 2] in Y's coordinates, cov
        [n, n_modes, mno, T_pred, 3] = (Cxx, Cyy, Cxy) per agent in unit^2 with var_floor added to the diagonal (zeros for a slot that does not
        take part), passes [n] int32.  With fut_ptr (and horizons): out [n, n_h, 2] = (mean, final) negative joint log-density of the ground
        truth under that mixture PER AGENT counted in the frame, clipped below at log_floor; frame [n, T_pred] the per-frame values."""
        hz, hzp = _horizons(horizons, optional=True)
        _chk(self.lib.desire_fit_scene_modes(self._h, yhat_ptr or None, present_ptr or None, worder_ptr or None, wscore_ptr or None, fut_ptr or None,
                                             int(n_modes), int(t_end), int(iters), C.c_float(unit_x), C.c_float(unit_y), C.c_float(var_floor), hzp,
                                             hz.size, C.c_float(log_floor), label_ptr or None, count_ptr or None, prob_ptr or None, mean_ptr or None,
                                             cov_ptr or None, passes_ptr or None, out_ptr or None, frame_ptr or None, stream or None))

    def occupancy(self, yhat_ptr: int, fut_ptr: int, present_ptr: int, score_ptr: int, horizons, mode: int, Oh: int, Ow: int, occ_ptr: int,
                  exp_ptr: int = 0, hit_ptr: int = 0, viol_ptr: int = 0, off_ptr: int = 0, mask_ptr: int = 0, mask_of_scene_ptr: int = 0,
                  stream: int = 0) -> None:
        """Predicted occupancy maps of the K weighted samples on an Oh x Ow grid over the normalised frame: occ [n, n_h, Oh, Ow] = the probability
        that at least one agent is in the cell at frame h - 1 (OCC_AT) or at any counted frame before h (OCC_UNTIL), exp (same shape) = the
        expected number of agents; per agent [A, n_h]: off = the weight of its samples that are off frame, viol = the weight on cells whose byte
        of mask [n_masks, Oh, Ow] uint8 is 0 (mask_of_scene [n] int32 on the device, negative: none), hit = the weight on the ground truth's cell
        (fut_ptr and OCC_AT only).  Exactly one of fut_ptr (evaluation) and present_ptr ([A] uint8, prediction time); score_ptr = 0: equal
        weights, else softmax(score) as in kde_nll."""
        hz, hzp = _horizons(horizons)
        _chk(self.lib.desire_occupancy(self._h, yhat_ptr or None, fut_ptr or None, present_ptr or None, score_ptr or None,
                                       hzp, hz.size, int(mode), int(Oh), int(Ow), mask_ptr or None,
                                       mask_of_scene_ptr or None, occ_ptr or None, exp_ptr or None, hit_ptr or None, viol_ptr or None,
                                       off_ptr or None, stream or None))

    def set_training(self, on: bool) -> None:
        _chk(self.lib.desire_set_training(self._h, int(on)))

    def backward(self, past_ptr: int, fut_ptr: int, eps_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_backward(self._h, past_ptr, fut_ptr, eps_ptr, stream or None))

    def get_grad(self, name: str, shape: Tuple[int, ...], stream: int = 0) -> np.ndarray:
        out = np.empty(shape, np.float32)
        _chk(self.lib.desire_get_grad(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, stream or None))
        return out

    def grad_buffer(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_size_t()
        _chk(self.lib.desire_grad_buffer(self._h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def graph_begin(self, stream: int) -> None:
        _chk(self.lib.desire_graph_begin(self._h, stream))

    def graph_end(self, stream: int) -> int:
        gid = C.c_int32(-1)
        _chk(self.lib.desire_graph_end(self._h, stream, C.byref(gid)))
        return int(gid.value)

    def graph_launch(self, graph_id: int, stream: int) -> None:
        _chk(self.lib.desire_graph_launch(self._h, graph_id, stream))

    def bin_table(self) -> np.ndarray:
        out = np.zeros(20, np.float32)
        _chk(self.lib.desire_get_bin_table(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def device_tensor(self, name: str, dtype: str = "<f4"):
        """A workspace tensor of the handle ("HxHy", "p_last", "valid", "Y0", ...) as a flat zero-copy torch tensor."""
        import torch
        p, n = C.c_void_p(), C.c_size_t()
        _chk(self.lib.desire_device_buffer(self._h, name.encode(), C.byref(p), C.byref(n)))
        cnt = int(n.value) // (1 if dtype == "|u1" else 4)

        class _Dev:
            __cuda_array_interface__ = {"shape": (cnt,), "typestr": dtype, "data": (int(p.value), False), "version": 2}
        return torch.as_tensor(_Dev(), device="cuda")

    def scene_grid_grad(self):
        """d(loss)/d(grids) [n_grids, Gh, Gw, C] of the last backward as a zero-copy device tensor (training mode with
        set_option("scene_grad", 1); refused otherwise).  A caller that computes the grids with its own encoder backprops this into it."""
        d = self.dims
        return self.device_tensor("scene_grid_grad")[: d.n_grids * d.Gh * d.Gw * d.C].view(d.n_grids, d.Gh, d.Gw, d.C)

    def ioc_step(self, t: int, rank: int, nranks: int, Yall_ptr: int, plast_all_ptr: int, valid_all_ptr: int, Hall_ptr: int,
                 h_state_ptr: int, score_state_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_ioc_step(self._h, t, rank, nranks, Yall_ptr, plast_all_ptr, valid_all_ptr, Hall_ptr, h_state_ptr,
                                      score_state_ptr, stream or None))

    def ioc_finish(self, h_state_ptr: int, score_state_ptr: int, Y_ptr: int, score_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_ioc_finish(self._h, h_state_ptr, score_state_ptr, Y_ptr, score_ptr, stream or None))

    def grad_tensor(self):
        """The flat gradient buffer as a zero-copy torch tensor (for torch.distributed.all_reduce over RCCL)."""
        import torch
        p, n = self.grad_buffer()

        class _Dev:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (p, False), "version": 2}
        return torch.as_tensor(_Dev(), device="cuda")

    def clip_grads(self, max_norm: float, want_norm: bool = False, stream: int = 0):
        out = C.c_float(0.0)
        _chk(self.lib.desire_clip_grads(self._h, C.c_float(max_norm), C.byref(out) if want_norm else None, stream or None))
        return float(out.value) if want_norm else None

    def train_loss(self, fut_ptr: int, stream: int = 0) -> Dict[str, float]:
        out = (C.c_float * 5)()
        _chk(self.lib.desire_train_loss(self._h, fut_ptr, out, stream or None))                 # (synchronises the stream)
        return self.loss_terms(self.read_buffer("loss_out", (8,), stream))                      # + the Gaussian-head term and the clip norm

    def peer_export(self) -> bytes:
        """This rank's exchange region as a 64-byte hipIpcMemHandle (allocated on the first call)."""
        buf = C.create_string_buffer(64)
        n = C.c_size_t(0)
        _chk(self.lib.desire_peer_export(self._h, buf, C.byref(n)))
        return bytes(buf.raw)

    def peer_open(self, rank: int, nranks: int, peer: int, handle: bytes = None) -> None:
        _chk(self.lib.desire_peer_open(self._h, rank, nranks, peer, None if peer == rank else bytes(handle)))

    def peer_region(self) -> int:
        p, n = C.c_void_p(), C.c_size_t(0)
        _chk(self.lib.desire_peer_region(self._h, C.byref(p), C.byref(n)))
        return int(p.value)

    def peer_open_ptr(self, rank: int, nranks: int, peer: int, region_ptr: int = 0) -> None:
        _chk(self.lib.desire_peer_open_ptr(self._h, rank, nranks, peer, region_ptr or None))

    def ioc_peer_pass(self, y_ptr: int, score_ptr: int, stream: int = 0) -> None:
        _chk(self.lib.desire_ioc_peer_pass(self._h, y_ptr, score_ptr, stream or None))

    def peer_timed_out(self) -> bool:
        """After synchronising the stream a peer pass ran on: did one of its bounded waits give up (results unusable)?"""
        v = C.c_int32(0)
        _chk(self.lib.desire_peer_status(self._h, C.byref(v)))
        return bool(v.value)

    def peer_close(self) -> None:
        _chk(self.lib.desire_peer_close(self._h))

    def set_head_loss(self, weight: float) -> None:
        """Weight of the reference's Gaussian-NLL term for the 5-wide output layer (model/model.py:494-550) in the training loss."""
        _chk(self.lib.desire_set_head_loss(self._h, C.c_float(float(weight))))

    def set_recon_loss(self, mode: int, tau: float = 0.0) -> None:
        """The reconstruction term of the training loss over the K samples: RECON_MEAN (default, the paper's mean), RECON_MIN (best-of-many: only
        the sample with the smallest error carries the gradient) or RECON_SOFTMIN (a soft-min at temperature tau > 0, normalised units)."""
        _chk(self.lib.desire_set_recon_loss(self._h, int(mode), C.c_float(float(tau))))

    def recon_weights(self, fut_ptr: int, yhat_ptr: int, mode: int, tau: float = 0.0, e_ptr: int = 0, w_ptr: int = 0, winner_ptr: int = 0,
                      recon_ptr: int = 0, stream: int = 0) -> None:
        """Per-sample reconstruction errors e [A, K] of yhat [R, T_pred, 2] against fut, the weights w [A, K] the mode gives the K samples, the
        sample with the smallest error winner [A] int32 and the mode's term recon [A]; each output is optional (0: kept in the workspace tensor
        "recon_e" / "recon_w" / "recon_win" / "recon_val").  Masking as in losses()."""
        _chk(self.lib.desire_recon_weights(self._h, fut_ptr or None, yhat_ptr or None, int(mode), C.c_float(float(tau)), e_ptr or None, w_ptr or None,
                                           winner_ptr or None, recon_ptr or None, stream or None))

    def set_recon_scope(self, scope: int) -> None:
        """The scope of that term: RECON_SCOPE_AGENT (default: every agent weighs its own K samples) or RECON_SCOPE_SCENE (a window's K joint
        futures are weighed by their mean error over the window's counted agents: the best world, or a soft-min over the worlds, carries the
        gradient of every agent of the window).  Ignored in RECON_MEAN."""
        _chk(self.lib.desire_set_recon_scope(self._h, int(scope)))

    def recon_weights_scene(self, fut_ptr: int, yhat_ptr: int, mode: int, tau: float = 0.0, e_ptr: int = 0, E_ptr: int = 0, count_ptr: int = 0,
                            w_ptr: int = 0, winner_ptr: int = 0, recon_ptr: int = 0, stream: int = 0) -> None:
        """recon_weights in the scene scope: e [A, K] as there, the world errors E [n_scenes, K] (the mean of e over the window's counted agents),
        count [n_scenes] int32, and the window's weights w [A, K], winner [A] int32 and term recon [A] on every slot of the window; each output is
        optional (0: kept in the workspace tensor "recon_e" / "recon_E" / "recon_cnt" / "recon_w" / "recon_win" / "recon_val")."""
        _chk(self.lib.desire_recon_weights_scene(self._h, fut_ptr or None, yhat_ptr or None, int(mode), C.c_float(float(tau)), e_ptr or None,
                                                 E_ptr or None, count_ptr or None, w_ptr or None, winner_ptr or None, recon_ptr or None,
                                                 stream or None))

    def set_collision_loss(self, weight: float, radius: float = 0.0, unit_x: float = 1.0, unit_y: float = 1.0) -> None:
        """The collision term of the training loss: weight (default 0: off, the step as it was) times the squared hinge (1 - dist / radius)^2 of
        every pair of counted agents of one (window, k) and frame that are closer than radius, distances scaled by (unit_x, unit_y) as in
        joint_metrics; the mean over K and over the counted agents.  The step leaves the term in the workspace tensor "col_term", the touching
        (pair, frame)s per (window, k) in "col_touch"."""
        _chk(self.lib.desire_set_collision_loss(self._h, C.c_float(float(weight)), C.c_float(float(radius)), C.c_float(float(unit_x)),
                                                C.c_float(float(unit_y))))

    def collision_loss(self, fut_ptr: int, yhat_ptr: int, radius: float, unit_x: float = 1.0, unit_y: float = 1.0, col_ptr: int = 0,
                       touch_ptr: int = 0, dy_ptr: int = 0, term_ptr: int = 0, stream: int = 0) -> None:
        """The collision penalty of yhat [R, T_pred, 2] read as K joint futures per window: col [A, K] per agent and sample, touch [n_scenes, K]
        int32 (touching (pair, frame)s), dY [R, T_pred, 2] (the gradient of the term) and term [1]; each output is optional (0: kept in the
        workspace tensor "col_val" / "col_touch" / "col_grad" / "col_term").  Masking as in losses()."""
        _chk(self.lib.desire_collision_loss(self._h, fut_ptr or None, yhat_ptr or None, C.c_float(float(radius)), C.c_float(float(unit_x)),
                                            C.c_float(float(unit_y)), col_ptr or None, touch_ptr or None, dy_ptr or None, term_ptr or None,
                                            stream or None))

    def mask_distance(self, mask_ptr: int, n_masks: int, Mh: int, Mw: int, cell_x: float, cell_y: float, field_ptr: int, stream: int = 0) -> None:
        """The exact distance field [n_masks, Mh, Mw] fp32 of the traversability masks [n_masks, Mh, Mw] uint8 (0 = not traversable): per cell the
        distance from its centre to the nearest traversable centre, cells of (cell_x, cell_y); 0 on the road, 0 everywhere for a mask without road."""
        _chk(self.lib.desire_mask_distance(self._h, mask_ptr or None, int(n_masks), int(Mh), int(Mw), C.c_float(float(cell_x)),
                                           C.c_float(float(cell_y)), field_ptr or None, stream or None))

    def set_offroad_field(self, field_ptr: int, n_fields: int, Mh: int, Mw: int, field_of_scene) -> None:
        """Attach distance fields [n_fields, Mh, Mw] (referenced, not copied: keep the tensor alive) and the field of every window (a negative
        entry: the window has none)."""
        fos = np.ascontiguousarray(field_of_scene, dtype=np.int32)
        if fos.shape != (self.dims.n_scenes,):
            raise ValueError("field_of_scene must have n_scenes = %d entries, got shape %r" % (self.dims.n_scenes, fos.shape))
        _chk(self.lib.desire_set_offroad_field(self._h, field_ptr or None, int(n_fields), int(Mh), int(Mw), fos.ctypes.data_as(C.POINTER(C.c_int32))))

    def set_offroad_loss(self, weight: float, scale: float = 0.0) -> None:
        """The off-road term of the training loss: weight (default 0: off, the step as it was) times the squared distance (d / scale)^2 of every
        counted position of the K joint futures to the nearest traversable cell, read bilinearly off the attached field; the mean over K and over
        the counted agents.  The step leaves the term in the workspace tensor "off_term", the off-road (slot, frame)s per (window, k) in "off_count"."""
        _chk(self.lib.desire_set_offroad_loss(self._h, C.c_float(float(weight)), C.c_float(float(scale))))

    def offroad_loss(self, fut_ptr: int, yhat_ptr: int, scale: float, off_ptr: int = 0, count_ptr: int = 0, dy_ptr: int = 0, term_ptr: int = 0,
                     stream: int = 0) -> None:
        """The off-road penalty of yhat [R, T_pred, 2] read as K joint futures per window: off [A, K] per agent and sample, count [n_scenes, K]
        int32 (off-road (slot, frame)s), dY [R, T_pred, 2] (the gradient of the term) and term [1]; each output is optional (0: kept in the
        workspace tensor "off_val" / "off_count" / "off_grad" / "off_term").  Masking as in losses()."""
        _chk(self.lib.desire_offroad_loss(self._h, fut_ptr or None, yhat_ptr or None, C.c_float(float(scale)), off_ptr or None, count_ptr or None,
                                          dy_ptr or None, term_ptr or None, stream or None))

    def set_refined_loss(self, recon: int = 0, collision_weight: float = 0.0, offroad_weight: float = 0.0) -> None:
        """The recon mode, the collision term and the off-road term on the REFINED trajectories (default (0, 0, 0): the step as it was).  recon = 1:
        the IOC regression term follows set_recon_loss / set_recon_scope, with weights from the refined errors; the weights add weight * L_col(Y) and
        weight * L_off(Y) with the radius / units of set_collision_loss and the field / scale of the off-road setters (whose own weights may be 0).
        The step leaves the terms in the workspace tensors "rcol_term" / "roff_term", the counts in "rcol_touch" / "roff_count"."""
        _chk(self.lib.desire_set_refined_loss(self._h, int(recon), C.c_float(float(collision_weight)), C.c_float(float(offroad_weight))))

    def train_loss_async(self, fut_ptr: int, out8_ptr: int, stream: int = 0) -> None:
        """The loss terms of the last training-mode forward into a device buffer of 8 floats, no synchronisation (see loss_terms)."""
        _chk(self.lib.desire_train_loss_async(self._h, fut_ptr, out8_ptr, stream or None))

    @staticmethod
    def loss_terms(v8) -> Dict[str, float]:
        v8 = [float(x) for x in list(v8)[:8]]
        r = dict(zip(("recon", "kld", "ce", "reg", "n_present", "nll_head", "grad_norm", "n_head"), v8))
        r["loss"] = r["recon"] + r["kld"] + r["ce"] + r["reg"] + r["nll_head"]
        return r

    def adam_step(self, lr: float = 0.005, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, stream: int = 0) -> None:
        _chk(self.lib.desire_adam_step(self._h, C.c_float(lr), C.c_float(beta1), C.c_float(beta2), C.c_float(eps), stream or None))

    def opt_state(self) -> Dict[str, np.ndarray]:
        """Adam moments (flat, the gradient buffer's layout) and step counter of a training handle."""
        t = C.c_int32(0)
        _chk(self.lib.desire_adam_state(self._h, C.byref(t), 0))
        return {"m": self.device_tensor("Mflat").cpu().numpy(), "v": self.device_tensor("Vflat").cpu().numpy(),
                "t": np.array([t.value], np.int64)}

    def set_opt_state(self, st: Dict[str, np.ndarray]) -> None:
        import torch
        m, v = self.device_tensor("Mflat"), self.device_tensor("Vflat")
        if st["m"].size != m.numel() or st["v"].size != v.numel():
            raise DesireError("optimiser state of %d values does not fit this model (%d)" % (st["m"].size, m.numel()))
        m.copy_(torch.as_tensor(np.ascontiguousarray(st["m"], np.float32), device=m.device))
        v.copy_(torch.as_tensor(np.ascontiguousarray(st["v"], np.float32), device=v.device))
        t = C.c_int32(int(np.asarray(st["t"]).reshape(-1)[0]))
        _chk(self.lib.desire_adam_state(self._h, C.byref(t), 1))

    def get_weight(self, name: str, shape: Tuple[int, ...], stream: int = 0) -> np.ndarray:
        out = np.empty(shape, np.float32)
        _chk(self.lib.desire_get_weight(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, stream or None))
        return out

    def set_profiling(self, on: bool) -> None:
        _chk(self.lib.desire_set_profiling(self._h, int(on)))

    def get_profile(self) -> List[Tuple[str, float]]:
        n0 = C.c_int32(1 << 30)
        _chk(self.lib.desire_get_profile(self._h, None, None, C.byref(n0)))
        cap = max(int(n0.value), 1)
        ms = (C.c_float * cap)()
        names = (C.c_char_p * cap)()
        n = C.c_int32(cap)
        _chk(self.lib.desire_get_profile(self._h, ms, names, C.byref(n)))
        return [(names[i].decode(), float(ms[i])) for i in range(n.value)]
