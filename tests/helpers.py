"""Shared synthetic-input builders for the parity tests (seeded, deterministic)."""
import numpy as np

from desire_amd.spec import Dims, init_weights  # noqa: F401


from desire_amd.synth import make_case  # noqa: F401,E402


def to_oracle_layout(win):
    """[n_scenes, T, mno, 3] -> [T, A, 3] (agent a = scene*mno + slot)."""
    n, T, m, _ = win.shape
    return np.ascontiguousarray(win.transpose(1, 0, 2, 3).reshape(T, n * m, 3))


def hinted_units(worst, hint, mul):
    """Mirror of dyn_units (desire_amd/csrc/dyn_count.h) for a launch that carries a device-side count: the units (agents / samples) a strided launch
    is sized for -- the hinted count with a quarter of slack plus 256, never above the worst case; no hint (<= 0) = the worst case.
    tests/test_dyn_count.py holds it equal to the header over a sweep."""
    if hint <= 0:
        return worst
    g = hint * mul
    return min(worst, g + g // 4 + 256)


def small_dims(**kw):
    base = dict(n_scenes=2, mno=32, K=4, T_obs=8, T_pred=12, H=128, L=128, n_grids=2,
                nb_w=0.25, nb_h=0.3, sx=1.0 / 1400.0, sy=1.0 / 1100.0)
    base.update(kw)
    return Dims(**base)


MISALIGNED_SHAPES = [(3, 1, 3, 7),      # (n_scenes, mno, K, T_pred): odd row length, segments of one row
                     (2, 8, 3, 7)]      # the whole-window segment
MISALIGNED_LONG = (2, 32, 2, 200)       # slot chunks of the error kernel, one segment per sample; the joint unit unchunked


def at_byte_offset(t, off):
    """The values of the float32 device tensor `t` at `off` (8 or 4) bytes past a torch allocation: a view into a flat buffer off / 4 floats larger.
    The evaluation kernels' 16-byte loads need a 16-byte aligned buffer (desire_kde_nll's 8-byte loads an 8-byte aligned one): this is their fallback."""
    import torch
    flat = torch.zeros(t.numel() + off // 4, device=t.device, dtype=torch.float32)
    v = flat[off // 4:].view(t.shape)
    v.copy_(t)
    assert flat.data_ptr() % 16 == 0 and v.data_ptr() % 16 == off and v.is_contiguous()
    return v


# the command line of the small model the evaluation tests share (8 slots, 5 samples, 6 target frames), the keys of the evaluation's result
# without an optional report, and the video they walk
EVAL_FLAGS = ["--batch_size", "2", "--seq_length", "4", "--pred_length", "6", "--max_num_obj", "8", "--d_dim", "64", "--latent_size", "64",
              "--num_samples", "5", "--neighborhood_size", "256", "--max_windows", "4", "--device_rng", "--seed", "3", "--checkpoint", "none.npz",
              "--units", "norm"]
PLAIN_KEYS = ["checkpoint", "generator", "units", "seed", "K", "top", "horizons", "windows", "agents", "top1", "best_of_top", "best_of_K", "mean_of_K"]


def walking_video():
    t = np.arange(60, dtype=np.float32)
    video = np.zeros((60, 8, 3), np.float32)                          # five objects walking straight lines, the last one leaves half way
    for i in range(5):
        video[:, i, 0] = i + 1
        video[:, i, 1] = 200 + 150 * i + 3 * t
        video[:, i, 2] = 150 + 100 * i + 2 * t
    video[30:, 4] = 0
    return video


# ---- what the GPU tests of the two mode fits (test_gpu_modes.py, test_gpu_scene_modes.py) compare with
def _t(torch, a):
    return None if a is None else torch.as_tensor(np.array(a, order="C"), device="cuda")      # (a copy: the shared inputs are read-only)


def _same_bits(a, b, keys, rows_a=slice(None), rows_b=slice(None)):
    """a[key][rows_a] and b[key][rows_b] are equal bit for bit; a NaN may differ in its payload only."""
    for key in keys:
        x, y = np.asarray(a[key])[rows_a], np.asarray(b[key])[rows_b]
        if x.dtype.kind == "f":
            x, y = x.astype(np.float32), y.astype(np.float32)
            nan = np.isnan(x)
            np.testing.assert_array_equal(nan, np.isnan(y), err_msg=key)
            np.testing.assert_array_equal(np.where(nan, 0, x).view(np.uint32), np.where(nan, 0, y).view(np.uint32), err_msg=key)
        else:
            np.testing.assert_array_equal(x, y, err_msg=key)


def _within(got, want, bound, key):
    """|got - want| <= bound wherever the float64 statement is finite, and a NaN exactly where it has one."""
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=key)
    gap = np.abs(got.astype(np.float64) - want)[fin]
    worst = float((gap / np.maximum(bound[fin], 1e-300)).max()) if gap.size else 0.0
    return (float(gap.max()) if gap.size else 0.0), worst


def _likelihood(got, f32, f64, tag):
    basis = float(np.abs(f32["frame"].astype(np.float64) - f64["frame"]).max())
    bar = max(4.0 * basis, 1e-5)
    err = float(np.abs(got["frame"].astype(np.float64) - f64["frame"]).max())
    print("%s: max |frame - f64| = %.3g, |f32 - f64| = %.3g, bar %.3g" % (tag, err, basis, bar))
    assert err <= bar
    np.testing.assert_allclose(got["out"], f64["out"], rtol=0, atol=bar)
