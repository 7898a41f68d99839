"""numpy restatement of the rollout counter of desire_amd/csrc/philox.h (include/desire_hip.h states it) and of the layout that
desire_rng_fill(kind DESIRE_RNG_ROLLOUT) writes: the normals [n_scenes, K, mno, T_pred, 2] of a NULL-normals desire_rollout_samples.  Built on
tests/rng_reference.py (Philox4x32-10, the uniform map and Box-Muller in float64 on the same bits)."""
import numpy as np

from tests import rng_reference as R

ROLL = 2                                  # counter word c3 (latent eps: 0, fill op: 1)
MAX_T = 2048                              # steps the packing holds, on top of rng_reference.MAX_SLOT / MAX_K
MASK = R.MASK


def roll_counter(draw, window, k, slot, t):
    """The four counter words of step t (either step of the block) of rollout k of (global window, global slot) in draw `draw`."""
    draw, window, k, slot, t = np.broadcast_arrays(*(np.asarray(v, np.uint64) for v in (draw, window, k, slot, t)))
    c0 = (t >> np.uint64(1)) | (slot << np.uint64(10)) | (k << np.uint64(19))
    return np.stack([c0 & MASK, window & MASK, draw & MASK, np.full_like(c0, ROLL)], -1).astype(np.uint32)


def rollout_normals(seed, draw, n_scenes, K, mno, T_pred, scene_base=0, slot_base=0):
    """float64 [n_scenes, K, mno, T_pred, 2]: step t takes normals 2 (t & 1) (x) and 2 (t & 1) + 1 (y) of the block of t >> 1."""
    assert T_pred <= MAX_T and slot_base + mno <= R.MAX_SLOT and K < R.MAX_K
    nb = (T_pred + 1) // 2
    sc, k, sl, b = np.meshgrid(np.arange(n_scenes), np.arange(K), np.arange(mno), np.arange(nb), indexing="ij")
    c = roll_counter(draw, (scene_base + sc) & MASK, k, slot_base + sl, 2 * b)
    n4 = R.normals(R.philox4x32_10(c, R.seed_key(seed)))                  # [..., nb, 4] = (x, y) of step 2b, (x, y) of step 2b + 1
    return n4.reshape(n_scenes, K, mno, 2 * nb, 2)[:, :, :, :T_pred]
