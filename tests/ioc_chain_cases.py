"""The cases of tests/test_gpu_ioc_chain_bits.py and of its digest generator tests/golden/make_ioc_chain_digests.py (plain helpers, no fixtures).

k_ioc's dense pooling chain (desire_amd/csrc/kernels_rnn.hip: ioc_bin_chain) runs once per (step, populated bin) and takes the next bin from the
tile's occupancy word; the weight fragments of a bin are requested before the next bin's operand is built.  One case per kind of instantiation of
the branch, each at T_pred = 5 (the operand double buffer and the fragment sets wrap across bins and steps) and K = 2 unless noted:

  full_plain   one window, 32 present agents, 4 x 4 bins, window 0.15: one full tile per (scene, k), every bin populated; dims.ioc_split = 1
  full_split   the same under the default dims.ioc_split: one window enters the bin-split regime (NSPL = 4)
  full_split2, full_split3   the same with dims.ioc_split = 2 / 3: the NSPL = 2 and NSPL = 3 instantiations
  sparse       three windows, 16 present agents each, window 0.02: a tile's populated bins are few and scattered, so the next bin comes from the
               occupancy word and not from b + 1, and a window without a close pair gives tiles with no populated bin at all
  sparse_split the same under the default dims.ioc_split
  sparse5      the same on 5 x 5 bins with two agents of window 0 walking half a pixel apart: tiles with EXACTLY ONE populated bin.  (A pair
               (i, j) populates the bin of j seen from i and its mirror image seen from j; only an odd grid has a bin that is its own mirror
               image, the centre one, so no input gives a 4 x 4 tile exactly one populated bin.)
  mno16        two groups per tile
  mno8_k3      mno = 8, K = 3: 24 rows, a partial tile
  grid6        6 x 6 = 36 bins: the occupancy word uses its upper half
  h64          H = 64: two waves per workgroup, the one-workgroup-per-CU launch bound, a chain of one pair of chunks
  h64_split, h64_pad   the bin-split and padded-tile forms at H = 64
  h256         H = 256: eight waves, a chain of four pairs of chunks (G = 32)
  wide         mno = 64: the 64-row tile (TM = 64)
  train_dense  training mode with dims.ioc_form = IOC_TRAIN_DENSE: the TRAIN instantiation of the dense chain on 32-row tiles
  train_wide, train_h256   training mode at mno = 64 and at H = 256: the TRAIN instantiations those shapes run by default
  train        CONTROL, runs none of the changed code: training mode under the default dims.ioc_form is the compact-pooling (CP) loop of k_ioc
  pad          DESIRE_FLAG_COMPACT_IOC, fold threshold 0, a window with 9 of 32 slots present: slot class 10, the PAD instantiation

run_case gives Y and score of one desire_forward, Y0 (the positions the IOC stage ran on) and, in training mode, the saved hidden states "ioc_sv_h"
[R, T_pred, H] -- the TRAIN instantiations' own output."""
import hashlib

import numpy as np

from desire_amd.spec import FLAG_COMPACT_IOC, IOC_TRAIN_DENSE, init_weights
from tests.helpers import make_case, small_dims

_ONE = dict(n_scenes=1, mno=32, K=2, T_obs=4, T_pred=5, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, ioc_split=1)
_SPARSE = dict(_ONE, n_scenes=3, nb_w=0.02, nb_h=0.02)
# id -> (small_dims keywords, absent slots per window, training mode, fold threshold of the slot classes or None)
CASES = {
    "full_plain": (dict(_ONE), 0, False, None),
    "full_split": (dict(_ONE, ioc_split=0), 0, False, None),
    "sparse": (dict(_SPARSE), 16, False, None),
    "sparse_split": (dict(_SPARSE, ioc_split=0), 16, False, None),
    "sparse5": (dict(_SPARSE, grid_size=5), 16, False, None),
    "mno16": (dict(_ONE, mno=16, n_scenes=2), 2, False, None),
    "mno8_k3": (dict(_ONE, mno=8, K=3), 1, False, None),
    "grid6": (dict(_ONE, grid_size=6, nb_w=0.3, nb_h=0.3), 0, False, None),
    "h64": (dict(_ONE, H=64), 3, False, None),
    "wide": (dict(_ONE, mno=64), 5, False, None),
    "train": (dict(_ONE, n_scenes=2), 3, True, None),
    "train_dense": (dict(_ONE, n_scenes=2, ioc_form=IOC_TRAIN_DENSE), 3, True, None),
    "full_split2": (dict(_ONE, ioc_split=2), 0, False, None),
    "full_split3": (dict(_ONE, ioc_split=3), 0, False, None),
    "h64_split": (dict(_ONE, H=64, ioc_split=0), 3, False, None),
    "h64_pad": (dict(_ONE, H=64, flags=FLAG_COMPACT_IOC), 23, False, 0),
    "h256": (dict(_ONE, H=256), 3, False, None),
    "train_wide": (dict(_ONE, mno=64), 5, True, None),
    "train_h256": (dict(_ONE, H=256), 3, True, None),
    "pad": (dict(_ONE, flags=FLAG_COMPACT_IOC), 23, False, 0),
}
SEEDS = {"sparse": 311, "sparse_split": 311, "sparse5": 311}          # (chosen on the CPU for the occupancies named above; every other case: 300)


def dims(cid):
    return small_dims(**CASES[cid][0])


def inputs(cid):
    past, fut, eps, grids, gos = make_case(dims(cid), seed=SEEDS.get(cid, 300), n_absent=CASES[cid][1])
    if cid == "sparse5":                                              # slot 1 of window 0 walks half a pixel beside slot 0
        for a in (past, fut):
            a[0, :, 1, 1:] = a[0, :, 0, 1:] + 0.5
    return past, fut, eps, grids, gos


def run_case(torch, cid):
    """(Y [R, T, 2], score [R], Y0 [R, T, 2], sv_h [R, T, H] or None outside training mode) of one forward of case `cid` on the GPU."""
    from desire_amd import _lib
    d = dims(cid)
    _, _, training, min_rows = CASES[cid]
    past, fut, eps, grids, gos = inputs(cid)
    h = _lib.Handle(d)
    h.set_weights(init_weights(d, 7))
    if training:
        h.set_training(True)
    if min_rows is not None:
        h.set_option("compact_min_rows", min_rows)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    past_t, fut_t, eps_t, grids_t = t(past), t(fut), t(eps), t(grids)
    h.set_scene_grids(grids_t.data_ptr(), gos)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda")
    score = torch.zeros((d.R,), device="cuda")
    h.forward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr(), Y.data_ptr(), score.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    Y0 = h.read_buffer("Y0", (d.R, d.T_pred, 2))
    sv_h = h.read_buffer("ioc_sv_h", (d.R, d.T_pred, d.H)) if training else None      # (one pass: the saves of pass 0 lead the buffer)
    h.close()
    return Y.cpu().numpy(), score.cpu().numpy(), Y0, sv_h


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def occupied(cid, Y0):
    """bool [groups, T_pred, B]: bin b holds a neighbour of some row of the (scene, k) group at that step, when the IOC stage of case `cid` runs on
    the positions Y0 -- the union of the group's rows' bins, i.e. the tile's occupancy word where a group is a tile (mno = 32)."""
    from oracle import desire_oracle as O
    d = dims(cid)
    past = inputs(cid)[0]
    valid = (past[:, d.T_obs - 1, :, 0] != 0)                                        # [n_scenes, mno]
    pos = Y0.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).transpose(0, 1, 3, 2, 4)   # [scene, k, t, slot, 2]
    v = np.broadcast_to(valid[:, None, None, :], pos.shape[:-1])
    bins = O.neighbor_bins(pos, v, d.nb_w, d.nb_h, d.grid_size)                      # [scene, k, t, centre, other]: absent OTHERS are dropped, as in the kernel
    occ = np.stack([(bins == b).any(axis=(-1, -2)) for b in range(d.B)], -1)
    return occ.reshape(d.n_scenes * d.K, d.T_pred, d.B)


def occupancy(cid, Y0):
    """Populated bins per (group, step): an int array [groups, T_pred]."""
    return occupied(cid, Y0).sum(-1)
