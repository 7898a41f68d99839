"""The cases of tests/test_gpu_ioc_pool_rows.py and of its digest generator tests/golden/make_ioc_pool_digests.py (plain helpers, no fixtures).

k_ioc's dense pooling reads the operand row of a (row, bin) where it already lies (desire_amd/csrc/kernels_rnn.hip: pool_rows): the zero row when
the row has no neighbour in the bin, the neighbour's h row when it has one, and a SUM SLOT when it has two or more.  A tile-step (one tile of 32
or 64 rows at one prediction step) has spec.ioc_pool_slots(H, TM) slots; with more such pairs it runs the former build loop.  What decides the path
is therefore the number of (row, bin) pairs with two or more neighbours per tile-step, on the positions Y0 the IOC stage runs on -- multi_pairs()
counts it on the CPU.  Each case is T_pred = 5, K = 2, H = 128, 4 x 4 bins, every slot present unless noted; a window is crowded by pulling its
agents towards their centroid (`crowd`: one factor per window, 1 = as make_case drew them):

  single        two windows, window 0.03, spread out: every populated (row, bin) holds exactly one neighbour -- no sum slot is used
  bench         one window as bench.py draws them (window 0.15)
  crowd_fit     one window, crowded until some tile-step needs at least half the slots and none more than all of them
  crowd_over    three windows, from very crowded to as drawn: tile-steps above the slot count and tile-steps at or below it in one launch, and
                (the positions move) within the five steps of the middle window's tiles -- the build loop and the new loop alternate on one
                carried state
  one_cell      one window, the agents on a diagonal half a pixel apart: all inside ONE bin cell, the first agent sees the other 31 in one bin.
                Agent i has i agents in one bin and 31 - i in another: 60 pairs with two or more, exactly the slots of the 32-row tile at H = 128
                (no placement of 32 agents inside one cell gives fewer), so the tile-steps run the new loop with every slot taken
  crowd_over_mno16   crowd_over at mno = 16: two groups per tile
  crowd_over_mno64   crowd_over at mno = 64: the 64-row tile
  crowd_over_train_dense   crowd_over in training mode, dims.ioc_form = IOC_TRAIN_DENSE; also digests the saved hidden states
  crowd_over_pad     crowd_over with 10 of 32 slots present under DESIRE_FLAG_COMPACT_IOC, fold threshold 0: slot class 10, three groups per padded
                     tile (tile 0 = both samples of window 0 and the first of window 1)
"""
import hashlib

import numpy as np

from desire_amd.spec import FLAG_COMPACT_IOC, IOC_TRAIN_DENSE, init_weights, ioc_pool_slots
from tests.helpers import make_case, small_dims

_ONE = dict(n_scenes=1, mno=32, K=2, T_obs=4, T_pred=5, n_grids=1, grid_size=4, nb_w=0.15, nb_h=0.15, ioc_split=1)
_OVER = dict(_ONE, n_scenes=3)
# id -> (small_dims keywords, absent slots per window, training mode, fold threshold of the slot classes or None, crowd factor per window or "diagonal")
CASES = {
    "single": (dict(_ONE, n_scenes=2, nb_w=0.03, nb_h=0.03), 0, False, None, (1.0, 1.0)),
    "bench": (dict(_ONE), 0, False, None, (1.0,)),
    "crowd_fit": (dict(_ONE), 0, False, None, (0.75,)),
    "crowd_over": (dict(_OVER), 0, False, None, (0.1, 0.59, 1.0)),
    "one_cell": (dict(_ONE), 0, False, None, "diagonal"),
    "crowd_over_mno16": (dict(_OVER, mno=16), 0, False, None, (0.1, 0.61, 1.0)),
    "crowd_over_mno64": (dict(_OVER, mno=64), 0, False, None, (0.1, 1.09, 2.0)),
    "crowd_over_train_dense": (dict(_OVER, ioc_form=IOC_TRAIN_DENSE), 0, True, None, (0.1, 0.59, 1.0)),
    "crowd_over_pad": (dict(_OVER, flags=FLAG_COMPACT_IOC), 22, False, 0, (0.05, 0.2, 1.0)),
}
SEEDS = {}                                  # (chosen on the CPU for the regimes named above; every other case: 300)
PAD_CLASS = 10                              # the slot class that seats 9 or 10 present agents (ctx.h)


def dims(cid):
    return small_dims(**CASES[cid][0])


def tile_rows(cid):
    return 64 if dims(cid).mno == 64 else 32


def slots(cid):
    return ioc_pool_slots(dims(cid).H, tile_rows(cid))


def inputs(cid):
    d = dims(cid)
    past, fut, eps, grids, gos = make_case(d, seed=SEEDS.get(cid, 300), n_absent=CASES[cid][1])
    crowd = CASES[cid][4]
    for s in range(d.n_scenes):
        here = past[s, -1, :, 0] != 0
        if crowd == "diagonal":                                       # slot i walks slot 0's track, i half pixels to the lower right
            for a in (past, fut):
                a[s, :, :, 1:] = a[s, :, :1, 1:] + 0.5 * np.arange(d.mno, dtype=np.float32)[None, :, None]
        else:
            c = past[s, -1][here, 1:].mean(0)
            for a in (past[s], fut[s]):                               # views [T, mno, 3]
                a[:, here, 1:] = np.round((c + crowd[s] * (a[:, here, 1:] - c)) * 2) / 2
    return past, fut, eps, grids, gos


def run_case(torch, cid):
    """(Y [R, T, 2], score [R], Y0 [R, T, 2], sv_h [R, T, H] or None outside training mode) of one forward of case `cid` on the GPU."""
    from desire_amd import _lib
    d = dims(cid)
    _, _, training, min_rows, _ = CASES[cid]
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


def neighbours(cid, Y0):
    """int [groups, T_pred, mno, B]: neighbours of centre row (group, slot) in bin b at that step, on the positions Y0 -- the popcount of the kernel's
    mask word.  Absent OTHERS are dropped, as in the kernel; an absent CENTRE keeps its row (the kernel builds its masks too)."""
    from oracle import desire_oracle as O
    d = dims(cid)
    past = inputs(cid)[0]
    valid = (past[:, d.T_obs - 1, :, 0] != 0)                                        # [n_scenes, mno]
    pos = Y0.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).transpose(0, 1, 3, 2, 4)   # [scene, k, t, slot, 2]
    v = np.broadcast_to(valid[:, None, None, :], pos.shape[:-1])
    bins = O.neighbor_bins(pos, v, d.nb_w, d.nb_h, d.grid_size)                      # [scene, k, t, centre, other]
    cnt = np.stack([(bins == b).sum(-1) for b in range(d.B)], -1)                    # [scene, k, t, centre, B]
    return cnt.reshape(d.n_scenes * d.K, d.T_pred, d.mno, d.B)


def multi_pairs(cid, Y0):
    """(lo, hi): int [tiles, T_pred] each, bounds on the (row, bin) pairs with two or more neighbours per tile-step, which is what the kernel's slot
    counter reaches.  Groups are seated in tiles in row order: 32 // mno groups per tile, one per 64-row tile, 32 // PAD_CLASS per padded tile.
    lo == hi except in a padded form with absent slots in its class, where only the present agents' rows are counted in lo and each absent slot
    of a group may add up to a pair per two present agents in hi."""
    d = dims(cid)
    n = neighbours(cid, Y0)
    padded = CASES[cid][3] is not None
    present = d.mno - CASES[cid][1]
    per_group = (n[:, :, :present if padded else d.mno] >= 2).sum((2, 3))            # [groups, T_pred]
    gpt = 32 // PAD_CLASS if padded else max(1, 32 // d.mno)
    tiles = -(-per_group.shape[0] // gpt)
    lo = np.stack([per_group[i * gpt:(i + 1) * gpt].sum(0) for i in range(tiles)])
    groups = np.array([len(per_group[i * gpt:(i + 1) * gpt]) for i in range(tiles)])[:, None]
    return lo, lo + (groups * (PAD_CLASS - present) * (present // 2) if padded else 0)
