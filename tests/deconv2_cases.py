"""The cases of tests/test_gpu_deconv2_regs.py and of its digest generator tests/golden/make_deconv2_digests.py (plain helpers, no fixtures).

k_deconv2 (desire_amd/csrc/kernels_conv.hip) works on tiles of four samples, one pair per wave and one sample per half-wave, and a workgroup strides over
tiles when its grid was sized from a count hint.  It can go wrong where a pair or a tile is partly empty or where a workgroup runs a second tile, so:

  rows1 .. rows9   R = P * K = 1, 2, 3, 5, 9 rows through the compacted path (DESIRE_FLAG_COMPACT_ROWS): one live half-wave and three clamped ones, ..,
                   a full tile plus a tile with one live sample
  hint             a graph baked with a count hint of one agent replayed on 715 (tests/test_gpu_count_hint.py's mechanism): 65 workgroups stride over
                   537 tiles, the last one ragged -- an accumulator that is not cleared per tile shows here
  dense            small_dims(), every slot present: k_deconv2<true> on full tiles
  bn1              small_dims(bn_mode=1): k_deconv2<false> (linear epilogue, then the per-object normalisation pass)

run_case gives the live rows of "d1" and "d2" as the GPU left them; reference_error holds d2 against the float64 evaluation of the deconv2 stage on that
very d1 under the rule of tests/stage_reference.py (check_stage: its bound, imported, not restated)."""
import hashlib

import numpy as np

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from oracle import desire_oracle as O
from tests import stage_reference as SR
from tests.helpers import make_case, small_dims

# id -> (P present agents of one window of 8 slots, K)
RAGGED = {"rows1": (1, 1), "rows2": (1, 2), "rows3": (3, 1), "rows5": (5, 1), "rows9": (3, 3)}
CASES = list(RAGGED) + ["hint", "dense", "bn1"]


def _per_object(i, w, d, dt, q=None):
    x = i["d1"].astype(dt)
    return O.deconv_layer(x.reshape(x.shape[0], 4, 4, 128), w, "deconv2", bn_mode="per_object", dt=dt).reshape(x.shape[0], -1)


STAGE = SR.stage("deconv2")                                                   # frozen batch-norm: the stage of the parity test itself
STAGE_BN1 = SR.Stage("deconv2", ("d1",), ("d2",), _per_object)                # dims.bn_mode = 1: the same layer with per-object moments


def weights(d, seed):
    return SR.spread_weights(init_weights(d, seed), SR.VEL_FC, SR.MASK_FC)


def _forward(torch, d, w, raw):
    from tests.test_gpu_parity import run_gpu
    h, _, _ = run_gpu(torch, d, w, *raw)
    d1, d2 = h.read_buffer("d1", (d.R, 2048)), h.read_buffer("d2", (d.R, 4096))
    h.close()
    return d1, d2


def _hint(torch):
    """Graph S of tests/test_gpu_count_hint.py: captured after a one-agent batch, replayed on the crowded one."""
    from tests import test_gpu_count_hint as CH
    d = small_dims(n_scenes=24, mno=32, K=3, T_obs=4, T_pred=6, n_grids=1).replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC)
    batches, grids, gos = CH.make_batches(d)
    P = int(batches["big"][3].sum())
    tiles, wgs = CH.stride_plan(d, P, hint=1)["deconv2/3"]
    assert tiles >= 2 * wgs and (P * d.K) % CH.DECONV_NS, (tiles, wgs)       # every workgroup runs at least two tiles, the last tile is ragged
    w = weights(d, 109)
    s = CH.Session(torch, d, w, batches, grids, gos)
    s.direct("big"); s.direct("one")
    S = s.capture()
    s.replay(S, "big")
    rows = P * d.K
    d1, d2 = s.h.read_buffer("d1", (d.R, 2048))[:rows], s.h.read_buffer("d2", (d.R, 4096))[:rows]
    s.h.close()
    # rows held to float64: the first tile, the tiles either side of the end of the first trip, the last full tile and the ragged one
    edge = wgs * CH.DECONV_NS
    pick = np.unique(np.concatenate([np.arange(8), np.arange(edge - 8, edge + 8), np.arange(rows - 8, rows)]))
    return d, w, d1, d2, pick


def run_case(torch, cid):
    """(dims, weights, d1 [rows, 2048], d2 [rows, 4096], rows held to the float64 reference, stage) of case `cid` on the GPU."""
    if cid == "hint":
        return _hint(torch) + (STAGE,)
    if cid in RAGGED:
        P, K = RAGGED[cid]
        d = small_dims(n_scenes=1, mno=8, K=K, T_obs=4, T_pred=6, n_grids=1).replace(flags=FLAG_COMPACT_ROWS)
        w = weights(d, 101 + P + 10 * K)
        d1, d2 = _forward(torch, d, w, make_case(d, seed=201 + P + 10 * K, n_absent=d.mno - P))
        rows = P * K
        assert rows in (1, 2, 3, 5, 9)
        return d, w, d1[:rows], d2[:rows], np.arange(rows), STAGE
    d = small_dims(bn_mode=1) if cid == "bn1" else small_dims()
    w = weights(d, 107)
    d1, d2 = _forward(torch, d, w, make_case(d, seed=207, n_absent=0))
    return d, w, d1, d2, np.arange(d.R), (STAGE_BN1 if cid == "bn1" else STAGE)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def reference_error(run, check=True):
    """max|d2 - float64 stage reference| over the picked rows of a run_case result, its tolerance, and max|d2| of the case;
    check=True applies stage_reference.check_stage (which asserts the bound)."""
    d, w, d1, d2, pick, st = run
    inp = {"d1": d1[pick]}
    ref, tol, _ = SR.stage_tolerance(st, inp, w, d)
    err = float(np.abs(d2[pick].astype(np.float64) - ref["d2"]).max())
    if check:
        SR.check_stage(st, inp, {"d2": d2[pick]}, w, d)
    return err, tol["d2"], float(np.abs(d2).max())
