"""The cases of tests/test_gpu_gen_chain_bits.py and of its digest generator tests/golden/make_gen_chain_digests.py (plain helpers, no fixtures).

k_deconv3 (desire_amd/csrc/kernels_conv.hip) runs 25 (parity class, tap) chains of 64 MFMAs per tile of four samples, one sample per wave, and a
workgroup strides over tiles when its grid was sized from a count hint; k_decoder (desire_amd/csrc/kernels_rnn.hip) runs three chains per step
on a 32- or 64-row tile.  k_deconv3 requests a chain's weight fragments and LDS row pointers a chain ahead, across class and tile boundaries, and
k_decoder runs its chains unrolled over named fragment sets with the A fragment read a group ahead, so the cases are the places where a fragment
set, a row pointer or an A fragment carried over such a boundary would be the wrong one:

  rows1 .. rows9   R = P * K = 1, 2, 3, 5, 9 rows through the compacted path (DESIRE_FLAG_COMPACT_ROWS): one live wave of four, .., a full tile plus
                   one live sample; the decoder runs its device-side row count (DYN_P) on a partial tile
  hint             a graph baked with a count hint of one agent replayed on 715 (tests/test_gpu_count_hint.py's mechanism): 65 workgroups stride
                   over 537 tiles, the last one ragged -- a prefetch or an A read carried wrongly across a tile's barriers shows here
  dense            small_dims(), every slot present: k_deconv3<true,4> on full tiles, k_decoder<128,32,false> on eight full tiles
  bn1              small_dims(bn_mode=1): k_deconv3<false,4> in mode 3 (linear epilogue, then the per-object normalisation pass)
  h64, h128, h256  three windows of 8 slots, K = 3: 72 rows = a 64-row tile + 8 rows of k_decoder<64,64>, two 32-row tiles + 8 rows of
                   k_decoder<128,32> and k_decoder<256,32> (chains of one, two and four pairs of chunks)
  ref_compat       dims.ref_compat: 7 decoder steps whose hidden states ("dec_states") are the output, through the SAVE instantiation
  train_h64, train_h128, train_h256   training mode: the SAVE instantiations; the saved gates, candidates and hidden states are the output
  train_step       one forward + backward in training mode: the flat gradient (backward.hip runs k_deconv3<false,4> for a data gradient)

Every sample exercises every border tap of deconv3 (each 8 x 8 image has all four borders), so no extra shape is needed for those.

run_case gives a dict of the buffers of one case as the GPU left them; INPUTS are the ones the two kernels read ("d2"; "xz" and "HxHy"), whose digests
are recorded next to the outputs' so that a moved input is reported as that.  reference_error holds d3 against the float64 evaluation of the deconv3
stage on that very d2 under the rule of tests/stage_reference.py (check_stage: its bound, imported, not restated)."""
import hashlib

import numpy as np

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, Dims, init_weights
from oracle import desire_oracle as O
from tests import stage_reference as SR
from tests.helpers import make_case, small_dims

# id -> (P present agents of one window of 8 slots, K)
RAGGED = {"rows1": (1, 1), "rows2": (1, 2), "rows3": (3, 1), "rows5": (5, 1), "rows9": (3, 3)}
D3_CASES = list(RAGGED) + ["hint", "dense", "bn1"]                           # held to the float64 stage reference of deconv3 as well
HIDDEN = {"h64": 64, "h128": 128, "h256": 256}
TRAIN = {"train_h64": 64, "train_h128": 128, "train_h256": 256}
CASES = D3_CASES + list(HIDDEN) + ["ref_compat"] + list(TRAIN) + ["train_step"]
INPUTS = ("d2", "xz", "HxHy")
SAVES = ("dec_sv_h", "dec_sv_r", "dec_sv_u", "dec_sv_c")


def _per_object(i, w, d, dt, q=None):
    x = i["d2"].astype(dt)
    return O.deconv_layer(x.reshape(x.shape[0], 8, 8, 64), w, "deconv3", bn_mode="per_object", dt=dt).reshape(x.shape[0], -1)


STAGE = SR.stage("deconv3")                                                   # frozen batch-norm: the stage of the parity test itself
STAGE_BN1 = SR.Stage("deconv3", ("d2",), ("d3",), _per_object)                # dims.bn_mode = 1: the same layer with per-object moments


def weights(d, seed):
    return SR.spread_weights(init_weights(d, seed), SR.VEL_FC, SR.MASK_FC)


def _buffers(h, d, rows):
    """The live rows of the sample-generation buffers of handle `h` ("Y0" whole: the compacted path scatters it back into the caller's rows)."""
    A = d.n_scenes * d.mno
    return {"d2": h.read_buffer("d2", (d.R, 4096))[:rows], "d3": h.read_buffer("d3", (d.R, 8192))[:rows], "xz": h.read_buffer("xz", (d.R, d.H))[:rows],
            "HxHy": np.concatenate([h.read_buffer("Hx", (A, d.H)), h.read_buffer("Hy", (A, d.H))], 1), "Y0": h.read_buffer("Y0", (d.R, d.T_pred, 2))}


def _forward(torch, d, w, raw, rows):
    from tests.test_gpu_parity import run_gpu
    h, _, _ = run_gpu(torch, d, w, *raw)
    out = _buffers(h, d, rows)
    h.close()
    return out


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
    out = _buffers(s.h, d, rows)
    s.h.close()
    # rows held to float64: the first tile, the tiles either side of the end of the first trip, the last full tile and the ragged one
    edge = wgs * CH.DECONV_NS
    pick = np.unique(np.concatenate([np.arange(8), np.arange(edge - 8, edge + 8), np.arange(rows - 8, rows)]))
    return d, w, out, pick


def _train(torch, d, w, raw, backward):
    from desire_amd import _lib
    past, fut, eps, grids, gos = raw
    h = _lib.Handle(d)
    h.set_weights(w)
    h.set_training(True)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    past_t, fut_t, eps_t, grids_t = t(past), t(fut), t(eps), t(grids)
    h.set_scene_grids(grids_t.data_ptr(), gos)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda")
    score = torch.zeros((d.R,), device="cuda")
    h.forward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr(), Y.data_ptr(), score.data_ptr())
    torch.cuda.synchronize()
    out = _buffers(h, d, d.R)
    for name in SAVES:
        out[name] = h.read_buffer(name, (d.R, d.T_pred, d.H))
    if backward:
        h.backward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr())
        torch.cuda.synchronize()
        out["grad"] = h.grad_tensor().cpu().numpy()
    h.close()
    return out


def _ref_compat(torch):
    """model/model.py:279-289 as dims.ref_compat runs it (tests/test_gpu_small_hidden.py): d_dim 16, 7 decoder steps, the states are the output."""
    from desire_amd import _lib
    T, n_dec, mno = 8, 7, 8
    d = Dims(n_scenes=2, mno=mno, K=1, T_obs=T, T_pred=T, H=2 * T, L=64, sx=1.0, sy=1.0, bn_mode=1, ref_compat=1, n_dec=n_dec, n_grids=1)
    w = init_weights(d, 117, ref_init=True)
    rng = np.random.default_rng(118)
    x = np.zeros((2, T + 1, mno, 3), np.float32)
    x[..., 0] = np.arange(1, mno + 1)
    x[..., 1:] = np.round(rng.uniform(5, 1400, (2, 1, mno, 2)) + np.cumsum(rng.normal(0, 3, (2, T + 1, mno, 2)), 1))
    x[:, :, mno - 2:] = 0                                    # two empty slots
    past, fut = np.ascontiguousarray(x[:, :T]), np.ascontiguousarray(x[:, 1:])
    eps = rng.standard_normal((d.A, d.L)).astype(np.float32)
    h = _lib.Handle(d)
    h.set_weights(w)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    p_t, f_t, e_t = t(past), t(fut), t(eps)
    states = torch.zeros((d.A, n_dec, T, 2), device="cuda")
    h.forward(p_t.data_ptr(), f_t.data_ptr(), e_t.data_ptr(), states.data_ptr(), 0)
    torch.cuda.synchronize()
    out = {"d2": h.read_buffer("d2", (d.R, 4096)), "d3": h.read_buffer("d3", (d.R, 8192)), "xz": h.read_buffer("xz", (d.R, d.H)),
           "HxHy": np.concatenate([h.read_buffer("Hx", (d.A, d.H)), h.read_buffer("Hy", (d.A, d.H))], 1), "dec_states": states.cpu().numpy()}
    h.close()
    return d, w, out


def run_case(torch, cid):
    """(dims, weights, buffers {name: array}, rows of d3 held to the float64 reference or None, stage) of case `cid` on the GPU."""
    if cid == "hint":
        return _hint(torch) + (STAGE,)
    if cid == "ref_compat":
        return _ref_compat(torch) + (None, None)
    if cid in RAGGED:
        P, K = RAGGED[cid]
        d = small_dims(n_scenes=1, mno=8, K=K, T_obs=4, T_pred=6, n_grids=1).replace(flags=FLAG_COMPACT_ROWS)
        w = weights(d, 101 + P + 10 * K)
        rows = P * K
        assert rows in (1, 2, 3, 5, 9)
        return d, w, _forward(torch, d, w, make_case(d, seed=201 + P + 10 * K, n_absent=d.mno - P), rows), np.arange(rows), STAGE
    if cid in ("dense", "bn1"):
        d = small_dims(bn_mode=1) if cid == "bn1" else small_dims()
        w = weights(d, 107)
        return d, w, _forward(torch, d, w, make_case(d, seed=207, n_absent=0), d.R), np.arange(d.R), (STAGE_BN1 if cid == "bn1" else STAGE)
    if cid == "train_step":
        d = small_dims(n_scenes=2, mno=8, K=3, T_obs=4, T_pred=6, n_grids=1)
        w = weights(d, 141)
        return d, w, _train(torch, d, w, make_case(d, seed=241, n_absent=1), True), None, None
    H = HIDDEN.get(cid) or TRAIN[cid]
    d = small_dims(n_scenes=3, mno=8, K=3, T_obs=4, T_pred=6, n_grids=1, H=H)
    assert d.R == 72                                                          # a 64-row tile + 8 rows; two 32-row tiles + 8 rows
    w = weights(d, 120 + H // 64)
    raw = make_case(d, seed=220 + H // 64, n_absent=0)
    return d, w, (_train(torch, d, w, raw, False) if cid in TRAIN else _forward(torch, d, w, raw, d.R)), None, None


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def digests(run):
    """{buffer name + "_sha256": digest} of a run_case result."""
    return {k + "_sha256": sha(v) for k, v in run[2].items()}


def reference_error(run, check=True):
    """max|d3 - float64 stage reference| over the picked rows of a run_case result, its tolerance, and max|d3| of the case;
    check=True applies stage_reference.check_stage (which asserts the bound)."""
    d, w, buf, pick, st = run
    inp = {"d2": buf["d2"][pick]}
    ref, tol, _ = SR.stage_tolerance(st, inp, w, d)
    err = float(np.abs(buf["d3"][pick].astype(np.float64) - ref["d3"]).max())
    if check:
        SR.check_stage(st, inp, {"d3": buf["d3"][pick]}, w, d)
    return err, tol["d3"], float(np.abs(buf["d3"]).max())
