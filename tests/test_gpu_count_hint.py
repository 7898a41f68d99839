"""The count-hinted strided launches of the compacted forward (desire_amd/csrc/dyn_count.h: DynCount.hint, dyn_units).

With device-side counts five kernels -- k_encoder_pair<64|128|256>, k_deconv2<true>, k_deconv3<true, 4>, k_deconv2_x6<3>, k_deconv3_x6i<3> -- get a grid sized
from a HINT of the present-agent count (the previous call's), and a workgroup strides over tiles bx, bx + gridDim.x, ..; launch_gemm_rows picks its <1,1>
or <4,2> variant from the same stale guess.  Every other compacted test shape lies below the 256 units of slack, so there every workgroup makes one trip.

Under hipGraph capture nothing executes: the hint is the count of the call BEFORE the capture and the grids are baked into the graph.  So here a graph S
captured after a one-agent batch (hint 1: 9 encoder tiles per encoder, 65 / 130 deconvolution workgroups) is replayed on a crowded batch (P = 715 agents:
23 encoder tiles -> 3 trips, 537 four-sample tiles -> 9 trips, 1073 two-sample tiles -> 9 trips, every last tile ragged and reached on the last trip), and
a graph B captured after the crowded batch is replayed on sparse ones.  Contract:
  * Y0 / Hx / Hy of present rows and agents BIT-IDENTICAL to a fresh uncompacted handle (flags = 0), exact zeros on absent ones;
  * Y and score within the bounds tests/test_gpu_compact_rows.py holds the device-count path to against the uncompacted handle (2e-6, 1e-4);
  * whole windows whose agents sit in the first, a middle and the last (ragged) trip against the CPU oracle at the bars of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests.helpers import hinted_units, small_dims, to_oracle_layout
from tests.test_gpu_compact_rows import ragged_counts, row_mask
from tests.test_gpu_parity import TOL_MID, TOL_Y

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
# windows of the crowded batch: 29 .. 32 present agents each, one empty, several full; P = 715 is odd (P % 32, P * 3 % 4, P * 3 % 2, P * 2 % 4 all != 0)
BIG = [31, 32, 30, 32, 29, 31, 0, 32, 31, 30, 32, 31, 32, 29, 32, 31, 30, 32, 31, 32, 30, 31, 32, 32]
MID = [5, 3, 0, 9, 4, 2, 7, 1, 6, 4, 0, 8, 3, 5, 2, 6, 4, 7, 1, 5, 3, 6, 4, 5]
ONE = [0] * 13 + [1] + [0] * 10
NONE = [0] * 24
ENC_TM, DECONV_NS, DECONV_X6I_NS, GEMM_TM = 32, 4, 2, 64          # units per tile: k_encoder_pair, k_deconv2 / k_deconv3 / k_deconv2_x6, k_deconv3_x6i; DS_TM


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def ceil_div(a, b):
    return -(-a // b)


def stride_plan(d, P, hint):
    """(tiles of work, workgroups) of every strided launch for P present agents when the grid was sized from `hint` (tests/helpers.py: hinted_units)."""
    return {"encoder": (ceil_div(P, ENC_TM), ceil_div(hinted_units(d.A, hint, 1), ENC_TM)),
            "deconv2/3": (ceil_div(P * d.K, DECONV_NS), ceil_div(hinted_units(d.R, hint, d.K), DECONV_NS)),
            "deconv3_x6i": (ceil_div(P * d.K, DECONV_X6I_NS), ceil_div(hinted_units(d.R, hint, d.K), DECONV_X6I_NS))}


def gemm_variant(rows, NT):
    """launch_gemm_rows (kernels_gemm.hip): <1,1> below 128 workgroups of the <4,2> form, else <4,2>."""
    return "<1,1>" if ceil_div(rows, GEMM_TM) * ceil_div(NT, 16) < 128 else "<4,2>"


def check_preconditions(d, P):
    """Before any GPU work: the shapes of this file do stride, and the stale hint does pick the other GEMM variant.  The figures describe the grid rule at
    these shapes; which of the launches a case RUNS depends on the case: dims.posterior = 0 runs launch_encoder on the worst-case grid (the control: the
    encoder plan is not exercised there), and dims.bf16 = 2 / 3 run deconv1 as launch_deconv1_x6, so only the fp32 operand cases at K = 3 (fp32, H = 64,
    posterior = 0) run launch_gemm_rows with the variant the stale hint picked."""
    assert len(BIG) == d.n_scenes and min(c for c in BIG if c) >= 29 and 0 in BIG and d.mno in BIG
    assert P == sum(BIG) and P % 2 == 1 and P >= 700 and P % ENC_TM and (P * d.K) % DECONV_NS
    plan = stride_plan(d, P, hint=1)
    trips = {k: ceil_div(t, g) for k, (t, g) in plan.items()}
    print("P_big = %d, K = %d; (tiles, workgroups) with hint 1: %s; trips: %s" % (P, d.K, plan, trips))
    assert plan["encoder"][1] == 9 and plan["encoder"][0] >= 22 and trips["encoder"] >= 3
    assert plan["deconv2/3"][1] == 65
    assert all(hinted_units(w, P, m) == w for w, m in ((d.A, 1), (d.R, d.K)))      # graph B: the worst-case grids, one trip
    if d.K == 3:
        assert plan["deconv2/3"][0] >= 525 and plan["deconv3_x6i"][0] >= 1050 and plan["deconv3_x6i"][1] == 130 and (P * d.K) % DECONV_X6I_NS
        # deconv1 [P * K, L] x [L, 2048] (NT = 64): the true count asks for <4,2>, the stale M_hint = 1 * K picks <1,1>
        assert ceil_div(P * d.K, GEMM_TM) * 4 >= 128
        assert gemm_variant(P * d.K, 64) == "<4,2>" and gemm_variant(1 * d.K, 64) == "<1,1>"
    else:       # K = 2 at the same n_scenes (the H = 256 case): the deconvolutions still make several trips; deconv1 stays <1,1> either way
        assert trips["deconv2/3"] >= 3
    return trips


def make_batches(d):
    """The four batches on ONE set of scene grids (a captured graph holds the grid pointer): name -> (past, fut, eps, keep)."""
    out, grids, gos = {}, None, None
    for seed, (name, counts) in enumerate((("big", BIG), ("one", ONE), ("none", NONE), ("mid", MID))):
        past, fut, eps, g, go, keep = ragged_counts(d, seed=60 + seed, counts=counts)
        if grids is None:
            grids, gos = g, go
        assert (keep.sum(1) == np.array(counts)).all()
        out[name] = (past, fut, eps, keep)
    return out, grids, gos


def pick_windows(d, keep, n):
    """n whole windows of the crowded batch for the oracle: the first and the last one with agents (compacted tiles of the first trip, and the ragged
    last tile of the last trip, of every strided kernel) and windows from the middle of the batch."""
    full = [i for i in range(d.n_scenes) if keep[i].any()]
    wins = [full[0], full[-1]] if n == 2 else [full[0], full[len(full) // 3], full[len(full) // 2], full[-1]]
    return sorted(set(wins))


def trips_of_windows(d, keep, wins):
    """Which trip of the hint-1 grids serves the agents / samples of `wins`: compacted agent p (scan order = agent order), sample r = k * P + p of the
    pseudo-scene of P slots the per-row stages run on."""
    P = int(keep.sum())
    plan = stride_plan(d, P, hint=1)
    idx = np.cumsum(keep.reshape(-1)) - 1                                   # agent -> compacted index (where present)
    sel = np.zeros_like(keep); sel[wins] = True
    p = idx[(keep & sel).reshape(-1)]
    rows = (np.arange(d.K)[:, None] * P + p[None, :]).reshape(-1)
    enc = set((p // ENC_TM // plan["encoder"][1]).tolist())
    dc = set((rows // DECONV_NS // plan["deconv2/3"][1]).tolist())
    dc6 = set((rows // DECONV_X6I_NS // plan["deconv3_x6i"][1]).tolist())
    last = {"encoder": (P - 1) // ENC_TM in set((p // ENC_TM).tolist()), "deconv": (P * d.K - 1) // DECONV_NS in set((rows // DECONV_NS).tolist())}
    return enc, dc, dc6, last


def outputs(h, d, Y, sc):
    out = dict(Y0=h.read_buffer("Y0", (d.R, d.T_pred, 2)), Hx=h.read_buffer("Hx", (d.A, d.H)), Y=Y.cpu().numpy(), score=sc.cpu().numpy())
    if d.posterior:
        out["Hy"] = h.read_buffer("Hy", (d.A, d.H))
    return out


def reference(torch, d, w, batch, grids, gos):
    """A fresh uncompacted handle (flags = 0) on the batch: Y0, Hx, Hy, Y, score.  (Not `run` of tests/test_gpu_compact_rows.py: that helper closes
    its handle before Hx and Hy can be read, and returns neither.)"""
    from desire_amd import _lib
    past, fut, eps, _ = batch
    h = _lib.Handle(d.replace(flags=0)); h.set_weights(w)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    p_t, f_t, e_t, g_t = t(past), t(fut), t(eps), t(grids)
    h.set_scene_grids(g_t.data_ptr(), gos)
    Y = torch.full((d.R, d.T_pred, 2), SENTINEL, device="cuda"); sc = torch.full((d.R,), SENTINEL, device="cuda")
    h.forward(p_t.data_ptr(), f_t.data_ptr() if d.posterior else 0, e_t.data_ptr(), Y.data_ptr(), sc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = outputs(h, d, Y, sc)
    h.close()
    return out


_ORACLE = {}


def oracle_windows(d, w, batch, grids, gos, wins):
    """The CPU oracle on the windows `wins` alone (it treats windows independently).  Its sample generation does not depend on the operand mode, so the
    cases that differ in dims.bf16 only share one run: the cache is keyed on every other field of the dims, and a hit must have been computed from
    the same weights and inputs."""
    from oracle import desire_oracle as O
    past, fut, eps, _ = batch
    dw = d.replace(n_scenes=len(wins), flags=0, bf16=0)
    eps_w = np.ascontiguousarray(eps.reshape(d.n_scenes, d.K * d.mno, d.L)[wins].reshape(-1, d.L))
    ins = [past[wins], fut[wins], eps_w, grids, gos[wins]] + [w[k] for k in sorted(w)]
    key = (repr(dw), tuple(wins))
    if key not in _ORACLE:
        ref = O.forward(to_oracle_layout(past[wins]), to_oracle_layout(fut[wins]) if d.posterior else None, eps_w, grids, gos[wins], w, dw)
        _ORACLE[key] = ({k: ref[k] for k in ("Hx", "Hy", "Y0") if k in ref}, ins)
    ref, ins0 = _ORACLE[key]
    assert len(ins) == len(ins0) and all(np.array_equal(a, b) for a, b in zip(ins, ins0)), "oracle cache hit with other weights or inputs"
    return ref


class Session:
    """One compacted handle (compact_min_rows = 0) with fixed device buffers, so that a captured graph can be replayed on another batch."""
    # the stages between the caller's outputs and the handle's: a tile that no trip reached keeps the sentinel instead of an earlier replay's rows
    SCRUB = ["Y0", "HxHy", "cp_Y0", "cp_HxHy", "cp_plast", "d1", "d2", "d3", "xhat", "xz"]

    def __init__(self, torch, d, w, batches, grids, gos):
        from desire_amd import _lib
        self.torch, self.d, self.batches = torch, d, batches
        self.t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
        self.h = _lib.Handle(d); self.h.set_weights(w); self.h.set_option("compact_min_rows", 0)
        self.g_t = self.t(grids)
        self.h.set_scene_grids(self.g_t.data_ptr(), gos)
        self.p, self.f, self.e = (self.t(x) for x in batches["big"][:3])
        self.Y = torch.full((d.R, d.T_pred, 2), SENTINEL, device="cuda"); self.sc = torch.full((d.R,), SENTINEL, device="cuda")
        self.side = torch.cuda.Stream(); self.sp = self.side.cuda_stream
        self.scrub = self.SCRUB + (["cp_params", "vae_in"] if d.posterior else [])

    def load(self, tag):
        past, fut, eps, _ = self.batches[tag]
        self.p.copy_(self.t(past)); self.f.copy_(self.t(fut)); self.e.copy_(self.t(eps))
        self.torch.cuda.synchronize()

    def forward(self):
        self.h.forward(self.p.data_ptr(), self.f.data_ptr() if self.d.posterior else 0, self.e.data_ptr(), self.Y.data_ptr(), self.sc.data_ptr(), self.sp)

    def direct(self, tag):
        self.load(tag)
        self.forward()
        self.torch.cuda.synchronize()

    def capture(self):
        """The forward as a graph: nothing executes, the grids are baked from the count of the call before."""
        self.h.graph_begin(self.sp)
        self.forward()
        return self.h.graph_end(self.sp)

    def replay(self, gid, tag):
        self.load(tag)
        self.Y.fill_(SENTINEL); self.sc.fill_(SENTINEL)
        for name in self.scrub:
            self.h.device_tensor(name).fill_(SENTINEL)
        self.torch.cuda.synchronize()
        self.h.graph_launch(gid, self.sp)
        self.side.synchronize()
        self.torch.cuda.synchronize()
        return outputs(self.h, self.d, self.Y, self.sc)


def check(d, got, ref, keep, what):
    """A replay's outputs against the uncompacted handle's on the same batch."""
    m, ma = row_mask(d, keep), keep.reshape(-1)
    for k in got:
        assert np.isfinite(got[k]).all(), (what, k)
    for k, mk in (("Y0", m), ("Hx", ma), ("Hy", ma)):
        if k not in got:
            continue
        np.testing.assert_array_equal(got[k][mk], ref[k][mk], err_msg="%s: %s of present rows" % (what, k))
        assert not got[k][~mk].any(), (what, k, "absent rows")
    if m.any():
        eY, es = float(np.abs(got["Y"][m] - ref["Y"][m]).max()), float(np.abs(got["score"][m] - ref["score"][m]).max())
        print("%s: max|Y - uncompacted| = %.2e, max|score - uncompacted| = %.2e" % (what, eY, es))
        assert eY < 2e-6 and es < 1e-4, (what, eY, es)
    assert not got["Y"][~m].any() and not got["score"][~m].any(), (what, "absent rows")


def check_oracle(d, got, orc, keep, wins):
    """The windows `wins` of a replay on the crowded batch against the CPU oracle on those windows: later trips against a high-precision reference,
    not only against another HIP path."""
    sel = np.zeros_like(keep); sel[wins] = True
    ka = keep[wins].reshape(-1)
    for k in ("Hx", "Hy"):
        if k in got:
            err = float(np.abs(got[k][(keep & sel).reshape(-1)] - orc[k].reshape(-1, d.H)[ka]).max())
            print("graph S on 'big', windows %s: max|%s - oracle| = %.2e" % (wins, k, err))
            assert err < TOL_MID, (k, err)
    err = float(np.abs(got["Y0"][row_mask(d, keep & sel)] - orc["Y0"].reshape(-1, d.T_pred, 2)[row_mask(d, keep[wins])]).max())
    print("graph S on 'big', windows %s: max|Y0 - oracle| = %.2e" % (wins, err))
    assert err < TOL_Y, err


CASES = [
    dict(),                                       # fp32: k_encoder_pair<128>, k_deconv2, k_deconv3; deconv1 on the GEMM variant the stale hint picked
    dict(bf16=3),                                 # the two six-product deconvolutions
    dict(bf16=2),                                 # the same generation kernels under the split IOC
    dict(H=64, L=64),                             # k_encoder_pair<64>
    dict(H=256, K=2),                             # k_encoder_pair<256>, the 512-thread form (oracle check on two windows)
    dict(posterior=0),                            # the control: launch_encoder with the worst-case grid, only the deconvolutions stride
]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()) or "fp32")
def test_graphs_baked_with_a_stale_count_hint_follow_the_data(torch_cuda, kw):
    torch = torch_cuda
    d = small_dims(**{**dict(n_scenes=24, mno=32, K=3, T_obs=4, T_pred=6, n_grids=1), **kw}).replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC)
    batches, grids, gos = make_batches(d)
    keep_big = batches["big"][3]
    P_big = int(keep_big.sum())
    check_preconditions(d, P_big)
    n_or = 2 if d.H == 256 else 4
    wins = pick_windows(d, keep_big, n_or)
    enc_trips, dc_trips, dc6_trips, last = trips_of_windows(d, keep_big, wins)
    plan = stride_plan(d, P_big, hint=1)
    n_enc, n_dc = ceil_div(*plan["encoder"]), ceil_div(*plan["deconv2/3"])
    assert len(wins) == n_or and 0 in enc_trips and n_enc - 1 in enc_trips and last["encoder"] and last["deconv"]
    assert {0, n_dc - 1} <= dc_trips and {0, ceil_div(*plan["deconv3_x6i"]) - 1} <= dc6_trips
    if n_or == 4:
        assert any(0 < t < n_enc - 1 for t in enc_trips) and any(0 < t < n_dc - 1 for t in dc_trips)

    w = init_weights(d, 9)
    refs = {tag: reference(torch, d, w, batches[tag], grids, gos) for tag in batches}
    s = Session(torch, d, w, batches, grids, gos)
    s.direct("big"); s.direct("one")                   # the lazy allocations happen outside capture; the count word now holds 1
    S = s.capture()                                    # baked with hint = 1
    s.direct("big")                                    # the count word holds P_big
    B = s.capture()                                    # baked with hint = P_big: the worst-case grids
    first = None
    for i, tag in enumerate(("big", "one", "none", "mid", "big")):
        got = s.replay(S, tag)
        check(d, got, refs[tag], batches[tag][3], "graph S (hint 1), replay %d on '%s'" % (i, tag))
        if tag == "big" and first is None:
            first = got
            check_oracle(d, got, oracle_windows(d, w, batches["big"], grids, gos, wins), keep_big, wins)
        elif tag == "big":
            for k in got:
                np.testing.assert_array_equal(got[k], first[k], err_msg="second replay of S on 'big': %s" % k)
    for i, tag in enumerate(("one", "big", "none", "mid")):
        check(d, s.replay(B, tag), refs[tag], batches[tag][3], "graph B (hint %d), replay %d on '%s'" % (P_big, i, tag))
    s.h.close()
