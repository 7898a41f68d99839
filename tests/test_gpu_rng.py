"""The device generator (include/desire_hip.h "device generator"; csrc/philox.h, csrc/kernels_rng.hip) on the GPU.

A latent normal is a pure function of (seed, draw, global window, k, global slot, latent), drawn where it is consumed.  Held here:
  1. the fill stream: raw words equal the numpy restatement (tests/rng_reference.py) exactly, normals within 1e-5 of float64 on the same bits (the
     bound is derived in tests/test_rng_cpu.py), mean / variance / Kolmogorov distance of 2^20 normals inside the bounds of rng_reference.moment_bounds
     for the fixed seed rng_reference.STREAM_SEED (which passes them on the restatement alone), a ragged fill equals the slice of a longer one;
  2. desire_forward with NULL eps == desire_forward on a second handle given the eps that the latent fill wrote: Y and score bit-identical;
  3. a compacted handle == a padded one, both generating: "Y0" of present rows bit-identical, "z" equal through the compact row map;
  4. the same through several trips of the compacted stride loops (a graph captured after a one-agent batch, replayed on a crowded one);
  5. cut independence: four windows at once == two calls of two windows at scene_base 0 and 2; a 16-slot handle at slot_base 16 == slots 16..31 of a
     32-slot handle;
  6. a captured forward draws fresh noise on every replay, and re-seeding replays the same noise bit for bit;
  7. a training step with NULL eps == the step on the explicit eps of the used draw: the flat gradient buffer bit-identical, one draw per step;
  8. NULL eps before desire_set_rng and dims outside the counter packing are refused."""
import numpy as np
import pytest

from desire_amd.spec import FLAG_COMPACT_IOC, FLAG_COMPACT_ROWS, init_weights
from tests import rng_reference as R
from tests.helpers import make_case, small_dims

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD9876F00D                    # (both key words in use)
NORMAL_TOL = 1e-5                            # fp32 normals against float64 on the same bits (derivation: tests/test_rng_cpu.py)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def handle(torch, d, w, grids, gos):
    """A handle with weights and grids; the grid tensor rides along so that it outlives the calls."""
    from desire_amd import _lib
    h = _lib.Handle(d)
    h.set_weights(w)
    h._grids = dev(torch, grids)
    h.set_scene_grids(h._grids.data_ptr(), gos)
    return h


def forward(torch, h, past, fut, eps_t=None, stream=0):
    """desire_forward; eps_t None = NULL eps.  Returns (Y, score) as numpy after synchronising."""
    d = h.dims
    p_t, f_t = dev(torch, past), dev(torch, fut)
    Y = torch.full((d.R, d.T_pred, 2), 7.0, device="cuda")
    sc = torch.full((d.R,), 7.0, device="cuda")
    h.forward(p_t.data_ptr(), f_t.data_ptr() if d.posterior else 0, 0 if eps_t is None else eps_t.data_ptr(), Y.data_ptr(), sc.data_ptr(), stream)
    torch.cuda.synchronize()
    return Y.cpu().numpy(), sc.cpu().numpy()


def latent_eps(torch, h, seed, draw):
    """The explicit eps [R, L] of (seed, draw) at the handle's origin, written by the latent fill."""
    from desire_amd import _lib
    d = h.dims
    e = torch.full((d.R, d.L), 9.0, device="cuda")
    h.rng_fill(seed, draw, 0, _lib.RNG_LATENT, e.data_ptr(), e.numel())
    torch.cuda.synchronize()
    return e


# ---- 1. the stream ------------------------------------------------------------------------------------------------------------------------------
def test_fill_stream_equals_the_restatement_and_is_normal(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    h = _lib.Handle(small_dims(n_scenes=1, mno=8, K=1, T_obs=4, T_pred=6))            # (the fill needs a handle, not its weights)
    n, pad = R.STREAM_N, 8
    bits = torch.full((n + pad,), 0x5A5A5A5A, device="cuda", dtype=torch.int32)
    nrm = torch.full((n + pad,), 9.0, device="cuda")
    h.rng_fill(R.STREAM_SEED, R.STREAM_ID, 0, _lib.RNG_BITS, bits.data_ptr(), n)
    h.rng_fill(R.STREAM_SEED, R.STREAM_ID, 0, _lib.RNG_NORMAL, nrm.data_ptr(), n)
    torch.cuda.synchronize()
    assert (bits[n:] == 0x5A5A5A5A).all() and (nrm[n:] == 9.0).all(), "a fill wrote past its n elements"
    got_b = bits[:n].cpu().numpy().view(np.uint32)
    want_b = R.fill_bits(R.STREAM_SEED, R.STREAM_ID, 0, n)
    np.testing.assert_array_equal(got_b, want_b)
    x = nrm[:n].cpu().numpy().astype(np.float64)
    ref = R.normals(want_b.reshape(-1, 4)).reshape(-1)
    err = float(np.abs(x - ref).max())
    b_mean, b_var, b_ks = R.moment_bounds(n)
    mean, var, ks = float(x.mean()), float(x.var()), R.kolmogorov_distance(x)
    print("2^20 normals of seed %d: max |fp32 - float64| = %.2e; mean %.3e (bound %.3e), var - 1 %.3e (%.3e), Kolmogorov distance %.3e (%.3e)"
          % (R.STREAM_SEED, err, mean, b_mean, var - 1, b_var, ks, b_ks))
    assert err <= NORMAL_TOL, err
    assert abs(mean) <= b_mean and abs(var - 1) <= b_var and ks <= b_ks
    # a ragged fill from an odd element: the matching slice of the long one, and not one element more
    first, m = 4097, 1001
    for kind, long_t, dt, fillv in ((_lib.RNG_BITS, bits, torch.int32, 0x5A5A5A5A), (_lib.RNG_NORMAL, nrm, torch.float32, 9.0)):
        part = torch.full((m + pad,), fillv, device="cuda", dtype=dt)
        h.rng_fill(R.STREAM_SEED, R.STREAM_ID, first, kind, part.data_ptr(), m)
        torch.cuda.synchronize()
        assert torch.equal(part[:m], long_t[first:first + m]) and (part[m:] == fillv).all(), kind
    # elements beyond 2^32 blocks: the high counter word
    far = torch.zeros(12, device="cuda", dtype=torch.int32)
    h.rng_fill(SEED, 1, (1 << 34) + 2, _lib.RNG_BITS, far.data_ptr(), 12)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(far.cpu().numpy().view(np.uint32), R.fill_bits(SEED, 1, (1 << 34) + 2, 12))
    h.close()


# ---- 2. fused equals explicit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("posterior", [1, 0], ids=["posterior", "prior"])
def test_forward_with_null_eps_equals_forward_on_the_filled_eps(torch_cuda, posterior):
    torch = torch_cuda
    d = small_dims(n_scenes=3, mno=8, K=3, T_obs=4, T_pred=6, posterior=posterior)
    w = init_weights(d, 9)
    past, fut, _, grids, gos = make_case(d, seed=5, n_absent=2)
    draw = 5
    a, b = handle(torch, d, w, grids, gos), handle(torch, d, w, grids, gos)
    a.set_rng(SEED, draw)
    Ya, sa = forward(torch, a, past, fut)
    assert a.rng_state() == (draw + 1, draw)
    eps = latent_eps(torch, b, SEED, draw)
    ref = R.latent_eps(SEED, draw, d.n_scenes, d.K, d.mno, d.L).reshape(d.R, d.L)
    err = float(np.abs(eps.cpu().numpy().astype(np.float64) - ref).max())
    print("latent fill against the restatement: max |eps - float64| = %.2e" % err)
    assert err <= NORMAL_TOL, err
    Yb, sb = forward(torch, b, past, fut, eps)
    np.testing.assert_array_equal(a.read_buffer("z", (d.R, d.L)), b.read_buffer("z", (d.R, d.L)))
    np.testing.assert_array_equal(Ya, Yb)
    np.testing.assert_array_equal(sa, sb)
    assert np.isfinite(Ya).all() and np.abs(Ya - 7.0).min() > 0
    a.close(); b.close()


# ---- 3. compaction --------------------------------------------------------------------------------------------------------------------------------
def present_of(past):
    return past[:, -1, :, 0] != 0


def compact_rows_of(d, present):
    """Full row index of every compact row r' = k * P + a' (kernels_compact.hip)."""
    agents = np.nonzero(present.reshape(-1))[0]
    sc, slot = agents // d.mno, agents % d.mno
    return np.concatenate([(sc * d.K + k) * d.mno + slot for k in range(d.K)])


@pytest.mark.parametrize("case", ["n_absent", "ragged"])
def test_compacted_and_padded_handles_draw_the_same_noise(torch_cuda, case):
    torch = torch_cuda
    from tests.test_gpu_compact_rows import ragged_case, row_mask
    d = small_dims(n_scenes=3, mno=8, K=3, T_obs=4, T_pred=6)
    w = init_weights(d, 9)
    if case == "n_absent":
        past, fut, _, grids, gos = make_case(d, seed=6, n_absent=3)
    else:
        past, fut, _, grids, gos, _ = ragged_case(d, seed=6, keep=0.5)
    present = present_of(past)
    assert 0 < present.sum() < d.A
    out = {}
    for name, flags in (("padded", 0), ("compact", FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC)):
        h = handle(torch, d.replace(flags=flags), w, grids, gos)
        h.set_rng(SEED, 2)
        forward(torch, h, past, fut)
        out[name] = (h.read_buffer("Y0", (d.R, d.T_pred, 2)), h.read_buffer("z", (d.R, d.L)))
        h.close()
    m = row_mask(d, present)
    np.testing.assert_array_equal(out["compact"][0][m], out["padded"][0][m])
    assert not out["compact"][0][~m].any()
    rows = compact_rows_of(d, present)
    np.testing.assert_array_equal(out["compact"][1][: rows.size], out["padded"][1][rows])


# ---- 4. several trips of the stride loop ------------------------------------------------------------------------------------------------------------
def test_a_graph_baked_with_a_stale_count_hint_draws_the_same_noise(torch_cuda):
    torch = torch_cuda
    from tests import test_gpu_count_hint as CH
    d = small_dims(n_scenes=24, mno=32, K=3, T_obs=4, T_pred=6, n_grids=1).replace(flags=FLAG_COMPACT_ROWS | FLAG_COMPACT_IOC)
    batches, grids, gos = CH.make_batches(d)
    keep = batches["big"][3]
    CH.check_preconditions(d, int(keep.sum()))
    # k_reparam_c_rng itself: 8192 workgroups of 256 lanes at most, one lane per four latents -- the crowded batch below fits one trip of ITS loop; the
    # trips here are those of the kernels downstream, which read z by compact row
    w = init_weights(d, 9)
    draw = 11

    class Session(CH.Session):
        def forward(self):
            self.h.forward(self.p.data_ptr(), self.f.data_ptr(), 0, self.Y.data_ptr(), self.sc.data_ptr(), self.sp)

    s = Session(torch, d, w, batches, grids, gos)
    s.h.set_rng(SEED, 0, s.sp)
    s.direct("big"); s.direct("one")                    # lazy allocations outside capture; the count word now holds 1
    g = s.capture()                                     # baked with hint = 1
    s.h.set_rng(SEED, draw, s.sp)
    got = s.replay(g, "big")
    assert s.h.rng_state(s.sp) == (draw + 1, draw)
    past, fut, _, _ = batches["big"]
    ref_h = handle(torch, d.replace(flags=0), w, grids, gos)
    ref_h.set_rng(SEED, draw)
    Y, sc = forward(torch, ref_h, past, fut)
    ref = dict(Y0=ref_h.read_buffer("Y0", (d.R, d.T_pred, 2)), Hx=ref_h.read_buffer("Hx", (d.A, d.H)), Hy=ref_h.read_buffer("Hy", (d.A, d.H)),
               Y=Y, score=sc)
    CH.check(d, got, ref, keep, "graph (hint 1) on 'big', generated eps")
    s.h.close(); ref_h.close()


# ---- 5. cut independence ------------------------------------------------------------------------------------------------------------------------------
def test_a_windows_noise_does_not_depend_on_the_batch_cut(torch_cuda):
    torch = torch_cuda
    d4 = small_dims(n_scenes=4, mno=8, K=3, T_obs=4, T_pred=6)
    d2 = d4.replace(n_scenes=2)
    w = init_weights(d4, 9)
    past, fut, _, grids, gos = make_case(d4, seed=7, n_absent=2)
    h4 = handle(torch, d4, w, grids, gos)
    h4.set_rng(SEED, 3)
    forward(torch, h4, past, fut)
    whole = h4.read_buffer("Y0", (d4.R, d4.T_pred, 2)).reshape(4, -1)
    h4.close()
    for base in (0, 2):
        h2 = handle(torch, d2, w, grids, gos[base:base + 2])
        h2.set_rng(SEED, 3)
        h2.set_rng_origin(base, 0)
        forward(torch, h2, past[base:base + 2], fut[base:base + 2])
        np.testing.assert_array_equal(h2.read_buffer("Y0", (d2.R, d2.T_pred, 2)).reshape(2, -1), whole[base:base + 2], err_msg="scene_base %d" % base)
        h2.close()
    assert not np.array_equal(whole[0], whole[2])


def test_a_slot_shard_draws_the_noise_of_its_global_slots(torch_cuda):
    """Prior mode, so that "z" is the noise itself and the comparison says nothing about the encoders of two handle shapes."""
    torch = torch_cuda
    d32 = small_dims(n_scenes=2, mno=32, K=3, T_obs=4, T_pred=6, posterior=0)
    d16 = d32.replace(mno=16)
    w = init_weights(d32, 9)
    past, fut, _, grids, gos = make_case(d32, seed=8, n_absent=0)
    h32 = handle(torch, d32, w, grids, gos)
    h32.set_rng(SEED, 4)
    forward(torch, h32, past, fut)
    z32 = h32.read_buffer("z", (d32.R, d32.L)).reshape(2, 3, 32, d32.L)
    h32.close()
    h16 = handle(torch, d16, w, grids, gos)
    h16.set_rng(SEED, 4)
    h16.set_rng_origin(0, 16)
    forward(torch, h16, past[:, :, 16:], fut[:, :, 16:])
    z16 = h16.read_buffer("z", (d16.R, d16.L)).reshape(2, 3, 16, d16.L)
    h16.close()
    np.testing.assert_array_equal(z16, z32[:, :, 16:])
    assert not np.array_equal(z16, z32[:, :, :16])


# ---- 6. graph replay --------------------------------------------------------------------------------------------------------------------------------------
def test_a_replayed_graph_draws_fresh_noise_and_a_reseed_replays_it(torch_cuda):
    torch = torch_cuda
    d = small_dims(n_scenes=3, mno=8, K=3, T_obs=4, T_pred=6)
    w = init_weights(d, 9)
    past, fut, _, grids, gos = make_case(d, seed=5, n_absent=2)
    h = handle(torch, d, w, grids, gos)
    side = torch.cuda.Stream(); sp = side.cuda_stream
    p_t, f_t = dev(torch, past), dev(torch, fut)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
    run = lambda: h.forward(p_t.data_ptr(), f_t.data_ptr(), 0, Y.data_ptr(), sc.data_ptr(), sp)
    draw0 = 20
    h.set_rng(SEED, 0, sp)                              # (allocates the words: before the capture)
    run(); side.synchronize()                           # lazy allocations outside capture
    h.graph_begin(sp)
    run()
    g = h.graph_end(sp)

    def replays(k):
        out = []
        for _ in range(k):
            h.graph_launch(g, sp)
            side.synchronize()
            out.append((Y.cpu().numpy().copy(), sc.cpu().numpy().copy()))
        return out

    h.set_rng(SEED, draw0, sp)
    first = replays(2)
    assert h.rng_state(sp) == (draw0 + 2, draw0 + 1)
    assert not np.array_equal(first[0][0], first[1][0])
    h.set_rng(SEED, draw0, sp)
    again = replays(2)
    for (Ya, sa), (Yb, sb) in zip(first, again):
        np.testing.assert_array_equal(Ya, Yb)
        np.testing.assert_array_equal(sa, sb)
    h.close()


# ---- 7. training -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, FLAG_COMPACT_ROWS], ids=["padded", "compact_rows"])
def test_a_training_step_keeps_no_eps(torch_cuda, flags):
    torch = torch_cuda
    from tests.stage_reference import spread_weights
    d = small_dims(n_scenes=2, mno=16, K=3, T_obs=5, T_pred=6, n_grids=1).replace(flags=flags)      # the smallest training shape of tests/test_gpu_train.py
    w = spread_weights(init_weights(d, 41))
    past, fut, _, grids, gos = make_case(d, seed=42, n_absent=4)
    p_t, f_t = dev(torch, past), dev(torch, fut)
    draw = 9

    def step(generated):
        h = handle(torch, d, w, grids, gos)
        h.set_training(True)
        Y = torch.zeros((d.R, d.T_pred, 2), device="cuda"); sc = torch.zeros((d.R,), device="cuda")
        if generated:
            h.set_rng(SEED, draw)
            e_ptr, e = 0, None
        else:
            e = latent_eps(torch, h, SEED, draw)
            e_ptr = e.data_ptr()
        h.forward(p_t.data_ptr(), f_t.data_ptr(), e_ptr, Y.data_ptr(), sc.data_ptr())
        h.backward(p_t.data_ptr(), f_t.data_ptr(), e_ptr)
        torch.cuda.synchronize()
        state = h.rng_state() if generated else None
        g = h.grad_tensor().clone().cpu().numpy()
        h.close()
        return g, Y.cpu().numpy(), state

    ga, Ya, state = step(True)
    gb, Yb, _ = step(False)
    assert state == (draw + 1, draw), state             # one draw for the forward, none for the backward
    assert np.isfinite(ga).all() and np.abs(ga).max() > 0
    np.testing.assert_array_equal(Ya, Yb)
    np.testing.assert_array_equal(ga, gb)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_null_eps_needs_the_generator_and_dims_must_fit_the_packing(torch_cuda):
    torch = torch_cuda
    from desire_amd import _lib
    d = small_dims(n_scenes=1, mno=8, K=2, T_obs=4, T_pred=6, posterior=0)
    w = init_weights(d, 9)
    past, fut, _, grids, gos = make_case(d, seed=5, n_absent=2)
    h = handle(torch, d, w, grids, gos)
    with pytest.raises(_lib.DesireError, match="error -1"):
        forward(torch, h, past, fut)                    # NULL eps before desire_set_rng: DESIRE_ERR_ARG, as ever
    with pytest.raises(_lib.DesireError, match="error -2"):
        h.rng_state()
    with pytest.raises(_lib.DesireError, match="error -1"):
        h.set_rng_origin(0, R.MAX_SLOT - d.mno + 1)
    h.set_rng_origin(0, R.MAX_SLOT - d.mno)
    h.set_rng(SEED, 0)
    forward(torch, h, past, fut)
    z = h.read_buffer("z", (d.R, d.L)).astype(np.float64)
    ref = R.latent_eps(SEED, 0, d.n_scenes, d.K, d.mno, d.L, slot_base=R.MAX_SLOT - d.mno).reshape(d.R, d.L)
    assert np.abs(z - ref).max() <= NORMAL_TOL              # the largest slot the packing holds
    h.close()
    for kw in (dict(L=R.MAX_L + 8), dict(K=R.MAX_K)):
        hb = _lib.Handle(small_dims(**{**dict(n_scenes=1, mno=1, K=1, T_obs=4, T_pred=6, L=8), **kw}))
        with pytest.raises(_lib.DesireError, match="error -1"):
            hb.set_rng(SEED, 0)
        e = torch.zeros(16, device="cuda")
        with pytest.raises(_lib.DesireError, match="error -1"):
            hb.rng_fill(SEED, 0, 0, _lib.RNG_LATENT, e.data_ptr(), 16)
        hb.close()
    ok = _lib.Handle(small_dims(n_scenes=1, mno=1, K=1, T_obs=4, T_pred=6, L=R.MAX_L))
    ok.set_rng(SEED, 0)                                 # L = 4096 fits
    ok.close()
