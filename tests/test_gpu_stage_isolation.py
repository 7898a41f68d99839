"""Every kernel stage of the forward against the float64 oracle of that ONE stage, evaluated on the inputs the GPU itself produced, on
weights that make the K samples of an agent differ (tests/stage_reference.py holds the stage table, the tolerance rule and the cases).

Per case: one handle, one forward, every stage buffer read back, check_stage per stage.  The IOC stage is the forward's own refinement of
the GPU's Y0: its references take that very array, the library's cells and bins of it are asserted equal to the oracle's, and the stage
is never skipped (O.bin_margin / O.cell_margin > 1e-5 is asserted where a seed with that property exists: stage_reference.CASES).
Then: the K rows of an agent are pairwise different in z, xz and Y0 by 100 tolerances, and (fp32-class forms) Y0 sits within
MARGIN fp32-oracle roundings of the float64 oracle run from the raw inputs."""
import numpy as np
import pytest

from tests import stage_reference as SR
from tests.test_gpu_parity import run_gpu, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

REPORT = []          # (case, form, stage, output, rule, err, yardstick, ratio): printed by the last test (pytest -s)

PARAMS = [(c[0], form) for form in SR.FORMS for c in (SR.CASES if form == "fp32" else SR.CASES[:SR.N_FORM_CASES])]


def assert_cells_and_bins_are_the_oracles(torch, h, case, Y0):
    """The library's scene cells and social bins of these positions equal the oracle's bit for bit: the IOC stage and its references then
    look up the same cells and pool the same neighbours, however close a position lies to an edge."""
    from oracle import desire_oracle as O
    d = case.d
    P, V = case.groups(Y0)
    pos_t = torch.as_tensor(P, device="cuda")
    val_t = torch.as_tensor(V.astype(np.uint8), device="cuda")
    bins_t = torch.full((len(P), d.mno, d.mno), -7, dtype=torch.int32, device="cuda")
    cells_t = torch.full((P.size // 2, 2), -7, dtype=torch.int32, device="cuda")
    h.neighbor_bins(pos_t.data_ptr(), val_t.data_ptr(), bins_t.data_ptr(), len(P))
    h.scene_cells(pos_t.data_ptr(), cells_t.data_ptr(), P.size // 2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bins_t.cpu().numpy(), O.neighbor_bins(P, V, d.nb_w, d.nb_h, d.grid_size))
    cy, cx = O.scene_cell(P.reshape(-1, 2), d.Gh, d.Gw)
    np.testing.assert_array_equal(cells_t.cpu().numpy(), np.stack([cy, cx], -1))


def run_form(torch, d, training, w, raw):
    past, fut, eps, grids, gos = raw
    if not training:
        return run_gpu(torch, d, w, past, fut, eps, grids, gos)
    from desire_amd import _lib
    h = _lib.Handle(d)
    h.set_weights(w)
    h.set_training(True)                                  # the forward that keeps the saves of the backward pass
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    past_t, fut_t, eps_t, grids_t = t(past), t(fut), t(eps), t(grids)
    h.set_scene_grids(grids_t.data_ptr(), gos)
    Y = torch.zeros((d.R, d.T_pred, 2), device="cuda")
    score = torch.zeros((d.R,), device="cuda")
    h.forward(past_t.data_ptr(), fut_t.data_ptr(), eps_t.data_ptr(), Y.data_ptr(), score.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return h, Y.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("cid,form", PARAMS)
def test_every_stage_against_its_own_float64_reference(torch_cuda, cid, form):
    case = SR.get_case(cid)
    d, w = case.d, case.w
    over, training, two_piece_stages = SR.FORMS[form]
    h, Y, score = run_form(torch_cuda, d.replace(**over), training, w, case.raw)
    buf = {name: h.read_buffer(name, shp) for name, shp in SR.buffer_shapes(d).items()}
    buf["Y"], buf["score"] = Y, score
    assert_cells_and_bins_are_the_oracles(torch_cuda, h, case, buf["Y0"])
    h.close()
    bm, cm = case.margins(buf["Y0"])
    print("%-10s %-8s bin margin %.2e cell margin %.2e" % (cid, form, bm, cm))
    if case.margins_hold:                                  # (where a seed with both margins exists; stage_reference.CASES says why not everywhere)
        assert bm > 1e-5 and cm > 1e-5, (bm, cm)
    inp = case.inputs(buf)
    tol, failures = {}, []
    for st in SR.stages_of(d):
        rule2 = st.name in two_piece_stages
        try:
            SR.check_stage(st, inp, buf, w, d, two_piece_rule=rule2, report=REPORT)
        except AssertionError as e:
            failures.append(str(e))
        tol[st.name] = SR.stage_tolerance(st, inp, w, d, rule2)[1]
    for r in REPORT[-sum(len(s.outputs) for s in SR.stages_of(d)):]:
        print("%-10s %-8s %-8s -> %-14s %-4s err %.3e yard %.3e ratio %.2f" % ((cid, form) + r))
    # sample identity: a sampler that fed every k the same eps, or a row map that lost k, gives identical rows.  (Measured in the fp32-rule
    # tolerance of the stage in every form: the two-piece tolerance of the decoder is ~1e-4 and no spread puts every pair 100 of those apart.)
    if d.K > 1:
        for name, st in (("z", "reparam"), ("xz", "mask"), ("Y0", "decoder")):
            dist, t32 = SR.min_pair_distance(buf[name], d), SR.stage_tolerance(SR.stage(st), inp, w, d)[1][name]
            if not dist > 100 * t32:
                failures.append("the K rows of %s are not pairwise different: min pair distance %.3e <= 100 x %.3e" % (name, dist, t32))
    # whole chain, fp32-class forms: from the raw inputs, measured in the fp32 oracle's own distance from float64
    if not two_piece_stages:
        r64, r32 = case.forward(np.float64)["Y0"], case.forward(np.float32)["Y0"]
        yard = float(np.abs(r32 - r64).max())
        err = float(np.abs(buf["Y0"] - r64).max())
        REPORT.append(("chain", "Y0", "fp32", err, yard, err / yard))
        print("%-10s %-8s whole chain Y0: err %.3e yard %.3e ratio %.2f" % (cid, form, err, yard, err / yard))
        if not SR.COLLECT_ONLY and not err <= SR.MARGIN * yard:
            failures.append("whole chain: |Y0 - float64| = %.3e > %g x %.3e" % (err, SR.MARGIN, yard))
    assert not failures, "\n".join(failures)


def test_report_largest_ratio_per_stage():
    """The table of tests/stage_reference.py's docstring: the largest ratio per stage and rule over what ran above (pytest -s shows it)."""
    worst = {}
    for st, out, rule, err, yard, ratio in REPORT:
        worst[(st, out, rule)] = max(worst.get((st, out, rule), 0.0), ratio)
    for (st, out, rule), r in worst.items():
        print("RATIO %-8s -> %-14s %-4s %.2f" % (st, out, rule, r))
    for (st, out, rule), r in worst.items():
        assert SR.COLLECT_ONLY or r <= (SR.MARGIN2 if rule == "2p" else SR.MARGIN), (st, out, rule, r)
