"""Are the inputs of tests/test_gpu_stage_isolation.py able to see a wrong kernel?  Oracle only, no GPU.

For every case the tolerance check_stage would apply to each stage is computed from the fp32 and float64 oracle (the fp32 oracle's chain
stands in for the GPU's buffers), and every mutant below -- the mistakes a kernel of that stage can make and still look plausible -- must move
the compared buffer of its stage by at least FACTOR tolerances.  FACTOR is a condition on the cases, not a measurement: a case that misses it
gets another seed or other spread_weights factors."""
import numpy as np
import pytest

from oracle import desire_oracle as O
from tests import stage_reference as SR

FACTOR = 100.0
F32 = np.float32


@pytest.fixture(scope="module", params=[c[0] for c in SR.CASES])
def ctx(request):
    case = SR.get_case(request.param)
    d, w = case.d, case.w
    buf = case.forward(F32)
    inp = case.inputs(buf)
    tol = {}
    for st in SR.stages_of(d):
        tol.update(SR.stage_tolerance(st, inp, w, d)[1])
    return case, buf, inp, tol


def moved(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64).reshape(np.shape(a))).max())


def test_margin_is_final():
    assert SR.MARGIN <= 16 and not SR.COLLECT_ONLY


def test_a_sample_that_repeats_its_neighbour_is_seen(ctx):
    """z of the last sample taken from sample K - 2 of the same agent: z, xz and Y0 move."""
    case, buf, inp, tol = ctx
    d, w = case.d, case.w
    if d.K == 1:
        pytest.skip("one sample per agent")
    z = buf["z"].reshape(d.n_scenes, d.K, d.mno, d.L).copy()
    z[:, d.K - 1] = z[:, d.K - 2]
    z = z.reshape(d.R, d.L)
    xz = SR.stage("mask").eval(dict(inp, xhat=O.vae_decoder(z, w)), w, d, F32)["xz"]
    Y0 = SR.stage("decoder").eval(dict(inp, xz=xz), w, d, F32)["Y0"]
    for name, got in (("z", z), ("xz", xz), ("Y0", Y0)):
        assert moved(buf[name], got) >= FACTOR * tol[name], (name, moved(buf[name], got), tol[name])


def test_the_masked_input_reaches_the_decoder(ctx):
    case, buf, inp, tol = ctx
    Y0 = SR.stage("decoder").eval(dict(inp, xz=np.zeros_like(buf["xz"])), case.w, case.d, F32)["Y0"]
    assert moved(buf["Y0"], Y0) >= FACTOR * tol["Y0"], (moved(buf["Y0"], Y0), tol["Y0"])


LAYERS = [("conv1", "vae_enc", 2), ("conv2", "vae_enc", 2), ("conv3", "vae_enc", 2), ("deconv1", "vae_dec", 3), ("deconv2", "vae_dec", 3),
          ("deconv3", "vae_dec", 3), ("deconv4", "vae_dec", 3)]            # (stage, weight scope, axis of the input channel in the kernel)


def _layer_mutants():
    for name, scope, cin in LAYERS:
        if name != "conv1":
            for tap in ([(3, 3)] if name == "deconv1" else [(0, 0), (4, 4)]):
                yield name, scope, cin, tap
        yield name, scope, cin, None


@pytest.mark.parametrize("name,scope,cin,tap", list(_layer_mutants()), ids=lambda v: str(v).replace(" ", ""))
def test_a_dropped_tap_or_input_channel_moves_its_layer(ctx, name, scope, cin, tap):
    """tap given: that kernel tap zeroed; tap None: the last input channel dropped."""
    case, buf, inp, tol = ctx
    d = case.d
    st = SR.stage(name)
    if st.posterior_only and not d.posterior:
        pytest.skip("prior sampling runs no encoder")
    key = "%s/%s/w" % (scope, name)
    k = case.w[key].copy()
    if tap is not None:
        k[tap[0], tap[1]] = 0
    elif cin == 2:
        k[:, :, -1, :] = 0
    else:
        k[:, :, :, -1] = 0
    out = st.outputs[0]
    got = st.eval(inp, dict(case.w, **{key: k}), d, F32)[out]
    assert moved(buf[out], got) >= FACTOR * tol[out], (name, tap, moved(buf[out], got), tol[out])


def test_the_last_row_and_the_last_agent_are_seen(ctx):
    """Every stage output with its last row (per-row stages: R - 1, per-agent stages: A - 1) zeroed."""
    case, buf, inp, tol = ctx
    d = case.d
    for st in SR.stages_of(d):
        for out in st.outputs:
            x = np.asarray(buf[out])
            assert x.shape[0] == (d.A if st.per_agent else d.R)
            m = float(np.abs(x[-1]).max())
            assert m >= FACTOR * tol[out], (st.name, out, m, tol[out])


def _ioc_moves(ctx, w=None, **changed):
    case, buf, inp, tol = ctx
    got = SR.stage("ioc").eval(dict(inp, **changed), w or case.w, case.d, F32)
    for out in ("Y", "score"):
        assert moved(buf[out], got[out]) >= FACTOR * tol[out], (out, moved(buf[out], got[out]), tol[out])


def test_the_velocity_embedding_reaches_the_ioc_outputs(ctx):
    case = ctx[0]
    _ioc_moves(ctx, w=dict(case.w, **{"ioc/vel_fc/w": np.zeros_like(case.w["ioc/vel_fc/w"])}))


def test_the_neighbours_reach_the_ioc_outputs(ctx):
    case = ctx[0]
    if case.d.mno == 1:
        pytest.skip("lone agents have no neighbour to remove")
    _ioc_moves(ctx, valid=np.zeros_like(case.valid))


def test_the_scene_grids_reach_the_ioc_outputs(ctx):
    _ioc_moves(ctx, grids=np.zeros_like(ctx[0].grids))
