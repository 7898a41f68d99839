"""What is checkable without a GPU about the selection of distinct joint futures (desire_select_worlds): the two numpy statements of the contract
(tests/worlds_reference.py) agree on order and count on the generator's inputs, which keep the stated margin by themselves; the anchors that pin
the contract to desire_select_diverse (one slot) and to desire_joint_metrics' order (radius 0); and a host-compiled sweep of the kernel's LDS
plan (desire_amd/csrc/eval_lds.h: WorldsLds, worlds_geometry): every accepted shape fits the budget, and the documented limit is the true one."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import small_dims
from tests.joint_reference import joint_f32, make_inputs as joint_inputs, planted_joint_scores
from tests.rank_reference import rank_order
from tests.select_reference import DIST_FINAL, DIST_MAX, DIST_MEAN, METRICS, select_f32
from tests.worlds_reference import (MARGIN, RADIUS_PX, REDUCES, SHAPES, WORLD_ALL, WORLD_MEAN, cases_of, make_inputs, planted_world_scores,
                                    worlds_f32, worlds_f64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dims(shape, **kw):
    n, m, K, T = shape
    return small_dims(n_scenes=n, mno=m, K=K, T_obs=4, T_pred=T, n_grids=1, H=64, **kw)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_K%d_T%d" % s)
def test_the_two_statements_agree_and_the_generator_keeps_the_margin(shape):
    d = _dims(shape)
    ux, uy, radius = 1.0 / d.sx, 1.0 / d.sy, RADIUS_PX
    Y, present, info = make_inputs(d, radius, ux, uy, seed=5)
    ws = planted_world_scores(d, 6)
    kept, worlds = 0, 0
    for metric, reduce, t_end in cases_of(d):
        f64 = worlds_f64(Y, present, ws, metric, reduce, t_end, radius, ux, uy, d)
        assert f64["margin"] > MARGIN, (metric, reduce, t_end, f64["margin"])      # the float64 pass alone
        f32 = worlds_f32(Y, present, ws, metric, reduce, t_end, radius, ux, uy, d)
        for key in ("order", "count", "label"):
            np.testing.assert_array_equal(f32[key], f64[key], err_msg="%s %s" % (key, (metric, reduce, t_end)))
        np.testing.assert_allclose(f32["mass"], f64["mass"], rtol=0, atol=1e-5)
        assert (np.sort(f32["order"], 1) == np.arange(d.K)).all() and (f32["count"] >= 1).all()
        if d.K >= 3:
            assert (f32["count"][:-1] < d.K).all()                                 # every case suppresses something
        assert (f32["count"][-1] == 1) if d.n_scenes >= 2 else True                # nobody present: everything is near the first
        w, k, _ = info["nan"]
        assert f32["order"][w, :f32["count"][w]].tolist().count(k) == 1            # the world with a NaN row is near nothing: kept
        kept += int(f32["count"].sum()); worlds += d.n_scenes * d.K
    print("shape %s: %.0f %% of the worlds kept" % (shape, 100.0 * kept / worlds))


def test_one_slot_is_the_per_agent_selection():
    """mno = 1, the slot present, DESIRE_WORLD_ALL: order, count and mass are select_f32's given the order by score and the same scores."""
    d = _dims((3, 1, 3, 7))
    ux, uy, radius = 1.0 / d.sx, 1.0 / d.sy, RADIUS_PX
    Y, _, _ = make_inputs(d, radius, ux, uy, seed=7)
    Y = np.nan_to_num(Y, nan=0.25)
    s = planted_world_scores(d, 8)                                                 # [n, K] = [n, K, mno] at one slot
    order = rank_order(s.reshape(d.n_scenes, d.K, 1), d)
    for scores in (s, None):
        for metric in METRICS:
            for t_end in (1, 4, d.T_pred):
                ref = select_f32(Y, order if scores is not None else np.tile(np.arange(d.K), (d.A, 1)), scores, metric, t_end, radius, ux, uy, d)
                got = worlds_f32(Y, None, scores, metric, WORLD_ALL, t_end, radius, ux, uy, d)
                np.testing.assert_array_equal(got["order"], ref["order"])
                np.testing.assert_array_equal(got["count"], ref["count"])
                np.testing.assert_array_equal(got["mass"].view(np.uint32), ref["mass"].view(np.uint32))


def test_radius_zero_is_the_joint_order():
    d = _dims((2, 8, 5, 12))
    ux, uy = 1.0 / d.sx, 1.0 / d.sy
    Y, fut, present, _ = joint_inputs(d, RADIUS_PX, ux, uy, seed=3)
    s = planted_joint_scores(d, 4)
    jm = joint_f32(Y, None, present, s, [d.T_pred], 1, 0.0, ux, uy, d)
    for metric, reduce in itertools.product(METRICS, REDUCES):
        got = worlds_f32(Y, present, jm["jscore"], metric, reduce, d.T_pred, 0.0, ux, uy, d)
        np.testing.assert_array_equal(got["order"], jm["order"])
        np.testing.assert_array_equal(got["count"], d.K)
        np.testing.assert_array_equal(got["label"], np.argsort(jm["order"], 1))


# ---- the LDS plan, compiled for the host (no ROCm header, no GPU)
DRIVER_SRC = r"""
#include <cstdio>
#include "eval_lds.h"
int main() {
    int m, K, metric, te;
    while (std::scanf("%d %d %d %d", &m, &K, &metric, &te) == 4) {
        int SC = 0;
        const bool ok = worlds_geometry(m, K, metric, te, &SC);
        const int F = SelLds::staged(metric, te);
        const WorldsLds L(F, ok ? SC : 1, K, m);
        // ok, SC, bytes, the end of the last region in bytes, the smallest plan (one slot), the dv stride
        std::printf("%d %d %zu %zu %zu %d\n", ok ? 1 : 0, SC, L.bytes(), L.pairs() * EVAL_PAIR_BYTES + 4 * (L.slots() + (size_t)m),
                    WorldsLds(F, 1, K, m).bytes(), L.dv_stride());
    }
    std::printf("%d %d\n", EVAL_LDS_BYTES, EVAL_THREADS);
    return 0;
}
"""
MNO = [1, 4, 8, 31, 32, 33, 96, 160, 256]
KS = [1, 2, 3, 20, 70, 130, 176, 1300, 1336, 1337, 4096]
TS = [1, 5, 7, 40, 200, 3800, 7680]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("worlds_lds")
    src, exe = str(tmp / "worlds_lds_driver.cpp"), str(tmp / "worlds_lds_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER_SRC)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def ask(shapes):
        r = subprocess.run([exe], input="".join("%d %d %d %d\n" % s for s in shapes), capture_output=True, text=True, check=True)
        rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(rows) == len(shapes) + 1 and rows[-1] == (60 * 1024, 256)
        return rows[:-1]
    return ask


def test_the_lds_plan_fits_and_its_limit_is_the_documented_one(plan):
    budget = 60 * 1024
    shapes = [(m, K, metric, te) for m, K, T in itertools.product(MNO, KS, TS) for metric in (DIST_FINAL, DIST_MEAN, DIST_MAX)
              for te in sorted({1, max(1, T // 2), T})]
    for (m, K, metric, te), (ok, SC, nbytes, end, smallest, stride) in zip(shapes, plan(shapes)):
        frames = 1 if metric == DIST_FINAL else te
        assert smallest == 44 * K + 4 * m + 8 * (frames | 1)                       # the limit desire_hip.h and the API's message state
        assert bool(ok) == (smallest <= budget), (m, K, metric, te)
        if not ok:
            continue
        assert nbytes == end <= budget, (m, K, metric, te)                         # the regions end where bytes() says
        chunks = -(-m // SC)
        assert 1 <= SC <= m and (chunks - 1) * SC < m and stride == SC | 1, (m, K, metric, te, SC)
    # every (mno <= 256, T_pred <= 200) of a handle at any K <= 176 is served, K up to 1300 too; the headline's window is one chunk
    for (ok, SC, nbytes, _, _, _), want in zip(plan([(256, 176, DIST_MEAN, 200), (256, 1300, DIST_MAX, 200), (32, 20, DIST_MEAN, 40), (256, 2, DIST_MEAN, 40)]),
                                               [22, 1, 32, 128]):
        assert ok and SC == want and nbytes <= budget
