"""The LDS plans and geometries of the evaluation kernels over the sample tensor (desire_amd/csrc/eval_lds.h: k_sample_errors, k_kde_nll,
k_select_diverse, k_recon_weights, k_joint_unit).  tests/c_host/eval_lds_driver.cpp is compiled against the header with g++ -- no ROCm header, no
GPU.  A sweep holds every accepted plan to the budget and to a cover of the slots and samples, every refusal to `the smallest plan does not fit`;
a table pins the documented cases to the values the geometry functions gave when they still lived in the kernel files."""
import itertools
import os
import shutil
import subprocess

import pytest

from tests.joint_reference import chunk_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "eval_lds_driver.cpp")
MNO = [1, 4, 8, 31, 32, 33, 96, 160, 256]
KS = [1, 2, 3, 20, 24, 25, 70, 130, 4096]
TS = [1, 5, 7, 40, 200, 3800, 3900, 7680, 7681]
FINAL, MEAN, MAX = 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("eval_lds") / "eval_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, reqs):
    """One driver process for all requests: a list of int tuples (ok, a, b, bytes, end, smallest)."""
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs)
    return rows


@pytest.fixture(scope="module")
def budget(driver):
    (lds, threads), = ask(driver, ["budget"])
    assert lds == 60 * 1024 and threads == 256
    return lds


def covers(n, per):
    """Chunks of `per` cover 0 .. n-1 exactly once with no empty chunk."""
    chunks = -(-n // per)
    return per >= 1 and (chunks - 1) * per < n <= chunks * per


def test_sweep_errors(driver, budget):
    shapes = list(itertools.product(MNO, KS, TS))
    for (m, K, T), (ok, SC, KC, nbytes, end, smallest) in zip(shapes, ask(driver, ["errors %d %d %d" % s for s in shapes])):
        assert smallest == 4 * (T | 1) * 4                                     # one slot's mask and targets, one row of errors
        if not ok:
            assert smallest > budget, (m, K, T)
            continue
        assert nbytes == end <= budget and smallest <= budget, (m, K, T)
        assert covers(m, SC) and covers(K, KC) and SC * KC <= 256, (m, K, T, SC, KC)


def test_sweep_kde(driver, budget):
    for T, (ok, SA, _, nbytes, end, smallest) in zip(TS, ask(driver, ["kde %d" % T for T in TS])):
        if not ok:
            assert smallest > budget, T
            continue
        assert smallest == 8 * (T | 1) <= budget and nbytes == end == SA * smallest <= budget, (T, SA)
        assert SA == max(1, 256 // T), (T, SA)                                  # as many whole agents as 256 (agent, t) pairs hold, one beyond


def test_sweep_select(driver, budget):
    shapes = [(m, K, metric, te) for m, K, T in itertools.product(MNO, KS, TS) for metric in (FINAL, MEAN, MAX) for te in sorted({1, max(1, T // 2), T})]
    for (m, K, metric, te), (ok, SC, G, nbytes, end, smallest) in zip(shapes, ask(driver, ["select %d %d %d %d" % s for s in shapes])):
        frames = 1 if metric == FINAL else te
        assert smallest == K * (8 * (frames | 1) + 20) + 8                      # the limit desire_hip.h and the API's message state
        if not ok:
            assert smallest > budget, (m, K, metric, te)
            continue
        assert nbytes == end == SC * smallest <= budget, (m, K, metric, te)
        assert covers(m, SC) and SC <= max(1, 512 // G), (m, K, metric, te, SC)
        assert G & (G - 1) == 0 and min(K, 64) <= G <= 64, (K, G)


def test_sweep_recon(driver, budget):
    shapes = list(itertools.product(MNO, KS, TS))
    for (m, K, T), (ok, SC, KC, nbytes, end, smallest) in zip(shapes, ask(driver, ["recon %d %d %d" % s for s in shapes])):
        assert smallest == 20 * (T | 1)                                        # a row, its slot's targets and flags
        if not ok:
            assert smallest > budget, (m, K, T)
            continue
        assert nbytes == end <= budget, (m, K, T)
        assert covers(m, SC) and 1 <= KC <= K and SC * KC <= 256, (m, K, T, SC, KC)     # the passes step through K by KC: every sample once


def test_sweep_joint(driver, budget):
    shapes = list(itertools.product(MNO, TS))
    for (m, T), (ok, TC, _, nbytes, end, smallest) in zip(shapes, ask(driver, ["joint %d %d" % s for s in shapes])):
        stride = m + 1 if m >= 32 else m
        assert ok and 1 <= TC <= T and nbytes == end == 8 * stride * TC + 8 * m <= budget, (m, T)
        assert TC == chunk_frames(m, T), (m, T)                                # tests/joint_reference.py's own statement
        assert TC == T or nbytes + 8 * stride > budget, (m, T)                  # chunked only where one more frame does not fit


# request -> (ok, a, b, bytes): the values of the geometry functions before they moved into the header
PINNED = {"errors 32 20 40": (1, 32, 7, 52480),         # every slot, KC = 7: three sample chunks
          "errors 32 2 200": (1, 16, 1, 51456),         # slot chunks, one sample per chunk
          "errors 160 3 9": (1, 160, 1, 23040),
          "errors 1 1 3839": (1, 1, 1, 61424),
          "errors 1 1 3840": (0, 0, 0, 0),
          "kde 40": (1, 6, 0, 1968),                    # six agents per workgroup
          "kde 200": (1, 1, 0, 1608),
          "kde 7679": (1, 1, 0, 61432),
          "select 32 20 1 40": (1, 8, 32, 55744),       # MEAN at t_end 40: eight agents
          "select 32 20 1 20": (1, 16, 32, 60288),      # sixteen at t_end 20
          "select 32 20 0 40": (1, 16, 32, 9088),       # and with FINAL
          "select 160 130 1 5": (1, 7, 64, 54656),      # chunks of seven slots
          "select 8 130 1 56": (0, 0, 0, 0),            # K = 130: 56 frames refused (61888 bytes)
          "select 8 130 1 55": (1, 1, 64, 59808),       # 55 accepted
          "select 8 130 2 200": (0, 0, 0, 0),
          "select 8 130 0 200": (1, 8, 64, 29184),      # the last frame alone fits
          "recon 32 20 40": (1, 3, 20, 21156),
          "recon 32 70 5": (1, 3, 70, 8580),
          "recon 8 3 3071": (1, 1, 1, 61420),
          "recon 8 3 3072": (0, 0, 0, 0),
          "joint 32 40": (1, 40, 0, 10816),
          "joint 256 40": (1, 28, 0, 59616)}            # the frame-chunked walk: 28 + 12 frames


def test_documented_cases(driver):
    reqs = list(PINNED)
    for q, got in zip(reqs, ask(driver, reqs)):
        assert got[:4] == PINNED[q], (q, got)
    assert -(-20 // 7) == 3 and -(-160 // 7) == 23 and 160 % 7 == 6          # three sample chunks; 23 slot chunks, the last one partial


def test_a_malformed_request_is_an_error(driver):
    for text in ("errors 32 20\n", "errors 32 x 40\n", "bogus 1\n"):
        r = subprocess.run([driver], input=text, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == ""
    assert subprocess.run([driver], input="", capture_output=True, text=True).returncode == 0
