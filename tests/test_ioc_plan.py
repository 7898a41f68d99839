"""The IOC plan (desire_amd/csrc/ioc_plan.h): which kernel family serves a call, the bin-split count, the BPTT family and whether slot class 10
(padded tiles) exists.  The header is host-only C++ without HIP headers: tests/c_host/ioc_plan_driver.cpp is compiled against it with g++ and
run over a table of documented cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "ioc_plan_driver.cpp")
BIG = 1 << 20                  # bin-split capacity: ample


def case(bf16=0, training=0, form=0, split=0, H=128, G=4, iters=1, mno=32, mask=0, vmno=None, gpt=0, windows=512, K=4, R=None, cap=BIG):
    vmno = mno if vmno is None else vmno
    if R is None:
        ngrp = windows * K
        R = ((ngrp + gpt - 1) // gpt) * 32 if gpt else ngrp * vmno
    return (bf16, training, form, split, H, G, iters, mno, mask, vmno, gpt, R, cap)


# (case, forward, nspl, backward, padded)
TABLE = [
    # fp32 operands
    (case(), "FP32", 1, "FP32", 1),                                          # 32-row tile
    (case(mno=64, H=128, G=4), "FP32_WIDE", 1, "FP32", 1),                   # 64 agents, 16 bins: the 64-row tile
    (case(mno=64, H=128, G=6), "FP32_CLUSTER", 1, "CLUSTER", 1),             # 36 bins: the 64-row tile's masks exceed 160 KB
    (case(mno=64, H=256), "FP32_CLUSTER", 1, "CLUSTER", 0),
    (case(mno=96), "FP32_CLUSTER", 1, "CLUSTER", 1),
    (case(mno=128), "FP32_CLUSTER", 1, "CLUSTER", 1),
    (case(mno=16, form=2), "FP32_WIDE", 1, "FP32", 0),                       # DESIRE_IOC_TILE64
    (case(mno=32, H=256, form=2), "FP32", 1, "FP32", 0),                     # H = 256: 32-row tiles only
    (case(mno=160), "STEPWISE", 1, "CLUSTER", 1),
    (case(mno=256, bf16=1), "STEPWISE", 1, "CLUSTER", 0),
    # split operands
    (case(bf16=2, H=256), "STEPWISE", 1, "FP32", 0),
    (case(bf16=3, H=256, mno=64), "STEPWISE", 1, "CLUSTER", 0),
    (case(bf16=2, H=256, form=2), "FP32", 1, "FP32", 0),                     # a form asked for: no step-wise
    (case(bf16=2, training=1, H=256), "FP32", 1, "FP32", 0),                 # training: the fp32 kernels
    (case(bf16=2, mno=64, H=128, G=4), "X3R2", 1, "FP32", 1),
    (case(bf16=2, mno=32), "X3", 1, "X3", 1),
    (case(bf16=2, training=1, mno=32), "X3", 1, "X3", 1),
    (case(bf16=2, training=1, mno=16, H=64), "X3", 1, "X3", 1),
    (case(bf16=2, training=1, mno=32, mask=4), "X3", 1, "FP32", 0),          # fp32 BPTT: no class 10
    (case(bf16=2, training=1, mno=64), "FP32_WIDE", 1, "FP32", 1),           # training at 64 agents: the fp32 forward
    (case(bf16=3, mno=32, windows=1024, K=16), "X6R2", 1, "FP32", 0),       # >= 256 64-row tiles
    (case(bf16=3, mno=32, windows=1024, K=16, form=13), "X6", 1, "FP32", 0),
    (case(bf16=3, mno=32, windows=8), "X6", 1, "FP32", 0),                   # a few windows: 32-row tiles
    (case(bf16=3, mno=32, windows=8, form=14), "X6R2", 1, "FP32", 0),
    (case(bf16=3, mno=64), "X6R2", 1, "FP32", 0),
    # plain bf16 operands
    (case(bf16=1, mno=32), "BF16", 1, "FP32", 0),
    (case(bf16=1, mno=64), "BF16_WIDE", 1, "FP32", 0),
    (case(bf16=1, mno=64, form=4), "BF16_CLUSTER", 1, "FP32", 0),
    (case(bf16=1, mno=64, form=6), "BF16_CLUSTER", 1, "FP32", 0),
    (case(bf16=1, mno=96), "BF16_CLUSTER", 1, "CLUSTER", 0),
    # the training forward's cluster test passes ioc_form, the BPTT's passes 0: ioc_form 4 at 64 agents trains on k_ioc_cl<TRAIN> + the 64-row k_ioc_bwd
    (case(training=1, mno=64, form=4), "FP32_CLUSTER", 1, "FP32", 0),
    # bin split (fp32 inference, a handful of windows; 4 slot-rows per window at K = 4)
    (case(windows=1), "FP32", 4, "FP32", 1),                                 # 4 tiles
    (case(windows=20), "FP32", 3, "FP32", 1),                                # 80 tiles
    (case(windows=30), "FP32", 2, "FP32", 1),                                # 120 tiles
    (case(windows=70), "FP32", 1, "FP32", 1),                                # 280 tiles
    (case(windows=1, split=3), "FP32", 3, "FP32", 1),                        # dims.ioc_split caps it
    (case(windows=1, split=2), "FP32", 2, "FP32", 1),
    (case(windows=1, split=1), "FP32", 1, "FP32", 1),                        # 1: never split
    (case(windows=1, cap=12), "FP32", 3, "FP32", 1),                         # 16 workgroups not resident, 12 are
    (case(windows=1, cap=0), "FP32", 1, "FP32", 1),
    (case(windows=1, G=1), "FP32", 1, "FP32", 1),                            # one bin
    (case(windows=1, iters=2), "FP32", 1, "FP32", 1),
    (case(windows=1, form=8), "FP32", 1, "FP32", 0),
    (case(windows=1, training=1), "FP32", 1, "FP32", 1),
    (case(windows=1, mno=16, vmno=10, gpt=3), "FP32", 1, "FP32", 1),          # padded tiles: not split
    # slot class 10: the padded-tile view
    (case(mno=32, vmno=10, gpt=3), "FP32", 1, "FP32", 1),
    (case(bf16=2, mno=32, vmno=10, gpt=3), "X3", 1, "X3", 1),
    (case(bf16=2, training=1, mno=32, vmno=10, gpt=3), "X3", 1, "X3", 1),
    (case(training=1, mno=32, vmno=10, gpt=3), "FP32", 1, "FP32", 1),
    (case(H=256, mno=32), "FP32", 1, "FP32", 0),
    (case(form=9, training=1), "FP32", 1, "FP32", 0),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ioc_plan") / "ioc_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_plan_table(driver):
    stdin = "".join(" ".join(str(x) for x in c) + "\n" for c, *_ in TABLE)
    r = subprocess.run([driver], input=stdin, capture_output=True, text=True, check=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(TABLE)
    for (c, fwd, nspl, bwd, padded), line in zip(TABLE, lines):
        got = line.split()
        assert got[:4] == [fwd, str(nspl), bwd, str(padded)], (c, line)
        cluster = fwd in ("FP32_CLUSTER", "BF16_CLUSTER")
        assert got[4:] == [str(int(cluster)), str(int(nspl > 1))], (c, line)         # the exchange buffers the plan needs
