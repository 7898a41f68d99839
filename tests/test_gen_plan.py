"""The sample-generation plan (desire_amd/csrc/gen_plan.h): which kernel family -- fp32, plain bf16, six-product -- serves each stage of
desire_encode / desire_sample, the piece count, the deconv3 + deconv4 fusion, and the split-operand switches of the training step.  The header is
host-only C++ without HIP headers: tests/c_host/gen_plan_driver.cpp is compiled against it with g++ and run over a table of documented cases
(written from the if / else chains the plan replaced, not computed), and over a sweep in which every operand a plan reads must exist, once, in
the operand table of pack.h built for the same dims."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "gen_plan_driver.cpp")
NO_FUSE34, TRAIN_FWD_3P = 1, 2                               # DESIRE_FLAG_* (include/desire_hip.h)


def case(bf16=0, training=0, flags=0, mask=0, bn_mode=0, ref_compat=0, H=128, L=64, V=1024):
    return (bf16, training, flags, mask, bn_mode, ref_compat, H, L, V)


F, B, X = "FP32", "BF16", "X6"
ALL_F, ALL_B = [F] * 7, [B] * 7
GEN_X = [F, F, X, X, X, X, X]                                # the five sample stages; the encoder stack has no six-product form
# (case, [encoder, conv23, deconv1, deconv2, deconv3, mask, decoder], fuse34, np, batch_stats, wgrad_pieces, dgrad_split)
TABLE = [
    # fp32 operands
    (case(), ALL_F, 0, 3, 0, 0, 0),
    (case(training=1), ALL_F, 0, 3, 0, 0, 0),
    (case(training=1, mask=15), ALL_F, 0, 3, 0, 0, 0),                       # the mask is a dims.bf16 = 2 matter
    (case(bn_mode=1), ALL_F, 0, 3, 1, 0, 0),
    (case(bn_mode=2, training=1), ALL_F, 0, 3, 1, 0, 0),
    (case(ref_compat=1, bn_mode=1), ALL_F, 0, 3, 1, 0, 0),
    # plain bf16 operands
    (case(bf16=1), ALL_B, 1, 3, 0, 0, 0),
    (case(bf16=1, flags=NO_FUSE34), ALL_B, 0, 3, 0, 0, 0),
    (case(bf16=1, L=512), ALL_B, 1, 3, 0, 0, 0),
    (case(bf16=1, L=520), [B, B, F, B, B, B, B], 1, 3, 0, 0, 0),             # deconv1 alone falls back: more than 512 latent columns
    (case(bf16=1, L=24), [B, B, F, B, B, B, B], 1, 3, 0, 0, 0),              # ... or a partial bf16 k-group
    (case(bf16=1, H=256, V=1088), ALL_B, 1, 3, 0, 0, 0),                     # the six-product shape limits are not the bf16 kernels'
    # three pieces, inference only
    (case(bf16=3), GEN_X, 0, 3, 0, 0, 0),
    (case(bf16=3, H=64), GEN_X, 0, 3, 0, 0, 0),
    (case(bf16=3, flags=TRAIN_FWD_3P), GEN_X, 0, 3, 0, 0, 0),                # the flag is about the training forward
    (case(bf16=3, H=256), [F, F, X, X, X, F, X], 0, 3, 0, 0, 0),             # no six-product mask fc at H = 256; the decoder has one
    (case(bf16=3, L=128), GEN_X, 0, 3, 0, 0, 0),
    (case(bf16=3, L=256), [F, F, F, X, X, X, X], 0, 3, 0, 0, 0),             # six-product deconv1: L <= 128
    (case(bf16=3, L=24), [F, F, F, X, X, X, X], 0, 3, 0, 0, 0),              # ... in whole k-groups of 16
    (case(bf16=3, V=1088), [F, F, X, X, X, F, X], 0, 3, 0, 0, 0),            # six-product mask fc: V in 128-column chunks
    (case(bf16=3, training=1), ALL_F, 0, 3, 0, 0, 0),                        # (desire_set_training refuses it)
    (case(bf16=3, bn_mode=1), ALL_F, 0, 3, 1, 0, 0),
    (case(bf16=3, ref_compat=1), ALL_F, 0, 3, 0, 0, 0),
    # two pieces in the IOC kernels and the training step: sample generation as dims.bf16 = 3
    (case(bf16=2), GEN_X, 0, 3, 0, 2, 1),
    (case(bf16=2, mask=8), GEN_X, 0, 3, 0, 2, 1),                            # the mask holds back the TRAINING forward only
    (case(bf16=2, H=256, L=256, V=1088), [F, F, F, X, X, F, X], 0, 3, 0, 2, 1),
    (case(bf16=2, training=1), GEN_X, 0, 3, 0, 2, 1),
    (case(bf16=2, training=1, flags=TRAIN_FWD_3P), GEN_X, 0, 2, 0, 2, 1),
    (case(bf16=2, training=1, mask=8), ALL_F, 0, 3, 0, 2, 1),
    (case(bf16=2, training=1, mask=8, flags=TRAIN_FWD_3P), ALL_F, 0, 2, 0, 2, 1),    # (no X6 stage reads np)
    (case(bf16=2, training=1, mask=1), GEN_X, 0, 3, 0, 0, 1),
    (case(bf16=2, training=1, mask=2), GEN_X, 0, 3, 0, 2, 0),
    (case(bf16=2, training=1, mask=4), GEN_X, 0, 3, 0, 2, 1),                # the IOC BPTT's bit: ioc_plan.h
    (case(bf16=2, training=1, mask=15), ALL_F, 0, 3, 0, 0, 0),
    (case(bf16=2, bn_mode=1), ALL_F, 0, 3, 1, 2, 1),
    (case(bf16=2, bn_mode=2, training=1), ALL_F, 0, 3, 1, 2, 1),
    (case(bf16=2, ref_compat=1), ALL_F, 0, 3, 0, 2, 1),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("gen_plan") / "gen_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run(driver, cases, *args):
    stdin = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
    lines = subprocess.run([driver, *args], input=stdin, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    return lines


def test_plan_table(driver):
    for (c, forms, fuse34, np_, batch_stats, wgrad, dgrad), line in zip(TABLE, run(driver, [t[0] for t in TABLE])):
        assert line.split() == forms + [str(fuse34), str(np_), str(batch_stats), str(wgrad), str(dgrad)], (c, line)
        bf16, mask = c[0], c[3]
        assert (wgrad == 2) == (bf16 == 2 and not mask & 1) and wgrad in (0, 2), c
        assert bool(dgrad) == (bf16 == 2 and not mask & 2), c


def test_every_operand_a_plan_reads_is_in_the_operand_table(driver):
    """A form chosen for dims whose pack was not built would hand a kernel a null weight pointer: over the product below, every name in the plan's
    needs() occurs exactly once in pack::operands() of the same dims.  Combinations desire_create / desire_set_training refuse are skipped."""
    axes = dict(bf16=(0, 1, 2, 3), training=(0, 1), flags=(0, NO_FUSE34, TRAIN_FWD_3P), mask=(0, 8, 15), bn_mode=(0, 1), H=(64, 128, 256),
                L=(24, 64, 128, 256, 520))
    sweep = [dict(zip(axes, v)) for v in itertools.product(*axes.values())]
    refused = lambda k: (k["bn_mode"] and k["bf16"] == 1) or (k["training"] and k["bf16"] in (1, 3))
    cases = [case(**k) for k in sweep if not refused(k)]
    checked = 0
    for c, line in zip(cases, run(driver, cases, "needs")):
        got = dict(item.rsplit("=", 1) for item in line.split())
        assert len(got) >= 13, (c, line)                     # ten stages, three of them GRUs with two operands each
        assert all(n == "1" for n in got.values()), (c, line)
        checked += 1
    # 2160 combinations; refused: batch statistics on bf16 operands (2 * 3 * 3 * 3 * 5 = 270), training with dims.bf16 = 1 (270, of which 135
    # are among the former) or 3 (270)
    print("checked %d of %d combinations" % (checked, len(sweep)))
    assert len(sweep) == 2160 and checked == 2160 - (270 + 135 + 270)


def test_the_pack_names_of_sample_generation_are_spelled_in_one_place():
    """Outside gen_plan.h (which operand a stage reads) and pack.h (how it is built) no host file names a bf16 or three-piece pack of sample
    generation.  Comments may: the kernel files say which pack a launcher expects."""
    csrc = os.path.join(ROOT, "desire_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name in ("gen_plan.h", "pack.h"):
            continue
        with open(os.path.join(csrc, name)) as fh:
            code = "\n".join(ln.split("//", 1)[0] for ln in fh)
        for word in ('W16"', 'W6"', "Whg6", "Whc6", "Whg16", "Whc16"):
            assert word not in code, (name, word)
