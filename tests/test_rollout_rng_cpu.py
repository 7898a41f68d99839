"""The rollout counter of the device generator (desire_rollout_samples with NULL normals; include/desire_hip.h "device generator") without a GPU:
desire_amd/csrc/philox.h compiled with g++ into tests/c_host/rollout_philox_driver.cpp, against the numpy restatement tests/rollout_reference.py.

  * the header's packed rollout counters and the words Philox makes of them equal the restatement BIT FOR BIT over a sweep that includes the field
    maxima of the packing (t = 2047, slot 511, k = 8191) and scene_base + scene wrapping 2^32;
  * the counter is injective over (draw, window, k, slot, t >> 1), and the two steps of a block share it;
  * the header's fp32 normals lie within 1e-5 of the float64 formula on the same bits (the bound tests/test_rng_cpu.py derives);
  * no rollout block equals the latent or the fill block of the same (c0, c1, c2): the counters differ in c3, and so do the words;
  * the restated fill layout hands step t normals 2 (t & 1) and 2 (t & 1) + 1 of block t >> 1, for odd and even T_pred;
  * the binding lists the new export and fill kind, and the evaluation command line knows the generator."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rng_reference as R
from tests import rollout_reference as RR
from tests.test_rng_cpu import NORMAL_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "rollout_philox_driver.cpp")
MASK = 0xFFFFFFFF
SEED = 0x1234ABCD9876F00D


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("rollout_philox") / "rollout_philox_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, rows, seed=SEED):
    key = R.seed_key(seed)
    text = "".join("R " + " ".join("%x" % int(v) for v in row) + " %x %x\n" % (int(key[0]), int(key[1])) for row in rows)
    r = subprocess.run([driver], input=text, capture_output=True, text=True, check=True)
    out = np.array([[int(w, 16) for w in line.split()] for line in r.stdout.splitlines()], np.uint64).astype(np.uint32)
    assert out.shape == (len(rows), 12)
    return out[:, :4], out[:, 4:8], out[:, 8:].copy().view(np.float32)


def counter_sweep():
    """(draw, scene_base, scene, k, slot, t) with every field at 0, at its maximum, and mixed; scene_base + scene wraps 2^32 in some rows."""
    draws, bases, scenes = [0, 1, MASK], [0, 2, MASK - 1, MASK], [0, 1, 3, 511]
    ks, slots, ts = [0, 1, 2, R.MAX_K - 1], [0, 1, 31, R.MAX_SLOT - 1], [0, 1, 2, 3, 8, 9, RR.MAX_T - 2, RR.MAX_T - 1]
    rows = [(d, b, s, k, sl, t) for d in draws for b in bases for s in scenes for k in ks for sl in slots for t in ts]
    assert any(b + s > MASK for _, b, s, _, _, _ in rows)
    assert any(r[3] == 8191 and r[4] == 511 and r[5] == 2047 for r in rows)
    return np.array(rows, np.uint64)


@pytest.fixture(scope="module")
def swept(driver):
    rows = counter_sweep()
    return (rows,) + ask(driver, rows)


def test_rollout_counters_and_words_of_the_header_equal_the_restatement(swept):
    rows, ctr, words, _ = swept
    want = RR.roll_counter(rows[:, 0], (rows[:, 1] + rows[:, 2]) & MASK, rows[:, 3], rows[:, 4], rows[:, 5])
    np.testing.assert_array_equal(ctr, want)
    assert (ctr[:, 3] == RR.ROLL).all()
    np.testing.assert_array_equal(words, R.philox4x32_10(want, R.seed_key(SEED)))
    # the fields do not overlap at their maxima: (t >> 1) < 2^10, slot < 2^9, k < 2^13
    top = RR.roll_counter(0, 0, R.MAX_K - 1, R.MAX_SLOT - 1, RR.MAX_T - 1)
    assert int(top[0]) == MASK and (RR.MAX_T - 1) >> 1 == 1023


def test_the_counter_is_injective_over_blocks_and_shared_by_the_two_steps_of_one(swept):
    rows, ctr, _, _ = swept
    keyed = {}
    for row, c in zip(rows, ctr):
        ident = (int(row[0]), int((row[1] + row[2]) & MASK), int(row[3]), int(row[4]), int(row[5]) >> 1)
        assert keyed.setdefault(tuple(int(v) for v in c), ident) == ident
    assert len(keyed) == len({(int(r[0]), int((r[1] + r[2]) & MASK), int(r[3]), int(r[4]), int(r[5]) >> 1) for r in rows})


def test_fp32_rollout_normals_of_the_header_are_within_1e_5_of_float64_on_the_same_bits(swept):
    _, _, words, nrm = swept
    ref = R.normals(words)
    err = float(np.abs(nrm.astype(np.float64) - ref).max())
    print("max |fp32 rollout normal - float64| over %d normals = %.2e" % (nrm.size, err))
    assert np.isfinite(nrm).all()
    assert err <= NORMAL_TOL, err


def test_no_rollout_block_equals_the_latent_or_fill_block_of_the_same_counter_words(swept):
    rows, ctr, words, _ = swept
    key = R.seed_key(SEED)
    for c3 in (0, 1):                                             # the latent eps (c3 = 0) and the fill op (c3 = 1) on the same (c0, c1, c2)
        other = ctr.copy()
        other[:, 3] = c3
        ow = R.philox4x32_10(other, key)
        assert not (ow == words).all(axis=1).any(), c3
    # ... spelled through their own counter functions: latent l = 4 (t >> 1) of the same (draw, window, k, slot) packs the same c0
    win = (rows[:, 1] + rows[:, 2]) & MASK
    lat = R.eps_counter(rows[:, 0], win, rows[:, 3], rows[:, 4], 4 * (rows[:, 5] >> np.uint64(1)))
    np.testing.assert_array_equal(lat[:, :3], ctr[:, :3])
    assert (lat[:, 3] == 0).all() and not (R.philox4x32_10(lat, key) == words).all(axis=1).any()
    blk = ctr[:, 0].astype(np.uint64) | (ctr[:, 1].astype(np.uint64) << np.uint64(32))
    for i in range(0, len(rows), 97):
        f = R.fill_counter(int(ctr[i, 2]), np.array([blk[i]], np.uint64))[0]
        np.testing.assert_array_equal(f[:3], ctr[i, :3])
        assert f[3] == 1 and not (R.philox4x32_10(f, key) == words[i]).all()


@pytest.mark.parametrize("T_pred", [9, 12, 1])
def test_the_fill_layout_hands_each_step_its_pair_of_the_block(driver, T_pred):
    n_scenes, K, mno, draw, sb, slb = 2, 3, 4, 5, MASK, 500        # (windows MASK, MASK + 1 -> 0: the wrap)
    got = RR.rollout_normals(SEED, draw, n_scenes, K, mno, T_pred, scene_base=sb, slot_base=slb)
    assert got.shape == (n_scenes, K, mno, T_pred, 2)
    rows = [(draw, sb, sc, k, sl + slb, t) for sc in range(n_scenes) for k in range(K) for sl in range(mno) for t in range(T_pred)]
    _, words, nrm = ask(driver, np.array(rows, np.uint64))
    pick = np.array([[2 * (r[5] & 1), 2 * (r[5] & 1) + 1] for r in rows])
    want64 = np.take_along_axis(R.normals(words), pick, 1).reshape(got.shape)
    np.testing.assert_array_equal(got, want64)                   # the restatement's layout on the header's own words
    hdr = np.take_along_axis(nrm.astype(np.float64), pick, 1).reshape(got.shape)
    assert np.abs(hdr - got).max() <= NORMAL_TOL


def test_a_malformed_request_is_an_error(driver):
    for text in ("R 0 0 0\n", "E 0 0 0 0 0 0\n", "R 0 0 0 0 zz 0 0 0\n"):
        assert subprocess.run([driver], input=text, capture_output=True, text=True).returncode != 0
    assert subprocess.run([driver], input="", capture_output=True, text=True).returncode == 0


def test_the_binding_and_the_command_line_know_the_rollout_generator():
    from desire_amd import _lib
    from desire_amd import evaluate as E
    assert "desire_rollout_samples" in _lib.EXPORTS and _lib.RNG_ROLLOUT == 3 and hasattr(_lib.Handle, "rollout_samples")
    with open(os.path.join(ROOT, "include", "desire_hip.h")) as fh:
        hdr = fh.read()
    assert "#define DESIRE_RNG_ROLLOUT 3" in hdr and "int desire_rollout_samples(desire_handle* h, const float* dev_past, const float* dev_normals," in hdr
    assert E.build_parser().parse_args(["--checkpoint", "c.npz"]).generator == "cvae"
    assert E.build_parser().parse_args(["--checkpoint", "c.npz", "--generator", "rollout"]).generator == "rollout"
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--checkpoint", "c.npz", "--generator", "gan"])
