"""The counter-based generator of desire_set_rng / desire_rng_fill without a GPU: desire_amd/csrc/philox.h, compiled with g++ into
tests/c_host/philox_driver.cpp, against the numpy restatement tests/rng_reference.py.

  * the restatement reproduces the three published known answers of Philox4x32-10;
  * the header's raw stream and its packed counters equal the restatement BIT FOR BIT over sweeps that include the field maxima of the packing
    (L = 4096, slot 511, k = 8191) and scene_base + scene wrapping 2^32;
  * the header's fp32 normals lie within 1e-5 (absolute) of the float64 formula on the same bits.  The bound: theta = 2 pi u2 carries at most
    half an ulp at 2 pi plus the fp32 constant's own error, about 6.5e-7; scaled by r <= 5.77 that is 3.7e-6; a few ulp of logf, sinf and cosf
    come on top, under 5e-6 in all.  The cap is twice that;
  * the fixed seed of the GPU stream test passes that test's three statistical bounds on the restatement alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rng_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "philox_driver.cpp")
NORMAL_TOL = 1e-5
MASK = 0xFFFFFFFF


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("philox") / "philox_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, lines):
    r = subprocess.run([driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
    out = np.array([[int(w, 16) for w in row.split()] for row in r.stdout.splitlines()], np.uint64).astype(np.uint32)
    assert len(out) == len(lines)
    return out


def stream_sweep():
    """(counter, key) rows: the known answers, single-bit and all-ones words in every position, and seeded random ones."""
    rows = [c + k for c, k, _ in R.KNOWN_ANSWERS]
    for pos in range(6):
        for val in (1, 0x80000000, MASK):
            row = [0] * 6
            row[pos] = val
            rows.append(tuple(row))
    rng = np.random.default_rng(20240)
    rows += [tuple(int(v) for v in r) for r in rng.integers(0, 2 ** 32, size=(4000, 6), dtype=np.uint64)]
    return np.array(rows, np.uint64)


def test_the_restatement_reproduces_the_published_known_answers():
    for ctr, key, want in R.KNOWN_ANSWERS:
        got = R.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert tuple(int(v) for v in got) == want, (ctr, key, [hex(int(v)) for v in got])


def test_uniforms_are_exact_in_fp32_and_never_0_or_1():
    x = np.array([0, 1, 511, 512, MASK - 511, MASK], np.uint32)
    u = R.uniform(x)
    assert (u.astype(np.float32).astype(np.float64) == u).all()
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert abs(np.sqrt(-2.0 * np.log(u.min())) - np.sqrt(48 * np.log(2.0))) < 1e-12


def test_raw_stream_of_the_header_equals_the_restatement(driver):
    rows = stream_sweep()
    got = ask(driver, ["P " + " ".join("%x" % int(v) for v in row) for row in rows])
    want = R.philox4x32_10(rows[:, :4], rows[:, 4:])
    np.testing.assert_array_equal(got[:, :4], want)
    for i, (_, _, out) in enumerate(R.KNOWN_ANSWERS):
        assert tuple(int(v) for v in got[i, :4]) == out


def test_fp32_normals_of_the_header_are_within_1e_5_of_float64_on_the_same_bits(driver):
    rows = stream_sweep()
    got = ask(driver, ["P " + " ".join("%x" % int(v) for v in row) for row in rows])
    nrm = got[:, 4:].copy().view(np.float32).astype(np.float64)
    ref = R.normals(got[:, :4])
    err = float(np.abs(nrm - ref).max())
    print("max |fp32 normal - float64| over %d normals = %.2e" % (nrm.size, err))
    assert np.isfinite(nrm).all() and np.abs(nrm).max() <= np.sqrt(48 * np.log(2.0)) + NORMAL_TOL
    assert err <= NORMAL_TOL, err


def counter_sweep():
    """(draw, scene_base, scene, k, slot, l) with every field at 0, at its maximum, and mixed; scene_base + scene wraps 2^32 in some rows."""
    draws, bases, scenes = [0, 1, MASK], [0, 2, MASK - 1, MASK], [0, 1, 3, 511]
    ks, slots, ls = [0, 1, 2, R.MAX_K - 1], [0, 1, 31, R.MAX_SLOT - 1], [0, 1, 3, 4, 127, R.MAX_L - 4, R.MAX_L - 1]
    rows = [(d, b, s, k, sl, l) for d in draws for b in bases for s in scenes for k in ks for sl in slots for l in ls]
    assert any(b + s > MASK for _, b, s, _, _, _ in rows)
    return np.array(rows, np.uint64)


def test_packed_counters_of_the_header_equal_the_restatement(driver):
    rows = counter_sweep()
    got = ask(driver, ["E " + " ".join("%x" % int(v) for v in row) for row in rows])
    want = R.eps_counter(rows[:, 0], (rows[:, 1] + rows[:, 2]) & MASK, rows[:, 3], rows[:, 4], rows[:, 5])
    np.testing.assert_array_equal(got, want)
    # injective over (draw, window, k, slot, l >> 2): no two different blocks share a counter
    keyed = {}
    for row, c in zip(rows, got):
        ident = (int(row[0]), int((row[1] + row[2]) & MASK), int(row[3]), int(row[4]), int(row[5]) >> 2)
        assert keyed.setdefault(tuple(int(v) for v in c), ident) == ident
    blocks = [0, 1, MASK, MASK + 1, 2 ** 62 - 1]
    frows = [(sid, b) for sid in (0, 7, MASK) for b in blocks]
    got = ask(driver, ["F %x %x" % r for r in frows])
    for (sid, b), c in zip(frows, got):
        np.testing.assert_array_equal(c, R.fill_counter(sid, np.array([b], np.uint64))[0])
        assert c[3] == 1                                          # never a latent's counter (c3 = 0)


def test_a_fill_is_a_slice_of_any_longer_fill():
    long_b, long_n = R.fill_bits(R.STREAM_SEED, 3, 0, 64), R.fill_normals(R.STREAM_SEED, 3, 0, 64)
    np.testing.assert_array_equal(R.fill_bits(R.STREAM_SEED, 3, 5, 41), long_b[5:46])
    np.testing.assert_array_equal(R.fill_normals(R.STREAM_SEED, 3, 5, 41), long_n[5:46])


def test_the_fixed_seed_of_the_stream_test_passes_on_the_restatement():
    n = R.STREAM_N
    x = R.fill_normals(R.STREAM_SEED, R.STREAM_ID, 0, n)
    b_mean, b_var, b_ks = R.moment_bounds(n)
    mean, var, ks = float(x.mean()), float(x.var()), R.kolmogorov_distance(x)
    print("seed %#x stream %d, n = 2^20: mean %.3e (bound %.3e), var - 1 %.3e (%.3e), Kolmogorov distance %.3e (%.3e)"
          % (R.STREAM_SEED, R.STREAM_ID, mean, b_mean, var - 1, b_var, ks, b_ks))
    # with room for the 1e-5 that the fp32 normals may differ by
    assert abs(mean) + 1e-5 <= b_mean and abs(var - 1) + 2e-4 <= b_var and ks + 1e-5 <= b_ks


def test_a_malformed_request_is_an_error(driver):
    for text in ("P 0 0 0\n", "X 1 2\n", "E 0 0 0 0 zz 0\n"):
        r = subprocess.run([driver], input=text, capture_output=True, text=True)
        assert r.returncode != 0
    assert subprocess.run([driver], input="", capture_output=True, text=True).returncode == 0
