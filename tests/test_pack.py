"""The packed device operands (desire_amd/csrc/pack.h): one table says which operands exist, where each element comes from, in which MFMA fragment
order and encoding.  tests/c_host/pack_driver.cpp is compiled against the header with g++ -- no ROCm header, no GPU -- fills every weight from a
fixed integer generator and prints, per operand, its byte count, a digest of its bytes and a digest of its device repack map.

tests/golden/pack_digests.json was recorded from the packing code BEFORE the table existed (the 300-line desire_pack_all, and for the maps its
index-coded second run), so it pins "the same bytes as before" for six configurations that between them reach every operand and every padding
case.  The fragment orders themselves are checked against their formulas, restated here in numpy, on shapes that hang over every tile edge."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "pack_driver.cpp")
with open(os.path.join(ROOT, "tests", "golden", "pack_digests.json")) as fh:
    GOLDEN = json.load(fh)
# A: narrowest tile, 2*T_pred = 6 under one k-group (WrT padding).  B: bf16 operands, L = 24 (padded bf16 k-group), 2*T_pred = 40 (partial second
# n-tile), 9 bins, chain order, deconv4/W16.  C: two- and three-piece packs, W?T16, Wbwd16.  D: three pieces, Wsoc16l through mno > 128.
# E: Wsoc16l through H = 256.  F: 36 bins, gamma / beta uploads.
N_OPERANDS = {"A": 95, "B": 112, "C": 110, "D": 106, "E": 111, "F": 109}
MAPS = ("A", "C", "F")                                       # the shapes training accepts: their repack maps are pinned too


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("pack") / "pack_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("tag", sorted(N_OPERANDS))
def test_every_operand_has_the_recorded_bytes_and_map(driver, tag):
    c = GOLDEN[tag]["config"]
    r = subprocess.run([driver, "digests"] + [str(c[k]) for k in ("bf16", "H", "grid_size", "L", "T_pred", "mno", "bn_mode")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {}
    for ln in r.stdout.splitlines():
        name, nbytes, digest, mdigest = ln.split()
        assert name not in got, name
        got[name] = (int(nbytes), digest, mdigest)
    want = GOLDEN[tag]["operands"]
    assert len(want) == N_OPERANDS[tag]
    assert set(got) == set(want)                             # the names match exactly: nothing new, nothing missing, nothing skipped
    for name, w in want.items():
        assert got[name][0] == w["bytes"], name
        assert got[name][1] == w["digest"], name
        if tag in MAPS and w["map"] is not None:             # (none: the folded scale / shift, which k_refold follows)
            assert got[name][2] == w["map"], name
    if tag in MAPS:
        assert sorted(n for n, w in want.items() if w["map"] is None) == sorted(n for n in got if got[n][2] == "-")


@pytest.mark.parametrize("missing", ["ioc/social_fc/w", "vae_dec/deconv2/bn/moving_var", "head/b"])
def test_a_weight_that_is_not_set_is_an_error_not_a_read(driver, missing):
    """A packed operand, a folded batch-norm and a raw upload: each names the weight it lacks instead of throwing or reading past an empty vector."""
    c = GOLDEN["C"]["config"]
    r = subprocess.run([driver, "digests"] + [str(c[k]) for k in ("bf16", "H", "grid_size", "L", "T_pred", "mno", "bn_mode")] + [missing],
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.strip() == "weight not set: " + missing


def slots(driver, which, K, N):
    r = subprocess.run([driver, "order", which, str(K), str(N)], capture_output=True, text=True, check=True)
    return np.array([int(x) for x in r.stdout.split()], dtype=np.int64)


def expect(k, n, K, N):
    return np.where((k < K) & (n < N), k * N + n, -1)


def check_permutation(got, K, N):
    assert np.array_equal(np.sort(got[got >= 0]), np.arange(K * N))      # every element once, everything else padding


@pytest.mark.parametrize("K,N", [(20, 40), (8, 32), (1, 1), (33, 65)])
def test_fp32_order(driver, K, N):
    """out[((nt*G + g)*64 + lane)*4 + i] = B(k = 8g + 4*(lane>>5) + i, n = 32nt + (lane&31)), G = ceil(K/8), nt < ceil(N/32)"""
    G, NT = -(-K // 8), -(-N // 32)
    s = np.arange(NT * G * 64 * 4)
    i, lane, g, nt = s % 4, s // 4 % 64, s // 256 % G, s // (256 * G)
    got = slots(driver, "f32", K, N)
    assert np.array_equal(got, expect(8 * g + 4 * (lane >> 5) + i, 32 * nt + (lane & 31), K, N))
    check_permutation(got, K, N)


@pytest.mark.parametrize("kmap", ["lin", "chain"])
@pytest.mark.parametrize("K,N", [(20, 40), (32, 32), (64, 25), (24, 2048)])
def test_bf16_order(driver, kmap, K, N):
    """out[((nt*G + g)*64 + lane)*8 + e] = B(k = kmap(g, lane>>5, e), n = 32nt + (lane&31)), G = ceil(K/16), nt < ceil(N/32);
    lin(g, hi, e) = 16g + 8hi + e; chain(g, hi, e) = 32*(g>>1) + (r&3) + 8*(r>>2) + 4hi with r = 8*(g&1) + e"""
    G, NT = -(-K // 16), -(-N // 32)
    s = np.arange(NT * G * 64 * 8)
    e, lane, g, nt = s % 8, s // 8 % 64, s // 512 % G, s // (512 * G)
    hi = lane >> 5
    if kmap == "lin":
        k = 16 * g + 8 * hi + e
    else:
        r = 8 * (g & 1) + e
        k = 32 * (g >> 1) + (r & 3) + 8 * (r >> 2) + 4 * hi
    got = slots(driver, kmap, K, N)
    assert np.array_equal(got, expect(k, 32 * nt + (lane & 31), K, N))
    check_permutation(got, K, N)


@pytest.mark.parametrize("K,N", [(32, 32), (64, 64), (20, 40)])
def test_16x16x4_order(driver, K, N):
    """out[((ct*G + g)*64 + lane)*4 + j] = B(k = 16g + 4*(lane>>4) + j, n = 16ct + (lane&15)), G = ceil(K/16), ct < ceil(N/16)"""
    G, CT = -(-K // 16), -(-N // 16)
    s = np.arange(CT * G * 64 * 4)
    j, lane, g, ct = s % 4, s // 4 % 64, s // 256 % G, s // (256 * G)
    got = slots(driver, "c16", K, N)
    assert np.array_equal(got, expect(16 * g + 4 * (lane >> 4) + j, 16 * ct + (lane & 15), K, N))
    check_permutation(got, K, N)
