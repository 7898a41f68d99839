"""k_ioc's dense pooling with the rows read in place (desire_amd/csrc/kernels_rnn.hip): the two pieces of it that the CPU can check.
tests/c_host/ioc_pool_driver.cpp is compiled with g++ against ioc_lds.h (the sum-slot count) and the plain-C++ head of ioc_tile.h (the row
source of a (row, bin) by its neighbour mask) -- no ROCm header, no GPU.

  * desire_amd.spec.ioc_pool_slots, which tests/test_gpu_ioc_pool_rows.py sizes its regimes by, equals the header's constexpr, and the
    row-source table of the largest grid (64 bins, one byte per pair) fits behind the slots in the AB region;
  * ioc_row_offset, the table's one-byte codes, sends every code to its own row: h rows, the zero row's lane slots and the sum slots lie apart;
  * ioc_row_source against numpy on masks of 0, 1, 2, 31, 32 and 64 set bits, both mask widths."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from desire_amd.spec import ioc_pool_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "ioc_pool_driver.cpp")
ZERO, SUM = -1, -2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ioc_pool") / "ioc_pool_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, reqs):
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs)
    return rows


def test_the_mirror_equals_the_header_and_the_table_fits(driver):
    shapes = [(H, TM) for H in (64, 128, 256) for TM in (32, 64)]
    for (H, TM), (n, behind, max_bins) in zip(shapes, ask(driver, ["slots %d %d" % s for s in shapes])):
        assert n == ioc_pool_slots(H, TM), (H, TM)
        assert max_bins == 64 and 0 < n < 2 * TM and behind >= TM * max_bins and 3 * TM < 256, (H, TM, n, behind)
        assert behind - (H + 4) * 4 < TM * max_bins, "a whole row more than the table needs: %s" % ((H, TM),)
    assert ioc_pool_slots(128, 32) == 60            # the headline's; 32 agents inside one bin cell need at least 60 (tests/ioc_pool_cases.py: one_cell)


def reference(m):
    """numpy's statement: no bit -> the zero row, one -> its index, more -> a sum slot."""
    bits = np.flatnonzero([(m >> i) & 1 for i in range(64)])
    return ZERO if bits.size == 0 else int(bits[0]) if bits.size == 1 else SUM


def masks(width, rng):
    out = [0, (1 << width) - 1, ((1 << width) - 1) >> 1, ((1 << width) - 1) & ~1]         # 0, all, all but the top (31 / 63), all but the lowest
    out += [1 << i for i in range(width)]                                                # one bit, every position
    out += [(1 << i) | (1 << j) for i in range(width) for j in range(i + 1, width, 7)]   # two bits
    for n in (2, 3, 31, min(32, width)):
        for _ in range(8):
            out.append(sum(1 << int(i) for i in rng.choice(width, n, replace=False)))
    return out


@pytest.mark.parametrize("width", [32, 64])
def test_row_source_against_numpy(driver, width):
    ms = masks(width, np.random.default_rng(width))
    counts = {bin(m).count("1") for m in ms}
    assert {0, 1, 2, 31, width} <= counts
    got = ask(driver, ["src%d %x" % (width, m) for m in ms])
    for m, (g,) in zip(ms, got):
        assert g == reference(m), hex(m)


@pytest.mark.parametrize("H,TM", [(128, 32), (64, 32), (256, 32), (128, 64), (64, 64)])
def test_row_codes_address_disjoint_rows_inside_the_tile(driver, H, TM):
    E = 16 + 32 + H
    LDX, LDB, n = E + H + 4, H + 4, ioc_pool_slots(H, TM)
    codes = list(range(TM + 1 + n))
    got = [g for g, in ask(driver, ["off %d %d %d %d %d %d" % (c, TM, LDX, E, LDB, 0) for c in codes])]
    assert got[:TM] == [r * LDX + E for r in range(TM)]                           # the h columns of tile row r
    assert got[TM] == TM * LDX                                                    # the zero row
    assert got[TM + 1:] == [(TM + 1) * LDX + s * LDB for s in range(n)]           # slot s of the AB region behind the TM + 1 rows of XH
    lanes = [g for g, in ask(driver, ["off %d %d %d %d %d %d" % (TM, TM, LDX, E, LDB, l) for l in range(16)])]
    assert lanes == [TM * LDX + 4 * l for l in range(16)]                         # sixteen 16-byte slots: one per lane of a 16-lane group
    reach = 4 + 8 * (H // 8 - 1) + 4                                              # what a lane reads behind its row pointer: upper half-wave, last k-group
    assert lanes[-1] + reach <= (TM + 1) * LDX and got[-1] + reach <= (TM + 1) * LDX + n * LDB
    assert (TM + 1) * LDX + n * LDB + TM * 64 / 4 <= (TM + 1) * LDX + 2 * TM * LDB  # the table ends inside the AB region
