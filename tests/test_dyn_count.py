"""The grid rule of the launches that stride over their tiles (desire_amd/csrc/dyn_count.h: dyn_units).  With a device-side count the grid is sized from
a HINT of the count -- hint * mul units, a quarter of slack, 256 more -- and never above the worst case; a count above the grid is served by the kernels'
stride loops (tests/test_gpu_count_hint.py).  tests/c_host/dyn_count_driver.cpp is compiled against the header with g++ -- no ROCm header, no GPU."""
import os
import shutil
import subprocess

import pytest

from tests.helpers import hinted_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "dyn_count_driver.cpp")
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("dyn_count") / "dyn_count_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, rows):
    """dyn_units for every (worst, hint, mul, has_cnt) of `rows`, one driver process for all of them."""
    r = subprocess.run([driver], input="".join("%d %d %d %d\n" % row for row in rows), capture_output=True, text=True, check=True)
    out = [int(x) for x in r.stdout.split()]
    assert len(out) == len(rows)
    return out


WORSTS = [0, 1, 255, 256, 257, 768, 2304, 327680, INT_MAX]
HINTS = [1, 2, 3, 59, 204, 205, 409, 700, 767, 768, 100000, 2 ** 30, INT_MAX]
MULS = [1, 2, 3, 4, 20]


def test_never_above_the_worst_case(driver):
    rows = [(w, h, m, 1) for w in WORSTS for h in HINTS for m in MULS]
    for row, got in zip(rows, ask(driver, rows)):
        assert 0 <= got <= row[0], (row, got)


def test_without_a_count_or_a_hint_the_grid_is_the_worst_case(driver):
    rows = [(w, h, m, 0) for w in WORSTS for h in [-5, 0] + HINTS for m in MULS]         # no device-side count: the hint is not looked at
    rows += [(w, h, m, 1) for w in WORSTS for h in (-INT_MAX - 1, -1, 0) for m in MULS]  # a count, but no (usable) hint
    for row, got in zip(rows, ask(driver, rows)):
        assert got == row[0], (row, got)


def test_monotone_in_the_hint(driver):
    hints = list(range(1, 1200)) + [2 ** k + e for k in range(11, 31) for e in (-1, 0, 1)] + [INT_MAX]
    for w in (300, 768, 2304, 327680, INT_MAX):
        for m in (1, 3, 4):
            got = ask(driver, [(w, h, m, 1) for h in hints])
            assert all(a <= b for a, b in zip(got, got[1:])), (w, m)
            assert got[0] == min(w, m + m // 4 + 256) and got[-1] == w


def test_no_overflow_where_hint_times_mul_passes_2_to_the_31(driver):
    """hint * mul and its quarter of slack are formed in 64 bits: a product around 2^31 must come out as the worst case, not as a negative or a small
    grid (a wrapped 32-bit product would give either)."""
    rows = []
    for h, m in [(2 ** 30, 2), (2 ** 30 - 1, 2), (2 ** 29, 4), (715827883, 3), (INT_MAX, 1), (INT_MAX, 2), (INT_MAX, 20), (INT_MAX, INT_MAX),
                 (1717986918, 1), (1717986919, 1), (46341, 46341), (65536, 32768), (65536, 65536)]:
        for w in (768, 327680, INT_MAX - 1, INT_MAX):
            rows.append((w, h, m, 1))
    for row, got in zip(rows, ask(driver, rows)):
        w, h, m, _ = row
        g = h * m
        assert got == min(w, g + g // 4 + 256), (row, got)
        if g >= 2 ** 31:
            assert got == w, (row, got)


def test_the_python_mirror_equals_the_header(driver):
    rows = [(w, h, m, 1) for w in WORSTS + [9, 64, 300, 329, 551, 1023] for h in [-1, 0] + list(range(1, 40)) + HINTS for m in MULS]
    rows += [(w, h, 3, 1) for w in (768, 2304) for h in range(40, 800)]
    got = ask(driver, rows)
    for row, g in zip(rows, got):
        assert hinted_units(*row[:3]) == g, (row, g)
    # the figures of the count-hint test: a graph captured after a one-agent batch, replayed on a crowded one
    assert hinted_units(768, 1, 1) == 257 and hinted_units(2304, 1, 3) == 259 and hinted_units(1536, 1, 2) == 258


def test_a_malformed_request_is_an_error(driver):
    for text in ("768 1 3\n", "768 one 3 1\n"):                  # a short line, a field that is no number
        r = subprocess.run([driver], input=text, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == ""
    assert subprocess.run([driver], input="", capture_output=True, text=True).returncode == 0
