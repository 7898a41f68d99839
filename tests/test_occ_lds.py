"""The LDS plan and geometry of the occupancy kernel (desire_amd/csrc/eval_lds.h: OccLds, occupancy_geometry; csrc/kernels_occ.hip).
tests/c_host/occ_lds_driver.cpp is compiled against the header with g++ -- no ROCm header, no GPU.  A sweep holds every plan to the budget, the
chunk to a cover of the samples and frames and the bands to a cover of the grid rows; a table pins the cases DESIGN.md section 7h documents."""
import itertools
import os
import shutil
import subprocess

import pytest

from tests.occupancy_reference import band_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "occ_lds_driver.cpp")
KS = [1, 2, 3, 20, 130, 511, 512, 513, 4096]
FRAMES = [1, 7, 40, 200, 511, 512, 513, 7680]
SIDES = [1, 3, 5, 16, 64, 96, 333, 1024]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("occ_lds") / "occ_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, reqs):
    r = subprocess.run([driver], input="".join(q + "\n" for q in reqs), capture_output=True, text=True, check=True)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(reqs)
    return rows


def covers(n, per):
    """Chunks of `per` cover 0 .. n-1 exactly once with no empty chunk."""
    chunks = -(-n // per)
    return per >= 1 and (chunks - 1) * per < n <= chunks * per


def test_sweep(driver):
    (budget, threads, entries), = ask(driver, ["budget"])
    assert budget == 60 * 1024 and threads == 256 and entries == 512
    shapes = [(K, F, Oh, Ow, u) for K, F, Oh, Ow, u in itertools.product(KS, FRAMES, SIDES, SIDES, (0, 1)) if u or F == 1]      # mode AT walks one frame
    for (K, F, Oh, Ow, u), (ok, KC, FC, rows, bands, nbytes, end) in zip(shapes, ask(driver, ["occ %d %d %d %d %d" % s for s in shapes])):
        what = (K, F, Oh, Ow, u)
        assert ok, what                                                         # every K, every horizon, every grid up to 1024 x 1024 is served
        assert nbytes == end <= budget, what
        assert nbytes == 4 * ((4 if u else 3) * rows * Ow + 5 * KC * FC), what
        assert KC * FC <= entries and covers(K, KC) and covers(F, FC), what     # the chunks step through k by KC and through the frames by FC
        assert KC == 1 or FC == F, what                                         # several samples per chunk only with all their frames
        assert covers(Oh, rows) and bands == -(-Oh // rows), what               # every grid row in exactly one band, none empty
        assert bands == 1 or 4 * (4 if u else 3) * Oh * Ow + 20 * KC * FC > budget, what      # banded only where the whole grid does not fit
        assert rows == band_rows(K, F, Oh, Ow, u), what                         # tests/occupancy_reference.py's own statement


# request -> (ok, KC, FC, rows, bands, bytes): the cases of the DESIGN.md section 7h table
PINNED = {"occ 20 1 64 64 0": (1, 20, 1, 64, 1, 49552),          # the headline grid in mode AT: one band
          "occ 20 40 64 64 1": (1, 10, 40, 32, 2, 40768),        # ... in UNTIL: two chunks of ten samples, two bands of 32 rows
          "occ 5 1 96 96 0": (1, 5, 1, 48, 2, 55396),            # the banded test case: 2 x 48 rows in AT
          "occ 5 9 96 96 1": (1, 5, 9, 32, 3, 50052),            # ... 3 x 32 in UNTIL
          "occ 5 9 48 96 1": (1, 5, 9, 24, 2, 37764),
          "occ 130 7 8 8 1": (1, 65, 7, 8, 1, 10124),            # K = 130: two chunks of 65 samples
          "occ 4 9 16 16 1": (1, 4, 9, 16, 1, 4816),
          "occ 20 7680 1024 1024 1": (1, 1, 512, 3, 342, 59392),   # a horizon beyond a chunk: 15 chunks of 512 frames per sample; three rows per band
          "occ 4096 1 1024 1024 0": (1, 512, 1, 4, 256, 59392)}


def test_documented_cases(driver):
    reqs = list(PINNED)
    for q, got in zip(reqs, ask(driver, reqs)):
        assert got[:6] == PINNED[q], (q, got)


def test_a_malformed_request_is_an_error(driver):
    for text in ("occ 20 40 64\n", "occ 20 x 64 64 1\n", "bogus 1\n"):
        r = subprocess.run([driver], input=text, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == ""
    assert subprocess.run([driver], input="", capture_output=True, text=True).returncode == 0
