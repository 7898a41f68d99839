"""The owner of the handle's named device buffers (desire_amd/csrc/workspace.h): ensure() is the single allocation primitive, lookups never insert
and never throw, and a failed allocation leaves no entry behind that would make the next call skip it.  tests/c_host/workspace_driver.cpp is
compiled against the header with g++ -- no ROCm header, no GPU -- over a counting fake allocator that can be told to fail the n-th allocation."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "workspace_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("workspace") / "workspace_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, lines):
    """One fresh workspace per call: the answers, each split into fields (the last three: allocations, frees, entries).  check=True: the driver
    exits non-zero on an exception, a malformed request, or when the frees at its end do not match the allocations."""
    r = subprocess.run([driver], input="".join(x + "\n" for x in lines), capture_output=True, text=True, check=True)
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def counters(ans):
    return tuple(int(x) for x in ans[-3:])


def test_ensure_is_idempotent_and_only_grows(driver):
    a = ask(driver, ["ensure buf 1024", "get buf", "ensure buf 1024", "get buf", "ensure buf 16", "get buf", "ensure buf 4096", "get buf"])
    assert a[0][:2] == ["0", "1"] and counters(a[0]) == (1, 0, 1)             # allocated, and says so
    p0 = int(a[1][0])
    assert p0 != 0 and a[1][1:4] == ["1024", "1", "1"]
    assert a[2][:2] == ["0", "0"] and counters(a[2]) == (1, 0, 1)             # the same size again: one allocation in all
    assert int(a[3][0]) == p0
    assert a[4][:2] == ["0", "0"] and counters(a[4]) == (1, 0, 1)             # a smaller request: the same buffer
    assert int(a[5][0]) == p0 and a[5][1] == "1024"
    assert a[6][:2] == ["0", "1"] and counters(a[6]) == (2, 1, 1)             # a larger one: one free and one allocation
    assert int(a[7][0]) != 0 and a[7][1] == "4096"


def test_lookups_neither_insert_nor_throw(driver):
    a = ask(driver, ["get nothing", "ensure buf 64", "get nothing", "get nothing", "get buf"])
    assert a[0][:4] == ["0", "0", "0", "0"] and counters(a[0]) == (0, 0, 0)   # get() nullptr, bytes() 0, find() nullptr; still no entry
    assert a[2][:4] == ["0", "0", "0", "0"] and counters(a[2]) == (1, 0, 1)
    assert counters(a[3]) == (1, 0, 1)
    assert int(a[4][0]) != 0 and a[4][1:4] == ["64", "1", "1"]                # and the entry that exists is untouched


def test_a_failed_allocation_leaves_no_trace(driver):
    """The partial failure that `!count(first) && (alloc(first) || alloc(second) || ..)` got wrong: the second of three allocations fails; the next
    call must allocate what is missing instead of finding the first name and skipping the rest."""
    lst = "ensure_all 3 hex 4096 grp_cnt 132 ioc_err 4"
    a = ask(driver, ["fail_at 2", lst, "get hex", "get grp_cnt", "get ioc_err", lst, "get hex", "get grp_cnt", "get ioc_err", lst])
    assert a[1][0] != "0" and a[1][1] == "grp_cnt" and counters(a[1]) == (1, 0, 1)      # non-zero, names the second; only the first is held
    hex0 = int(a[2][0])
    assert hex0 != 0
    assert a[3][:4] == ["0", "0", "0", "0"] and a[4][:4] == ["0", "0", "0", "0"]        # never a pointer for a name whose allocation failed
    assert counters(a[4]) == (1, 0, 1)                                                  # (and asking did not create them)
    assert a[5][:2] == ["0", "-"] and counters(a[5]) == (3, 0, 3)                       # healthy allocator: exactly the two missing ones
    assert int(a[6][0]) == hex0                                                         # the survivor did not move
    assert int(a[7][0]) != 0 and a[7][1] == "132" and int(a[8][0]) != 0 and a[8][1] == "4"
    assert a[9][:2] == ["0", "-"] and counters(a[9]) == (3, 0, 3)                       # and a third call allocates nothing


def test_a_failed_growth_leaves_no_trace_either(driver):
    a = ask(driver, ["ensure buf 64", "fail_at 1", "ensure buf 128", "get buf", "ensure buf 128", "get buf"])
    assert a[2][0] != "0" and a[2][1] == "0" and counters(a[2]) == (1, 1, 0)            # the old buffer is gone, the name with it
    assert a[3][:4] == ["0", "0", "0", "0"]
    assert a[4][:2] == ["0", "1"] and counters(a[4]) == (2, 1, 1)                       # the retry allocates
    assert int(a[5][0]) != 0 and a[5][1] == "128"


def test_release_all_frees_exactly_what_was_allocated(driver):
    a = ask(driver, ["ensure_all 3 a 16 b 32 c 64", "ensure b 1024", "fail_at 1", "ensure d 8", "release_all", "get a", "ensure a 16", "release_all"])
    assert counters(a[1]) == (4, 1, 3)
    assert a[3][0] != "0" and counters(a[3]) == (4, 1, 3)
    assert counters(a[4]) == (4, 4, 0)                                                  # allocations - frees = 0, no entry left
    assert a[5][:4] == ["0", "0", "0", "0"]
    assert a[6][:2] == ["0", "1"] and counters(a[6]) == (5, 4, 1)                       # usable afterwards
    assert counters(a[7]) == (5, 5, 0)


def test_zero_bytes_holds_a_pointer_of_recorded_size_zero(driver):
    a = ask(driver, ["ensure empty 0", "get empty", "ensure empty 0"])
    assert a[0][:2] == ["0", "1"] and counters(a[0]) == (1, 0, 1)
    assert int(a[1][0]) != 0 and a[1][1:4] == ["0", "1", "1"]
    assert a[2][:2] == ["0", "0"] and counters(a[2]) == (1, 0, 1)
