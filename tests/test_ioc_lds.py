"""The LDS plans of the IOC kernels (desire_amd/csrc/ioc_lds.h): every launcher -- and ioc_plan.h -- takes the byte count from the kernel's plan,
and the kernels' hand carve-ups are tied to the plans by static_asserts.  tests/c_host/ioc_lds_driver.cpp is compiled against the header with g++ and asked for the plans of a sweep of
shapes.  The SPEC functions below are the launch formulas the launchers held before the plans existed, transcribed as they stood: the plans
must not change a single total."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "c_host", "ioc_lds_driver.cpp")
LIMIT = 160 * 1024
EV, C, MAXM = 16, 32, 128
IOC16_SPLIT = 1                # bf16.h


# ---- the former launch formulas (bytes) ----
def spec_tile(H, TM, B):                                   # ioc_lds_bytes (k_ioc)
    NT, E = H // 32, EV + 32 + H
    LDX, LDB = E + H + 4, H + 4
    f = (TM + 1) * LDX + 2 * TM * LDB + TM * B * (1 if TM == 32 else 2) + TM * 4 + 3 * EV + NT * TM
    return f * 4 + TM + 64 + 256


def spec_tile_planner(H, B):                               # the copy ioc_uses_cluster held (64-row tile): 256 bytes short of the launcher's
    return (65 * (2 * H + 52) + 2 * 64 * (H + 4) + 64 * 4 + 48 + (H // 32) * 64) * 4 + 64 * B * 8 + 128


def spec_cluster(H, B):                                    # ioc_cl_lds_bytes (k_ioc_cl)
    NT, E, TM = H // 32, EV + 32 + H, 32
    LDX, LDB = E + H + 4, H + 4
    f = TM * LDX + 2 * TM * LDB + TM * B * 4 + 128 * 2 + TM * 2 + 3 * EV + NT * TM
    return f * 4 + 128 + 64


def spec_step(H, B, MW):                                   # ioc_step_lds (k_ioc_step)
    NT, E, TM = H // 32, EV + 32 + H, 32
    LDX, LDB = E + H + 4, H + 4
    return (TM * LDX + 2 * TM * LDB + TM * B * MW * 2 + 3 * EV + NT * TM) * 4 + 64


def spec_step_x2(H, B, MW):                                # ioc_step_x2_lds (k_ioc_step_x2)
    NT, TM = H // 32, 32
    KX = EV + 32 + 2 * H
    return 2 * TM * (KX + 8) * 2 + 2 * 2 * TM * (H + 8) * 2 + TM * B * MW * 8 + (3 * EV + NT * TM) * 4 + 64


def spec_bf16(H, WM, B):                                   # ioc16_lds (k_ioc_bf16)
    TM, NT = 32 * WM, H // 32
    KX = 16 + 32 + 2 * H
    b = TM * (KX + 8) * 2 + TM * (H + 8) * 2 + H * (TM + 8) * 2
    b += TM * (B + 1) * 8 + 16 * 8 + TM * 4 * 4 + 3 * 16 * 4 + NT * TM * 4 + TM + 64
    if IOC16_SPLIT and NT <= 4:
        b += WM * NT * 4096 + 16 + (WM * NT * 2048 if B <= 32 else 0)
    return b


def spec_bf16_cluster(H, B):                               # ioc16_cl_lds (k_ioc_bf16_cl)
    TM, NT = 32, H // 32
    KX = 16 + 32 + 2 * H
    b = TM * (KX + 8) * 2 + TM * (H + 8) * 2 + H * (MAXM + 8) * 2
    return b + TM * (B + 1) * 16 + 16 * 8 + MAXM * 2 * 4 + TM * 2 * 4 + 3 * 16 * 4 + NT * TM * 4 + MAXM + 8 + MAXM * 8 + 64


def spec_x3(H, NP, B):                                     # iocx3_lds (k_ioc_x3)
    TM, NT = 32, H // 32
    KX = 16 + 32 + 2 * H
    b = NP * (TM * (KX + 8) * 2 + TM * (H + 8) * 2 + H * (TM + 8) * 2)
    return b + ((TM * (B + 1) + 1) & ~1) * 4 + 16 * 8 + TM * 4 * 4 + 3 * 16 * 4 + NT * TM * 4 + TM + 16


def spec_x6r2(H, B):                                       # iocx6r2_lds (k_ioc_x6r2)
    TM, NT = 64, H // 32
    KX = 16 + 32 + 2 * H
    b = (TM * (KX + 4) + TM * (H + 4) + H * (TM + 4)) * 4
    return b + TM * (B + 1) * 8 + 16 * 8 + TM * 4 * 4 + 3 * 16 * 4 + NT * TM * 4 + TM + 64


def spec_x6r2_planner(H, B):                               # the copy ioc_x6r2_supported held
    KX, NT = 16 + 32 + 2 * H, H // 32
    return (64 * (KX + 4) + 64 * (H + 4) + H * 68) * 4 + 64 * (B + 1) * 8 + 128 + 1024 + 192 + NT * 256 + 128


def spec_bwd_tile(H, TM, B):                               # ioc_bwd_lds (k_ioc_bwd)
    LD1 = H + 4
    f = TM * LD1 * 4 + TM * B * (2 if TM == 32 else 4) + TM * 2 + TM + H
    return f * 4 + TM + 64 + 512


def spec_bwd_x3(H, B):                                     # the formula inside launch_ioc_bwd_x3_t (k_ioc_bwd_x3)
    return 32 * (H + 4) * 3 * 4 + 2 * 32 * (H + 8) * 2 + 2 * 32 * B * 4 + (32 * 2 + 32 + H) * 4 + 32 + 64 + 16 * 8


def spec_bwd_cluster(H, B):                                # ioc_bwd_cl_lds (k_ioc_bwd_cl)
    LD1, TM = H + 4, 32
    f = TM * LD1 + 2 * TM * LD1 + MAXM * LD1 + MAXM * 2 + TM + H
    return f * 4 + 4 * TM * B * 8 + MAXM + 8 + 64


# ---- plans: region names in layout order, and the alignment each region's accesses need: 16 = float4 / b128 tiles, 8 = 64-bit mask words and
# the float2 / uint2 arrays, 4 = words, 1 = bytes.  "M" = the mask word of the form (4 or 8 bytes). ----
R_IOC = ["XH", "AB", "MASKS", "PC", "PP", "WV", "RED", "VLD", "OCC", "ROWBITS", "ROWLIST", "SPARE"]
A_IOC = {"XH": 16, "AB": 16, "MASKS": "M", "PC": 8, "PP": 8, "WV": 4, "RED": 4, "VLD": 1, "OCC": 4, "ROWBITS": 4, "ROWLIST": 4, "SPARE": 1}
R_HT = ["X", "RH", "HT", "MASKS", "LUT", "PC", "PP", "WV", "RED", "VLD", "OCC", "PGV", "EX", "EXB", "SPARE"]
A_HT = {"X": 16, "RH": 16, "HT": 16, "MASKS": "M", "LUT": 8, "PC": 8, "PP": 8, "WV": 4, "RED": 4, "VLD": 1, "OCC": 4, "PGV": 8, "EX": 16, "EXB": 16,
        "SPARE": 1}
R_BWD = ["A1", "A2", "A3", "MASKS", "OBS", "PC", "DSC", "WSC", "VLD", "OCC", "ROWBITS", "ROWLIST", "LUT", "SPARE"]
A_BWD = {"A1": 16, "A2": 16, "A3": 16, "MASKS": "M", "OBS": "M", "PC": 8, "DSC": 4, "WSC": 4, "VLD": 1, "OCC": 4, "ROWBITS": 4, "ROWLIST": 1, "LUT": 8,
         "SPARE": 1}

HS, GS = (64, 128, 256), (1, 2, 3, 4, 5, 6)


def requests():
    """(request line, region names, alignments, mask word bytes, the former formula's bytes, documented aliases [(host region, bytes)])"""
    out = []
    for H in HS:
        NT = H // 32
        for G in GS:
            B = G * G
            for TM in (32, 64):                            # TRAIN / CP / NSPL / PAD instantiations share the layout of their tile height
                out.append((f"lds tile {H} {TM} {B} 0 0 0", R_IOC, A_IOC, 4 if TM == 32 else 8, spec_tile(H, TM, B), []))
                out.append((f"lds bwd_tile {H} {TM} {B} 0 0 0", R_BWD, A_BWD, 4 if TM == 32 else 8, spec_bwd_tile(H, TM, B),
                            [("A2", 32 * (2 * 32 + 4) * 4)]))                   # DR (T_pred <= 32 here) inside A2
                WM = TM // 32
                split = int(IOC16_SPLIT and NT <= 4)
                out.append((f"lds bf16 {H} {TM} {B} 0 0 {split}", R_HT, A_HT, 8, spec_bf16(H, WM, B), []))
            out.append((f"lds cluster {H} 32 {B} 0 0 0", R_IOC, A_IOC, 8, spec_cluster(H, B), []))           # groups of 64 / 96 / 128: one layout (MAXM)
            out.append((f"lds bf16_cluster {H} 32 {B} 0 0 0", R_HT, A_HT, 8, spec_bf16_cluster(H, B), [("HT", 2 * NT * 4096)]))
            out.append((f"lds bwd_cluster {H} 32 {B} 0 0 0", R_BWD, A_BWD, 8, spec_bwd_cluster(H, B), [("A2", 32 * (2 * 32 + 4) * 4)]))
            for MW in (1, 2, 3, 4):                        # scenes of up to 64 / 128 / 192 / 256 agents
                out.append((f"lds step {H} 32 {B} 0 {MW} 0", R_IOC, A_IOC, 8, spec_step(H, B, MW), []))
                out.append((f"lds step {H} 32 {B} 2 {MW} 1", R_IOC, A_IOC, 8, spec_step_x2(H, B, MW), []))
            if H <= 128:
                for NP in (2, 3):
                    out.append((f"lds x3 {H} 32 {B} {NP} 0 0", R_HT, A_HT, 4, spec_x3(H, NP, B), [("HT", NT * 4096), ("RH", NT * 4096)]))
                out.append((f"lds x6r2 {H} 64 {B} 0 0 0", R_HT, A_HT, 8, spec_x6r2(H, B), [("HT", 2 * NT * 4096)]))   # NP = 2 / 3: one layout
                out.append((f"lds bwd_x3 {H} 32 {B} 0 0 0", R_BWD, A_BWD, 4, spec_bwd_x3(H, B), [("A2", 32 * (2 * 32 + 4) * 4)]))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ioc_lds") / "ioc_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "desire_amd", "csrc"), DRIVER, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(driver, lines):
    r = subprocess.run([driver], input="".join(x + "\n" for x in lines), capture_output=True, text=True, check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def test_plans_match_the_former_formulas_and_are_well_formed(driver):
    reqs = requests()
    for (line, names, align, mword, spec, aliases), got in zip(reqs, ask(driver, [r[0] for r in reqs])):
        v = [int(x) for x in got.split()]
        n, off, total = v[0], v[1:-1], v[-1]
        assert n == len(names) and len(off) == n + 1, line
        assert total == off[-1] == spec, (line, total, spec)                   # bytes() = the former launch formula
        assert off[0] == 0 and all(a <= b for a, b in zip(off, off[1:])), (line, off)      # ascending, back to back: no overlap
        size = {nm: off[i + 1] - off[i] for i, nm in enumerate(names)}
        for i, nm in enumerate(names):
            a = mword if align[nm] == "M" else align[nm]
            assert size[nm] == 0 or off[i] % a == 0, (line, nm, off[i], a)
        for host, nbytes in aliases:                                            # the documented aliases lie inside their host region
            assert nbytes <= size[host], (line, host, nbytes, size[host])
        if "ROWBITS" in size and size["ROWBITS"]:
            assert size["ROWBITS"] >= 36 * 4, line                              # one word per bin, up to 36 bins


def test_planner_decides_as_its_former_copies_did(driver):
    """ioc_plan.h held its own copies of two formulas.  The 64-row k_ioc one was 256 bytes short of the launcher's; ioc_uses_cluster and
    ioc_x6r2_supported, which now ask the plans, must decide as those copies did for every bin count."""
    cases = [(H, B) for H in HS for B in range(1, 400)]
    for (H, B), got in zip(cases, ask(driver, [f"fits {H} {B}" for H, B in cases])):
        uses_cluster, x6r2_ok = (int(x) for x in got.split())
        assert uses_cluster == int(H == 256 or spec_tile_planner(H, B) > LIMIT), (H, B)
        assert x6r2_ok == int(H in (64, 128) and spec_x6r2_planner(H, B) <= LIMIT), (H, B)


FWD_PLAN = {       # forward family -> (request, former formula)
    "FP32": lambda H, B, mno: (f"lds tile {H} 32 {B} 0 0 0", spec_tile(H, 32, B)),
    "FP32_WIDE": lambda H, B, mno: (f"lds tile {H} 64 {B} 0 0 0", spec_tile(H, 64, B)),
    "FP32_CLUSTER": lambda H, B, mno: (f"lds cluster {H} 32 {B} 0 0 0", spec_cluster(H, B)),
    "BF16": lambda H, B, mno: (f"lds bf16 {H} 32 {B} 0 0 {int(H <= 128)}", spec_bf16(H, 1, B)),
    "BF16_WIDE": lambda H, B, mno: (f"lds bf16 {H} 64 {B} 0 0 {int(H <= 128)}", spec_bf16(H, 2, B)),
    "BF16_CLUSTER": lambda H, B, mno: (f"lds bf16_cluster {H} 32 {B} 0 0 0", spec_bf16_cluster(H, B)),
    "X3": lambda H, B, mno: (f"lds x3 {H} 32 {B} 2 0 0", spec_x3(H, 2, B)),
    "X6": lambda H, B, mno: (f"lds x3 {H} 32 {B} 3 0 0", spec_x3(H, 3, B)),
    "X3R2": lambda H, B, mno: (f"lds x6r2 {H} 64 {B} 0 0 0", spec_x6r2(H, B)),
    "X6R2": lambda H, B, mno: (f"lds x6r2 {H} 64 {B} 0 0 0", spec_x6r2(H, B)),
}


def test_every_routed_shape_fits_160_kb(driver):
    """Every shape of the sweep that ioc_plan() routes to a family fits that family's kernel into 160 KB, but for the shapes named in
    NEVER_FITTED below, which never did."""
    shapes = [(bf16, tr, H, G, mno) for bf16 in (0, 1, 2, 3) for tr in (0, 1) for H in HS for G in GS for mno in (1, 2, 4, 8, 16, 32, 64, 96, 128)
              if not (tr and bf16 in (1, 3))]                                   # training: fp32 or two-piece operands only
    routes = ask(driver, [f"route {b} {t} {H} {G} {m}" for b, t, H, G, m in shapes])
    reqs, meta = [], []
    for (bf16, tr, H, G, mno), route in zip(shapes, routes):
        fwd, bwd, uses_cluster, x6r2_ok = route.split()
        B = G * G
        assert int(uses_cluster) == int(mno > 64 or (mno == 64 and (H == 256 or spec_tile(H, 64, B) > LIMIT)))
        assert int(x6r2_ok) == int(H in (64, 128) and (32 % mno == 0 or mno == 64) and spec_x6r2(H, B) <= LIMIT)
        if fwd == "STEPWISE":
            MW = (mno + 63) // 64
            np_ = 2 if bf16 == 2 else 3 if bf16 == 3 else 0
            req = (f"lds step {H} 32 {B} {np_} {MW} {int(np_ == 2)}", spec_step_x2(H, B, MW) if np_ == 2 else spec_step(H, B, MW))
        else:
            req = FWD_PLAN[fwd](H, B, mno)
        reqs.append(req)
        meta.append((bf16, tr, H, G, mno, fwd))
        if tr:
            reqs.append((f"lds bwd_x3 {H} 32 {B} 0 0 0", spec_bwd_x3(H, B)) if bwd == "X3" else
                        (f"lds bwd_cluster {H} 32 {B} 0 0 0", spec_bwd_cluster(H, B)) if bwd == "CLUSTER" else
                        (f"lds bwd_tile {H} {64 if mno > 32 else 32} {B} 0 0 0", spec_bwd_tile(H, 64 if mno > 32 else 32, B)))
            meta.append((bf16, tr, H, G, mno, "bwd " + bwd))
    # bf16 operands, H = 256, 64 agents, 36 bins: ioc_plan() routes it to BF16_WIDE, whose tile has always been 165 824 B -- the launch cannot
    # fit.  Changing the route is a change of behaviour of its own (it needs its own test on a GPU); the shape is left out here by name.
    NEVER_FITTED = {(1, 0, 256, 6, 64, "BF16_WIDE"): 165824}
    # The cluster BPTT at H = 256 (groups of 64 / 96 / 128 agents, fp32 or two-piece training): k_ioc_bwd_cl keeps dpre_r of the whole group
    # in LDS and exceeds 160 KB for every bin count; launch_ioc_bwd_cluster has always refused these shapes (it serves H = 64 / 128 only).
    BWD_CL_256 = {1: 236360, 2: 239432, 3: 244552, 4: 251720, 5: 260936, 6: 272200}          # by grid_size
    NEVER_FITTED.update({(b, 1, 256, G, m, "bwd CLUSTER"): n for b in (0, 2) for m in (64, 96, 128) for G, n in BWD_CL_256.items()})
    for (line, spec), m, got in zip(reqs, meta, ask(driver, [r[0] for r in reqs])):
        total = int(got.split()[-1])
        assert total == spec, (m, line)
        if m in NEVER_FITTED:
            assert total == NEVER_FITTED[m], (m, line, total)
            continue
        assert total <= LIMIT, (m, line, total)
