// ioc_lds.h -- the dynamic-LDS layout of every IOC kernel as a plan: a list of named regions with their sizes.  The launchers and
// ioc_plan.h take bytes() from it; the kernels carve their LDS by hand (a typed pointer chain: taking the pointers from the plan changed
// their instruction streams) and tie that chain to the plan with IOC_LDS_TIED clauses, checked when the kernel is compiled.
// Plain C++ without HIP headers (ioc_plan.h includes it and is compiled with g++ by the tests).
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define IOC_HD __host__ __device__
#else
#define IOC_HD
#endif

// N consecutive regions of sz[r] bytes each, region r at off(r) of the workgroup's dynamic LDS; a region a kernel form does not have is
// empty.  The last region of every plan, SPARE, is what is left of the slack the former launch formulas added by hand ("+ TM + 64 + 256"
// and the like) once the small regions behind VLD have their own names: not a tunable, it keeps every total what it was.
template <int N>
struct IocLdsRegions {
    int sz[N] = {};
    IOC_HD constexpr int off(int r) const { int o = 0; for (int i = 0; i < r; ++i) o += sz[i]; return o; }
    IOC_HD constexpr size_t bytes() const { return (size_t)off(N); }
};
// in a kernel that carves its LDS by hand: one clause tying its pointer chain to the plan its launcher sizes the LDS by
#define IOC_LDS_TIED(cond) static_assert(cond, "hand carve-up and ioc_lds.h plan disagree: " #cond)
IOC_HD constexpr int ioc_kx(int H, int EV, int C) { return EV + C + 2 * H; }      // columns of [e_v | e_s | e_r | h]

// k_ioc, the dense pooling with rows read in place: between the position phase and the candidate the AB region holds no operand tile but
// the sums of the (row, bin) pairs with two or more neighbours, one slot of H + 4 floats each, and behind them the row-source table
// [TM][bins] of one byte per pair (ioc_tile.h: ioc_row_code; bins <= 64, the occupancy word).  The slots are what fits in front of the
// table; a tile-step with more such pairs runs the build loop, so the count is a performance choice only (tests/test_ioc_pool_plan.py)
constexpr int IOC_POOL_MAX_BINS = 64;
IOC_HD constexpr int ioc_pool_slots(int H, int TM) {
    return 2 * TM - (TM * IOC_POOL_MAX_BINS + (H + 4) * 4 - 1) / ((H + 4) * 4);
}

// fp32 operand tiles XH [rows][KX + 4] and AB [2][TM][H + 4]: k_ioc, k_ioc_cl, k_ioc_step, k_ioc_step_x2
struct IocLds : IocLdsRegions<12> {
    enum { XH, AB, MASKS, PC, PP, WV, RED, VLD, OCC, ROWBITS, ROWLIST, SPARE };         // PC = pg (the whole group's positions) in the cluster form
    // k_ioc: TM = 32 (32-bit masks) or 64 (64-bit); XH has a zero row TM; ROWBITS [36] / ROWLIST [2][TM / 4] words are the CP form's
    IOC_HD static constexpr IocLds tile(int H, int EV, int C, int TM, int bins) {
        IocLds l;
        l.sz[XH] = (TM + 1) * (ioc_kx(H, EV, C) + 4) * 4;
        l.sz[AB] = 2 * TM * (H + 4) * 4;
        l.sz[MASKS] = TM * bins * (TM == 32 ? 4 : 8);
        l.sz[PC] = TM * 8;
        l.sz[PP] = TM * 8;
        l.sz[WV] = 3 * EV * 4;
        l.sz[RED] = (H / 32) * TM * 4;
        l.sz[VLD] = TM;
        l.sz[OCC] = 8;
        l.sz[ROWBITS] = 36 * 4;
        l.sz[ROWLIST] = 2 * TM;
        l.sz[SPARE] = 168 - 2 * TM;
        return l;
    }
    // k_ioc_cl: 32-row tiles of groups of up to MAXM agents, two 64-bit mask words per (row, bin)
    IOC_HD static constexpr IocLds cluster(int H, int EV, int C, int bins, int MAXM = 128) {
        IocLds l;
        l.sz[XH] = 32 * (ioc_kx(H, EV, C) + 4) * 4;
        l.sz[AB] = 2 * 32 * (H + 4) * 4;
        l.sz[MASKS] = 32 * bins * 16;
        l.sz[PC] = MAXM * 8;
        l.sz[PP] = 32 * 8;
        l.sz[WV] = 3 * EV * 4;
        l.sz[RED] = (H / 32) * 32 * 4;
        l.sz[VLD] = MAXM;
        l.sz[OCC] = 8;
        l.sz[SPARE] = 56;
        return l;
    }
    // k_ioc_step: fp32 tiles, MW 64-bit mask words per (row, bin)
    IOC_HD static constexpr IocLds step(int H, int EV, int C, int bins, int MW) {
        IocLds l;
        l.sz[XH] = 32 * (ioc_kx(H, EV, C) + 4) * 4;
        l.sz[AB] = 2 * 32 * (H + 4) * 4;
        l.sz[MASKS] = 32 * bins * MW * 8;
        l.sz[WV] = 3 * EV * 4;
        l.sz[RED] = (H / 32) * 32 * 4;
        l.sz[OCC] = 8;
        l.sz[SPARE] = 56;
        return l;
    }
    // k_ioc_step_x2: the same step with both tiles as [hi | lo] bf16 piece images, rows of KX + 8 / H + 8 elements
    IOC_HD static constexpr IocLds step_x2(int H, int EV, int C, int bins, int MW) {
        IocLds l = step(H, EV, C, bins, MW);
        l.sz[XH] = 2 * 32 * (ioc_kx(H, EV, C) + 8) * 2;
        l.sz[AB] = 2 * 2 * 32 * (H + 8) * 2;
        return l;
    }
};

// operand tiles X, RH and the transposed state HT, 64-bit (x3: 32-bit) masks of bins + 1 words per row, the nibble table:
// k_ioc_bf16, k_ioc_bf16_cl, k_ioc_x3, k_ioc_x6r2
struct IocHtLds : IocLdsRegions<15> {
    enum { X, RH, HT, MASKS, LUT, PC, PP, WV, RED, VLD, OCC, PGV, EX, EXB, SPARE };     // PC = pg in the cluster form
    // what the four forms share behind the masks: T rows of positions, the velocity fc, the score reduction, presence of M slots
    IOC_HD constexpr void tail(int H, int EV, int T, int M) {
        sz[LUT] = 16 * 8;
        sz[PC] = M * 8;
        sz[PP] = T * 8;
        sz[WV] = 3 * EV * 4;
        sz[RED] = (H / 32) * T * 4;
        sz[VLD] = M;
        sz[OCC] = 8;
    }
    // k_ioc_bf16, TM = 32 WM: bf16 tiles; split: the partial-tile exchange EX [WM][NT][1024] floats, EXB its second set's upper half
    // (bins <= 32).  Every region in front of OCC is a multiple of 16 bytes: 8 bytes of padding (PGV here) put EX on a 16-byte boundary.
    IOC_HD static constexpr IocHtLds bf16(int H, int EV, int C, int WM, int bins, bool split) {
        const int T = 32 * WM, NT = H / 32;
        IocHtLds l;
        l.sz[X] = T * (ioc_kx(H, EV, C) + 8) * 2;
        l.sz[RH] = T * (H + 8) * 2;
        l.sz[HT] = H * (T + 8) * 2;
        l.sz[MASKS] = T * (bins + 1) * 8;
        l.tail(H, EV, T, T);
        l.sz[PGV] = split ? 8 : 0;
        l.sz[EX] = split ? WM * NT * 4096 : 0;
        l.sz[EXB] = split && bins <= 32 ? WM * NT * 2048 : 0;
        l.sz[SPARE] = split ? 64 : 56;
        return l;
    }
    // k_ioc_bf16_cl: HT holds the whole group (MAXM columns), two mask words per (row, bin); PGV = the positions again with NaN for absent
    // agents.  Its exchange sets alias HT.
    IOC_HD static constexpr IocHtLds bf16_cluster(int H, int EV, int C, int bins, int MAXM = 128) {
        IocHtLds l;
        l.sz[X] = 32 * (ioc_kx(H, EV, C) + 8) * 2;
        l.sz[RH] = 32 * (H + 8) * 2;
        l.sz[HT] = H * (MAXM + 8) * 2;
        l.sz[MASKS] = 32 * (bins + 1) * 16;
        l.tail(H, EV, 32, MAXM);
        l.sz[PGV] = MAXM * 8;
        l.sz[SPARE] = 64;
        return l;
    }
    // k_ioc_x3: NP piece images per tile, 32-bit masks padded to an even word count.  Exchange set 0 aliases HT, set 1 RH.
    IOC_HD static constexpr IocHtLds x3(int H, int EV, int C, int NP, int bins) {
        IocHtLds l;
        l.sz[X] = NP * 32 * (ioc_kx(H, EV, C) + 8) * 2;
        l.sz[RH] = NP * 32 * (H + 8) * 2;
        l.sz[HT] = NP * H * (32 + 8) * 2;
        l.sz[MASKS] = ((32 * (bins + 1) + 1) & ~1) * 4;
        l.tail(H, EV, 32, 32);
        l.sz[SPARE] = 8;
        return l;
    }
    // k_ioc_x6r2: 64-row fp32 tiles.  Both exchange sets alias HT (set 1 at + NT * 4096 bytes).
    IOC_HD static constexpr IocHtLds x6r2(int H, int EV, int C, int bins) {
        IocHtLds l;
        l.sz[X] = 64 * (ioc_kx(H, EV, C) + 4) * 4;
        l.sz[RH] = 64 * (H + 4) * 4;
        l.sz[HT] = H * (64 + 4) * 4;
        l.sz[MASKS] = 64 * (bins + 1) * 8;
        l.tail(H, EV, 64, 64);
        l.sz[SPARE] = 56;
        return l;
    }
};

// BPTT: three operand tiles (A2 = two tiles of H + 4 columns), neighbour and observer masks: k_ioc_bwd, k_ioc_bwd_x3, k_ioc_bwd_cl
struct IocBwdLds : IocLdsRegions<14> {
    enum { A1, A2, A3, MASKS, OBS, PC, DSC, WSC, VLD, OCC, ROWBITS, ROWLIST, LUT, SPARE };   // PC = pg in the cluster form
    // what the three forms share: tiles of T rows, mw mask bytes per (row, bin), positions and presence of M slots
    IOC_HD constexpr void common(int H, int T, int bins, int mw, int M) {
        sz[A1] = T * (H + 4) * 4;
        sz[A2] = 2 * T * (H + 4) * 4;
        sz[MASKS] = T * bins * mw;
        sz[OBS] = T * bins * mw;
        sz[PC] = M * 8;
        sz[DSC] = T * 4;
        sz[WSC] = H * 4;
        sz[VLD] = M;
        sz[OCC] = 8;
    }
    // k_ioc_bwd: ROWBITS [36] words and ROWLIST, 32 bytes per wave, are the packed dpool's (CPB: 32-row tiles, H <= 128)
    IOC_HD static constexpr IocBwdLds tile(int H, int TM, int bins) {
        IocBwdLds l;
        l.common(H, TM, bins, TM == 32 ? 4 : 8, TM);
        l.sz[A3] = TM * (H + 4) * 4;
        l.sz[ROWBITS] = 36 * 4;
        l.sz[ROWLIST] = TM == 32 && H <= 128 ? (H / 32) * 32 : 0;
        l.sz[SPARE] = 424 - l.sz[ROWLIST];
        return l;
    }
    // k_ioc_bwd_x3: A3 = the [hi | lo] images [2][32][H + 8] of da_c / dpre_r; LUT = the nibble table
    IOC_HD static constexpr IocBwdLds x3(int H, int bins) {
        IocBwdLds l;
        l.common(H, 32, bins, 4, 32);
        l.sz[A3] = 2 * 32 * (H + 8) * 2;
        l.sz[LUT] = 16 * 8;
        l.sz[SPARE] = 56;
        return l;
    }
    // k_ioc_bwd_cl: A3 = GD, dpre_r of the whole group [MAXM][H + 4]; two mask words per (row, bin)
    IOC_HD static constexpr IocBwdLds cluster(int H, int bins, int MAXM = 128) {
        IocBwdLds l;
        l.common(H, 32, bins, 16, MAXM);
        l.sz[A3] = MAXM * (H + 4) * 4;
        l.sz[SPARE] = 64;
        return l;
    }
};
