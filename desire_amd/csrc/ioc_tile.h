// ioc_tile.h -- the small pieces of an IOC tile that every kernel form (operand format, tile height, cluster or not) runs as the same
// statements, and that compile to the instructions the kernels had with their private copies.  Everything else stays in the kernels.
#pragma once
#include "ioc_lds.h"

// Where the pooled operand row of one (row, bin) comes from (k_ioc, rows read in place), by the row's neighbour mask for the bin (bit j = slot j
// of the row's group): no neighbour -> the zero row; one neighbour j -> that row's h columns where they lie (h_j + 0 = h_j); two or more -> a
// sum slot.  Returns IOC_ROW_ZERO, IOC_ROW_SUM or j.  Plain C++ up to here: tests/test_ioc_pool_plan.py compiles it with g++.
constexpr int IOC_ROW_ZERO = -1, IOC_ROW_SUM = -2;
IOC_HD constexpr int ioc_row_source(unsigned m) { return m == 0u ? IOC_ROW_ZERO : (m & (m - 1u)) ? IOC_ROW_SUM : __builtin_ctz(m); }
IOC_HD constexpr int ioc_row_source(unsigned long long m) { return m == 0ull ? IOC_ROW_ZERO : (m & (m - 1ull)) ? IOC_ROW_SUM : __builtin_ctzll(m); }
// The row-source table keeps one byte per (row, bin): tile row r < TM = the h columns of that row of XH, TM = the zero row, TM + 1 + s = sum
// slot s (at most 2 TM - 1 slots: 3 TM < 256).  ioc_row_offset: the float offset from the tile's LDS base (XH) of the operand row a code stands
// for; XH rows are LDX floats with h at column E, the zero row TM holds a 16-byte slot per lane of a 16-lane group (lane15), the slots are AB's
// rows of LDB floats behind the TM + 1 rows of XH.
IOC_HD constexpr int ioc_row_offset(int code, int TM, int LDX, int E, int LDB, int lane15) {
    // (one multiply-add on two selected constants: code * LDX + E, TM * LDX + 4 * lane15, (TM + 1) * LDX + (code - TM - 1) * LDB)
    return code * (code <= TM ? LDX : LDB) + (code < TM ? E : code == TM ? 4 * lane15 : (TM + 1) * (LDX - LDB));
}

#ifdef __HIPCC__
#include "common.h"

// per-phase cycle counters of the IOC kernels (DESIRE_IOC_TIMING builds: tacc / tprev are locals of the kernel)
#ifdef DESIRE_IOC_TIMING
#define IOC_TICK(k) { const long long now_ = clock64(); tacc[k] += now_ - tprev; tprev = now_; }
#else
#define IOC_TICK(k)
#endif

// wv = [w_vel (2 x EV) | b_vel (EV)]: the velocity fc
template <int EV, int NTHR>
__device__ __forceinline__ void ioc_stage_wv(float* wv, const float* __restrict__ w_vel, const float* __restrict__ b_vel, int tid) {
    for (int i = tid; i < 3 * EV; i += NTHR) wv[i] = (i < 2 * EV) ? w_vel[i] : b_vel[i - 2 * EV];
}
// lut[nibble] = four bf16 values 0.0 / 1.0, one per bit: the 0/1 operand fragments of the pooling MFMAs
__device__ __forceinline__ void ioc_stage_lut(uint2* lut, int tid) {
    if (tid < 16) {
        const unsigned lo = ((tid & 1) ? 0x3F80u : 0u) | ((tid & 2) ? 0x3F800000u : 0u);
        const unsigned hi2 = ((tid & 4) ? 0x3F80u : 0u) | ((tid & 8) ? 0x3F800000u : 0u);
        lut[tid] = make_uint2(lo, hi2);
    }
}
// the tile's occupied-bin words occ[0..1] as one wave-uniform 64-bit mask
__device__ __forceinline__ unsigned long long ioc_occ64(const unsigned* occ) {
    unsigned long long om = (unsigned long long)__builtin_amdgcn_readfirstlane((int)occ[0]) & 0xffffffffull;
    om |= (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)occ[1]) << 32;
    return om;
}
// sum over the 32 lanes (columns) of a half wave
__device__ __forceinline__ float ioc_sum32(float v) {
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8); v += __shfl_xor(v, 16);
    return v;
}
#endif      // __HIPCC__
