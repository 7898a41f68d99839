// ioc_tile.h -- the small pieces of an IOC tile that every kernel form (operand format, tile height, cluster or not) runs as the same
// statements, and that compile to the instructions the kernels had with their private copies.  Everything else stays in the kernels.
#pragma once
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
