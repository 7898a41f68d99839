// kernels_rng.hip -- the device generator (philox.h; desire_set_rng / desire_rng_fill) and the twins of the three kernels that read eps.
//
// A latent normal is a pure function of (seed, draw, global window, k, global slot, latent): the twins compute it where k_reparam (kernels_gemm.hip),
// k_reparam_c (kernels_compact.hip) and k_reparam_bwd (kernels_bwd.hip) read eps[r, l], with the same arithmetic around it, so a twin's output is
// bit-identical to its original's on the eps that k_reparam_rng writes in prior mode (desire_rng_fill, kind 2: the same device function).  One lane
// handles whole Philox blocks: four latents, one float4 of every operand.  All VALU (about 100 operations per four normals), no LDS, no atomics.
// Whether a * b + c is one rounding or two is the compiler's choice in the originals (the tree builds with its default contraction); the twins spell
// out the choice it makes there -- fmaf where it fuses, contraction off around the rest -- because bit-identity with the originals is their contract
// (tests/test_gpu_rng.py holds it: Y, score and the flat gradient buffer).
//
// rng_state (four device words, allocated by desire_set_rng): next, used, seed_lo, seed_hi.  k_rng_begin moves the draw counter ON THE DEVICE, so a
// replayed hipGraph draws fresh noise; a re-seed is a kernel too (kernels_aux.hip on memset nodes in graph replay).
#include "common.h"
#include "kernels.h"
#include "philox.h"

__global__ void k_rng_set(uint32_t* __restrict__ st, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { st[0] = draw; st[1] = draw; st[2] = seed_lo; st[3] = seed_hi; }
}
void launch_rng_set(uint32_t* st, uint64_t seed, uint32_t draw, hipStream_t s) {
    hipLaunchKernelGGL(k_rng_set, dim3(1), dim3(64), 0, s, st, (uint32_t)seed, (uint32_t)(seed >> 32), draw);
}
// one thread: used = next; next += 1
__global__ void k_rng_begin(uint32_t* __restrict__ st) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { const uint32_t n = st[0]; st[1] = n; st[0] = n + 1u; }
}
void launch_rng_begin(uint32_t* st, hipStream_t s) { hipLaunchKernelGGL(k_rng_begin, dim3(1), dim3(64), 0, s, st); }

static inline unsigned rng_grid(long n) { const long b = (n + 255) / 256; return (unsigned)(b < 8192 ? (b < 1 ? 1 : b) : 8192); }
#define RNG_FOR(i, total) for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)(total); i += (long)gridDim.x * blockDim.x)

// ---- the stand-alone fill: out[e - first] = word / normal (e & 3) of block e >> 2 of stream `stream_id`, first <= e < first + n ----------------
__global__ void k_rng_fill(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream_id, uint64_t first, int normals, uint32_t* __restrict__ out, uint64_t n) {
    const uint64_t b0 = first >> 2, nb = ((first + n + 3) >> 2) - b0;
    RNG_FOR(t, nb) {
        const uint64_t b = b0 + (uint64_t)t;
        const Philox4 x = philox4x32_10(philox_fill_counter(stream_id, b), seed_lo, seed_hi);
        float nrm[4];
        if (normals) philox_normal4(x, nrm);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t e = 4 * b + j;
            if (e >= first && e - first < n) out[e - first] = normals ? __float_as_uint(nrm[j]) : x.v[j];
        }
    }
}
void launch_rng_fill(uint64_t seed, uint32_t stream_id, uint64_t first, int normals, void* out, uint64_t n, hipStream_t s) {
    if (n == 0) return;
    const uint64_t nb = ((first + n + 3) >> 2) - (first >> 2);
    hipLaunchKernelGGL(k_rng_fill, dim3(rng_grid((long)nb)), dim3(256), 0, s, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, first, normals,
                       static_cast<uint32_t*>(out), n);
}

__device__ __forceinline__ float4 reparam4(const float* __restrict__ params, size_t a, int L, int l, const float e[4]) {
    const float4 mu = *reinterpret_cast<const float4*>(params + a * 2 * L + l), ls = *reinterpret_cast<const float4*>(params + a * 2 * L + L + l);
    float4 z;                                            // k_reparam: mu + sd * eps is one fma
    z.x = fmaf(sqrtf(expf(ls.x)), e[0], mu.x);
    z.y = fmaf(sqrtf(expf(ls.y)), e[1], mu.y);
    z.z = fmaf(sqrtf(expf(ls.z)), e[2], mu.z);
    z.w = fmaf(sqrtf(expf(ls.w)), e[3], mu.w);
    return z;
}

// ---- k_reparam's twin: z[r, 4b .. 4b + 3], r = (scene * K + k) * mno + slot.  posterior == 0: z = eps, which is also the explicit eps tensor ------
__global__ void k_reparam_rng(const float* __restrict__ params, RngArgs g, float* __restrict__ z, int R, int L, int K, int mno, int posterior) {
    const int L4 = L >> 2;
    const RngKey key = rng_key(g);
    RNG_FOR(i, (long)R * L4) {
        const int r = (int)(i / L4), l = (int)(i - (long)r * L4) << 2;
        const int sk = r / mno, slot = r - sk * mno, sc = sk / K, k = sk - sc * K;
        float e[4];
        philox_eps4(key.lo, key.hi, key.draw, g.scene_base + (uint32_t)sc, (uint32_t)k, g.slot_base + (uint32_t)slot, (uint32_t)l, e);
        float4 o = make_float4(e[0], e[1], e[2], e[3]);
        if (posterior) o = reparam4(params, (size_t)sc * mno + slot, L, l, e);
        *reinterpret_cast<float4*>(z + (size_t)r * L + l) = o;
    }
}
void launch_reparam_rng(const float* params, const RngArgs& g, float* z, int R, int L, int K, int mno, int posterior, hipStream_t s) {
    const long n = (long)R * (L >> 2);
    if (n <= 0) return;
    hipLaunchKernelGGL(k_reparam_rng, dim3(rng_grid(n)), dim3(256), 0, s, params, g, z, R, L, K, mno, posterior);
}

// ---- the normals of a generating desire_rollout_samples, [R, T, 2]: one lane per Philox block = steps 2b, 2b + 1 of a row (k_rollout computes the same
// blocks with the same device function and never stores them) ----
__global__ void k_rollout_normals(RngArgs g, float* __restrict__ out, int R, int T, int K, int mno) {
    const int T2 = (T + 1) >> 1;
    const RngKey key = rng_key(g);
    RNG_FOR(i, (long)R * T2) {
        const int r = (int)(i / T2), t = (int)(i - (long)r * T2) << 1;
        const int sk = r / mno, slot = r - sk * mno, sc = sk / K, k = sk - sc * K;
        float n[4];
        philox_roll4(key.lo, key.hi, key.draw, g.scene_base + (uint32_t)sc, (uint32_t)k, g.slot_base + (uint32_t)slot, (uint32_t)t, n);
        float* o = out + ((size_t)r * T + t) * 2;
        o[0] = n[0]; o[1] = n[1];
        if (t + 1 < T) { o[2] = n[2]; o[3] = n[3]; }
    }
}
void launch_rollout_normals(const RngArgs& g, float* out, int R, int T, int K, int mno, hipStream_t s) {
    const long n = (long)R * ((T + 1) >> 1);
    if (n <= 0) return;
    hipLaunchKernelGGL(k_rollout_normals, dim3(rng_grid(n)), dim3(256), 0, s, g, out, R, T, K, mno);
}

// ---- k_reparam_c's twin: compact row r' = k * P + a' (kernels_compact.hip); the counter is the ORIGINAL (scene, k, slot) of amap[a'], never r' ----
__global__ void k_reparam_c_rng(const float* __restrict__ params_c, RngArgs g, float* __restrict__ z, const int32_t* __restrict__ amap,
                                int P, int K, int mno, int L, int posterior, const int32_t* __restrict__ dynP) {
    if (dynP) P = dynP[0];
    const int L4 = L >> 2;
    const RngKey key = rng_key(g);
    RNG_FOR(i, (long)P * K * L4) {
        const int rp = (int)(i / L4), l = (int)(i - (long)rp * L4) << 2;
        const int k = rp / P, ap = rp - k * P;
        const int a = amap[ap];
        const int sc = a / mno, slot = a - sc * mno;
        float e[4];
        philox_eps4(key.lo, key.hi, key.draw, g.scene_base + (uint32_t)sc, (uint32_t)k, g.slot_base + (uint32_t)slot, (uint32_t)l, e);
        float4 o = make_float4(e[0], e[1], e[2], e[3]);
        if (posterior) o = reparam4(params_c, (size_t)ap, L, l, e);
        *reinterpret_cast<float4*>(z + (size_t)rp * L + l) = o;
    }
}
void launch_reparam_c_rng(const float* params_c, const RngArgs& g, float* z, const int32_t* amap, int P, int K, int mno, int L, int posterior,
                          hipStream_t s, const int32_t* dynP) {
    const long n = (long)P * K * (L >> 2);
    if (n <= 0) return;
    hipLaunchKernelGGL(k_reparam_c_rng, dim3(rng_grid(n)), dim3(256), 0, s, params_c, g, z, amap, P, K, mno, L, posterior, dynP);
}

// ---- k_reparam_bwd's twin: regenerates the eps of the draw in rng_state.used, so a training step keeps no eps ---------------------------------
__global__ void k_reparam_bwd_rng(const float* __restrict__ dz, RngArgs g, const float* __restrict__ params, const uint8_t* __restrict__ valid,
                                  const float* __restrict__ nvalid, float* __restrict__ dparams, int n_scenes, int mno, int K, int L,
                                  const int32_t* __restrict__ inv, int P) {
#pragma clang fp contract(off)
    // k_reparam_bwd as compiled: its loop adds (g, g * eps) to (dmu, dls) as ONE packed add, so the product is rounded; the tail is
    // dls = fma(0.5 sd, dls, -((1 - exp(ls)) * (0.5 wv))) and dmu = fma(wv, mu, dmu)
    const int L4 = L >> 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int A = n_scenes * mno;
    if (i >= (long)A * L4) return;
    const RngKey key = rng_key(g);
    const int a = (int)(i / L4), l = (int)(i - (long)a * L4) << 2;
    const int sc = a / mno, slot = a - sc * mno;
    const float4 mu4 = *reinterpret_cast<const float4*>(params + (size_t)a * 2 * L + l), ls4 = *reinterpret_cast<const float4*>(params + (size_t)a * 2 * L + L + l);
    const float mu[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, ls[4] = {ls4.x, ls4.y, ls4.z, ls4.w};
    float dmu[4] = {0.f, 0.f, 0.f, 0.f}, dls[4] = {0.f, 0.f, 0.f, 0.f};
    const int ip = inv ? inv[a] : 0;
    if (ip >= 0)
        for (int k = 0; k < K; ++k) {
            const size_t r = ((size_t)sc * K + k) * mno + slot;
            const float4 g4 = *reinterpret_cast<const float4*>(dz + (inv ? (size_t)k * P + ip : r) * L + l);
            const float gz[4] = {g4.x, g4.y, g4.z, g4.w};
            float e[4];
            philox_eps4(key.lo, key.hi, key.draw, g.scene_base + (uint32_t)sc, (uint32_t)k, g.slot_base + (uint32_t)slot, (uint32_t)l, e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dmu[j] += gz[j];
                dls[j] += gz[j] * e[j];
            }
        }
    const float wv = valid[a] ? 1.0f / nvalid[0] : 0.f;
    float om[4], ol[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float ex = expf(ls[j]), sd = sqrtf(ex);
        om[j] = fmaf(wv, mu[j], dmu[j]);
        ol[j] = fmaf(0.5f * sd, dls[j], -((1.0f - ex) * (0.5f * wv)));
    }
    *reinterpret_cast<float4*>(dparams + (size_t)a * 2 * L + l) = make_float4(om[0], om[1], om[2], om[3]);
    *reinterpret_cast<float4*>(dparams + (size_t)a * 2 * L + L + l) = make_float4(ol[0], ol[1], ol[2], ol[3]);
}
void launch_reparam_bwd_rng(const float* dz, const RngArgs& g, const float* params, const uint8_t* valid, const float* nvalid, float* dparams,
                            int n_scenes, int mno, int K, int L, hipStream_t s, const int32_t* inv, int P) {
    const long n = (long)n_scenes * mno * (L >> 2);
    hipLaunchKernelGGL(k_reparam_bwd_rng, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dz, g, params, valid, nvalid, dparams, n_scenes, mno, K, L, inv, P);
}
