// kernels_scene.hip -- gradient of the training loss with respect to the scene feature grids (desire_set_option(h, "scene_grad", 1)).
//
// The IOC reads x_t = [e_v | e_s | e_r] with e_s = grid[grid_of_scene[scene]][cell(Y_in[r, t])][0:C] (kernels_rnn.hip, P1).  Its BPTT leaves
// the gate gradients of every (row, step) of a pass in ioc_dag [R*T, 2H] / ioc_dac [R*T, H], so per pass
//     ds[(r,t), 0:C] = dag[(r,t), :] . Wg[E_v + c, :]^T + dac[(r,t), :] . Wc[E_v + c, :]^T          (k_scene_ds, fp32 MFMA)
// and d loss / d grid[g, cell, :] = the sum of the ds rows whose (grid, cell) key is (g, cell).  That sum is taken WITHOUT float atomics, so the
// result is bitwise reproducible: a stable radix sort of the row indices by key, fixed chunks of the sorted order summed in order by one
// 32-lane group each (k_scene_chunks: positions crowd into few cells, so one destination can own most rows), and per destination the chunk
// partials added in chunk order (k_scene_final).
#include "kernels.h"
#include "common.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int SG_C = 32;          // scene channels (dims.C: the instantiated IOC width)
constexpr int SG_CHUNK = 256;     // sorted positions one 32-lane group sums

// Wcat[k][c], k < 2H: Wg[E_v + c][k]; 2H <= k < 3H: Wc[E_v + c][k - 2H] (natural layouts, read from the master weights)
__global__ void k_scene_wcat(const float* __restrict__ Wg, const float* __restrict__ Wc, int H, int Ev, float* __restrict__ wcat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * H * SG_C) return;
    const int k = i / SG_C, c = i - k * SG_C;
    wcat[i] = k < 2 * H ? Wg[(size_t)(Ev + c) * 2 * H + k] : Wc[(size_t)(Ev + c) * H + (k - 2 * H)];
}

// One wave per 32-row tile of the (r, t) rows: ds = [dag | dac] . Wcat on v_mfma_f32_32x32x2_f32.  Each lane loads 4 consecutive k of its
// row (float4) and feeds them to 4 MFMAs: MFMA j takes k = kb + j from lane half 0 and k = kb + 4 + j from half 1, for A and B alike (the
// order of the k terms is fixed, so the result is deterministic).  Lanes 0..31 also write the row's sort key and index.
__global__ __launch_bounds__(256) void k_scene_ds(SceneDsArgs a) {
    const int lane = threadIdx.x & 63;
    const long n = (long)a.R * a.T;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long row0 = tile * 32;
    if (row0 >= n) return;
    const int i = lane & 31, hf = lane >> 5, H = a.H;
    const long my_row = min(row0 + i, n - 1);
    const float* ag = a.dag + (size_t)my_row * 2 * H + 4 * hf;
    const float* ac = a.dac + (size_t)my_row * H + 4 * hf;
    const float* bw = a.wcat + (size_t)(4 * hf) * SG_C + i;
    f32x16 acc = zero16();
    for (int kb = 0; kb < 2 * H; kb += 8) {
        const float4 x = *reinterpret_cast<const float4*>(ag + kb);
        const float* b = bw + (size_t)kb * SG_C;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, b[SG_C], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, b[2 * SG_C], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, b[3 * SG_C], acc, 0, 0, 0);
    }
    for (int kb = 0; kb < H; kb += 8) {
        const float4 x = *reinterpret_cast<const float4*>(ac + kb);
        const float* b = bw + (size_t)(2 * H + kb) * SG_C;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, b[SG_C], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, b[2 * SG_C], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, b[3 * SG_C], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long row = row0 + (r & 3) + 8 * (r >> 2) + 4 * hf;
        if (row < n) a.ds[(size_t)row * SG_C + i] = acc[r];
    }
    if (hf == 0 && row0 + i < n) {
        const long q = row0 + i;
        const int r = (int)(q / a.T);
        uint32_t key = (uint32_t)a.n_keys;                       // padding rows of a padded class tile: sorted past every real key
        if (ioc_agent_of_row(r, a.K, a.mno, a.gpt, a.ngrp) >= 0) {
            const int scene = a.gpt ? ((r >> 5) * a.gpt + (r & 31) / a.mno) / a.K : r / (a.K * a.mno);
            int cy, cx;
            scene_cell_dev(a.Y[q * 2], a.Y[q * 2 + 1], a.Gh, a.Gw, cy, cx);
            key = (uint32_t)((a.gos[scene] * a.Gh + cy) * a.Gw + cx);
        }
        a.keys[q] = key;
        a.idx[q] = (int32_t)q;
    }
}

// beg[k] / end[k]: the range of key k in the sorted order (both stay 0 for a key no row has)
__global__ void k_scene_bounds(const uint32_t* __restrict__ keys, long n, uint32_t n_keys, int32_t* __restrict__ beg, int32_t* __restrict__ end) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k >= n_keys) return;
    if (i == 0 || keys[i - 1] != k) beg[k] = (int32_t)i;
    if (i == n - 1 || keys[i + 1] != k) end[k] = (int32_t)(i + 1);
}

// One 32-lane group per SG_CHUNK sorted positions, lane c = channel c: the ds rows of each run of equal keys inside the chunk are summed in
// sorted order and the sum is stored at the run's first position (part[pos][c]).
__global__ __launch_bounds__(256) void k_scene_chunks(const uint32_t* __restrict__ keys, const int32_t* __restrict__ idx, const float* __restrict__ ds,
                                                      long n, uint32_t n_keys, float* __restrict__ part) {
    const long grp = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    const int c = threadIdx.x & 31;
    const long p0 = grp * SG_CHUNK;
    if (p0 >= n) return;
    const long p1 = min(p0 + SG_CHUNK, n);
    uint32_t cur = keys[p0];
    if (cur >= n_keys) return;
    long seg = p0;
    float acc = 0.f;
    for (long p = p0; p < p1; p += 8) {
        uint32_t kk[8]; float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long q = min(p + j, p1 - 1);
            kk[j] = p + j < p1 ? keys[q] : n_keys;
            v[j] = ds[(size_t)idx[q] * SG_C + c];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (kk[j] != cur) {
                part[(size_t)seg * SG_C + c] = acc;
                if (kk[j] >= n_keys) return;
                cur = kk[j]; seg = p + j; acc = 0.f;
            }
            acc += v[j];
        }
    }
    part[(size_t)seg * SG_C + c] = acc;
}

// dG[k][c] (+)= the partials of key k in chunk order: the one at beg[k], then one at every chunk boundary inside [beg, end)
__global__ void k_scene_final(const int32_t* __restrict__ beg, const int32_t* __restrict__ end, const float* __restrict__ part, uint32_t n_keys,
                              float* __restrict__ dG, int accumulate) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_keys * SG_C) return;
    const long k = i / SG_C;
    const int c = (int)(i - k * SG_C);
    const int b = beg[k], e = end[k];
    float s = 0.f;
    if (e > b) {
        s = part[(size_t)b * SG_C + c];
        for (long j = ((long)b / SG_CHUNK + 1) * SG_CHUNK; j < e; j += SG_CHUNK) s += part[(size_t)j * SG_C + c];
    }
    dG[i] = accumulate ? dG[i] + s : s;
}

__global__ void k_im2col5(const float* __restrict__ in, float* __restrict__ out, int n, int Hi, int Wi, int Ci, int Ho, int Wo, int stride, int pad, int ld) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n * Ho * Wo * ld) return;
    const long p = i / ld;
    const int col = (int)(i - p * ld);
    float v = 0.f;
    if (col < 25 * Ci) {
        const int kk = col / Ci, ci = col - kk * Ci, ky = kk / 5, kx = kk - ky * 5;
        const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((long)Wo * Ho));
        const int iy = oy * stride + ky - pad, ix = ox * stride + kx - pad;
        if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) v = in[(((size_t)b * Hi + iy) * Wi + ix) * Ci + ci];
    }
    out[i] = v;
}

__global__ void k_conv5_dgrad_relu(const float* __restrict__ dY, const float* __restrict__ w, const float* __restrict__ X, float* __restrict__ dX,
                                   int n, int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int stride, int pad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n * Hi * Wi * Ci) return;
    const int ci = (int)(i % Ci);
    const long q = i / Ci;
    const int ix = (int)(q % Wi), iy = (int)((q / Wi) % Hi), b = (int)(q / ((long)Wi * Hi));
    float acc = 0.f;
    if (X[i] > 0.f) {
        for (int ky = 0; ky < 5; ++ky) {
            const int ty = iy + pad - ky;
            if (ty < 0 || ty % stride) continue;
            const int oy = ty / stride;
            if (oy >= Ho) continue;
            for (int kx = 0; kx < 5; ++kx) {
                const int tx = ix + pad - kx;
                if (tx < 0 || tx % stride) continue;
                const int ox = tx / stride;
                if (ox >= Wo) continue;
                const float* g = dY + (((size_t)b * Ho + oy) * Wo + ox) * Co;
                const float* wr = w + ((size_t)(ky * 5 + kx) * Ci + ci) * Co;
                for (int co = 0; co < Co; ++co) acc = fmaf(g[co], wr[co], acc);
            }
        }
    }
    dX[i] = acc;
}

}  // namespace

void launch_im2col5(const float* in, float* out, int n, int Hi, int Wi, int Ci, int Ho, int Wo, int stride, int pad, int ld, hipStream_t s) {
    const long m = (long)n * Ho * Wo * ld;
    hipLaunchKernelGGL(k_im2col5, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, in, out, n, Hi, Wi, Ci, Ho, Wo, stride, pad, ld);
}

void launch_conv5_dgrad_relu(const float* dY, const float* w, const float* X, float* dX, int n, int Hi, int Wi, int Ci, int Ho, int Wo, int Co,
                             int stride, int pad, hipStream_t s) {
    const long m = (long)n * Hi * Wi * Ci;
    hipLaunchKernelGGL(k_conv5_dgrad_relu, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, dY, w, X, dX, n, Hi, Wi, Ci, Ho, Wo, Co, stride, pad);
}

int scene_key_bits(long n_keys) {
    int bits = 1;
    while (bits < 32 && ((long)1 << bits) <= n_keys) ++bits;
    return bits;
}

size_t scene_grad_sort_bytes(long n, int key_bits) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                                    (size_t)n, 0, (unsigned)key_bits);
    return bytes;
}

void launch_scene_wcat(const float* Wg, const float* Wc, int H, int Ev, float* wcat, hipStream_t s) {
    const int n = 3 * H * SG_C;
    hipLaunchKernelGGL(k_scene_wcat, dim3((n + 255) / 256), dim3(256), 0, s, Wg, Wc, H, Ev, wcat);
}

int launch_scene_grid_grad(const SceneDsArgs& a, const SceneSortBufs& b, float* dG, int accumulate, hipStream_t s) {
    if (a.H % 8 != 0) return -1;                               // k_scene_ds steps k by 8 (float4 per lane half); ds rows are SG_C = dims.C = 32 wide
    const long n = (long)a.R * a.T;
    const uint32_t nk = (uint32_t)a.n_keys;
    if (n > 0) {
        const long tiles = (n + 31) / 32;
        hipLaunchKernelGGL(k_scene_ds, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, a);
        size_t tb = b.tmp_bytes;
        if (rocprim::radix_sort_pairs(b.tmp, tb, a.keys, b.keys_sorted, a.idx, b.idx_sorted, (size_t)n, 0, (unsigned)a.key_bits, s) != hipSuccess)
            return -1;
        (void)hipMemsetAsync(b.beg, 0, (size_t)nk * sizeof(int32_t), s);
        (void)hipMemsetAsync(b.end, 0, (size_t)nk * sizeof(int32_t), s);
        hipLaunchKernelGGL(k_scene_bounds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b.keys_sorted, n, nk, b.beg, b.end);
        const long groups = (n + SG_CHUNK - 1) / SG_CHUNK;
        hipLaunchKernelGGL(k_scene_chunks, dim3((unsigned)((groups + 7) / 8)), dim3(256), 0, s, b.keys_sorted, b.idx_sorted, a.ds, n, nk, b.part);
    } else {
        (void)hipMemsetAsync(b.beg, 0, (size_t)nk * sizeof(int32_t), s);
        (void)hipMemsetAsync(b.end, 0, (size_t)nk * sizeof(int32_t), s);
    }
    const long m = (long)nk * SG_C;
    hipLaunchKernelGGL(k_scene_final, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, b.beg, b.end, b.part, nk, dG, accumulate);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
