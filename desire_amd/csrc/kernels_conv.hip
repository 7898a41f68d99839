// kernels_conv.hip -- the conv-CVAE stack of DESIRE on the fp32 matrix pipe.
// Replaces vae_encoder (model/model.py:471-492) and vae_decoder (model/model.py:453-469 +
// utils/convolutional_vae_util.py:27-135), batched over agents / (agent,k) rows instead of the
// reference's one-object-at-a-time unroll (model/model.py:211).  NHWC activations, frozen
// batch-norm + bias folded to per-channel (scale, shift), ELU / sigmoid fused in the epilogue.
//
//   conv1   VALU   [32,32,1]  -s2 SAME->  [16,16,32]     (0.4 MF/agent)
//   conv2   MFMA   gather, rows = output pixels, K = 25 taps x 32 ci
//   conv3   MFMA   gather, VALID, K = 25 taps x 64 ci
//   deconv2 MFMA   scatter: G[(sample,in-pixel), (tap,co)] = In @ W, accumulated into the lane's
//                  64 output registers (gather form would waste 75% of the MFMAs on a 4->8 VALID
//                  transposed conv); a half-wave owns (sample, co-half) entirely, so the
//                  accumulation is register-local and deterministic
//   deconv3 MFMA   stride-2 transposed conv split in its 4 output-parity classes, each a
//                  stride-1 gather conv with 2x2 / 2x3 / 3x2 / 3x3 taps: accumulators ARE the
//                  output, no scatter
//   deconv4 VALU   one output channel: 32-wide dot per tap, parity class per wave (+sigmoid)
#include "common.h"
#include "kernels.h"
#include <type_traits>
#include <utility>

// ------------------------------------------------------------------------------------------------
// conv1 (VALU): one workgroup per agent
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_WG) void k_conv1(ConvArgs a) {
    // image with a one-pixel zero border ([35][40], image at +1,+1): no bounds tests, the five taps of a row come from two
    // aligned 16-byte LDS reads; the lane's 25 weights (its output channel) live in registers
    __shared__ __attribute__((aligned(16))) float in_s[36 * 40];
    const int n = blockIdx.x, tid = threadIdx.x;
    DYN_N(a, n, n)
    for (int i = tid; i < 36 * 40; i += DS_WG) in_s[i] = 0.f;
    __syncthreads();
    for (int i = tid; i < 1024; i += DS_WG) in_s[((i >> 5) + 1) * 40 + (i & 31) + 1] = a.in[(size_t)n * 1024 + i];
    const int co = tid & 31, pg = tid >> 5;
    float wr[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) wr[k] = a.w_raw[k * 32 + co];       // [ky][kx][0][co]
    __syncthreads();
    const float sc = a.scale[co], sh = a.shift[co];
    for (int p = pg; p < 256; p += 8) {
        const int oy = p >> 4, ox = p & 15;
        const int base = (2 * ox) & ~3;
        const bool odd = ox & 1;                                      // uniform in the wave (one pixel per wave)
        float acc = 0.f;
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) {
            const float* row = in_s + (2 * oy + ky) * 40 + base;
            const float4 v0 = *reinterpret_cast<const float4*>(row), v1 = *reinterpret_cast<const float4*>(row + 4);
            const float t0 = odd ? v0.z : v0.x, t1 = odd ? v0.w : v0.y, t2 = odd ? v1.x : v0.z, t3 = odd ? v1.y : v0.w, t4 = odd ? v1.z : v1.x;
            acc = fmaf(t0, wr[ky * 5 + 0], acc);                      // same tap order as before: ky outer, kx inner
            acc = fmaf(t1, wr[ky * 5 + 1], acc);
            acc = fmaf(t2, wr[ky * 5 + 2], acc);
            acc = fmaf(t3, wr[ky * 5 + 3], acc);
            acc = fmaf(t4, wr[ky * 5 + 4], acc);
        }
        { const size_t ix = ((size_t)n * 256 + p) * 32 + co; a.out[ix] = conv_epilogue(acc, sc, sh, a.mode, false, a.yprev, ix); }
    }
}
void launch_conv1(const ConvArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_conv1, dim3(a.n), dim3(DS_WG), 0, s, a);
}

// ------------------------------------------------------------------------------------------------
// forward conv, gather form.  Workgroup = 64 output rows = SPW samples x OW*OW pixels.
// NT = CO/32 n-tiles:  NT==2 -> wave = (nt = w&1, m-tile = w>>1), MT = 1
//                      NT==4 -> wave = (nt = w), MT = 2
// ------------------------------------------------------------------------------------------------
template <int CI, int IW, int OW, int STRIDE, int PAD, int CO>
__global__ __launch_bounds__(DS_WG) void k_conv_gather(ConvArgs a) {
    constexpr int PIX = OW * OW, SPW = DS_TM / PIX, LDP = CI + 4, NT = CO / 32, G = CI / 8;
    constexpr int MT = (NT == 4) ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* zero_row = smem;                       // LDP zeros
    float* in_s = smem + LDP;                     // [SPW][IW*IW][LDP]
    const int lane = lane_id(), w = wave_id(), tid = threadIdx.x;
    const int s0 = blockIdx.x * SPW;
    DYN_N(a, n, s0)
    for (int i = tid; i < LDP; i += DS_WG) zero_row[i] = 0.f;
    constexpr int Q = CI / 4;
    // position of pixel (y, x) in a sample's LDS image.  Stride 2: the four parity classes are kept as separate (IW/2)^2 sub-images -- a tap
    // reads ONE class, so the lanes of a fragment read neighbouring pixels LDP floats apart (conflict-free 16-byte reads) instead of
    // every second pixel (2 LDP = 288 bytes apart: eight lanes per bank group, half of the LDS cycles were conflicts)
    auto pos = [](int y, int x) {
        if (STRIDE == 2) return (((y & 1) * 2 + (x & 1)) * (IW / 2) + (y >> 1)) * (IW / 2) + (x >> 1);
        return y * IW + x;
    };
    for (int i = tid; i < SPW * IW * IW * Q; i += DS_WG) {
        const int pix = i / Q, c4 = i - pix * Q;
        const int ls = pix / (IW * IW), pp = pix - ls * IW * IW;
        const int smp = s0 + ls;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (smp < a.n) v = *reinterpret_cast<const float4*>(a.in + ((size_t)s0 * IW * IW + pix) * CI + c4 * 4);
        *reinterpret_cast<float4*>(in_s + (ls * IW * IW + pos(pp / IW, pp % IW)) * LDP + c4 * 4) = v;
    }
    __syncthreads();
    const int nt = (NT == 4) ? w : (w & 1);
    const int mt0 = (NT == 4) ? 0 : (w >> 1);
    f32x16 acc[MT];
    int oy[MT], ox[MT], sm[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        acc[m] = zero16();
        const int r = (mt0 + m) * 32 + (lane & 31);
        sm[m] = r / PIX;
        const int q = r - sm[m] * PIX;
        oy[m] = q / OW;
        ox[m] = q - oy[m] * OW;
    }
    for (int ky = 0; ky < 5; ++ky)
        for (int kx = 0; kx < 5; ++kx) {
            const float* ap[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int iy = oy[m] * STRIDE + ky - PAD, ix = ox[m] * STRIDE + kx - PAD;
                const bool ok = iy >= 0 && iy < IW && ix >= 0 && ix < IW;
                ap[m] = (ok ? in_s + (sm[m] * IW * IW + pos(iy, ix)) * LDP : zero_row) + 4 * (lane >> 5);
            }
            mma_groups_ptr<MT>(acc, ap, a.Wp + ((size_t)((ky * 5 + kx) * NT + nt) * G) * 64 + lane, G);
        }
    const int co = nt * 32 + (lane & 31);
    const float sc = a.scale[co], sh = a.shift[co];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = (mt0 + m) * 32 + acc_row(i);
            const int smp = s0 + r / PIX;
            if (smp < a.n) { const size_t ix = ((size_t)s0 * PIX + r) * CO + co; a.out[ix] = conv_epilogue(acc[m][i], sc, sh, a.mode, false, a.yprev, ix); }
        }
}
void launch_conv2(const ConvArgs& a, hipStream_t s) {
    const size_t lds = (36 + 256 * 36) * sizeof(float);
    hipLaunchKernelGGL((k_conv_gather<32, 16, 8, 2, 1, 64>), dim3(a.n), dim3(DS_WG), lds, s, a);
}
void launch_conv3(const ConvArgs& a, hipStream_t s) {
    const size_t lds = (68 + 4 * 64 * 68) * sizeof(float);
    launch_big_lds<k_conv_gather<64, 8, 4, 1, 0, 128>>(dim3((a.n + 3) / 4), dim3(DS_WG), lds, s, a);
}

// ------------------------------------------------------------------------------------------------
// deconv2: [n,4,4,128] -> [n,8,8,64], 5x5 VALID stride 1, scatter form with the output tile in registers.
// Workgroup = 4 samples; wave = (co-half hf = w&1, sample pair sp = w>>1).
// M-tile rows r = ix + 4 s + 8 iy (sample s of the pair, input pixel (iy, ix)); A (K=128) lives in 64 VGPRs.
// With these rows acc_row(i) puts sample s0 + (lane>>5) ENTIRELY into its half-wave and input pixel (i>>2, i&3) into accumulator
// register i, so a lane keeps the whole 8 x 8 output column of one (sample, channel) in 64 registers O[oy][ox] and tap (ky, kx) is
//     O[iy + ky][ix + kx] += acc[4 iy + ix]
// with compile-time register indices: 16 VALU adds, no LDS read-modify-write, no zeroing pass, no cross-lane traffic.
// (Until the rows were renumbered they were (s << 4) | p: a lane's 16 registers belonged to 8 pixels of EACH sample and the tile was
// accumulated in LDS, 16 reads + 16 writes per lane and tap, fenced against the next tap's MFMAs.  Same sums in the same order: bit-identical.)
// ------------------------------------------------------------------------------------------------
// Measured on the register form (512 windows, same box, step ms; scatter form 135.1 - 135.5; history and the scatter form's own dropped
// experiments -- workgroup stagger, K = 128 as two chains over its halves, ds_add_f32 -- in docs/DESIGN_DETAIL.md section 4):
//   kept     taps in order, one accumulator, tile staged once through LDS for float4 stores          133.0 - 133.2
//   dropped  epilogue straight from registers (64 dword stores per lane, a full 128-byte line each)   133.3 - 133.5 (and 200 - 370 B of scratch)
//   dropped  the adds of tap t issued behind the first four MFMAs of tap t+1 (second accumulator)     133.2 - 133.4
//   dropped  two taps in flight: two accumulators whose MFMAs alternate, quarter-tap fragment sets    133.1 - 133.3
//   dropped  two workgroups per CU (what 241 registers give when nothing holds the count up)          136.3 - 136.8
// A dependent 32x32x2 chain issues at the pipe's rate (issue interval = dependent latency = 64 cycles), so a second chain has nothing to fill.
template <bool FWD>
__global__ __launch_bounds__(DS_WG) void k_deconv2(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float out_s[];     // [4][64 px][64 co]: the finished tile on its way to the float4 stores
    const int lane = lane_id(), w = wave_id();
    const int hf = w & 1, sp = w >> 1;
    // One wave per SIMD, as the scatter form ran (286 registers).  This form needs 241, and left at that two workgroups share a CU: step 136.3 - 136.8 ms
    // against 133.0 - 133.2 with one (scatter form 135.1 - 135.5).  Naming the last accumulation register as clobbered puts the kernel's register count
    // above half of the SIMD's 512.
    asm volatile("" ::: "a255");
    // tiles bx, bx + gridDim.x, ..: one per workgroup unless the grid was sized from a count HINT (dyn_count.h: DynCount.hint) that the real count exceeds
    DYN_N(a, n, blockIdx.x * 4)
    for (int bx = blockIdx.x; bx * 4 < a.n; bx += gridDim.x) {
        const int s0 = bx * 4 + sp * 2;
        const int c = lane & 31, hi = lane >> 5;
        // this lane's output: sample s0 + hi, channel hf * 32 + c, all 8 x 8 pixels -- cleared for every tile
        float O[8][8];
    #pragma unroll
        for (int oy = 0; oy < 8; ++oy)
    #pragma unroll
            for (int ox = 0; ox < 8; ++ox) O[oy][ox] = 0.f;
        // A fragments: row = lane&31 = ix + 4 s + 8 iy -> (s = (row>>2)&1, p = 4 iy + ix)
        float4 af[16];
        {
            const int row = lane & 31;
            const int smp = min(s0 + ((row >> 2) & 1), a.n - 1);
            const float* src = a.in + ((size_t)smp * 16 + (row >> 3) * 4 + (row & 3)) * 128 + 4 * hi;
    #pragma unroll
            for (int g = 0; g < 16; ++g) af[g] = *reinterpret_cast<const float4*>(src + g * 8);
        }
        // taps in halves of 8 k-groups: the B fragments of half q+1 are fetched while half q contracts (32 MFMAs = 2048 cycles in flight).  Two
        // register sets of 8 float4; the 50 halves are unrolled so that the sets and the elements of O are addressed statically, with the
        // sched_barrier fences that keep hipcc from sinking a prefetch to its use.  The offset is opaque per tile: the fragment addresses do not
        // depend on the tile, and hoisted out of the tile loop the 400 loads live across it (3.6 KB of scratch per lane).
        int woff = 0;
        asm volatile("" : "+s"(woff));
        const float4* wp = a.Wp + woff + lane;
        auto load_b = [&](float4 (&b)[8], int q) {
            const float4* bp = wp + ((size_t)((q >> 1) * 2 + hf) * 16 + (q & 1) * 8) * 64;
    #pragma unroll
            for (int g = 0; g < 8; ++g) b[g] = bp[g * 64];
        };
        float4 b[2][8];
        load_b(b[0], 0);
        f32x16 acc = zero16();
    #pragma unroll
        for (int q = 0; q < 50; ++q) {
            if (q + 1 < 50) load_b(b[(q + 1) & 1], q + 1);
            __builtin_amdgcn_sched_barrier(0);
            const float4 (&bt)[8] = b[q & 1];
            if (!(q & 1)) acc = zero16();
    #pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 av = af[(q & 1) * 8 + g];
                acc = mfma32(av.x, bt[g].x, acc);
                acc = mfma32(av.y, bt[g].y, acc);
                acc = mfma32(av.z, bt[g].z, acc);
                acc = mfma32(av.w, bt[g].w, acc);
            }
            if (q & 1) {
                // accumulator register i = input pixel (iy, ix) = (i >> 2, i & 3) of this lane's own sample and channel: the tap is 16 adds.
                // Every output element receives 0 + G_tap0 + G_tap1 + .. in ascending tap order, as in the scatter form: the same bits
                const int tap = q >> 1, ky = tap / 5, kx = tap - ky * 5;
    #pragma unroll
                for (int i = 0; i < 16; ++i) O[(i >> 2) + ky][(i & 3) + kx] = O[(i >> 2) + ky][(i & 3) + kx] + acc[i];
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // the finished tile goes through LDS once, so that 8 lanes x float4 store one 128-byte row of (pixel, 32 channels).  This wave's region =
        // [2 samples x 64 px] x its 32 output channels; it is the only reader and writer of it (no barrier)
        float* my = out_s + (sp * 2) * 4096;
    #pragma unroll
        for (int o = 0; o < 64; ++o) my[(hi * 64 + o) * 64 + hf * 32 + c] = O[o >> 3][o & 7];
        const int er = lane >> 3, ec = hf * 32 + (lane & 7) * 4;
        const float4 sc4 = *reinterpret_cast<const float4*>(a.scale + ec), sh4 = *reinterpret_cast<const float4*>(a.shift + ec);
        for (int i = 0; i < 16; ++i) {
            const int sp_px = i * 8 + er;                                  // 0..127 = (sample, pixel)
            const int smp = s0 + (sp_px >> 6);
            if (smp < a.n) {
                const float4 v = *reinterpret_cast<const float4*>(my + sp_px * 64 + ec);
                const size_t ix = ((size_t)smp * 64 + (sp_px & 63)) * 64 + ec;
                float4 o;
                if (FWD) {                                                 // forward: BN + ELU, nothing else in the loop
                    o.x = eluf_(v.x * sc4.x + sh4.x); o.y = eluf_(v.y * sc4.y + sh4.y);
                    o.z = eluf_(v.z * sc4.z + sh4.z); o.w = eluf_(v.w * sc4.w + sh4.w);
                } else {
                    o.x = conv_epilogue(v.x, sc4.x, sh4.x, a.mode, false, a.yprev, ix);
                    o.y = conv_epilogue(v.y, sc4.y, sh4.y, a.mode, false, a.yprev, ix + 1);
                    o.z = conv_epilogue(v.z, sc4.z, sh4.z, a.mode, false, a.yprev, ix + 2);
                    o.w = conv_epilogue(v.w, sc4.w, sh4.w, a.mode, false, a.yprev, ix + 3);
                }
                *reinterpret_cast<float4*>(a.out + ix) = o;
            }
        }
    }
}
void launch_deconv2(const ConvArgs& a, hipStream_t s) {
    const int ng = dyn_units(a.n, a.dyn);                  // (device-side count: the grid follows the count hint, the kernel strides over what is left)
    if (a.mode == 0) launch_big_lds<k_deconv2<true>>(dim3((ng + 3) / 4), dim3(DS_WG), 4 * 4096 * sizeof(float), s, a);
    else launch_big_lds<k_deconv2<false>>(dim3((ng + 3) / 4), dim3(DS_WG), 4 * 4096 * sizeof(float), s, a);
}

// ------------------------------------------------------------------------------------------------
// deconv3: [n,8,8,64] -> [n,16,16,32], 5x5 SAME stride 2:  o = 2i + k - 1.
// Output parity class p = o&1 uses taps k with k = p+1 (mod 2): p=0 -> k in {1,3}, p=1 -> {0,2,4};
// input shift d = (p + 1 - k)/2, i = q + d for o = 2q + p.  One wave per sample, MT = 2 covers the
// 64 outputs of a class.
// ------------------------------------------------------------------------------------------------
// A tile is one statically unrolled sequence of 25 (class, tap) chains.  The eight B-fragment loads of chain s + 1 and its LDS row pointers are
// issued before the MFMAs of chain s (two named fragment sets; across class boundaries, so ahead of the class epilogue's stores; chain 0's ahead
// of the staging loop and its barrier), and a row outside the image is a select between the image row and its zero_row slot, not a divergent
// region.  Until then each chain was one mma_groups_ptr<2, true> call: about 45 instructions of address set-up with four s_and_saveexec
// regions, eight loads, and `s_waitcnt vmcnt(7)` on the first of them, 25 times per tile and wave.  Same products in the same order per
// accumulator, same stores: bit-identical (tests/test_gpu_gen_chain_bits.py).  Measured (512 windows, same box, step ms, three alternating runs
// each; the rule and the tables: profiles/README.md, gen_heads):
//   parent   rolled chains, B fragments requested at the head of each chain                         130.83 - 130.93   (118 + 32 registers)
//   kept     weights and row pointers a chain ahead                                                 129.17 - 129.34   (162 + 32, no scratch)
//   dropped  ... + the A fragment of unit (g, m) + 1 read before the MFMAs of unit (g, m)           129.33 - 129.40   (166 + 32): the other M-tile's
//            four MFMAs already cover the LDS read -- the two accumulators alternate, which k_ioc's single chain does not have
//   not built  a second accumulator pair, so that a class's ELU and stores issue between the first MFMAs of the next class
// Kernel time 17.50 -> 15.94 ms, MfmaUtil 0.79 -> 0.88, the same SQ_VALU_MFMA_BUSY_CYCLES.
// The 25 (class, tap) chains of a tile, 64 MFMAs per M-tile each, in the order of the nest  py, px, ky = 1 - py (+2) .., kx = 1 - px (+2) .. :
// chains 0-3 class (0,0), 4-9 (0,1), 10-15 (1,0), 16-24 (1,1).  first / last: the chain that opens / closes its class's accumulators.
struct D3Chain { int py, px, ky, kx; bool first, last; };
__host__ __device__ constexpr D3Chain d3_chain(int s) {
    const int c = s < 4 ? 0 : s < 10 ? 1 : s < 16 ? 2 : 3, s0 = c == 0 ? 0 : c == 1 ? 4 : c == 2 ? 10 : 16;
    const int py = c >> 1, px = c & 1, nkx = px ? 3 : 2, n = (py ? 3 : 2) * nkx, i = s - s0;
    return D3Chain{py, px, 1 - py + 2 * (i / nkx), 1 - px + 2 * (i % nkx), i == 0, i == n - 1};
}
// f(integral_constant<int, 0>), .., f(integral_constant<int, N - 1>) in order: a loop whose index is a constant in the body by construction (the
// epilogue of the training-mode form is large enough for `#pragma unroll` to give up on 25 chains, and a rolled loop indexes the fragment sets at run time)
template <class F, int... S>
__device__ __forceinline__ void static_for_(F&& f, std::integer_sequence<int, S...>) { (f(std::integral_constant<int, S>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_(f, std::make_integer_sequence<int, N>{}); }
// NS = samples (= waves) per workgroup (4; NS = 2 -- four small workgroups per CU instead of two -- measured 15 % slower).
template <bool FWD, int NS>
__global__ __launch_bounds__(NS * 64) void k_deconv3(ConvArgs a) {
    constexpr int LDP = 68;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // 384 bytes of zeros for the taps outside the image.  A lane whose tap is outside reads them at the byte offset (mod 256) its pixel
    // WOULD have had: ds_read_b128 is serviced in 16-lane groups over a 256-byte bank row, consecutive pixels (272 bytes apart) fill its
    // sixteen 16-byte slots exactly once, and ONE shared zero address sits on the slot of some valid lane of the group -- a second LDS
    // cycle for every group of a border tap (19 % of this kernel's LDS cycles were such conflicts)
    float* zero_row = smem;                                            // [96] floats, 256-byte aligned (dynamic LDS base)
    float* in_s = smem + 128;                                          // [NS][64][LDP]
    const int lane = lane_id(), w = wave_id(), tid = threadIdx.x;
    // tiles bx, bx + gridDim.x, ..: one per workgroup unless the grid was sized from a count HINT (dyn_count.h: DynCount.hint) that the real count exceeds
    DYN_N(a, n, blockIdx.x * NS)
    for (int bx = blockIdx.x; bx * NS < a.n; bx += gridDim.x) {
        const int s0 = bx * NS;
        // B fragments (the packed weights of a tap: 8 k-groups) in two statically named sets: the eight loads of chain s + 1 are issued before the
        // MFMAs of chain s, across class boundaries, and chain 0's before the staging below.  The offset is opaque per tile, as in k_deconv2: the
        // fragment addresses do not depend on the tile, and hoisted out of the tile loop the 200 loads would live across it.
        int woff = 0;
        asm volatile("" : "+s"(woff));
        const float4* wp = a.Wp + woff + lane;
        auto load_b = [&](float4 (&f)[8], const D3Chain ch) __attribute__((always_inline)) {
            const float4* bp = wp + ((size_t)(ch.ky * 5 + ch.kx) * 8) * 64;
    #pragma unroll
            for (int g = 0; g < 8; ++g) f[g] = bp[g * 64];
        };
        float4 b[2][8];
        load_b(b[0], d3_chain(0));
        __builtin_amdgcn_sched_barrier(0);
        for (int i = tid; i < 128; i += NS * 64) zero_row[i] = 0.f;
        for (int i = tid; i < NS * 64 * 16; i += NS * 64) {
            const int pix = i >> 4, c4 = i & 15;
            const int smp = s0 + (pix >> 6);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (smp < a.n) v = *reinterpret_cast<const float4*>(a.in + ((size_t)s0 * 64 + pix) * 64 + c4 * 4);
            *reinterpret_cast<float4*>(in_s + pix * LDP + c4 * 4) = v;
        }
        __syncthreads();
        const int smp = s0 + w;
        const int hi = lane >> 5;
        // transposed contraction (weights as the A operand): the accumulators hold D[co][pixel] with lane = pixel and the 16
        // registers = output channels in runs of four, so the epilogue stores float4 (4x fewer store instructions)
        float4 sc[4], sh[4];
    #pragma unroll
        for (int q = 0; q < 4; ++q) {
            sc[q] = *reinterpret_cast<const float4*>(a.scale + 8 * q + 4 * hi);
            sh[q] = *reinterpret_cast<const float4*>(a.shift + 8 * q + 4 * hi);
        }
        int qy[2], qx[2];
    #pragma unroll
        for (int m = 0; m < 2; ++m) { const int q = m * 32 + (lane & 31); qy[m] = q >> 3; qx[m] = q & 7; }
        // LDS rows of chain s: the pixel's row of this wave's image, or its slot of zero_row outside the image -- one select per M-tile, no divergence
        auto rows = [&](const D3Chain ch, const float* (&ap)[2]) __attribute__((always_inline)) {
            const int dy = (ch.py + 1 - ch.ky) / 2, dx = (ch.px + 1 - ch.kx) / 2;   // exact: numerators even
    #pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int iy = qy[m] + dy, ix = qx[m] + dx;
                const bool ok = iy >= 0 && iy < 8 && ix >= 0 && ix < 8;
                const int in_off = 128 + (w * 64 + iy * 8 + ix) * LDP, zero_off = ((w * 64 + iy * 8 + ix + 64) * LDP + 128) & 63;
                ap[m] = smem + (ok ? in_off : zero_off) + 4 * hi;
            }
        };
        const float* ap[2][2];
        rows(d3_chain(0), ap[0]);
        f32x16 acc[2];
        static_for<25>([&](auto chain_no) __attribute__((always_inline)) {
            constexpr int s = decltype(chain_no)::value;
            constexpr D3Chain ch = d3_chain(s);
            constexpr int py = ch.py, px = ch.px;
            if constexpr (s + 1 < 25) { load_b(b[(s + 1) & 1], d3_chain(s + 1)); rows(d3_chain(s + 1), ap[(s + 1) & 1]); }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ch.first) { acc[0] = zero16(); acc[1] = zero16(); }
            const float4 (&bt)[8] = b[s & 1];
            // unit (g, m) = k-group g on M-tile m, in mma_chunk's order, fenced per unit
    #pragma unroll
            for (int g = 0; g < 8; ++g)
    #pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const float4 av = *reinterpret_cast<const float4*>(ap[s & 1][m] + g * 8);
                    acc[m] = mfma32(bt[g].x, av.x, acc[m]);
                    acc[m] = mfma32(bt[g].y, av.y, acc[m]);
                    acc[m] = mfma32(bt[g].z, av.z, acc[m]);
                    acc[m] = mfma32(bt[g].w, av.w, acc[m]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            if constexpr (ch.last) {
                if (smp < a.n) {
    #pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        const int oy = 2 * qy[m] + py, ox = 2 * qx[m] + px;       // this lane's output pixel
                        const size_t base = ((size_t)smp * 256 + oy * 16 + ox) * 32 + 4 * hi;
    #pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const size_t ix = base + 8 * q;
                            float4 o;
                            if (FWD) {
                                o.x = eluf_(acc[m][4 * q] * sc[q].x + sh[q].x); o.y = eluf_(acc[m][4 * q + 1] * sc[q].y + sh[q].y);
                                o.z = eluf_(acc[m][4 * q + 2] * sc[q].z + sh[q].z); o.w = eluf_(acc[m][4 * q + 3] * sc[q].w + sh[q].w);
                            } else {
                                o.x = conv_epilogue(acc[m][4 * q], sc[q].x, sh[q].x, a.mode, false, a.yprev, ix);
                                o.y = conv_epilogue(acc[m][4 * q + 1], sc[q].y, sh[q].y, a.mode, false, a.yprev, ix + 1);
                                o.z = conv_epilogue(acc[m][4 * q + 2], sc[q].z, sh[q].z, a.mode, false, a.yprev, ix + 2);
                                o.w = conv_epilogue(acc[m][4 * q + 3], sc[q].w, sh[q].w, a.mode, false, a.yprev, ix + 3);
                            }
                            *reinterpret_cast<float4*>(a.out + ix) = o;
                        }
                    }
                }
            }
        });
        __syncthreads();                                   // (the next tile of this workgroup restages the LDS tiles)
    }
}
void launch_deconv3(const ConvArgs& a, hipStream_t s) {
    const size_t lds = (128 + (size_t)4 * 64 * 68) * sizeof(float);
    const int ng = dyn_units(a.n, a.dyn);
    if (a.mode == 0) launch_big_lds<k_deconv3<true, 4>>(dim3((ng + 3) / 4), dim3(256), lds, s, a);
    else launch_big_lds<k_deconv3<false, 4>>(dim3((ng + 3) / 4), dim3(256), lds, s, a);
}

// ------------------------------------------------------------------------------------------------
// deconv4 (VALU): [n,16,16,32] -> [n,32,32], 5x5 SAME stride 2, BN + sigmoid.
// One workgroup per sample; wave = output parity class (uniform tap set), 4 pixels per lane.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_WG) void k_deconv4(ConvArgs a) {
    constexpr int LDP = 36;
    __shared__ __attribute__((aligned(16))) float in_s[256 * LDP];
    __shared__ __attribute__((aligned(16))) float w_s[25 * 32];
    const int n = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = wave_id();
    for (int i = tid; i < 256 * 8; i += DS_WG) {
        const int pix = i >> 3, c4 = i & 7;
        *reinterpret_cast<float4*>(in_s + pix * LDP + c4 * 4) =
            *reinterpret_cast<const float4*>(a.in + ((size_t)n * 256 + pix) * 32 + c4 * 4);
    }
    for (int i = tid; i < 800; i += DS_WG) w_s[i] = a.w_raw[i];        // [ky][kx][0][ci]
    __syncthreads();
    const int py = w >> 1, px = w & 1;
    const float sc = a.scale[0], sh = a.shift[0];
    for (int j = 0; j < 4; ++j) {
        const int q = j * 64 + lane;                                   // 0..255 within the class
        const int qy = q >> 4, qx = q & 15;
        float acc = 0.f;
        for (int ky = 1 - py; ky < 5; ky += 2) {
            const int iy = qy + (py + 1 - ky) / 2;
            if (iy < 0 || iy >= 16) continue;
            for (int kx = 1 - px; kx < 5; kx += 2) {
                const int ix = qx + (px + 1 - kx) / 2;
                if (ix < 0 || ix >= 16) continue;
                const float* ip = in_s + (iy * 16 + ix) * LDP;
                const float* wp = w_s + (ky * 5 + kx) * 32;
#pragma unroll
                for (int c4 = 0; c4 < 8; ++c4) {
                    const float4 x = *reinterpret_cast<const float4*>(ip + c4 * 4);
                    const float4 ww = *reinterpret_cast<const float4*>(wp + c4 * 4);
                    acc = fmaf(x.x, ww.x, acc); acc = fmaf(x.y, ww.y, acc);
                    acc = fmaf(x.z, ww.z, acc); acc = fmaf(x.w, ww.w, acc);
                }
            }
        }
        { const size_t ix = (size_t)n * 1024 + (2 * qy + py) * 32 + 2 * qx + px; a.out[ix] = conv_epilogue(acc, sc, sh, a.mode, true, a.yprev, ix); }
    }
}
// Forward form, "tap products first": deconv4 has ONE output channel, so every input pixel contributes 25 scalars
//     T[tap] = sum_c d3[pixel, c] * w[tap, c]
// to the outputs o = 2i + k - 1.  A lane owns a pixel (its 32 channels sit in registers, read once, coalesced from HBM),
// the weights of a tap are wave-uniform (scalar loads), and the products are accumulated into an fp32 LDS image of the
// sample with plain read-add-write: inside one instruction all lanes hold the SAME tap, so the addresses are distinct
// (deterministic).  One wave per sample; HBM-bound (the gather form above is LDS-read-bound: 3x slower).
__global__ __launch_bounds__(DS_WG) void k_deconv4_tp(ConvArgs a) {
    __shared__ float xacc[4 * 1024];
    const int lane = lane_id(), w = wave_id(), tid = threadIdx.x;
    const int smp = blockIdx.x * 4 + w;
    DYN_N(a, n, blockIdx.x * 4)
    for (int i = tid; i < 4 * 1024; i += DS_WG) xacc[i] = 0.f;
    __syncthreads();
    float* xa = xacc + w * 1024;
    const float* __restrict__ wr = a.w_raw;                              // [25][32]
    if (smp < a.n) {
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int p = j * 64 + lane, iy = p >> 4, ix = p & 15;
            float4 x[8];
            const float4* src = reinterpret_cast<const float4*>(a.in + ((size_t)smp * 256 + p) * 32);
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4) x[c4] = src[c4];
#pragma unroll 1
            for (int ky = 0; ky < 5; ++ky) {
                const int Y = 2 * iy + ky - 1;
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
                    const float* wt = wr + (ky * 5 + kx) * 32;           // wave-uniform
                    float acc = 0.f;
#pragma unroll
                    for (int c4 = 0; c4 < 8; ++c4) {
                        acc = fmaf(x[c4].x, wt[c4 * 4], acc); acc = fmaf(x[c4].y, wt[c4 * 4 + 1], acc);
                        acc = fmaf(x[c4].z, wt[c4 * 4 + 2], acc); acc = fmaf(x[c4].w, wt[c4 * 4 + 3], acc);
                    }
                    const int X = 2 * ix + kx - 1;
                    if (Y >= 0 && Y < 32 && X >= 0 && X < 32) xa[Y * 32 + X] += acc;
                }
            }
        }
        const float sc = a.scale[0], sh = a.shift[0];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int o = i * 64 + lane;
            a.out[(size_t)smp * 1024 + o] = sigmoidf_(xa[o] * sc + sh);
        }
    }
}
void launch_deconv4(const ConvArgs& a, hipStream_t s) {
    if (a.mode == 0) hipLaunchKernelGGL(k_deconv4_tp, dim3((a.n + 3) / 4), dim3(DS_WG), 0, s, a);
    else hipLaunchKernelGGL(k_deconv4, dim3(a.n), dim3(DS_WG), 0, s, a);
}
