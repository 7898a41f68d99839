// kernels_rollout.hip -- K Gaussian-head rollouts per agent in one launch, written in the sample layout (desire_rollout_samples).
//
// Row r = (scene * K + k) * mno + slot of dev_Yhat is one rollout of agent (scene, slot): sample()'s prediction loop (model/model.py:643-681) from
// the agent's warmed-up X-encoder state h_T -- per step: the 5-wide head reads (mux, muy, log sx, log sy, corr) off the state, a position is drawn
// from that bivariate Gaussian, clipped to <= 1.0 and fed back through the "enc_x" GRU cell.  The warm-up itself is k_encoder (kernels_rnn.hip), once
// per AGENT; this kernel starts K rows per agent from its result.
//
// One workgroup owns 32 consecutive ROWS for all T steps: H / 32 waves, wave w owns hidden columns [32 w, 32 w + 32) of the 32 rows, the state lives
// in registers (accumulator layout) and in LDS (A-operand layout), the gate / candidate contractions run on v_mfma_f32_32x32x2_f32 out of the
// encoder's own "enc_x" packs -- the GRU arithmetic is encoder_tile's, operation for operation.  Rows are decoded one by one (scene, k, slot of EVERY
// row), so a tile may hold any mix of (scene, k) groups and the last one may be partial; nothing a row computes depends on its tile.
//
// THE HEAD is computed by the whole workgroup: the 2 H / 32 threads that share a row (tid & 31) each contract 16 consecutive hidden columns with the
// five head columns (80 fmaf, ascending column), lane l adds the partial of lane l + 32 (one cross-half shuffle), and the row's thread adds the H / 32
// wave partials in ascending wave order, then the bias: a fixed order that depends on H alone.  No atomics.  (k_encoder<.., ROLL> runs the whole
// H-step chain five times on 32 of its threads, in front of every GRU step.)
//
// THE NORMALS of ROLL_CH steps are brought into LDS at a time by all threads: read from dev_normals [R, T, 2], or computed from the rollout counter
// (philox.h: philox_roll4, one block = two steps of a row) and never stored.
#include "common.h"
#include "kernels.h"
#include "philox.h"

constexpr int ROLL_CH = 16;                // steps of normals held in LDS (8 Philox blocks per row and refill)
constexpr int ROLL_NZLD = 2 * ROLL_CH + 4; // row stride of that image (floats)

static size_t roll_lds_bytes(int H) {
    const int NT = H >> 5;
    return (size_t)(32 * (H + 4) + 64 + 5 * H + 32 * NT * 5 + 32 * ROLL_NZLD) * sizeof(float);
}

// one 32x32 output tile of this wave: acc += hs[32 rows][H] . Wp(ntile)
__device__ __forceinline__ void roll_mma(f32x16& acc, const float* a_lane, const float4* __restrict__ b_lane, int G) {
    f32x16 t[1] = {acc};
    mma_groups<1>(t, a_lane, 0, b_lane, G);
    acc = t[0];
}

template <int H>
__global__ __launch_bounds__((H / 32) * 64) void k_rollout(RollArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LDH = H + 4, NT = H >> 5, G = H >> 3, NTHR = NT * 64;
    float* hs = smem;                      // [32][LDH]   h_{t-1}, then r * h_{t-1}
    float* xs = hs + 32 * LDH;             // [32][2]     this step's drawn position = the GRU input
    float* w5s = xs + 64;                  // [5][H]      head weights, transposed
    float* ps = w5s + 5 * H;               // [32][NT][5] head partials per wave
    float* nz = ps + 32 * NT * 5;          // [32][ROLL_NZLD] normals of steps [tc, tc + ROLL_CH)
    const int lane = lane_id(), w = wave_id(), tid = threadIdx.x;
    const int col = w * 32 + (lane & 31);
    const int r0 = blockIdx.x * 32;
    // the row this thread serves in the head and in the normals' refill, and where it comes from (dead rows of the last tile repeat row R - 1)
    const int hrow = tid & 31, part = tid >> 5;
    const int rr = min(r0 + hrow, a.R - 1);
    const int sk = rr / a.mno, slot = rr - sk * a.mno, sc = sk / a.K, kk = sk - sc * a.K;
    const int agent = sc * a.mno + slot;

    for (int i = tid; i < 5 * H; i += NTHR) { const int c = i / 5, j = i - c * 5; w5s[j * H + c] = a.w5[i]; }
    {   // h_T of the row's agent, columns [16 part, 16 part + 16)
        const float4* src = reinterpret_cast<const float4*>(a.h_T + (size_t)agent * H + part * 16);
        float4* dst = reinterpret_cast<float4*>(hs + hrow * LDH + part * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q] = src[q];
    }
    const float wr0 = a.wx_g[col], wr1 = a.wx_g[2 * H + col], wu0 = a.wx_g[H + col], wu1 = a.wx_g[2 * H + H + col];
    const float wc0 = a.wx_c[col], wc1 = a.wx_c[H + col], br = a.b_g[col], bu = a.b_g[H + col], bc = a.b_c[col];
    float b5r[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) b5r[j] = a.b5[j];
    RngKey key{0u, 0u, 0u};
    if (!a.normals) key = rng_key(a.g);
    __syncthreads();
    f32x16 h;
#pragma unroll
    for (int i = 0; i < 16; ++i) h[i] = hs[acc_row(i) * LDH + col];
    const float* a_lane = hs + (lane & 31) * LDH + 4 * (lane >> 5);
    float* my_h = hs + (4 * (lane >> 5)) * LDH + col;       // + acc-row offset * LDH

    for (int t = 0; t < a.T; ++t) {
        // hs holds h_{t-1} of every wave (the barrier above / at the end of the last step)
        if ((t % ROLL_CH) == 0) {
            for (int blk = part; blk < ROLL_CH / 2; blk += 2 * NT) {
                const int tb = t + 2 * blk;
                if (tb >= a.T) continue;
                float n[4] = {0.f, 0.f, 0.f, 0.f};
                if (a.normals) {
                    const float* src = a.normals + ((size_t)rr * a.T + tb) * 2;
                    n[0] = src[0]; n[1] = src[1];
                    if (tb + 1 < a.T) { n[2] = src[2]; n[3] = src[3]; }
                } else {
                    philox_roll4(key.lo, key.hi, key.draw, a.g.scene_base + (uint32_t)sc, (uint32_t)kk, a.g.slot_base + (uint32_t)slot, (uint32_t)tb, n);
                }
                *reinterpret_cast<float4*>(nz + hrow * ROLL_NZLD + blk * 4) = make_float4(n[0], n[1], n[2], n[3]);
            }
        }
        {   // head, this thread's 16 columns of its row
            const float4* hv4 = reinterpret_cast<const float4*>(hs + hrow * LDH + part * 16);
            const float4 h0 = hv4[0], h1 = hv4[1], h2 = hv4[2], h3 = hv4[3];
            float p[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float4* wv = reinterpret_cast<const float4*>(w5s + j * H + part * 16);
                const float4 w0 = wv[0], w1 = wv[1], w2 = wv[2], w3 = wv[3];
                float s = 0.f;
                s = fmaf(h0.x, w0.x, s); s = fmaf(h0.y, w0.y, s); s = fmaf(h0.z, w0.z, s); s = fmaf(h0.w, w0.w, s);
                s = fmaf(h1.x, w1.x, s); s = fmaf(h1.y, w1.y, s); s = fmaf(h1.z, w1.z, s); s = fmaf(h1.w, w1.w, s);
                s = fmaf(h2.x, w2.x, s); s = fmaf(h2.y, w2.y, s); s = fmaf(h2.z, w2.z, s); s = fmaf(h2.w, w2.w, s);
                s = fmaf(h3.x, w3.x, s); s = fmaf(h3.y, w3.y, s); s = fmaf(h3.z, w3.z, s); s = fmaf(h3.w, w3.w, s);
                p[j] = s;
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float o = __shfl_xor(p[j], 32);       // the other half-wave's 16 columns of the same row
                if (lane < 32) ps[(hrow * NT + w) * 5 + j] = __fadd_rn(p[j], o);
            }
        }
        __syncthreads();                                   // partials and normals ready
        if (tid < 32) {
            // model/model.py:661-669: exp / exp / tanh of the head, one draw (Cholesky form), clip to <= 1.0 -- k_encoder<.., ROLL>'s arithmetic
            float q[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                float s = ps[hrow * NT * 5 + j];
#pragma unroll
                for (int ww = 1; ww < NT; ++ww) s = __fadd_rn(s, ps[(hrow * NT + ww) * 5 + j]);
                q[j] = __fadd_rn(s, b5r[j]);
            }
            const float2 nn = *reinterpret_cast<const float2*>(nz + hrow * ROLL_NZLD + (t % ROLL_CH) * 2);
            const float sdx = expf(q[2]), sdy = expf(q[3]), rho = tanhf(q[4]);
            const float x = fminf(q[0] + sdx * nn.x, 1.0f);
            const float y = fminf(q[1] + sdy * (rho * nn.x + sqrtf(fmaxf(1.0f - rho * rho, 0.f)) * nn.y), 1.0f);
            xs[hrow * 2] = x; xs[hrow * 2 + 1] = y;
            if (r0 + hrow < a.R) *reinterpret_cast<float2*>(a.Y + ((size_t)(r0 + hrow) * a.T + t) * 2) = make_float2(x, y);
        }
        if (t + 1 == a.T) break;                           // the state after the last draw has no reader
        __syncthreads();                                   // xs ready
        f32x16 rh, u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = acc_row(i);
            rh[i] = fmaf(xs[row * 2 + 1], wr1, fmaf(xs[row * 2], wr0, br));
            u[i] = fmaf(xs[row * 2 + 1], wu1, fmaf(xs[row * 2], wu0, bu));
        }
        roll_mma(rh, a_lane, a.Whg + ((size_t)w * G) * 64 + lane, G);
        roll_mma(u, a_lane, a.Whg + ((size_t)(w + NT) * G) * 64 + lane, G);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float r = sigmoidf_(rh[i]);
            rh[i] = r * h[i]; u[i] = sigmoidf_(u[i]);
        }
        __syncthreads();                                   // every wave done reading h_{t-1}
#pragma unroll
        for (int i = 0; i < 16; ++i) my_h[((i & 3) + 8 * (i >> 2)) * LDH] = rh[i];
        __syncthreads();
        f32x16 ac;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = acc_row(i);
            ac[i] = fmaf(xs[row * 2 + 1], wc1, fmaf(xs[row * 2], wc0, bc));
        }
        roll_mma(ac, a_lane, a.Whc + ((size_t)w * G) * 64 + lane, G);
#pragma unroll
        for (int i = 0; i < 16; ++i) h[i] = gru_blend(u[i], h[i], tanhf_(ac[i]));
        __syncthreads();                                   // every wave done reading r * h
#pragma unroll
        for (int i = 0; i < 16; ++i) my_h[((i & 3) + 8 * (i >> 2)) * LDH] = h[i];
        __syncthreads();
    }
}

void launch_rollout_samples(const RollArgs& a, hipStream_t s) {
    if (a.R <= 0 || a.T <= 0) return;
    const dim3 grid((a.R + 31) / 32);
    const size_t lds = roll_lds_bytes(a.H);
    if (a.H == 256) hipLaunchKernelGGL(k_rollout<256>, grid, dim3(512), lds, s, a);
    else if (a.H == 128) hipLaunchKernelGGL(k_rollout<128>, grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL(k_rollout<64>, grid, dim3(128), lds, s, a);
}
