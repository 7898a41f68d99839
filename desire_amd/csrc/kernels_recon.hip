// kernels_recon.hip -- per-sample reconstruction errors of an agent's K futures and the weights of the best-of-many / soft-min reconstruction
// loss (desire_set_recon_loss, desire_recon_weights; the contract, operation by operation, is in include/desire_hip.h).
//
//   k_recon_weights  one workgroup = (window, a chunk of SC slots).  For one (window, k) Y is contiguous over (slot, t), so the chunk's rows of KC
//                  samples at a time are streamed into LDS (eval_tile.h's streamer, one segment per sample); the chunk's targets g and counted
//                  flags are staged once.  Then one lane per row (the fixed lane group of a row is that one lane: the contract's sum is one
//                  sequence, frame after frame) walks its LDS row in increasing t and leaves e[a, k]; the passes over k repeat until K is
//                  done -- K has no limit.  At the end one lane per agent walks its K errors: the strict-comparison minimum, then exp / sum /
//                  divide in increasing k.
//
// LDS rows are float2 [t], row stride T | 1 pairs: odd, so the lanes of a wave -- each on its own row, the same t -- fall on distinct 8-byte
// bank pairs; their targets are rows of the same stride, one per slot (lanes on the same slot, another k, read one address: a broadcast).
// The errors go through the e buffer itself (global memory, written and read by the same workgroup on either side of a barrier), so no LDS is
// spent on K.  No atomics, no scratch, no host wait: capturable, bitwise reproducible, and a result
// depends on its agent's rows and targets only.  The LDS plan (ReconLds), the slot chunk and the samples of a pass are eval_lds.h's.
//
// The scene scope (desire_set_recon_scope, desire_recon_weights_scene) weighs the K joint futures of a window -- its worlds -- instead of each
// agent's K samples: the streaming pass runs in its e-only form (TAIL = false: no per-agent walk) and, a kernel boundary later -- a window's
// reduction crosses its slot chunks --,
//
//   k_recon_scene   one workgroup = one window.  The lanes count the window's lmask slots; then lane k (striding over K) walks the window's
//                  slots in increasing slot over e[(w * mno + s) * K + k] -- consecutive lanes, consecutive addresses -- and leaves the
//                  world error E[w, k] in the E buffer itself, written and read by the same workgroup on either side of a barrier as e is
//                  above.  One lane does the winner walk and exp / sum / divide in increasing k on E, with w's first row of the window as its
//                  scratch and result; all lanes then copy that row, the winner and the term to the window's other slots with coalesced
//                  stores.  K has no limit and no LDS grows with K; the static LDS is the count's 256 ints and two result words.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int RW_BATCH = 4;                    // 16-byte loads a lane has in flight

// TAIL: the per-agent walk at the end (false: e only -- w, win, val, mode and tau are not read)
template <bool TAIL>
__global__ __launch_bounds__(EVAL_THREADS) void k_recon_weights(const float* __restrict__ Y, const float* __restrict__ fut,
                                                              const uint8_t* __restrict__ lmask, const float* __restrict__ nfut, float* e,
                                                              float* w, int32_t* __restrict__ win, float* __restrict__ val, int n_scenes, int mno,
                                                              int K, int T, int SC, int n_sc, int KC, int vec, int mode, float tau, float sx,
                                                              float sy) {
    extern __shared__ __attribute__((aligned(16))) float2 rw_sm[];
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4);
    const ReconLds L_(T, SC, KC);
    const int Tp = L_.Tp;
    float2* Yl = rw_sm;                                                 // [KC, SC, Tp]
    float2* gl = Yl + L_.rows();                                        // [SC, Tp] the targets
    int* cl = reinterpret_cast<int*>(gl + L_.slots());                  // [SC, Tp] frame t of the slot counts

    const int tid = threadIdx.x;
    const int sc = blockIdx.x % n_sc, scene = blockIdx.x / n_sc;
    const int slot0 = sc * SC, ns = min(SC, mno - slot0);
    const size_t a0 = (size_t)scene * mno + slot0;                      // first agent of the chunk

    // ---- the chunk's targets, scaled as k_train_loss scales them, and which frames count
    for (int i = tid; i < ns * T; i += EVAL_THREADS) {
        const int t = i / ns, s = i - t * ns;
        const float* f = fut + (((size_t)scene * T + t) * mno + slot0 + s) * 3;
        gl[s * Tp + t] = make_float2(__fmul_rn(f[1], sx), __fmul_rn(f[2], sy));
        cl[s * Tp + t] = f[0] != 0.f;
    }

    // ---- passes of KC samples: stage, then one lane per row
    const int L = ns * T;                                               // (slot, t) pairs of one k: contiguous in Y
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = min(KC, K - k0);
        __syncthreads();                                                // the rows of the pass before are done with (first pass: nothing to wait for)
        eval_stream<RW_BATCH>(
            Y, vec, kc, L, T, [&](int kk) { return EvalSeg{(((size_t)scene * K + k0 + kk) * mno + slot0) * T, kk}; },      // the chunk's rows of sample k0 + kk
            [&](int kk, int s, int t, float y0, float y1) { Yl[((size_t)kk * ns + s) * Tp + t] = make_float2(y0, y1); });
        __syncthreads();
        for (int rw = tid; rw < kc * ns; rw += EVAL_THREADS) {
            const int k = rw / ns, s = rw - k * ns;
            float ev = 0.f;
            if (lmask[a0 + s]) {
                const float2* y = Yl + (size_t)rw * Tp;
                const float2* g = gl + s * Tp;
                const int* c = cl + s * Tp;
                float sum = 0.f;
                for (int t = 0; t < T; ++t) {
                    if (!c[t]) continue;
                    const float dx = y[t].x - g[t].x, dy = y[t].y - g[t].y;
                    sum += sqrtf(dx * dx + dy * dy);
                }
                ev = sum / nfut[a0 + s];
            }
            e[(a0 + s) * K + k0 + k] = ev;
        }
    }
    if constexpr (!TAIL) return;
    __syncthreads();                                                    // every e of the chunk is written (and visible to this workgroup)

    // ---- one lane per agent: the walk for the minimum, then the weights and the term in increasing k
    for (int s = tid; s < ns; s += EVAL_THREADS) {
        const float* ea = e + (a0 + s) * K;
        float* wa = w + (a0 + s) * K;
        int wn = 0;
        float m = ea[0];
        for (int k = 1; k < K; ++k) {
            const float v = ea[k];
            if (v < m || (m != m && v == v)) { m = v; wn = k; }        // strict: a tie stays with the lower k; a NaN gives way to any number
        }
        float r;
        if (mode == DESIRE_RECON_MIN) {
            for (int k = 0; k < K; ++k) wa[k] = k == wn ? 1.f : 0.f;
            r = m;
        } else if (mode == DESIRE_RECON_SOFTMIN) {
            float S = 0.f;
            for (int k = 0; k < K; ++k) { const float x = expf(-(ea[k] - m) / tau); wa[k] = x; S += x; }
            for (int k = 0; k < K; ++k) wa[k] = wa[k] / S;
            r = m - tau * logf(S / (float)K);
        } else {
            float S = 0.f;
            const float u = 1.f / (float)K;
            for (int k = 0; k < K; ++k) { S += ea[k]; wa[k] = u; }
            r = S / (float)K;
        }
        win[a0 + s] = wn;
        val[a0 + s] = r;
    }
}

// ---- the scene scope: a window's K world errors, the walk over them, and the result on every slot of the window
__global__ __launch_bounds__(EVAL_THREADS) void k_recon_scene(const uint8_t* __restrict__ lmask, const float* __restrict__ e, float* E,
                                                            int32_t* __restrict__ cnt, float* w, int32_t* __restrict__ win,
                                                            float* __restrict__ val, int mno, int K, int mode, float tau) {
    __shared__ int red[EVAL_THREADS];
    __shared__ int wn_s;
    __shared__ float r_s;
    const int tid = threadIdx.x, scene = blockIdx.x;
    const size_t a0 = (size_t)scene * mno;                              // first agent of the window
    float* Ew = E + (size_t)scene * K;
    float* w0 = w + a0 * K;                                             // the window's first row of w: lane 0's scratch, then the result

    // ---- 1. the counted slots
    int c = 0;
    for (int s = tid; s < mno; s += EVAL_THREADS) c += lmask[a0 + s] != 0;
    red[tid] = c;
    __syncthreads();
    for (int o = EVAL_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const int count = red[0];
    if (tid == 0) cnt[scene] = count;

    // ---- 2. one lane per world: the sum over the counted slots in increasing slot, over the count
    for (int k = tid; k < K; k += EVAL_THREADS) {
        const float* ek = e + a0 * K + k;
        float sum = 0.f;
#pragma unroll 4
        for (int s = 0; s < mno; ++s) {
            const float v = ek[(size_t)s * K];
            if (lmask[a0 + s]) sum += v;
        }
        Ew[k] = count > 0 ? sum / (float)count : 0.f;
    }
    __syncthreads();                                                    // every E of the window is written (and visible to this workgroup)

    // ---- 3. one lane: the walk for the minimum, then the weights and the term in increasing k (k_recon_weights' tail, on E)
    if (tid == 0) {
        int wn = 0;
        float m = Ew[0];
        for (int k = 1; k < K; ++k) {
            const float v = Ew[k];
            if (v < m || (m != m && v == v)) { m = v; wn = k; }        // strict: a tie stays with the lower k; a NaN gives way to any number
        }
        float r;
        if (mode == DESIRE_RECON_MIN) {
            for (int k = 0; k < K; ++k) w0[k] = k == wn ? 1.f : 0.f;
            r = m;
        } else if (mode == DESIRE_RECON_SOFTMIN) {
            float S = 0.f;
            for (int k = 0; k < K; ++k) { const float x = expf(-(Ew[k] - m) / tau); w0[k] = x; S += x; }
            for (int k = 0; k < K; ++k) w0[k] = w0[k] / S;
            r = m - tau * logf(S / (float)K);
        } else {
            float S = 0.f;
            const float u = 1.f / (float)K;
            for (int k = 0; k < K; ++k) { S += Ew[k]; w0[k] = u; }
            r = S / (float)K;
        }
        wn_s = wn;
        r_s = r;
    }
    __syncthreads();                                                    // the first row of w is final (and visible to this workgroup)

    // ---- 4. every slot of the window gets the window's weights, winner and term (the first row of w holds them already)
    const size_t nw = (size_t)mno * K;
    for (size_t i = (size_t)K + tid; i < nw; i += EVAL_THREADS) w0[i] = w0[i % K];
    const int wn = wn_s;
    const float r = r_s;
    for (int s = tid; s < mno; s += EVAL_THREADS) { win[a0 + s] = wn; val[a0 + s] = r; }
}

}  // namespace

// the streaming pass: with the per-agent tail (TAIL) or e only
template <bool TAIL>
static void launch_recon_pass(const EvalIn& in, const ReconParams& p, const EvalScale& sc, const ReconOut& o, hipStream_t s) {
    int SC = 1, KC = 1;
    if (!recon_geometry(in.mno, in.K, in.T, &SC, &KC)) return;          // (refused by the caller before it gets here)
    const int n_sc = eval_chunks(in.mno, SC);
    const size_t lds = ReconLds(in.T, SC, KC).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0;
    hipLaunchKernelGGL(k_recon_weights<TAIL>, dim3((unsigned)((size_t)in.n_scenes * n_sc)), dim3(EVAL_THREADS), lds, s, in.Y, in.fut, p.lmask, p.nfut,
                       o.e, TAIL ? o.w : nullptr, TAIL ? o.winner : nullptr, TAIL ? o.recon : nullptr, in.n_scenes, in.mno, in.K, in.T, SC, n_sc, KC,
                       vec, p.mode, p.tau, sc.sx, sc.sy);
}

void launch_recon_weights(const EvalIn& in, const ReconParams& p, const EvalScale& sc, const ReconOut& o, hipStream_t s) {
    launch_recon_pass<true>(in, p, sc, o, s);
}

void launch_recon_weights_scene(const EvalIn& in, const ReconParams& p, const EvalScale& sc, const ReconOut& o, hipStream_t s) {
    launch_recon_pass<false>(in, p, sc, o, s);
    hipLaunchKernelGGL(k_recon_scene, dim3((unsigned)in.n_scenes), dim3(EVAL_THREADS), 0, s, p.lmask, o.e, o.E, o.count, o.w, o.winner, o.recon, in.mno,
                       in.K, p.mode, p.tau);
}
