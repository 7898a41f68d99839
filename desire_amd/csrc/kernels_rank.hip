// kernels_rank.hip -- what consumes the IOC score on the device: the per-agent order of the K samples by score, the gather of the
// n_top best-scored trajectories, and the errors of the paper's protocol (top-1 by score and best of the top n, per horizon).
//
//   k_rank_select    one wave per agent: rank by counting (an integer path, bit-exact), write order [A,K], copy the n_top best rows
//   k_sample_errors  streams Y once with 16-byte loads and writes a table [R, n_h, 2] = (ADE_h, FDE_h) of every sample, plus the
//                    number of counted frames [A, n_h] of every agent
//   k_ranked_pick    reads the table through the order: [A, n_h, 4]
//
// No atomics, no host synchronisation, horizons by value: every result is a fixed sequence of fp32 operations per (row, horizon), so
// it does not depend on the grid or on the rest of the batch, and the calls can be captured in a graph.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_LDS_BYTES = 60 * 1024;        // dynamic LDS of k_sample_errors (below the 64 KiB a launch gets without asking for more)
constexpr int RK_BATCH = 4;                    // 16-byte loads a lane has in flight

// rank_k = #{ j : s_j before s_k }.  "Before": IEEE > on the fp32 scores, ties (-0 == +0 among them) to the lower index, NaNs after
// everything else and among themselves by index -- a strict total order, so the ranks are a permutation of 0 .. K-1.
__global__ __launch_bounds__(64) void k_rank_select(const float* __restrict__ score, const float* __restrict__ Y, int32_t* __restrict__ order,
                                                    float* __restrict__ top_Y, float* __restrict__ top_score, int mno, int K, int T,
                                                    int n_top) {
    extern __shared__ float rk_sm[];
    float* s = rk_sm;
    int* ord = reinterpret_cast<int*>(rk_sm + K);
    const int a = blockIdx.x, lane = threadIdx.x;
    const int scene = a / mno, slot = a - scene * mno;
    const size_t row0 = (size_t)scene * K * mno + slot;            // row of sample k: row0 + k * mno
    for (int k = lane; k < K; k += 64) s[k] = score[row0 + (size_t)k * mno];
    __syncthreads();
    for (int k = lane; k < K; k += 64) {
        const float sk = s[k];
        const bool nk = sk != sk;
        int r = 0;
        for (int j = 0; j < K; ++j) {
            const float sj = s[j];
            const bool before = (sj != sj) ? (nk && j < k) : (nk || sj > sk || (sj == sk && j < k));
            r += before ? 1 : 0;
        }
        ord[r] = k;
        order[(size_t)a * K + r] = k;
    }
    if (!top_Y && !top_score) return;
    __syncthreads();
    const int T2 = 2 * T;
    for (int j = 0; j < n_top; ++j) {
        const int k = ord[j];
        if (top_score && lane == 0) top_score[(size_t)a * n_top + j] = s[k];
        if (top_Y) {
            const float* src = Y + (row0 + (size_t)k * mno) * T2;
            float* dst = top_Y + ((size_t)a * n_top + j) * T2;
            for (int i = lane; i < T2; i += 64) dst[i] = src[i];
        }
    }
}

// One workgroup = (window, a chunk of SC slots, a chunk of KC samples).  The ground truth of the slot chunk goes to LDS once
// (fut [n, T, mno, 3] is contiguous over the slots of a frame), then the rows of the chunk -- contiguous in Y over (slot, t) for one
// (window, k), and over k as well when the chunk holds every slot -- are streamed: a lane owns whole (row, t) pairs, two per 16-byte
// load, and leaves the pair's error in LDS.  After the barrier one lane per row walks its T errors in increasing t (the fixed summation
// order) and writes (ADE_h, FDE_h) at each horizon.  Row stride in LDS is T | 1 dwords: odd, so the walk is bank-conflict free.
__global__ __launch_bounds__(RK_THREADS) void k_sample_errors(const float* __restrict__ Y, const float* __restrict__ fut,
                                                              float* __restrict__ tab, int32_t* __restrict__ cnt, int mno, int K, int T,
                                                              int SC, int KC, int n_sc, int n_kc, int vec, float sx, float sy, float ux,
                                                              float uy, RankHz hz) {
    extern __shared__ float rk_sm[];
    __shared__ int hzs[8];
    const int Tp = T | 1;
    float* gm = rk_sm;
    float* gx = gm + SC * Tp;
    float* gy = gx + SC * Tp;
    float* eL = gy + SC * Tp;
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int kc = b % n_kc; b /= n_kc;
    const int sc = b % n_sc;
    const int scene = b / n_sc;
    const int slot0 = sc * SC, ns = min(SC, mno - slot0), k0 = kc * KC, nk = min(KC, K - k0);
    if (tid < 8) hzs[tid] = tid < hz.n ? hz.h[tid] : 0;
    const int w3 = ns * 3;
    for (int i = tid; i < T * w3; i += RK_THREADS) {
        const int t = i / w3, rem = i - t * w3, s = rem / 3, c = rem - 3 * s;
        const float v = fut[(((size_t)scene * T + t) * mno + slot0) * 3 + rem];
        const int o = s * Tp + t;
        if (c == 0) gm[o] = v != 0.f ? 1.f : 0.f;
        else if (c == 1) gx[o] = __fmul_rn(v, sx);
        else gy[o] = __fmul_rn(v, sy);
    }
    __syncthreads();

    auto put = [&](float* e, int rl, int t, float y0, float y1) {
        const int g = (rl % ns) * Tp + t;
        const float dx = (y0 - gx[g]) * ux, dy = (y1 - gy[g]) * uy;
        e[rl * Tp + t] = sqrtf(dx * dx + dy * dy);
    };
    // segments of rows that are contiguous in Y: the whole chunk when it holds every slot, else one per sample
    const bool whole = ns == mno;
    const int n_seg = whole ? 1 : nk, seg_rows = whole ? nk * ns : ns;
    for (int sg = 0; sg < n_seg; ++sg) {
        float* e = eL + (size_t)sg * seg_rows * Tp;
        const size_t P0 = (((size_t)scene * K + k0 + sg) * mno + slot0) * T, P1 = P0 + (size_t)seg_rows * T;    // (row, t) pairs [P0, P1)
        const size_t qb = (P1 + 1) >> 1;                                                                          // 16-byte quads of the whole buffer
        for (size_t q = (P0 >> 1) + tid; q < qb; q += (size_t)RK_THREADS * RK_BATCH) {
            float4 v[RK_BATCH];
            bool full[RK_BATCH];
#pragma unroll
            for (int u = 0; u < RK_BATCH; ++u) {
                const size_t qq = q + (size_t)u * RK_THREADS, p = 2 * qq;
                full[u] = vec && qq < qb && p >= P0 && p + 1 < P1;
                if (full[u]) v[u] = *reinterpret_cast<const float4*>(Y + 4 * qq);
            }
#pragma unroll
            for (int u = 0; u < RK_BATCH; ++u) {
                const size_t qq = q + (size_t)u * RK_THREADS, p = 2 * qq;
                if (qq >= qb) break;
                if (full[u]) {
                    const int local = (int)(p - P0);
                    int rl = local / T, t = local - rl * T;
                    put(e, rl, t, v[u].x, v[u].y);
                    if (++t == T) { t = 0; ++rl; }
                    put(e, rl, t, v[u].z, v[u].w);
                } else {
                    for (size_t pp = p; pp < p + 2; ++pp) {        // a quad that straddles the segment's ends, or a buffer that is not 16-byte aligned
                        if (pp < P0 || pp >= P1) continue;
                        const int local = (int)(pp - P0);
                        const int rl = local / T;
                        put(e, rl, local - rl * T, Y[2 * pp], Y[2 * pp + 1]);
                    }
                }
            }
        }
    }
    __syncthreads();

    const int n_h = hz.n, h_max = hzs[n_h - 1];
    for (int rr = tid; rr < nk * ns; rr += RK_THREADS) {
        const int kk = rr / ns, s = rr - kk * ns;
        const size_t row = ((size_t)scene * K + k0 + kk) * mno + slot0 + s;
        const float* er = eL + (size_t)rr * Tp;
        const float* mr = gm + s * Tp;
        float* trow = tab + row * n_h * 2;
        int32_t* crow = (k0 + kk == 0) ? cnt + ((size_t)scene * mno + slot0 + s) * n_h : nullptr;
        float sum = 0.f, last = 0.f;
        int np = 0, hi = 0;
        for (int t = 0; t < h_max; ++t) {
            if (mr[t] != 0.f) { last = er[t]; sum += last; ++np; }      // frames the object is absent from carry no ground truth
            if (t + 1 == hzs[hi]) {
                trow[2 * hi] = np ? sum / (float)np : 0.f;
                trow[2 * hi + 1] = last;
                if (crow) crow[hi] = np;
                ++hi;
            }
        }
    }
}

// out [A, n_h, 4] = (ADE_h, FDE_h of the best-scored sample; min over the n_top best-scored of ADE_h, of FDE_h); zeros without a counted frame.
// The minimum keeps a NaN (a NaN trajectory is reported, not hidden).
__global__ __launch_bounds__(RK_THREADS) void k_ranked_pick(const float* __restrict__ tab, const int32_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ order, float* __restrict__ out, int A, int mno,
                                                            int K, int n_h, int n_top) {
    const size_t idx = (size_t)blockIdx.x * RK_THREADS + threadIdx.x;
    if (idx >= (size_t)A * n_h) return;
    const int a = (int)(idx / n_h), hi = (int)(idx - (size_t)a * n_h);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cnt[idx] > 0) {
        const int scene = a / mno, slot = a - scene * mno;
        for (int j = 0; j < n_top; ++j) {
            const int k = min(max(order[(size_t)a * K + j], 0), K - 1);       // (a caller's buffer: never an index outside the table)
            const float* e = tab + ((((size_t)scene * K + k) * mno + slot) * n_h + hi) * 2;
            const float ade = e[0], fde = e[1];
            if (j == 0) o = make_float4(ade, fde, ade, fde);
            else {
                if (ade < o.z || ade != ade) o.z = ade;
                if (fde < o.w || fde != fde) o.w = fde;
            }
        }
    }
    float* op = out + idx * 4;
    op[0] = o.x; op[1] = o.y; op[2] = o.z; op[3] = o.w;
}

}  // namespace

void launch_rank_select(const float* score, const float* Y, int32_t* order, float* top_Y, float* top_score, int n_scenes, int mno, int K,
                        int T, int n_top, hipStream_t s) {
    hipLaunchKernelGGL(k_rank_select, dim3(n_scenes * mno), dim3(64), (size_t)K * 8, s, score, Y, order, top_Y, top_score, mno, K, T, n_top);
}

// The chunking of k_sample_errors: every slot of a window and as many samples as 256 rows hold, shrunk until the LDS fits; the samples are
// then spread evenly over the chunks.  false: not even one row fits (T_pred beyond ~3800).
bool sample_errors_geometry(int mno, int K, int T, int* SC, int* KC) {
    const size_t Tp = (size_t)(T | 1);
    int sc = mno, kc = max(1, min(K, RK_THREADS / sc));
    auto bytes = [&](int s_, int k_) { return 4 * Tp * ((size_t)3 * s_ + (size_t)s_ * k_); };
    while (bytes(sc, kc) > (size_t)RK_LDS_BYTES && kc > 1) kc = (kc + 1) / 2;
    while (bytes(sc, kc) > (size_t)RK_LDS_BYTES && sc > 1) sc = (sc + 1) / 2;
    if (bytes(sc, kc) > (size_t)RK_LDS_BYTES) return false;
    const int n_kc = (K + kc - 1) / kc;
    *SC = sc; *KC = (K + n_kc - 1) / n_kc;
    return true;
}

// The table alone: tab [R, hz.n, 2] and cnt [A, hz.n] (desire_joint_metrics sums the same rows per (window, k)).
void launch_sample_errors(const float* Y, const float* fut, float* tab, int32_t* cnt, int n_scenes, int mno, int K, int T, const RankHz& hz,
                          float sx, float sy, float ux, float uy, hipStream_t s) {
    int SC = 1, KC = 1;
    if (!sample_errors_geometry(mno, K, T, &SC, &KC)) return;         // (refused by the caller before it gets here)
    const int n_sc = (mno + SC - 1) / SC, n_kc = (K + KC - 1) / KC;
    const size_t lds = 4 * (size_t)(T | 1) * ((size_t)3 * SC + (size_t)SC * KC);
    const int vec = (reinterpret_cast<uintptr_t>(Y) & 15) == 0;
    hipLaunchKernelGGL(k_sample_errors, dim3((unsigned)((size_t)n_scenes * n_sc * n_kc)), dim3(RK_THREADS), lds, s, Y, fut, tab, cnt, mno, K, T,
                       SC, KC, n_sc, n_kc, vec, sx, sy, ux, uy, hz);
}

void launch_ranked_errors(const float* Y, const float* fut, const int32_t* order, float* tab, int32_t* cnt, float* out, int n_scenes, int mno,
                          int K, int T, int n_top, const RankHz& hz, float sx, float sy, float ux, float uy, hipStream_t s) {
    int SC = 1, KC = 1;
    if (!sample_errors_geometry(mno, K, T, &SC, &KC)) return;         // (refused by the caller before it gets here)
    launch_sample_errors(Y, fut, tab, cnt, n_scenes, mno, K, T, hz, sx, sy, ux, uy, s);
    const size_t n = (size_t)n_scenes * mno * hz.n;
    hipLaunchKernelGGL(k_ranked_pick, dim3((unsigned)((n + RK_THREADS - 1) / RK_THREADS)), dim3(RK_THREADS), 0, s, tab, cnt, order, out,
                       n_scenes * mno, mno, K, hz.n, n_top);
}
