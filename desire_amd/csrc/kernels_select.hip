// kernels_select.hip -- score-ordered non-maximum suppression of an agent's K samples (desire_select_diverse; the contract, operation by
// operation, is in include/desire_hip.h).
//
//   k_select_diverse<METRIC>  one workgroup = (window, a chunk of SC slots).  The staged range of every row of the chunk is streamed into LDS
//                  once (the item loop of eval_tile.h's streamer, written out below): only the frames t < t_end, only frame t_end - 1 for
//                  FINAL.  The order rows and scores go to LDS too; one lane per agent range-checks its row and turns its scores into
//                  weights.  Then a group of G lanes (G = the power of two >= K, 64 at most) runs the agent's pass out of LDS, and one lane
//                  per agent lays out order, count and mass, which leave the workgroup with coalesced stores.  The gather of the n_top
//                  first rows re-reads them from Y (n_top / K of it, the lines this workgroup fetched a moment ago).
//
// The pass is form (b) of the two the design admits: count sequential steps.  A step finds the first candidate in processing order that is still
// live (a min over the group's lanes, by shuffles), keeps it, and every lane tests its own live candidates against it; a candidate near it is
// owned by it -- it was near no sample kept before, so this is the first kept sample it is near, which is the contract's owner.  Why not (a), the
// K x K bit matrix and a one-lane pass over words: the matrix costs K (K - 1) / 2 predicates of t_end frames whatever the outcome, (b) count * K.
// A CVAE's twenty samples fall into two or three modes, so (b) computes about 60 predicates per agent where (a) computes 190, and a MEAN predicate
// is t_end square roots; (a)'s serial pass would also leave all but SC lanes idle for K steps.  (b) loses only where nothing is suppressed
// (radius 0: K steps, K (K - 1) / 2 predicates -- what (a) always pays).  A pair's predicate is the same fixed sequence of fp32 operations
// whichever lane computes it (sd_near, below), so the result is the contract's bit for bit in either form.
//
// LDS rows are float2 [t], row stride (frames staged | 1) pairs: odd, so the lanes of a group -- each on its own row, the same t -- fall on
// distinct 8-byte bank pairs (ds_read_b64 banks over a 32-lane half), and the kept sample's row is one address, a broadcast.  A candidate's
// state has one owner lane (j mod G), so the pass needs no barrier.  No atomics, no host synchronisation: capturable, bitwise reproducible, and
// a result depends on its agent's rows, order and scores only.  The LDS plan (SelLds) and the slot chunk are eval_lds.h's.
#include "eval_tile.h"

#include <climits>

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int SD_BATCH = 8;                    // 16-byte loads a lane has in flight
constexpr int SD_LIVE = -1;                    // own[j]: not yet kept or owned
constexpr int SD_KEPT = 1 << 30;               // own[j] = i | SD_KEPT: kept as number i; own[j] = i: owned by kept number i

// the predicate of (k, k') over the staged frames of two LDS rows: the contract's sequence, the same for every caller
template <int METRIC>
__device__ inline bool sd_near(const float2* __restrict__ p, const float2* __restrict__ q, int nt, float ux, float uy, float radius, float r2) {
    if constexpr (METRIC == DESIRE_DIST_FINAL) {
        const float a = (p[0].x - q[0].x) * ux, b = (p[0].y - q[0].y) * uy;
        return a * a + b * b < r2;
    } else if constexpr (METRIC == DESIRE_DIST_MAX) {
        float m = 0.f;
#pragma unroll 4
        for (int t = 0; t < nt; ++t) {
            const float a = (p[t].x - q[t].x) * ux, b = (p[t].y - q[t].y) * uy;
            const float d = a * a + b * b;
            m = (t == 0 || d > m || d != d) ? d : m;                   // a NaN stays: it is never near
        }
        return m < r2;
    } else {
        float s = 0.f;
#pragma unroll 4
        for (int t = 0; t < nt; ++t) {
            const float a = (p[t].x - q[t].x) * ux, b = (p[t].y - q[t].y) * uy;
            s += sqrtf(a * a + b * b);
        }
        return s / (float)nt < radius;
    }
}

template <int METRIC>
__global__ __launch_bounds__(EVAL_THREADS) void k_select_diverse(const float* __restrict__ Y, const int32_t* __restrict__ order,
                                                               const float* __restrict__ score, int32_t* __restrict__ order_out,
                                                               int32_t* __restrict__ count, float* __restrict__ mass, float* __restrict__ top_Y,
                                                               float* __restrict__ top_score, int n_scenes, int mno, int K, int T, int t_end,
                                                               int SC, int n_sc, int G, int vec, int n_top, float radius, float ux, float uy) {
    extern __shared__ float2 sd_sm[];
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4 && sizeof(float) == 4 && SelLds::K_WORDS == 5 && SelLds::SLOT_WORDS == 2);
    const int nt = SelLds::staged(METRIC, t_end), t_lo = t_end - nt;
    const SelLds L(nt, SC, K);
    const int Tp = L.Tp;
    float2* Yl = sd_sm;                                                 // [SC, K, Tp]
    int* wd = reinterpret_cast<int*>(Yl + L.pairs());                   // the words behind the pairs
    int* ordL = wd + L.k_words(0);                                      // [SC, K] the input order
    int* own = wd + L.k_words(1);                                       // [SC, K] state of candidate j
    float* wL = reinterpret_cast<float*>(wd + L.k_words(2));            // [SC, K] weight of sample k
    int* outL = wd + L.k_words(3);                                      // [SC, K] the diverse order
    float* massL = reinterpret_cast<float*>(wd + L.k_words(4));         // [SC, K]
    int* cntL = wd + L.slot_words(0);                                   // [SC]
    int* badL = wd + L.slot_words(1);                                   // [SC] the order row holds an index outside 0 .. K-1

    const int tid = threadIdx.x;
    const int sc = blockIdx.x % n_sc, scene = blockIdx.x / n_sc;
    const int slot0 = sc * SC, ns = min(SC, mno - slot0);
    const size_t a0 = (size_t)scene * mno + slot0;                      // first agent of the chunk

    // ---- stage: item = (k, slot, u): quad u of the staged range of row (k, slot).  A quad is two (row, t) pairs at an even pair index.  This is
    // eval_tile.h's item loop with the segment a part of one row; it stays written out here because the kernel measured 1 - 3 % slower through
    // the shared loop (FINAL and MAX), with the same statements.
    const int nq = nt / 2 + 1;                                          // quads that cover nt pairs at either parity of their first index
    const int n_items = K * ns * nq;
    for (int i0 = tid; i0 < n_items; i0 += EVAL_THREADS * SD_BATCH) {
        float4 v[SD_BATCH];
        size_t ps[SD_BATCH], qq[SD_BATCH];
        int dst[SD_BATCH];
        bool full[SD_BATCH];
#pragma unroll
        for (int u = 0; u < SD_BATCH; ++u) {
            const int i = i0 + u * EVAL_THREADS;
            full[u] = false;
            if (i >= n_items) continue;
            const int rw = i / nq, uq = i - rw * nq, k = rw / ns, s = rw - k * ns;
            ps[u] = (((size_t)scene * K + k) * mno + slot0 + s) * T + t_lo;       // first staged pair of the row
            qq[u] = (ps[u] >> 1) + uq;
            dst[u] = (s * K + k) * Tp;
            const size_t p = 2 * qq[u];
            full[u] = vec && p >= ps[u] && p + 1 < ps[u] + nt;
            if (full[u]) v[u] = *reinterpret_cast<const float4*>(Y + 4 * qq[u]);
        }
#pragma unroll
        for (int u = 0; u < SD_BATCH; ++u) {
            const int i = i0 + u * EVAL_THREADS;
            if (i >= n_items) break;
            const size_t p = 2 * qq[u];
            if (full[u]) {
                const int t = (int)(p - ps[u]);
                Yl[dst[u] + t] = make_float2(v[u].x, v[u].y);
                Yl[dst[u] + t + 1] = make_float2(v[u].z, v[u].w);
            } else {
                for (size_t pp = p; pp < p + 2; ++pp) {                 // a quad that straddles the staged range, or a buffer off 16-byte alignment
                    if (pp < ps[u] || pp >= ps[u] + nt) continue;
                    Yl[dst[u] + (int)(pp - ps[u])] = make_float2(Y[2 * pp], Y[2 * pp + 1]);
                }
            }
        }
    }
    // ---- the chunk's order rows (contiguous: [ns, K]; read through the range check below) and scores (contiguous over the slots of one k)
    for (int i = tid; i < ns * K; i += EVAL_THREADS) {
        ordL[i] = order[a0 * K + i];
        if (mass) {
            const int k = i / ns, sl = i - k * ns;
            wL[sl * K + k] = score ? score[((size_t)scene * K + k) * mno + slot0 + sl] : 0.f;
            massL[i] = 0.f;
        }
    }
    __syncthreads();
    // ---- one lane per agent: the range check, and the weights (desire_kde_nll's step 1, eval_weight_stats) in place of the scores
    for (int sl = tid; sl < ns; sl += EVAL_THREADS) {
        int bad = 0;
        for (int j = 0; j < K; ++j) bad |= (unsigned)ordL[sl * K + j] >= (unsigned)K;
        badL[sl] = bad;
        if (bad) cntL[sl] = 0;
        if (!mass) continue;
        float* w = wL + sl * K;
        const EvalWeightStats ws = eval_weight_stats(score != nullptr, K, [&](int k) { return w[k]; }, [&](int k, float e) { w[k] = e; });
        const float u = 1.f / (float)K;
        for (int k = 0; k < K; ++k) w[k] = ws.uniform ? u : w[k] / ws.sum;
    }
    __syncthreads();

    // ---- the pass: group g of G lanes takes the agents g, g + n_groups, ...  Every lane of a wave stays in the loops (the shuffles need them all).
    const float r2 = radius * radius;
    const int g = tid / G, lg = tid - g * G, n_groups = EVAL_THREADS / G;
    for (int s0 = 0; s0 < ns; s0 += n_groups) {
        const int s = s0 + g;
        const bool active = s < ns && !badL[min(s, ns - 1)];
        const int* ord = ordL + min(s, ns - 1) * K;
        int* st = own + min(s, ns - 1) * K;
        const float2* Ya = Yl + (size_t)min(s, ns - 1) * K * Tp;
        if (active)
            for (int j = lg; j < K; j += G) st[j] = SD_LIVE;
        int cur = active ? lg : K;                                      // the lane's first live candidate (K and beyond: none)
        int cnt = 0;
        for (;;) {
            int jmin = cur < K ? cur : INT_MAX;
            for (int off = G >> 1; off; off >>= 1) jmin = min(jmin, __shfl_xor(jmin, off));
            if (!__any(jmin != INT_MAX)) break;
            if (jmin != INT_MAX) {
                const float2* ys = Ya + (size_t)ord[jmin] * Tp;
                for (int j = cur; j < K; j += G) {
                    if (st[j] != SD_LIVE) continue;
                    if (j == jmin) st[j] = cnt | SD_KEPT;
                    else if (sd_near<METRIC>(Ya + (size_t)ord[j] * Tp, ys, nt, ux, uy, radius, r2)) st[j] = cnt;
                }
                ++cnt;
                while (cur < K && st[cur] != SD_LIVE) cur += G;
            }
        }
        if (active && lg == 0) cntL[s] = cnt;
    }
    __syncthreads();

    // ---- one lane per agent: kept in keeping order, then owned in processing order; the mass in processing order
    for (int s = tid; s < ns; s += EVAL_THREADS) {
        const int c = cntL[s];
        int no = c;
        for (int j = 0; j < K; ++j) {
            if (badL[s]) { outL[s * K + j] = j; continue; }
            const int o = own[s * K + j] & ~SD_KEPT, k = ordL[s * K + j];
            if (own[s * K + j] & SD_KEPT) outL[s * K + o] = k;
            else outL[s * K + no++] = k;
            if (mass) massL[s * K + o] += wL[s * K + k];
        }
        count[a0 + s] = c;
    }
    __syncthreads();
    for (int i = tid; i < ns * K; i += EVAL_THREADS) {
        order_out[a0 * K + i] = outL[i];
        if (mass) mass[a0 * K + i] = massL[i];
    }
    // ---- gather: the rows and scores of the first n_top entries, as desire_rank_samples copies them
    if (top_score)
        for (int i = tid; i < ns * n_top; i += EVAL_THREADS) {
            const int s = i / n_top, j = i - s * n_top;
            top_score[a0 * n_top + i] = score[((size_t)scene * K + outL[s * K + j]) * mno + slot0 + s];
        }
    if (top_Y) {
        const int T2 = 2 * T;
        for (int i = tid; i < ns * n_top * T2; i += EVAL_THREADS) {
            const int rw = i / T2, e = i - rw * T2, s = rw / n_top, j = rw - s * n_top;
            top_Y[a0 * n_top * T2 + i] = Y[(((size_t)scene * K + outL[s * K + j]) * mno + slot0 + s) * T2 + e];
        }
    }
}

}  // namespace

void launch_select_diverse(const EvalIn& in, const SelectParams& p, const EvalScale& sc, const SelectOut& o, hipStream_t s) {
    int SC = 1, G = 1;
    if (!select_geometry(in.mno, in.K, p.metric, p.t_end, &SC, &G)) return;       // (refused by the caller before it gets here)
    const int n_sc = eval_chunks(in.mno, SC);
    const size_t lds = SelLds(SelLds::staged(p.metric, p.t_end), SC, in.K).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0;
    const dim3 grid((unsigned)((size_t)in.n_scenes * n_sc)), block(EVAL_THREADS);
#define SD_LAUNCH(M)                                                                                                                           \
    hipLaunchKernelGGL(k_select_diverse<M>, grid, block, lds, s, in.Y, p.order, in.score, o.order_out, o.count, o.mass, o.top_Y, o.top_score,   \
                       in.n_scenes, in.mno, in.K, in.T, p.t_end, SC, n_sc, G, vec, p.n_top, p.radius, sc.ux, sc.uy)
    if (p.metric == DESIRE_DIST_FINAL) SD_LAUNCH(DESIRE_DIST_FINAL);
    else if (p.metric == DESIRE_DIST_MAX) SD_LAUNCH(DESIRE_DIST_MAX);
    else SD_LAUNCH(DESIRE_DIST_MEAN);
#undef SD_LAUNCH
}
