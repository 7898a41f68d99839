// kernels_plan_cond.hip -- the K joint futures of a window conditioned on each candidate ego plan (desire_plan_risk_cond; the contract, operation
// by operation, is in include/desire_hip.h, steps C1 - C6): per (plan, world) the mean squared distance between the plan and the world's own
// prediction of the slot the plan replaces, and from it the plan's K weights, their effective sample size and the plan's support.
//
//   k_plan_cond_weights   one workgroup = (window, chunk of PC plans).  The window's prior weights W_k and logits p_k come from k_plan_weights
//                         (kernels_plan.hip: `takes part` and the joint scores are formed there, once per window).  A lane owns (plan, k) items
//                         for the whole call and walks the compared frames in increasing t with the sum in a register; the lane of plan p then
//                         runs eval_weight_stats over the plan's K logits.
//
// The plans' frames are staged through eval_stream as k_plan_risk stages them.  The compared mask needs no array: a frame that is not compared
// (no ego slot, the slot is not counted there, a NaN coordinate of the plan) gets a marker NaN in x, and a marked frame leaves the sum alone.  The K
// ego rows are staged next to the plans when the chunk's plans name ONE slot (the planner's case) and the plan of eval_lds.h has room for them;
// otherwise a lane reads its world's row from global memory.  Beyond the frames one pass holds the walk runs in passes, the sums carried in the
// call's own output dev_cw -- an item is its lane's for the whole call -- with the bits of an unchunked walk.
//
// Parking.  The K distances D_k of a plan are written to dev_cw by the item lanes; the plan's lane reads them back as logits (p_k - D_k * inv),
// overwrites them with the numerators expf(l_k - m) and then with the weights.  Nothing in the LDS grows with K, so every K is served.  No float
// atomics, no host synchronisation: capturable, bitwise reproducible, a window's results depend on that window only.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int PCW_BATCH = 4;                   // 16-byte loads a lane has in flight
constexpr unsigned PCW_MARK = 0x7fc0a5a5u;     // x of a plan frame that is not compared: a quiet NaN

__device__ __forceinline__ bool pcw_marked(const float2& v) { return __float_as_uint(v.x) == PCW_MARK; }

__global__ __launch_bounds__(EVAL_THREADS) void k_plan_cond_weights(const float* __restrict__ Y, const float* __restrict__ fut,
                                                                  const uint8_t* __restrict__ present, const float* __restrict__ plans,
                                                                  const int32_t* __restrict__ ego, const float* __restrict__ w,
                                                                  const float* __restrict__ prior, float* cw, float* __restrict__ dist,
                                                                  float* __restrict__ ess, float* __restrict__ support, int32_t* __restrict__ cond,
                                                                  int M, int mno, int K, int T, int t_cond, int PC, int TC, int rows_in_lds,
                                                                  int vecY, int vecP, float ux, float uy, float inv) {
    extern __shared__ float2 pcw_sm[];
    __shared__ int slotL[2];                                            // the smallest and the greatest ego slot of the chunk
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4 && PlanCondLds::MAX_PC <= EVAL_THREADS && PlanCondLds::PLAN_WORDS == 2);
    const PlanCondLds L(K, PC, TC, rows_in_lds);
    const int tp = L.stride();
    float2* PL = pcw_sm;                                                // [PC, tp]
    float2* E = PL + L.plans();                                         // [K, tp] (rows_in_lds)
    int* words = reinterpret_cast<int*>(E + L.rows());
    int* egoL = words + L.ego();                                        // [PC]
    int* ncL = words + L.count();                                       // [PC]
    const int tid = threadIdx.x;
    const int n_ch = (M + PC - 1) / PC;
    const int scene = blockIdx.x / n_ch, m0 = (blockIdx.x - scene * n_ch) * PC, pc = min(PC, M - m0);
    const size_t plan0 = (size_t)scene * M + m0;                        // first plan of the chunk
    float* cwc = cw + plan0 * K;                                        // the chunk's [pc, K] table: item it = p * K + k
    float* dc = dist ? dist + plan0 * K : nullptr;
    const int n_it = pc * K;

    // ---- C1: the ego slot of every plan of the chunk, and whether they name one slot
    if (tid < 2) slotL[tid] = tid == 0 ? 0x7fffffff : -1;
    __syncthreads();
    if (tid < pc) {
        int e = ego ? ego[plan0 + tid] : -1;
        if (e < 0 || e >= mno) e = -1;
        egoL[tid] = e;
        ncL[tid] = 0;
        if (e >= 0) { atomicMin(&slotL[0], e); atomicMax(&slotL[1], e); }
    }
    __syncthreads();
    const int e0 = slotL[1];
    const bool staged = rows_in_lds && e0 >= 0 && slotL[0] == e0;       // (the same for every lane)

    for (int t0 = 0; t0 < t_cond; t0 += TC) {
        const int tc = min(TC, t_cond - t0);
        const bool last = t0 + tc == t_cond;
        __syncthreads();                                                // the last pass's walk is over
        eval_stream<PCW_BATCH>(                                         // ---- the plans' frames of the pass
            plans, vecP, pc, tc, EVAL_ONE_ROW, [&](int sg) { return EvalSeg{(plan0 + sg) * T + t0, sg}; },
            [&](int sg, int, int tl, float y0, float y1) { PL[sg * tp + tl] = make_float2(y0, y1); });
        if (staged)                                                     // ---- the K rows of the one ego slot
            eval_stream<PCW_BATCH>(
                Y, vecY, K, tc, EVAL_ONE_ROW, [&](int sg) { return EvalSeg{(((size_t)scene * K + sg) * mno + e0) * T + t0, sg}; },
                [&](int sg, int, int tl, float y0, float y1) { E[sg * tp + tl] = make_float2(y0, y1); });
        __syncthreads();
        for (int it = tid; it < pc * tc; it += EVAL_THREADS) {          // ---- C1: what is not compared gets the marker
            const int p = it / tc, tl = it - p * tc, e = egoL[p];
            bool c = false;
            if (e >= 0) c = fut ? fut[(((size_t)scene * T + t0 + tl) * mno + e) * 3] != 0.f : present[(size_t)scene * mno + e] != 0;
            const float2 v = PL[p * tp + tl];
            if (!(c && v.x == v.x && v.y == v.y)) PL[p * tp + tl].x = __uint_as_float(PCW_MARK);
        }
        __syncthreads();
        if (tid < pc) {                                                 // n_c: the plan's lane counts
            int nc = ncL[tid];
            for (int tl = 0; tl < tc; ++tl) nc += pcw_marked(PL[tid * tp + tl]) ? 0 : 1;
            ncL[tid] = nc;
        }
        __syncthreads();
        for (int it = tid; it < n_it; it += EVAL_THREADS) {             // ---- C2: the walk of (plan p, world k), in increasing t
            const int p = it / K, k = it - p * K, e = egoL[p];
            float S = t0 == 0 ? 0.f : cwc[it];
            if (e >= 0) {
                const float2* prow = PL + p * tp;
                if (staged) {
                    const float2* er = E + k * tp;
#pragma unroll 4
                    for (int tl = 0; tl < tc; ++tl) {
                        const float2 pv = prow[tl], y = er[tl];
                        const float a = (pv.x - y.x) * ux, b = (pv.y - y.y) * uy;
                        const float q = a * a + b * b;
                        S = pcw_marked(pv) ? S : S + q;
                    }
                } else {
                    const float* yr = Y + 2 * ((((size_t)scene * K + k) * mno + e) * T + t0);
#pragma unroll 4
                    for (int tl = 0; tl < tc; ++tl) {
                        const float2 pv = prow[tl];
                        const float a = (pv.x - yr[2 * tl]) * ux, b = (pv.y - yr[2 * tl + 1]) * uy;
                        const float q = a * a + b * b;
                        S = pcw_marked(pv) ? S : S + q;
                    }
                }
            }
            if (last) {
                const int nc = ncL[p];
                S = nc >= 1 ? S / (float)nc : 0.f;                      // D_k; a plan without an ego slot has no compared frame
                if (dc) dc[it] = S;
            }
            cwc[it] = S;
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---- C3 - C6: the lane of plan p
    if (tid < pc) {
        float* cp = cwc + (size_t)tid * K;
        const float* ws = w + (size_t)scene * K;
        const float* ps = prior + (size_t)scene * K;
        const int nc = ncL[tid];
        float sup = 0.f;
        const EvalWeightStats st = eval_weight_stats(
            egoL[tid] >= 0 && nc >= 1, K, [&](int k) { return ps[k] - cp[k] * inv; },
            [&](int k, float ek) {
                sup += ws[k] * expf(-(cp[k] * inv));
                cp[k] = ek;
            });
        const bool conditioned = !st.uniform;
        float s2 = 0.f;
        for (int k = 0; k < K; ++k) {
            const float c = conditioned ? cp[k] / st.sum : ws[k];
            cp[k] = c;
            s2 += c * c;
        }
        if (ess) ess[plan0 + tid] = 1.f / s2;
        if (support) support[plan0 + tid] = conditioned ? sup : 1.f;
        if (cond) cond[plan0 + tid] = conditioned ? nc : 0;
    }
}

}  // namespace

void launch_plan_cond_weights(const EvalIn& in, const PlanIn& pl, const PlanCondParams& p, const EvalScale& sc, const PlanCondOut& o, hipStream_t s) {
    int PC = 0, TC = 0, rows = 0;
    plan_cond_geometry(in.K, p.t_cond, pl.M, &PC, &TC, &rows);
    const size_t lds = PlanCondLds(in.K, PC, TC, rows).bytes();
    const int vecY = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0, vecP = (reinterpret_cast<uintptr_t>(pl.plans) & 15) == 0;
    const size_t n_ch = (size_t)((pl.M + PC - 1) / PC);
    hipLaunchKernelGGL(k_plan_cond_weights, dim3((unsigned)((size_t)in.n_scenes * n_ch)), dim3(EVAL_THREADS), lds, s, in.Y, in.fut, in.present, pl.plans,
                       pl.ego, p.w, p.prior, o.cw, o.dist, o.ess, o.support, o.cond, pl.M, in.mno, in.K, in.T, p.t_cond, PC, TC, rows, vecY, vecP, sc.ux,
                       sc.uy, p.inv);
}
