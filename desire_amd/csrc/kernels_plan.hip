// kernels_plan.hip -- candidate ego plans against the K joint futures of a window (desire_plan_risk; the contract, operation by operation, is in
// include/desire_hip.h): per (plan, joint future) the first contact and the clearance per horizon, per plan the weighted risk per horizon and
// the blame per slot.
//
//   k_plan_weights  one workgroup per window: which slots take part, the K joint scores (desire_joint_metrics' step 7: one lane per k walks the
//                   slots in increasing order), their weight statistics (eval_weight_stats, one lane) and the K weights, into the handle's scratch.
//                   For desire_plan_risk_cond (launch_plan_prior) it also keeps the K logits p_k that kernels_plan_cond.hip conditions.
//   k_plan_risk     one workgroup = (window, chunk of PC plans).  It walks k = 0 .. K (K = the ground truth) and stages each unit's positions as
//                   k_joint_unit does; a lane owns ONE (plan, slot) item for the whole call and walks the frames in increasing t, keeping its
//                   first contact and a running minimum of q in registers.  Over the slots of a plan both are reduced by order-free minima
//                   (a shuffle over 32 lanes or fewer, then an LDS atomic: integers, and the bits of non-negative floats as unsigned integers).
//                   The lane of item (plan, slot) adds W_k into its blame registers, one fixed lane per (plan, horizon) adds W_k into its risk
//                   register: the k order is the loop's, and both are written once at the end.  Its second instantiation (PER_PLAN_W,
//                   launch_plan_risk_per_plan) reads the weight of (plan, k) from desire_plan_risk_cond's table instead of the window's W_k.
//
// The streaming loop over Y, the horizon list and the weight statistics are eval_tile.h's; the LDS plan (PlanLds) and its geometry are eval_lds.h's.
//
// LDS layout.  P is k_joint_unit's: float2 [frame of the pass][slot], frame stride JointLds::stride.  Lane = plan * mno + slot, so the 32 lanes of
// a half wave read 32 consecutive slots of one frame (mno >= 32) or 32 / mno whole plans' slots (mno < 32: the same mno addresses for every
// plan, a broadcast): conflict-free.  The plan position PL [plan][frame], row stride eval_odd(TC) pairs, is one address for every lane of a plan
// and, for mno < 32, 32 / mno addresses an odd number of pairs apart: distinct banks.
//
// The counted mask needs no array: a position that is not counted holds a marker NaN (PLAN_MARK in x), and q of a NaN is a NaN, which neither
// touches (q < r2 is false) nor replaces the minimum (q < mn is false).  When a unit fits the LDS the markers are written once and every later
// unit's rows overwrite only what is not a marker; a row of Y whose x happens to have the marker's bits is stored as another NaN -- the same q.
//
// The minima are carried in registers across the frame chunks of a unit and reduced at each horizon's last frame, so a chunked walk gives the bits of
// an unchunked one.  No float atomics, no host synchronisation, horizons by value: capturable, bitwise reproducible, a window's results depend on
// that window only.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int PR_BATCH = 4;                    // 16-byte loads a lane has in flight
constexpr unsigned PLAN_MARK = 0x7fc0a5a5u;    // x of a position that is not counted: a quiet NaN
constexpr unsigned PLAN_INF = 0x7f800000u;     // +inf: where a clearance starts

__device__ __forceinline__ bool plan_marked(const float2& v) { return __float_as_uint(v.x) == PLAN_MARK; }

// minimum over groups of `width` consecutive lanes (a power of two, 32 at most); every lane of the wave calls it
__device__ __forceinline__ unsigned plan_group_min(unsigned v, int width) {
    for (int o = width >> 1; o > 0; o >>= 1) {
        const unsigned u = (unsigned)__shfl_xor((int)v, o);
        v = u < v ? u : v;
    }
    return v;
}

// KEEP_PRIOR: desire_plan_risk_cond's launch also keeps prior [n_scenes, K] = the logits p_k
template <bool KEEP_PRIOR>
__global__ __launch_bounds__(EVAL_THREADS) void k_plan_weights(const float* __restrict__ fut, const uint8_t* __restrict__ present,
                                                             const float* __restrict__ score, float* w, float* __restrict__ prior, int mno,
                                                             int K, int T) {
    __shared__ int part[EVAL_THREADS];                                  // mno <= 256: the slot takes part before T_pred
    __shared__ float stL[2];
    __shared__ int uniL;
    const int tid = threadIdx.x, scene = blockIdx.x;
    float* ws = w + (size_t)scene * K;
    for (int i = tid; i < mno; i += EVAL_THREADS) {
        bool c = false;
        if (fut)
            for (int t = 0; t < T; ++t) c |= fut[(((size_t)scene * T + t) * mno + i) * 3] != 0.f;
        else c = present[(size_t)scene * mno + i] != 0;
        part[i] = c ? 1 : 0;
    }
    __syncthreads();
    if (score)
        for (int k = tid; k < K; k += EVAL_THREADS) {                   // desire_joint_metrics' step 7: increasing slot from 0.f
            const float* sr = score + ((size_t)scene * K + k) * mno;
            float s = 0.f;
            for (int i = 0; i < mno; ++i)
                if (part[i]) s += sr[i];
            ws[k] = s;
        }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        const EvalWeightStats st = eval_weight_stats(score != nullptr, K, [&](int k) { return ws[k]; }, [](int, float) {});
        stL[0] = st.mx; stL[1] = st.sum; uniL = st.uniform ? 1 : 0;
    }
    __syncthreads();
    const bool uni = uniL != 0;
    const float mx = stL[0], sum = stL[1];
    for (int k = tid; k < K; k += EVAL_THREADS) {
        if (KEEP_PRIOR) prior[(size_t)scene * K + k] = uni ? 0.f : ws[k];  // p_k: the joint score where every one of the window is finite
        ws[k] = uni ? 1.f / (float)K : expf(ws[k] - mx) / sum;
    }
}

// PER_PLAN_W: w is desire_plan_risk_cond's table [n_scenes, M, K] -- the blame lane reads its plan's row, the risk lane its own -- instead of the
// window's K weights
template <bool PER_PLAN_W>
__global__ __launch_bounds__(EVAL_THREADS) void k_plan_risk(const float* __restrict__ Y, const float* __restrict__ fut,
                                                          const uint8_t* __restrict__ present, const float* __restrict__ plans,
                                                          const int32_t* __restrict__ ego, const float* __restrict__ w,
                                                          int32_t* __restrict__ first_out, float* __restrict__ clear_out, float* __restrict__ risk,
                                                          float* __restrict__ blame, int M, int mno, int K, int T, int PC, int TC, int vecY,
                                                          int vecP, float sx, float sy, float ux, float uy, float r2, RankHz hz) {
    extern __shared__ float2 pr_sm[];
    __shared__ int hzs[8];
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4 && sizeof(unsigned) == 4 && PlanLds::HZ == 8);
    const PlanLds L(mno, PC, TC);
    const int mp = JointLds::stride(mno), tp = L.plan_stride();
    float2* PL = pr_sm;                                                 // [PC, tp]
    float2* P = PL + L.plans();                                         // [TC, mp]
    int* words = reinterpret_cast<int*>(P + L.pos());                   // two sets of first [PC] and clear [PC, HZ]
    const int tid = threadIdx.x, n_h = hz.n;
    const int n_ch = (M + PC - 1) / PC;
    const int scene = blockIdx.x / n_ch, m0 = (blockIdx.x - scene * n_ch) * PC, pc = min(PC, M - m0);
    const size_t plan0 = (size_t)scene * M + m0;                        // first plan of the chunk
    // ---- the lane's item (plan p, slot i); a lane without one, and the slot the plan replaces, walk plan 0 and keep nothing
    const int p = tid / mno, i = tid - p * mno;
    bool active = p < pc;
    if (active && ego) active = ego[plan0 + p] != i;
    const int pp = p < pc ? p : 0;
    const float r2l = active ? r2 : -1.f;                               // q < -1 never holds
    const int width = min(mno, 32);                                     // lanes of one plan in a row: mno divides 32 or is a multiple of it
    const bool lead = (tid & (width - 1)) == 0;
    // ---- the lane of (plan rp, horizon rh): risk, and the rows of first / clear
    const int rp = tid / n_h, rh = tid - rp * n_h;
    const bool rlane = rp < pc;
    const float nanf_ = __uint_as_float(PLAN_MARK);
    eval_stage_horizons(hzs, hz);
    for (int j = tid; j < L.first(PlanLds::SETS); j += EVAL_THREADS) {
        const int r = j % L.first(1);
        words[j] = r < PC ? T : (int)PLAN_INF;
    }
    float bl[PlanLds::HZ];
#pragma unroll
    for (int hi = 0; hi < PlanLds::HZ; ++hi) bl[hi] = 0.f;
    float rk = 0.f;

    const bool chunked = TC < T;
    const int k_end = present ? K : K + 1;                              // no ground truth without dev_fut
    for (int k = 0; k < k_end; ++k) {
        const bool gt = k == K;
        const size_t U0 = (((size_t)scene * K + k) * mno) * T;          // the unit's first (row, t) pair (k < K)
        int* firstL = words + L.first(k & 1);
        unsigned* clrL = reinterpret_cast<unsigned*>(words + L.clear(k & 1));
        int fi = T, hi = 0;
        float mn = __uint_as_float(PLAN_INF);
        for (int t0 = 0; t0 < T; t0 += TC) {
            const int tc = min(TC, T - t0), n_it = tc * mno;
            __syncthreads();                                            // the last pass's walk is over (and the words are initialised)
            if (chunked || k == 0)                                      // ---- the plans' frames of the pass
                eval_stream<PR_BATCH>(
                    plans, vecP, chunked ? pc : 1, chunked ? tc : pc * T, chunked ? EVAL_ONE_ROW : T,
                    [&](int sg) { return EvalSeg{(plan0 + (chunked ? sg : 0)) * T + (chunked ? t0 : 0), sg}; },
                    [&](int sg, int row, int tl, float y0, float y1) { PL[(chunked ? sg : row) * tp + tl] = make_float2(y0, y1); });
            if (chunked || k == 0 || gt) {                              // ---- the counted mask of the pass; the ground truth's positions with it
                for (int it = tid; it < n_it; it += EVAL_THREADS) {
                    const int tl = it / mno, s = it - tl * mno, t = t0 + tl;
                    bool c;
                    float2 v = make_float2(0.f, 0.f);
                    if (fut) {
                        const float* f = fut + (((size_t)scene * T + t) * mno + s) * 3;
                        c = f[0] != 0.f;
                        if (gt) v = make_float2(__fmul_rn(f[1], sx), __fmul_rn(f[2], sy));
                    } else c = present[(size_t)scene * mno + s] != 0;
                    P[tl * mp + s] = c ? v : make_float2(nanf_, nanf_);
                }
                __syncthreads();
            }
            if (!gt) {                                                  // ---- the unit's rows, as k_joint_unit stages them
                eval_stream<PR_BATCH>(
                    Y, vecY, chunked ? mno : 1, chunked ? tc : mno * T, chunked ? EVAL_ONE_ROW : T,
                    [&](int sg) { return EvalSeg{U0 + (chunked ? (size_t)sg * T + t0 : 0), sg}; },
                    [&](int sg, int row, int tl, float y0, float y1) {
                        const int o = tl * mp + (chunked ? sg : row);
                        if (!plan_marked(P[o]))                         // counted: the last unit's position gives way to this one's
                            P[o] = make_float2(__float_as_uint(y0) == PLAN_MARK ? __builtin_nanf("") : y0, y1);
                    });
            }
            __syncthreads();
            // ---- the walk: q of (plan, slot) frame by frame, in increasing t
            const float2* prow = PL + pp * tp;
            const float2* ycol = P + i;
            for (int tl = 0; tl < tc;) {                                // runs of frames up to the next horizon: no branch inside a run
                const int hnext = hi < n_h ? hzs[hi] : T + 1;           // (the same for every lane)
                const int end = min(tc, hnext - t0);
#pragma unroll 4
                for (; tl < end; ++tl) {
                    const float2 y = ycol[tl * mp], pv = prow[tl];
                    const float a = (pv.x - y.x) * ux, b = (pv.y - y.y) * uy;
                    const float q = a * a + b * b;
                    fi = q < r2l ? min(fi, t0 + tl) : fi;
                    mn = q < mn ? q : mn;
                }
                if (t0 + tl == hnext) {                                 // the horizon's frames are through: its clearance
                    const unsigned v = plan_group_min(active ? __float_as_uint(mn) : PLAN_INF, width);
                    if (lead && v != PLAN_INF) atomicMin(&clrL[pp * PlanLds::HZ + hi], v);
                    ++hi;
                }
            }
        }
        // ---- first contact of the plan: an integer minimum over its slots
        {
            const int v = (int)plan_group_min((unsigned)fi, width);     // 0 .. T: ordered alike as unsigned
            if (lead && v < T) atomicMin(&firstL[pp], v);
        }
        const float wk = gt ? 0.f : w[PER_PLAN_W ? (plan0 + pp) * K + k : (size_t)scene * K + k];
        if (!gt) {
#pragma unroll
            for (int h = 0; h < PlanLds::HZ; ++h)
                if (h < n_h && fi < hz.h[h]) bl[h] += wk;
        }
        __syncthreads();
        if (rlane) {
            const int f = firstL[rp];
            if (!gt && f < hzs[rh]) rk += PER_PLAN_W ? w[(plan0 + rp) * K + k] : wk;
            const size_t row = (plan0 + rp) * (K + 1) + k;
            if (first_out && rh == 0) first_out[row] = f;
            if (clear_out) clear_out[row * n_h + rh] = __uint_as_float(clrL[rp * PlanLds::HZ + rh]);
        }
        // the other parity's set is clean again before unit k + 1 reduces into it: its readers (unit k - 1) are a barrier behind, and the next
        // unit's first atomic is a barrier ahead
        for (int j = tid; j < L.first(1); j += EVAL_THREADS) words[L.first((k + 1) & 1) + j] = j < PC ? T : (int)PLAN_INF;
    }

    // ---- outputs that are written once
    if (rlane) {
        risk[(plan0 + rp) * n_h + rh] = rk;
        if (present) {                                                  // no ground truth: row K says so
            const size_t row = (plan0 + rp) * (K + 1) + K;
            if (first_out && rh == 0) first_out[row] = T;
            if (clear_out) clear_out[row * n_h + rh] = __uint_as_float(PLAN_INF);
        }
    }
    if (blame && p < pc) {
#pragma unroll
        for (int h = 0; h < PlanLds::HZ; ++h)
            if (h < n_h) blame[((plan0 + p) * n_h + h) * mno + i] = bl[h];
    }
}

}  // namespace

// w: the window's weights [n_scenes, K], or with PER_PLAN_W every plan's [n_scenes, M, K]
template <bool PER_PLAN_W>
static void plan_risk_launch(const EvalIn& in, const PlanIn& pl, const float* w, const RankHz& hz, const EvalScale& sc, float radius, const PlanOut& o,
                             hipStream_t s) {
    int PC = 0, TC = 0;
    plan_geometry(in.mno, in.T, pl.M, &PC, &TC);
    const size_t lds = PlanLds(in.mno, PC, TC).bytes();
    const int vecY = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0, vecP = (reinterpret_cast<uintptr_t>(pl.plans) & 15) == 0;
    const size_t n_ch = (size_t)((pl.M + PC - 1) / PC);
    hipLaunchKernelGGL(k_plan_risk<PER_PLAN_W>, dim3((unsigned)((size_t)in.n_scenes * n_ch)), dim3(EVAL_THREADS), lds, s, in.Y, in.fut, in.present,
                       pl.plans, pl.ego, w, o.first, o.clear, o.risk, o.blame, pl.M, in.mno, in.K, in.T, PC, TC, vecY, vecP, sc.sx, sc.sy, sc.ux, sc.uy,
                       radius * radius, hz);
}

void launch_plan_risk(const EvalIn& in, const PlanIn& pl, const RankHz& hz, const EvalScale& sc, float radius, const PlanOut& o, hipStream_t s) {
    hipLaunchKernelGGL(k_plan_weights<false>, dim3(in.n_scenes), dim3(EVAL_THREADS), 0, s, in.fut, in.present, in.score, o.w,
                       static_cast<float*>(nullptr), in.mno, in.K, in.T);
    plan_risk_launch<false>(in, pl, o.w, hz, sc, radius, o, s);
}

void launch_plan_prior(const EvalIn& in, const PlanPriorOut& o, hipStream_t s) {
    hipLaunchKernelGGL(k_plan_weights<true>, dim3(in.n_scenes), dim3(EVAL_THREADS), 0, s, in.fut, in.present, in.score, o.w, o.prior, in.mno, in.K, in.T);
}

void launch_plan_risk_per_plan(const EvalIn& in, const PlanIn& pl, const float* cw, const RankHz& hz, const EvalScale& sc, float radius, const PlanOut& o,
                               hipStream_t s) {
    plan_risk_launch<true>(in, pl, cw, hz, sc, radius, o, s);
}
