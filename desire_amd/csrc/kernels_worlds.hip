// kernels_worlds.hip -- score-ordered non-maximum suppression of a window's K joint futures ("worlds": sample k of every slot together;
// desire_select_worlds; the contract, operation by operation, is in include/desire_hip.h).
//
//   k_select_worlds<METRIC>  one workgroup = one window.  It ranks the window's K world scores (eval_before, by counting), lists the slots that
//                  take part, and runs the greedy pass: per KEPT world its rows of a chunk of taking-part slots go to LDS; every lane owns
//                  (live candidate, slot) items and walks its own row of Y in increasing t with 16-byte loads of two frames, against the
//                  kept row in LDS; one lane per candidate then reduces the chunk's slots in increasing slot into the candidate's running
//                  sum / conjunction.  After the last chunk a candidate that is near is owned by the world just kept -- it was near no world
//                  kept before, so this is the first kept world it is near, the contract's owner.  One lane lays out order, count, mass and
//                  label, which leave the workgroup with coalesced stores.
//
// This is form (b) of the two the design admits (DESIGN.md section 7k counts the work): count sequential steps of about K predicates, no K x K
// state, so K has no limit beyond the per-world words of the LDS plan.  A predicate is mno * t_end pair distances, and a window's K worlds do
// not fit LDS together (20 x 32 x 40 positions are 205 KB), so the candidates' rows are read from Y once per kept world: count * (K - 1) *
// mno rows per window, from L2 after the first step.
//
// The chunks run over the slots and not over the frames: a slot's value (q, m or s) is then finished by one lane inside one chunk, in one
// fixed sequence, and what is carried across chunks is the per-world reduction alone -- the sum of d_i in increasing slot from 0.f, or the
// conjunction -- which a chunked walk performs in the very order of an unchunked one.  Slots that do not take part are never staged and never
// read.  LDS rows of the kept world are float2 [t], row stride (frames staged | 1) pairs: the lanes of a wave sit on consecutive slots and the
// same t, so they fall on distinct bank pairs.  No atomics, no host synchronisation: capturable, bitwise reproducible, and a window's result
// depends on that window's taking-part rows, scores and presence only.  The LDS plan (WorldsLds) and the slot chunk are eval_lds.h's.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int SW_LIVE = -1;                    // st[j]: not yet kept or owned
constexpr int SW_KEPT = 1 << 30;               // st[j] = i | SW_KEPT: kept as number i; st[j] = i: owned by kept number i

// desire_select_diverse's steps 1 - 2 on one slot of (candidate, kept): the candidate's row from Y (p0 = its first staged pair), the kept row
// from LDS.  FINAL: q; MAX: m; MEAN: s -- the contract's sequence, symmetric in the two rows bit for bit (a, b only change sign).
template <int METRIC>
__device__ __forceinline__ float sw_value(const float* __restrict__ Y, size_t p0, int vec, const float2* __restrict__ kr, int nt, float ux,
                                          float uy) {
    float acc = 0.f;
    auto step = [&](float y0, float y1, int t) {
        const float2 k = kr[t];
        const float a = (y0 - k.x) * ux, b = (y1 - k.y) * uy;
        const float d = a * a + b * b;
        if constexpr (METRIC == DESIRE_DIST_MEAN) acc += sqrtf(d);
        else if constexpr (METRIC == DESIRE_DIST_MAX) acc = (t == 0 || d > acc || d != d) ? d : acc;      // a NaN stays: it is never near
        else acc = d;
    };
    int t = 0;
    if (vec) {                                                          // quads at even pair indices of a 16-byte aligned buffer
        if (p0 & 1) { step(Y[2 * p0], Y[2 * p0 + 1], 0); t = 1; }
#pragma unroll 4
        for (; t + 1 < nt; t += 2) {
            const float4 v = *reinterpret_cast<const float4*>(Y + 2 * (p0 + t));
            step(v.x, v.y, t);
            step(v.z, v.w, t + 1);
        }
    }
    for (; t < nt; ++t) step(Y[2 * (p0 + t)], Y[2 * (p0 + t) + 1], t);
    return acc;
}

template <int METRIC>
__global__ __launch_bounds__(EVAL_THREADS) void k_select_worlds(const float* __restrict__ Y, const uint8_t* __restrict__ present,
                                                              const float* __restrict__ wscore, int32_t* __restrict__ worder,
                                                              int32_t* __restrict__ wcount, float* __restrict__ wmass,
                                                              int32_t* __restrict__ wlabel, int mno, int K, int T, int t_end, int SC, int vec,
                                                              int reduce, float radius, float ux, float uy) {
    extern __shared__ float2 sw_sm[];
    __shared__ int nlS, npS;
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4 && sizeof(float) == 4 && WorldsLds::K_WORDS == 9);
    const int nt = SelLds::staged(METRIC, t_end), t_lo = t_end - nt;
    const WorldsLds L(nt, SC, K, mno);
    const int Fp = L.Fp, DS = L.dv_stride();
    float2* Yk = sw_sm;                                                 // [SC, Fp] the kept world's rows of the chunk
    int* wd = reinterpret_cast<int*>(Yk + L.pairs());                   // the words behind the pairs
    int* dvi = wd + L.dv();                                             // [K, DS] near_i (DESIRE_WORLD_ALL)
    float* dvf = reinterpret_cast<float*>(dvi);                         //         d_i    (DESIRE_WORLD_MEAN)
    int* ordL = wd + L.k_words(0);                                      // [K] the processing order
    int* st = wd + L.k_words(1);                                        // [K] state of candidate j (by processing position)
    float* wL = reinterpret_cast<float*>(wd + L.k_words(2));            // [K] score, then weight, of world k
    int* outL = wd + L.k_words(3);                                      // [K] the order out
    float* massL = reinterpret_cast<float*>(wd + L.k_words(4));         // [K]
    int* labL = wd + L.k_words(5);                                      // [K] label of world k
    float* accD = reinterpret_cast<float*>(wd + L.k_words(6));          // [K] running sum of d_i of candidate c
    int* accA = wd + L.k_words(7);                                      // [K] running conjunction of near_i of candidate c
    int* live = wd + L.k_words(8);                                      // [K] the live processing positions, increasing
    int* slotL = wd + L.slots();                                        // [mno] the taking-part slots, increasing

    const int tid = threadIdx.x;
    const size_t scene = blockIdx.x;
    const float* ws = wscore ? wscore + scene * K : nullptr;
    const bool all = reduce == DESIRE_WORLD_ALL;

    // ---- the scores, the taking-part slots, then the processing order (by counting) and the weights (desire_plan_risk's step 6)
    for (int k = tid; k < K; k += EVAL_THREADS) {
        wL[k] = ws ? ws[k] : 0.f;
        st[k] = SW_LIVE;
        massL[k] = 0.f;
    }
    if (tid < 64) {
        const uint8_t* pr = present ? present + scene * mno : nullptr;
        const int n = eval_compact(mno, slotL, [&](int i) { return !pr || pr[i] != 0; });
        if (tid == 0) npS = n;
    }
    __syncthreads();
    for (int k = tid; k < K; k += EVAL_THREADS) {
        int r = k;
        if (ws) {
            const float sk = wL[k];
            r = 0;
            for (int j = 0; j < K; ++j) r += eval_before(wL[j], j, sk, k) ? 1 : 0;
        }
        ordL[r] = k;
    }
    __syncthreads();
    if (tid == 0 && wmass) {
        const EvalWeightStats s = eval_weight_stats(ws != nullptr, K, [&](int k) { return wL[k]; }, [&](int k, float e) { wL[k] = e; });
        const float u = 1.f / (float)K;
        for (int k = 0; k < K; ++k) wL[k] = s.uniform ? u : wL[k] / s.sum;
    }
    const int np = npS;
    const bool test = radius > 0.f && np > 0;                           // else the predicate needs no row: never near / always near

    // ---- the greedy pass: one step per kept world
    int cnt = 0;
    for (;;) {
        __syncthreads();                                                // the states of the last step
        if (tid < 64) {
            const int n = eval_compact(K, live, [&](int j) { return st[j] == SW_LIVE; });
            if (tid == 0) nlS = n;
        }
        __syncthreads();
        const int nl = nlS;
        if (nl == 0) break;
        const int jk = live[0], kk = ordL[jk], nc = nl - 1;             // the first live candidate is kept; live[1 ..] are tested against it
        for (int c = tid; c < nc; c += EVAL_THREADS) { accD[c] = 0.f; accA[c] = 1; }
        if (test && nc > 0) {
            const size_t rk = (scene * K + kk) * mno;
            for (int s0 = 0; s0 < np; s0 += SC) {
                const int ns = min(SC, np - s0);
                __syncthreads();                                        // the last chunk's readers are done
                for (int it = tid; it < ns * nt; it += EVAL_THREADS) {
                    const int s = it / nt, t = it - s * nt;
                    const size_t e = ((rk + slotL[s0 + s]) * T + t_lo + t) * 2;
                    Yk[s * Fp + t] = make_float2(Y[e], Y[e + 1]);
                }
                __syncthreads();
                for (int it = tid; it < nc * ns; it += EVAL_THREADS) {
                    const int c = it / ns, s = it - c * ns;
                    const size_t p0 = ((scene * K + ordL[live[1 + c]]) * mno + slotL[s0 + s]) * T + t_lo;
                    const float v = sw_value<METRIC>(Y, p0, vec, Yk + s * Fp, nt, ux, uy);
                    if (all) {
                        bool near;
                        if constexpr (METRIC == DESIRE_DIST_MEAN) near = v / (float)nt < radius;
                        else near = v < radius * radius;
                        dvi[c * DS + s] = near ? 1 : 0;
                    } else {
                        float d;
                        if constexpr (METRIC == DESIRE_DIST_MEAN) d = v / (float)nt;
                        else d = sqrtf(v);
                        dvf[c * DS + s] = d;
                    }
                }
                __syncthreads();
                for (int c = tid; c < nc; c += EVAL_THREADS) {          // increasing slot: the chunks continue one sequence
                    if (all) {
                        int a = accA[c];
                        for (int s = 0; s < ns; ++s) a &= dvi[c * DS + s];
                        accA[c] = a;
                    } else {
                        float d = accD[c];
                        for (int s = 0; s < ns; ++s) d += dvf[c * DS + s];
                        accD[c] = d;
                    }
                }
            }
        }
        __syncthreads();
        for (int c = tid; c < nc; c += EVAL_THREADS) {
            bool near;
            if (!test) near = radius > 0.f;                             // radius 0: nothing is near; nobody takes part: everything is
            else if (all) near = accA[c] != 0;
            else near = accD[c] / (float)np < radius;
            if (near) st[live[1 + c]] = cnt;
        }
        if (tid == 0) st[jk] = cnt | SW_KEPT;
        ++cnt;
    }

    // ---- one lane: kept in keeping order, then owned in processing order; mass in processing order; the label of every world
    if (tid == 0) {
        int no = cnt;
        for (int j = 0; j < K; ++j) {
            const int o = st[j] & ~SW_KEPT, k = ordL[j];
            if (st[j] & SW_KEPT) outL[o] = k;
            else outL[no++] = k;
            if (wmass) massL[o] += wL[k];
            labL[k] = o;
        }
        wcount[scene] = cnt;
    }
    __syncthreads();
    for (int k = tid; k < K; k += EVAL_THREADS) {
        worder[scene * K + k] = outL[k];
        if (wmass) wmass[scene * K + k] = massL[k];
        if (wlabel) wlabel[scene * K + k] = labL[k];
    }
}

}  // namespace

void launch_select_worlds(const EvalIn& in, const WorldsParams& p, const EvalScale& sc, const WorldsOut& o, hipStream_t s) {
    int SC = 1;
    if (!worlds_geometry(in.mno, in.K, p.metric, p.t_end, &SC)) return;           // (refused by the caller before it gets here)
    const size_t lds = WorldsLds(SelLds::staged(p.metric, p.t_end), SC, in.K, in.mno).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0;
    const dim3 grid((unsigned)in.n_scenes), block(EVAL_THREADS);
#define SW_LAUNCH(M)                                                                                                                            \
    hipLaunchKernelGGL(k_select_worlds<M>, grid, block, lds, s, in.Y, in.present, in.score, o.worder, o.wcount, o.wmass, o.wlabel, in.mno, in.K, \
                       in.T, p.t_end, SC, vec, p.reduce, p.radius, sc.ux, sc.uy)
    if (p.metric == DESIRE_DIST_FINAL) SW_LAUNCH(DESIRE_DIST_FINAL);
    else if (p.metric == DESIRE_DIST_MAX) SW_LAUNCH(DESIRE_DIST_MAX);
    else SW_LAUNCH(DESIRE_DIST_MEAN);
#undef SW_LAUNCH
}
