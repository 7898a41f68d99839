// eval_tile.h -- the device pieces that the evaluation kernels over the sample tensor Y [R, T_pred, 2] share, each stated once: the streaming
// loop over Y, the order rule of the scores, the pick through an order, the horizon list and its walk, the weight statistics of the scores, the compaction of a predicate.
// The sinks and everything that is arithmetic on positions stay in the kernels.
//
// RULE: no floating-point multiply that feeds an add in this header.  kernels_rank.hip is compiled with the compiler's default contraction,
// the other files (kernels_offroad.hip among them) set `#pragma clang fp contract(off)` AFTER their includes, so this header is compiled under the default in every
// file: a product-sum here could be fused in all of them.  What is here is integer index work, comparisons, expf(a - b), plain sums and one
// division; every product-sum (the distance, the density, the moments) belongs in the including file, behind its pragma.
#pragma once
#include "common.h"
#include "kernels.h"

#include <cfloat>

// ---- the streamer.  n_seg segments of seg_len (row, t) pairs each, a segment being whole rows of row_len pairs, or part of one row (row_len =
// EVAL_ONE_ROW, a runtime value: every pair comes out as row 0, the split itself still runs).  seg(sg) gives segment sg's first pair index in Y and a tag for the sink;
// every pair of every segment reaches sink(tag, row within the segment, t within the row, y0, y1) exactly once.  The tag is whatever the
// kernel wants to derive from sg once per item instead of once per pair:
//   k_sample_errors   the segment's first row in the error region (sg * rows per segment)
//   k_joint_unit      sg: the slot when the unit is walked in frame chunks (one segment per slot, EVAL_ONE_ROW), 0 for the whole unit
//   k_recon_weights   sg: the sample of the pass
//   k_occupancy       sg: the sample of the chunk (one segment per sample: a run of one row's frames, EVAL_ONE_ROW)
//   k_collision_unit, k_offroad_unit   k_joint_unit's: sg, the slot of a frame chunk's segment, 0 for the whole unit
// An item is (segment, quad): a quad is two pairs at an even pair index of the buffer, and seg_len / 2 + 1 quads cover a segment at either
// parity of its first index.  A lane issues the BATCH 16-byte loads of its items before it consumes any; a quad that straddles its segment's
// ends, and every quad of a buffer off 16-byte alignment (vec == 0), takes 8-byte loads of the pairs that are inside.  With one segment its
// descriptor is formed once, outside the loop, and no item pays the division by the quads per segment.  Called by all EVAL_THREADS lanes of
// the workgroup: a kernel that uses it launches EVAL_THREADS lanes.  k_select_diverse stages a part of every row with the same item loop
// written out in its own file: through this function it measured 1 - 3 % slower (kernels_select.hip says where).
struct EvalSeg { size_t first; int tag; };
constexpr int EVAL_ONE_ROW = 0x7fffffff;
template <int BATCH, class Seg, class Sink>
__device__ __forceinline__ void eval_stream(const float* __restrict__ Y, int vec, int n_seg, int seg_len, int row_len, Seg seg, Sink sink) {
    const int nq = seg_len / 2 + 1, n_items = n_seg * nq;
    const EvalSeg d0 = seg(0);                                         // (index arithmetic only: harmless without a segment)
    for (int i0 = threadIdx.x; i0 < n_items; i0 += EVAL_THREADS * BATCH) {
        float4 v[BATCH];
        size_t ps[BATCH], qq[BATCH];
        int tag[BATCH];
        bool full[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int it = i0 + u * EVAL_THREADS;
            full[u] = false;
            if (it >= n_items) continue;
            int sg = 0;
            EvalSeg d = d0;
            if (n_seg > 1) { sg = it / nq; d = seg(sg); }
            ps[u] = d.first; tag[u] = d.tag;
            qq[u] = (ps[u] >> 1) + (size_t)(it - sg * nq);
            const size_t p = 2 * qq[u];
            full[u] = vec && p >= ps[u] && p + 1 < ps[u] + seg_len;
            if (full[u]) v[u] = *reinterpret_cast<const float4*>(Y + 4 * qq[u]);
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            if (i0 + u * EVAL_THREADS >= n_items) break;
            const size_t p = 2 * qq[u];
            if (full[u]) {
                const int rel = (int)(p - ps[u]);
                int r = rel / row_len, t = rel - r * row_len;            // one integer division per quad
                sink(tag[u], r, t, v[u].x, v[u].y);
                if (++t == row_len) { t = 0; ++r; }
                sink(tag[u], r, t, v[u].z, v[u].w);
            } else {
                for (size_t pp = p; pp < p + 2; ++pp) {
                    if (pp < ps[u] || pp >= ps[u] + seg_len) continue;       // the neighbouring segment's pair, or nobody's
                    const int rel = (int)(pp - ps[u]), r = rel / row_len;
                    sink(tag[u], r, rel - r * row_len, Y[2 * pp], Y[2 * pp + 1]);
                }
            }
        }
    }
}

// ---- the order rule: is (score sj, index j) before (sk, k)?  IEEE > on the fp32 scores, ties (-0 == +0 among them) to the lower index, NaNs
// after everything else and among themselves by index -- a strict total order, so rank_k = #{ j : j before k } is a permutation of 0 .. K-1.
__device__ __forceinline__ bool eval_before(float sj, int j, float sk, int k) {
    const bool nk = sk != sk;
    return (sj != sj) ? (nk && j < k) : (nk || sj > sk || (sj == sk && j < k));
}

// ---- the compaction of a predicate: called by wave 0 alone (lanes 0 .. 63 of the workgroup); out[0 .. n) = the i < N with pred(i), in increasing
// i; n comes back in every lane of the wave.
template <class Pred>
__device__ __forceinline__ int eval_compact(int N, int* out, Pred pred) {
    const int lane = threadIdx.x;
    int n = 0;
    for (int b = 0; b < N; b += 64) {
        const int i = b + lane;
        const bool p = i < N && pred(i);
        const unsigned long long m = __ballot(p);
        if (p) out[n + __popcll(m & ((1ull << lane) - 1ull))] = i;
        n += __popcll(m);
    }
    return n;
}

// ---- the pick through an order row: (ADE, FDE of the first entry; min over the n_top first entries of ADE, of FDE), tab(k) being the
// (ADE, FDE) pair of sample k.  The minimum keeps a NaN (a NaN trajectory is reported, not hidden).
template <class Tab>
__device__ __forceinline__ float4 eval_pick(const int32_t* ord, int n_top, Tab tab) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < n_top; ++j) {
        const float* e = tab(ord[j]);
        const float ade = e[0], fde = e[1];
        if (j == 0) o = make_float4(ade, fde, ade, fde);
        else {
            if (ade < o.z || ade != ade) o.z = ade;
            if (fde < o.w || fde != fde) o.w = fde;
        }
    }
    return o;
}

// ---- the horizon list (by value in the kernel arguments) into hzs [8] of LDS; the caller's next barrier publishes it
__device__ __forceinline__ void eval_stage_horizons(int* hzs, const RankHz& hz) {
    if (threadIdx.x < 8) hzs[threadIdx.x] = (int)threadIdx.x < hz.n ? hz.h[threadIdx.x] : 0;
}
// One lane walks a row's T values in increasing t (the fixed summation order): the sum, the last value and the number of the counted frames
// (mr[t] != 0) so far go to emit(hi, sum, last, np) at each horizon.
template <class Emit>
__device__ __forceinline__ void eval_horizon_walk(const float* mr, const float* vr, const int* hzs, int n_h, Emit emit) {
    const int h_max = hzs[n_h - 1];
    float sum = 0.f, last = 0.f;
    int np = 0, hi = 0;
    for (int t = 0; t < h_max; ++t) {
        if (mr[t] != 0.f) { last = vr[t]; sum += last; ++np; }          // frames the object is absent from carry no value
        if (t + 1 == hzs[hi]) { emit(hi, sum, last, np); ++hi; }
    }
}

// ---- the weight statistics of an agent's K scores s(k): weight k is expf(s(k) - mx) / sum, or 1 / K for every k when `uniform` -- no scores,
// or one of them is not finite (NaN, +-inf).  The sum runs in increasing k from 0.f; park(k, expf(s(k) - mx)) lets a caller that can overwrite
// its scores keep the numerators (a serial lane then pays one expf per k, not two); a caller that cannot recomputes them: the same bits.
struct EvalWeightStats { bool uniform; float mx, sum; };
template <class Score, class Park>
__device__ __forceinline__ EvalWeightStats eval_weight_stats(bool scored, int K, Score s, Park park) {
    EvalWeightStats st{!scored, -FLT_MAX, 0.f};
    if (!st.uniform) {
        for (int k = 0; k < K; ++k) {
            const float v = s(k);
            if (!(fabsf(v) <= FLT_MAX)) st.uniform = true;
            st.mx = fmaxf(st.mx, v);
        }
    }
    if (!st.uniform)
        for (int k = 0; k < K; ++k) { const float e = expf(s(k) - st.mx); park(k, e); st.sum += e; }
    return st;
}
