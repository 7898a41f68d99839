// kernels_joint.hip -- the K samples of a window as K joint futures of the scene (desire_joint_metrics; the contract, operation by operation, is
// in include/desire_hip.h): first contact of every slot with any other slot of its (window, k), the counts per horizon, the joint errors
// (JADE / JFDE), the joint score, its order and the pick through that order.
//
//   k_joint_unit   one workgroup = one (window, k), k = K being the ground truth.  The unit's positions go to LDS once per frame chunk, a lane
//                  owns (slot i, frame t) and loops over the partners j, the first contact is an integer minimum in LDS; then one lane per
//                  (horizon, column) walks the slots in increasing order: the counts, the sums of the per-agent (ADE_h, FDE_h), the joint score.
//   k_joint_pick   one wave per window: the order of the K joint scores (desire_rank_samples' rule, by counting: an integer path) and the pick.
//
// The streaming loop over Y, the order rule, the pick and the horizon list are eval_tile.h's; the LDS plan (JointLds) and the frame chunk are
// eval_lds.h's.
//
// LDS layout.  P is float2 [frame of the chunk][slot], frame stride `mp` pairs: mp = mno below 32 slots (mno then divides 32) and mno + 1 from
// 32 on.  The items of the pair loop are numbered frame-major, so the 32 lanes of a half wave -- the group a ds_read_b64 banks over, bank =
// (address / 4) mod 64 -- hold 32 consecutive slots of one frame (mno >= 32) or 32 / mno whole frames (mno < 32): 256 contiguous bytes, or
// contiguous runs one pair apart that together cover fewer than 64 dwords, so a lane's OWN position is read conflict-free.  The PARTNER (t, j) is
// one address for every lane of a frame -- a broadcast -- and for mno < 32 the 32 / mno frames of a half wave read 32 / mno addresses 2 mno
// dwords apart: distinct banks.  The + 1 from 32 slots on is for the staging WRITES: Y arrives row-major (consecutive lanes = consecutive
// frames of one slot), and an even frame stride of 64 dwords or more would put every store of a half wave on one bank (32-way); the odd
// stride leaves it 4-way on a twentieth of the reads' instruction count.
//
// The counted mask needs no array of its own: a position that is not counted is stored as a NaN pair.  Differences, products and sums carry the
// NaN into q, and `q < r2` is false for a NaN -- exactly c(i,t) && c(j,t) && q < r2, and a NaN row of Y never touches by the same comparison.
//
// `first` is an LDS atomicMin and not a one-lane walk: the minimum of integers does not depend on the order of its operands, so the atomic is
// as deterministic as the walk, and it keeps every lane of the frame-parallel pair loop busy where the walk would serialise T_pred frames behind
// one lane per slot.  It lives in LDS across the frame chunks, so a chunked unit gives the bits of an unchunked one.
//
// Errors: the per-agent (ADE_h, FDE_h) are NOT recomputed here.  desire_joint_metrics fills desire_ranked_errors' table [R, n_h, 2] with that
// call's own kernel (k_sample_errors) and this kernel sums a unit's rows in increasing slot: the bits of the parent's table by construction
// (its file is compiled with the compiler's default contraction, so a second statement of the same expression in a file that rounds every
// operation once need not give the same bits).  The price is a second pass over Y and the table's bytes.
//
// No float atomics, no host synchronisation, horizons by value: capturable, bitwise reproducible, a window's results depend on that window only.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int JM_BATCH = 4;                    // 16-byte loads a lane has in flight

__global__ __launch_bounds__(EVAL_THREADS) void k_joint_unit(const float* __restrict__ Y, const float* __restrict__ fut,
                                                           const uint8_t* __restrict__ present, const float* __restrict__ score,
                                                           const float* __restrict__ tab, int32_t* __restrict__ first_out,
                                                           int32_t* __restrict__ cnt, float* __restrict__ jerr, float* __restrict__ jscore, int mno,
                                                           int K, int T, int TC, int vec, float sx, float sy, float ux, float uy, float r2,
                                                           RankHz hz) {
    extern __shared__ float2 jm_sm[];
    __shared__ int hzs[8];
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4);
    const int mp = JointLds::stride(mno);
    float2* P = jm_sm;                                                  // [TC, mp]
    int* firstL = reinterpret_cast<int*>(P + JointLds(mno, TC).pairs());    // [mno] first contact, T = none
    int* tc0L = firstL + mno;                                           // [mno] first counted frame, T = never counted
    const int tid = threadIdx.x;
    const int scene = blockIdx.x / (K + 1), k = blockIdx.x - scene * (K + 1);
    const bool gt = k == K;
    const size_t r0 = ((size_t)scene * K + k) * mno;                    // first row of the unit (k < K)
    const size_t U0 = r0 * T;                                           // its first (row, t) pair
    const float nanf_ = __builtin_nanf("");
    eval_stage_horizons(hzs, hz);
    for (int i = tid; i < mno; i += EVAL_THREADS) {
        firstL[i] = T;
        tc0L[i] = (present && !gt && present[(size_t)scene * mno + i]) ? 0 : T;
    }
    __syncthreads();

    const bool chunked = TC < T;
    for (int t0 = 0; t0 < T && !(gt && present); t0 += TC) {
        const int tc = min(TC, T - t0), n_it = tc * mno;
        // ---- the counted mask of the chunk: (0, 0) where counted, a NaN pair where not; the ground-truth unit's positions with it
        for (int it = tid; it < n_it; it += EVAL_THREADS) {
            const int tl = it / mno, i = it - tl * mno, t = t0 + tl;
            bool c;
            float2 v = make_float2(0.f, 0.f);
            if (fut) {
                const float* f = fut + (((size_t)scene * T + t) * mno + i) * 3;
                c = f[0] != 0.f;
                if (gt) v = make_float2(__fmul_rn(f[1], sx), __fmul_rn(f[2], sy));
                if (c) atomicMin(&tc0L[i], t);
            } else c = tc0L[i] == 0;
            P[tl * mp + i] = c ? v : make_float2(nanf_, nanf_);
        }
        __syncthreads();
        // ---- the unit's rows: contiguous over (slot, t) when the chunk is the whole horizon, else one segment of tc pairs per slot
        if (!gt) {
            eval_stream<JM_BATCH>(
                Y, vec, chunked ? mno : 1, chunked ? tc : mno * T, chunked ? EVAL_ONE_ROW : T,
                [&](int sg) { return EvalSeg{U0 + (chunked ? (size_t)sg * T + t0 : 0), sg}; },
                [&](int sg, int row, int tl, float y0, float y1) {
                    const int o = tl * mp + (chunked ? sg : row);
                    if (P[o].x == P[o].x) P[o] = make_float2(y0, y1);   // counted: the marker gives way to the position
                });
            __syncthreads();
        }
        // ---- pair tests: a lane owns (i, t) and walks the partners; q is symmetric in (i, j) bit for bit (a, b only change sign)
        for (int it = tid; it < n_it; it += EVAL_THREADS) {
            const int tl = it / mno, i = it - tl * mno;
            const float2* row = P + tl * mp;
            const float2 p = row[i];
            if (p.x != p.x) continue;                                   // not counted (or a NaN row): q would be a NaN for every partner
            bool touch = false;
#pragma unroll 4
            for (int j = 0; j < mno; ++j) {
                const float2 q = row[j];
                const float a = (p.x - q.x) * ux, b = (p.y - q.y) * uy;
                const float d = a * a + b * b;
                touch |= (d < r2) & (j != i);
            }
            if (touch) atomicMin(&firstL[i], t0 + tl);
        }
        __syncthreads();
    }

    // ---- outputs.  One lane per (horizon, column) walks the slots in increasing order: integers, and float sums in one fixed order from 0.f
    const size_t unit = (size_t)scene * (K + 1) + k;
    if (first_out)
        for (int i = tid; i < mno; i += EVAL_THREADS) first_out[unit * mno + i] = firstL[i];
    const int n_h = hz.n;
    if (tid < 2 * n_h) {
        const int hi = tid >> 1, col = tid & 1, h = hzs[hi];
        const float* tb = (tab && !gt) ? tab + (r0 * n_h + hi) * 2 + col : nullptr;
        int nf = 0, nt = 0;
        float s = 0.f;
        for (int i = 0; i < mno; ++i) {
            const bool tp = tc0L[i] < h;
            nt += tp ? 1 : 0;
            nf += firstL[i] < h ? 1 : 0;
            if (tp && tb) s += tb[(size_t)i * n_h * 2];
        }
        cnt[(unit * n_h + hi) * 2 + col] = col ? nt : nf;
        if (tb && jerr) jerr[((r0 / mno) * n_h + hi) * 2 + col] = nt ? s / (float)nt : 0.f;
    } else if (tid == 2 * n_h && !gt && jscore) {
        float s = 0.f;
        if (score)
            for (int i = 0; i < mno; ++i)
                if (tc0L[i] < T) s += score[r0 + i];
        jscore[r0 / mno] = s;
    }
}

// The order of a window's K joint scores: rank_k = #{ j : s_j before s_k } (eval_before, desire_rank_samples' rule), read from global memory
// so that K has no limit.  Then out [n_h, 4] through that order (eval_pick, as k_ranked_pick picks).
__global__ __launch_bounds__(64) void k_joint_pick(const float* __restrict__ js, const float* __restrict__ jerr, const int32_t* __restrict__ cnt,
                                                   int32_t* __restrict__ jorder, float* __restrict__ out, int K, int n_h, int n_top) {
    const int scene = blockIdx.x, lane = threadIdx.x;
    const float* s = js + (size_t)scene * K;
    int32_t* ord = jorder + (size_t)scene * K;
    for (int k = lane; k < K; k += 64) {
        const float sk = s[k];
        int r = 0;
        for (int j = 0; j < K; ++j) r += eval_before(s[j], j, sk, k) ? 1 : 0;
        ord[r] = k;
    }
    if (!out) return;
    __threadfence_block();
    __syncthreads();
    for (int hi = lane; hi < n_h; hi += 64) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cnt[(((size_t)scene * (K + 1)) * n_h + hi) * 2 + 1] > 0)    // taking part does not depend on k: row 0
            o = eval_pick(ord, n_top, [&](int k) { return jerr + (((size_t)scene * K + k) * n_h + hi) * 2; });
        float* op = out + ((size_t)scene * n_h + hi) * 4;
        op[0] = o.x; op[1] = o.y; op[2] = o.z; op[3] = o.w;
    }
}

}  // namespace

void launch_joint_metrics(const EvalIn& in, const JointParams& p, const RankHz& hz, const EvalScale& sc, const JointOut& o, hipStream_t s) {
    const int TC = joint_chunk_frames(in.mno, in.T);
    const size_t lds = JointLds(in.mno, TC).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0;
    hipLaunchKernelGGL(k_joint_unit, dim3((unsigned)((size_t)in.n_scenes * (in.K + 1))), dim3(EVAL_THREADS), lds, s, in.Y, in.fut, in.present, in.score,
                       p.tab, o.first, o.cnt, o.jerr, o.jscore, in.mno, in.K, in.T, TC, vec, sc.sx, sc.sy, sc.ux, sc.uy, p.radius * p.radius, hz);
    hipLaunchKernelGGL(k_joint_pick, dim3(in.n_scenes), dim3(64), 0, s, o.jscore, o.jerr, o.cnt, o.jorder, o.out, in.K, hz.n, p.n_top);
}
