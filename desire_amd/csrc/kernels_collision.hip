// kernels_collision.hip -- the collision penalty of the K joint futures of a window (desire_collision_loss, desire_set_collision_loss; the
// contract, operation by operation, is in include/desire_hip.h): a squared hinge in the distance of every pair of counted slots of one
// (window, k) and frame, its sum per agent, the number of touching (pair, frame)s, the term and its gradient with respect to Y.
//
//   k_collision_unit   one workgroup = one (window, k), on k_joint_unit's plan: the unit's positions go to LDS once per frame chunk as float2
//                      [frame][slot] (JointLds' frame stride), a not-counted position as a NaN pair, so that `q < r2` alone is the pair rule.  A
//                      lane owns (slot i, frame t) items with i fastest and walks the partners j: P[t][j] and 1 / nfut[j] are one LDS address
//                      per frame -- a broadcast -- and s(i, t) and the two gradient components stay in registers; the pair rule runs for a
//                      block of 32 partners first, the root and the divisions then for the partners that touch alone.  They are parked slot-major
//                      (CollLds: [slot][frame], odd stride), then one lane per slot adds its s(i, .) in increasing t to the slot's running sum --
//                      the contract's one sequence, carried in LDS across the chunks, so a chunked unit has the bits of an unchunked one -- and
//                      the gradient leaves in row order: a quad of two (row, t) pairs per lane at an even pair index, 16 bytes where the quad
//                      lies inside the unit's segment and the buffer is aligned (a lane-per-item store would stride by 8 T_pred bytes).  In the
//                      training step that pass is the read-modify-write dY0 = dY0 + weight * G; every element has one owner.
//   k_collision_term   one workgroup: the mean over K per agent, the agents in a fixed order, divided by nvalid.
//
// Each (i, t) gathers its own sum over j: nothing scatters, there are no float atomics.  `touch` counts the pairs j > i in integers (per lane,
// then an integer atomicAdd in LDS: the sum of integers does not depend on the order of its operands).  No host synchronisation: capturable,
// bitwise reproducible, a window's results depend on that window's rows and targets only.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int CL_BATCH = 4;                    // 16-byte loads a lane has in flight

template <bool ACC>
__global__ __launch_bounds__(EVAL_THREADS) void k_collision_unit(const float* __restrict__ Y, const float* __restrict__ fut,
                                                               const uint8_t* __restrict__ lmask, const float* __restrict__ nfut,
                                                               const float* __restrict__ nvalid, float* __restrict__ col,
                                                               int32_t* __restrict__ touch, float* __restrict__ dY, int mno, int K, int T, int TC,
                                                               int vec, int vec_out, float ux, float uy, float radius, float weight) {
    extern __shared__ float2 cl_sm[];
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4 && sizeof(float) == 4);
    const CollLds L(mno, TC);
    const int mp = JointLds::stride(mno), tp = L.park_stride();
    float2* P = cl_sm;                                                  // [TC, mp]
    float2* Gl = P + L.pos();                                           // [mno, tp] the gradient of the chunk
    float* words = reinterpret_cast<float*>(Gl + L.grad());
    float* Sl = words;                                                  // [mno, tp] s(i, t) of the chunk
    float* invL = words + L.slot_words(0);                              // [mno] 1 / nfut where lmask, else 0
    float* accL = words + L.slot_words(1);                              // [mno] the sum of s so far
    int* touchL = reinterpret_cast<int*>(words + L.unit_words());
    const int tid = threadIdx.x;
    const int scene = blockIdx.x / K, k = blockIdx.x - scene * K;
    const size_t r0 = ((size_t)scene * K + k) * mno;                    // first row of the unit
    const size_t U0 = r0 * T;                                           // its first (row, t) pair
    const float nanf_ = __builtin_nanf("");
    const float r2 = radius * radius;
    const float nk = nvalid[0] * (float)K, scale = -2.f / nk;
    for (int i = tid; i < mno; i += EVAL_THREADS) {
        const size_t a = (size_t)scene * mno + i;
        invL[i] = lmask[a] ? 1.f / nfut[a] : 0.f;
        accL[i] = 0.f;
    }
    if (tid == 0) *touchL = 0;
    __syncthreads();

    const bool chunked = TC < T;
    int nt = 0;
    for (int t0 = 0; t0 < T; t0 += TC) {
        const int tc = min(TC, T - t0), n_it = tc * mno;
        // ---- the counted mask of the chunk: (0, 0) where counted, a NaN pair where not
        for (int it = tid; it < n_it; it += EVAL_THREADS) {
            const int tl = it / mno, i = it - tl * mno, t = t0 + tl;
            const bool c = invL[i] != 0.f && fut[(((size_t)scene * T + t) * mno + i) * 3] != 0.f;
            P[tl * mp + i] = c ? make_float2(0.f, 0.f) : make_float2(nanf_, nanf_);
        }
        __syncthreads();
        // ---- the unit's rows: contiguous over (slot, t) when the chunk is the whole horizon, else one segment of tc pairs per slot
        eval_stream<CL_BATCH>(
            Y, vec, chunked ? mno : 1, chunked ? tc : mno * T, chunked ? EVAL_ONE_ROW : T,
            [&](int sg) { return EvalSeg{U0 + (chunked ? (size_t)sg * T + t0 : 0), sg}; },
            [&](int sg, int row, int tl, float y0, float y1) {
                const int o = tl * mp + (chunked ? sg : row);
                if (P[o].x == P[o].x) P[o] = make_float2(y0, y1);       // counted: the marker gives way to the position
            });
        __syncthreads();
        // ---- pairs: a lane owns (i, t) and walks the partners in increasing j; q is symmetric in (i, j) bit for bit (a, b only change sign)
        for (int it = tid; it < n_it; it += EVAL_THREADS) {
            const int tl = it / mno, i = it - tl * mno;
            const float2* row = P + tl * mp;
            const float2 p = row[i];
            float s = 0.f, gx = 0.f, gy = 0.f;
            if (p.x == p.x) {                                           // else not counted (or a NaN row): q would be a NaN for every partner
                const float inv_i = invL[i];
                // Two steps per block of 32 partners: the pair rule alone for all of them (the broadcast reads, six operations a pair), its
                // outcome one bit each; then the root and the two divisions for the set bits only, in increasing j.  A wave whose lanes
                // branched on every partner would run the long path whenever ANY of its 64 lanes touches -- most partners at a few
                // per cent of touching pairs -- where this runs it as often as the busiest lane has partners.
                for (int j0 = 0; j0 < mno; j0 += 32) {
                    const int jn = min(32, mno - j0);
                    unsigned hit = 0u;
#pragma unroll 4
                    for (int jj = 0; jj < jn; ++jj) {
                        const float2 o = row[j0 + jj];
                        const float a = (p.x - o.x) * ux, b = (p.y - o.y) * uy;
                        const float q = a * a + b * b;
                        hit |= (q < r2 ? 1u : 0u) << jj;
                    }
                    if (i >= j0 && i < j0 + 32) hit &= ~(1u << (i - j0));       // j != i
                    while (hit) {
                        const int j = j0 + __ffs(hit) - 1;
                        hit &= hit - 1u;
                        const float2 o = row[j];
                        const float a = (p.x - o.x) * ux, b = (p.y - o.y) * uy;     // the same operations: the same bits
                        const float q = a * a + b * b;
                        const float dist = sqrtf(q), u = 1.f - dist / radius;
                        s += u * u;
                        nt += j > i ? 1 : 0;
                        if (dist > 0.f) {
                            const float c = (inv_i + invL[j]) * (u / (radius * dist));
                            gx += c * a;
                            gy += c * b;
                        }
                    }
                }
            }
            Sl[i * tp + tl] = s;
            Gl[i * tp + tl] = make_float2((gx * ux) * scale, (gy * uy) * scale);
        }
        __syncthreads();
        // ---- one lane per slot: its s(i, .) in increasing t onto the running sum (a frame that is not counted holds 0.f, which changes no bit)
        for (int i = tid; i < mno; i += EVAL_THREADS) {
            float a = accL[i];
            for (int tl = 0; tl < tc; ++tl) a += Sl[i * tp + tl];
            accL[i] = a;
        }
        // ---- the gradient leaves in row order: a lane takes a quad (two pairs at an even pair index of the buffer) of a segment
        {
            const int n_seg = chunked ? mno : 1, seg_len = chunked ? tc : mno * T, nq = seg_len / 2 + 1;
            for (int it = tid; it < n_seg * nq; it += EVAL_THREADS) {
                const int sg = n_seg > 1 ? it / nq : 0;
                const size_t ps = U0 + (chunked ? (size_t)sg * T + t0 : 0);
                const size_t qq = (ps >> 1) + (size_t)(it - sg * nq);
                float2 g[2];
                bool in[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const size_t pp = 2 * qq + e;
                    in[e] = pp >= ps && pp < ps + seg_len;
                    g[e] = make_float2(0.f, 0.f);
                    if (in[e]) {
                        const int rel = (int)(pp - ps), slot = chunked ? sg : rel / T, tl = chunked ? rel : rel - slot * T;
                        g[e] = Gl[slot * tp + tl];
                    }
                }
                if (in[0] && in[1] && vec_out) {
                    float4* d = reinterpret_cast<float4*>(dY + 4 * qq);
                    float4 o = make_float4(g[0].x, g[0].y, g[1].x, g[1].y);
                    if (ACC) {
                        const float4 v = *d;
                        o = make_float4(v.x + weight * o.x, v.y + weight * o.y, v.z + weight * o.z, v.w + weight * o.w);
                    }
                    *d = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        if (!in[e]) continue;
                        float* d = dY + 2 * (2 * qq + e);
                        if (ACC) { d[0] = d[0] + weight * g[e].x; d[1] = d[1] + weight * g[e].y; }
                        else { d[0] = g[e].x; d[1] = g[e].y; }
                    }
                }
            }
        }
        __syncthreads();
    }

    if (nt) atomicAdd(touchL, nt);                                      // integers: any order gives the same sum
    __syncthreads();
    for (int i = tid; i < mno; i += EVAL_THREADS) {
        const size_t a = (size_t)scene * mno + i;
        col[a * K + k] = lmask[a] ? accL[i] / nfut[a] : 0.f;
    }
    if (tid == 0) touch[(size_t)scene * K + k] = *touchL;
}

// L_col: per agent the sum of col[a, .] in increasing k from 0.f over (float)K; lane l adds the agents a = l, l + 256, .. in increasing a from
// 0.f (col is 0.f where lmask = 0); the 256 partial sums meet in a binary tree, red[l] += red[l + st] for st = 128 .. 1; the root over nvalid.
__global__ __launch_bounds__(256) void k_collision_term(const float* __restrict__ col, const float* __restrict__ nvalid, float* __restrict__ term,
                                                        int A, int K) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int a = tid; a < A; a += 256) {
        float m = 0.f;
        for (int k = 0; k < K; ++k) m += col[(size_t)a * K + k];
        s += m / (float)K;
    }
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) term[0] = red[0] / nvalid[0];
}

}  // namespace

void launch_collision_loss(const EvalIn& in, const CollParams& p, const EvalScale& sc, const CollOut& o, hipStream_t s) {
    const int TC = coll_chunk_frames(in.mno, in.T);
    const size_t lds = CollLds(in.mno, TC).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0, vec_out = (reinterpret_cast<uintptr_t>(o.dY) & 15) == 0;
    const dim3 grid((unsigned)((size_t)in.n_scenes * in.K));
    auto* kern = p.accumulate ? k_collision_unit<true> : k_collision_unit<false>;
    hipLaunchKernelGGL(kern, grid, dim3(EVAL_THREADS), lds, s, in.Y, in.fut, p.lmask, p.nfut, p.nvalid, o.col, o.touch, o.dY, in.mno, in.K, in.T, TC, vec,
                       vec_out, sc.ux, sc.uy, p.radius, p.weight);
    launch_collision_term(o.col, p.nvalid, o.term, in.n_scenes * in.mno, in.K, s);
}

void launch_collision_term(const float* val, const float* nvalid, float* term, int A, int K, hipStream_t s) {
    hipLaunchKernelGGL(k_collision_term, dim3(1), dim3(256), 0, s, val, nvalid, term, A, K);
}
