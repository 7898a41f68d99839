// kernels_offroad.hip -- the off-road penalty of the K joint futures of a window (desire_mask_distance, desire_offroad_loss,
// desire_set_offroad_loss; the contracts, operation by operation, are in include/desire_hip.h): the exact distance field of a traversability mask,
// and against it a squared distance per counted (agent, sample, frame), its sum per agent, the number of off-road (slot, frame)s, the term and
// its gradient with respect to Y.
//
//   k_mask_columns     pass 1 of the field: one lane per column x' sweeps it down and up; g(y, x') = the integer distance in rows to the nearest
//                      traversable cell of that column (MD_NONE: the column has none), parked in the field buffer itself as integers.
//   k_mask_rows        pass 2: one workgroup per (mask, row y) takes the row of g into LDS and overwrites it with the field: per cell the min over
//                      the columns that hold a traversable cell of ((x - x') * cell_x)^2 + (g(y, x') * cell_y)^2, then the root.  The rounded
//                      expression is monotone in |y - y'|, so the nearest cell of a column is that column's minimiser, and a min does not depend
//                      on the order of its operands: the bits of the brute-force statement.  g(y, .) is one LDS address per step -- a broadcast.
//   k_offroad_unit     one workgroup = one (window, k) on k_collision_unit's plan (OffLds): the unit's positions go to LDS once per frame chunk
//                      through the shared row streamer, a not-counted position as a NaN pair; the window's field sits behind them when it fits
//                      (STAGED), else the four taps are gathered from global memory -- the same values, the same bits.  A lane owns (slot i, frame
//                      t) items: lookup, phi and the two gradient components, parked slot-major; one lane per slot then adds its phi(i, .) in
//                      increasing t to the slot's running sum (carried in LDS across the chunks: a chunked unit has the bits of an unchunked one),
//                      and the gradient leaves in row order as 16-byte quads where alignment allows.  In the training step that pass is the
//                      read-modify-write dY0 = dY0 + weight * G; every element has one owner.
//   (the term)         launch_collision_term: the mean over K per agent, the agents in a fixed order, divided by nvalid.
//
// Nothing scatters, there are no float atomics; `count` is summed in integers (per lane, then an integer atomicAdd in LDS).  No host
// synchronisation: capturable, bitwise reproducible, a window's results depend on that window's rows, targets and field only.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contracts round every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int OF_BATCH = 4;                    // 16-byte loads a lane has in flight
constexpr int MD_NONE = 0x7fffffff;            // g of a column without a traversable cell

__global__ __launch_bounds__(EVAL_THREADS) void k_mask_columns(const uint8_t* __restrict__ mask, int32_t* __restrict__ g, int Mh, int Mw) {
    const int x = blockIdx.x * EVAL_THREADS + threadIdx.x;
    if (x >= Mw) return;
    const size_t base = (size_t)blockIdx.y * Mh * Mw + x;
    int d = MD_NONE;
    for (int y = 0; y < Mh; ++y) {                                      // down: the nearest traversable cell at or above
        const size_t o = base + (size_t)y * Mw;
        d = mask[o] ? 0 : (d == MD_NONE ? MD_NONE : d + 1);
        g[o] = d;
    }
    d = MD_NONE;
    for (int y = Mh - 1; y >= 0; --y) {                                 // up: at or below, the smaller of the two stays
        const size_t o = base + (size_t)y * Mw;
        d = mask[o] ? 0 : (d == MD_NONE ? MD_NONE : d + 1);
        g[o] = min(g[o], d);
    }
}

__global__ __launch_bounds__(EVAL_THREADS) void k_mask_rows(float* field, int Mw, float cell_x, float cell_y) {
    __shared__ int gl[DESIRE_OCC_MAX_SIDE];
    float* row = field + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * Mw;
    const int32_t* grow = reinterpret_cast<const int32_t*>(row);
    for (int x = threadIdx.x; x < Mw; x += EVAL_THREADS) gl[x] = grow[x];
    __syncthreads();                                                    // every read of the row's integers is behind this: the row is overwritten
    for (int x = threadIdx.x; x < Mw; x += EVAL_THREADS) {
        float best = 0.f;
        bool any = false;
        for (int xs = 0; xs < Mw; ++xs) {
            const int gv = gl[xs];
            if (gv == MD_NONE) continue;
            const float a = (float)(x - xs) * cell_x, b = (float)gv * cell_y;
            const float q = a * a + b * b;
            best = any ? fminf(best, q) : q;
            any = true;
        }
        row[x] = any ? sqrtf(best) : 0.f;                               // a mask without a traversable cell: 0.f everywhere, no constraint
    }
}

template <bool ACC, bool STAGED>
__global__ __launch_bounds__(EVAL_THREADS) void k_offroad_unit(const float* __restrict__ Y, const float* __restrict__ fut,
                                                             const uint8_t* __restrict__ lmask, const float* __restrict__ nfut,
                                                             const float* __restrict__ nvalid, const float* __restrict__ field,
                                                             const int32_t* __restrict__ field_of_scene, float* __restrict__ off,
                                                             int32_t* __restrict__ count, float* __restrict__ dY, int mno, int K, int T, int TC,
                                                             int vec, int vec_out, int Mh, int Mw, float scale, float weight) {
    extern __shared__ float2 of_sm[];
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4 && sizeof(float) == 4);
    const OffLds L(mno, TC, STAGED ? Mh * Mw : 0);
    const int mp = JointLds::stride(mno), tp = L.c.park_stride();
    float2* P = of_sm;                                                  // [TC, mp]
    float2* Gl = P + L.c.pos();                                         // [mno, tp] the gradient of the chunk
    float* words = reinterpret_cast<float*>(Gl + L.c.grad());
    float* Sl = words;                                                  // [mno, tp] phi(i, t) of the chunk
    float* invL = words + L.c.slot_words(0);                            // [mno] 1 / nfut where counted at all, else 0
    float* accL = words + L.c.slot_words(1);                            // [mno] the sum of phi so far
    int* countL = reinterpret_cast<int*>(words + L.c.unit_words());
    float* Fl = words + L.field_words();                                // [Mh, Mw] when STAGED
    const int tid = threadIdx.x;
    const int scene = blockIdx.x / K, k = blockIdx.x - scene * K;
    const size_t r0 = ((size_t)scene * K + k) * mno;                    // first row of the unit
    const size_t U0 = r0 * T;                                           // its first (row, t) pair
    const float nanf_ = __builtin_nanf("");
    const int fi = field_of_scene[scene];                               // negative: the window has no field, nothing of it is counted
    const float* Fg = field + (size_t)(fi < 0 ? 0 : fi) * Mh * Mw;
    const float* F = STAGED ? Fl : Fg;
    const float fMw = (float)Mw, fMh = (float)Mh, xmax = (float)(Mw - 1), ymax = (float)(Mh - 1);
    const float nk = nvalid[0] * (float)K;
    for (int i = tid; i < mno; i += EVAL_THREADS) {
        const size_t a = (size_t)scene * mno + i;
        invL[i] = (fi >= 0 && lmask[a]) ? 1.f / nfut[a] : 0.f;
        accL[i] = 0.f;
    }
    if (STAGED && fi >= 0)
        for (int c = tid; c < Mh * Mw; c += EVAL_THREADS) Fl[c] = Fg[c];
    if (tid == 0) *countL = 0;
    __syncthreads();

    const bool chunked = TC < T;
    int nc = 0;
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
        eval_stream<OF_BATCH>(
            Y, vec, chunked ? mno : 1, chunked ? tc : mno * T, chunked ? EVAL_ONE_ROW : T,
            [&](int sg) { return EvalSeg{U0 + (chunked ? (size_t)sg * T + t0 : 0), sg}; },
            [&](int sg, int row, int tl, float y0, float y1) {
                const int o = tl * mp + (chunked ? sg : row);
                if (P[o].x == P[o].x) P[o] = make_float2(y0, y1);       // counted: the marker gives way to the position
            });
        __syncthreads();
        // ---- a lane owns (i, t): the lookup, phi and the gradient; a NaN coordinate (or a position that is not counted) costs and pushes nothing
        for (int it = tid; it < n_it; it += EVAL_THREADS) {
            const int tl = it / mno, i = it - tl * mno;
            const float2 p = P[tl * mp + i];
            float phi = 0.f, gx = 0.f, gy = 0.f;
            if (p.x == p.x && p.y == p.y) {
                const float xm = p.x * fMw, ym = p.y * fMh;
                const float u = xm - 0.5f, v = ym - 0.5f;
                const float uc = fminf(fmaxf(u, 0.f), xmax), vc = fminf(fmaxf(v, 0.f), ymax);
                const float ufl = floorf(uc), vfl = floorf(vc);
                const int x0 = (int)ufl, y0 = (int)vfl, x1 = min(x0 + 1, Mw - 1), y1 = min(y0 + 1, Mh - 1);
                const float fx = uc - ufl, fy = vc - vfl;
                const float D00 = F[y0 * Mw + x0], D01 = F[y0 * Mw + x1], D10 = F[y1 * Mw + x0], D11 = F[y1 * Mw + x1];
                const float h0 = D01 - D00, h1 = D11 - D10;
                const float top = D00 + fx * h0, bot = D10 + fx * h1;
                const float vd = bot - top;
                const float d = top + fy * vd;
                const float e = d / scale;
                phi = e * e;
                float sx = (h0 + fy * (h1 - h0)) * fMw, sy = vd * fMh;
                if (!(u >= 0.f && u <= xmax)) sx = 0.f;                 // clamped: the lookup does not move with x
                if (!(v >= 0.f && v <= ymax)) sy = 0.f;
                const float m = (2.f * e) / scale, coef = invL[i] / nk;
                gx = (m * sx) * coef;
                gy = (m * sy) * coef;
                // the count: desire_occupancy's cell (no clamp), off-road where the field is positive there
                const float cx = floorf(xm), cy = floorf(ym);
                if (cx >= 0.f && cx <= xmax && cy >= 0.f && cy <= ymax && F[(int)cy * Mw + (int)cx] > 0.f) ++nc;
            }
            Sl[i * tp + tl] = phi;
            Gl[i * tp + tl] = make_float2(gx, gy);
        }
        __syncthreads();
        // ---- one lane per slot: its phi(i, .) in increasing t onto the running sum (a frame that is not counted holds 0.f, which changes no bit)
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
                        const float4 w = *d;
                        o = make_float4(w.x + weight * o.x, w.y + weight * o.y, w.z + weight * o.z, w.w + weight * o.w);
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

    if (nc) atomicAdd(countL, nc);                                      // integers: any order gives the same sum
    __syncthreads();
    for (int i = tid; i < mno; i += EVAL_THREADS) {
        const size_t a = (size_t)scene * mno + i;
        off[a * K + k] = invL[i] != 0.f ? accL[i] / nfut[a] : 0.f;
    }
    if (tid == 0) count[(size_t)scene * K + k] = *countL;
}

}  // namespace

void launch_mask_distance(const uint8_t* mask, int n_masks, int Mh, int Mw, float cell_x, float cell_y, float* field, hipStream_t s) {
    hipLaunchKernelGGL(k_mask_columns, dim3((unsigned)eval_chunks(Mw, EVAL_THREADS), (unsigned)n_masks), dim3(EVAL_THREADS), 0, s, mask,
                       reinterpret_cast<int32_t*>(field), Mh, Mw);
    hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)Mh, (unsigned)n_masks), dim3(EVAL_THREADS), 0, s, field, Mw, cell_x, cell_y);
}

void launch_offroad_loss(const EvalIn& in, const OffParams& p, const OffOut& o, hipStream_t s) {
    int TC = 0, staged = 0;
    offroad_geometry(in.mno, in.T, p.Mh, p.Mw, &TC, &staged);
    const size_t lds = OffLds(in.mno, TC, staged ? p.Mh * p.Mw : 0).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0, vec_out = (reinterpret_cast<uintptr_t>(o.dY) & 15) == 0;
    const dim3 grid((unsigned)((size_t)in.n_scenes * in.K));
    auto* kern = p.accumulate ? (staged ? k_offroad_unit<true, true> : k_offroad_unit<true, false>)
                              : (staged ? k_offroad_unit<false, true> : k_offroad_unit<false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(EVAL_THREADS), lds, s, in.Y, in.fut, p.lmask, p.nfut, p.nvalid, p.field, p.field_of_scene, o.off, o.count,
                       o.dY, in.mno, in.K, in.T, TC, vec, vec_out, p.Mh, p.Mw, p.scale, p.weight);
    launch_collision_term(o.off, p.nvalid, o.term, in.n_scenes * in.mno, in.K, s);
}
