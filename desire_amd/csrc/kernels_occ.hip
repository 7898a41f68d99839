// kernels_occ.hip -- predicted occupancy maps of the K weighted samples of every agent of a window (desire_occupancy; the contract, operation by
// operation, is in include/desire_hip.h): per (window, horizon) the expected number of agents per cell E, the probability that at least one
// agent is there 1 - q, and per agent the off-frame mass, the mass on cells the mask forbids and the mass on the ground truth's cell.
//
//   k_occupancy    one workgroup = one (window, horizon, band of grid rows).  E, q and the marginal P of one agent live in LDS over the band's
//                  cells.  The agents are walked in increasing slot.  An agent's positions arrive in chunks of KC samples x FC frames through
//                  eval_tile.h's streamer; the sink turns a position into its cell id (or a marker: not counted, off frame) in LDS and raises
//                  the sample's `off` / `viol` flags.  Then, for the chunk's samples in increasing k, the lanes of that sample's frames add w_k
//                  into P.  In mode UNTIL a sample must add to a cell once however often it comes back: the lane exchanges the sample's stamp
//                  (slot * K + k + 1, unique within the workgroup) into the cell's word of S, and only the lane that did not find the stamp there
//                  adds -- an integer exchange, whose one winner per (sample, cell) adds the same w_k whoever it is.  The winners of one sample hold
//                  distinct cells, and a barrier separates the samples, so P[c] is the sum over k in increasing k from 0.f with no float atomic.
//                  After the agent's last chunk every lane folds its cells of P into E and q and clears them: per cell one fixed sequence of
//                  operations in slot order.  One lane per column sums `off`, `viol` and `hit` over k in increasing k.
//
// A band's cells see exactly the operations an unbanded call applies to them, so banding does not change a bit; the per-agent columns do not
// depend on the band and are written by band 0.  The chunking only groups the samples (and, for horizons beyond OccLds::ENTRIES frames, the
// frames of one sample): the order of the additions to a cell is k's in every grouping.
//
// The LDS plan (OccLds) and its geometry are eval_lds.h's; the streaming loop and the horizon list are eval_tile.h's; the weights are
// desire_kde_nll's (k_kde_weights, the handle's "kde_w").  No float atomics, no host synchronisation, horizons by value: capturable, bitwise
// reproducible, a window's results depend on that window only.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr int OC_BATCH = 4;                    // 16-byte loads a lane has in flight
constexpr int OC_NOT_COUNTED = -1, OC_OFF_FRAME = -2;      // markers in the id region (a cell id is >= 0)

// the cell of a position, or OC_OFF_FRAME: one rounded multiply per axis, floorf, no clamp; a NaN fails every comparison
__device__ __forceinline__ int occ_cell(float x, float y, int Oh, int Ow) {
    const float fx = floorf(x * (float)Ow), fy = floorf(y * (float)Oh);
    const bool in = fx >= 0.f && fx <= (float)(Ow - 1) && fy >= 0.f && fy <= (float)(Oh - 1);
    return in ? (int)fy * Ow + (int)fx : OC_OFF_FRAME;
}

__global__ __launch_bounds__(EVAL_THREADS) void k_occupancy(const float* __restrict__ Y, const float* __restrict__ fut,
                                                          const uint8_t* __restrict__ present, const float* __restrict__ w,
                                                          const uint8_t* __restrict__ mask, const int32_t* __restrict__ mask_of_scene,
                                                          float* __restrict__ occ, float* __restrict__ expv, float* __restrict__ hit,
                                                          float* __restrict__ viol, float* __restrict__ off, int mno, int K, int T, int Oh, int Ow,
                                                          int until, int KC, int FC, int rows, int n_bands, int vec, float sx, float sy, RankHz hz) {
    extern __shared__ float oc_sm[];
    EVAL_LDS_TIED(sizeof(float) == 4 && sizeof(int) == 4 && sizeof(unsigned) == 4);
    const int tid = threadIdx.x;
    const int n_h = hz.n;
    const int band = blockIdx.x % n_bands, wh = blockIdx.x / n_bands, hi = wh % n_h, scene = wh / n_h;
    const int h = hz.h[hi];
    const int f_lo = until ? 0 : h - 1, F = until ? h : 1;            // the frames of a sample this workgroup walks: f_lo .. f_lo + F - 1
    const int row_lo = band * rows, n_rows = min(rows, Oh - row_lo);
    const int cells = n_rows * Ow, cell_lo = row_lo * Ow;
    const OccLds L(rows * Ow, KC * FC, until);
    float* El = oc_sm + L.E();
    float* ql = oc_sm + L.q();
    float* Pl = oc_sm + L.P();
    unsigned* Sl = reinterpret_cast<unsigned*>(oc_sm + L.S());
    int* idl = reinterpret_cast<int*>(oc_sm + L.chunk(0));
    float* wl = oc_sm + L.chunk(1);
    int* offl = reinterpret_cast<int*>(oc_sm + L.chunk(2));
    int* violl = reinterpret_cast<int*>(oc_sm + L.chunk(3));
    int* cml = reinterpret_cast<int*>(oc_sm + L.chunk(4));

    for (int c = tid; c < cells; c += EVAL_THREADS) {
        El[c] = 0.f; ql[c] = 1.f; Pl[c] = 0.f;
        if (until) Sl[c] = 0u;
    }
    const bool cols = band == 0;                                        // the per-agent columns are band 0's
    const uint8_t* mk = nullptr;                                        // the window's mask, when the violation column is asked for
    if (cols && viol) {
        const int mi = mask_of_scene[scene];
        if (mi >= 0) mk = mask + (size_t)mi * Oh * Ow;
    }
    const bool want_off = cols && off, want_hit = cols && hit;
    __syncthreads();

    for (int slot = 0; slot < mno; ++slot) {
        const size_t a = (size_t)scene * mno + slot;
        const size_t row0 = (size_t)scene * K * mno + slot;             // row of sample k: row0 + k * mno (the score layout: w is indexed the same)
        const bool there = present ? present[a] != 0 : true;            // (uniform over the workgroup)
        float acc = 0.f;                                                // lane 0: off, lane 64: viol, lane 128: hit
        int cg = OC_NOT_COUNTED;                                        // lane 128: the cell of the scaled target at frame h - 1
        if (want_hit && tid == 128) {
            const float* f = fut + (((size_t)scene * T + (h - 1)) * mno + slot) * 3;
            if (f[0] != 0.f) cg = occ_cell(f[1] * sx, f[2] * sy, Oh, Ow);
        }
        if (there) {
            for (int k0 = 0; k0 < K; k0 += KC) {
                const int kc = min(KC, K - k0);
                for (int f0 = 0; f0 < F; f0 += FC) {
                    const int fc = min(FC, F - f0);
                    // ---- the chunk's weights and flags (once per sample: at its first frames), and the counted mask of its frames
                    if (f0 == 0)
                        for (int kl = tid; kl < kc; kl += EVAL_THREADS) {
                            wl[kl] = w[row0 + (size_t)(k0 + kl) * mno];
                            offl[kl] = 0; violl[kl] = 0;
                        }
                    if (fut)
                        for (int t = tid; t < fc; t += EVAL_THREADS)
                            cml[t] = fut[(((size_t)scene * T + (f_lo + f0 + t)) * mno + slot) * 3] != 0.f ? 1 : 0;
                    __syncthreads();
                    // ---- positions -> cell ids: one segment of fc pairs per sample of the chunk
                    eval_stream<OC_BATCH>(
                        Y, vec, kc, fc, EVAL_ONE_ROW,
                        [&](int sg) { return EvalSeg{(row0 + (size_t)(k0 + sg) * mno) * T + (size_t)(f_lo + f0), sg}; },
                        [&](int kl, int, int t, float y0, float y1) {
                            int id = OC_NOT_COUNTED;
                            if (!fut || cml[t]) {
                                id = occ_cell(y0, y1, Oh, Ow);
                                if (id == OC_OFF_FRAME) offl[kl] = 1;             // (every lane that stores here stores 1)
                                else if (mk && mk[id] == 0) violl[kl] = 1;
                            }
                            idl[kl * fc + t] = id;
                        });
                    __syncthreads();
                    // ---- the columns: one lane each, k in increasing order, once a sample's last frames are in
                    if (f0 + fc == F) {
                        if (tid == 0 && want_off) {
                            for (int kl = 0; kl < kc; ++kl)
                                if (offl[kl]) acc += wl[kl];
                        } else if (tid == 64 && mk) {
                            for (int kl = 0; kl < kc; ++kl)
                                if (violl[kl]) acc += wl[kl];
                        } else if (tid == 128 && cg >= 0) {                       // (mode AT: fc == 1, a sample's id is idl[kl])
                            for (int kl = 0; kl < kc; ++kl)
                                if (idl[kl] == cg) acc += wl[kl];
                        }
                    }
                    // ---- the marginal: sample after sample, the lanes of its frames; a cell takes a sample's weight once
                    for (int kl = 0; kl < kc; ++kl) {
                        const unsigned stamp = (unsigned)slot * (unsigned)K + (unsigned)(k0 + kl) + 1u;
                        const float wk = wl[kl];
                        for (int t = tid; t < fc; t += EVAL_THREADS) {
                            const int id = idl[kl * fc + t];
                            if (id < 0) continue;
                            const int lc = id - cell_lo;
                            if (lc < 0 || lc >= cells) continue;                   // another band's cell
                            if (!until || atomicExch(&Sl[lc], stamp) != stamp) Pl[lc] += wk;
                        }
                        __syncthreads();
                    }
                }
            }
            // ---- fold the agent into the window's maps and clear its marginal (p == 0: adding 0.f and multiplying by 1.f change nothing)
            for (int c = tid; c < cells; c += EVAL_THREADS) {
                const float p = Pl[c];
                if (p != 0.f) {
                    El[c] = El[c] + p;
                    ql[c] = ql[c] * (1.f - p);
                    Pl[c] = 0.f;
                }
            }
        }
        if (cols) {
            const size_t o = a * n_h + hi;
            if (tid == 0 && off) off[o] = acc;
            if (tid == 64 && viol) viol[o] = acc;
            if (tid == 128 && hit) hit[o] = acc;
        }
    }
    __syncthreads();
    const size_t g0 = ((size_t)scene * n_h + hi) * Oh * Ow + cell_lo;
    for (int c = tid; c < cells; c += EVAL_THREADS) {
        occ[g0 + c] = 1.f - ql[c];
        if (expv) expv[g0 + c] = El[c];
    }
}

}  // namespace

void launch_occupancy(const EvalIn& in, const OccParams& p, const RankHz& hz, const EvalScale& sc, const OccOut& o, hipStream_t s) {
    const int until = p.mode == DESIRE_OCC_UNTIL;
    int KC = 1, FC = 1, rows = 1;
    if (!occupancy_geometry(in.K, until ? hz.h[hz.n - 1] : 1, p.Oh, p.Ow, until, &KC, &FC, &rows)) return;      // (refused by the caller before it gets here)
    const int n_bands = eval_chunks(p.Oh, rows);
    const size_t lds = OccLds(rows * p.Ow, KC * FC, until).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0;
    hipLaunchKernelGGL(k_occupancy, dim3((unsigned)((size_t)in.n_scenes * hz.n * n_bands)), dim3(EVAL_THREADS), lds, s, in.Y, in.fut, in.present, p.w,
                       p.mask, p.mask_of_scene, o.occ, o.exp, o.hit, o.viol, o.off, in.mno, in.K, in.T, p.Oh, p.Ow, until, KC, FC, rows, n_bands, vec,
                       sc.sx, sc.sy, hz);
}
