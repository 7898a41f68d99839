// kernels_scene_modes.hip -- n scene modes with per-frame covariances fitted to a window's K weighted joint futures ("worlds": sample k of every
// slot together), and the joint likelihood of the ground truth under that mixture (desire_fit_scene_modes; the contract, operation by operation,
// is in include/desire_hip.h).
//
//   k_fit_scene_modes   one workgroup = one window.  Neither the K worlds (20 x 32 x 40 positions are 205 KB) nor the n x mno x T_pred means fit
//                  LDS, so the window is walked in chunks of SC taking-part slots, once per pass of the weighted Lloyd iteration.  What a mode's
//                  mean is formed from is kept as a set of member worlds (a bit per world) and a mass, not as positions: a chunk
//                    stages    all T_pred frames of the K rows of its slots (eval_tile.h's streamer, a segment per (world, slot));
//                    update    a lane owns a (mode, slot, t) and sums the mode's member worlds in increasing k -- the contract's order, no
//                              reduction, no atomics -- into the chunk's means, next to the rows with the same stride;
//                    distance  a lane owns a (world, mode, slot) and walks t < t_end: d_s;
//                    reduce    one lane per (world, mode) adds the chunk's d_s in increasing slot to the running D [K][n].
//                  After the last chunk a lane per world assigns, one __syncthreads_or compares with the labels before, and n lanes form the
//                  masses and member sets of the next update.  A mode whose mass is 0 keeps its member set, so the mean it keeps is formed
//                  again by the very sequence that formed it (a mode that never had mass: its seed's rows).  The stop is exact.  The last
//                  pass walks the chunks once more: update(final labels), the covariances (the same lanes), means and covariances straight to
//                  the outputs (consecutive t: coalesced), and per (mode, slot, t) the slot's term of the likelihood; a lane per (mode, t)
//                  chains the terms in increasing slot across the chunks.  Then a lane per t: log-sum-exp over the usable modes, per agent.
//
// What crosses a chunk border is the per-(world, mode) sum in increasing slot and the per-(mode, t) chain in increasing slot: a chunked window has
// the bits of an unchunked one by construction (DESIGN.md section 7k's argument).  Slots that do not take part are never staged and never read.
// LDS rows are float2 [t] at a stride of (T_pred | 1) pairs: the lanes of the distance phase, each on its own row at the same t, fall on distinct
// bank pairs and a mean's row is a broadcast; in the update the lanes of a wave walk consecutive t of one row.  No atomics, no host wait:
// capturable, bitwise reproducible, and a window's result depends on that window's taking-part rows, order row, scores and targets only.  The
// LDS plan (SceneModesLds) and the slot chunk are eval_lds.h's.  The arithmetic of the contract is modes_fit.h's, shared with k_fit_modes: the
// seed check, the weights, the row-to-mean distance, the member sums of the update and of the covariance, the Gaussian term and its chain step
// and the horizon emit.  Three things are NOT taken from there, because this kernel sits at the SGPR limit (106, 75 of them spilled to lanes)
// and with any of them it measured 0.7 - 1 % slower than the code below, which compiles to the instructions it had before the header existed
// (DESIGN.md section 7l): the nearest mode of the assign and the mixture's value of a frame are written out (the same statements as
// modes_nearest and modes_frame_value), and SceneModesArgs keeps its own field order, filled from ModesFitOut / ModesFitParams.
#include "eval_tile.h"
#include "modes_fit.h"                         // (sets fp contract(off) from here on: the contract rounds every operation once)

namespace {

constexpr int SM_BATCH = 4;                    // 16-byte loads a lane has in flight while staging
constexpr int SM_ABSENT = 0, SM_USABLE = 1, SM_UNUSABLE = 2;        // state of (slot, mode, t) in the likelihood

struct SceneModesArgs {
    const float* Y; const uint8_t* present; const int32_t* worder; const float* wscore; const float* fut;
    int32_t* label; int32_t* count; float* prob; float* mean; float* cov; int32_t* passes; float* out; float* frame;
    int mno, K, T, n, t_end, iters, SC, vec;
    float sx, sy, ux, uy, var_floor, log_floor;
    RankHz hz;
};

__global__ __launch_bounds__(EVAL_THREADS) void k_fit_scene_modes(const SceneModesArgs A) {
    extern __shared__ float2 sm_sm[];
    __shared__ int hzs[8];
    __shared__ int npS, badS;
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4 && sizeof(float) == 4 && sizeof(unsigned) == 4 &&
                  SceneModesLds::TERM_WORDS == 3 && SceneModesLds::K_WORDS == 3 && SceneModesLds::MODE_WORDS == 5 &&
                  SceneModesLds::FRAME_WORDS == 2 && SceneModesLds::T_WORDS == 3);
    const int K = A.K, T = A.T, n = A.n, SC = A.SC, mno = A.mno;
    const SceneModesLds L(T, SC, K, n, mno);
    const int Tp = L.Tp, DS = L.ds_stride(), KW = SceneModesLds::member_words(K);
    float2* Yl = sm_sm;                                                 // [SC, K, Tp] the chunk's rows
    float2* ml = Yl + L.rows();                                         // [SC, n, Tp] the chunk's means
    int* wd = reinterpret_cast<int*>(sm_sm + L.pairs());                // the words behind the pairs
    float* tq = reinterpret_cast<float*>(wd + L.term(0));               // [SC, n, T] quad_s / det_s
    float* th = reinterpret_cast<float*>(wd + L.term(1));               // [SC, n, T] 0.5f * logf(det_s)
    int* ts = wd + L.term(2);                                           // [SC, n, T] SM_ABSENT / SM_USABLE / SM_UNUSABLE
    float* dsL = reinterpret_cast<float*>(wd + L.ds());                 // [K * n, DS] d_s of the chunk
    float* DL = reinterpret_cast<float*>(wd + L.dist());                // [K, n] the running D
    float* wL = reinterpret_cast<float*>(wd + L.k_words(0));            // [K] score, then weight, of world k
    int* labL = wd + L.k_words(1);                                      // [K] label
    int* prevL = wd + L.k_words(2);                                     // [K] the label of the pass before
    float* WmL = reinterpret_cast<float*>(wd + L.mode_words(0));        // [n] mass of mode i under the labels
    float* WdL = reinterpret_cast<float*>(wd + L.mode_words(1));        // [n] mass of its member set: what its mean is divided by
    int* cntL = wd + L.mode_words(2);                                   // [n] members under the labels
    int* seedL = wd + L.mode_words(3);                                  // [n] the seed world
    int* hasL = wd + L.mode_words(4);                                   // [n] the mode has had mass: its mean is its member set's, not the seed's
    unsigned* memL = reinterpret_cast<unsigned*>(wd + L.member());      // [n, KW] the member set
    float* LrL = reinterpret_cast<float*>(wd + L.frame_words(0));       // [n, T] the running L_i
    int* useL = wd + L.frame_words(1);                                  // [n, T] usable so far
    int* ctL = wd + L.t_words(0);                                       // [T] taking-part slots counted at t
    float* val = reinterpret_cast<float*>(wd + L.t_words(1));           // [T] the frame's value
    float* cm = reinterpret_cast<float*>(wd + L.t_words(2));            // [T] counted
    int* slotL = wd + L.slots();                                        // [mno] the taking-part slots, increasing

    const int tid = threadIdx.x;
    const size_t scene = blockIdx.x;
    const float* ws = A.wscore ? A.wscore + scene * K : nullptr;
    const uint8_t* pr = A.present ? A.present + scene * mno : nullptr;
    const float ux = A.ux, uy = A.uy;
    if (A.fut) eval_stage_horizons(hzs, A.hz);

    // ---- the scores, the taking-part slots; then one lane: the range check of the n seeds and the weights (desire_select_worlds' step 6)
    for (int k = tid; k < K; k += EVAL_THREADS) {
        wL[k] = ws ? ws[k] : 0.f;
        labL[k] = prevL[k] = -1;
    }
    for (int i = tid; i < n; i += EVAL_THREADS) { WmL[i] = 0.f; WdL[i] = 0.f; cntL[i] = 0; hasL[i] = 0; }
    for (int t = tid; t < T; t += EVAL_THREADS) ctL[t] = 0;
    if (tid < 64) {
        const int np = eval_compact(mno, slotL, [&](int i) { return !pr || pr[i] != 0; });
        if (tid == 0) npS = np;
    }
    __syncthreads();
    if (tid == 0) {
        badS = modes_seed_check(A.worder + scene * K, n, K, [&](int i, int c, int bad) { seedL[i] = bad ? 0 : c; });
        modes_weights(ws != nullptr, K, wL);
    }
    __syncthreads();
    const int np = npS;
    const bool bad = badS != 0;                                         // (uniform over the workgroup)

    // one walk over the chunks.  !last: update, then D(k, i) of every world to the updated means.  last: update, covariance, the outputs of both
    // and the likelihood's chain.
    auto walk = [&](const bool last) {
        const int Tm = last ? T : A.t_end;                            // the assignment looks at t < t_end only
        for (int c = tid; c < K * n; c += EVAL_THREADS) DL[c] = 0.f;
        for (int s0 = 0; s0 < np; s0 += SC) {
            const int ns = min(SC, np - s0);
            __syncthreads();                                            // the last chunk's readers are done
            eval_stream<SM_BATCH>(A.Y, A.vec, K * ns, T, T,
                                  [&](int sg) {
                                      const int k = sg / ns, s = sg - k * ns;
                                      return EvalSeg{((scene * K + k) * mno + slotL[s0 + s]) * T, s * K + k};
                                  },
                                  [&](int row, int, int t, float y0, float y1) { Yl[(size_t)row * Tp + t] = make_float2(y0, y1); });
            __syncthreads();
            for (int it = tid; it < ns * n * Tm; it += EVAL_THREADS) {
                const int si = it / Tm, t = it - si * Tm, s = si / n, i = si - s * n;
                const float2* ys = Yl + (size_t)s * K * Tp + t;
                const unsigned* mb = memL + i * KW;
                const auto member = [&](int k) -> bool { return (mb[k >> 5] >> (k & 31)) & 1u; };
                const auto weight = [&](int k) { return wL[k]; };
                float2 m = ys[(size_t)seedL[i] * Tp];                   // a mode that never had mass: its seed's rows
                if (hasL[i]) {
                    const ModesSum sum = modes_member_sum<false>(ys, Tp, K, member, weight);
                    const float W = WdL[i];
                    m = make_float2(sum.x / W, sum.y / W);
                }
                ml[(size_t)si * Tp + t] = m;
                if (!last) continue;
                // covariance about the final means: the members in increasing k (with mass the member set is the labels')
                const float W = WmL[i];
                ModesCov cv{0.f, 0.f, 0.f};
                if (W > 0.f) cv = modes_member_cov(ys, Tp, K, m, ux, uy, W, A.var_floor, member, weight);
                const int slot = slotL[s0 + s];
                const size_t o = ((scene * n + i) * mno + slot) * T + t;
                if (A.mean) { A.mean[2 * o] = m.x; A.mean[2 * o + 1] = m.y; }
                if (A.cov) { A.cov[3 * o] = cv.xx; A.cov[3 * o + 1] = cv.yy; A.cov[3 * o + 2] = cv.xy; }
                if (!A.fut) continue;
                const float* f = A.fut + ((scene * T + t) * mno + slot) * 3;
                int st = SM_ABSENT;
                ModesTerm g{0.f, 0.f};
                if (f[0] != 0.f) {
                    float det;
                    st = SM_UNUSABLE;
                    if (modes_cov_usable(cv.xx, cv.yy, cv.xy, det)) {
                        g = modes_gauss_term(cv.xx, cv.yy, cv.xy, det, m.x, m.y, f[1] * A.sx, f[2] * A.sy, ux, uy);
                        st = SM_USABLE;
                    }
                }
                tq[it] = g.q; th[it] = g.hl; ts[it] = st;
            }
            __syncthreads();
            if (!last) {
                for (int it = tid; it < K * n * ns; it += EVAL_THREADS) {
                    const int r = it / K, k = it - r * K, s = r / n, i = r - s * n;
                    dsL[(k * n + i) * DS + s] = modes_row_dist(Yl + ((size_t)s * K + k) * Tp, ml + ((size_t)s * n + i) * Tp, A.t_end, ux, uy);
                }
                __syncthreads();
                for (int c = tid; c < K * n; c += EVAL_THREADS) {       // increasing slot: the chunks continue one sequence
                    float D = DL[c];
                    for (int s = 0; s < ns; ++s) D = D + dsL[c * DS + s];
                    DL[c] = D;
                }
            } else if (A.fut) {
                for (int it = tid; it < n * T; it += EVAL_THREADS) {    // increasing slot: the chunks continue one chain
                    const int i = it / T, t = it - i * T;
                    float Lv = LrL[it];
                    int use = useL[it], c = 0;
                    for (int s = 0; s < ns; ++s) {
                        const int e = (s * n + i) * T + t, st = ts[e];
                        if (st == SM_USABLE) Lv = modes_chain(Lv, ModesTerm{tq[e], th[e]});
                        if (st == SM_UNUSABLE) use = 0;
                        c += st != SM_ABSENT;
                    }
                    LrL[it] = Lv; useL[it] = use;
                    if (i == 0) ctL[t] += c;
                }
            }
        }
        __syncthreads();
    };
    // assign: a lane per world, the modes in increasing i; true: a label of this lane changed
    auto assign = [&]() {
        bool changed = false;
        for (int k = tid; k < K; k += EVAL_THREADS) {
            int best = -1;
            float bd = 0.f;
            for (int i = 0; i < n; ++i) {
                const float D = DL[k * n + i];
                if (D == D && (best < 0 || D < bd)) { best = i; bd = D; }      // modes_nearest's rule, written out (the file header says why)
            }
            const int old = labL[k];
            prevL[k] = old;
            labL[k] = best;
            changed = changed || best != old;
        }
        return changed;
    };
    // the masses and member counts of the labels, and the member set of every mode with mass (without mass the mode keeps the set it has)
    auto masses = [&]() {
        for (int i = tid; i < n; i += EVAL_THREADS) {
            float W = 0.f;
            int c = 0;
            for (int k = 0; k < K; ++k) {
                const bool in = labL[k] == i;
                W = W + (in ? wL[k] : 0.f); c += in;
            }
            WmL[i] = W; cntL[i] = c;
            if (W > 0.f) {
                WdL[i] = W; hasL[i] = 1;
                for (int q = 0; q < KW; ++q) {
                    unsigned bits = 0u;
                    for (int k = q * 32; k < min(K, q * 32 + 32); ++k) bits |= (labL[k] == i ? 1u : 0u) << (k & 31);
                    memL[i * KW + q] = bits;
                }
            }
        }
    };

    int pass = 0;
    if (!bad) {
        walk(false);                                                    // the distances to the seeds' rows
        assign();
        for (int j = 0;; ++j) {                                         // uniform over the workgroup: every lane reaches every barrier
            __syncthreads();
            masses();
            __syncthreads();
            if (j == A.iters) break;
            walk(false);
            pass = j + 1;
            if (!__syncthreads_or(assign())) break;                     // the labels stood: the masses and member sets are the final labels' already
        }
        if (A.fut)
            for (int it = tid; it < n * T; it += EVAL_THREADS) {
                const float P = WmL[it / T];
                LrL[it] = logf(P); useL[it] = P > 0.f;
            }
        walk(true);
    } else if (A.fut) {                                                 // the frames that count, for the floor
        for (int t = tid; t < T; t += EVAL_THREADS) {
            int c = 0;
            for (int s = 0; s < np; ++s) c += A.fut[((scene * T + t) * mno + slotL[s]) * 3] != 0.f;
            ctL[t] = c;
        }
        __syncthreads();
    }

    // ---- the outputs of the fit (a refused order row: labels -1, zeros); the slots that do not take part get zeros
    for (int i = tid; i < n; i += EVAL_THREADS) { A.count[scene * n + i] = cntL[i]; A.prob[scene * n + i] = WmL[i]; }
    if (A.label)
        for (int k = tid; k < K; k += EVAL_THREADS) A.label[scene * K + k] = labL[k];
    if (A.passes && tid == 0) A.passes[scene] = pass;
    if (A.mean || A.cov)
        for (int it = tid; it < n * mno * T; it += EVAL_THREADS) {
            const int slot = (it / T) % mno;
            if (!bad && (!pr || pr[slot] != 0)) continue;
            const size_t o = scene * n * mno * T + it;
            if (A.mean) { A.mean[2 * o] = 0.f; A.mean[2 * o + 1] = 0.f; }
            if (A.cov) { A.cov[3 * o] = 0.f; A.cov[3 * o + 1] = 0.f; A.cov[3 * o + 2] = 0.f; }
        }
    if (!A.fut) return;                                                 // (uniform)

    // ---- the mixture at the ground truth: a lane per t, the usable modes in increasing i; per agent counted at t (written out: see the header)
    for (int t = tid; t < T; t += EVAL_THREADS) {
        const int c = ctL[t];
        float v = 0.f;
        if (c > 0) {
            v = A.log_floor;
            float M = -INFINITY;
            bool any = false;
            for (int i = 0; i < n; ++i)
                if (!bad && useL[i * T + t]) { M = fmaxf(M, LrL[i * T + t]); any = true; }
            if (any) {
                float S = 0.f;
                for (int i = 0; i < n; ++i)
                    if (useL[i * T + t]) S = S + expf(LrL[i * T + t] - M);
                const float r = (M + logf(S)) / (float)c;
                if (r > A.log_floor) v = r;
            }
        }
        val[t] = v;
        cm[t] = c > 0 ? 1.f : 0.f;
        if (A.frame) A.frame[scene * T + t] = v;
    }
    __syncthreads();
    if (tid == 0) modes_emit_nll(cm, val, hzs, A.hz.n, A.out + scene * A.hz.n * 2);
}

}  // namespace

void launch_fit_scene_modes(const EvalIn& in, const int32_t* worder, const ModesFitOut& o, const ModesFitParams& p, int chunk, hipStream_t s) {
    int SC = 1;
    if (!scene_modes_geometry(in.mno, in.K, in.T, p.n, &SC)) return;    // (refused by the caller before it gets here)
    if (chunk > 0) SC = eval_min(SC, chunk);                            // a smaller chunk than the LDS holds: the same bits (the tests' lever)
    const size_t lds = SceneModesLds(in.T, SC, in.K, p.n, in.mno).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0;
    const SceneModesArgs a{in.Y, in.present, worder, in.score, in.fut, o.label, o.count, o.prob, o.mean, o.cov, o.passes, o.out, o.frame, in.mno, in.K,
                           in.T, p.n, p.t_end, p.iters, SC, vec, p.sx, p.sy, p.ux, p.uy, p.var_floor, p.log_floor, p.hz};
    hipLaunchKernelGGL(k_fit_scene_modes, dim3((unsigned)in.n_scenes), dim3(EVAL_THREADS), lds, s, a);
}
