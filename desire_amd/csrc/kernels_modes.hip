// kernels_modes.hip -- n modes with per-frame covariances fitted to an agent's K weighted samples, and the likelihood of the ground truth under
// that mixture (desire_fit_modes; the contract, operation by operation, is in include/desire_hip.h).
//
//   k_fit_modes    one workgroup = (window, a chunk of SC slots).  All T_pred frames of all K rows of the chunk are streamed into LDS once
//                  (eval_tile.h's streamer: for one (window, k) the chunk's rows are one contiguous run of Y); the n running means of every agent
//                  sit next to them with the same row stride.  One lane per agent range-checks the first n entries of its order row and turns
//                  its scores into weights.  Then the weighted Lloyd iteration runs out of LDS:
//                    assign   a group of G lanes (G = the power of two >= K, 64 at most; beyond, the lanes loop) serves an agent, a lane owns a
//                             sample: its distance over the frames t < t_end to each running mean, in the contract's order.
//                    update   a lane owns one (agent, mode, t) and sums the mode's members in increasing k -- the contract's order, so the
//                             update needs no reduction and no atomics.  Every such lane forms the mode's mass by the same sequence.
//                  The stop is per agent and exact (equal labels reproduce the means bit for bit), but every barrier is reached by the whole
//                  workgroup: it loops while any of its agents still changes, an agent that stopped is skipped by both phases, and its pass
//                  count stays where it stopped.  The last phase is the covariance (again a lane per (agent, mode, t), out of the same LDS),
//                  then a lane per (agent, t) evaluates the mixture at the ground truth and one lane per agent walks its horizons.  Every
//                  output leaves the workgroup with coalesced stores.
//
// LDS rows are float2 [t] at a stride of (T_pred | 1) pairs: odd, so the lanes of a group in the assign -- each on its own row, the same t -- fall on
// distinct bank pairs and the running mean's row is one address, a broadcast; in the update and the covariance the lanes of a wave walk
// consecutive t of one row.  A workgroup takes up to 60 KB of LDS (two of them share a CU's 160 KB); the chunk is at most one agent per group, so
// the assign has a lane for every sample.  No atomics, no host wait: capturable, bitwise reproducible, and a result depends on its agent's rows,
// order, scores and targets only.  The LDS plan (ModesLds) and the slot chunk are eval_lds.h's.  The arithmetic of the contract is modes_fit.h's,
// shared with k_fit_scene_modes: the seed check, the weights, the row-to-mean distance, the nearest mode, the member sums of the update and of
// the covariance, the Gaussian term, the mixture's value of a frame and the horizon emit.
#include "eval_tile.h"
#include "modes_fit.h"                         // (sets fp contract(off) from here on: the contract rounds every operation once)

namespace {

constexpr int FM_BATCH = 4;                    // 16-byte loads a lane has in flight while staging

struct ModesArgs {
    const float* Y; const int32_t* order; const float* score; const float* fut;
    ModesFitOut o;
    ModesFitParams p;
    int mno, K, T, SC, n_sc, G, vec;
};

__global__ __launch_bounds__(EVAL_THREADS) void k_fit_modes(const ModesArgs A) {
    extern __shared__ float2 fm_sm[];
    __shared__ int hzs[8];
    EVAL_LDS_TIED(sizeof(float2) == EVAL_PAIR_BYTES && sizeof(int) == 4 && sizeof(float) == 4 && ModesLds::FRAME_WORDS == 2 &&
                  ModesLds::K_WORDS == 3 && ModesLds::MODE_WORDS == 2 && ModesLds::SLOT_WORDS == 4);
    const int K = A.K, T = A.T, n = A.p.n, SC = A.SC;
    const ModesLds L(T, SC, K, n);
    const int Tp = L.Tp;
    float2* Yl = fm_sm;                                                 // [SC, K, Tp]
    float2* ml = Yl + L.rows();                                         // [SC, n, Tp] the running means
    int* wd = reinterpret_cast<int*>(fm_sm + L.pairs());                // the words behind the pairs
    float* covL = reinterpret_cast<float*>(wd + L.cov());               // [SC, n, T, 3]
    float* val = reinterpret_cast<float*>(wd + L.frame_words(0));       // [SC, Tp] the frame's value
    float* cm = reinterpret_cast<float*>(wd + L.frame_words(1));        // [SC, Tp] counted
    float* wL = reinterpret_cast<float*>(wd + L.k_words(0));            // [SC, K] weight of sample k
    int* labL = wd + L.k_words(1);                                      // [SC, K] label
    int* prevL = wd + L.k_words(2);                                     // [SC, K] the label of the pass before
    float* WmL = reinterpret_cast<float*>(wd + L.mode_words(0));        // [SC, n] mass of mode i
    int* cntL = wd + L.mode_words(1);                                   // [SC, n] members of mode i (the seeds, until the first update)
    int* badL = wd + L.slot_words(0);                                   // [SC] the order row is refused
    int* passL = wd + L.slot_words(1);                                  // [SC] the pass reached
    int* chgL = wd + L.slot_words(2);                                   // [2, SC] parity j & 1: the agent runs iteration j

    const int tid = threadIdx.x;
    const int sc = blockIdx.x % A.n_sc, scene = blockIdx.x / A.n_sc;
    const int slot0 = sc * SC, ns = min(SC, A.mno - slot0);
    const size_t a0 = (size_t)scene * A.mno + slot0;                    // first agent of the chunk
    const float ux = A.p.ux, uy = A.p.uy;
    if (A.fut) eval_stage_horizons(hzs, A.p.hz);

    // ---- stage: segment k = the chunk's rows of (window, k), contiguous in Y; the scores of the chunk (contiguous over the slots of one k)
    eval_stream<FM_BATCH>(A.Y, A.vec, K, ns * T, T,
                          [&](int k) { return EvalSeg{(((size_t)scene * K + k) * A.mno + slot0) * T, k}; },
                          [&](int k, int r, int t, float y0, float y1) { Yl[((size_t)r * K + k) * Tp + t] = make_float2(y0, y1); });
    for (int i = tid; i < ns * K; i += EVAL_THREADS) {
        const int k = i / ns, sl = i - k * ns;
        wL[sl * K + k] = A.score ? A.score[((size_t)scene * K + k) * A.mno + slot0 + sl] : 0.f;
    }
    __syncthreads();
    // ---- one lane per agent: the range check of its n seeds, and the weights (desire_kde_nll's step 1, eval_weight_stats) in place of the scores
    for (int sl = tid; sl < ns; sl += EVAL_THREADS) {
        const int bad = modes_seed_check(A.order + (a0 + sl) * K, n, K, [&](int i, int c, int) { cntL[sl * n + i] = c; });
        badL[sl] = bad;
        passL[sl] = 0;
        chgL[sl] = !bad;
        chgL[SC + sl] = 0;
        if (bad)
            for (int i = 0; i < n; ++i) { cntL[sl * n + i] = 0; WmL[sl * n + i] = 0.f; }
        modes_weights(A.score != nullptr, K, wL + sl * K);
    }
    __syncthreads();
    // ---- the seed means: the rows of the first n entries of the order (zeros, and labels -1, for a refused agent)
    for (int it = tid; it < ns * n * T; it += EVAL_THREADS) {
        const int si = it / T, t = it - si * T, s = si / n;
        ml[(size_t)si * Tp + t] = badL[s] ? make_float2(0.f, 0.f) : Yl[((size_t)s * K + cntL[si]) * Tp + t];
    }
    for (int i = tid; i < ns * K; i += EVAL_THREADS) labL[i] = prevL[i] = -1;
    __syncthreads();

    // ---- the two phases.  Group g of G lanes serves agent g of the chunk (SC <= EVAL_THREADS / G), a lane the samples lg, lg + G, ...
    const int g = tid / A.G, lg = tid - g * A.G;
    // assign for the agents that run iteration j; true: a label of this lane changed
    auto assign = [&](int j, int pass) {
        bool changed = false;
        if (g < ns && chgL[(j & 1) * SC + g]) {
            const float2* ma = ml + (size_t)g * n * Tp;
            for (int k = lg; k < K; k += A.G) {
                const float2* y = Yl + ((size_t)g * K + k) * Tp;
                const int best = modes_nearest(n, [&](int i) { return modes_row_dist(y, ma + (size_t)i * Tp, A.p.t_end, ux, uy); });
                const int old = labL[g * K + k];
                prevL[g * K + k] = old;
                labL[g * K + k] = best;
                changed = changed || best != old;
            }
            if (pass > 0) {
                if (lg == 0) passL[g] = pass;
                if (changed) chgL[((j + 1) & 1) * SC + g] = 1;
            }
        }
        return changed;
    };
    // update for the agents that run iteration j: mass, member count and, where the mass is positive, the weighted mean of every frame
    auto update = [&](int j) {
        for (int it = tid; it < ns * n * T; it += EVAL_THREADS) {
            const int si = it / T, t = it - si * T, s = si / n, i = si - s * n;
            if (!chgL[(j & 1) * SC + s]) continue;
            const ModesSum m = modes_member_sum<true>(Yl + (size_t)s * K * Tp + t, Tp, K, [&](int k) { return labL[s * K + k] == i; },
                                                      [&](int k) { return wL[s * K + k]; });
            if (m.W > 0.f) ml[(size_t)si * Tp + t] = make_float2(m.x / m.W, m.y / m.W);      // without mass the mode keeps its mean
            if (t == 0) { WmL[si] = m.W; cntL[si] = m.c; }
        }
    };

    assign(0, 0);
    __syncthreads();
    for (int j = 0;; ++j) {                                             // uniform over the workgroup: every lane reaches every barrier
        update(j);
        if (tid < ns) chgL[((j + 1) & 1) * SC + tid] = 0;               // (last read before the barrier that ended iteration j - 1)
        __syncthreads();
        if (j == A.p.iters) break;
        if (!__syncthreads_or(assign(j, j + 1))) break;                 // every agent's labels stood: their means are update(final labels) already
    }

    // ---- covariance about the final means: a lane per (agent, mode, t), the members in increasing k
    for (int it = tid; it < ns * n * T; it += EVAL_THREADS) {
        const int si = it / T, t = it - si * T, s = si / n, i = si - s * n;
        const float W = WmL[si];
        ModesCov cv{0.f, 0.f, 0.f};
        if (W > 0.f)
            cv = modes_member_cov(Yl + (size_t)s * K * Tp + t, Tp, K, ml[(size_t)si * Tp + t], ux, uy, W, A.p.var_floor,
                                  [&](int k) { return labL[s * K + k] == i; }, [&](int k) { return wL[s * K + k]; });
        float* c = covL + (size_t)it * 3;
        c[0] = cv.xx; c[1] = cv.yy; c[2] = cv.xy;
    }
    __syncthreads();

    // ---- the outputs of the fit, coalesced
    for (int i = tid; i < ns * n; i += EVAL_THREADS) { A.o.count[a0 * n + i] = cntL[i]; A.o.prob[a0 * n + i] = WmL[i]; }
    if (A.o.label)
        for (int i = tid; i < ns * K; i += EVAL_THREADS) A.o.label[a0 * K + i] = labL[i];
    if (A.o.passes && tid < ns) A.o.passes[a0 + tid] = passL[tid];
    if (A.o.cov)
        for (int i = tid; i < ns * n * T * 3; i += EVAL_THREADS) A.o.cov[a0 * n * T * 3 + i] = covL[i];
    if (A.o.mean) {
        const float* mf = reinterpret_cast<const float*>(ml);
        const int T2 = 2 * T;
        for (int i = tid; i < ns * n * T2; i += EVAL_THREADS) {
            const int si = i / T2;
            A.o.mean[a0 * n * T2 + i] = mf[(size_t)si * Tp * 2 + (i - si * T2)];
        }
    }
    if (!A.fut) return;                                                 // (uniform)

    // ---- the mixture at the ground truth: a lane per (agent, t), the usable modes in increasing i
    for (int it = tid; it < ns * T; it += EVAL_THREADS) {
        const int s = it / T, t = it - s * T;
        const float* f = A.fut + (((size_t)scene * T + t) * A.mno + slot0 + s) * 3;
        const bool counted = f[0] != 0.f;
        float v = 0.f;
        if (counted) {
            const float gx = f[1] * A.p.sx, gy = f[2] * A.p.sy;
            v = modes_frame_value(n, A.p.log_floor, [&](int i, float& l) {
                const int si = s * n + i;
                const float P = WmL[si];
                const float* c = covL + ((size_t)si * T + t) * 3;
                const float cxx = c[0], cyy = c[1], cxy = c[2];
                float det;
                const bool usable = modes_cov_usable(cxx, cyy, cxy, det);
                if (!(P > 0.f) || !usable) return false;
                const float2 m = ml[(size_t)si * Tp + t];
                l = modes_chain(logf(P), modes_gauss_term(cxx, cyy, cxy, det, m.x, m.y, gx, gy, ux, uy));
                return true;
            });
        }
        val[s * Tp + t] = v;
        cm[s * Tp + t] = counted ? 1.f : 0.f;
        if (A.o.frame) A.o.frame[(a0 + s) * T + t] = v;
    }
    __syncthreads();
    const int n_h = A.p.hz.n;
    for (int s = tid; s < ns; s += EVAL_THREADS) modes_emit_nll(cm + s * Tp, val + s * Tp, hzs, n_h, A.o.out + (a0 + s) * n_h * 2);
}

}  // namespace

void launch_fit_modes(const EvalIn& in, const int32_t* order, const ModesFitOut& o, const ModesFitParams& p, hipStream_t s) {
    int SC = 1, G = 1;
    if (!modes_geometry(in.mno, in.K, in.T, p.n, &SC, &G)) return;     // (refused by the caller before it gets here)
    const int n_sc = eval_chunks(in.mno, SC);
    const size_t lds = ModesLds(in.T, SC, in.K, p.n).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0;
    const ModesArgs a{in.Y, order, in.score, in.fut, o, p, in.mno, in.K, in.T, SC, n_sc, G, vec};
    hipLaunchKernelGGL(k_fit_modes, dim3((unsigned)((size_t)in.n_scenes * n_sc)), dim3(EVAL_THREADS), lds, s, a);
}
