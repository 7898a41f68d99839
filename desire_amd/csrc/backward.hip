// backward.hip -- desire_backward: the host-side orchestration of the training step's backward pass, one function per stage.
// The reference computes tf.gradients(cost) but never runs them (model/model.py:388-403, train.py:181); here they run.  Every stage
// writes its weight gradients into the flat buffer "Gflat" (train.hip: natural TF layouts, one tensor to all-reduce).
#include "ctx.h"

namespace {

float* G(desire_ctx* h, const std::string& name) { return W(h, "Gflat") + h->slots.at(name).off; }

// weight gradient block: out[Kd, N] = A^T G over M rows, written into a [.., ldo] matrix
void tn(desire_ctx* h, const float* A, int lda, const float* Gm, int ldg, long M, int Kd, int N, float* out, int ldo,
        int accumulate, hipStream_t s, const unsigned long long* flags = nullptr, int fcols = 0,
        const int* rowlist = nullptr, const int* binbase = nullptr, const int* bintotal = nullptr) {
    TnArgs a{};
    a.A = A; a.lda = lda; a.G = Gm; a.ldg = ldg; a.M = M; a.Kd = Kd; a.N = N; a.flags = flags; a.fcols = fcols;
    a.rowlist = rowlist; a.binbase = binbase; a.bintotal = bintotal;
    // row lists serve the 128 x 128 tile form only (one tile row = one flag block of 128 columns); anything else keeps the flag words
    if (rowlist && !(fcols == 128 && N > 64 && gemm_tn_big_tiles(a) > 0)) a.rowlist = nullptr;
    if (a.rowlist) a.flags = nullptr;
    a.np = gen_plan(h).wgrad_pieces;
    // slices.  Split operands: the large forms keep two workgroups per CU and a workgroup's time per chunk does not depend on its MFMA count
    // (it waits for its operands), so ONE full round of 512 workgroups is best -- 680 took 2.56 ms where 512 take 1.87.  fp32 operands: the
    // kernel is bound by the matrix pipe, tiles that hang over Kd / N finish early, and more workgroups than slots balance that (4.16 vs 5.22 ms)
    const long big_tiles = a.np == 2 ? gemm_tn_big_tiles(a) : 0;
    const long blocks = ((Kd + 63) / 64) * ((N + 63) / 64);
    long sl = big_tiles ? 512 / big_tiles : 2048 / blocks;
    if (sl < 1) sl = 1; if (sl > (big_tiles ? 512 : 256)) sl = big_tiles ? 512 : 256;
    const long maxsl = (M + 63) / 64; if (sl > maxsl) sl = maxsl;
    while ((size_t)sl * Kd * N * sizeof(float) > h->ws.bytes("tn_partial") && sl > 1) sl /= 2;
    a.nslices = (int)sl; a.partial = W(h, "tn_partial");
    launch_gemm_tn(a, out, ldo, accumulate, s);
}
void colsum(desire_ctx* h, const float* Gm, int ldg, long M, int N, float* out, int accumulate, hipStream_t s) {
    long sl = 256; const long maxsl = (M + 3) / 4; if (sl > maxsl) sl = maxsl; if (sl < 1) sl = 1;
    launch_colsum(Gm, ldg, M, N, (int)sl, W(h, "tn_partial"), out, accumulate, s);
}

// ------------------------------------------------------------------------------------------------------------------
// The reference's loss for its 5-wide output layer (model/model.py:315-366: output_w / output_b on the state, get_coef :552-565,
// -log(max(N(next position), 1e-20)) :494-550, the id == 0 masking :351-366, the mean :374-376), teacher-forced over the observed
// frames of the X encoder.  One wave per (agent, observed frame t): o = h_t W5 + b5; target = the position in frame t + 1 (the next
// observed frame, or the first future frame for t = T_obs - 1); the pair counts when the object exists in both frames.  Log form
// (z / (2 (1 - rho^2)) + log(2 pi sx sy sqrt(1 - rho^2)), clamped at -log 1e-20 with no gradient beyond, like the reference's max):
// the pdf itself underflows fp32 long before its logarithm matters.  Writes nll[a,t] (0 when not counted), cnt[a,t] and the raw
// gradient dO[a,t,5] = d nll / d o (Graves 2013, eq. 25-28); k_head_sum / k_head_scale turn them into the mean and its gradient.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head_nll(const float* __restrict__ sv_h, const float* __restrict__ sv_x, const float* __restrict__ past,
                                                  const float* __restrict__ fut, const float* __restrict__ W5, const float* __restrict__ b5,
                                                  int A, int T, int T_pred, int H, int mno, float sx_, float sy_, float* __restrict__ nll,
                                                  float* __restrict__ cnt, float* __restrict__ dO) {
    const int wv = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wv >= A * T) return;
    const int a = wv / T, t = wv - a * T, scene = a / mno, slot = a - scene * mno;
    float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const float* hrow = sv_h + (size_t)wv * H;
    for (int c = lane; c < H; c += 64) {
        const float hv = hrow[c];
#pragma unroll
        for (int j = 0; j < 5; ++j) o[j] = fmaf(hv, W5[c * 5 + j], o[j]);
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) o[j] += __shfl_xor(o[j], m);
        o[j] += b5[j];
    }
    if (lane) return;
    const float* now = past + (((size_t)scene * T + t) * mno + slot) * 3;
    const float* nxt = (t + 1 < T) ? now + (size_t)mno * 3 : fut + ((size_t)scene * T_pred * mno + slot) * 3;
    float x, y;
    if (t + 1 < T) { x = sv_x[((size_t)a * T + t + 1) * 2]; y = sv_x[((size_t)a * T + t + 1) * 2 + 1]; }
    else { x = __fmul_rn(nxt[1], sx_); y = __fmul_rn(nxt[2], sy_); }
    const bool counted = now[0] != 0.f && nxt[0] != 0.f;
    float L = 0.f, g[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (counted) {
        const float sx = __expf(o[2]), sy = __expf(o[3]), rho = tanhf(o[4]);
        const float nx = (x - o[0]) / sx, ny = (y - o[1]) / sy;
        const float neg = fmaxf(1.0f - rho * rho, 1e-12f);
        const float z = nx * nx + ny * ny - 2.0f * rho * nx * ny;
        L = z / (2.0f * neg) + 1.8378770664093453f + o[2] + o[3] + 0.5f * __logf(neg);      // log(2 pi) + log sx + log sy + log sqrt(1 - rho^2)
        if (L < 46.051701859880914f) {                   // -log(1e-20): beyond it the reference's max() pins the value and kills the gradient
            g[0] = -(nx - rho * ny) / (neg * sx);
            g[1] = -(ny - rho * nx) / (neg * sy);
            g[2] = 1.0f - nx * (nx - rho * ny) / neg;
            g[3] = 1.0f - ny * (ny - rho * nx) / neg;
            g[4] = -nx * ny + rho * z / neg - rho;
        } else L = 46.051701859880914f;
    }
    nll[wv] = L; cnt[wv] = counted ? 1.f : 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) dO[(size_t)wv * 5 + j] = g[j];
}
// loss_out[5] = weight * mean nll over the counted pairs, loss_out[7] = their number (one block, fixed order: deterministic)
__global__ void k_head_sum(const float* __restrict__ nll, const float* __restrict__ cnt, int n, float weight, float* __restrict__ loss_out) {
    __shared__ float rs[256], rc[256];
    float s = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { s += nll[i]; c += cnt[i]; }
    rs[threadIdx.x] = s; rc[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        float ts = 0.f, tc = 0.f;
        for (int i = 0; i < 256; ++i) { ts += rs[i]; tc += rc[i]; }
        loss_out[5] = weight * ts / fmaxf(tc, 1.f);
        loss_out[7] = tc;
    }
}
__global__ void k_head_scale(float* __restrict__ dO, int n5, float weight, const float* __restrict__ loss_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n5) dO[i] *= weight / fmaxf(loss_out[7], 1.f);
}

// What the stages of one desire_backward call share.  Two domains besides the caller's own (R rows, A agents, dims.mno slots per scene):
//  _s  DESIRE_FLAG_COMPACT_ROWS: the training-mode forward ran the per-row sample-generation stages on the K*P rows of the P present agents (compact
//      row order r' = k*P + a', one pseudo-scene of P slots: kernels_compact.hip) and left their saves in that order; their whole backward runs on
//      the same rows.  A gradient enters this domain once (dY0) and leaves it twice (dparams, dHx).
//  _e  the encoder stack may have run on the present agents as well (desire_encode): saves in compact agent order, backward on the same agents.
// The IOC module keeps the caller's layout, or its own slot classes (IocView).
struct BwdPass {
    desire_ctx* h; hipStream_t s;
    const float* past; const float* fut; const float* eps;     // the caller's inputs (device)
    const uint8_t* valid;             // loss mask [A]: present at the last observed frame and in at least one target frame
    bool rows_compact; int n_present; // the per-row stages ran compacted, on P present agents (0 otherwise)
    const int32_t* amap;              // compact agent -> agent (nullptr when not compacted)
    long rows_s; int mno_s;           // rows the per-row stages saw, in scenes of mno_s slots
    const float* Hx_s; float* dHx_s;  // their Hx (ld 2H) and d loss / d Hx rows [rows_s, H]
    bool enc_compact;                 // the encoder stack ran on the present agents
    int agents_e, mno_e;              // agents it ran on, in scenes of mno_e slots
    const float* Hx_e; float* dH_e;   // its (Hx | Hy) and d loss / d (Hx | Hy), both [agents_e, 2H]
};
BwdPass make_pass(desire_ctx* h, const float* dev_past, const float* dev_fut, const float* dev_eps, hipStream_t s) {
    BwdPass bp{};
    bp.h = h; bp.s = s; bp.past = dev_past; bp.fut = dev_fut; bp.eps = dev_eps;
    bp.valid = Wt<const uint8_t>(h, "lmask");
    const bool c = bp.rows_compact = h->cp_last, ce = bp.enc_compact = c && h->cp_enc;
    bp.n_present = c ? h->cp_P : 0;
    bp.amap = c ? Wt<const int32_t>(h, "cp_amap") : nullptr;
    bp.rows_s = c ? (long)bp.n_present * h->d.K : (long)h->R; bp.mno_s = c ? bp.n_present : h->d.mno;
    bp.Hx_s = c ? W(h, "cp_HxHy") : W(h, "HxHy"); bp.dHx_s = c ? W(h, "cp_dHx_rows") : W(h, "dHx_rows");
    bp.agents_e = ce ? bp.n_present : h->A; bp.mno_e = ce ? bp.n_present : h->d.mno;
    bp.Hx_e = ce ? W(h, "cp_HxHy") : W(h, "HxHy"); bp.dH_e = ce ? W(h, "cp_dHxHy") : W(h, "dHxHy");
    return bp;
}

// Gradient buffers that exist only for a compacted step.  Allocated before the first launch: nothing has been enqueued when an allocation fails,
// and no hipMalloc falls between the launches of a call that may be under stream capture (everything else: desire_set_training).
int backward_alloc(desire_ctx* h) {
    const size_t R = h->R, A = h->A, RS = ioc_save_rows(h), T = h->d.T_pred, H = h->d.H, f = sizeof(float);
    if (h->cp_last) { if (int rc = ws_ensure(h, {{"cp_dY0", R * T * 2 * f}, {"cp_dHx_rows", R * H * f}, {"cp_dHx", A * H * f}})) return rc; }
    if (h->cp_last && h->cp_enc) { if (int rc = ws_ensure(h, {{"cp_dparams", A * 2 * h->d.L * f}, {"cp_dHxHy", A * 2 * H * f}, {"dHxHy_ioc", A * H * f}})) return rc; }
    if (h->ci_last) {
        if (int rc = ws_ensure(h, {{"ci_dYr", RS * T * 2 * f}, {"ci_dscore", RS * f}, {"ci_dscoreT", RS * T * f}, {"ci_dHx_rows", RS * H * f}, {"ci_dHx", A * H * f},
                                   {"dHxHy_ioc", A * H * f}})) return rc;
    }
    return DESIRE_OK;
}

// Weight gradients of one GRU into the slots <slot>/{gates,candidate}/{kernel,bias}, after its BPTT `a` (DecBwdArgs / IocBwdArgs: the streams dag, dac,
// rh, hprev).  kernel = [(E + H), 2H | H]: the input half contracts x [rows_x, E] with dxg / dxc, the hidden half hprev / rh [rows_h, H] with dag / dac.
// (The decoder's input is constant over time, its dxg / dxc already summed over t: rows_x = rows_h / T.  Elsewhere dxg / dxc ARE dag / dac, same rows.)
// Biases: column sums of dag / dac, or -- a.bias_part set -- the per-tile sums the BPTT kernel left there ([n_tiles, ld_part]: gates, then candidate).
template <class BpttArgs>
void gru_wgrad(const BwdPass& bp, const std::string& slot, const BpttArgs& a, const float* x, int E, const float* dxg, const float* dxc, long rows_x,
               long rows_h, int n_tiles, int ld_part, int acc) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s;
    const int H = h->d.H;
    float* gk = G(h, slot + "/gates/kernel");
    tn(h, x, E, dxg, 2 * H, rows_x, E, 2 * H, gk, 2 * H, acc, s);
    tn(h, a.hprev, H, a.dag, 2 * H, rows_h, H, 2 * H, gk + (size_t)E * 2 * H, 2 * H, acc, s);
    if (a.bias_part) launch_reduce_parts(a.bias_part, n_tiles, ld_part, 0, 2 * H, G(h, slot + "/gates/bias"), acc, s);
    else colsum(h, a.dag, 2 * H, rows_h, 2 * H, G(h, slot + "/gates/bias"), acc, s);
    float* ck = G(h, slot + "/candidate/kernel");
    tn(h, x, E, dxc, H, rows_x, E, H, ck, H, acc, s);
    tn(h, a.rh, H, a.dac, H, rows_h, H, H, ck + (size_t)E * H, H, acc, s);
    if (a.bias_part) launch_reduce_parts(a.bias_part, n_tiles, ld_part, 2 * H, H, G(h, slot + "/candidate/bias"), acc, s);
    else colsum(h, a.dac, H, rows_h, H, G(h, slot + "/candidate/bias"), acc, s);
}

// batch statistics -- per object (bn_mode 1, the reference graph's batch of one) or over the whole batch (mode 2): the conv data-gradient kernels
// run with a linear epilogue and norm_bwd takes the gradient through activation + normalisation.
// (under per-object statistics a conv bias cancels against the mean: its gradient is exactly zero, so the column sums of the
//  post-norm gradients -- pure rounding noise -- are NOT fed to Adam; the Gflat slots of vae_*/b stay at the fill value 0)
void norm_bwd(const BwdPass& bp, float* dy, const float* pre, const float* y, int n, int px, int C, const float* gamma, int sig) {
    desire_ctx* h = bp.h;
    if (h->d.bn_mode == 2) launch_batchnorm_act_bwd(dy, pre, y, (size_t)n, px, C, gamma, sig, W(h, "bn_part2"), W(h, "bn_statb"), W(h, "bn_stat2"), bp.s);
    else launch_instnorm_act_bwd(dy, pre, y, n, px, C, gamma, sig, bp.s);
}

// ---- loss mask, counts, d loss / d Y0 ----
int loss_grads(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    launch_fill_f32(W(h, "Gflat"), h->n_params, 0.f, s);
    // loss mask: present at the last observed frame and in at least one target frame; every loss term below is masked per
    // target frame (model/model.py:351-366).  `valid` (presence at the last observed frame) stays what social pooling uses.
    launch_loss_mask(Wt<const uint8_t>(h, "valid"), bp.fut, Wt<uint8_t>(h, "lmask"), W(h, "nfut"), d.n_scenes, d.mno, d.T_pred, s);
    launch_count_valid(bp.valid, h->A, W(h, "nvalid"), s);
    if (h->recon_mode == DESIRE_RECON_MEAN) {
        launch_loss_grad_y(W(h, "Y0"), bp.fut, bp.valid, W(h, "nfut"), W(h, "nvalid"), W(h, "dY0"), d.n_scenes, d.mno, d.K, d.T_pred, d.sx, d.sy, s);
    } else {          // best-of-many / soft-min (desire_set_recon_loss): the weights of the K samples -- per agent, or in the scene scope the window's for
                      // every one of its slots (desire_set_recon_scope) -- on the full layout, then the weighted gradient
        recon_weights_enqueue(h, RECON_Y0, bp.fut, bp.valid, s);
        launch_loss_grad_y_w(W(h, "Y0"), bp.fut, bp.valid, W(h, "nfut"), W(h, "nvalid"), W(h, "recon_w"), W(h, "dY0"), d.n_scenes, d.mno, d.K, d.T_pred,
                             d.sx, d.sy, s);
    }
    if (h->col_w > 0.f) collision_enqueue(h, col_target_y0(h), bp.fut, bp.valid, s);      // desire_set_collision_loss: dY0 += weight * d L_col / d Y0, on the full layout too
    if (h->off_w > 0.f) offroad_enqueue(h, off_target_y0(h), bp.fut, bp.valid, s);        // desire_set_offroad_loss: dY0 += weight * d L_off / d Y0, after the collision term
    if (bp.rows_compact) launch_gather_rows(W(h, "dY0"), W(h, "cp_dY0"), bp.amap, bp.n_present, d.K, d.mno, d.T_pred * 2, s);
    return DESIRE_OK;
}

// ---- sample-generation module: decoder BPTT and its weight gradients (rows_s > 0) ----
int decoder_bwd(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    const int H = d.H, T = d.T_pred;
    const long Rs = bp.rows_s;
    const float* dY0s = bp.rows_compact ? W(h, "cp_dY0") : W(h, "dY0");
    DecBwdArgs b{};
    b.dY0 = dY0s; b.sv_r = W(h, "dec_sv_r"); b.sv_u = W(h, "dec_sv_u"); b.sv_c = W(h, "dec_sv_c"); b.sv_h = W(h, "dec_sv_h");
    b.Hx = bp.Hx_s; b.ldhx = 2 * H; b.w_head = D(h, "head/w");
    b.WcT_h = D4(h, "dec/WcT_h"); b.WgT_h = D4(h, "dec/WgT_h"); b.WgT_x = D4(h, "dec/WgT_x"); b.WcT_x = D4(h, "dec/WcT_x");
    b.R = (int)Rs; b.K = d.K; b.mno = bp.mno_s; b.T = T; b.H = H;
    b.dag = W(h, "dec_dag"); b.dac = W(h, "dec_dac"); b.rh = W(h, "dec_rh"); b.hprev = W(h, "dec_hprev");
    b.dxg = W(h, "dec_dxg"); b.dxc = W(h, "dec_dxc"); b.dxz = W(h, "dxz"); b.dHx_rows = bp.dHx_s;
    // bias gradients = column sums of the gate-gradient streams: summed per tile inside the BPTT kernels (no further pass over the streams)
    b.bias_part = W(h, "bias_part");
    { Timer t(h, s, "bwd_decoder"); launch_decoder_bwd(b, s); }
    Timer t(h, s, "bwd_decoder_wgrad");
    tn(h, W(h, "dec_sv_h"), H, dY0s, 2, Rs * T, H, 2, G(h, "head/w"), 2, 0, s);
    colsum(h, dY0s, 2, Rs * T, 2, G(h, "head/b"), 0, s);
    gru_wgrad(bp, "dec", b, W(h, "xz"), H, b.dxg, b.dxc, Rs, Rs * T, (int)((Rs + 31) / 32), 3 * H, 0);
    return DESIRE_OK;
}

// the loss gradients of one view's rows and its d loss / d Hx rows: the caller's buffers, or the class's own (ci_*)
struct IocRowGrads { float* dYr; float* dscore; float* dscoreT; float* dHx; };

// One (view, pass) of the IOC module: BPTT in the form ioc_plan picks for the view, scene-grid gradient, weight gradients.  acc: the weight
// gradients accumulate (every launch sequence but the first); scene_first: nothing has written d loss / d grids yet.
int ioc_pass_bwd(const BwdPass& bp, const IocView& v, bool first_view, int pass, const IocRowGrads& g, int acc, bool& scene_first) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    const int H = d.H, T = d.T_pred, E = h->E, B = h->B;
    const long RT = v.R * T;
    const bool last_pass = pass == d.iters - 1;
    const int acc_s = first_view ? 0 : 1;         // (score weights: the last pass of every view)
    const size_t po = ioc_save_off(h, pass, v);
    const float* sv_h = W(h, "ioc_sv_h") + po * H;
    const float* sv_x = W(h, "ioc_sv_x") + po * E;
    IocBwdArgs q{};
    q.Y0 = W(h, "ioc_Yin") + po * 2; q.p_last = v.p_last; q.valid = v.valid; q.Hx = v.Hx; q.ldhx = 2 * H;
    q.dYr = g.dYr; q.dscore = last_pass ? g.dscore : W(h, "dscore0");
    q.sv_x = sv_x; q.sv_r = W(h, "ioc_sv_r") + po * H; q.sv_u = W(h, "ioc_sv_u") + po * H; q.sv_c = W(h, "ioc_sv_c") + po * H; q.sv_h = sv_h;
    q.w_score = D(h, "ioc/score_w");
    q.R = (int)v.R; q.K = d.K; q.mno = v.mno; q.T = T; q.H = H; q.G = d.grid_size; q.nb_w = d.nb_w; q.nb_h = d.nb_h;
    q.gpt = v.gpt; q.ngrp = v.ngrp;
    q.WrT = D4(h, "ioc/WrT"); q.WcT_h = D4(h, "ioc/WcT_h"); q.WcT_er = D4(h, "ioc/WcT_er"); q.WcT_ev = D4(h, "ioc/WcT_ev");
    q.WgT_h = D4(h, "ioc/WgT_h"); q.WgT_er = D4(h, "ioc/WgT_er"); q.WgT_ev = D4(h, "ioc/WgT_ev"); q.WsT = D4(h, "ioc/WsT"); q.WsT_c = D4(h, "ioc/WsT_c");
    q.dag = W(h, "ioc_dag"); q.dac = W(h, "ioc_dac"); q.rh = W(h, "ioc_rh"); q.hprev = W(h, "ioc_hprev");
    q.dpre_r = W(h, "ioc_dpre_r"); q.dpre_v = W(h, "ioc_dpre_v"); q.vel = W(h, "ioc_vel"); q.pooled = W(h, "ioc_pooled");
    q.pool_flags = Wt<unsigned long long>(h, "ioc_pool_flags");
    q.dHx_rows = g.dHx;
    q.bin_tab = d.bin_mode == 1 ? W(h, "bin_tab") : nullptr;
    const IocBwd bwd = ioc_plan(d, true, v.mno, v.gpt, v.R).bwd; const bool cl_bwd = bwd == IocBwd::CLUSTER;
    q.bias_part = cl_bwd ? nullptr : W(h, "bias_part");           // (the cluster form keeps the separate column-sum passes)
    if (cl_bwd) {
        if (int rc = ioc_cluster_exchange(h, (size_t)v.R / v.mno, first_view && last_pass, s)) return rc;
        if (launch_ioc_bwd_cluster(q, Wt<int>(h, "grp_cnt"), Wt<int>(h, "ioc_err"), s))
            return fail(DESIRE_ERR_STATE, "cluster-form IOC backward does not serve this shape");
    } else if (bwd == IocBwd::X3) {      // split-bf16 operands in the data-gradient contractions
        q.WcT_h = D4(h, "ioc/WcT16"); q.WgT_h = D4(h, "ioc/WgT16"); q.WsT = D4(h, "ioc/WsT16");
#ifdef DESIRE_IOC_TIMING
        if (int rc = ws_ensure(h, {{"dbgb", 12 * sizeof(long long)}})) return rc;
        q.dbg = Wt<long long>(h, "dbgb");
#endif
        launch_ioc_bwd_x3(q, s);
#ifdef DESIRE_IOC_TIMING
        const char* nm[12] = {"loop tail (dh)", "bar top", "P0 pos/clear/load h", "bar P0", "P1 masks + part 1 (loads, stores, images)", "barriers after parts",
                              "t2 mma + dar", "gates mma + dpr", "pooled rebuild + store", "dpool mma + tile write", "bin barrier", "gather / NB"};
        ioc_timing_report(q.dbg, nm, 12, s);       // (k_ioc_bwd_x3, block 7, wave 0)
#endif
    } else
        launch_ioc_bwd(q, s);
    if (scene_grad_on(h)) {                // d loss / d grids from this pass's gate gradients (dag / dac are overwritten by the next pass)
        Timer ts(h, s, "bwd_scene_grad");
        SceneDsArgs sa{};
        sa.dag = q.dag; sa.dac = q.dac; sa.Y = q.Y0; sa.gos = v.gos; sa.wcat = W(h, "sg_wcat");
        sa.R = (int)v.R; sa.T = T; sa.H = H; sa.K = d.K; sa.mno = v.mno; sa.gpt = v.gpt; sa.ngrp = v.ngrp; sa.Gh = d.Gh; sa.Gw = d.Gw;
        sa.n_keys = d.n_grids * d.Gh * d.Gw; sa.key_bits = scene_key_bits(sa.n_keys);
        sa.ds = W(h, "sg_ds"); sa.keys = Wt<uint32_t>(h, "sg_keys"); sa.idx = Wt<int32_t>(h, "sg_idx");
        SceneSortBufs sb{Wt<void>(h, "sg_tmp"), h->ws.bytes("sg_tmp"), Wt<uint32_t>(h, "sg_keys_sorted"), Wt<int32_t>(h, "sg_idx_sorted"),
                         Wt<int32_t>(h, "sg_beg"), Wt<int32_t>(h, "sg_end"), W(h, "sg_part")};
        if (launch_scene_grid_grad(sa, sb, W(h, "scene_grid_grad"), scene_first ? 0 : 1, s))
            return fail(DESIRE_ERR_HIP, "scene-grid gradient: launch failed");
        scene_first = false;
    }
    tn(h, sv_h + (size_t)(T - 1) * H, T * H, g.dYr, 2 * T, v.R, H, 2 * T, G(h, "ioc/reg/w"), 2 * T, acc, s);
    colsum(h, g.dYr, 2 * T, v.R, 2 * T, G(h, "ioc/reg/b"), acc, s);
    if (last_pass) {
        tn(h, sv_h, H, g.dscoreT, 1, RT, H, 1, G(h, "ioc/score/w"), 1, acc_s, s);
        colsum(h, g.dscoreT, 1, RT, 1, G(h, "ioc/score/b"), acc_s, s);
    }
    const int n_tiles32 = (int)((v.R + 31) / 32);
    gru_wgrad(bp, "ioc", q, sv_x, E, q.dag, q.dac, RT, RT, n_tiles32, 4 * H, acc);
    const unsigned long long* pflags = q.pool_flags;
    if (H == 128 && (size_t)RT * (size_t)B < ((size_t)1 << 31)) {      // (list positions are ints)
        // one output tile row = one bin (128 columns): each contracts only the (row, t) pairs that hold a neighbour in ITS bin, from
        // per-bin row lists built out of the flags -- 23 % of the rows at the bench's density, where skipping whole 32-row chunks
        // by their OR-ed flags still visited about half of them, zero rows and all
        int* bl_counts = Wt<int>(h, "bin_counts"); int* bl_base = Wt<int>(h, "bin_base");
        int* bl_total = Wt<int>(h, "bin_total"); int* bl_list = Wt<int>(h, "bin_list");
        launch_bin_lists(pflags, RT, B, bl_counts, bl_base, bl_total, bl_list, s);
        tn(h, q.pooled, B * H, q.dpre_r, H, RT, B * H, H, G(h, "ioc/social_fc/w"), H, acc, s, pflags, H, bl_list, bl_base, bl_total);
    } else
        tn(h, q.pooled, B * H, q.dpre_r, H, RT, B * H, H, G(h, "ioc/social_fc/w"), H, acc, s, pflags, H);   // empty (row, t, bin) blocks are skipped
    if (cl_bwd) colsum(h, q.dpre_r, H, RT, H, G(h, "ioc/social_fc/b"), acc, s);
    else launch_reduce_parts(q.bias_part, n_tiles32, 4 * H, 3 * H, H, G(h, "ioc/social_fc/b"), acc, s);
    tn(h, q.vel, 2, q.dpre_v, d.E_v, RT, 2, d.E_v, G(h, "ioc/vel_fc/w"), d.E_v, acc, s);
    colsum(h, q.dpre_v, d.E_v, RT, d.E_v, G(h, "ioc/vel_fc/b"), acc, s);
    return DESIRE_OK;
}

// a slot class's share of d loss / d Hx: rows -> class agents -> agents (padding slots dropped), accumulated into "dHxHy_ioc"
void ioc_class_dHx(const BwdPass& bp, const IocView& v, const float* dHx_rows) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s;
    const int H = h->d.H;
    launch_fill_f32(W(h, "ci_dHx"), (size_t)v.n_scenes * v.mno * H, 0.f, s);
    launch_rows_to_agents(dHx_rows, W(h, "ci_dHx"), H, v.n_scenes, v.mno, h->d.K, H, s, v.gpt);
    launch_cls_scatter_add_agents(W(h, "ci_dHx"), H, W(h, "dHxHy_ioc"), H, v.cmap, v.n_scenes * v.mno, H, s);
}

// ---- ranking / refinement module (trajectories detached: its only path into the rest is dHx) ----
// One BPTT per refinement pass, last pass first: Y_final = Y0 + sum_p dY_p, so every pass's regression head sees the same dL/dY_final; only
// the last pass's scores enter the loss.  Weight gradients of the passes accumulate.
// DESIRE_FLAG_COMPACT_IOC: the forward ran one launch sequence per slot class (api_forward.hip: class_layout) and left each class's saves at its
// row offset; the BPTT and every weight-gradient reduction run per class on the same views, accumulating.  Otherwise: one view, the handle's own shape.
int ioc_bwd(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    const int H = d.H, T = d.T_pred;
    if (bp.rows_compact) launch_fill_f32(W(h, "dHx_rows"), (size_t)h->R * H, 0.f, s);      // the IOC module accumulates into it; the decoder no longer initialises it
    Timer t(h, s, "bwd_ioc");
    // d loss / d Y of the refined trajectories, on the full layout (before the class gather; every pass reads it).  desire_set_refined_loss: the
    // regression term takes the recon mode's weights from the refined errors; then dYr += weight * G of the collision and of the off-road term
    if (h->ref_recon && h->recon_mode != DESIRE_RECON_MEAN) {
        recon_weights_enqueue(h, RECON_REFINED, bp.fut, bp.valid, s);
        launch_loss_grad_y_w(W(h, "Y_ref"), bp.fut, bp.valid, W(h, "nfut"), W(h, "nvalid"), W(h, "rrecon_w"), W(h, "dYr"), d.n_scenes, d.mno, d.K, T,
                             d.sx, d.sy, s);
    } else
        launch_loss_grad_y(W(h, "Y_ref"), bp.fut, bp.valid, W(h, "nfut"), W(h, "nvalid"), W(h, "dYr"), d.n_scenes, d.mno, d.K, T, d.sx, d.sy, s);
    if (h->rcol_w > 0.f) collision_enqueue(h, col_target_refined(h), bp.fut, bp.valid, s);
    if (h->roff_w > 0.f) offroad_enqueue(h, off_target_refined(h), bp.fut, bp.valid, s);
    launch_score_grad(W(h, "Y0"), bp.fut, W(h, "score_sv"), bp.valid, W(h, "nvalid"), W(h, "dscore"), W(h, "dscoreT"), d.n_scenes,
                      d.mno, d.K, T, d.sx, d.sy, s);
    std::vector<IocView> views;
    if (h->ci_last) {
        launch_fill_f32(W(h, "dHxHy_ioc"), (size_t)h->A * H, 0.f, s);
        const ClassLayout cl = class_layout(h, ioc_plan(h).padded, h->ci_cnt);
        for (int c = 0; c < cl.n; ++c)
            if (cl.c[c].n_scenes > 0) views.push_back(ioc_view(h, &cl.c[c]));
    } else
        views.push_back(ioc_view(h));
    launch_fill_f32(W(h, "dscore0"), (size_t)h->R, 0.f, s);
    const bool sg_on = scene_grad_on(h);                    // d loss / d grids wanted (the option, or scene images attached)
    if (sg_on) {
        Timer ts(h, s, "bwd_scene_grad");
        launch_scene_wcat(W(h, "Wflat") + h->slots.at("ioc/gates/kernel").off, W(h, "Wflat") + h->slots.at("ioc/candidate/kernel").off, H, d.E_v,
                          W(h, "sg_wcat"), s);
    }
    bool scene_first = true;                    // the first (view, pass) writes d loss / d grids, the others accumulate
    bool first = true;                          // the first launch sequence writes the weight gradients, the others accumulate
    for (size_t vi = 0; vi < views.size(); ++vi) {
        const IocView& v = views[vi];
        IocRowGrads g{W(h, "dYr"), W(h, "dscore"), W(h, "dscoreT"), W(h, "dHx_rows")};
        if (v.cmap) {          // the class's rows of the loss gradients; its own d loss / d Hx rows
            g = IocRowGrads{W(h, "ci_dYr"), W(h, "ci_dscore"), W(h, "ci_dscoreT"), W(h, "ci_dHx_rows")};
            launch_cls_rows(W(h, "dYr"), g.dYr, v.cmap, v.n_scenes, v.mno, d.K, d.mno, 2 * T, 0, s, v.gpt);
            launch_cls_rows(W(h, "dscore"), g.dscore, v.cmap, v.n_scenes, v.mno, d.K, d.mno, 1, 0, s, v.gpt);
            launch_cls_rows(W(h, "dscoreT"), g.dscoreT, v.cmap, v.n_scenes, v.mno, d.K, d.mno, T, 0, s, v.gpt);
            launch_fill_f32(g.dHx, (size_t)v.R * H, 0.f, s);
        }
        for (int pass = d.iters - 1; pass >= 0; --pass) {
            if (int rc = ioc_pass_bwd(bp, v, vi == 0, pass, g, first ? 0 : 1, scene_first)) return rc;
            first = false;
        }
        if (v.cmap) ioc_class_dHx(bp, v, g.dHx);
    }
    if (sg_on && scene_first) launch_fill_f32(W(h, "scene_grid_grad"), (size_t)d.n_grids * d.Gh * d.Gw * d.C, 0.f, s);     // no IOC row ran
    return DESIRE_OK;
}

// ---- scene CNN (desire_set_scene_images): from d loss / d grids back through conv3 (5x5 s1, linear), ReLU, conv2 (5x5 s2), ReLU, conv1 (5x5 s2)
// into the Gflat slots scene_cnn/*.  Weight gradients: im2col rows [pixels, 25 Ci] contracted with the output gradient on the MFMA reduction tn()
// (fixed slices, fixed order: bitwise reproducible); bias gradients: column sums; data gradients: one gather per input element (no atomics).
int scene_cnn_bwd(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    Timer t(h, s, "bwd_scene_cnn");
    const int n = d.n_grids, G1h = 2 * d.Gh, G1w = 2 * d.Gw, Ih = 4 * d.Gh, Iw = 4 * d.Gw;
    const long P3 = (long)n * d.Gh * d.Gw, P1 = (long)n * G1h * G1w;
    float* col = W(h, "sg_col");
    const float* dG = W(h, "scene_grid_grad");
    launch_im2col5(W(h, "scnn2"), col, n, d.Gh, d.Gw, 32, d.Gh, d.Gw, 1, 2, 800, s);
    tn(h, col, 800, dG, d.C, P3, 800, d.C, G(h, "scene_cnn/conv3/w"), d.C, 0, s);
    colsum(h, dG, d.C, P3, d.C, G(h, "scene_cnn/conv3/b"), 0, s);
    launch_conv5_dgrad_relu(dG, D(h, "scene_cnn/conv3/w"), W(h, "scnn2"), W(h, "sg_d2"), n, d.Gh, d.Gw, 32, d.Gh, d.Gw, d.C, 1, 2, s);
    launch_im2col5(W(h, "scnn1"), col, n, G1h, G1w, 16, d.Gh, d.Gw, 2, 1, 400, s);
    tn(h, col, 400, W(h, "sg_d2"), 32, P3, 400, 32, G(h, "scene_cnn/conv2/w"), 32, 0, s);
    colsum(h, W(h, "sg_d2"), 32, P3, 32, G(h, "scene_cnn/conv2/b"), 0, s);
    launch_conv5_dgrad_relu(W(h, "sg_d2"), D(h, "scene_cnn/conv2/w"), W(h, "scnn1"), W(h, "sg_d1"), n, G1h, G1w, 16, d.Gh, d.Gw, 32, 2, 1, s);
    launch_im2col5(h->img, col, n, Ih, Iw, 3, G1h, G1w, 2, 1, 76, s);               // 75 columns, rows padded to 76 floats
    tn(h, col, 76, W(h, "sg_d1"), 16, P1, 75, 16, G(h, "scene_cnn/conv1/w"), 16, 0, s);
    colsum(h, W(h, "sg_d1"), 16, P1, 16, G(h, "scene_cnn/conv1/b"), 0, s);
    return DESIRE_OK;
}

// ---- mask fc (rows_s > 0) ----
int mask_bwd(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    const int H = d.H, V = h->V;
    const long Rs = bp.rows_s;
    Timer t(h, s, "bwd_mask");
    launch_mask_bwd(W(h, "mask_sv_p"), W(h, "dxz"), bp.Hx_s, 2 * H, W(h, "dq_mask"), bp.dHx_s, (int)Rs, H, h->Hl, d.K, bp.mno_s, h->recon_mode != DESIRE_RECON_MEAN, s);
    colsum(h, W(h, "dq_mask"), H, Rs, H, G(h, "mask_fc/b"), 0, s);
    tn(h, W(h, "xhat"), V, W(h, "dq_mask"), H, Rs, V, H, G(h, "mask_fc/w"), H, 0, s);
    GemmArgs g{};
    g.A = W(h, "dq_mask"); g.lda = H; g.M = (int)Rs; g.K = H; g.Bp = D4(h, "mask/WT"); g.G = H / 8; g.NT = V / 32;
    g.out = W(h, "dconv4"); g.ldo = V; g.N = V; g.p0 = D(h, "vae_dec/deconv4/scale"); g.chmod = 1; g.aux = W(h, "xhat");
    if (d.bn_mode != 0) {          // per-object batch-norm: gradient w.r.t. the layer OUTPUT first, then through activation + instance norm
        launch_gemm_rows(g, EPI_NONE, s);
        norm_bwd(bp, W(h, "dconv4"), W(h, "deconv4_pre"), W(h, "xhat"), (int)Rs, 1024, 1, D(h, "vae_dec/deconv4/gamma"), 1);
    } else
        launch_gemm_rows(g, EPI_SIGGRAD, s);
    return DESIRE_OK;
}

// ---- CVAE decoder (rows_s > 0; each data gradient = the forward kernel of the mirrored layer with a gradient epilogue) ----
int cvae_dec_bwd(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    const int L = d.L;
    const long Rs = bp.rows_s;
    const bool bn1 = d.bn_mode != 0;
    Timer t(h, s, "bwd_cvae_dec");
    const int NSL = 78;
    launch_w1ch_grad(W(h, "dconv4"), W(h, "d3"), (int)Rs, Rs < 2048 ? (int)Rs : 2048, W(h, "tn_partial"), G(h, "vae_dec/deconv4/w"), s);
    if (!bn1) colsum(h, W(h, "dconv4"), 1, Rs * 1024, 1, G(h, "vae_dec/deconv4/b"), 0, s);
    ConvArgs c{};
    c.n = (int)Rs;
    c.in = W(h, "dconv4"); c.out = W(h, "dconv3"); c.w_raw = D(h, "vae_dec/deconv4/raw");
    c.scale = D(h, "vae_dec/deconv3/scale"); c.shift = c.scale; c.mode = bn1 ? 3 : 1; c.yprev = W(h, "d3");
    launch_conv1(c, s);
    if (bn1) norm_bwd(bp, W(h, "dconv3"), W(h, "deconv3_pre"), W(h, "d3"), (int)Rs, 256, 32, D(h, "vae_dec/deconv3/gamma"), 0);
    ConvWgradArgs wg{};
    wg.np = gen_plan(h).wgrad_pieces;
    wg.S = W(h, "d2"); wg.Cs = 64; wg.Ps = 8; wg.Lg = W(h, "dconv3"); wg.Cl = 32; wg.Pl = 16; wg.stride = 2; wg.pad = 1;
    wg.n = (int)Rs; wg.partial = W(h, "tn_partial");
    launch_conv_wgrad(wg, NSL, G(h, "vae_dec/deconv3/w"), s);
    if (!bn1) colsum(h, W(h, "dconv3"), 32, Rs * 256, 32, G(h, "vae_dec/deconv3/b"), 0, s);
    const bool x3 = gen_plan(h).dgrad_split;
    c.in = W(h, "dconv3"); c.out = W(h, "dconv2"); c.Wp = D4(h, x3 ? "vae_dec/deconv3/Wbwd16" : "vae_dec/deconv3/Wbwd");
    c.scale = D(h, "vae_dec/deconv2/scale"); c.shift = c.scale; c.yprev = W(h, "d2");
    if (x3) launch_conv2_x3(c, s); else launch_conv2(c, s);
    if (bn1) norm_bwd(bp, W(h, "dconv2"), W(h, "deconv2_pre"), W(h, "d2"), (int)Rs, 64, 64, D(h, "vae_dec/deconv2/gamma"), 0);
    wg.S = W(h, "d1"); wg.Cs = 128; wg.Ps = 4; wg.Lg = W(h, "dconv2"); wg.Cl = 64; wg.Pl = 8; wg.stride = 1; wg.pad = 0;
    launch_conv_wgrad(wg, NSL, G(h, "vae_dec/deconv2/w"), s);
    if (!bn1) colsum(h, W(h, "dconv2"), 64, Rs * 64, 64, G(h, "vae_dec/deconv2/b"), 0, s);
    c.in = W(h, "dconv2"); c.out = W(h, "dconv1"); c.Wp = D4(h, x3 ? "vae_dec/deconv2/Wbwd16" : "vae_dec/deconv2/Wbwd");
    c.scale = D(h, "vae_dec/deconv1/scale"); c.shift = c.scale; c.yprev = W(h, "d1");
    if (x3) launch_conv3_x3(c, s); else launch_conv3(c, s);
    if (bn1) norm_bwd(bp, W(h, "dconv1"), W(h, "deconv1_pre"), W(h, "d1"), (int)Rs, 16, 128, D(h, "vae_dec/deconv1/gamma"), 0);
    tn(h, W(h, "dconv1"), 2048, W(h, "z"), L, Rs, 2048, L, G(h, "vae_dec/deconv1/w"), L, 0, s);
    if (!bn1) colsum(h, W(h, "dconv1"), 128, Rs * 16, 128, G(h, "vae_dec/deconv1/b"), 0, s);
    GemmArgs g{};
    g.A = W(h, "dconv1"); g.lda = 2048; g.M = (int)Rs; g.K = 2048; g.Bp = D4(h, "vae_dec/deconv1/WT"); g.G = 2048 / 8;
    g.NT = (L + 31) / 32; g.out = W(h, "dz"); g.ldo = L; g.N = L;
    launch_gemm_rows(g, EPI_NONE, s);
    return DESIRE_OK;
}

// ---- latent + CVAE encoder + fc_c: d loss / d params from dz, then (agents_e > 0) back through the encoder stack into dH_e (written, both halves) ----
int cvae_enc_bwd(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    const int H = d.H, V = h->V, L = d.L, Ae = bp.agents_e;
    const bool bn1 = d.bn_mode != 0;
    const int32_t* inv = bp.rows_compact ? Wt<const int32_t>(h, "cp_inv") : nullptr;
    if (bp.eps) launch_reparam_bwd(W(h, "dz"), bp.eps, W(h, "params"), bp.valid, W(h, "nvalid"), W(h, "dparams"), d.n_scenes, d.mno, d.K, L, s, inv, bp.n_present);
    else launch_reparam_bwd_rng(W(h, "dz"), rng_args(h), W(h, "params"), bp.valid, W(h, "nvalid"), W(h, "dparams"), d.n_scenes, d.mno, d.K, L, s, inv,
                                bp.n_present);      // eps regenerated from rng_state.used: the draw of the forward this backward follows
    if (bp.enc_compact) launch_gather_agents(W(h, "dparams"), W(h, "cp_dparams"), bp.amap, bp.n_present, 2 * L, s);
    const float* dparE = bp.enc_compact ? W(h, "cp_dparams") : W(h, "dparams");
    if (Ae <= 0) return DESIRE_OK;
    tn(h, W(h, "c3"), 2048, dparE, 2 * L, Ae, 2048, 2 * L, G(h, "vae_enc/fc/w"), 2 * L, 0, s);
    colsum(h, dparE, 2 * L, Ae, 2 * L, G(h, "vae_enc/fc/b"), 0, s);
    GemmArgs g{};
    g.A = dparE; g.lda = 2 * L; g.M = Ae; g.K = 2 * L; g.Bp = D4(h, "vae_enc/fc/WT"); g.G = 2 * L / 8; g.NT = 64;
    g.out = W(h, "dconvE3"); g.ldo = 2048; g.N = 2048; g.p0 = D(h, "vae_enc/conv3/scale"); g.chmod = 128; g.aux = W(h, "c3");
    if (bn1) {
        launch_gemm_rows(g, EPI_NONE, s);
        norm_bwd(bp, W(h, "dconvE3"), W(h, "conv3_pre"), W(h, "c3"), Ae, 16, 128, D(h, "vae_enc/conv3/gamma"), 0);
    } else
        launch_gemm_rows(g, EPI_ELUGRAD, s);
    const int NSL = Ae >= 2048 ? 64 : (Ae >= 256 ? 16 : 4);
    ConvWgradArgs wg{};
    wg.np = gen_plan(h).wgrad_pieces;
    wg.n = Ae; wg.partial = W(h, "tn_partial");
    wg.S = W(h, "dconvE3"); wg.Cs = 128; wg.Ps = 4; wg.Lg = W(h, "c2"); wg.Cl = 64; wg.Pl = 8; wg.stride = 1; wg.pad = 0;
    launch_conv_wgrad(wg, NSL, G(h, "vae_enc/conv3/w"), s);
    if (!bn1) colsum(h, W(h, "dconvE3"), 128, (long)Ae * 16, 128, G(h, "vae_enc/conv3/b"), 0, s);
    ConvArgs c{};
    c.n = Ae; c.mode = bn1 ? 3 : 1;
    c.in = W(h, "dconvE3"); c.out = W(h, "dconvE2"); c.Wp = D4(h, "vae_enc/conv3/Wbwd");
    c.scale = D(h, "vae_enc/conv2/scale"); c.shift = c.scale; c.yprev = W(h, "c2");
    launch_deconv2(c, s);
    if (bn1) norm_bwd(bp, W(h, "dconvE2"), W(h, "conv2_pre"), W(h, "c2"), Ae, 64, 64, D(h, "vae_enc/conv2/gamma"), 0);
    wg.S = W(h, "dconvE2"); wg.Cs = 64; wg.Ps = 8; wg.Lg = W(h, "c1"); wg.Cl = 32; wg.Pl = 16; wg.stride = 2; wg.pad = 1;
    launch_conv_wgrad(wg, NSL, G(h, "vae_enc/conv2/w"), s);
    if (!bn1) colsum(h, W(h, "dconvE2"), 64, (long)Ae * 64, 64, G(h, "vae_enc/conv2/b"), 0, s);
    c.in = W(h, "dconvE2"); c.out = W(h, "dconvE1"); c.Wp = D4(h, "vae_enc/conv2/Wbwd");
    c.scale = D(h, "vae_enc/conv1/scale"); c.shift = c.scale; c.yprev = W(h, "c1");
    launch_deconv3(c, s);
    if (bn1) norm_bwd(bp, W(h, "dconvE1"), W(h, "conv1_pre"), W(h, "c1"), Ae, 256, 32, D(h, "vae_enc/conv1/gamma"), 0);
    launch_w1ch_grad(W(h, "vae_in"), W(h, "dconvE1"), Ae, Ae < 1024 ? Ae : 1024, W(h, "tn_partial"), G(h, "vae_enc/conv1/w"), s);
    if (!bn1) colsum(h, W(h, "dconvE1"), 32, (long)Ae * 256, 32, G(h, "vae_enc/conv1/b"), 0, s);
    c.in = W(h, "dconvE1"); c.out = W(h, "dq_c"); c.w_raw = D(h, "vae_enc/conv1/raw"); c.mode = 2; c.yprev = W(h, "vae_in");
    launch_deconv4(c, s);
    tn(h, bp.Hx_e, 2 * H, W(h, "dq_c"), V, Ae, 2 * H, V, G(h, "fc_c/w"), V, 0, s);
    colsum(h, W(h, "dq_c"), V, Ae, V, G(h, "fc_c/b"), 0, s);
    g = GemmArgs{};
    g.A = W(h, "dq_c"); g.lda = V; g.M = Ae; g.K = V; g.Bp = D4(h, "fc_c/WT"); g.G = V / 8; g.NT = 2 * H / 32;
    g.out = bp.dH_e; g.ldo = 2 * H; g.N = 2 * H;
    launch_gemm_rows(g, EPI_NONE, s);
    return DESIRE_OK;
}

// ---- d loss / d (Hx | Hy), assembled in dH_e [agents_e, 2H] where the encoder BPTTs start from ----
// fc_c's data gradient is already there (cvae_enc_bwd wrote both halves); this stage ADDS the Hx shares of the row-level stages (K rows per agent):
//   S = decoder + mask fc, in dHx_s (rows of the per-row stages);  I = IOC module, see below.
//   flags            | "dHx_rows" (caller's rows) holds | I reaches the agents through
//   none             | S + I (one buffer)               | "dHx_rows" with S
//   COMPACT_IOC      | S                                | "dHxHy_ioc" [A, H] (ioc_class_dHx: every class's share)
//   COMPACT_ROWS     | I  (S: "cp_dHx_rows")            | "dHx_rows"
//   both             | zeros (S: "cp_dHx_rows")         | "dHxHy_ioc"
// Encoders in the caller's agent order: dH_e += agents("dHx_rows") [+ "dHxHy_ioc"] [+ scatter(agents("cp_dHx_rows"))].
// Encoders on the present agents (COMPACT_ROWS, desire_encode compacted): dH_e += agents("cp_dHx_rows") + gather("dHxHy_ioc"), the latter
// built here from "dHx_rows" when the IOC module did not run per class.  Adds are in this fixed order (bitwise reproducible).
int assemble_dH(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    const int H = d.H, P = bp.n_present;
    if (bp.enc_compact) {
        if (P <= 0) return DESIRE_OK;
        launch_rows_to_agents(bp.dHx_s, bp.dH_e, 2 * H, 1, P, d.K, H, s);                 // S: compact rows -> compact agents
        if (!h->ci_last) {                                                                // I: the caller's rows -> agents -> compact agents
            launch_fill_f32(W(h, "dHxHy_ioc"), (size_t)h->A * H, 0.f, s);
            launch_rows_to_agents(W(h, "dHx_rows"), W(h, "dHxHy_ioc"), H, d.n_scenes, d.mno, d.K, H, s);
        }
        launch_gather_add_agents(W(h, "dHxHy_ioc"), H, bp.dH_e, 2 * H, bp.amap, P, H, s);
        return DESIRE_OK;
    }
    launch_rows_to_agents(W(h, "dHx_rows"), bp.dH_e, 2 * H, d.n_scenes, d.mno, d.K, H, s);      // (all zeros under both flags: kept, it costs one small launch)
    if (h->ci_last) launch_rows_to_agents(W(h, "dHxHy_ioc"), bp.dH_e, 2 * H, h->A, 1, 1, H, s);       // + the slot classes' share (one "row" per agent)
    if (bp.rows_compact && P > 0) {         // S: compact rows -> compact agents -> agents
        launch_fill_f32(W(h, "cp_dHx"), (size_t)P * H, 0.f, s);
        launch_rows_to_agents(bp.dHx_s, W(h, "cp_dHx"), H, 1, P, d.K, H, s);
        launch_scatter_add_agents(W(h, "cp_dHx"), H, bp.dH_e, 2 * H, bp.amap, P, H, s);
    }
    return DESIRE_OK;
}

// ---- Gaussian-head term (desire_set_head_loss; agents_e > 0): nll and d nll / d o per (agent, observed frame), the mean, its gradient; then the
// head's own weight gradients.  The gradient w.r.t. the encoder states enters the X-encoder BPTT, step by step.
int head_nll_bwd(const BwdPass& bp) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s; const desire_dims& d = h->d;
    const int H = d.H, n = bp.agents_e * d.T_obs;
    const float* pastE = bp.enc_compact ? W(h, "cp_past") : bp.past; const float* futE = bp.enc_compact ? W(h, "cp_fut") : bp.fut;
    Timer t(h, s, "bwd_head_nll");
    hipLaunchKernelGGL(k_head_nll, dim3((n * 64 + 255) / 256), dim3(256), 0, s, W(h, "ex_sv_h"), W(h, "ex_sv_x"), pastE, futE,
                       D(h, "gauss_head/w"), D(h, "gauss_head/b"), bp.agents_e, d.T_obs, d.T_pred, H, bp.mno_e, d.sx, d.sy, W(h, "head_nll"), W(h, "head_cnt"),
                       W(h, "head_dO"));
    hipLaunchKernelGGL(k_head_sum, dim3(1), dim3(256), 0, s, W(h, "head_nll"), W(h, "head_cnt"), n, h->head_loss_w, W(h, "loss_out"));
    hipLaunchKernelGGL(k_head_scale, dim3((n * 5 + 255) / 256), dim3(256), 0, s, W(h, "head_dO"), n * 5, h->head_loss_w, W(h, "loss_out"));
    tn(h, W(h, "ex_sv_h"), H, W(h, "head_dO"), 5, (long)n, H, 5, G(h, "gauss_head/w"), 5, 0, s);
    colsum(h, W(h, "head_dO"), 5, (long)n, 5, G(h, "gauss_head/b"), 0, s);
    return DESIRE_OK;
}

// ---- one encoder (agents_e > 0): BPTT over Te steps from the final state (columns col0 .. col0 + H of dH_e), zero initial state, and its weight
// gradients.  slot: the weights' prefix ("enc_x"); sv: the saves' prefix ("ex"); head: the Gaussian-head gradient enters at every step.
int encoder_bwd(const BwdPass& bp, const char* label, const std::string& slot, const std::string& sv, int Te, int col0, bool head) {
    desire_ctx* h = bp.h; hipStream_t s = bp.s;
    const int H = h->d.H;
    Timer t(h, s, label);
    DecBwdArgs e{};
    e.sv_r = W(h, (sv + "_sv_r").c_str()); e.sv_u = W(h, (sv + "_sv_u").c_str());
    e.sv_c = W(h, (sv + "_sv_c").c_str()); e.sv_h = W(h, (sv + "_sv_h").c_str());
    e.w_head = D(h, "head/w");
    if (head) { e.dY0 = W(h, "head_dO"); e.w_head = D(h, "gauss_head/w"); e.nw = 5; }     // d L_head / d h_t = dO_t W5^T, every step
    e.WcT_h = D4(h, (slot + "/WcT_h").c_str()); e.WgT_h = D4(h, (slot + "/WgT_h").c_str());
    e.R = bp.agents_e; e.K = 1; e.mno = bp.mno_e; e.T = Te; e.H = H;
    e.dag = W(h, "enc_dag"); e.dac = W(h, "enc_dac"); e.rh = W(h, "enc_rh"); e.hprev = W(h, "enc_hprev");
    e.dh_init = bp.dH_e + col0; e.ld_init = 2 * H;
    launch_decoder_bwd(e, s);
    const long n = (long)bp.agents_e * Te;
    gru_wgrad(bp, slot, e, W(h, (sv + "_sv_x").c_str()), 2, e.dag, e.dac, n, n, 0, 0, 0);     // (e.bias_part unset: column sums)
    return DESIRE_OK;
}

}  // namespace

extern "C" int desire_backward(desire_handle* h, const float* dev_past, const float* dev_fut, const float* dev_eps, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!h->training) return fail(DESIRE_ERR_STATE, "desire_set_training(h, 1) and a training-mode desire_forward come first");
    if (!dev_past || !dev_fut || (!dev_eps && !h->rng_state)) return fail(DESIRE_ERR_ARG, "null argument");      // (dev_eps == NULL: legal after desire_set_rng)
    if (scene_grad_on(h) && !h->ws.find("sg_wcat")) return fail(DESIRE_ERR_STATE, "scene-gradient buffers missing");
    if (h->roff_w > 0.f && !(h->off_scale > 0.f)) return fail(DESIRE_ERR_STATE, "desire_set_refined_loss: the off-road scale was reset to a value that is not > 0");
    if (int rc = backward_alloc(h)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const BwdPass bp = make_pass(h, dev_past, dev_fut, dev_eps, s);
    const bool rows = bp.rows_s > 0, agents = bp.agents_e > 0, head = h->head_loss_w > 0.f;
    int rc = loss_grads(bp);
    if (!rc && rows) rc = decoder_bwd(bp);
    if (!rc) rc = ioc_bwd(bp);
    if (!rc && h->img_set) rc = scene_cnn_bwd(bp);
    if (!rc && rows) rc = mask_bwd(bp);
    if (!rc && rows) rc = cvae_dec_bwd(bp);
    if (!rc) {
        Timer t(h, s, "bwd_cvae_enc");              // (one label over both stages, as the profile tables have it)
        rc = cvae_enc_bwd(bp);                       // (guards agents_e > 0 itself, after the latent's gradient)
        if (!rc) rc = assemble_dH(bp);
    }
    if (!rc && agents && head) rc = head_nll_bwd(bp);
    if (!rc && agents) rc = encoder_bwd(bp, "bwd_encoder_y", "enc_y", "ey", h->d.T_pred, h->d.H, false);
    if (!rc && agents) rc = encoder_bwd(bp, "bwd_encoder_x", "enc_x", "ex", h->d.T_obs, 0, head);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    // (the read-back tests the plan of the handle's own mno, not of the slot classes that ran: kept as it is)
    return ioc_plan(h).bwd == IocBwd::CLUSTER ? ioc_cluster_check(h, s, "IOC cluster backward:") : DESIRE_OK;
}
