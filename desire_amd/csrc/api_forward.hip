// api_forward.hip -- the launch sequence of the hot path behind desire_encode / desire_sample / desire_ioc_refine / desire_forward, including the
// present-row compaction and the IOC slot classes (DESIRE_FLAG_COMPACT_*).  Host code only; split out of api.hip in round 5.
#include "ctx.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// DESIRE_FLAG_COMPACT_ROWS: the per-row sample-generation stages run on the rows of present agents only (kernels_compact.hip)
bool compact_rows(const desire_ctx* h) { return (h->d.flags & DESIRE_FLAG_COMPACT_ROWS) != 0; }
// DESIRE_FLAG_COMPACT_IOC: windows re-seated in the smallest slot class that holds their present agents (kernels_compact.hip).  Shapes served by the
// step-wise IOC (more than 128 slots, or split operands at H = 256) keep their own layout.
bool compact_ioc(const desire_ctx* h) { return (h->d.flags & DESIRE_FLAG_COMPACT_IOC) && ioc_plan(h).fwd != IocFwd::STEPWISE; }
ClassLayout class_layout(const desire_ctx* h, bool pad, const int* counts) {
    const desire_dims& d = h->d;
    ClassLayout L;
    // the three largest candidates below the handle's own mno, then mno itself.  Candidates: 8, 16, 32, 64, 96; with padded tiles also 10 (three
    // groups of <= 10 slots per 32-row tile: a window with 9 present agents -- the typical SDD bookstore window -- runs in 10 rows per sample, not 16)
    int cand[6], nc = 0;
    for (int m : {8, 10, 16, 32, 64, 96}) if (m < d.mno && (m != 10 || pad)) cand[nc++] = m;
    for (int i = nc > 3 ? nc - 3 : 0; i < nc; ++i) L.m[L.n++] = cand[i];
    L.m[L.n++] = d.mno;
    for (int i = L.n; i < 4; ++i) L.m[i] = d.mno;
    for (int c = 0; c < L.n; ++c) {
        IocView& v = L.c[c];
        v.cls = c; v.mno = L.m[c]; v.n_scenes = counts ? counts[c] : d.n_scenes;
        v.gpt = (v.mno <= 32 && 32 % v.mno) ? 32 / v.mno : 0; v.ngrp = v.n_scenes * d.K;          // padded tiles for a class that does not divide 32
        v.R = v.gpt ? (long)((v.ngrp + v.gpt - 1) / v.gpt) * 32 : (long)v.ngrp * v.mno;
        v.agent_off = L.agents; v.row_off = L.rows; v.win_off = L.wins;
        L.agents += (size_t)v.n_scenes * v.mno; L.rows += (size_t)v.R; L.wins += (size_t)v.n_scenes;
    }
    return L;
}
IocView ioc_view(desire_ctx* h, const IocView* cls) {
    if (!cls)
        return IocView{-1, h->d.mno, h->d.n_scenes, 0, 0, h->R, 0, 0, 0, W(h, "HxHy"), W(h, "p_last"), Wt<uint8_t>(h, "valid"),
                       Wt<int32_t>(h, "grid_of_scene")};
    IocView v = *cls;
    v.Hx = W(h, "ci_Hx") + v.agent_off * 2 * h->d.H; v.p_last = W(h, "ci_pl") + v.agent_off * 2;
    v.valid = Wt<uint8_t>(h, "ci_valid") + v.agent_off; v.gos = Wt<int32_t>(h, "ci_gos") + v.win_off;
    v.cmap = Wt<const int32_t>(h, "ci_map") + (size_t)v.cls * h->A; v.win = Wt<const int32_t>(h, "ci_win") + (size_t)v.cls * h->d.n_scenes;
    v.Y = W(h, "ci_Y") + v.row_off * h->d.T_pred * 2; v.score = W(h, "ci_score") + v.row_off;
    return v;
}
// DEVICE-SIDE COUNTS (round 6): in inference with frozen batch-norm the host never learns how many agents are present -- every compacted launch is
// sized for the worst case and reads its count from the scans' device words (dyn_count.h: DynCount), so a compacted call has no host wait and can be
// captured in a hipGraph.  Training keeps the read-back (its backward sizes two dozen reductions from P), and so do per-sample batch statistics
// (bn_mode 1: the normalisation kernels are not count-aware) and desire_set_option("compact_host_counts", 1) -- the A/B switch.
bool compact_dyn(const desire_ctx* h) { return !h->training && h->d.bn_mode == 0 && !h->cp_host_counts; }
int compact_setup(desire_ctx* h) {
    const desire_dims& d = h->d;
    const size_t A = h->A, R = h->R, f = sizeof(float);
    // slot-class buffers: with device-side counts a class's region starts at a STATIC offset (the sum of the worst cases of the classes before it).
    // Sized for both class sets the handle can take -- with and without class 10, which ioc_form, train_fp32_mask and the training mode switch on a
    // live handle -- so they never grow and pointers captured in a hipGraph stay valid.
    size_t Ac = A, Rc = ioc_save_rows(h), Wc = (size_t)d.n_scenes;
    if (d.flags & DESIRE_FLAG_COMPACT_IOC) {
        const ClassLayout a = class_layout(h, false, nullptr), b = class_layout(h, true, nullptr);
        Ac = std::max({a.agents, b.agents, A}); Rc = std::max({a.rows, b.rows, ioc_save_rows(h)}); Wc = std::max(a.wins, b.wins);
    }
    const WsItem list[] = {{"cp_amap", A * sizeof(int32_t)}, {"cp_inv", A * sizeof(int32_t)}, {"cp_count", 8 * sizeof(int32_t)}, {"cp_HxHy", A * 2 * d.H * f},
                       {"cp_plast", A * 2 * f}, {"cp_params", A * 2 * d.L * f}, {"cp_Y0", R * (size_t)d.T_pred * 2 * f},
                       {"cp_past", A * (size_t)d.T_obs * 3 * f}, {"cp_fut", A * (size_t)d.T_pred * 3 * f}, {"cp_valid2", A}};
    const WsItem list_ioc[] = {{"ci_win", 4 * (size_t)d.n_scenes * sizeof(int32_t)}, {"ci_map", 4 * A * sizeof(int32_t)}, {"ci_Hx", Ac * 2 * d.H * f}, {"ci_pl", Ac * 2 * f},
                           {"ci_valid", Ac}, {"ci_gos", Wc * sizeof(int32_t)}, {"ci_Y", Rc * (size_t)d.T_pred * 2 * f}, {"ci_score", Rc * f}};      // (+ a partial padded tile per class)
    if (int rc = ws_ensure(h, list)) return rc;
    if (h->d.flags & DESIRE_FLAG_COMPACT_IOC) { if (int rc = ws_ensure(h, list_ioc)) return rc; }
    if (!h->cp_ev) HIPCHK(hipEventCreateWithFlags(&h->cp_ev, hipEventDisableTiming));
    if (!h->cp_host) {
        int32_t* p = nullptr;
        if (hipHostMalloc(reinterpret_cast<void**>(&p), 8 * sizeof(int32_t), hipHostMallocMapped) != hipSuccess || !p)
            return fail(DESIRE_ERR_HIP, "hipHostMalloc failed for the present-agent count words");
        for (int i = 0; i < 8; ++i) p[i] = 0;
        h->cp_host = p;
    }
    return DESIRE_OK;
}
// the present-agent scan (+ the slot-class scan) over `valid`, and the event desire_sample / desire_ioc_refine wait on
static int compact_scans(desire_ctx* h, hipStream_t s) {
    const desire_dims& d = h->d;
    launch_present_scan(Wt<const uint8_t>(h, "valid"), h->A, Wt<int32_t>(h, "cp_amap"), Wt<int32_t>(h, "cp_inv"), Wt<int32_t>(h, "cp_count"), h->cp_host, s);
    if (compact_ioc(h)) {
        const ClassLayout L = class_layout(h, ioc_plan(h).padded, nullptr);
        launch_class_scan(Wt<const uint8_t>(h, "valid"), d.n_scenes, d.mno, L.n, L.m, d.K, h->ci_min_rows, Wt<int32_t>(h, "ci_win"),
                          Wt<int32_t>(h, "ci_map"), Wt<int32_t>(h, "cp_count") + 4, h->cp_host + 4, s);
    }
    if (!compact_dyn(h)) HIPCHK(hipEventRecord(h->cp_ev, s));             // (device-side counts: nobody waits, and the call stays capturable)
    h->cp_pending = true;
    return DESIRE_OK;
}
// waits (once per desire_encode) for the scans' counts to reach the host
static int compact_wait(desire_ctx* h, hipStream_t s) {
    if (!h->cp_pending) return fail(DESIRE_ERR_STATE, "DESIRE_FLAG_COMPACT_*: desire_encode comes first (it builds the present-agent maps)");
    if (compact_dyn(h)) return DESIRE_OK;                                // the kernels read the counts themselves
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(DESIRE_ERR_STATE, "DESIRE_FLAG_COMPACT_* read the present-agent counts back: not capturable in a hipGraph");
    HIPCHK(hipEventSynchronize(h->cp_ev));
    return DESIRE_OK;
}
// the mapped present-agent count word: read back after compact_wait (an out-of-range value is an error), or as a GUESS of P for choices that are about
// speed only: whatever the word holds -- the previous call's count, or this one's if the scan has already run (under hipGraph capture always the
// previous call's, baked into the graph).  It picks the variant of a row GEMM (GemmArgs.M_hint) and, as DynCount.hint (dyn_count.h), it SHRINKS the grids
// of the strided launches -- the encoder pair, deconv2, deconv3 and the six-product forms of those two -- from the worst case to hint * 1.25 + 256
// units (dyn_units).  The guess is never a bound on the work: every kernel reads the real count, and a strided kernel serves a count above its grid
// with further trips of its tile loop.
static int present_count(const desire_ctx* h, int* P) {
    *P = *static_cast<volatile int32_t*>(h->cp_host);
    return (*P < 0 || *P > h->A) ? fail(DESIRE_ERR_HIP, "present-agent scan returned a count out of range") : 0;
}
static int count_hint(const desire_ctx* h) {
    const int P = *static_cast<volatile int32_t*>(h->cp_host);
    return (P < 0 || P > h->A) ? 0 : P;
}

// the packed operand(s) stage st reads under form f (gen_plan.h: the one place that names them)
static const float4* gen_op(desire_ctx* h, GenStage st, GenForm f) { return D4(h, gen_operands(st, f).a); }
static void gen_op2(desire_ctx* h, GenStage st, GenForm f, const float4*& Whg, const float4*& Whc) {
    const GenOps o = gen_operands(st, f);
    Whg = D4(h, o.a); Whc = D4(h, o.b);
}

// the fp32 weights of the GRU encoder `prefix` ("enc_x" / "enc_y")
void enc_weights(desire_ctx* h, const char* prefix, EncArgs& e) {
    const std::string p(prefix);
    e.wx_g = D(h, (p + "/gk").c_str()); e.b_g = D(h, (p + "/gb").c_str()); e.wx_c = D(h, (p + "/ck").c_str()); e.b_c = D(h, (p + "/cb").c_str());
    e.Whg = D4(h, (p + "/Whg").c_str()); e.Whc = D4(h, (p + "/Whc").c_str());
}

// batch statistics of one conv layer's output x [n, P, C] (dims.bn_mode != 0: the conv ran with a linear epilogue): normalise + activate in place,
// 1: per sample (k_instnorm_act), 2: over the whole batch.  Training keeps the pre-norm tensor next to the activation for the backward.
static void batch_stats_act(desire_ctx* h, const char* layer, float* x, int n, int P, int C, int sig, hipStream_t s) {
    const std::string l(layer);
    const float* ga = D(h, (l + "/gamma").c_str()); const float* be = D(h, (l + "/beta").c_str());
    if (h->training) launch_copy_f32(W(h, (l.substr(l.rfind('/') + 1) + "_pre").c_str()), x, (size_t)n * P * C, s);
    if (h->d.bn_mode == 2) launch_batchnorm_act(x, (size_t)n, P, C, ga, be, sig, W(h, "bn_part"), W(h, "bn_stat"), s);
    else launch_instnorm_act(x, n, P, C, ga, be, sig, s);
}

extern "C" int desire_encode(desire_handle* h, const float* dev_past, const float* dev_fut, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    const desire_dims& d = h->d;
    if (!dev_past) return fail(DESIRE_ERR_ARG, "dev_past is null");
    if (d.posterior && !dev_fut) return fail(DESIRE_ERR_ARG, "dims.posterior=1 needs dev_fut");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int H = d.H, A = h->A;
    const GenPlan plan = gen_plan(h);
    // DESIRE_FLAG_COMPACT_ROWS: the encoder stack is per-agent as well.  `valid` is read off the last observed frame first, the scans run, the host
    // learns P, and the GRU encoders + CVAE encoder run on the P present agents as ONE pseudo-scene of P slots (frames gathered to [1, T, P, 3]);
    // HxHy / p_last / params are scattered back for the stages that keep the caller's layout (IOC, losses).  Ae = agents the stack runs on.
    // (not while the Gaussian-head loss is on: that term counts every (object, observed frame) pair, including objects that have left by the last
    //  observed frame, which the present-agent map does not hold)
    const bool enc_c = compact_rows(h) && !(h->training && h->head_loss_w > 0.f);
    const bool dyn = enc_c && compact_dyn(h);
    const int32_t* dynP = nullptr;                                       // the present-agent count on the device (cp_count[0]) when `dyn`
    int hintP = 0;
    h->cp_enc = false;
    int Ae = A;
    const float* pastE = dev_past; const float* futE = dev_fut;
    float* HxE = W(h, "HxHy"); float* plE = W(h, "p_last"); uint8_t* validE = Wt<uint8_t>(h, "valid");
    float* paramsE = W(h, "params");
    const int32_t* amap = nullptr;
    if (enc_c) {
        if (int rc = compact_setup(h)) return rc;
        if (dyn) {
            dynP = Wt<const int32_t>(h, "cp_count");
            hintP = count_hint(h);
        }
        launch_valid_from_frames(dev_past, d.n_scenes, d.T_obs, d.mno, validE, s);
        if (int rc = compact_scans(h, s)) return rc;
        if (int rc = compact_wait(h, s)) return rc;
        int P = A;                                                       // device-side counts: the worst case sizes the launches
        if (!dyn) { if (int rc = present_count(h, &P)) return rc; }
        h->cp_P = dyn ? -1 : P; h->cp_enc = true; Ae = P;
        launch_fill_f32(W(h, "HxHy"), (size_t)A * 2 * H, 0.f, s); launch_fill_f32(W(h, "p_last"), (size_t)A * 2, 0.f, s);
        if (d.posterior) launch_fill_f32(W(h, "params"), (size_t)A * 2 * d.L, 0.f, s);
        if (P == 0) { HIPCHK(hipGetLastError()); return DESIRE_OK; }
        amap = Wt<const int32_t>(h, "cp_amap");
        launch_gather_frames(dev_past, W(h, "cp_past"), amap, P, d.T_obs, d.mno, s, dynP);
        if (d.posterior) launch_gather_frames(dev_fut, W(h, "cp_fut"), amap, P, d.T_pred, d.mno, s, dynP);
        pastE = W(h, "cp_past"); futE = W(h, "cp_fut");
        HxE = W(h, "cp_HxHy"); plE = W(h, "cp_plast"); validE = Wt<uint8_t>(h, "cp_valid2"); paramsE = W(h, "cp_params");
    }
    EncArgs e{};
    e.n_scenes = enc_c ? 1 : d.n_scenes; e.mno = enc_c ? Ae : d.mno; e.sx = d.sx; e.sy = d.sy; e.H = H;
    e.frames = pastE; e.T = d.T_obs;
    enc_weights(h, "enc_x", e);
    e.out = HxE; e.ldo = 2 * H; e.p_last = plE; e.valid = validE;
    e.dyn = DynCount{dynP, 1, hintP};
    if (h->training) { e.sv_r = W(h, "ex_sv_r"); e.sv_u = W(h, "ex_sv_u"); e.sv_c = W(h, "ex_sv_c"); e.sv_h = W(h, "ex_sv_h"); e.sv_x = W(h, "ex_sv_x"); }
    const EncArgs ex = e;
    if (d.posterior) {
        e.frames = futE; e.T = d.T_pred;
        enc_weights(h, "enc_y", e);
        e.out = HxE + H; e.p_last = nullptr; e.valid = nullptr;
        if (h->training) { e.sv_r = W(h, "ey_sv_r"); e.sv_u = W(h, "ey_sv_u"); e.sv_c = W(h, "ey_sv_c"); e.sv_h = W(h, "ey_sv_h"); e.sv_x = W(h, "ey_sv_x"); }
    }
    if (plan.encoder == GenForm::BF16) {
        EncArgs e16 = ex;
        gen_op2(h, GenStage::ENC_X, plan.encoder, e16.Whg, e16.Whc);
        { Timer t(h, s, "encoder_x"); launch_encoder_bf16(e16, s); }
        if (d.posterior) { gen_op2(h, GenStage::ENC_Y, plan.encoder, e.Whg, e.Whc); Timer t(h, s, "encoder_y"); launch_encoder_bf16(e, s); }
    } else if (d.posterior) {      // the two encoders are independent and latency-bound: one launch
        Timer t(h, s, "encoder_xy"); launch_encoder_pair(ex, e, s);
    } else { Timer t(h, s, "encoder_x"); launch_encoder(ex, s); }
    if (enc_c) {          // back to the caller's layout for the IOC stage (absent agents: zeros, filled above)
        launch_scatter_agents(HxE, W(h, "HxHy"), amap, Ae, 2 * H, s, dynP);
        launch_scatter_agents(plE, W(h, "p_last"), amap, Ae, 2, s, dynP);
    } else if (compact_rows(h) || compact_ioc(h)) {
        // DESIRE_FLAG_COMPACT_IOC alone: the slot-class maps are built behind the encoder that writes `valid`; their sizes reach the host through a
        // mapped word while the CVAE encoder below keeps the device busy, and desire_ioc_refine waits on the event before it sizes its launches
        if (int rc = compact_setup(h)) return rc;
        if (int rc = compact_scans(h, s)) return rc;
    }
    if (d.posterior) {
        GemmArgs g{};
        g.A = HxE; g.lda = 2 * H; g.M = Ae; g.K = 2 * H; g.Bp = D4(h, "fc_c/W"); g.G = 2 * H / 8;
        g.NT = h->V / 32; g.out = W(h, "vae_in"); g.ldo = h->V; g.N = h->V; g.p0 = D(h, "fc_c/b");
        g.dyn = DynCount{dynP, 1, hintP}; g.M_hint = hintP;
        { Timer t(h, s, "fc_c"); launch_gemm_rows(g, EPI_BIAS_RELU, s); }
        ConvArgs c{};
        c.n = Ae; c.dyn = DynCount{dynP, 1, hintP};
        c.in = W(h, "vae_in"); c.out = W(h, "c1"); c.w_raw = D(h, "vae_enc/conv1/raw");
        c.scale = D(h, "vae_enc/conv1/scale"); c.shift = D(h, "vae_enc/conv1/shift");
        const bool pobn = plan.batch_stats;               // batch statistics: linear conv epilogue, then a normalise + activate pass per layer
        auto norm = [&](const char* layer, float* x, int P, int C) { batch_stats_act(h, layer, x, Ae, P, C, 0, s); };
        if (pobn) c.mode = 3;
        { Timer t(h, s, "conv1"); launch_conv1(c, s); if (pobn) norm("vae_enc/conv1", W(h, "c1"), 256, 32); }
        c.in = W(h, "c1"); c.out = W(h, "c2"); c.Wp = gen_op(h, GenStage::CONV2, plan.conv23);
        c.scale = D(h, "vae_enc/conv2/scale"); c.shift = D(h, "vae_enc/conv2/shift");
        if (plan.conv23 == GenForm::BF16) { Timer t(h, s, "conv2"); launch_conv2_bf16(c, s); }
        else { Timer t(h, s, "conv2"); launch_conv2(c, s); if (pobn) norm("vae_enc/conv2", W(h, "c2"), 64, 64); }
        c.in = W(h, "c2"); c.out = W(h, "c3"); c.Wp = gen_op(h, GenStage::CONV3, plan.conv23);
        c.scale = D(h, "vae_enc/conv3/scale"); c.shift = D(h, "vae_enc/conv3/shift");
        if (plan.conv23 == GenForm::BF16) { Timer t(h, s, "conv3"); launch_conv3_bf16(c, s); }
        else { Timer t(h, s, "conv3"); launch_conv3(c, s); if (pobn) norm("vae_enc/conv3", W(h, "c3"), 16, 128); }
        g = GemmArgs{};
        g.A = W(h, "c3"); g.lda = 2048; g.M = Ae; g.K = 2048; g.Bp = D4(h, "vae_enc/fc/W"); g.G = 2048 / 8;
        g.NT = (2 * d.L + 31) / 32; g.out = paramsE; g.ldo = 2 * d.L; g.N = 2 * d.L; g.p0 = D(h, "vae_enc/fc/b");
        g.dyn = DynCount{dynP, 1, hintP}; g.M_hint = hintP;
        { Timer t(h, s, "vae_enc_fc"); launch_gemm_rows(g, EPI_BIAS, s); }
        if (enc_c) launch_scatter_agents(paramsE, W(h, "params"), amap, Ae, 2 * d.L, s, dynP);       // desire_losses / the reparam backward read them per agent
    }
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_sample(desire_handle* h, const float* dev_eps, float* dev_Yhat, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!dev_Yhat || (!dev_eps && !h->rng_state)) return fail(DESIRE_ERR_ARG, "null argument");      // (dev_eps == NULL: legal after desire_set_rng)
    const desire_dims& d = h->d;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int H = d.H;
    const GenPlan plan = gen_plan(h);
    if (!dev_eps) launch_rng_begin(h->rng_state, s);           // a sampling call that generates its eps is one draw, whatever it then runs
    // per-row stages: all R = A*K rows, or (DESIRE_FLAG_COMPACT_ROWS) the K*P rows of the P present agents laid out as one pseudo-scene of P
    // slots (kernels_compact.hip) -- the kernels below are the same either way, they only see (R, K, mno) and the agent-level inputs
    int R = h->R, mno = d.mno;
    const float* HxS = W(h, "HxHy"); const float* plS = W(h, "p_last"); float* Yout = W(h, "Y0");
    const bool compact = compact_rows(h);
    const bool dyn = compact && compact_dyn(h);
    const int32_t* dynP = dyn ? Wt<const int32_t>(h, "cp_count") : nullptr;      // device-side count: launches sized for P = A
    h->cp_last = compact;
    if (compact) {
        if (int rc = compact_wait(h, s)) return rc;
        int P = h->A;
        if (!dyn) { if (int rc = present_count(h, &P)) return rc; }
        h->cp_P = dyn ? -1 : P;
        R = P * d.K; mno = P;
        const size_t RT2 = (size_t)h->R * d.T_pred * 2;
        if (P == 0) {       // nothing present: every row is padding
            launch_fill_f32(W(h, "Y0"), RT2, 0.f, s); launch_fill_f32(dev_Yhat, RT2, 0.f, s);
            HIPCHK(hipGetLastError());
            return DESIRE_OK;
        }
        const int32_t* amap = Wt<const int32_t>(h, "cp_amap");
        Timer t(h, s, "compact_gather");
        if (!h->cp_enc) {           // (an encoder stack that ran compact has left all three in place)
            launch_gather_agents(W(h, "HxHy"), W(h, "cp_HxHy"), amap, P, 2 * H, s, dynP);
            launch_gather_agents(W(h, "p_last"), W(h, "cp_plast"), amap, P, 2, s, dynP);
            if (d.posterior) launch_gather_agents(W(h, "params"), W(h, "cp_params"), amap, P, 2 * d.L, s, dynP);
        }
        HxS = W(h, "cp_HxHy"); plS = W(h, "cp_plast"); Yout = W(h, "cp_Y0");
    }
    if (!dev_eps) {          // the generator's twins (kernels_rng.hip): eps computed in the kernel from rng_state.used
        Timer t(h, s, "reparam");
        if (compact) launch_reparam_c_rng(W(h, "cp_params"), rng_args(h), W(h, "z"), Wt<const int32_t>(h, "cp_amap"), mno, d.K, d.mno, d.L, d.posterior, s, dynP);
        else launch_reparam_rng(W(h, "params"), rng_args(h), W(h, "z"), R, d.L, d.K, d.mno, d.posterior, s);
    }
    else if (compact) { Timer t(h, s, "reparam"); launch_reparam_c(W(h, "cp_params"), dev_eps, W(h, "z"), Wt<const int32_t>(h, "cp_amap"), mno, d.K, d.mno, d.L, d.posterior, s, dynP); }
    else { Timer t(h, s, "reparam"); launch_reparam(W(h, "params"), dev_eps, W(h, "z"), R, d.L, d.K, d.mno, d.posterior, s); }
    auto normd = [&](const char* layer, float* x, int P, int C, int sig) { batch_stats_act(h, layer, x, R, P, C, sig, s); };
    GemmArgs g{};
    g.A = W(h, "z"); g.lda = d.L; g.M = R; g.K = d.L; g.Bp = gen_op(h, GenStage::DECONV1, plan.deconv1); g.G = d.L / 8;
    g.NT = 64; g.out = W(h, "d1"); g.ldo = 2048; g.N = 2048;
    g.p0 = D(h, "vae_dec/deconv1/scale"); g.p1 = D(h, "vae_dec/deconv1/shift"); g.chmod = 128;
    int hintS = 0;                                                       // count hint for this call's launches (see desire_encode)
    if (dyn) hintS = count_hint(h);
    g.dyn = DynCount{dynP, d.K, hintS}; g.M_hint = hintS * d.K;
    const bool pobn = plan.batch_stats;
    { Timer t(h, s, "deconv1");
      switch (plan.deconv1) {
          case GenForm::BF16: launch_deconv1_bf16(g, s); break;
          case GenForm::X6: launch_deconv1_x6(g, s); break;
          case GenForm::FP32: launch_gemm_rows(g, pobn ? EPI_NONE : EPI_SCALE_SHIFT_ELU, s); if (pobn) normd("vae_dec/deconv1", W(h, "d1"), 16, 128, 0);
      } }
    ConvArgs c{};
    c.n = R; c.dyn = DynCount{dynP, d.K, hintS};
    if (pobn) c.mode = 3;
    c.in = W(h, "d1"); c.out = W(h, "d2"); c.Wp = gen_op(h, GenStage::DECONV2, plan.deconv2);
    c.scale = D(h, "vae_dec/deconv2/scale"); c.shift = D(h, "vae_dec/deconv2/shift");
    { Timer t(h, s, "deconv2");
      switch (plan.deconv2) {
          case GenForm::BF16: launch_deconv2_bf16(c, s); break;
          case GenForm::X6: launch_deconv2_x6(c, s, plan.np); break;
          case GenForm::FP32: launch_deconv2(c, s); if (pobn) normd("vae_dec/deconv2", W(h, "d2"), 64, 64, 0);
      } }
    c.in = W(h, "d2"); c.out = W(h, "d3"); c.Wp = gen_op(h, GenStage::DECONV3, plan.deconv3);
    c.scale = D(h, "vae_dec/deconv3/scale"); c.shift = D(h, "vae_dec/deconv3/shift");
    const float* w4 = D(h, gen_operands(GenStage::DECONV4, plan.deconv4()).a);       // fused: the tap-product pack; else deconv4's raw taps
    if (plan.fuse34) {
        c.w_raw = w4; c.out = W(h, "xhat");
        Timer t(h, s, "deconv34");
        launch_deconv34_bf16(c, D(h, "vae_dec/deconv4/scale"), D(h, "vae_dec/deconv4/shift"), s);
    } else {
        { Timer t(h, s, "deconv3");
          switch (plan.deconv3) {
              case GenForm::BF16: launch_deconv3_bf16(c, s); break;
              case GenForm::X6: launch_deconv3_x6(c, s, plan.np); break;
              case GenForm::FP32: launch_deconv3(c, s); if (pobn) normd("vae_dec/deconv3", W(h, "d3"), 256, 32, 0);
          } }
        c.in = W(h, "d3"); c.out = W(h, "xhat"); c.w_raw = w4;
        c.scale = D(h, "vae_dec/deconv4/scale"); c.shift = D(h, "vae_dec/deconv4/shift");
        { Timer t(h, s, "deconv4"); launch_deconv4(c, s);
          if (pobn) normd("vae_dec/deconv4", W(h, "xhat"), 1024, 1, 1); }
    }
    MaskArgs m{};
    m.xhat = W(h, "xhat"); m.R = R; m.V = h->V; m.H = H; m.Hl = h->Hl; m.K = d.K; m.mno = mno;
    m.Wp = gen_op(h, GenStage::MASK, plan.mask); m.bias = D(h, "mask/b"); m.Hx = HxS; m.ldhx = 2 * H; m.xz = W(h, "xz");
    m.dyn = DynCount{dynP, 1, hintS};
    if (h->training) m.sv_p = W(h, "mask_sv_p");
    { Timer t(h, s, "mask_fc");
      switch (plan.mask) {
          case GenForm::BF16: launch_mask_bf16(m, s); break;
          case GenForm::X6: launch_mask_x6(m, s); break;
          case GenForm::FP32: launch_mask(m, s);
      } }
    DecArgs a{};
    a.xz = W(h, "xz"); a.Hx = HxS; a.ldhx = 2 * H; a.p_last = plS;
    a.R = R; a.K = d.K; a.mno = mno; a.H = H; a.T = d.T_pred;
    a.Wxg = D4(h, "dec/Wxg"); a.Wxc = D4(h, "dec/Wxc"); gen_op2(h, GenStage::DECODER, plan.decoder, a.Whg, a.Whc);
    a.b_g = D(h, "dec/gb"); a.b_c = D(h, "dec/cb"); a.w_head = D(h, "head/w"); a.b_head = D(h, "head/b");
    a.Y = Yout; a.hdump = nullptr; a.dyn = DynCount{dynP, 1, hintS};
    if (d.ref_compat) { a.T = d.n_dec; a.hdump = W(h, "dec_states"); }       // model/model.py:280-285: 7 steps, the states are the output
    if (h->training) { a.hdump = W(h, "dec_sv_h"); a.sv_r = W(h, "dec_sv_r"); a.sv_u = W(h, "dec_sv_u"); a.sv_c = W(h, "dec_sv_c"); }
    { Timer t(h, s, "decoder");
      switch (plan.decoder) {
          case GenForm::BF16: launch_decoder_bf16(a, s); break;
          case GenForm::X6: launch_decoder_x6(a, s, plan.np); break;
          case GenForm::FP32: launch_decoder(a, s);
      } }
    if (d.ref_compat)      // model/model.py:286-289: each state [H] re-read as T_obs points (x, y) -> [A, n_dec, T_obs, 2]
        launch_copy_cols(dev_Yhat, W(h, "dec_states"), (size_t)R * d.n_dec, h->Hl, H, s);
    else if (compact) {     // back to the caller's row layout; rows of absent agents are zeros (the cost masks them, model/model.py:351-366)
        Timer t(h, s, "compact_scatter");
        const size_t RT2 = (size_t)h->R * d.T_pred * 2;
        launch_fill_f32(W(h, "Y0"), RT2, 0.f, s); launch_fill_f32(dev_Yhat, RT2, 0.f, s);
        launch_scatter_rows(Yout, W(h, "Y0"), dev_Yhat, Wt<const int32_t>(h, "cp_amap"), mno, d.K, d.mno, d.T_pred * 2, s, dynP);
    } else
        launch_copy_f32(dev_Yhat, W(h, "Y0"), (size_t)R * d.T_pred * 2, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

int ioc_cluster_exchange(desire_ctx* h, size_t n_groups, bool reset_err, hipStream_t s) {
    if (int rc = ws_ensure(h, {{"hex", (size_t)2 * h->R * h->d.H * sizeof(float)}, {"grp_cnt", ((size_t)h->R / 32 + 1) * sizeof(int)}, {"ioc_err", sizeof(int)}})) return rc;
    HIPCHK(hipMemsetAsync(W(h, "grp_cnt"), 0, n_groups * sizeof(int), s));
    if (reset_err) HIPCHK(hipMemsetAsync(W(h, "ioc_err"), 0, sizeof(int), s));
    return DESIRE_OK;
}
int ioc_cluster_check(desire_ctx* h, hipStream_t s, const char* what) {
    int err = 0;
    HIPCHK(hipMemcpyAsync(&err, W(h, "ioc_err"), sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return err ? fail(DESIRE_ERR_HIP, std::string(what) + " hand-off timed out (workgroups of a group were not co-resident)") : DESIRE_OK;
}
#ifdef DESIRE_IOC_TIMING
void ioc_timing_report(const long long* dbg, const char* const* names, int n, hipStream_t s) {
    long long host[16];
    (void)hipStreamSynchronize(s); (void)hipMemcpy(host, dbg, n * sizeof(long long), hipMemcpyDeviceToHost);
    long long tot = 0; for (int k = 0; k < n; ++k) tot += host[k];
    for (int k = 0; k < n; ++k) fprintf(stderr, "[ioc timing] %-45s %12lld cyc  %5.1f%%\n", names[k], host[k], 100.0 * host[k] / (double)tot);
}
#endif

// One IOC launch sequence over a view of the handle's rows (the handle's own layout, or one slot class); training-mode saves go to the view's
// row offset in the shared buffers.
static int ioc_core(desire_handle* h, const IocView& v, hipStream_t s) {
    const desire_dims& d = h->d;
    if (h->training && d.bf16 == 1) return fail(DESIRE_ERR_STATE, "bf16 operands are inference-only");
    IocArgs a{};
    a.Y = v.Y; a.score = v.score; a.Hx = v.Hx; a.ldhx = 2 * d.H; a.p_last = v.p_last; a.valid = v.valid;
    a.R = (int)v.R; a.K = d.K; a.mno = v.mno; a.H = d.H; a.T = d.T_pred; a.iters = d.iters;
    a.C = d.C; a.Gh = d.Gh; a.Gw = d.Gw; a.E_v = d.E_v; a.G = d.grid_size; a.nb_w = d.nb_w; a.nb_h = d.nb_h;
    a.grids = h->grids; a.grid_of_scene = v.gos; a.bin_tab = d.bin_mode == 1 ? W(h, "bin_tab") : nullptr;
    a.w_vel = D(h, "ioc/vel_w"); a.b_vel = D(h, "ioc/vel_b");
    a.Wsoc = D4(h, "ioc/Wsoc"); a.b_soc = D(h, "ioc/soc_b"); a.Wsoc_c = D4(h, "ioc/Wsoc_c");
    a.Wg = D4(h, "ioc/Wg"); a.Wc = D4(h, "ioc/Wc"); a.b_g = D(h, "ioc/gb"); a.b_c = D(h, "ioc/cb");
    a.w_score = D(h, "ioc/score_w"); a.b_score = D(h, "ioc/score_b");
    a.Wreg = D4(h, "ioc/Wreg"); a.b_reg = D(h, "ioc/reg_b"); a.NTreg = (2 * d.T_pred + 31) / 32;
    a.variant = d.ioc_form; a.gpt = v.gpt; a.ngrp = v.ngrp; a.dyn = DynCount{v.dynN, 1, 0};
    const IocPlan p = ioc_plan(d, h->training, v.mno, v.gpt, v.R, [&](int n) { return ioc_bin_split_capacity(a, n); });
    if (!p.fp32_weights()) { a.Wsoc = D4(h, "ioc/Wsoc16"); a.Wg = D4(h, "ioc/Wg16"); a.Wc = D4(h, "ioc/Wc16"); a.Wreg = D4(h, "ioc/Wreg16"); }
    if (p.cluster()) {
        if (int rc = ioc_cluster_exchange(h, (size_t)v.R / v.mno, true, s)) return rc;
        a.hex = W(h, "hex"); a.grp_cnt = Wt<int>(h, "grp_cnt"); a.err = Wt<int>(h, "ioc_err");
    }
    if (p.nspl > 1) {
        const size_t tiles = ((size_t)v.R + 31) / 32, tiles_max = ((size_t)h->R + 31) / 32;
        if (int rc = ws_ensure(h, {{"hex_s", tiles_max * 2 * 4 * 32 * d.H * sizeof(float)}, {"cnt_s", tiles_max * sizeof(int)}})) return rc;
        // the error word is mapped host memory: no read-back (and no stream synchronisation) per call; a timed-out hand-off is
        // reported by the NEXT call on this handle.  The kernels write it with system-scope atomics.
        if (!h->host_err) {
            if (hipHostMalloc(reinterpret_cast<void**>(&h->host_err), sizeof(int), hipHostMallocMapped) != hipSuccess || !h->host_err)
                { h->host_err = nullptr; return fail(DESIRE_ERR_HIP, "hipHostMalloc failed for the bin-split error word"); }
            *h->host_err = 0;
        }
        if (*static_cast<volatile int*>(h->host_err)) {
            *h->host_err = 0;
            return fail(DESIRE_ERR_HIP, "bin-split IOC hand-off timed out in an earlier call (workgroups of a tile were not co-resident)");
        }
        // (a fill KERNEL, not hipMemsetAsync: memset nodes of a captured graph were seen to run out of order on replay -- section 6a --
        //  and a counter that still holds the previous pass's arrivals lets every member read its peers' slots before they are written)
        launch_fill_f32(W(h, "cnt_s"), tiles, 0.f, s);
        a.hex = W(h, "hex_s"); a.grp_cnt = Wt<int>(h, "cnt_s"); a.err = h->host_err;
        a.nspl = p.nspl;
    }
#ifdef DESIRE_IOC_TIMING
    if (int rc = ws_ensure(h, {{"dbg", 10 * sizeof(long long)}})) return rc;
    a.dbg = Wt<long long>(h, "dbg");
#endif
    // training-mode forward: one launch per refinement pass, each keeping its own activations and the positions it ran on (the pass's input is
    // DETACHED where it enters the features -- cells, bins, velocity embedding -- and Y_p = Y_{p-1} + dY_p carries the gradient: DESIGN.md section 8)
    const int passes = h->training ? d.iters : 1;
    if (h->training) a.iters = 1;
    for (int it = 0; it < passes; ++it) {
        if (h->training) {
            const size_t po = ioc_save_off(h, it, v);         // a pass's saves (rows + slack), a view's at its row offset
            launch_copy_f32(W(h, "ioc_Yin") + po * 2, v.Y, (size_t)v.R * d.T_pred * 2, s);
            a.sv_x = W(h, "ioc_sv_x") + po * h->E; a.sv_r = W(h, "ioc_sv_r") + po * d.H; a.sv_u = W(h, "ioc_sv_u") + po * d.H;
            a.sv_c = W(h, "ioc_sv_c") + po * d.H; a.sv_h = W(h, "ioc_sv_h") + po * d.H;
            if (p.cluster() && it > 0) { if (int rc = ioc_cluster_exchange(h, (size_t)v.R / v.mno, false, s)) return rc; }
        }
        Timer t(h, s, "ioc");
        switch (p.fwd) {
            case IocFwd::FP32: case IocFwd::FP32_WIDE: launch_ioc(a, p.fwd == IocFwd::FP32_WIDE, s); break;
            case IocFwd::FP32_CLUSTER: launch_ioc_cluster(a, s); break;
            case IocFwd::BF16: case IocFwd::BF16_WIDE: launch_ioc_bf16(a, p.fwd == IocFwd::BF16_WIDE, s); break;
            case IocFwd::BF16_CLUSTER: if (launch_ioc_bf16_cluster(a, s)) return fail(DESIRE_ERR_HIP, "bf16 cluster IOC: no resident grid for this shape"); break;
            case IocFwd::X3: launch_ioc_x3(a, s); break;
            case IocFwd::X3R2: launch_ioc_x3r2(a, s); break;
            case IocFwd::X6: launch_ioc_x6(a, s); break;
            case IocFwd::X6R2: launch_ioc_x6r2(a, s); break;
            case IocFwd::STEPWISE: return fail(DESIRE_ERR_STATE, "the step-wise IOC has no view form");
        }
    }
#ifdef DESIRE_IOC_TIMING
    const char* n32[9] = {"P0 pos+clear", "P1 ev/es/masks", "build0+bar", "build(b+1)", "mma bin", "bin barrier", "P3 e_r+bar", "P4 gates(2 mma)+ep+2bar", "P5 cand+ep+2bar"};
    const char* n16[9] = {"loop top", "P1 ev/es/masks", "barrier 1", "P2 pooling chain + e_r", "barrier 2", "P4 gates + r*h", "barrier 3", "P5 cand + publish", "barrier 4"};
    const char* nx3[10] = {"step top (bar 4 wait)", "P1 ev/es/masks", "barrier 1", "P2 pooling chain", "exchange + e_r", "barrier 2", "P4 gates + r*h", "barrier 3", "P5 cand + publish", "barrier 4"};
    const char* ncl[10] = {"step top: positions + clear + bar", "P1 ev/es/masks", "wait for the peers", "copy peers' Ht + bar", "P2 pooling chains",
                           "exchange + e_r", "barrier 2", "P4 gates + r*h + cand frags", "bar 3 + P5 cand + publish stores", "drain + arrive + bar"};
    const bool split = !p.fp32_weights() && d.bf16 != 1, cl16 = p.fwd == IocFwd::BF16_CLUSTER;
    ioc_timing_report(a.dbg, split ? nx3 : cl16 ? ncl : d.bf16 == 1 ? n16 : n32, split || cl16 ? 10 : 9, s);
#endif
    HIPCHK(hipGetLastError());
    return p.cluster() ? ioc_cluster_check(h, s, "IOC cluster") : DESIRE_OK;
}

extern "C" int desire_ioc_refine(desire_handle* h, float* dev_Yhat, float* dev_score, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!dev_Yhat || !dev_score) return fail(DESIRE_ERR_ARG, "null argument");
    if (h->d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat: the reference graph has no ranking/refinement module (model/model.py:312-313)");
    if (!h->grids_set) return fail(DESIRE_ERR_STATE, "scene grids not set (desire_set_scene_grids)");
    if (h->img_set && (h->training || h->img_stale)) {          // images attached: training runs the CNN every step (its saves feed the backward),
        if (int rc = scene_images_run(h, static_cast<hipStream_t>(stream))) return rc;       // inference when weights or images changed
    }
    const desire_dims& d = h->d;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ioc_plan(h).fwd == IocFwd::STEPWISE) {        // one launch of the agent-sharded kernel per step, a single rank (ioc_plan.h)
        if (h->training) return fail(DESIRE_ERR_STATE, "training supports up to 128 agents per scene");
        const size_t RH = (size_t)h->R * d.H;
        if (int rc = ws_ensure(h, {{"stw_h", 2 * RH * sizeof(float)}, {"stw_sc", (size_t)h->R * sizeof(float)}})) return rc;
        float* hb[2] = {W(h, "stw_h"), W(h, "stw_h") + RH};
        const int NTs = d.H / 32, KXs = d.E_v + d.C + 2 * d.H;
        for (int it = 0; it < d.iters; ++it) {
            launch_hx_rows(hb[1], W(h, "HxHy"), 2 * d.H, d.n_scenes, d.K, d.mno, d.H, s);       // h_{-1} = Hx of the row's agent
            Timer tm(h, s, "ioc");                                                            // (one profile entry per pass, as for the persistent kernels)
            for (int t = 0; t < d.T_pred; ++t) {
                IocStepArgs q = ioc_step_args(h, t);
                q.rank = 0; q.nranks = 1;
                q.Yall = dev_Yhat; q.plast_all = W(h, "p_last"); q.valid_all = Wt<const uint8_t>(h, "valid"); q.Hall = hb[(t + 1) & 1];
                q.st_h = hb[(t + 1) & 1]; q.st_h_out = hb[t & 1]; q.st_score = W(h, "stw_sc");
                if (d.bf16 == 2 || d.bf16 == 3) {
                    q.np = d.bf16 == 3 ? 3 : 2;
                    q.Wsoc = D4(h, "ioc/Wsoc16l"); q.Wg = D4(h, "ioc/Wg16"); q.Wc = D4(h, "ioc/Wc16");
                    q.plo_soc = (size_t)d.grid_size * d.grid_size * NTs * (d.H / 16) * 64; q.plo_g = (size_t)2 * NTs * (KXs / 16) * 64; q.plo_c = (size_t)NTs * (KXs / 16) * 64;
                }
                launch_ioc_step(q, s);
            }
            if (int rc = desire_ioc_finish(h, hb[(d.T_pred - 1) & 1], W(h, "stw_sc"), dev_Yhat, dev_score, stream)) return rc;
        }
        HIPCHK(hipGetLastError());
        return DESIRE_OK;
    }
    if (compact_ioc(h)) {
        // DESIRE_FLAG_COMPACT_IOC: one launch sequence per slot class over the windows seated in it; windows without a present agent are not run
        // (their rows keep the Y they came with and score 0)
        if (int rc = compact_wait(h, s)) return rc;
        // device-side counts: every class is launched for the worst case (all windows in it) at a static offset; an empty class's grids exit
        const bool pad = ioc_plan(h).padded, dyn = compact_dyn(h);
        int cnt[4] = {0, 0, 0, 0};
        for (int c = 0, n = class_layout(h, pad, nullptr).n; c < n; ++c) {
            cnt[c] = dyn ? d.n_scenes : static_cast<volatile const int32_t*>(h->cp_host + 4)[c];
            if (cnt[c] < 0 || cnt[c] > d.n_scenes) return fail(DESIRE_ERR_HIP, "slot-class scan returned a count out of range");
        }
        const ClassLayout L = class_layout(h, pad, cnt);
        const int T2 = d.T_pred * 2;
        launch_fill_f32(dev_score, (size_t)h->R, 0.f, s);
        for (int c = 0; c < 4; ++c) h->ci_cnt[c] = c < L.n ? L.c[c].n_scenes : 0;
        for (int c = 0; c < L.n; ++c) {
            if (L.c[c].n_scenes == 0) continue;
            IocView v = ioc_view(h, &L.c[c]);
            if (dyn) v.dynN = Wt<const int32_t>(h, "cp_count") + 4 + c;
            {
                Timer t(h, s, "ioc_repack");
                launch_cls_gather_agents(W(h, "HxHy"), 2 * d.H, W(h, "p_last"), Wt<const int32_t>(h, "grid_of_scene"), v.cmap, v.win, v.n_scenes, v.mno,
                                         v.Hx, v.p_last, v.valid, v.gos, s, v.dynN);
                launch_cls_rows(dev_Yhat, v.Y, v.cmap, v.n_scenes, v.mno, d.K, d.mno, T2, 0, s, v.gpt, v.dynN);
            }
            if (int rc = ioc_core(h, v, s)) return rc;
            {
                Timer t(h, s, "ioc_repack");
                launch_cls_rows(dev_Yhat, v.Y, v.cmap, v.n_scenes, v.mno, d.K, d.mno, T2, 1, s, v.gpt, v.dynN);
                launch_cls_rows(dev_score, v.score, v.cmap, v.n_scenes, v.mno, d.K, d.mno, 1, 1, s, v.gpt, v.dynN);
            }
        }
        h->ci_last = true;
    } else {
        h->ci_last = false;
        IocView full = ioc_view(h); full.Y = dev_Yhat; full.score = dev_score;
        if (int rc = ioc_core(h, full, s)) return rc;
    }
    if (h->training && d.bf16 != 1) {
        launch_copy_f32(W(h, "Y_ref"), dev_Yhat, (size_t)h->R * d.T_pred * 2, s);
        launch_copy_f32(W(h, "score_sv"), dev_score, (size_t)h->R, s);
    }
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_forward(desire_handle* h, const float* dev_past, const float* dev_fut, const float* dev_eps,
                              float* dev_Yhat, float* dev_score, void* stream) {
    if (int rc = desire_encode(h, dev_past, dev_fut, stream)) return rc;
    if (int rc = desire_sample(h, dev_eps, dev_Yhat, stream)) return rc;
    if (h && h->d.ref_compat) return DESIRE_OK;          // the reference graph ends at the decoder states (dev_score untouched)
    return desire_ioc_refine(h, dev_Yhat, dev_score, stream);
}

