// api_eval.hip -- the evaluation ops of the ABI over the sample tensor Y [R, T_pred, 2]: ranking and ranked errors, KDE, the two selections, joint
// metrics, plan risk (plain and conditioned), the two mode fits, occupancy, the reconstruction weights.  Host code only: each entry point checks its
// arguments in the order its contract states (include/desire_hip.h; tests/eval_refusal_cases.py pins it), fills the argument blocks of kernels.h by
// field name and launches.
#include "ctx.h"

#include <cmath>
#include <string>

namespace {
// ---- the blocks every launcher takes: the handle's shape and normalisation with the call's pointers and unit ----
EvalIn eval_in(const desire_ctx* h, const float* Y, const float* fut, const uint8_t* present, const float* score) {
    EvalIn in{}; in.Y = Y; in.fut = fut; in.present = present; in.score = score;
    in.n_scenes = h->d.n_scenes; in.mno = h->d.mno; in.K = h->d.K; in.T = h->d.T_pred;
    return in;
}
EvalScale eval_scale(const desire_ctx* h, float unit_x = 1.f, float unit_y = 1.f) {      // (no unit: the op reads sx, sy alone)
    EvalScale sc{};
    sc.sx = h->d.sx; sc.sy = h->d.sy; sc.ux = unit_x; sc.uy = unit_y;
    return sc;
}

// ---- argument checks that the entry points share (each call keeps its own order of checks) ----
// the horizon list: 1..8 frame counts, each 1..T_pred, strictly increasing
int parse_horizons(const int32_t* host_horizons, int32_t n_h, int T_pred, RankHz* hz) {
    if (n_h < 1 || n_h > 8) return fail(DESIRE_ERR_ARG, "n_h must be 1..8");
    hz->n = n_h;
    for (int i = 0; i < n_h; ++i) {
        hz->h[i] = host_horizons[i];
        if (hz->h[i] < 1 || hz->h[i] > T_pred) return fail(DESIRE_ERR_ARG, "host_horizons[" + std::to_string(i) + "] must be 1..T_pred");
        if (i && hz->h[i] <= hz->h[i - 1]) return fail(DESIRE_ERR_ARG, "host_horizons must be strictly increasing");
    }
    return DESIRE_OK;
}
int check_units(float unit_x, float unit_y) {
    if (!std::isfinite(unit_x) || !(unit_x > 0.f)) return fail(DESIRE_ERR_ARG, "unit_x must be finite and > 0");
    if (!std::isfinite(unit_y) || !(unit_y > 0.f)) return fail(DESIRE_ERR_ARG, "unit_y must be finite and > 0");
    return DESIRE_OK;
}
int check_radius(float radius) {
    if (!std::isfinite(radius) || radius < 0.f) return fail(DESIRE_ERR_ARG, "radius must be finite and >= 0");
    return DESIRE_OK;
}
// exactly one of dev_fut / dev_present says what is counted
int check_counted(const float* dev_fut, const uint8_t* dev_present) {
    if (dev_fut && dev_present) return fail(DESIRE_ERR_ARG, "dev_fut and dev_present are both given: exactly one of them says what is counted");
    if (!dev_fut && !dev_present) return fail(DESIRE_ERR_ARG, "dev_fut and dev_present are both NULL: exactly one of them says what is counted");
    return DESIRE_OK;
}
// what desire_fit_modes and desire_fit_scene_modes check alike, in their order: the checks that need no handle come first, so a caller's
// constants can be validated before a handle exists.  order_name is the call's name of dev_order, `fitted` what it fits; p (filled by the
// caller from its arguments) gets the handle's sx, sy and, with dev_fut, the horizons
int check_fit_modes_args(const desire_handle* h, const float* dev_Yhat, const int32_t* dev_order, const char* order_name, const char* fitted,
                         const float* dev_fut, const int32_t* host_horizons, int32_t n_h, const ModesFitOut& o, ModesFitParams* p) {
    const std::string n_modes = "n_modes must be 1..min(K, " + std::to_string(DESIRE_MODES_MAX) + ")";
    if (p->n < 1 || p->n > DESIRE_MODES_MAX) return fail(DESIRE_ERR_ARG, n_modes);
    if (p->t_end < 1) return fail(DESIRE_ERR_ARG, "t_end must be 1..T_pred");
    if (p->iters < 0 || p->iters > DESIRE_MODES_MAX_ITERS) return fail(DESIRE_ERR_ARG, "iters must be 0.." + std::to_string(DESIRE_MODES_MAX_ITERS));
    if (int rc = check_units(p->ux, p->uy)) return rc;
    if (!std::isfinite(p->var_floor) || p->var_floor < 0.f) return fail(DESIRE_ERR_ARG, "var_floor must be finite and >= 0");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_order) return fail(DESIRE_ERR_ARG, std::string(order_name) + " is NULL");
    if (!o.count) return fail(DESIRE_ERR_ARG, "dev_count is NULL");
    if (!o.prob) return fail(DESIRE_ERR_ARG, "dev_prob is NULL");
    if (!dev_fut && o.out) return fail(DESIRE_ERR_ARG, "dev_out needs dev_fut (the likelihood is that of the ground truth)");
    if (!dev_fut && o.frame) return fail(DESIRE_ERR_ARG, "dev_frame needs dev_fut (the likelihood is that of the ground truth)");
    if (dev_fut && !o.out) return fail(DESIRE_ERR_ARG, "dev_out is NULL (dev_fut asks for the likelihood)");
    if (dev_fut && !host_horizons) return fail(DESIRE_ERR_ARG, "host_horizons is NULL");
    if (dev_fut && !std::isfinite(p->log_floor)) return fail(DESIRE_ERR_ARG, "log_floor must be finite");
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to fit " + std::string(fitted) + " to");
    if (p->n > d.K) return fail(DESIRE_ERR_ARG, n_modes);
    if (p->t_end > d.T_pred) return fail(DESIRE_ERR_ARG, "t_end must be 1..T_pred");
    p->sx = d.sx; p->sy = d.sy;
    return dev_fut ? parse_horizons(host_horizons, n_h, d.T_pred, &p->hz) : DESIRE_OK;
}
// where desire_plan_risk and desire_plan_risk_cond end alike: the horizons, the radius, the unit, then the LDS plans of the kernels that run -- the
// walk's, and with t_cond > 0 the conditioning kernel's -- and the grid of the one with the fewest plans per chunk
int check_plan_tail(const desire_dims& d, const int32_t* host_horizons, int32_t n_h, float radius, float unit_x, float unit_y, int M, int t_cond,
                    RankHz* hz) {
    if (int rc = parse_horizons(host_horizons, n_h, d.T_pred, hz)) return rc;
    if (int rc = check_radius(radius)) return rc;
    if (int rc = check_units(unit_x, unit_y)) return rc;
    int pc = 0, tc = 0, cpc = 0, ctc = 1, rows = 0;
    plan_geometry(d.mno, d.T_pred, M, &pc, &tc);
    if (t_cond) plan_cond_geometry(d.K, t_cond, M, &cpc, &ctc, &rows);
    if (tc < 1 || ctc < 1)                                                                                 // (not reachable at mno <= 256)
        return fail(DESIRE_ERR_ARG, t_cond ? "one frame of the window does not fit the plan kernels' LDS" : "one frame of the window does not fit the plan kernel's LDS");
    const int least = t_cond && cpc < pc ? cpc : pc;
    if ((uint64_t)d.n_scenes * (uint64_t)((M + least - 1) / least) >= (1ull << 31)) return fail(DESIRE_ERR_ARG, "n_scenes * plan chunks must be below 2^31");
    return DESIRE_OK;
}
}  // namespace

// ---- ranking by IOC score (kernels_rank.hip): the order of every agent's K samples, the n_top best rows, the errors of the paper's protocol ----
extern "C" int desire_rank_samples(desire_handle* h, const float* dev_score, const float* dev_Yhat, int32_t n_top, int32_t* dev_order,
                                   float* dev_top_Y, float* dev_top_score, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_score) return fail(DESIRE_ERR_ARG, "dev_score is NULL");
    if (!dev_order) return fail(DESIRE_ERR_ARG, "dev_order is NULL");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no IOC score to rank by");
    if (n_top < 1 || n_top > d.K) return fail(DESIRE_ERR_ARG, "n_top must be 1..K");
    if (dev_top_Y && !dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL (dev_top_Y is gathered from it)");
    if (d.K > RANK_MAX_K) return fail(DESIRE_ERR_ARG, "K above " + std::to_string(RANK_MAX_K) + " is not ranked on the device");
    RankOut o{}; o.order = dev_order; o.top_Y = dev_top_Y; o.top_score = dev_top_score;
    launch_rank_select(eval_in(h, dev_Yhat, nullptr, nullptr, dev_score), n_top, o, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_ranked_errors(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const int32_t* dev_order, int32_t n_top,
                                    const int32_t* host_horizons, int32_t n_h, float unit_x, float unit_y, float* dev_out, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_fut) return fail(DESIRE_ERR_ARG, "dev_fut is NULL");
    if (!dev_order) return fail(DESIRE_ERR_ARG, "dev_order is NULL");
    if (!host_horizons) return fail(DESIRE_ERR_ARG, "host_horizons is NULL");
    if (!dev_out) return fail(DESIRE_ERR_ARG, "dev_out is NULL");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no IOC score to rank by");
    if (n_top < 1 || n_top > d.K) return fail(DESIRE_ERR_ARG, "n_top must be 1..K");
    RankHz hz{};
    if (int rc = parse_horizons(host_horizons, n_h, d.T_pred, &hz)) return rc;
    int sc = 0, kc = 0;
    if (!sample_errors_geometry(d.mno, d.K, d.T_pred, &sc, &kc)) return fail(DESIRE_ERR_ARG, "T_pred is too long for the error kernel's LDS");
    ErrOut o{}; o.out = dev_out; o.tab = W(h, "rank_tab"); o.cnt = Wt<int32_t>(h, "rank_cnt");
    launch_ranked_errors(eval_in(h, dev_Yhat, dev_fut, nullptr, nullptr), dev_order, n_top, hz, eval_scale(h, unit_x, unit_y), o,
                         static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- KDE log-likelihood of the ground truth under the K samples (kernels_kde.hip): the contract is stated in include/desire_hip.h ----
extern "C" int desire_kde_nll(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const float* dev_score, const int32_t* host_horizons,
                              int32_t n_h, float unit_x, float unit_y, float log_floor, float* dev_out, float* dev_frame, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_fut) return fail(DESIRE_ERR_ARG, "dev_fut is NULL");
    if (!host_horizons) return fail(DESIRE_ERR_ARG, "host_horizons is NULL");
    if (!dev_out) return fail(DESIRE_ERR_ARG, "dev_out is NULL");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to fit a density to");
    RankHz hz{};
    if (int rc = parse_horizons(host_horizons, n_h, d.T_pred, &hz)) return rc;
    if (int rc = check_units(unit_x, unit_y)) return rc;
    if (!std::isfinite(log_floor)) return fail(DESIRE_ERR_ARG, "log_floor must be finite");
    int sa = 0;
    if (!kde_geometry(d.T_pred, &sa)) return fail(DESIRE_ERR_ARG, "T_pred is too long for the KDE kernel's LDS");
    KdeOut o{}; o.out = dev_out; o.frame = dev_frame; o.w = W(h, "kde_w"); o.st = W(h, "kde_st");
    launch_kde_nll(eval_in(h, dev_Yhat, dev_fut, nullptr, dev_score), hz, eval_scale(h, unit_x, unit_y), log_floor, o, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- score-ordered non-maximum suppression of the K samples (kernels_select.hip): the contract is stated in include/desire_hip.h.  The checks
// that need no handle come first, so a caller's constants can be validated before a handle exists. ----
extern "C" int desire_select_diverse(desire_handle* h, const float* dev_Yhat, const int32_t* dev_order, const float* dev_score, int32_t metric,
                                     int32_t t_end, float radius, float unit_x, float unit_y, int32_t n_top, int32_t* dev_order_out,
                                     int32_t* dev_count, float* dev_mass, float* dev_top_Y, float* dev_top_score, void* stream) {
    if (metric < DESIRE_DIST_FINAL || metric > DESIRE_DIST_MAX) return fail(DESIRE_ERR_ARG, "metric must be DESIRE_DIST_FINAL, _MEAN or _MAX (0..2)");
    if (int rc = check_radius(radius)) return rc;
    if (int rc = check_units(unit_x, unit_y)) return rc;
    if (t_end < 1) return fail(DESIRE_ERR_ARG, "t_end must be 1..T_pred");
    if (n_top < 1) return fail(DESIRE_ERR_ARG, "n_top must be 1..K");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_order) return fail(DESIRE_ERR_ARG, "dev_order is NULL");
    if (!dev_order_out) return fail(DESIRE_ERR_ARG, "dev_order_out is NULL");
    if (!dev_count) return fail(DESIRE_ERR_ARG, "dev_count is NULL");
    if (dev_top_score && !dev_score) return fail(DESIRE_ERR_ARG, "dev_score is NULL (dev_top_score is gathered from it)");
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to select from");
    if (t_end > d.T_pred) return fail(DESIRE_ERR_ARG, "t_end must be 1..T_pred");
    if (n_top > d.K) return fail(DESIRE_ERR_ARG, "n_top must be 1..K");
    int sc = 0, g = 0;
    if (!select_geometry(d.mno, d.K, metric, t_end, &sc, &g))
        return fail(DESIRE_ERR_ARG, "K samples of t_end frames do not fit the selection kernel's LDS: K * (" + std::to_string(EVAL_PAIR_BYTES) +
                                        " * (frames | 1) + " + std::to_string(4 * SelLds::K_WORDS) + ") + " + std::to_string(4 * SelLds::SLOT_WORDS) +
                                        " must be <= " + std::to_string(EVAL_LDS_BYTES));
    SelectParams p{}; p.order = dev_order; p.metric = metric; p.t_end = t_end; p.n_top = n_top; p.radius = radius;
    SelectOut o{}; o.order_out = dev_order_out; o.count = dev_count; o.mass = dev_mass; o.top_Y = dev_top_Y; o.top_score = dev_top_score;
    launch_select_diverse(eval_in(h, dev_Yhat, nullptr, nullptr, dev_score), p, eval_scale(h, unit_x, unit_y), o, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- the K samples of a window as K joint futures (kernels_joint.hip): the contract is stated in include/desire_hip.h ----
extern "C" int desire_joint_metrics(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const uint8_t* dev_present,
                                    const float* dev_score, const int32_t* host_horizons, int32_t n_h, int32_t n_top, float radius, float unit_x,
                                    float unit_y, int32_t* dev_first, int32_t* dev_cnt, float* dev_jerr, float* dev_jscore, int32_t* dev_jorder,
                                    float* dev_out, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_cnt) return fail(DESIRE_ERR_ARG, "dev_cnt is NULL");
    if (!dev_jorder) return fail(DESIRE_ERR_ARG, "dev_jorder is NULL");
    if (!host_horizons) return fail(DESIRE_ERR_ARG, "host_horizons is NULL");
    if (int rc = check_counted(dev_fut, dev_present)) return rc;
    if (!dev_fut && dev_jerr) return fail(DESIRE_ERR_ARG, "dev_jerr needs dev_fut (the errors are against the ground truth)");
    if (!dev_fut && dev_out) return fail(DESIRE_ERR_ARG, "dev_out needs dev_fut (the errors are against the ground truth)");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to read joint futures from");
    if (n_top < 1 || n_top > d.K) return fail(DESIRE_ERR_ARG, "n_top must be 1..K");
    RankHz hz{};
    if (int rc = parse_horizons(host_horizons, n_h, d.T_pred, &hz)) return rc;
    if (int rc = check_radius(radius)) return rc;
    if (int rc = check_units(unit_x, unit_y)) return rc;
    const bool errors = dev_jerr || dev_out;           // the per-agent table is desire_ranked_errors' own kernel's: its limit on T_pred comes with it
    int sc = 0, kc = 0;
    if (errors && !sample_errors_geometry(d.mno, d.K, d.T_pred, &sc, &kc))
        return fail(DESIRE_ERR_ARG, "dev_jerr / dev_out: T_pred is too long for the error kernel's LDS (desire_ranked_errors' limit)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EvalIn in = eval_in(h, dev_Yhat, dev_fut, dev_present, dev_score);
    const EvalScale scale = eval_scale(h, unit_x, unit_y);
    JointParams p{}; p.n_top = n_top; p.radius = radius;
    if (errors) {
        ErrOut t{}; t.tab = W(h, "rank_tab"); t.cnt = Wt<int32_t>(h, "rank_cnt");
        launch_sample_errors(in, hz, scale, t, s);
        p.tab = t.tab;
    }
    JointOut o{}; o.first = dev_first; o.cnt = dev_cnt; o.jorder = dev_jorder; o.out = dev_out;
    o.jerr = errors ? (dev_jerr ? dev_jerr : W(h, "joint_je")) : nullptr;
    o.jscore = dev_jscore ? dev_jscore : W(h, "joint_js");
    launch_joint_metrics(in, p, hz, scale, o, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- score-ordered non-maximum suppression of a window's K joint futures (kernels_worlds.hip): the contract is stated in include/desire_hip.h.
// As in desire_select_diverse the checks that need no handle come first. ----
extern "C" int desire_select_worlds(desire_handle* h, const float* dev_Yhat, const uint8_t* dev_present, const float* dev_wscore, int32_t metric,
                                    int32_t reduce, int32_t t_end, float radius, float unit_x, float unit_y, int32_t* dev_worder,
                                    int32_t* dev_wcount, float* dev_wmass, int32_t* dev_wlabel, void* stream) {
    if (metric < DESIRE_DIST_FINAL || metric > DESIRE_DIST_MAX) return fail(DESIRE_ERR_ARG, "metric must be DESIRE_DIST_FINAL, _MEAN or _MAX (0..2)");
    if (reduce != DESIRE_WORLD_ALL && reduce != DESIRE_WORLD_MEAN) return fail(DESIRE_ERR_ARG, "reduce must be DESIRE_WORLD_ALL or DESIRE_WORLD_MEAN (0, 1)");
    if (int rc = check_radius(radius)) return rc;
    if (int rc = check_units(unit_x, unit_y)) return rc;
    if (t_end < 1) return fail(DESIRE_ERR_ARG, "t_end must be 1..T_pred");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_worder) return fail(DESIRE_ERR_ARG, "dev_worder is NULL");
    if (!dev_wcount) return fail(DESIRE_ERR_ARG, "dev_wcount is NULL");
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to read joint futures from");
    if (t_end > d.T_pred) return fail(DESIRE_ERR_ARG, "t_end must be 1..T_pred");
    int sc = 0;
    if (!worlds_geometry(d.mno, d.K, metric, t_end, &sc))
        return fail(DESIRE_ERR_ARG, "K worlds of mno slots and t_end frames do not fit the world-selection kernel's LDS: " +
                                        std::to_string(4 * (WorldsLds::K_WORDS + 2)) + " * K + 4 * mno + " + std::to_string(EVAL_PAIR_BYTES) +
                                        " * (frames | 1) must be <= " + std::to_string(EVAL_LDS_BYTES));
    WorldsParams p{}; p.metric = metric; p.reduce = reduce; p.t_end = t_end; p.radius = radius;
    WorldsOut o{}; o.worder = dev_worder; o.wcount = dev_wcount; o.wmass = dev_wmass; o.wlabel = dev_wlabel;
    launch_select_worlds(eval_in(h, dev_Yhat, nullptr, dev_present, dev_wscore), p, eval_scale(h, unit_x, unit_y), o, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- candidate ego plans against the K joint futures (kernels_plan.hip): the contract is stated in include/desire_hip.h ----
extern "C" int desire_plan_risk(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const uint8_t* dev_present, const float* dev_score,
                                const float* dev_plans, const int32_t* dev_ego, int32_t M, const int32_t* host_horizons, int32_t n_h, float radius,
                                float unit_x, float unit_y, int32_t* dev_first, float* dev_clear, float* dev_risk, float* dev_blame, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_plans) return fail(DESIRE_ERR_ARG, "dev_plans is NULL");
    if (!dev_risk) return fail(DESIRE_ERR_ARG, "dev_risk is NULL");
    if (!host_horizons) return fail(DESIRE_ERR_ARG, "host_horizons is NULL");
    if (int rc = check_counted(dev_fut, dev_present)) return rc;
    if (M < 1) return fail(DESIRE_ERR_ARG, "M must be at least 1 (the candidate plans per window)");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to read joint futures from");
    RankHz hz{};
    if (int rc = check_plan_tail(d, host_horizons, n_h, radius, unit_x, unit_y, M, 0, &hz)) return rc;
    PlanIn pl{}; pl.plans = dev_plans; pl.ego = dev_ego; pl.M = M;
    PlanOut o{}; o.first = dev_first; o.clear = dev_clear; o.risk = dev_risk; o.blame = dev_blame; o.w = W(h, "joint_js");
    launch_plan_risk(eval_in(h, dev_Yhat, dev_fut, dev_present, dev_score), pl, hz, eval_scale(h, unit_x, unit_y), radius, o,
                     static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- the same against the K joint futures reweighted by their agreement with each plan (kernels_plan_cond.hip, then kernels_plan.hip's walk
// reading dev_cw): the contract is stated in include/desire_hip.h.  The window's weights live in "joint_js" as in desire_plan_risk, its logits
// p_k in the first n_scenes * K floats of "joint_je"; nothing grows with M but the caller's own dev_cw. ----
extern "C" int desire_plan_risk_cond(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const uint8_t* dev_present,
                                     const float* dev_score, const float* dev_plans, const int32_t* dev_ego, int32_t M,
                                     const int32_t* host_horizons, int32_t n_h, float radius, float unit_x, float unit_y, float sigma, int32_t t_cond,
                                     int32_t* dev_first, float* dev_clear, float* dev_risk, float* dev_blame, float* dev_cw, float* dev_dist,
                                     float* dev_ess, float* dev_support, int32_t* dev_cond, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_plans) return fail(DESIRE_ERR_ARG, "dev_plans is NULL");
    if (!dev_risk) return fail(DESIRE_ERR_ARG, "dev_risk is NULL");
    if (!dev_cw) return fail(DESIRE_ERR_ARG, "dev_cw is NULL (the [n_scenes, M, K] weight table the risk is summed from)");
    if (!host_horizons) return fail(DESIRE_ERR_ARG, "host_horizons is NULL");
    if (int rc = check_counted(dev_fut, dev_present)) return rc;
    if (M < 1) return fail(DESIRE_ERR_ARG, "M must be at least 1 (the candidate plans per window)");
    if (!std::isfinite(sigma) || !(sigma > 0.f)) return fail(DESIRE_ERR_ARG, "sigma must be finite and > 0");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to read joint futures from");
    if (t_cond < 1 || t_cond > d.T_pred) return fail(DESIRE_ERR_ARG, "t_cond must be 1..T_pred");
    RankHz hz{};
    if (int rc = check_plan_tail(d, host_horizons, n_h, radius, unit_x, unit_y, M, t_cond, &hz)) return rc;
    const volatile float two_s = 2.f * sigma, two_s2 = two_s * sigma;  // fp32, every operation rounded once (2 * sigma is exact)
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EvalIn in = eval_in(h, dev_Yhat, dev_fut, dev_present, dev_score);
    const EvalScale scale = eval_scale(h, unit_x, unit_y);
    PlanIn pl{}; pl.plans = dev_plans; pl.ego = dev_ego; pl.M = M;
    PlanPriorOut pr{}; pr.w = W(h, "joint_js"); pr.prior = W(h, "joint_je");
    launch_plan_prior(in, pr, s);
    PlanCondParams p{}; p.w = pr.w; p.prior = pr.prior; p.t_cond = t_cond; p.inv = 1.f / two_s2;
    PlanCondOut c{}; c.cw = dev_cw; c.dist = dev_dist; c.ess = dev_ess; c.support = dev_support; c.cond = dev_cond;
    launch_plan_cond_weights(in, pl, p, scale, c, s);
    PlanOut o{}; o.first = dev_first; o.clear = dev_clear; o.risk = dev_risk; o.blame = dev_blame;
    launch_plan_risk_per_plan(in, pl, dev_cw, hz, scale, radius, o, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- n modes with covariances fitted to the K samples (kernels_modes.hip): the contract is stated in include/desire_hip.h.  As in
// desire_select_diverse the checks that need no handle come first. ----
extern "C" int desire_fit_modes(desire_handle* h, const float* dev_Yhat, const int32_t* dev_order, const float* dev_score, const float* dev_fut,
                                int32_t n_modes, int32_t t_end, int32_t iters, float unit_x, float unit_y, float var_floor,
                                const int32_t* host_horizons, int32_t n_h, float log_floor, int32_t* dev_label, int32_t* dev_count, float* dev_prob,
                                float* dev_mean, float* dev_cov, int32_t* dev_passes, float* dev_out, float* dev_frame, void* stream) {
    const ModesFitOut o{dev_label, dev_count, dev_prob, dev_mean, dev_cov, dev_passes, dev_out, dev_frame};
    ModesFitParams p{n_modes, t_end, iters, unit_x, unit_y, 0.f, 0.f, var_floor, log_floor, RankHz{}};
    if (int rc = check_fit_modes_args(h, dev_Yhat, dev_order, "dev_order", "modes", dev_fut, host_horizons, n_h, o, &p)) return rc;
    const desire_dims& d = h->d;
    int sc = 0, g = 0;
    if (!modes_geometry(d.mno, d.K, d.T_pred, n_modes, &sc, &g))
        return fail(DESIRE_ERR_ARG, "K samples and n_modes means of T_pred frames do not fit the mode kernel's LDS: " + std::to_string(EVAL_PAIR_BYTES) +
                                        " * (K + n_modes) * (T_pred | 1) + 12 * n_modes * T_pred + " + std::to_string(4 * ModesLds::FRAME_WORDS) +
                                        " * (T_pred | 1) + " + std::to_string(4 * ModesLds::K_WORDS) + " * K + " +
                                        std::to_string(4 * ModesLds::MODE_WORDS) + " * n_modes + " + std::to_string(4 * ModesLds::SLOT_WORDS) +
                                        " must be <= " + std::to_string(EVAL_LDS_BYTES));
    if ((uint64_t)d.n_scenes * (uint64_t)((d.mno + sc - 1) / sc) >= (1ull << 31)) return fail(DESIRE_ERR_ARG, "n_scenes * slot chunks must be below 2^31");
    launch_fit_modes(eval_in(h, dev_Yhat, dev_fut, nullptr, dev_score), dev_order, o, p, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- n scene modes with covariances fitted to a window's K joint futures (kernels_scene_modes.hip): the contract is stated in
// include/desire_hip.h.  As in desire_fit_modes the checks that need no handle come first. ----
extern "C" int desire_fit_scene_modes(desire_handle* h, const float* dev_Yhat, const uint8_t* dev_present, const int32_t* dev_worder,
                                      const float* dev_wscore, const float* dev_fut, int32_t n_modes, int32_t t_end, int32_t iters, float unit_x,
                                      float unit_y, float var_floor, const int32_t* host_horizons, int32_t n_h, float log_floor, int32_t* dev_label,
                                      int32_t* dev_count, float* dev_prob, float* dev_mean, float* dev_cov, int32_t* dev_passes, float* dev_out,
                                      float* dev_frame, void* stream) {
    const ModesFitOut o{dev_label, dev_count, dev_prob, dev_mean, dev_cov, dev_passes, dev_out, dev_frame};
    ModesFitParams p{n_modes, t_end, iters, unit_x, unit_y, 0.f, 0.f, var_floor, log_floor, RankHz{}};
    if (int rc = check_fit_modes_args(h, dev_Yhat, dev_worder, "dev_worder", "scene modes", dev_fut, host_horizons, n_h, o, &p)) return rc;
    const desire_dims& d = h->d;
    int sc = 0;
    if (!scene_modes_geometry(d.mno, d.K, d.T_pred, n_modes, &sc))
        return fail(DESIRE_ERR_ARG, "K worlds and n_modes means of one slot's T_pred frames do not fit the scene-mode kernel's LDS: " +
                                        std::to_string(EVAL_PAIR_BYTES) + " * (K + n_modes) * (T_pred | 1) + " +
                                        std::to_string(4 * (SceneModesLds::TERM_WORDS + SceneModesLds::FRAME_WORDS)) + " * n_modes * T_pred + 12 * K * n_modes + " +
                                        std::to_string(4 * SceneModesLds::K_WORDS) + " * K + " + std::to_string(4 * SceneModesLds::MODE_WORDS) +
                                        " * n_modes + 4 * n_modes * ceil(K / 32) + " + std::to_string(4 * SceneModesLds::T_WORDS) +
                                        " * T_pred + 4 * mno must be <= " + std::to_string(EVAL_LDS_BYTES));
    launch_fit_scene_modes(eval_in(h, dev_Yhat, dev_fut, dev_present, dev_wscore), dev_worder, o, p, h->scene_modes_chunk, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- predicted occupancy maps of the K weighted samples (kernels_occ.hip): the contract is stated in include/desire_hip.h ----
extern "C" int desire_occupancy(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const uint8_t* dev_present, const float* dev_score,
                                const int32_t* host_horizons, int32_t n_h, int32_t mode, int32_t Oh, int32_t Ow, const uint8_t* dev_mask,
                                const int32_t* dev_mask_of_scene, float* dev_occ, float* dev_exp, float* dev_hit, float* dev_viol, float* dev_off,
                                void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!dev_occ) return fail(DESIRE_ERR_ARG, "dev_occ is NULL");
    if (!host_horizons) return fail(DESIRE_ERR_ARG, "host_horizons is NULL");
    if (mode != DESIRE_OCC_AT && mode != DESIRE_OCC_UNTIL) return fail(DESIRE_ERR_ARG, "mode must be DESIRE_OCC_AT or DESIRE_OCC_UNTIL (0, 1)");
    if (Oh < 1 || Oh > DESIRE_OCC_MAX_SIDE) return fail(DESIRE_ERR_ARG, "Oh must be 1.." + std::to_string(DESIRE_OCC_MAX_SIDE));
    if (Ow < 1 || Ow > DESIRE_OCC_MAX_SIDE) return fail(DESIRE_ERR_ARG, "Ow must be 1.." + std::to_string(DESIRE_OCC_MAX_SIDE));
    if (int rc = check_counted(dev_fut, dev_present)) return rc;
    if (dev_hit && !dev_fut) return fail(DESIRE_ERR_ARG, "dev_hit needs dev_fut (the cell of the ground truth)");
    if (dev_hit && mode != DESIRE_OCC_AT) return fail(DESIRE_ERR_ARG, "dev_hit is defined in mode DESIRE_OCC_AT only");
    if (dev_viol && (!dev_mask || !dev_mask_of_scene)) return fail(DESIRE_ERR_ARG, "dev_viol needs dev_mask and dev_mask_of_scene");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to read occupancy from");
    RankHz hz{};
    if (int rc = parse_horizons(host_horizons, n_h, d.T_pred, &hz)) return rc;
    if ((uint64_t)d.mno * (uint64_t)d.K >= (1ull << 32)) return fail(DESIRE_ERR_ARG, "mno * K must be below 2^32 (the stamps of the occupancy kernel)");
    int kc = 0, fc = 0, rows = 0;
    const int until = mode == DESIRE_OCC_UNTIL;
    if (!occupancy_geometry(d.K, until ? hz.h[hz.n - 1] : 1, Oh, Ow, until, &kc, &fc, &rows))
        return fail(DESIRE_ERR_ARG, "one grid row does not fit the occupancy kernel's LDS");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EvalIn in = eval_in(h, dev_Yhat, dev_fut, dev_present, dev_score);
    KdeOut k{}; k.w = W(h, "kde_w"); k.st = W(h, "kde_st");
    launch_kde_weights(in, k, s);
    OccParams p{};
    p.w = k.w; p.mask = dev_viol ? dev_mask : nullptr; p.mask_of_scene = dev_viol ? dev_mask_of_scene : nullptr; p.Oh = Oh; p.Ow = Ow; p.mode = mode;
    OccOut o{}; o.occ = dev_occ; o.exp = dev_exp; o.hit = dev_hit; o.viol = dev_viol; o.off = dev_off;
    launch_occupancy(in, p, hz, eval_scale(h), o, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- per-sample reconstruction errors and the weights of the best-of-many / soft-min loss (kernels_recon.hip): the contract is stated in
// include/desire_hip.h.  The training step (backward.hip: loss_grads) runs the same kernel into the same workspace tensors.  The scene scope: the K
// worlds of a window weighed by their mean error over the window's counted agents. ----
int recon_ws_setup(desire_ctx* h) {
    const size_t f = sizeof(float);
    return ws_ensure(h, {{"recon_e", (size_t)h->R * f}, {"recon_w", (size_t)h->R * f}, {"recon_win", (size_t)h->A * sizeof(int32_t)}, {"recon_val", (size_t)h->A * f}});
}
int recon_scene_ws_setup(desire_ctx* h) {
    if (int rc = recon_ws_setup(h)) return rc;
    return ws_ensure(h, {{"recon_E", (size_t)h->d.n_scenes * h->d.K * sizeof(float)}, {"recon_cnt", (size_t)h->d.n_scenes * sizeof(int32_t)}});
}

namespace {
// the launch of either scope: every output the caller did not give (o: its pointers, null = not wanted) goes to the workspace tensor of its name
// (tg: the names of those tensors; the stand-alone ops keep the Y0 side's)
void recon_weights_launch(desire_ctx* h, bool scene, const float* Y, const float* fut, const uint8_t* lmask, int mode, float tau, ReconOut o,
                          hipStream_t s, const ReconTarget& tg = RECON_Y0) {
    if (!o.e) o.e = W(h, tg.e);
    if (!o.w) o.w = W(h, tg.w);
    if (!o.winner) o.winner = Wt<int32_t>(h, tg.win);
    if (!o.recon) o.recon = W(h, tg.val);
    if (scene && !o.E) o.E = W(h, tg.E);
    if (scene && !o.count) o.count = Wt<int32_t>(h, tg.cnt);
    ReconParams p{}; p.lmask = lmask; p.nfut = W(h, "nfut"); p.mode = mode; p.tau = tau;
    (scene ? launch_recon_weights_scene : launch_recon_weights)(eval_in(h, Y, fut, nullptr, nullptr), p, eval_scale(h), o, s);
}
// desire_recon_weights and desire_recon_weights_scene: the same checks in the same order, then the scope's workspace and launches
int recon_weights_call(desire_handle* h, bool scene, const float* dev_fut, const float* dev_Yhat, int32_t mode, float tau, const ReconOut& o,
                       void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_fut) return fail(DESIRE_ERR_ARG, "dev_fut is NULL");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (mode < DESIRE_RECON_MEAN || mode > DESIRE_RECON_SOFTMIN) return fail(DESIRE_ERR_ARG, "mode must be DESIRE_RECON_MEAN, _MIN or _SOFTMIN (0..2)");
    if (mode == DESIRE_RECON_SOFTMIN && (!std::isfinite(tau) || !(tau > 0.f))) return fail(DESIRE_ERR_ARG, "tau must be finite and > 0 for DESIRE_RECON_SOFTMIN");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to take errors of");
    int sc = 0, kc = 0;
    if (!recon_geometry(d.mno, d.K, d.T_pred, &sc, &kc)) return fail(DESIRE_ERR_ARG, "T_pred is too long for the reconstruction-weight kernel's LDS");
    if (int rc = desire_ready(h)) return rc;
    if (int rc = scene ? recon_scene_ws_setup(h) : recon_ws_setup(h)) return rc;          // (the first call allocates; later calls are capturable)
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_loss_mask(Wt<const uint8_t>(h, "valid"), dev_fut, Wt<uint8_t>(h, "lmask"), W(h, "nfut"), d.n_scenes, d.mno, d.T_pred, s);
    recon_weights_launch(h, scene, dev_Yhat, dev_fut, Wt<const uint8_t>(h, "lmask"), mode, tau, o, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}
}  // namespace

// the training step's: the handle's mode and scope over the target's samples ("Y0", or the refined "Y_ref"), everything into the target's tensors
void recon_weights_enqueue(desire_ctx* h, const ReconTarget& tg, const float* fut, const uint8_t* lmask, hipStream_t s) {
    recon_weights_launch(h, h->recon_scope == DESIRE_RECON_SCOPE_SCENE, W(h, tg.Y), fut, lmask, h->recon_mode, h->recon_tau, ReconOut{}, s, tg);
}

// the refined side's tensors (desire_set_refined_loss).  No gradient tensor of its own: the terms add to "dYr", and the stand-alone ops keep theirs.
int refined_ws_setup(desire_ctx* h, bool recon, bool collision, bool offroad) {
    const size_t f = sizeof(float), A = h->A, K = h->d.K, n = h->d.n_scenes;
    if (recon) {          // both scopes: the scope is read at the time of the step and may change after the setter
        if (int rc = ws_ensure(h, {{"rrecon_e", (size_t)h->R * f}, {"rrecon_w", (size_t)h->R * f}, {"rrecon_win", A * sizeof(int32_t)}, {"rrecon_val", A * f},
                                   {"rrecon_E", n * K * f}, {"rrecon_cnt", n * sizeof(int32_t)}})) return rc;
    }
    if (collision) { if (int rc = ws_ensure(h, {{"rcol_val", A * K * f}, {"rcol_touch", n * K * sizeof(int32_t)}, {"rcol_term", f}, {"nvalid", 4 * f}})) return rc; }
    if (offroad) { if (int rc = ws_ensure(h, {{"roff_val", A * K * f}, {"roff_count", n * K * sizeof(int32_t)}, {"roff_term", f}, {"nvalid", 4 * f}})) return rc; }
    return DESIRE_OK;
}

extern "C" int desire_recon_weights(desire_handle* h, const float* dev_fut, const float* dev_Yhat, int32_t mode, float tau, float* dev_e,
                                    float* dev_w, int32_t* dev_winner, float* dev_recon, void* stream) {
    ReconOut o{}; o.e = dev_e; o.w = dev_w; o.winner = dev_winner; o.recon = dev_recon;
    return recon_weights_call(h, false, dev_fut, dev_Yhat, mode, tau, o, stream);
}

extern "C" int desire_recon_weights_scene(desire_handle* h, const float* dev_fut, const float* dev_Yhat, int32_t mode, float tau, float* dev_e,
                                          float* dev_E, int32_t* dev_count, float* dev_w, int32_t* dev_winner, float* dev_recon, void* stream) {
    ReconOut o{}; o.e = dev_e; o.E = dev_E; o.count = dev_count; o.w = dev_w; o.winner = dev_winner; o.recon = dev_recon;
    return recon_weights_call(h, true, dev_fut, dev_Yhat, mode, tau, o, stream);
}

// ---- the collision penalty of a window's K joint futures (kernels_collision.hip): the contract is stated in include/desire_hip.h.  The training
// step (backward.hip: loss_grads) runs the same kernel in its accumulating form on "dY0". ----
int collision_ws_setup(desire_ctx* h) {
    const size_t f = sizeof(float);
    return ws_ensure(h, {{"col_val", (size_t)h->A * h->d.K * f}, {"col_touch", (size_t)h->d.n_scenes * h->d.K * sizeof(int32_t)},
                         {"col_grad", (size_t)h->R * h->d.T_pred * 2 * f}, {"col_term", f}, {"nvalid", 4 * f}});
}
int check_collision_args(float radius, float unit_x, float unit_y) {
    if (int rc = check_radius(radius)) return rc;
    return check_units(unit_x, unit_y);
}
void collision_enqueue(desire_ctx* h, const TermTarget& tg, const float* fut, const uint8_t* lmask, hipStream_t s) {
    CollParams p{}; p.lmask = lmask; p.nfut = W(h, "nfut"); p.nvalid = W(h, "nvalid"); p.radius = h->col_radius; p.weight = tg.weight; p.accumulate = true;
    CollOut o{}; o.col = W(h, tg.val); o.touch = Wt<int32_t>(h, tg.count); o.dY = W(h, tg.dY); o.term = W(h, tg.term);
    launch_collision_loss(eval_in(h, W(h, tg.Y), fut, nullptr, nullptr), p, eval_scale(h, h->col_ux, h->col_uy), o, s);
}

extern "C" int desire_collision_loss(desire_handle* h, const float* dev_fut, const float* dev_Yhat, float radius, float unit_x, float unit_y,
                                     float* dev_col, int32_t* dev_touch, float* dev_dY, float* dev_term, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_fut) return fail(DESIRE_ERR_ARG, "dev_fut is NULL");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (int rc = check_collision_args(radius, unit_x, unit_y)) return rc;
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to read joint futures from");
    if (int rc = desire_ready(h)) return rc;
    if (int rc = collision_ws_setup(h)) return rc;          // (the first call allocates; later calls are capturable)
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_loss_mask(Wt<const uint8_t>(h, "valid"), dev_fut, Wt<uint8_t>(h, "lmask"), W(h, "nfut"), d.n_scenes, d.mno, d.T_pred, s);
    launch_count_valid(Wt<const uint8_t>(h, "lmask"), h->A, W(h, "nvalid"), s);
    CollParams p{}; p.lmask = Wt<const uint8_t>(h, "lmask"); p.nfut = W(h, "nfut"); p.nvalid = W(h, "nvalid"); p.radius = radius; p.weight = 1.f;
    CollOut o{}; o.col = dev_col ? dev_col : W(h, "col_val"); o.touch = dev_touch ? dev_touch : Wt<int32_t>(h, "col_touch");
    o.dY = dev_dY ? dev_dY : W(h, "col_grad"); o.term = dev_term ? dev_term : W(h, "col_term");
    launch_collision_loss(eval_in(h, dev_Yhat, dev_fut, nullptr, nullptr), p, eval_scale(h, unit_x, unit_y), o, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- the off-road penalty of a window's K joint futures against the distance field of its scene mask (kernels_offroad.hip): the contracts are
// stated in include/desire_hip.h.  The training step (backward.hip: loss_grads, ioc_bwd) runs the same kernel in its accumulating form on "dY0" / "dYr". ----
extern "C" int desire_mask_distance(desire_handle* h, const uint8_t* dev_mask, int32_t n_masks, int32_t Mh, int32_t Mw, float cell_x, float cell_y,
                                    float* dev_field, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_mask) return fail(DESIRE_ERR_ARG, "dev_mask is NULL");
    if (!dev_field) return fail(DESIRE_ERR_ARG, "dev_field is NULL");
    if (n_masks < 1 || n_masks > DESIRE_OFFROAD_MAX_MASKS) return fail(DESIRE_ERR_ARG, "n_masks must be 1.." + std::to_string(DESIRE_OFFROAD_MAX_MASKS));
    if (Mh < 1 || Mh > DESIRE_OCC_MAX_SIDE) return fail(DESIRE_ERR_ARG, "Mh must be 1.." + std::to_string(DESIRE_OCC_MAX_SIDE));
    if (Mw < 1 || Mw > DESIRE_OCC_MAX_SIDE) return fail(DESIRE_ERR_ARG, "Mw must be 1.." + std::to_string(DESIRE_OCC_MAX_SIDE));
    if (!std::isfinite(cell_x) || !(cell_x > 0.f)) return fail(DESIRE_ERR_ARG, "cell_x must be finite and > 0");
    if (!std::isfinite(cell_y) || !(cell_y > 0.f)) return fail(DESIRE_ERR_ARG, "cell_y must be finite and > 0");
    if (h->d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] for a field to be read against");
    launch_mask_distance(dev_mask, n_masks, Mh, Mw, cell_x, cell_y, dev_field, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_set_offroad_field(desire_handle* h, const float* dev_field, int32_t n_fields, int32_t Mh, int32_t Mw,
                                        const int32_t* host_field_of_scene) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_field) return fail(DESIRE_ERR_ARG, "dev_field is NULL");
    if (!host_field_of_scene) return fail(DESIRE_ERR_ARG, "host_field_of_scene is NULL");
    if (n_fields < 1 || n_fields > DESIRE_OFFROAD_MAX_MASKS) return fail(DESIRE_ERR_ARG, "n_fields must be 1.." + std::to_string(DESIRE_OFFROAD_MAX_MASKS));
    if (Mh < 1 || Mh > DESIRE_OCC_MAX_SIDE) return fail(DESIRE_ERR_ARG, "Mh must be 1.." + std::to_string(DESIRE_OCC_MAX_SIDE));
    if (Mw < 1 || Mw > DESIRE_OCC_MAX_SIDE) return fail(DESIRE_ERR_ARG, "Mw must be 1.." + std::to_string(DESIRE_OCC_MAX_SIDE));
    if (h->d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] for a field to be read against");
    for (int i = 0; i < h->d.n_scenes; ++i)
        if (host_field_of_scene[i] >= n_fields) return fail(DESIRE_ERR_ARG, "field_of_scene entry out of range (a negative entry: no field)");
    if (int rc = ws_ensure(h, {{"off_fos", (size_t)h->d.n_scenes * sizeof(int32_t)}})) return rc;
    HIPCHK(hipMemcpy(Wt<int32_t>(h, "off_fos"), host_field_of_scene, h->d.n_scenes * sizeof(int32_t), hipMemcpyHostToDevice));
    h->off_field = dev_field; h->off_n = n_fields; h->off_Mh = Mh; h->off_Mw = Mw;
    return DESIRE_OK;
}

int offroad_ws_setup(desire_ctx* h) {
    const size_t f = sizeof(float);
    return ws_ensure(h, {{"off_val", (size_t)h->A * h->d.K * f}, {"off_count", (size_t)h->d.n_scenes * h->d.K * sizeof(int32_t)},
                         {"off_grad", (size_t)h->R * h->d.T_pred * 2 * f}, {"off_term", f}, {"nvalid", 4 * f}});
}
namespace {
OffParams offroad_params(desire_ctx* h, const uint8_t* lmask, float scale, float weight, bool accumulate) {
    OffParams p{}; p.lmask = lmask; p.nfut = W(h, "nfut"); p.nvalid = W(h, "nvalid"); p.field = h->off_field;
    p.field_of_scene = Wt<const int32_t>(h, "off_fos"); p.Mh = h->off_Mh; p.Mw = h->off_Mw; p.scale = scale; p.weight = weight; p.accumulate = accumulate;
    return p;
}
}  // namespace
void offroad_enqueue(desire_ctx* h, const TermTarget& tg, const float* fut, const uint8_t* lmask, hipStream_t s) {
    OffOut o{}; o.off = W(h, tg.val); o.count = Wt<int32_t>(h, tg.count); o.dY = W(h, tg.dY); o.term = W(h, tg.term);
    launch_offroad_loss(eval_in(h, W(h, tg.Y), fut, nullptr, nullptr), offroad_params(h, lmask, h->off_scale, tg.weight, true), o, s);
}

extern "C" int desire_offroad_loss(desire_handle* h, const float* dev_fut, const float* dev_Yhat, float scale, float* dev_off, int32_t* dev_count,
                                   float* dev_dY, float* dev_term, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_fut) return fail(DESIRE_ERR_ARG, "dev_fut is NULL");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    if (!std::isfinite(scale) || !(scale > 0.f)) return fail(DESIRE_ERR_ARG, "scale must be finite and > 0");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to read joint futures from");
    if (!h->off_field) return fail(DESIRE_ERR_STATE, "no distance field set (desire_set_offroad_field)");
    if (int rc = desire_ready(h)) return rc;
    if (int rc = offroad_ws_setup(h)) return rc;            // (the first call allocates; later calls are capturable)
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_loss_mask(Wt<const uint8_t>(h, "valid"), dev_fut, Wt<uint8_t>(h, "lmask"), W(h, "nfut"), d.n_scenes, d.mno, d.T_pred, s);
    launch_count_valid(Wt<const uint8_t>(h, "lmask"), h->A, W(h, "nvalid"), s);
    OffOut o{}; o.off = dev_off ? dev_off : W(h, "off_val"); o.count = dev_count ? dev_count : Wt<int32_t>(h, "off_count");
    o.dY = dev_dY ? dev_dY : W(h, "off_grad"); o.term = dev_term ? dev_term : W(h, "off_term");
    launch_offroad_loss(eval_in(h, dev_Yhat, dev_fut, nullptr, nullptr), offroad_params(h, Wt<const uint8_t>(h, "lmask"), scale, 1.f, false), o, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}
