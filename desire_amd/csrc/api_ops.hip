// api_ops.hip -- the stand-alone ops of the ABI: integer paths, scene CNN, losses, the reference's literal tensors, window builder, Gaussian head,
// rollout, ADE / FDE.  Host code only; split out of api.hip in round 5.
#include "ctx.h"
#include "philox.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" int desire_neighbor_bins(desire_handle* h, const float* dev_pos, const uint8_t* dev_valid,
                                    int32_t* dev_bins, int32_t n_groups, void* stream) {
    if (!h || !dev_pos || !dev_valid || !dev_bins || n_groups < 0) return fail(DESIRE_ERR_ARG, "bad argument");
    if (n_groups == 0) return DESIRE_OK;
    launch_neighbor_bins(dev_pos, dev_valid, dev_bins, n_groups, h->d.mno, h->d.nb_w, h->d.nb_h, h->d.grid_size,
                         h->d.bin_mode == 1 ? W(h, "bin_tab") : nullptr, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_scene_cells(desire_handle* h, const float* dev_pos, int32_t* dev_cells, int32_t n, void* stream) {
    if (!h || !dev_pos || !dev_cells || n < 0) return fail(DESIRE_ERR_ARG, "bad argument");
    if (n == 0) return DESIRE_OK;
    launch_scene_cells(dev_pos, dev_cells, n, h->d.Gh, h->d.Gw, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_scene_cnn(desire_handle* h, const float* dev_image, int32_t Hi, int32_t Wi, float* dev_grids, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!dev_image || !dev_grids) return fail(DESIRE_ERR_ARG, "null argument");
    const desire_dims& d = h->d;
    if (Hi != 4 * d.Gh || Wi != 4 * d.Gw) return fail(DESIRE_ERR_ARG, "scene image must be [n_grids, 4*Gh, 4*Gw, 3]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n1 = (size_t)d.n_grids * (Hi / 2) * (Wi / 2) * 16, n2 = (size_t)d.n_grids * d.Gh * d.Gw * 32;
    if (int rc = ws_ensure(h, {{"scnn1", n1 * sizeof(float)}, {"scnn2", n2 * sizeof(float)}})) return rc;
    { Timer t(h, s, "scene_cnn");
      launch_conv_direct(dev_image, D(h, "scene_cnn/conv1/w"), D(h, "scene_cnn/conv1/b"), W(h, "scnn1"), d.n_grids, Hi, Wi, 3, 16, 2, 1, s);
      launch_conv_direct(W(h, "scnn1"), D(h, "scene_cnn/conv2/w"), D(h, "scene_cnn/conv2/b"), W(h, "scnn2"), d.n_grids, Hi / 2, Wi / 2, 16, 32, 2, 1, s);
      launch_conv_direct(W(h, "scnn2"), D(h, "scene_cnn/conv3/w"), D(h, "scene_cnn/conv3/b"), dev_grids, d.n_grids, d.Gh, d.Gw, 32, d.C, 1, 0, s); }
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// the scene CNN of desire_set_scene_images: the same three launches as desire_scene_cnn (bit-identical grid), post-ReLU scnn1 / scnn2 kept
int scene_images_run(desire_ctx* h, hipStream_t s) {
    if (int rc = desire_scene_cnn(h, h->img, 4 * h->d.Gh, 4 * h->d.Gw, W(h, "scene_img_grid"), s)) return rc;
    h->img_stale = false;
    return DESIRE_OK;
}

extern "C" int desire_losses(desire_handle* h, const float* dev_fut, const float* dev_Yhat, float* dev_kld,
                             float* dev_recon, float* dev_cost, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!dev_fut || !dev_Yhat || !dev_kld || !dev_recon || !dev_cost) return fail(DESIRE_ERR_ARG, "null argument");
    const desire_dims& d = h->d;
    if (!d.posterior) return fail(DESIRE_ERR_STATE, "losses need the posterior path (dims.posterior = 1)");
    if (d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat has no trajectory head: the reference's cost has undefined inputs (model/model.py:342)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_loss_mask(Wt<const uint8_t>(h, "valid"), dev_fut, Wt<uint8_t>(h, "lmask"), W(h, "nfut"), d.n_scenes, d.mno, d.T_pred, s);
    launch_losses(W(h, "params"), dev_Yhat, dev_fut, Wt<const uint8_t>(h, "lmask"), W(h, "nfut"), dev_kld, dev_recon,
                  dev_cost, d.n_scenes, d.mno, d.K, d.T_pred, d.L, d.sx, d.sy, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- per-sample reconstruction errors and the weights of the best-of-many / soft-min loss (kernels_recon.hip): the contract is stated in
// include/desire_hip.h.  The training step (backward.hip: loss_grads) runs the same kernel into the same workspace tensors. ----
int recon_ws_setup(desire_ctx* h) {
    const size_t f = sizeof(float);
    return ws_ensure(h, {{"recon_e", (size_t)h->R * f}, {"recon_w", (size_t)h->R * f}, {"recon_win", (size_t)h->A * sizeof(int32_t)}, {"recon_val", (size_t)h->A * f}});
}

extern "C" int desire_recon_weights(desire_handle* h, const float* dev_fut, const float* dev_Yhat, int32_t mode, float tau, float* dev_e,
                                    float* dev_w, int32_t* dev_winner, float* dev_recon, void* stream) {
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
    if (int rc = recon_ws_setup(h)) return rc;          // (the first call allocates; later calls are capturable)
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_loss_mask(Wt<const uint8_t>(h, "valid"), dev_fut, Wt<uint8_t>(h, "lmask"), W(h, "nfut"), d.n_scenes, d.mno, d.T_pred, s);
    launch_recon_weights(dev_Yhat, dev_fut, Wt<const uint8_t>(h, "lmask"), W(h, "nfut"), dev_e ? dev_e : W(h, "recon_e"), dev_w ? dev_w : W(h, "recon_w"),
                         dev_winner ? dev_winner : Wt<int32_t>(h, "recon_win"), dev_recon ? dev_recon : W(h, "recon_val"), d.n_scenes, d.mno, d.K,
                         d.T_pred, mode, tau, d.sx, d.sy, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- the scene scope: the K worlds of a window weighed by their mean error over the window's counted agents ----
int recon_scene_ws_setup(desire_ctx* h) {
    if (int rc = recon_ws_setup(h)) return rc;
    return ws_ensure(h, {{"recon_E", (size_t)h->d.n_scenes * h->d.K * sizeof(float)}, {"recon_cnt", (size_t)h->d.n_scenes * sizeof(int32_t)}});
}

void recon_weights_enqueue(desire_ctx* h, const float* fut, const uint8_t* lmask, hipStream_t s) {
    const desire_dims& d = h->d;
    if (h->recon_scope == DESIRE_RECON_SCOPE_SCENE)
        launch_recon_weights_scene(W(h, "Y0"), fut, lmask, W(h, "nfut"), W(h, "recon_e"), W(h, "recon_E"), Wt<int32_t>(h, "recon_cnt"), W(h, "recon_w"),
                                   Wt<int32_t>(h, "recon_win"), W(h, "recon_val"), d.n_scenes, d.mno, d.K, d.T_pred, h->recon_mode, h->recon_tau,
                                   d.sx, d.sy, s);
    else
        launch_recon_weights(W(h, "Y0"), fut, lmask, W(h, "nfut"), W(h, "recon_e"), W(h, "recon_w"), Wt<int32_t>(h, "recon_win"), W(h, "recon_val"),
                             d.n_scenes, d.mno, d.K, d.T_pred, h->recon_mode, h->recon_tau, d.sx, d.sy, s);
}

extern "C" int desire_recon_weights_scene(desire_handle* h, const float* dev_fut, const float* dev_Yhat, int32_t mode, float tau, float* dev_e,
                                          float* dev_E, int32_t* dev_count, float* dev_w, int32_t* dev_winner, float* dev_recon, void* stream) {
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
    if (int rc = recon_scene_ws_setup(h)) return rc;    // (the first call allocates; later calls are capturable)
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_loss_mask(Wt<const uint8_t>(h, "valid"), dev_fut, Wt<uint8_t>(h, "lmask"), W(h, "nfut"), d.n_scenes, d.mno, d.T_pred, s);
    launch_recon_weights_scene(dev_Yhat, dev_fut, Wt<const uint8_t>(h, "lmask"), W(h, "nfut"), dev_e ? dev_e : W(h, "recon_e"),
                               dev_E ? dev_E : W(h, "recon_E"), dev_count ? dev_count : Wt<int32_t>(h, "recon_cnt"), dev_w ? dev_w : W(h, "recon_w"),
                               dev_winner ? dev_winner : Wt<int32_t>(h, "recon_win"), dev_recon ? dev_recon : W(h, "recon_val"), d.n_scenes, d.mno,
                               d.K, d.T_pred, mode, tau, d.sx, d.sy, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_temporal_conv(desire_handle* h, const float* dev_past, float* dev_rho, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!dev_past || !dev_rho) return fail(DESIRE_ERR_ARG, "null argument");
    const desire_dims& d = h->d;
    launch_temporal_conv(dev_past, D(h, "temporal/w"), D(h, "temporal/b"), dev_rho, d.n_scenes, d.T_obs, d.mno,
                         static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_feature_pooling(desire_handle* h, const float* dev_Yhat, const float* dev_rho, float* dev_out, void* stream) {
    if (!h || !dev_Yhat || !dev_rho || !dev_out) return fail(DESIRE_ERR_ARG, "null argument");
    const desire_dims& d = h->d;
    // ref_compat: dev_Yhat = output_states [A, n_dec, T_obs, 2] -> [A, n_dec*T_obs, 200] (model/model.py:291-311 over the 7 states)
    launch_feature_pooling(dev_Yhat, dev_rho, dev_out, h->R, d.ref_compat ? d.n_dec * d.T_obs : d.T_pred, d.K, d.mno, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_build_windows(desire_handle* h, const float* dev_frames, int32_t n_frames, int32_t mno_in,
                                    const int32_t* host_starts, int32_t n_windows, float* dev_past, float* dev_fut, void* stream) {
    return desire_build_windows_la(h, dev_frames, n_frames, mno_in, host_starts, n_windows, 0, dev_past, dev_fut, stream);
}

extern "C" int desire_build_windows_la(desire_handle* h, const float* dev_frames, int32_t n_frames, int32_t mno_in,
                                     const int32_t* host_starts, int32_t n_windows, int32_t lookahead, float* dev_past, float* dev_fut,
                                     void* stream) {
    if (!h || !dev_frames || !host_starts || !dev_past || !dev_fut) return fail(DESIRE_ERR_ARG, "null argument");
    if (lookahead != 0 && lookahead != 1) return fail(DESIRE_ERR_ARG, "lookahead must be 0 or 1");
    const desire_dims& d = h->d;
    if (n_windows < 1 || n_windows > d.n_scenes) return fail(DESIRE_ERR_ARG, "n_windows must be 1..n_scenes");
    if (mno_in < 1 || n_frames < d.T_obs + d.T_pred) return fail(DESIRE_ERR_ARG, "video shorter than one window");
    for (int i = 0; i < n_windows; ++i)
        if (host_starts[i] < 0 || host_starts[i] + d.T_obs + d.T_pred > n_frames)
            return fail(DESIRE_ERR_ARG, "window start out of range");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (plain pointers cached by desire_create, not the handle's map: this call may run on a feeder thread while another call inserts into the map)
    HIPCHK(hipMemcpyAsync(h->bw_starts, host_starts, n_windows * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->bw_err, 0, sizeof(int32_t), s));
    launch_build_windows(dev_frames, n_frames, mno_in, h->bw_starts, n_windows, d.T_obs,
                         d.T_pred, d.mno, dev_past, dev_fut, h->bw_err, lookahead, s);
    int32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, h->bw_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (err & 2) return fail(DESIRE_ERR_ARG, "a window holds more unique ids than max_num_obj slots (utils/data_loader.py:227 IndexError)");
    if (err & 4) return fail(DESIRE_ERR_ARG, "a track id occurs twice in one frame of a window (utils/data_loader.py:224-229 ValueError)");
    if (err & 1) return fail(DESIRE_ERR_ARG, "track id outside [0, 65536)");
    return DESIRE_OK;
}

extern "C" int desire_gaussian_sample(desire_handle* h, const float* dev_params, const float* dev_normals, float* dev_out,
                                      int32_t n, void* stream) {
    if (!h || !dev_params || !dev_normals || !dev_out || n < 0) return fail(DESIRE_ERR_ARG, "bad argument");
    if (n == 0) return DESIRE_OK;
    launch_gaussian_sample(dev_params, dev_normals, dev_out, n, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// sample()'s autoregressive rollout (model/model.py:623-688): warm-up over the observed frames with the X-encoder GRU (the
// reference's loop :623-632 carrying `states`), then `num` prediction steps, each: 5-wide Gaussian head on the state (:651,
// 661-663) -> draw (:665) -> clip (:666-669) -> feed the drawn position back as the next input (:680-681).
extern "C" int desire_rollout(desire_handle* h, const float* dev_past, const float* dev_normals, int32_t num, float* dev_out,
                              void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!dev_past || !dev_normals || !dev_out) return fail(DESIRE_ERR_ARG, "null argument");
    if (num < 1) return fail(DESIRE_ERR_ARG, "num must be >= 1");
    const desire_dims& d = h->d;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = ws_ensure(h, {{"roll_h", (size_t)h->A * d.H * sizeof(float)}})) return rc;
    EncArgs e{};
    e.n_scenes = d.n_scenes; e.mno = d.mno; e.sx = d.sx; e.sy = d.sy; e.H = d.H;
    e.frames = dev_past; e.T = d.T_obs;
    enc_weights(h, "enc_x", e);
    e.out = W(h, "roll_h"); e.ldo = d.H;
    e.n_roll = num; e.w5 = D(h, "gauss_head/w"); e.b5 = D(h, "gauss_head/b"); e.normals = dev_normals; e.roll_out = dev_out;
    { Timer t(h, s, "rollout"); launch_encoder(e, s); }
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// K rollouts per agent in the sample layout: the warm-up above ONCE per agent into "roll_h" (k_encoder, no prediction step), then k_rollout
// (kernels_rollout.hip) over the R = A * K rows, each from its agent's state.  dev_normals == NULL: drawn in the kernel (one draw of the generator).
static int rollout_check_packing(const desire_ctx* h);
extern "C" int desire_rollout_samples(desire_handle* h, const float* dev_past, const float* dev_normals, float* dev_Yhat, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!dev_past) return fail(DESIRE_ERR_ARG, "dev_past is NULL");
    if (!dev_Yhat) return fail(DESIRE_ERR_ARG, "dev_Yhat is NULL");
    const desire_dims& d = h->d;
    if (d.ref_compat) return fail(DESIRE_ERR_ARG, "handle: ref_compat has no sample layout [R, T_pred, 2] to roll out into");
    if (!dev_normals) {
        if (!h->rng_state) return fail(DESIRE_ERR_ARG, "dev_normals is NULL and desire_set_rng has not been called");
        if (int rc = rollout_check_packing(h)) return rc;
    }
    if (int rc = desire_ready(h)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = ws_ensure(h, {{"roll_h", (size_t)h->A * d.H * sizeof(float)}})) return rc;
    if (!dev_normals) launch_rng_begin(h->rng_state, s);       // one draw per generating call
    EncArgs e{};
    e.n_scenes = d.n_scenes; e.mno = d.mno; e.sx = d.sx; e.sy = d.sy; e.H = d.H;
    e.frames = dev_past; e.T = d.T_obs;
    enc_weights(h, "enc_x", e);
    e.out = W(h, "roll_h"); e.ldo = d.H;
    { Timer t(h, s, "rollout_warmup"); launch_encoder(e, s); }
    RollArgs r{};
    r.h_T = W(h, "roll_h"); r.R = h->R; r.K = d.K; r.mno = d.mno; r.H = d.H; r.T = d.T_pred;
    r.wx_g = e.wx_g; r.b_g = e.b_g; r.wx_c = e.wx_c; r.b_c = e.b_c; r.Whg = e.Whg; r.Whc = e.Whc;
    r.w5 = D(h, "gauss_head/w"); r.b5 = D(h, "gauss_head/b");
    r.normals = dev_normals; r.g = rng_args(h); r.Y = dev_Yhat;
    { Timer t(h, s, "rollout_samples"); launch_rollout_samples(r, s); }
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_ade_fde(desire_handle* h, const float* dev_Yhat, const float* dev_fut, float* dev_out, void* stream) {
    if (!h || !dev_Yhat || !dev_fut || !dev_out) return fail(DESIRE_ERR_ARG, "null argument");
    const desire_dims& d = h->d;
    launch_ade_fde(dev_Yhat, dev_fut, dev_out, d.n_scenes, d.mno, d.K, d.T_pred, d.sx, d.sy, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- argument checks that the evaluation entry points share (each call keeps its own order of checks) ----
namespace {
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
    launch_rank_select(dev_score, dev_Yhat, dev_order, dev_top_Y, dev_top_score, d.n_scenes, d.mno, d.K, d.T_pred, n_top,
                       static_cast<hipStream_t>(stream));
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
    launch_ranked_errors(dev_Yhat, dev_fut, dev_order, W(h, "rank_tab"), Wt<int32_t>(h, "rank_cnt"), dev_out, d.n_scenes,
                         d.mno, d.K, d.T_pred, n_top, hz, d.sx, d.sy, unit_x, unit_y, static_cast<hipStream_t>(stream));
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
    launch_kde_nll(dev_Yhat, dev_fut, dev_score, W(h, "kde_w"), W(h, "kde_st"), dev_out, dev_frame, d.n_scenes, d.mno, d.K, d.T_pred, hz,
                   d.sx, d.sy, unit_x, unit_y, log_floor, static_cast<hipStream_t>(stream));
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
    launch_select_diverse(dev_Yhat, dev_order, dev_score, dev_order_out, dev_count, dev_mass, dev_top_Y, dev_top_score, d.n_scenes, d.mno, d.K,
                          d.T_pred, metric, t_end, n_top, radius, unit_x, unit_y, static_cast<hipStream_t>(stream));
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
    if (errors)
        launch_sample_errors(dev_Yhat, dev_fut, W(h, "rank_tab"), Wt<int32_t>(h, "rank_cnt"), d.n_scenes, d.mno, d.K, d.T_pred, hz, d.sx, d.sy,
                             unit_x, unit_y, s);
    launch_joint_metrics(dev_Yhat, dev_fut, dev_present, dev_score, errors ? W(h, "rank_tab") : nullptr, dev_first, dev_cnt,
                         errors ? (dev_jerr ? dev_jerr : W(h, "joint_je")) : nullptr, dev_jscore ? dev_jscore : W(h, "joint_js"), dev_jorder, dev_out,
                         d.n_scenes, d.mno, d.K, d.T_pred, n_top, hz, d.sx, d.sy, unit_x, unit_y, radius, s);
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
    launch_select_worlds(dev_Yhat, dev_present, dev_wscore, dev_worder, dev_wcount, dev_wmass, dev_wlabel, d.n_scenes, d.mno, d.K, d.T_pred, metric,
                         reduce, t_end, radius, unit_x, unit_y, static_cast<hipStream_t>(stream));
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
    if (int rc = parse_horizons(host_horizons, n_h, d.T_pred, &hz)) return rc;
    if (int rc = check_radius(radius)) return rc;
    if (int rc = check_units(unit_x, unit_y)) return rc;
    int pc = 0, tc = 0;
    plan_geometry(d.mno, d.T_pred, M, &pc, &tc);
    if (tc < 1) return fail(DESIRE_ERR_ARG, "one frame of the window does not fit the plan kernel's LDS");      // (not reachable at mno <= 256)
    if ((uint64_t)d.n_scenes * (uint64_t)((M + pc - 1) / pc) >= (1ull << 31)) return fail(DESIRE_ERR_ARG, "n_scenes * plan chunks must be below 2^31");
    launch_plan_risk(dev_Yhat, dev_fut, dev_present, dev_score, dev_plans, dev_ego, W(h, "joint_js"), dev_first, dev_clear, dev_risk, dev_blame,
                     d.n_scenes, d.mno, d.K, d.T_pred, M, hz, d.sx, d.sy, unit_x, unit_y, radius, static_cast<hipStream_t>(stream));
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
    if (int rc = parse_horizons(host_horizons, n_h, d.T_pred, &hz)) return rc;
    if (int rc = check_radius(radius)) return rc;
    if (int rc = check_units(unit_x, unit_y)) return rc;
    int pc = 0, tc = 0, cpc = 0, ctc = 0, rows = 0;
    plan_geometry(d.mno, d.T_pred, M, &pc, &tc);
    plan_cond_geometry(d.K, t_cond, M, &cpc, &ctc, &rows);
    if (tc < 1 || ctc < 1) return fail(DESIRE_ERR_ARG, "one frame of the window does not fit the plan kernels' LDS");      // (not reachable)
    const int least = pc < cpc ? pc : cpc;
    if ((uint64_t)d.n_scenes * (uint64_t)((M + least - 1) / least) >= (1ull << 31)) return fail(DESIRE_ERR_ARG, "n_scenes * plan chunks must be below 2^31");
    const volatile float two_s = 2.f * sigma, two_s2 = two_s * sigma;  // fp32, every operation rounded once (2 * sigma is exact)
    const float inv = 1.f / two_s2;
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_plan_prior(dev_fut, dev_present, dev_score, W(h, "joint_js"), W(h, "joint_je"), d.n_scenes, d.mno, d.K, d.T_pred, s);
    launch_plan_cond_weights(dev_Yhat, dev_fut, dev_present, dev_plans, dev_ego, W(h, "joint_js"), W(h, "joint_je"), dev_cw, dev_dist, dev_ess,
                             dev_support, dev_cond, d.n_scenes, d.mno, d.K, d.T_pred, M, t_cond, unit_x, unit_y, inv, s);
    launch_plan_risk_per_plan(dev_Yhat, dev_fut, dev_present, dev_plans, dev_ego, dev_cw, dev_first, dev_clear, dev_risk, dev_blame, d.n_scenes,
                              d.mno, d.K, d.T_pred, M, hz, d.sx, d.sy, unit_x, unit_y, radius, s);
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
    launch_fit_modes(dev_Yhat, dev_order, dev_score, dev_fut, o, p, d.n_scenes, d.mno, d.K, d.T_pred, static_cast<hipStream_t>(stream));
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
    launch_fit_scene_modes(dev_Yhat, dev_present, dev_worder, dev_wscore, dev_fut, o, p, d.n_scenes, d.mno, d.K, d.T_pred, h->scene_modes_chunk,
                           static_cast<hipStream_t>(stream));
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
    launch_kde_weights(dev_score, W(h, "kde_w"), W(h, "kde_st"), d.n_scenes, d.mno, d.K, s);
    launch_occupancy(dev_Yhat, dev_fut, dev_present, W(h, "kde_w"), dev_viol ? dev_mask : nullptr, dev_viol ? dev_mask_of_scene : nullptr, dev_occ,
                     dev_exp, dev_hit, dev_viol, dev_off, d.n_scenes, d.mno, d.K, d.T_pred, Oh, Ow, mode, hz, d.sx, d.sy, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

// ---- the device generator (philox.h, kernels_rng.hip): the packing of its counters is stated in include/desire_hip.h ------------------------
namespace {
int rng_check_packing(const desire_ctx* h, uint32_t slot_base) {
    const desire_dims& d = h->d;
    if (d.L > PHILOX_MAX_L) return fail(DESIRE_ERR_ARG, "the generator's counter holds latents up to L = 4096");
    if (d.K >= PHILOX_MAX_K) return fail(DESIRE_ERR_ARG, "the generator's counter holds sample indices k < 8192");
    if ((uint64_t)slot_base + (uint64_t)d.mno > (uint64_t)PHILOX_MAX_SLOT) return fail(DESIRE_ERR_ARG, "the generator's counter holds global slots (slot_base + mno) up to 512");
    return 0;
}
}  // namespace
// the rollout counter packs the step where the latent counter packs the latent: T_pred <= 2048 on top of the latent's limits
static int rollout_check_packing(const desire_ctx* h) {
    if (int rc = rng_check_packing(h, h->rng_slot_base)) return rc;
    if (h->d.T_pred > PHILOX_MAX_T) return fail(DESIRE_ERR_ARG, "the generator's rollout counter holds steps up to T_pred = 2048");
    return 0;
}

extern "C" int desire_set_rng(desire_handle* h, uint64_t seed, uint32_t draw, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null argument");
    if (int rc = rng_check_packing(h, h->rng_slot_base)) return rc;
    if (!h->rng_state) {          // the first call allocates the words (never a sampling call); later calls are one kernel and capturable
        if (int rc = ws_ensure(h, {{"rng_state", 4 * sizeof(uint32_t)}})) return rc;
        h->rng_state = Wt<uint32_t>(h, "rng_state");
    }
    launch_rng_set(h->rng_state, seed, draw, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_set_rng_origin(desire_handle* h, uint32_t scene_base, uint32_t slot_base) {
    if (!h) return fail(DESIRE_ERR_ARG, "null argument");
    if (int rc = rng_check_packing(h, slot_base)) return rc;
    h->rng_scene_base = scene_base; h->rng_slot_base = slot_base;
    return DESIRE_OK;
}

extern "C" int desire_rng_state(desire_handle* h, uint32_t* host_out2, void* stream) {
    if (!h || !host_out2) return fail(DESIRE_ERR_ARG, "null argument");
    if (!h->rng_state) return fail(DESIRE_ERR_STATE, "desire_set_rng comes first");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(hipMemcpyAsync(host_out2, h->rng_state, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return DESIRE_OK;
}

extern "C" int desire_rng_fill(desire_handle* h, uint64_t seed, uint32_t stream_id, uint64_t first, int32_t kind, void* dev_out, size_t n, void* stream) {
    if (!h || !dev_out) return fail(DESIRE_ERR_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (kind == DESIRE_RNG_BITS || kind == DESIRE_RNG_NORMAL) {
        if (first + (uint64_t)n < first) return fail(DESIRE_ERR_ARG, "first + n passes 2^64");
        launch_rng_fill(seed, stream_id, first, kind == DESIRE_RNG_NORMAL, dev_out, n, s);
    } else if (kind == DESIRE_RNG_LATENT) {       // the eps [n_scenes, K, mno, L] of draw `stream_id` at the handle's origin: k_reparam_rng in prior mode
        if (int rc = rng_check_packing(h, h->rng_slot_base)) return rc;
        if (first != 0 || n != (size_t)h->R * h->d.L) return fail(DESIRE_ERR_ARG, "DESIRE_RNG_LATENT writes the whole eps: first = 0, n = R * L");
        const RngArgs g{nullptr, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, h->rng_scene_base, h->rng_slot_base};
        launch_reparam_rng(nullptr, g, static_cast<float*>(dev_out), h->R, h->d.L, h->d.K, h->d.mno, 0, s);
    } else if (kind == DESIRE_RNG_ROLLOUT) {      // the normals [R, T_pred, 2] of draw `stream_id` at the handle's origin: k_rollout's own device function
        if (int rc = rollout_check_packing(h)) return rc;
        if (first != 0 || n != (size_t)h->R * h->d.T_pred * 2) return fail(DESIRE_ERR_ARG, "DESIRE_RNG_ROLLOUT writes the whole tensor: first = 0, n = R * T_pred * 2");
        const RngArgs g{nullptr, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, h->rng_scene_base, h->rng_slot_base};
        launch_rollout_normals(g, static_cast<float*>(dev_out), h->R, h->d.T_pred, h->d.K, h->d.mno, s);
    } else return fail(DESIRE_ERR_ARG, "kind must be DESIRE_RNG_BITS, DESIRE_RNG_NORMAL, DESIRE_RNG_LATENT or DESIRE_RNG_ROLLOUT");
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}
