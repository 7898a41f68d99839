// api_ops.hip -- the stand-alone ops of the ABI: integer paths, scene CNN, losses, the reference's literal tensors, window builder, Gaussian head,
// rollout, ADE / FDE, and the calls of the device generator.  Host code only; the evaluation ops over the sample tensor are api_eval.hip's.
#include "ctx.h"
#include "philox.h"

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
