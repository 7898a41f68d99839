// api.hip -- C ABI of libdesire_hip.so (include/desire_hip.h): handle, weights as set by the caller (their packed device forms: pack.h,
// api_pack.hip), workspace, buffer read-back and hipGraph capture.  Host code only.
#include "ctx.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static thread_local std::string g_err;
int desire_fail(int code, const std::string& msg) { g_err = msg; return code; }

extern "C" const char* desire_last_error(void) { return g_err.c_str(); }
extern "C" int desire_version(void) { return 5; }
extern "C" int desire_dims_size(void) { return (int)sizeof(desire_dims); }
#ifndef DESIRE_SRC_HASH
#define DESIRE_SRC_HASH "unstamped"
#endif
extern "C" const char* desire_build_hash(void) { return DESIRE_SRC_HASH; }

int desire_upload(desire_ctx* h, const std::string& name, const std::vector<float>& v) {
    const size_t bytes = v.size() * sizeof(float);
    const DevBuf* b = h->dev.find(name.c_str());
    if (!b || b->bytes != bytes) {                           // same shape: refresh in place (pointers stay valid); otherwise exactly the new size
        h->dev.release(name.c_str());
        if (h->dev.ensure(name.c_str(), bytes)) return -1;
    }
    return hipMemcpy(h->dev.get(name.c_str()), v.data(), bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

static void embed_walk(const Embed& em, const std::function<void(size_t, size_t)>& f) {
    size_t cl = 0, cp = 0;
    for (auto& c : em.cols.seg) { cl += c.first; cp += c.second; }
    size_t rl = 0, rp = 0;
    for (auto& r : em.rows.seg) {
        for (int i = 0; i < r.first; ++i) {
            size_t ol = 0, op = 0;
            for (auto& c : em.cols.seg) {
                for (int j = 0; j < c.first; ++j) f((rl + i) * cl + ol + j, (rp + i) * cp + op + j);
                ol += c.first; op += c.second;
            }
        }
        rl += r.first; rp += r.second;
    }
}
std::vector<float> desire_embed(const desire_ctx* h, const std::string& name, const float* user) {
    auto it = h->emb.find(name);
    const size_t np = h->want.at(name);
    if (it == h->emb.end()) return std::vector<float>(user, user + np);
    std::vector<float> out(np, 0.f);
    embed_walk(it->second, [&](size_t il, size_t ip) { out[ip] = user[il]; });
    return out;
}
void desire_extract(const desire_ctx* h, const std::string& name, const float* phys, float* user) {
    auto it = h->emb.find(name);
    if (it == h->emb.end()) { std::memcpy(user, phys, h->want.at(name) * sizeof(float)); return; }
    embed_walk(it->second, [&](size_t il, size_t ip) { user[il] = phys[ip]; });
}

namespace {

// logical -> physical embedding of every weight that has a hidden-width axis (ctx.h: Embed)
void embeddings(desire_ctx* h) {
    const desire_dims& d = h->d;
    const std::pair<int, int> Hs{h->Hl, d.H};
    auto fix = [](int n) { return std::pair<int, int>{n, n}; };
    auto& e = h->emb;
    auto gru = [&](const std::string& p, std::vector<std::pair<int, int>> in) {
        in.push_back(Hs);
        e[p + "/gates/kernel"] = Embed{{in}, {{Hs, Hs}}};
        e[p + "/gates/bias"] = Embed{{{fix(1)}}, {{Hs, Hs}}};
        e[p + "/candidate/kernel"] = Embed{{in}, {{Hs}}};
        e[p + "/candidate/bias"] = Embed{{{fix(1)}}, {{Hs}}};
    };
    gru("enc_x", {fix(2)}); gru("enc_y", {fix(2)}); gru("dec", {Hs}); gru("ioc", {fix(d.E_v + d.C), Hs});
    e["fc_c/w"] = Embed{{{Hs, Hs}}, {{fix(h->V)}}};
    e["mask_fc/w"] = Embed{{{fix(h->V)}}, {{Hs}}};
    e["mask_fc/b"] = Embed{{{fix(1)}}, {{Hs}}};
    e["head/w"] = Embed{{{Hs}}, {{fix(2)}}};
    e["ioc/social_fc/w"] = Embed{{std::vector<std::pair<int, int>>(h->B, Hs)}, {{Hs}}};
    e["ioc/social_fc/b"] = Embed{{{fix(1)}}, {{Hs}}};
    e["ioc/score/w"] = Embed{{{Hs}}, {{fix(1)}}};
    e["ioc/reg/w"] = Embed{{{Hs}}, {{fix(2 * d.T_pred)}}};
    e["gauss_head/w"] = Embed{{{Hs}}, {{fix(5)}}};
}

int check_options(const desire_dims& d) {
    switch (d.ioc_form) {
        case DESIRE_IOC_AUTO: case DESIRE_IOC_TILE64: case DESIRE_IOC_CLUSTER: case DESIRE_IOC_CLUSTER_BINS: case DESIRE_IOC_COMPACT:
        case DESIRE_IOC_TRAIN_DENSE: case DESIRE_IOC_X6_TILE32: case DESIRE_IOC_X6_TILE64: break;
        default: return fail(DESIRE_ERR_ARG, "ioc_form must be one of DESIRE_IOC_* (include/desire_hip.h)");
    }
    if (d.ioc_split < 0 || d.ioc_split > 4) return fail(DESIRE_ERR_ARG, "ioc_split must be 0 (auto), 1 (never split: batch-size invariant results) or 2..4 (cap)");
    if (d.train_fp32_mask < 0 || d.train_fp32_mask > 15) return fail(DESIRE_ERR_ARG, "train_fp32_mask is a mask of bits 1, 2, 4, 8");
    if (d.flags & ~(DESIRE_FLAG_NO_FUSE34 | DESIRE_FLAG_TRAIN_FWD_3P | DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC)) return fail(DESIRE_ERR_ARG, "unknown bit in flags (DESIRE_FLAG_*)");
    if ((d.flags & DESIRE_FLAG_COMPACT_IOC) && d.ref_compat) return fail(DESIRE_ERR_ARG, "DESIRE_FLAG_COMPACT_IOC: ref_compat has no IOC stage");
    if ((d.flags & DESIRE_FLAG_COMPACT_ROWS) && (d.bn_mode == 2 || d.ref_compat))
        return fail(DESIRE_ERR_ARG, "DESIRE_FLAG_COMPACT_ROWS: not with bn_mode = 2 (whole-batch statistics depend on the padding rows) or ref_compat");
    return 0;
}

int check_dims(const desire_dims& d) {
    if (d.S != 32) return fail(DESIRE_ERR_ARG, "S must be 32 (rnn_size=512): CVAE stack shapes, model/model.py:465-468");
    if (d.mno < 1 || d.mno > 256 || (d.mno <= 32 ? (32 % d.mno) : (d.mno % 32)))
        return fail(DESIRE_ERR_ARG, "mno must divide 32 or be a multiple of 32 up to 256 (above 128: inference, step-wise IOC)");
    if (d.mno > 128 && d.bf16 == 1) return fail(DESIRE_ERR_ARG, "more than 128 agents per scene run the fp32 step-wise IOC (bf16 = 0, 2 or 3)");
    if (d.H != 16 && d.H != 32 && d.H != 64 && d.H != 128 && d.H != 256)
        return fail(DESIRE_ERR_ARG, "H must be 16, 32 (run zero-padded on the 64-wide tile), 64, 128 or 256");

    if (d.L % 8 || d.L < 8) return fail(DESIRE_ERR_ARG, "L must be a positive multiple of 8");
    if (d.C != 32 || d.E_v != 16) return fail(DESIRE_ERR_ARG, "C=32 and E_v=16 are the instantiated IOC widths in this round");
    if (d.n_scenes < 1 || d.K < 1 || d.T_obs < 1 || d.T_pred < 1 || d.n_grids < 1 || d.iters < 1 || d.Gh < 1 || d.Gw < 1)
        return fail(DESIRE_ERR_ARG, "sizes must be >= 1");
    if (d.grid_size < 1 || d.grid_size > 6) return fail(DESIRE_ERR_ARG, "grid_size must be 1..6 (6 x 6 = the paper's 36 bins)");
    if (d.grid_size > 4 && d.H == 256) return fail(DESIRE_ERR_ARG, "grid_size 5..6 needs H <= 128 (LDS budget of the IOC tile)");
    if (d.bf16 < 0 || d.bf16 > 3)
        return fail(DESIRE_ERR_ARG, "bf16 must be 0 (fp32 operands), 1 (bf16 operands), 2 (split-bf16 operands: hi + lo, three products) or 3 (three "
                                    "bf16 pieces, six products: fp32-class accuracy)");
    if (d.bn_mode < 0 || d.bn_mode > 2) return fail(DESIRE_ERR_ARG, "bn_mode must be 0 (frozen statistics), 1 (per-object statistics) or 2 (whole-batch statistics)");
    if (d.bn_mode && d.bf16 == 1) return fail(DESIRE_ERR_ARG, "batch statistics (bn_mode 1 / 2) run on fp32 operands (bf16 = 0 or 2)");
    if (d.bin_mode != 0 && d.bin_mode != 1) return fail(DESIRE_ERR_ARG, "bin_mode must be 0 (rectangular) or 1 (log-polar)");
    if (d.bin_mode == 1 && (d.grid_size < 3 || !(d.nb_h > 0.f) || !(d.nb_w > d.nb_h)))
        return fail(DESIRE_ERR_ARG, "log-polar bins: grid_size >= 3 and 0 < nb_h (inner radius) < nb_w (outer radius)");
    if (!(d.nb_w > 0.f) || !(d.nb_h > 0.f)) return fail(DESIRE_ERR_ARG, "nb_w/nb_h must be > 0");
    if (d.ref_compat != 0 && d.ref_compat != 1) return fail(DESIRE_ERR_ARG, "ref_compat must be 0 or 1");
    if (int rc = check_options(d)) return rc;
    if (d.ref_compat) {
        if (d.K != 1 || !d.posterior || d.bn_mode != 1 || d.bf16 || d.n_dec < 1 || d.H != 2 * d.T_obs || d.T_pred != d.T_obs)
            return fail(DESIRE_ERR_ARG, "ref_compat (the reference graph as written, model/model.py:116-311) needs K = 1 (one eps per object, "
                                        ":262-263), posterior = 1, bn_mode = 1, bf16 = 0, H == 2*T_obs (:286-289), T_pred == T_obs and n_dec >= 1 (:280 runs 7)");
    } else if (d.n_dec != 0) return fail(DESIRE_ERR_ARG, "n_dec belongs to ref_compat (0 otherwise)");
    return 0;
}

}  // namespace

extern "C" int desire_set_option(desire_handle* h, const char* name, int32_t value) {
    if (!h || !name) return fail(DESIRE_ERR_ARG, "null argument");
    desire_dims d = h->d;
    const std::string nm(name);
    if (nm == "ioc_form") d.ioc_form = value;
    else if (nm == "ioc_split") d.ioc_split = value;
    else if (nm == "train_fp32_mask") d.train_fp32_mask = value;
    else if (nm == "flags") d.flags = value;
    else if (nm == "compact_host_counts") {    // DESIRE_FLAG_COMPACT_*, inference: 1 = read the scans' counts back and size the launches exactly (one host wait per
        h->cp_host_counts = value != 0;        // desire_encode, not capturable -- what training always does); 0 (default) = device-side counts (dyn_count.h: DynCount)
        h->cp_pending = false; h->cp_enc = false;
        return DESIRE_OK;
    }
    else if (nm == "scene_grad") {             // desire_backward also writes d loss / d grids into the workspace tensor "scene_grid_grad"
        if (value != 0 && value != 1) return fail(DESIRE_ERR_ARG, "scene_grad must be 0 or 1");
        h->scene_grad = value != 0;
        return scene_grad_on(h) && h->training ? scene_grad_setup(h) : DESIRE_OK;
    }
    else if (nm == "compact_min_rows") {       // DESIRE_FLAG_COMPACT_IOC: a slot class with fewer rows than this is folded into the next larger one (default 8192)
        if (value < 0) return fail(DESIRE_ERR_ARG, "compact_min_rows must be >= 0");
        h->ci_min_rows = value;
        return DESIRE_OK;
    }
    else if (nm == "scene_modes_chunk") {      // desire_fit_scene_modes: at most this many slots per chunk (0, the default: as many as the LDS plan holds); the bits do not depend on it
        if (value < 0) return fail(DESIRE_ERR_ARG, "scene_modes_chunk must be >= 0");
        h->scene_modes_chunk = value;
        return DESIRE_OK;
    }
    else return fail(DESIRE_ERR_ARG, "unknown option: " + nm + " (ioc_form, ioc_split, train_fp32_mask, flags, compact_min_rows, compact_host_counts, scene_grad, scene_modes_chunk)");
    if (int rc = check_options(d)) return rc;
    // the maps of the last desire_encode were built for the other setting, or for the other slot-class set (ioc_form and train_fp32_mask decide
    // whether class 10 exists): a new desire_encode comes first
    if (((d.flags ^ h->d.flags) & (DESIRE_FLAG_COMPACT_ROWS | DESIRE_FLAG_COMPACT_IOC)) ||
        ((d.flags & DESIRE_FLAG_COMPACT_IOC) && (d.ioc_form != h->d.ioc_form || d.train_fp32_mask != h->d.train_fp32_mask)))
        h->cp_pending = h->cp_enc = false;
    h->d = d;
    return DESIRE_OK;
}

extern "C" int desire_create(const desire_dims* dims, desire_handle** out) {
    if (!dims || !out) return fail(DESIRE_ERR_ARG, "null argument");
    if (int rc = check_dims(*dims)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(DESIRE_ERR_NODEV, "no HIP device: libdesire_hip has no CPU path");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DESIRE_ERR_NODEV, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    desire_ctx* h = new desire_ctx();
    h->d = *dims;
    h->Hl = dims->H;
    if (dims->H < 64) h->d.H = 64;          // narrowest instantiated recurrent tile; the padding is exact (ctx.h: EmbedAxis)
    h->A = dims->n_scenes * dims->mno;
    h->R = h->A * dims->K;
    h->V = dims->S * dims->S;
    h->B = dims->grid_size * dims->grid_size;
    h->E = dims->E_v + dims->C + h->d.H;
    pack::weight_shapes(h->d, h->d.H, h->V, h->B, h->want);
    pack::weight_shapes(h->d, h->Hl, h->V, h->B, h->want_user);
    if (h->Hl != h->d.H) embeddings(h);
    const desire_dims& d = h->d;
    const size_t A = h->A, R = h->R, f = sizeof(float);
    const WsItem list[] = {
        {"HxHy", A * 2 * d.H * f}, {"p_last", A * 2 * f}, {"valid", A}, {"lmask", A}, {"nfut", A * f}, {"vae_in", A * h->V * f},
        {"c1", A * 8192 * f}, {"c2", A * 4096 * f}, {"c3", A * 2048 * f}, {"params", A * 2 * d.L * f},
        {"z", R * d.L * f}, {"d1", R * 2048 * f}, {"d2", R * 4096 * f}, {"d3", R * 8192 * f},
        {"xhat", R * 1024 * f}, {"xz", R * d.H * f}, {"Y0", R * (size_t)(d.n_dec > d.T_pred ? d.n_dec : d.T_pred) * 2 * f},
        {"dec_states", d.ref_compat ? R * (size_t)d.n_dec * d.H * f : 0},
        {"bn_part", d.bn_mode == 2 ? (size_t)512 * 128 * f : 0}, {"bn_stat", d.bn_mode == 2 ? (size_t)2 * 128 * f : 0},
        {"grid_of_scene", (size_t)d.n_scenes * sizeof(int32_t)},
        // desire_build_windows*: allocated here, not lazily, because a feeder thread may call the builder while the owner thread runs a forward on
        // the same handle (desire_amd/prefetch.py: DeviceWindowFeeder) -- the builder then touches these two buffers (through h->bw_starts / h->bw_err,
        // never through the map: allocating calls insert into it) and nothing else of the handle
        {"bw_starts", (size_t)d.n_scenes * sizeof(int32_t)}, {"bw_err", sizeof(int32_t)},
        // desire_ranked_errors: (ADE_h, FDE_h) of every sample for the 8 horizons a call accepts, counted frames of every agent -- here, so that
        // no call allocates and a captured call never has to
        {"rank_tab", d.ref_compat ? 0 : R * 16 * f}, {"rank_cnt", d.ref_compat ? 0 : A * 8 * sizeof(int32_t)},
        // desire_kde_nll: the K weights of every agent (the score layout) and its (den, h2), for the same reason
        {"kde_w", d.ref_compat ? 0 : R * f}, {"kde_st", d.ref_compat ? 0 : A * 2 * f},
        // desire_joint_metrics: the K joint scores of every window and its (JADE_h, JFDE_h) for 8 horizons, for the calls that do not ask for them
        {"joint_js", d.ref_compat ? 0 : (size_t)d.n_scenes * d.K * f}, {"joint_je", d.ref_compat ? 0 : (size_t)d.n_scenes * d.K * 16 * f},
    };
    if (int rc = ws_ensure(h, list)) { desire_destroy(h); return rc; }
    for (const WsItem& w : list) (void)hipMemset(W(h, w.n), 0, w.bytes);
    h->bw_starts = Wt<int32_t>(h, "bw_starts"); h->bw_err = Wt<int32_t>(h, "bw_err");
    if (d.bin_mode == 1) {
        // log-polar social bins: G rings with geometric radii between r_min = nb_h and r_max = nb_w, G equal sectors
        std::vector<float> tab(20, 0.f);
        const int G = d.grid_size;
        for (int k = 0; k < G; ++k) {
            const float t = (float)((double)d.nb_h * std::pow((double)d.nb_w / (double)d.nb_h, (double)(k + 1) / G));
            tab[k] = t * t;
            tab[8 + 2 * k] = (float)std::cos(2.0 * M_PI * k / G);
            tab[9 + 2 * k] = (float)std::sin(2.0 * M_PI * k / G);
        }
        h->bin_tab_host = tab;
        if (int rc = ws_ensure(h, {{"bin_tab", 20 * f}})) { desire_destroy(h); return rc; }
        if (hipMemcpy(W(h, "bin_tab"), tab.data(), 20 * f, hipMemcpyHostToDevice) != hipSuccess) { desire_destroy(h); return fail(DESIRE_ERR_HIP, "bin table upload failed"); }
    }
    *out = h;
    return DESIRE_OK;
}

extern "C" int desire_get_bin_table(desire_handle* h, float* host_out20) {
    if (!h || !host_out20) return fail(DESIRE_ERR_ARG, "null argument");
    if (h->d.bin_mode != 1) return fail(DESIRE_ERR_STATE, "the rectangular grid has no table (dims.bin_mode = 0)");
    std::memcpy(host_out20, h->bin_tab_host.data(), 20 * sizeof(float));
    return DESIRE_OK;
}

extern "C" int desire_peer_close(desire_handle* h);
extern "C" int desire_destroy(desire_handle* h) {
    if (!h) return DESIRE_OK;
    if (h->host_err) { (void)hipHostFree(h->host_err); h->host_err = nullptr; }
    if (h->cp_host) { (void)hipHostFree(h->cp_host); h->cp_host = nullptr; }
    if (h->cp_ev) { (void)hipEventDestroy(h->cp_ev); h->cp_ev = nullptr; }
    (void)desire_peer_close(h);
    h->dev.release_all();
    h->ws.release_all();
    for (auto& p : h->prof) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
    for (void* g : h->graphs) if (g) (void)hipGraphExecDestroy(static_cast<hipGraphExec_t>(g));
    delete h;
    return DESIRE_OK;
}

extern "C" int desire_set_weight(desire_handle* h, const char* name, const float* host_data, size_t n) {
    if (!h || !name || !host_data) return fail(DESIRE_ERR_ARG, "null argument");
    auto it = h->want_user.find(name);
    if (it == h->want_user.end()) return fail(DESIRE_ERR_ARG, std::string("unknown weight: ") + name);
    if (it->second != n)
        return fail(DESIRE_ERR_ARG, std::string("weight ") + name + ": expected " + std::to_string(it->second) +
                                        " values, got " + std::to_string(n));
    h->host_w[name] = desire_embed(h, name, host_data);
    h->finalized = false;
    h->img_stale = true;
    h->training = false;            // the optimiser's master copy is rebuilt by the next desire_set_training(h, 1)
    return DESIRE_OK;
}

extern "C" int desire_finalize_weights(desire_handle* h) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    for (auto& kv : h->want)
        if (!h->host_w.count(kv.first)) return fail(DESIRE_ERR_STATE, "weight not set: " + kv.first);
    if (int rc = desire_pack_all(h)) return rc;
    h->finalized = true;
    h->img_stale = true;
    return DESIRE_OK;
}

extern "C" int desire_set_scene_grids(desire_handle* h, const float* dev_grids, const int32_t* host_grid_of_scene) {
    if (!h || !dev_grids || !host_grid_of_scene) return fail(DESIRE_ERR_ARG, "null argument");
    for (int i = 0; i < h->d.n_scenes; ++i)
        if (host_grid_of_scene[i] < 0 || host_grid_of_scene[i] >= h->d.n_grids)
            return fail(DESIRE_ERR_ARG, "grid_of_scene entry out of range");
    HIPCHK(hipMemcpy(W(h, "grid_of_scene"), host_grid_of_scene, h->d.n_scenes * sizeof(int32_t), hipMemcpyHostToDevice));
    h->grids = dev_grids;
    h->grids_set = true;
    h->img_set = false; h->img = nullptr;          // the last of desire_set_scene_grids / desire_set_scene_images wins
    return DESIRE_OK;
}

extern "C" int desire_set_scene_images(desire_handle* h, const float* dev_images, int32_t Hi, int32_t Wi, const int32_t* host_grid_of_scene) {
    if (!h || !dev_images || !host_grid_of_scene) return fail(DESIRE_ERR_ARG, "null argument");
    const desire_dims& d = h->d;
    if (Hi != 4 * d.Gh || Wi != 4 * d.Gw) return fail(DESIRE_ERR_ARG, "scene image must be [n_grids, 4*Gh, 4*Gw, 3]");
    const size_t n1 = (size_t)d.n_grids * (Hi / 2) * (Wi / 2) * 16, n2 = (size_t)d.n_grids * d.Gh * d.Gw * 32;
    if (int rc = ws_ensure(h, {{"scnn1", n1 * sizeof(float)}, {"scnn2", n2 * sizeof(float)},
                               {"scene_img_grid", (size_t)d.n_grids * d.Gh * d.Gw * d.C * sizeof(float)}})) return rc;
    if (int rc = desire_set_scene_grids(h, W(h, "scene_img_grid"), host_grid_of_scene)) return rc;
    h->img = dev_images; h->img_set = true; h->img_stale = true;
    if (h->training) return scene_grad_setup(h);
    return DESIRE_OK;
}

int desire_ready(desire_handle* h) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (!h->finalized) return fail(DESIRE_ERR_STATE, "weights not finalized (desire_finalize_weights)");
    return 0;
}

extern "C" int desire_read_buffer(desire_handle* h, const char* name, float* host_out, size_t n, void* stream) {
    if (!h || !name || !host_out) return fail(DESIRE_ERR_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(hipStreamSynchronize(s));
    const desire_dims& d = h->d;
    const size_t A = h->A, R = h->R, f = sizeof(float);
    const std::string nm(name);
    auto strided = [&](const float* src, size_t cols, size_t pitch_cols, size_t rows) -> int {
        if (n != rows * cols) return fail(DESIRE_ERR_ARG, nm + ": expected " + std::to_string(rows * cols) + " values");
        HIPCHK(hipMemcpy2D(host_out, cols * f, src, pitch_cols * f, cols * f, rows, hipMemcpyDeviceToHost));
        return 0;
    };
    if (nm == "Hx") return strided(W(h, "HxHy"), h->Hl, 2 * d.H, A);
    if (nm == "Hy") return strided(W(h, "HxHy") + d.H, h->Hl, 2 * d.H, A);
    if (nm == "xz") return strided(W(h, "xz"), h->Hl, d.H, R);
    if (nm == "z_mean") return strided(W(h, "params"), d.L, 2 * d.L, A);
    if (nm == "z_log_sigma_sq") return strided(W(h, "params") + d.L, d.L, 2 * d.L, A);
    struct P { const char* n; size_t cnt; };
    const P plain[] = {{"vae_in", A * h->V}, {"c1", A * 8192}, {"c2", A * 4096}, {"c3", A * 2048}, {"z", R * d.L},
                       {"d1", R * 2048}, {"d2", R * 4096}, {"d3", R * 8192}, {"xhat", R * 1024},
                       {"Y0", R * d.T_pred * 2}, {"p_last", A * 2}};
    for (const P& p : plain)
        if (nm == p.n) {
            if (n != p.cnt) return fail(DESIRE_ERR_ARG, nm + ": expected " + std::to_string(p.cnt) + " values");
            HIPCHK(hipMemcpy(host_out, W(h, p.n), p.cnt * f, hipMemcpyDeviceToHost));
            return DESIRE_OK;
        }
    {   // any other workspace buffer by its internal name (training-mode saves and gradient streams; the caller knows the layout)
        if (const DevBuf* b = h->ws.find(name)) {
            if (n * f > b->bytes) return fail(DESIRE_ERR_ARG, nm + ": holds " + std::to_string(b->bytes / f) + " values");
            HIPCHK(hipMemcpy(host_out, b->p, n * f, hipMemcpyDeviceToHost));
            return DESIRE_OK;
        }
    }
    return fail(DESIRE_ERR_ARG, "unknown buffer: " + nm);
}

// ---- hipGraph capture of any sequence of desire_* calls made on `stream` (launch-bound shapes: small batches, the
// training step's ~100 launches, the agent-sharded IOC loop).  Everything the library enqueues is stream-ordered and
// pointer-stable, so a captured sequence can be replayed as long as the caller keeps the same device buffers.
// Not capturable: calls that synchronise or copy to the host (desire_train_loss, desire_read_buffer, desire_get_*, the
// cluster-form IOC's error read-back) and desire_adam_step (its bias-corrected step size is a per-call kernel argument).
extern "C" int desire_graph_begin(desire_handle* h, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!stream) return fail(DESIRE_ERR_ARG, "graph capture needs an explicit (non-default) stream");
    if (h->profiling) return fail(DESIRE_ERR_STATE, "switch profiling off before capturing (event records are not part of the graph)");
    HIPCHK(hipStreamBeginCapture(static_cast<hipStream_t>(stream), hipStreamCaptureModeThreadLocal));
    return DESIRE_OK;
}

extern "C" int desire_graph_end(desire_handle* h, void* stream, int32_t* graph_id) {
    if (!h || !stream || !graph_id) return fail(DESIRE_ERR_ARG, "null argument");
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamEndCapture(static_cast<hipStream_t>(stream), &g));
    hipGraphExec_t ex = nullptr;
    const hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return fail(DESIRE_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    h->graphs.push_back(ex);
    *graph_id = (int32_t)h->graphs.size() - 1;
    return DESIRE_OK;
}

extern "C" int desire_graph_launch(desire_handle* h, int32_t graph_id, void* stream) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    if (graph_id < 0 || graph_id >= (int32_t)h->graphs.size() || !h->graphs[graph_id]) return fail(DESIRE_ERR_ARG, "unknown graph id");
    HIPCHK(hipGraphLaunch(static_cast<hipGraphExec_t>(h->graphs[graph_id]), static_cast<hipStream_t>(stream)));
    return DESIRE_OK;
}

extern "C" int desire_device_buffer(desire_handle* h, const char* name, void** dev_ptr, size_t* bytes) {
    if (!h || !name || !dev_ptr || !bytes) return fail(DESIRE_ERR_ARG, "null argument");
    if (!std::strcmp(name, "scene_grid_grad") && !(scene_grad_on(h) && h->training))
        return fail(DESIRE_ERR_STATE, "scene_grid_grad needs training mode and desire_set_option(h, \"scene_grad\", 1)");
    const DevBuf* b = h->ws.find(name);
    if (!b) return fail(DESIRE_ERR_ARG, std::string("unknown buffer: ") + name);
    *dev_ptr = b->p; *bytes = b->bytes;
    return DESIRE_OK;
}

extern "C" int desire_set_profiling(desire_handle* h, int enable) {
    if (!h) return fail(DESIRE_ERR_ARG, "null handle");
    h->profiling = enable != 0;
    return DESIRE_OK;
}

extern "C" int desire_get_profile(desire_handle* h, float* host_ms, const char** host_names, int32_t* count) {
    if (!h || !count) return fail(DESIRE_ERR_ARG, "null argument");
    const int cap = *count;
    int n = 0;
    for (auto& p : h->prof) {
        if (n >= cap) break;
        HIPCHK(hipEventSynchronize(p.e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, p.e0, p.e1));
        if (host_ms) host_ms[n] = ms;
        if (host_names) host_names[n] = p.name.c_str();
        ++n;
    }
    *count = n;
    if (!host_ms && !host_names) return DESIRE_OK;      // count query only
    h->prof_name_store.clear();
    for (auto& p : h->prof) h->prof_name_store.push_back(p.name);
    if (host_names) for (int i = 0; i < n; ++i) host_names[i] = h->prof_name_store[i].c_str();
    for (auto& p : h->prof) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
    h->prof.clear();
    return DESIRE_OK;
}
