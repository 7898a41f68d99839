// train.hip -- training half of the C ABI: training-mode buffers, gradient access, losses, device-side clip / Adam / repack (the backward: backward.hip).
// The reference computes tf.gradients(cost) and an Adam update but never runs them (model/model.py:388-403,
// train.py:181); here they run.  Gradients live in ONE flat fp32 buffer in natural (TF) layouts, so a multi-GPU
// caller all-reduces a single tensor (RCCL through torch.distributed) between desire_backward and desire_adam_step.
#include "ctx.h"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace {

// ---- optimiser state lives next to the gradients: Wflat (master weights), Mflat, Vflat, all in Gflat's layout ----
__global__ void k_adam(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                       size_t n, float lr_t, float b1, float b2, float eps) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float gi = g[i];
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        w[i] -= lr_t * mi / (sqrtf(vi) + eps);
    }
}

// global-norm clipping (tf.clip_by_global_norm, model/model.py:390): g *= min(1, clip / ||g||), all on the device
__global__ void k_sqsum(const float* __restrict__ g, size_t n, float* __restrict__ partial) {
    __shared__ float red[256];
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s += g[i] * g[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ void k_clip_scale(float* __restrict__ g, size_t n, const float* __restrict__ partial, int np, float clip, float* norm_out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    const float norm = sqrtf(red[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    const float sc = norm > clip ? clip / norm : 1.f;
    if (sc == 1.f) return;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) g[i] *= sc;
}

// every packed / raw device operand is a gather of the master weights: dst[i] = idx[i] ? Wflat[idx[i]-1] : 0
struct Seg { float* dst; unsigned long long idx_off; unsigned long long n; };
__global__ void k_repack(const Seg* __restrict__ segs, const uint32_t* __restrict__ idx, const float* __restrict__ w) {
    const Seg sg = segs[blockIdx.y];
    const uint32_t* ix = idx + sg.idx_off;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < sg.n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t j = ix[i];
        sg.dst[i] = j ? w[j - 1] : 0.f;
    }
}

// split [hi | lo] bf16 packs of kernels_x3.hip (dims.bf16 = 2): dst[i] = bf16(w), dst[n + i] = bf16(w - hi), w = Wflat[idx[i]-1]
struct Seg16 { uint16_t* dst; unsigned long long idx_off; unsigned long long n; unsigned long long np; };     // np = pieces (pack.h: Enc::SPLIT2 / SPLIT3)
__device__ __forceinline__ uint16_t bf16_rne_dev(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__global__ void k_repack_split(const Seg16* __restrict__ segs, const uint32_t* __restrict__ idx, const float* __restrict__ w) {
    const Seg16 sg = segs[blockIdx.y];
    const uint32_t* ix = idx + sg.idx_off;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < sg.n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t j = ix[i];
        float v = j ? w[j - 1] : 0.f;
        for (unsigned long long pc = 0; pc < sg.np; ++pc) {               // piece pc = bf16 of what the earlier pieces left (each subtraction exact)
            const uint16_t b = bf16_rne_dev(v);
            sg.dst[pc * sg.n + i] = b;
            v -= __uint_as_float((uint32_t)b << 16);
        }
    }
}

// folded batch-norm shift follows the (trainable) conv bias: shift = beta + scale * (b - mean); scale is frozen
__global__ void k_refold(const float* __restrict__ w, float* __restrict__ shift, const float* __restrict__ scale, size_t off_b,
                         size_t off_beta, size_t off_mean, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) shift[c] = w[off_beta + c] + scale[c] * (w[off_b + c] - w[off_mean + c]);
}


// per-agent loss terms of DESIGN.md section 8: out[a] = {recon, kld, ce, reg} (0 for absent agents)
__global__ void k_train_loss(const float* __restrict__ Y0, const float* __restrict__ Yr, const float* __restrict__ fut,
                             const float* __restrict__ score, const float* __restrict__ params, const uint8_t* __restrict__ valid,
                             const float* __restrict__ nfut, float* __restrict__ out, int n_scenes, int mno, int K, int T, int L,
                             float sx, float sy) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_scenes * mno) return;
    const int sc = a / mno, slot = a - sc * mno;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid[a]) {
        float m1 = -3.0e38f, m2 = -3.0e38f, e0s = 0.f, e1s = 0.f;
        for (int k = 0; k < K; ++k) {
            const size_t r = ((size_t)sc * K + k) * mno + slot;
            float dm = 0.f;
            for (int t = 0; t < T; ++t) {
                const float* f = fut + (((size_t)sc * T + t) * mno + slot) * 3;
                if (f[0] == 0.f) continue;               // absent in this target frame (model/model.py:351-366)
                const float gx = __fmul_rn(f[1], sx), gy = __fmul_rn(f[2], sy);
                float dx = Y0[(r * T + t) * 2] - gx, dy = Y0[(r * T + t) * 2 + 1] - gy;
                const float e0 = sqrtf(dx * dx + dy * dy);
                dx = Yr[(r * T + t) * 2] - gx; dy = Yr[(r * T + t) * 2 + 1] - gy;
                e0s += e0; e1s += sqrtf(dx * dx + dy * dy);
                dm = fmaxf(dm, e0);
            }
            m1 = fmaxf(m1, -dm); m2 = fmaxf(m2, score[r]);
        }
        float s1 = 0.f, s2 = 0.f;
        for (int k = 0; k < K; ++k) {
            const size_t r = ((size_t)sc * K + k) * mno + slot;
            float dm = 0.f;
            for (int t = 0; t < T; ++t) {
                const float* f = fut + (((size_t)sc * T + t) * mno + slot) * 3;
                if (f[0] == 0.f) continue;
                const float dx = Y0[(r * T + t) * 2] - __fmul_rn(f[1], sx), dy = Y0[(r * T + t) * 2 + 1] - __fmul_rn(f[2], sy);
                dm = fmaxf(dm, sqrtf(dx * dx + dy * dy));
            }
            s1 += expf(-dm - m1); s2 += expf(score[r] - m2);
        }
        float ce = 0.f;
        for (int k = 0; k < K; ++k) {
            const size_t r = ((size_t)sc * K + k) * mno + slot;
            float dm = 0.f;
            for (int t = 0; t < T; ++t) {
                const float* f = fut + (((size_t)sc * T + t) * mno + slot) * 3;
                if (f[0] == 0.f) continue;
                const float dx = Y0[(r * T + t) * 2] - __fmul_rn(f[1], sx), dy = Y0[(r * T + t) * 2 + 1] - __fmul_rn(f[2], sy);
                dm = fmaxf(dm, sqrtf(dx * dx + dy * dy));
            }
            ce -= expf(-dm - m1) / s1 * (score[r] - m2 - logf(s2));
        }
        float kl = 0.f;
        for (int j = 0; j < L; ++j) {
            const float mu = params[(size_t)a * 2 * L + j], ls = params[(size_t)a * 2 * L + L + j];
            kl += 1.f + ls - mu * mu - expf(ls);
        }
        o = make_float4(e0s / ((float)K * nfut[a]), -0.5f * kl, ce, e1s / ((float)K * nfut[a]));
    }
    reinterpret_cast<float4*>(out)[a] = o;
}
// desire_set_recon_loss (MIN / SOFTMIN): the per-agent term of k_recon_weights (0 for agents that do not count) takes slot 0
__global__ void k_put_recon(const float* __restrict__ val, float* __restrict__ per_agent, int A) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < A) per_agent[(size_t)a * 4] = val[a];
}
// desire_set_recon_scope (SCENE): every slot of a window carries the window's term, so the agents that do not count are zeroed here
__global__ void k_put_recon_counted(const float* __restrict__ val, const uint8_t* __restrict__ lmask, float* __restrict__ per_agent, int A) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < A) per_agent[(size_t)a * 4] = lmask[a] ? val[a] : 0.f;
}
__global__ void k_sum_loss(const float* __restrict__ per_agent, const uint8_t* __restrict__ valid, int A, float* __restrict__ out) {
    __shared__ float red[4][256];
    float s[4] = {0.f, 0.f, 0.f, 0.f}; float nv = 0.f;
    for (int a = threadIdx.x; a < A; a += 256) {
        for (int j = 0; j < 4; ++j) s[j] += per_agent[(size_t)a * 4 + j];
        nv += valid[a] ? 1.f : 0.f;
    }
    __shared__ float rnv[256];
    for (int j = 0; j < 4; ++j) red[j][threadIdx.x] = s[j];
    rnv[threadIdx.x] = nv;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[4] = {0.f, 0.f, 0.f, 0.f}; float n = 0.f;
        for (int i = 0; i < 256; ++i) { for (int j = 0; j < 4; ++j) t[j] += red[j][i]; n += rnv[i]; }
        n = fmaxf(n, 1.f);
        for (int j = 0; j < 4; ++j) out[j] = t[j] / n;
        out[4] = n;
    }
}

// The master weights go to Wflat, and every gather operand of pack.h's table becomes a segment of k_repack (fp32) or k_repack_split (bf16 pieces):
// its gather map plus the offset of its source weight in the flat buffers.  One map is alive at a time.  The folded shifts follow through k_refold.
int build_repack_maps(desire_ctx* h) {
    std::vector<float> flat(h->n_params, 0.f);
    for (auto& kv : h->slots) {
        const auto w = h->host_w.find(kv.first);
        if (w == h->host_w.end() || w->second.size() != kv.second.n) return fail(DESIRE_ERR_STATE, "weight not set: " + kv.first);
        std::memcpy(flat.data() + kv.second.off, w->second.data(), kv.second.n * sizeof(float));
    }
    if (int rc = ws_ensure(h, {{"Wflat", h->n_params * sizeof(float)}, {"Mflat", h->n_params * sizeof(float)}, {"Vflat", h->n_params * sizeof(float)}})) return rc;
    HIPCHK(hipMemcpy(W(h, "Wflat"), flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(W(h, "Mflat"), 0, h->n_params * sizeof(float)));
    HIPCHK(hipMemset(W(h, "Vflat"), 0, h->n_params * sizeof(float)));
    const std::vector<pack::Operand> ops = pack::operands(h->d, h->V, h->B);
    std::vector<Seg> segs; std::vector<Seg16> segs16;
    size_t n_idx = 0;                                      // every map starts at a multiple of 4 indices
    for (const pack::Operand& o : ops) {
        if (o.kind != pack::Kind::GATHER) continue;
        const auto sl = h->slots.find(o.src);
        const DevBuf* op = h->dev.find(o.name.c_str());
        if (sl == h->slots.end() || !op || op->bytes != pack::bytes(o, sl->second.n))
            return fail(DESIRE_ERR_STATE, "repack map: operand " + o.name + " changed shape");
        if (o.enc == pack::Enc::BF16) return fail(DESIRE_ERR_STATE, "repack map: the bf16 operand " + o.name + " has no device repack");
        const unsigned long long n = pack::slots(o, sl->second.n), np = pack::pieces(o.enc);
        if (np) segs16.push_back(Seg16{static_cast<uint16_t*>(op->p), (unsigned long long)n_idx, n, np});
        else segs.push_back(Seg{op->f(), (unsigned long long)n_idx, n});
        n_idx += (n + 3) / 4 * 4;
    }
    if (int rc = ws_ensure(h, {{"repack_idx", n_idx * sizeof(uint32_t)}, {"repack_segs", segs.size() * sizeof(Seg)},
                               {"repack_segs16", std::max<size_t>(1, segs16.size()) * sizeof(Seg16)}})) return rc;
    HIPCHK(hipMemset(W(h, "repack_idx"), 0, n_idx * sizeof(uint32_t)));
    size_t i3 = 0, i16 = 0;
    for (const pack::Operand& o : ops) {
        if (o.kind != pack::Kind::GATHER) continue;
        const WSlot& sl = h->slots.find(o.src)->second;
        std::vector<uint32_t> m = pack::gather_map(o, sl.n);
        for (uint32_t& j : m) if (j) j += (uint32_t)sl.off;
        const size_t off = pack::pieces(o.enc) ? segs16[i16++].idx_off : segs[i3++].idx_off;
        HIPCHK(hipMemcpy(Wt<uint32_t>(h, "repack_idx") + off, m.data(), m.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (!segs16.empty()) HIPCHK(hipMemcpy(W(h, "repack_segs16"), segs16.data(), segs16.size() * sizeof(Seg16), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(W(h, "repack_segs"), segs.data(), segs.size() * sizeof(Seg), hipMemcpyHostToDevice));
    h->n_seg = (int)segs.size(); h->n_seg16 = (int)segs16.size();
    return DESIRE_OK;
}

int repack(desire_ctx* h, hipStream_t s) {
    h->img_stale = true;                                   // scene_cnn/* may have moved: an inference forward reruns the scene CNN
    hipLaunchKernelGGL(k_repack, dim3(64, h->n_seg), dim3(256), 0, s, Wt<const Seg>(h, "repack_segs"),
                       Wt<const uint32_t>(h, "repack_idx"), W(h, "Wflat"));
    if (h->n_seg16)
        hipLaunchKernelGGL(k_repack_split, dim3(64, h->n_seg16), dim3(256), 0, s, Wt<const Seg16>(h, "repack_segs16"),
                           Wt<const uint32_t>(h, "repack_idx"), W(h, "Wflat"));
    for (const char* n : pack::conv_layers) {
        const std::string p(n);
        const int C = (int)h->slots.at(p + "/b").n;
        hipLaunchKernelGGL(k_refold, dim3((C + 63) / 64), dim3(64), 0, s, W(h, "Wflat"), h->dev.get((p + "/shift").c_str()),
                           h->dev.get((p + "/scale").c_str()), h->slots.at(p + "/b").off, h->slots.at(p + "/bn/beta").off,
                           h->slots.at(p + "/bn/moving_mean").off, C);
    }
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

}  // namespace

// scene-grid gradient (kernels_scene.hip): per-row ds, sort keys / indices and their sorted copies, chunk partials for up to RS * T rows of one
// (view, pass); per-key ranges; the [3H, 32] operand; the result [n_grids, Gh, Gw, C].  Allocated here, never inside desire_backward.
int scene_grad_setup(desire_ctx* h) {
    const desire_dims& d = h->d;
    const size_t n = ioc_save_rows(h) * d.T_pred, nk = (size_t)d.n_grids * d.Gh * d.Gw, f = sizeof(float);
    const int bits = scene_key_bits((long)nk);
    const WsItem bufs[] = {
        {"sg_ds", n * 32 * f}, {"sg_part", n * 32 * f}, {"sg_keys", n * 4}, {"sg_keys_sorted", n * 4}, {"sg_idx", n * 4}, {"sg_idx_sorted", n * 4},
        {"sg_beg", nk * 4}, {"sg_end", nk * 4}, {"sg_wcat", (size_t)3 * d.H * 32 * f}, {"sg_tmp", scene_grad_sort_bytes((long)n, bits)},
        {"scene_grid_grad", nk * d.C * f},
        {"sg_col", nk * 800 * f}, {"sg_d2", nk * 32 * f}, {"sg_d1", nk * 4 * 16 * f}};        // scene CNN backward (im2col rows, data gradients)
    for (const WsItem& b : bufs) {
        bool fresh = false;
        if (h->ws.ensure(b.n, b.bytes, &fresh)) return fail(DESIRE_ERR_HIP, std::string("hipMalloc failed for scene-gradient buffer ") + b.n);
        if (fresh && !std::strcmp(b.n, "scene_grid_grad")) HIPCHK(hipMemset(W(h, b.n), 0, b.bytes));
    }
    return DESIRE_OK;
}

extern "C" int desire_set_training(desire_handle* h, int enable) {
    if (int rc = desire_ready(h)) return rc;
    if ((enable != 0) != h->training) { h->cp_pending = false; h->cp_enc = false; }      // compaction maps: inference and training learn the counts differently (a new desire_encode comes first)
    if (!enable) {
        if (h->training) {          // the trained master copy becomes the handle's weights: desire_get_weight and a later
            std::vector<float> flat(h->n_params);          // desire_set_training(h, 1) start from it (Adam moments restart at zero)
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipMemcpy(flat.data(), W(h, "Wflat"), flat.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (auto& kv : h->slots) h->host_w[kv.first].assign(flat.begin() + kv.second.off, flat.begin() + kv.second.off + kv.second.n);
        }
        h->training = false;
        return DESIRE_OK;
    }
    const desire_dims& d = h->d;
    if (!d.posterior) return fail(DESIRE_ERR_STATE, "training needs the posterior path (dims.posterior = 1)");
    if (d.bf16 == 1 || d.bf16 == 3) return fail(DESIRE_ERR_STATE, "training runs with dims.bf16 = 0 (fp32 operands) or 2 (split-bf16 operands where a kernel has that form, fp32 kernels elsewhere); 1 and 3 are inference-only");
    if (d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat is forward-only: the reference never defines a runnable cost (model/model.py:342)");
    if (d.mno > 128) return fail(DESIRE_ERR_STATE, "training supports up to 128 agents per scene (160 .. 256 run the step-wise IOC: inference)");
    if (ioc_plan(h).bwd == IocBwd::CLUSTER && (d.H > 128 || d.grid_size > 4))
        return fail(DESIRE_ERR_STATE, "training of groups larger than one workgroup tile (64 / 96 / 128 agents: cluster-form BPTT) needs H <= 128 and grid_size <= 4");
    if (d.iters > 4) return fail(DESIRE_ERR_STATE, "training keeps the activations of every IOC refinement pass: iters <= 4");
    if (d.T_pred > d.H) return fail(DESIRE_ERR_STATE, "training needs T_pred <= H");
    if (d.grid_size > 4 && d.mno > 32)
        return fail(DESIRE_ERR_STATE, "training with more than 16 social bins needs mno <= 32 (LDS budget of the 64-row IOC backward tile)");
    if (h->slots.empty()) {
        size_t off = 0;
        for (auto& kv : h->want) { h->slots[kv.first] = WSlot{off, kv.second}; off += (kv.second + 3) / 4 * 4; }
        h->n_params = off;
    }
    const size_t R = h->R, T = d.T_pred, H = d.H, f = sizeof(float);
    const size_t RS = ioc_save_rows(h);                         // IOC buffers: rows + slack
    const size_t Tm = d.T_pred > d.T_obs ? d.T_pred : d.T_obs;
    const size_t NP = d.iters;                                  // IOC passes: each keeps its own saves
    const WsItem bufs[] = {
        {"Gflat", h->n_params * f}, {"nvalid", 4 * f}, {"tn_partial", (size_t)96 << 20},
        {"dec_sv_r", R * T * H * f}, {"dec_sv_u", R * T * H * f}, {"dec_sv_c", R * T * H * f}, {"dec_sv_h", R * T * H * f},
        {"dY0", R * T * 2 * f}, {"dec_dag", R * T * 2 * H * f}, {"dec_dac", R * T * H * f}, {"dec_rh", R * T * H * f},
        {"dec_hprev", R * T * H * f}, {"dec_dxg", R * 2 * H * f}, {"dec_dxc", R * H * f}, {"dxz", R * H * f},
        {"dHx_rows", R * H * f}, {"mask_sv_p", R * H * f}, {"dq_mask", R * H * f},
        {"dconv4", R * 1024 * f}, {"dconv3", R * 8192 * f}, {"dconv2", R * 4096 * f}, {"dconv1", R * 2048 * f},
        {"dz", R * d.L * f}, {"dparams", (size_t)h->A * 2 * d.L * f}, {"dconvE3", (size_t)h->A * 2048 * f},
        {"dconvE2", (size_t)h->A * 4096 * f}, {"dconvE1", (size_t)h->A * 8192 * f}, {"dq_c", (size_t)h->A * h->V * f},
        {"dHxHy", (size_t)h->A * 2 * H * f},
        {"ioc_sv_x", NP * RS * T * (size_t)h->E * f}, {"ioc_sv_r", NP * RS * T * H * f}, {"ioc_sv_u", NP * RS * T * H * f}, {"ioc_sv_c", NP * RS * T * H * f},
        {"ioc_sv_h", NP * RS * T * H * f}, {"ioc_Yin", NP * RS * T * 2 * f}, {"dscore0", RS * f},
        {"Y_ref", R * T * 2 * f}, {"score_sv", R * f}, {"dYr", R * T * 2 * f}, {"dscore", R * f},
        {"dscoreT", R * T * f}, {"ioc_dag", RS * T * 2 * H * f}, {"ioc_dac", RS * T * H * f}, {"ioc_rh", RS * T * H * f},
        {"ioc_hprev", RS * T * H * f}, {"ioc_dpre_r", RS * T * H * f}, {"ioc_dpre_v", RS * T * d.E_v * f}, {"ioc_vel", RS * T * 2 * f},
        {"ioc_pooled", RS * T * (size_t)h->B * H * f}, {"ioc_pool_flags", RS * T * sizeof(unsigned long long)},
        {"bin_counts", ((RS * T + 2047) / 2048) * (size_t)h->B * sizeof(int)}, {"bin_base", ((size_t)h->B + 1) * sizeof(int)},
        {"bin_total", (size_t)h->B * sizeof(int)}, {"bin_list", H == 128 ? RS * T * (size_t)h->B * sizeof(int) : 4},
        {"enc_dag", (size_t)h->A * Tm * 2 * H * f}, {"enc_dac", (size_t)h->A * Tm * H * f}, {"enc_rh", (size_t)h->A * Tm * H * f},
        {"enc_hprev", (size_t)h->A * Tm * H * f},
        {"ex_sv_r", (size_t)h->A * d.T_obs * H * f}, {"ex_sv_u", (size_t)h->A * d.T_obs * H * f}, {"ex_sv_c", (size_t)h->A * d.T_obs * H * f},
        {"ex_sv_h", (size_t)h->A * d.T_obs * H * f}, {"ex_sv_x", (size_t)h->A * d.T_obs * 2 * f},
        {"ey_sv_r", (size_t)h->A * T * H * f}, {"ey_sv_u", (size_t)h->A * T * H * f}, {"ey_sv_c", (size_t)h->A * T * H * f},
        {"ey_sv_h", (size_t)h->A * T * H * f}, {"ey_sv_x", (size_t)h->A * T * 2 * f},
    };
    if (int rc = ws_ensure(h, bufs)) return rc;
    if (d.bn_mode != 0) {          // pre-norm copies of the seven conv layers (instance-norm / batch-norm backward)
        const WsItem pre[] = {{"conv1_pre", (size_t)h->A * 8192 * f}, {"conv2_pre", (size_t)h->A * 4096 * f}, {"conv3_pre", (size_t)h->A * 2048 * f},
                         {"deconv1_pre", R * 2048 * f}, {"deconv2_pre", R * 4096 * f}, {"deconv3_pre", R * 8192 * f}, {"deconv4_pre", R * 1024 * f}};
        if (int rc = ws_ensure(h, pre)) return rc;
    }
    if (d.bn_mode == 2) {          // batch-norm backward scratch
        if (int rc = ws_ensure(h, {{"bn_part2", (size_t)512 * 256 * f}, {"bn_stat2", (size_t)2 * 128 * f}, {"bn_statb", (size_t)2 * 128 * f}})) return rc;
    }
    if (int rc = ws_ensure(h, {{"head_nll", (size_t)h->A * d.T_obs * f}, {"head_cnt", (size_t)h->A * d.T_obs * f}, {"head_dO", (size_t)h->A * d.T_obs * 5 * f},      // Gaussian-head loss
                               {"loss_pa", (size_t)h->A * 4 * f}, {"loss_out", 8 * f}, {"bias_part", ((RS + 31) / 32 + 1) * 4 * H * f}})) return rc;
    HIPCHK(hipMemset(W(h, "loss_out"), 0, 8 * f));
    if (int rc = build_repack_maps(h)) return rc;
    if (scene_grad_on(h)) { if (int rc = scene_grad_setup(h)) return rc; }
    h->adam_t = 0;
    h->training = true;
    return DESIRE_OK;
}

extern "C" int desire_set_head_loss(desire_handle* h, float weight) {
    if (!h) return fail(DESIRE_ERR_ARG, "null argument");
    if (!(weight >= 0.f)) return fail(DESIRE_ERR_ARG, "weight must be >= 0");
    if (h->d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat is forward-only");
    h->head_loss_w = weight;
    if (h->training && weight == 0.f) {              // the reported term goes back to zero with the switch
        const float z[3] = {0.f, 0.f, 0.f};
        HIPCHK(hipMemcpy(W(h, "loss_out") + 5, z, sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(W(h, "loss_out") + 7, z, sizeof(float), hipMemcpyHostToDevice));
    }
    return DESIRE_OK;
}

extern "C" int desire_set_recon_loss(desire_handle* h, int32_t mode, float tau) {
    if (!h) return fail(DESIRE_ERR_ARG, "null argument");
    if (mode < DESIRE_RECON_MEAN || mode > DESIRE_RECON_SOFTMIN) return fail(DESIRE_ERR_ARG, "mode must be DESIRE_RECON_MEAN, _MIN or _SOFTMIN (0..2)");
    if (mode == DESIRE_RECON_SOFTMIN && (!std::isfinite(tau) || !(tau > 0.f))) return fail(DESIRE_ERR_ARG, "tau must be finite and > 0 for DESIRE_RECON_SOFTMIN");
    if (mode != DESIRE_RECON_MEAN) {
        if (h->d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat is forward-only");
        int sc = 0, kc = 0;
        if (!recon_geometry(h->d.mno, h->d.K, h->d.T_pred, &sc, &kc)) return fail(DESIRE_ERR_ARG, "T_pred is too long for the reconstruction-weight kernel's LDS");
        if (int rc = recon_ws_setup(h)) return rc;          // here, so that no training step allocates
    }
    h->recon_mode = mode;
    h->recon_tau = mode == DESIRE_RECON_SOFTMIN ? tau : 0.f;
    return DESIRE_OK;
}

extern "C" int desire_set_recon_scope(desire_handle* h, int32_t scope) {
    if (!h) return fail(DESIRE_ERR_ARG, "null argument");
    if (scope < DESIRE_RECON_SCOPE_AGENT || scope > DESIRE_RECON_SCOPE_SCENE) return fail(DESIRE_ERR_ARG, "scope must be DESIRE_RECON_SCOPE_AGENT or _SCENE (0..1)");
    if (scope == DESIRE_RECON_SCOPE_SCENE) {
        if (h->d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat is forward-only");
        int sc = 0, kc = 0;
        if (!recon_geometry(h->d.mno, h->d.K, h->d.T_pred, &sc, &kc)) return fail(DESIRE_ERR_ARG, "T_pred is too long for the reconstruction-weight kernel's LDS");
        if (int rc = recon_scene_ws_setup(h)) return rc;    // here, whatever the mode is or becomes, so that no training step allocates
    }
    h->recon_scope = scope;
    return DESIRE_OK;
}

extern "C" int desire_set_collision_loss(desire_handle* h, float weight, float radius, float unit_x, float unit_y) {
    if (!h) return fail(DESIRE_ERR_ARG, "null argument");
    if (!std::isfinite(weight) || weight < 0.f) return fail(DESIRE_ERR_ARG, "weight must be finite and >= 0");
    if (int rc = check_collision_args(radius, unit_x, unit_y)) return rc;
    if (h->d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat is forward-only");
    if (weight > 0.f) { if (int rc = collision_ws_setup(h)) return rc; }      // here, so that no training step allocates
    h->col_w = weight; h->col_radius = radius; h->col_ux = unit_x; h->col_uy = unit_y;
    return DESIRE_OK;
}

extern "C" int desire_set_offroad_loss(desire_handle* h, float weight, float scale) {
    if (!h) return fail(DESIRE_ERR_ARG, "null argument");
    if (!std::isfinite(weight) || weight < 0.f) return fail(DESIRE_ERR_ARG, "weight must be finite and >= 0");
    if (weight > 0.f && (!std::isfinite(scale) || !(scale > 0.f))) return fail(DESIRE_ERR_ARG, "scale must be finite and > 0");
    if (h->d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat is forward-only");
    if (weight > 0.f) {
        if (!h->off_field) return fail(DESIRE_ERR_STATE, "no distance field set (desire_set_offroad_field)");
        if (int rc = offroad_ws_setup(h)) return rc;       // here, so that no training step allocates
    }
    h->off_w = weight; h->off_scale = scale;
    return DESIRE_OK;
}

extern "C" int desire_set_refined_loss(desire_handle* h, int32_t recon, float collision_weight, float offroad_weight) {
    if (!h) return fail(DESIRE_ERR_ARG, "null argument");
    if (recon != 0 && recon != 1) return fail(DESIRE_ERR_ARG, "recon must be 0 or 1");
    if (!std::isfinite(collision_weight) || collision_weight < 0.f) return fail(DESIRE_ERR_ARG, "collision_weight must be finite and >= 0");
    if (!std::isfinite(offroad_weight) || offroad_weight < 0.f) return fail(DESIRE_ERR_ARG, "offroad_weight must be finite and >= 0");
    if (h->d.ref_compat) return fail(DESIRE_ERR_STATE, "ref_compat is forward-only");
    if (collision_weight > 0.f && !(std::isfinite(h->col_radius) && h->col_radius > 0.f))
        return fail(DESIRE_ERR_STATE, "collision_weight > 0: no radius > 0 set (desire_set_collision_loss; its own weight may be 0)");
    if (offroad_weight > 0.f && !h->off_field) return fail(DESIRE_ERR_STATE, "offroad_weight > 0: no distance field set (desire_set_offroad_field)");
    if (offroad_weight > 0.f && !(std::isfinite(h->off_scale) && h->off_scale > 0.f))
        return fail(DESIRE_ERR_STATE, "offroad_weight > 0: no scale > 0 set (desire_set_offroad_loss; its own weight may be 0)");
    if (recon) {
        int sc = 0, kc = 0;
        if (!recon_geometry(h->d.mno, h->d.K, h->d.T_pred, &sc, &kc)) return fail(DESIRE_ERR_ARG, "T_pred is too long for the reconstruction-weight kernel's LDS");
    }
    if (int rc = refined_ws_setup(h, recon != 0, collision_weight > 0.f, offroad_weight > 0.f)) return rc;      // here, so that no training step allocates
    h->ref_recon = recon; h->rcol_w = collision_weight; h->roff_w = offroad_weight;
    return DESIRE_OK;
}

extern "C" int desire_get_grad(desire_handle* h, const char* name, float* host_out, size_t n, void* stream) {
    if (!h || !name || !host_out) return fail(DESIRE_ERR_ARG, "null argument");
    if (!h->training) return fail(DESIRE_ERR_STATE, "not in training mode");
    auto it = h->slots.find(name);
    if (it == h->slots.end()) return fail(DESIRE_ERR_ARG, std::string("unknown weight: ") + name);
    const size_t nu = h->want_user.at(name);
    if (nu != n) return fail(DESIRE_ERR_ARG, std::string(name) + ": expected " + std::to_string(nu) + " values");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIPCHK(hipStreamSynchronize(s));
    std::vector<float> phys(it->second.n);
    HIPCHK(hipMemcpy(phys.data(), W(h, "Gflat") + it->second.off, phys.size() * sizeof(float), hipMemcpyDeviceToHost));
    desire_extract(h, name, phys.data(), host_out);
    return DESIRE_OK;
}

extern "C" int desire_grad_buffer(desire_handle* h, float** dev_ptr, size_t* n) {
    if (!h || !dev_ptr || !n) return fail(DESIRE_ERR_ARG, "null argument");
    if (!h->training) return fail(DESIRE_ERR_STATE, "not in training mode");
    *dev_ptr = W(h, "Gflat");
    *n = h->n_params;
    return DESIRE_OK;
}

static int train_loss_enqueue(desire_handle* h, const float* dev_fut, hipStream_t s) {
    const desire_dims& d = h->d;
    const uint8_t* valid = Wt<const uint8_t>(h, "lmask");
    launch_loss_mask(Wt<const uint8_t>(h, "valid"), dev_fut, Wt<uint8_t>(h, "lmask"), W(h, "nfut"), d.n_scenes, d.mno, d.T_pred, s);
    hipLaunchKernelGGL(k_train_loss, dim3((h->A + 63) / 64), dim3(64), 0, s, W(h, "Y0"), W(h, "Y_ref"), dev_fut, W(h, "score_sv"),
                       W(h, "params"), valid, W(h, "nfut"), W(h, "loss_pa"), d.n_scenes, d.mno, d.K, d.T_pred, d.L, d.sx, d.sy);
    if (h->recon_mode != DESIRE_RECON_MEAN) {          // slot 0 reports the term that is trained: the min / soft-min over the K samples, or in the scene scope over the window's K worlds (kernels_recon.hip)
        recon_weights_enqueue(h, RECON_Y0, dev_fut, valid, s);
        if (h->recon_scope == DESIRE_RECON_SCOPE_SCENE)
            hipLaunchKernelGGL(k_put_recon_counted, dim3((h->A + 255) / 256), dim3(256), 0, s, W(h, "recon_val"), valid, W(h, "loss_pa"), h->A);
        else
            hipLaunchKernelGGL(k_put_recon, dim3((h->A + 255) / 256), dim3(256), 0, s, W(h, "recon_val"), W(h, "loss_pa"), h->A);
        if (h->ref_recon) {          // desire_set_refined_loss: slot 3 by the same rule, the term of the refined errors (per_agent + 3: the same stride, slot 3)
            recon_weights_enqueue(h, RECON_REFINED, dev_fut, valid, s);
            if (h->recon_scope == DESIRE_RECON_SCOPE_SCENE)
                hipLaunchKernelGGL(k_put_recon_counted, dim3((h->A + 255) / 256), dim3(256), 0, s, W(h, "rrecon_val"), valid, W(h, "loss_pa") + 3, h->A);
            else
                hipLaunchKernelGGL(k_put_recon, dim3((h->A + 255) / 256), dim3(256), 0, s, W(h, "rrecon_val"), W(h, "loss_pa") + 3, h->A);
        }
    }
    hipLaunchKernelGGL(k_sum_loss, dim3(1), dim3(256), 0, s, W(h, "loss_pa"), valid, h->A, W(h, "loss_out"));
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_train_loss(desire_handle* h, const float* dev_fut, float* host_out5, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!h->training) return fail(DESIRE_ERR_STATE, "not in training mode");
    if (!dev_fut || !host_out5) return fail(DESIRE_ERR_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = train_loss_enqueue(h, dev_fut, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(host_out5, W(h, "loss_out"), 5 * sizeof(float), hipMemcpyDeviceToHost));
    return DESIRE_OK;
}

// The same terms (the 8 floats of loss_out: the five above, then the Gaussian-head terms of desire_set_head_loss) into a DEVICE buffer, stream-ordered, no synchronisation: the training loop reads them one step late (a pinned
// copy + event), so the host never waits for the step it has just enqueued and the loader thread keeps running ahead.
extern "C" int desire_train_loss_async(desire_handle* h, const float* dev_fut, float* dev_out8, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!h->training) return fail(DESIRE_ERR_STATE, "not in training mode");
    if (!dev_fut || !dev_out8) return fail(DESIRE_ERR_ARG, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = train_loss_enqueue(h, dev_fut, s)) return rc;
    launch_copy_f32(dev_out8, W(h, "loss_out"), 8, s);
    HIPCHK(hipGetLastError());
    return DESIRE_OK;
}

extern "C" int desire_adam_step(desire_handle* h, float lr, float beta1, float beta2, float eps, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!h->training) return fail(DESIRE_ERR_STATE, "not in training mode");
    if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return fail(DESIRE_ERR_ARG, "bad Adam hyper-parameters");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int t = ++h->adam_t;
    const double lr_t = (double)lr * std::sqrt(1.0 - std::pow((double)beta2, t)) / (1.0 - std::pow((double)beta1, t));
    Timer tm(h, s, "bwd_adam_repack");
    hipLaunchKernelGGL(k_adam, dim3(1024), dim3(256), 0, s, W(h, "Wflat"), W(h, "Gflat"), W(h, "Mflat"), W(h, "Vflat"), h->n_params,
                       (float)lr_t, beta1, beta2, eps);
    return repack(h, s);
}

// Optimiser state for checkpoints: the Adam moments are the workspace tensors "Mflat" / "Vflat" (desire_device_buffer; same flat
// layout as the gradient buffer), the step counter t of the bias correction is read (set = 0) or written (set = 1) here.
extern "C" int desire_adam_state(desire_handle* h, int32_t* step, int set) {
    if (!h || !step) return fail(DESIRE_ERR_ARG, "null argument");
    if (!h->training) return fail(DESIRE_ERR_STATE, "not in training mode");
    if (set) { if (*step < 0) return fail(DESIRE_ERR_ARG, "step must be >= 0"); h->adam_t = *step; }
    else *step = h->adam_t;
    return DESIRE_OK;
}

extern "C" int desire_get_weight(desire_handle* h, const char* name, float* host_out, size_t n, void* stream) {
    if (!h || !name || !host_out) return fail(DESIRE_ERR_ARG, "null argument");
    auto w = h->want_user.find(name);
    if (w == h->want_user.end()) return fail(DESIRE_ERR_ARG, std::string("unknown weight: ") + name);
    if (w->second != n) return fail(DESIRE_ERR_ARG, std::string(name) + ": expected " + std::to_string(w->second) + " values");
    if (h->training) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIPCHK(hipStreamSynchronize(s));
        const WSlot& sl = h->slots.at(name);
        std::vector<float> phys(sl.n);
        HIPCHK(hipMemcpy(phys.data(), W(h, "Wflat") + sl.off, sl.n * sizeof(float), hipMemcpyDeviceToHost));
        desire_extract(h, name, phys.data(), host_out);
        return DESIRE_OK;
    }
    auto it = h->host_w.find(name);
    if (it == h->host_w.end()) return fail(DESIRE_ERR_STATE, std::string("weight not set: ") + name);
    desire_extract(h, name, it->second.data(), host_out);
    return DESIRE_OK;
}

extern "C" int desire_clip_grads(desire_handle* h, float max_norm, float* host_norm_out, void* stream) {
    if (int rc = desire_ready(h)) return rc;
    if (!h->training) return fail(DESIRE_ERR_STATE, "not in training mode");
    if (!(max_norm > 0.f)) return fail(DESIRE_ERR_ARG, "max_norm must be positive");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = W(h, "tn_partial");
    hipLaunchKernelGGL(k_sqsum, dim3(512), dim3(256), 0, s, W(h, "Gflat"), h->n_params, part);
    hipLaunchKernelGGL(k_clip_scale, dim3(512), dim3(256), 0, s, W(h, "Gflat"), h->n_params, part, 512, max_norm, W(h, "loss_out") + 6);
    HIPCHK(hipGetLastError());
    if (host_norm_out) {
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(host_norm_out, W(h, "loss_out") + 6, sizeof(float), hipMemcpyDeviceToHost));
    }
    return DESIRE_OK;
}
