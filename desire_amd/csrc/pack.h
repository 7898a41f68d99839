// pack.h -- the weights of a handle and every device operand built from them, described in one table: operands() below.  An entry names
// its source weight, where element B(k, n) of each block lives in it (View), the MFMA fragment order the kernels read and the encoding.
// From an entry comes its gather map (per operand element: 1 + index in the source weight, 0 = zero), and from the map both the host
// pack (api_pack.hip: gather, encode, upload) and the device repack of the training step (train.hip: the same map plus the weight's offset
// in the flat master buffer).  Host code only, no ROCm header: tests/c_host/pack_driver.cpp compiles it with g++, and
// tests/test_pack.py pins every operand's bytes and map against tests/golden/pack_digests.json.
#pragma once
#include "../../include/desire_hip.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace pack {

// ---- the weights: name -> element count at hidden width H (V = S * S mask pixels, B = social bins) ----
inline void weight_shapes(const desire_dims& d, int H, int V, int B, std::map<std::string, size_t>& s) {
    const int L = d.L;
    const int E = d.E_v + d.C + H;
    auto gru = [&](const std::string& p, int n_in) {
        s[p + "/gates/kernel"] = (size_t)(n_in + H) * 2 * H;
        s[p + "/gates/bias"] = 2 * H;
        s[p + "/candidate/kernel"] = (size_t)(n_in + H) * H;
        s[p + "/candidate/bias"] = H;
    };
    auto bn = [&](const std::string& p, int c) {
        for (const char* n : {"beta", "gamma", "moving_mean", "moving_var"}) s[p + "/bn/" + n] = c;
    };
    gru("enc_x", 2); gru("enc_y", 2);
    s["fc_c/w"] = (size_t)2 * H * V; s["fc_c/b"] = V;
    struct CL { const char* n; int k, ci, co; };
    for (CL c : {CL{"conv1", 5, 1, 32}, CL{"conv2", 5, 32, 64}, CL{"conv3", 5, 64, 128}}) {
        const std::string p = std::string("vae_enc/") + c.n;
        s[p + "/w"] = (size_t)c.k * c.k * c.ci * c.co; s[p + "/b"] = c.co; bn(p, c.co);
    }
    s["vae_enc/fc/w"] = (size_t)2048 * 2 * L; s["vae_enc/fc/b"] = 2 * L;
    for (CL c : {CL{"deconv1", 4, L, 128}, CL{"deconv2", 5, 128, 64}, CL{"deconv3", 5, 64, 32}, CL{"deconv4", 5, 32, 1}}) {
        const std::string p = std::string("vae_dec/") + c.n;
        s[p + "/w"] = (size_t)c.k * c.k * c.ci * c.co; s[p + "/b"] = c.co; bn(p, c.co);
    }
    s["mask_fc/w"] = (size_t)V * H; s["mask_fc/b"] = H;
    gru("dec", H);
    s["head/w"] = 2 * H; s["head/b"] = 2;
    s["ioc/vel_fc/w"] = 2 * d.E_v; s["ioc/vel_fc/b"] = d.E_v;
    s["ioc/social_fc/w"] = (size_t)B * H * H; s["ioc/social_fc/b"] = H;
    gru("ioc", E);
    s["ioc/score/w"] = H; s["ioc/score/b"] = 1;
    s["ioc/reg/w"] = (size_t)H * 2 * d.T_pred; s["ioc/reg/b"] = 2 * d.T_pred;
    s["scene_cnn/conv1/w"] = 25 * 3 * 16; s["scene_cnn/conv1/b"] = 16;
    s["scene_cnn/conv2/w"] = 25 * 16 * 32; s["scene_cnn/conv2/b"] = 32;
    s["scene_cnn/conv3/w"] = (size_t)25 * 32 * d.C; s["scene_cnn/conv3/b"] = d.C;
    s["temporal/w"] = (size_t)d.T_obs * 2 * 100; s["temporal/b"] = 200;
    s["gauss_head/w"] = (size_t)H * 5; s["gauss_head/b"] = 5;       // sample()'s 5-wide output layer (model/model.py:315-321,445-449)
}

// the conv layers whose batch-norm is folded into <layer>/scale and <layer>/shift (the training step refolds the shift: train.hip)
constexpr const char* conv_layers[] = {"vae_enc/conv1", "vae_enc/conv2", "vae_enc/conv3", "vae_dec/deconv1", "vae_dec/deconv2",
                                       "vae_dec/deconv3", "vae_dec/deconv4"};

// frozen batch-norm + bias -> (scale, shift); float64 then one rounding (desire_amd/spec.py:fold_bn)
inline void fold_bn(const std::vector<float>& g, const std::vector<float>& be, const std::vector<float>& mu, const std::vector<float>& var,
                    const std::vector<float>& b, std::vector<float>& scale, std::vector<float>& shift) {
    scale.resize(g.size()); shift.resize(g.size());
    for (size_t i = 0; i < g.size(); ++i) {
        const double sc = (double)g[i] / std::sqrt((double)var[i] + 1e-3);
        scale[i] = (float)sc;
        shift[i] = (float)((double)be[i] + sc * ((double)b[i] - (double)mu[i]));
    }
}

// ---- where the elements come from ----
// Block s of `count` (the 25 taps of a 5x5 conv, the social bins) is a K x N matrix B_s(k, n) = w[s * block + base + k * sk + n * sn] for k < Kv
// and n among a column segment's first nv columns, zero elsewhere.  The N axis is a concatenation of column segments with a base each.
struct Cols { int n, nv; size_t base; };
struct View {
    int K = 0, Kv = 0; size_t sk = 0, sn = 0;
    std::vector<Cols> cols;
    int count = 1; size_t block = 0;
    int N() const { int n = 0; for (const Cols& c : cols) n += c.n; return n; }
    // The index splits into a k part and an n part, tabulated once per view (with room for the padding slots of every fragment order):
    // element (s, k, n) is w[s * block + k[k] + n[n] - 2] when both parts are non-zero, and zero otherwise
    struct Lut { std::vector<uint32_t> k, n; };
    Lut lut() const {
        Lut t;
        t.k.assign((size_t)(K + 31) / 32 * 32, 0); t.n.assign((size_t)(N() + 31) / 32 * 32, 0);
        for (int k = 0; k < Kv; ++k) t.k[k] = (uint32_t)(k * sk + 1);
        int n0 = 0;
        for (const Cols& c : cols) {
            for (int j = 0; j < c.nv; ++j) t.n[n0 + j] = (uint32_t)(c.base + j * sn + 1);
            n0 += c.n;
        }
        return t;
    }
    View pad_k(int K_) const { View v = *this; v.K = K_; return v; }                       // zero rows up to K_
    View valid_n(int nv) const { View v = *this; v.cols[0].nv = nv; return v; }            // only the first nv columns exist
};
inline View rows(int K, int N, int row0 = 0) { return View{K, K, (size_t)N, 1, {{N, N, (size_t)row0 * N}}}; }       // B(k, n) = w[(row0 + k) * N + n]
inline View rowsT(int K, int N, int row0 = 0) { return View{K, K, 1, (size_t)K, {{N, N, (size_t)row0 * K}}}; }      // transposed: B(k, n) = w[(row0 + n) * K + k]
inline View hcat(View a, const View& b) { a.cols.insert(a.cols.end(), b.cols.begin(), b.cols.end()); return a; }  // [a | b] along n (same K and strides)
inline View stack(View v, int count) { v.count = count; v.block = (size_t)v.K * v.N(); return v; }                  // `count` consecutive K x N blocks
inline View taps(const View& v) { return stack(v, 25); }    // conv weights [tap][ci][co] (rows) or transposed-conv weights [tap][co][ci] (rowsT)

// ---- the fragment orders: put(k, n) is called once per slot, in slot order (k >= K or n >= N: the slot is padding) ----
// fp32, v_mfma_f32_32x32x2_f32: out[((nt*G + g)*64 + lane)*4 + i] = B(k = 8g + 4*(lane>>5) + i, n = 32nt + (lane&31)), G = ceil(K/8), nt < ceil(N/32)
template <class F> void order_f32(int K, int N, F&& put) {
    const int G = (K + 7) / 8, NT = (N + 31) / 32;
    for (int nt = 0; nt < NT; ++nt)
        for (int g = 0; g < G; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 4; ++i) put(8 * g + 4 * (lane >> 5) + i, nt * 32 + (lane & 31));
}
// The k of slot (g, hi = lane>>5, e) of the bf16 order.  lin: plain k order.  chain: group g = 2*hb + g2 holds hidden 32*hb + rowmap(8*g2 + e, hi),
// the accumulator row a lane of the pooling MFMA owns (rowmap(r, hi) = (r&3) + 8*(r>>2) + 4*hi), so that a product chains into the next
inline int kmap_lin(int g, int hi, int e) { return 16 * g + 8 * hi + e; }
inline int kmap_chain(int g, int hi, int e) { const int hb = g >> 1, r = 8 * (g & 1) + e; return 32 * hb + (r & 3) + 8 * (r >> 2) + 4 * hi; }
// bf16, v_mfma_f32_32x32x16_bf16: out[((nt*G + g)*64 + lane)*8 + e] = B(k = kmap(g, lane>>5, e), n = 32nt + (lane&31)), G = ceil(K/16), nt < ceil(N/32)
template <class F> void order_bf16(int K, int N, int (*kmap)(int, int, int), F&& put) {
    const int G = (K + 15) / 16, NT = (N + 31) / 32;
    for (int nt = 0; nt < NT; ++nt)
        for (int g = 0; g < G; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) put(kmap(g, lane >> 5, e), nt * 32 + (lane & 31));
}
// fp32, 16x16x4 tiles (row-compacted pooling): out[((ct*G + g)*64 + lane)*4 + j] = B(k = 16g + 4*(lane>>4) + j, n = 16ct + (lane&15)), G = ceil(K/16),
// ct < ceil(N/16)
template <class F> void order_16x16x4(int K, int N, F&& put) {
    const int G = (K + 15) / 16, CT = (N + 15) / 16;
    for (int ct = 0; ct < CT; ++ct)
        for (int g = 0; g < G; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) put(16 * g + 4 * (lane >> 4) + j, 16 * ct + (lane & 15));
}
enum class Order { RAW, F32, BF16_LIN, BF16_CHAIN, F32_16x16x4 };      // RAW: the source weight as it is
template <class F> void order_slots(Order o, int K, int N, F&& put) {
    switch (o) {
        case Order::F32: order_f32(K, N, put); break;
        case Order::BF16_LIN: order_bf16(K, N, kmap_lin, put); break;
        case Order::BF16_CHAIN: order_bf16(K, N, kmap_chain, put); break;
        case Order::F32_16x16x4: order_16x16x4(K, N, put); break;
        case Order::RAW: break;
    }
}

// ---- the encodings ----
inline uint16_t bf16_rne(float f) {
    uint32_t u; std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t b) { const uint32_t u = (uint32_t)b << 16; float f; std::memcpy(&f, &u, 4); return f; }
// F32: one float per slot.  BF16: one bf16 (RNE) per slot.  SPLIT2 / SPLIT3: [p0 | p1 (| p2)], n bf16 each, piece p = bf16 of what the earlier
// pieces left (each subtraction exact in fp32; three pieces hold an fp32 value exactly).  16-bit encodings travel as floats holding two each.
enum class Enc { F32, BF16, SPLIT2, SPLIT3 };
inline size_t pieces(Enc e) { return e == Enc::SPLIT2 ? 2 : e == Enc::SPLIT3 ? 3 : e == Enc::BF16 ? 1 : 0; }      // bf16 per slot (0: fp32)

// ---- the table ----
enum class Kind { GATHER, SCALE, SHIFT };                   // SCALE / SHIFT: fold_bn of the layer `src`, not a gather
struct Operand { std::string name, src; View v; Order order = Order::RAW; Enc enc = Enc::F32; Kind kind = Kind::GATHER; };

// Every device operand of a handle with dims d (d.H: the physical hidden width), in upload order
inline std::vector<Operand> operands(const desire_dims& d, int V, int B) {
    const int H = d.H, L = d.L, T2 = 2 * d.T_pred, E = d.E_v + d.C + H;
    const int xr = d.E_v + d.C;                              // first e_r row of the IOC GRU kernels
    const bool b16 = d.bf16 == 1, x3 = d.bf16 == 2, x36 = d.bf16 == 2 || d.bf16 == 3;
    const Enc e16 = b16 ? Enc::BF16 : d.bf16 == 3 ? Enc::SPLIT3 : Enc::SPLIT2;       // "<name>16" operands: bf16 (kernels_bf16.hip) or split pieces (kernels_x3.hip)
    std::vector<Operand> t;
    auto raw = [&](const std::string& name, const std::string& src) { t.push_back({name, src, View{}}); };
    auto f32 = [&](const std::string& name, const std::string& src, const View& v, Order o = Order::F32) { t.push_back({name, src, v, o}); };
    auto w16 = [&](bool exists, const std::string& name, const std::string& src, const View& v, Enc e, Order o = Order::BF16_LIN) {
        if (exists) t.push_back({name, src, v, o, e});
    };
    auto bins = [&](const View& v) { return stack(v, B); };  // social weights [bin][H][H]
    // GRUs.  h-blocks of the kernels [x rows | h rows][gate columns]; W?T_*: the transposed blocks of the backward data-gradient contractions
    for (const std::string s : {"enc_x", "enc_y"}) {
        const std::string gk = s + "/gates/kernel", ck = s + "/candidate/kernel";
        raw(s + "/gk", gk); raw(s + "/gb", s + "/gates/bias"); raw(s + "/ck", ck); raw(s + "/cb", s + "/candidate/bias");
        f32(s + "/Whg", gk, rows(H, 2 * H, 2)); f32(s + "/Whc", ck, rows(H, H, 2));
        f32(s + "/WgT_h", gk, rowsT(2 * H, H, 2)); f32(s + "/WcT_h", ck, rowsT(H, H, 2));
        w16(b16, s + "/Whg16", gk, rows(H, 2 * H, 2), Enc::BF16); w16(b16, s + "/Whc16", ck, rows(H, H, 2), Enc::BF16);
    }
    {
        const std::string gk = "dec/gates/kernel", ck = "dec/candidate/kernel";
        raw("dec/gb", "dec/gates/bias"); raw("dec/cb", "dec/candidate/bias");
        f32("dec/Wxg", gk, rows(H, 2 * H, 0)); f32("dec/Whg", gk, rows(H, 2 * H, H));
        f32("dec/Wxc", ck, rows(H, H, 0)); f32("dec/Whc", ck, rows(H, H, H));
        f32("dec/WgT_x", gk, rowsT(2 * H, H, 0)); f32("dec/WgT_h", gk, rowsT(2 * H, H, H));
        f32("dec/WcT_x", ck, rowsT(H, H, 0)); f32("dec/WcT_h", ck, rowsT(H, H, H));
        w16(b16, "dec/Whg16", gk, rows(H, 2 * H, H), Enc::BF16); w16(b16, "dec/Whc16", ck, rows(H, H, H), Enc::BF16);
        // three pieces for the sample-generation kernels (kernels_x6.hip): dims.bf16 = 3, and the training-mode forward of dims.bf16 = 2
        w16(x36, "dec/Whg6", gk, rows(H, 2 * H, H), Enc::SPLIT3); w16(x36, "dec/Whc6", ck, rows(H, H, H), Enc::SPLIT3);
    }
    raw("head/w", "head/w"); raw("head/b", "head/b");
    {   // IOC GRU: input rows [e_v | scene features | e_r | h]
        const std::string gk = "ioc/gates/kernel", ck = "ioc/candidate/kernel", wr = "ioc/reg/w", wsoc = "ioc/social_fc/w";
        raw("ioc/gb", "ioc/gates/bias"); raw("ioc/cb", "ioc/candidate/bias");
        f32("ioc/Wg", gk, rows(E + H, 2 * H)); f32("ioc/Wc", ck, rows(E + H, H));
        const View gT_h = rowsT(2 * H, H, E), gT_er = rowsT(2 * H, H, xr), gT_ev = rowsT(2 * H, 32).valid_n(d.E_v);
        const View cT_h = rowsT(H, H, E), cT_er = rowsT(H, H, xr), cT_ev = rowsT(H, 32).valid_n(d.E_v);
        f32("ioc/WgT_h", gk, gT_h); f32("ioc/WgT_er", gk, gT_er); f32("ioc/WgT_ev", gk, gT_ev);
        f32("ioc/WcT_h", ck, cT_h); f32("ioc/WcT_er", ck, cT_er); f32("ioc/WcT_ev", ck, cT_ev);
        f32("ioc/WrT", wr, rowsT(T2, H).pad_k((T2 + 7) / 8 * 8));
        f32("ioc/WsT", wsoc, bins(rowsT(H, H))); f32("ioc/WsT_c", wsoc, bins(rowsT(H, H)), Order::F32_16x16x4);     // _c: k_ioc_bwd's row-compacted dpool
        w16(d.bf16 != 0, "ioc/Wg16", gk, rows(E + H, 2 * H), e16); w16(d.bf16 != 0, "ioc/Wc16", ck, rows(E + H, H), e16);
        w16(d.bf16 != 0, "ioc/Wreg16", wr, rows(H, T2), e16);
        w16(d.bf16 != 0, "ioc/Wsoc16", wsoc, bins(rows(H, H)), e16, Order::BF16_CHAIN);
        // the step-wise split kernel (k_ioc_step<.., NP>) pools into a plain fp32 tile: the social weights in plain k order as well
        w16(x36 && (d.mno > 128 || H == 256), "ioc/Wsoc16l", wsoc, bins(rows(H, H)), e16);
        // k_ioc_bwd_x3 (training under dims.bf16 = 2): n-tiles [h columns | e_r columns | one e_v tile]
        w16(x3, "ioc/WcT16", ck, hcat(hcat(cT_h, cT_er), cT_ev), Enc::SPLIT2); w16(x3, "ioc/WgT16", gk, hcat(hcat(gT_h, gT_er), gT_ev), Enc::SPLIT2);
        w16(x3, "ioc/WsT16", wsoc, bins(rowsT(H, H)), Enc::SPLIT2);
        raw("ioc/vel_w", "ioc/vel_fc/w"); raw("ioc/vel_b", "ioc/vel_fc/b");
        f32("ioc/Wsoc", wsoc, bins(rows(H, H))); f32("ioc/Wsoc_c", wsoc, bins(rows(H, H)), Order::F32_16x16x4);     // _c: k_ioc<..., CP>
        raw("ioc/soc_b", "ioc/social_fc/b"); raw("ioc/score_w", "ioc/score/w"); raw("ioc/score_b", "ioc/score/b");
        f32("ioc/Wreg", wr, rows(H, T2)); raw("ioc/reg_b", "ioc/reg/b");
    }
    // dense layers; *T: operands of the backward data-gradient passes (the forward kernels run with swapped roles)
    f32("fc_c/W", "fc_c/w", rows(2 * H, V)); f32("fc_c/WT", "fc_c/w", rowsT(V, 2 * H)); raw("fc_c/b", "fc_c/b");
    f32("vae_enc/fc/W", "vae_enc/fc/w", rows(2048, 2 * L)); f32("vae_enc/fc/WT", "vae_enc/fc/w", rowsT(2 * L, 2048)); raw("vae_enc/fc/b", "vae_enc/fc/b");
    f32("mask/W", "mask_fc/w", rows(V, H)); f32("mask/WT", "mask_fc/w", rowsT(H, V)); raw("mask/b", "mask_fc/b");
    w16(b16, "mask/W16", "mask_fc/w", rows(V, H), Enc::BF16); w16(x36, "mask/W6", "mask_fc/w", rows(V, H), Enc::SPLIT3);
    // conv stack: folded batch-norm (its parameters as well when the kernels take batch statistics), then the taps
    for (const std::string n : conv_layers) {
        t.push_back({n + "/scale", n, View{}, Order::RAW, Enc::F32, Kind::SCALE}); t.push_back({n + "/shift", n, View{}, Order::RAW, Enc::F32, Kind::SHIFT});
        if (d.bn_mode != 0) { raw(n + "/gamma", n + "/bn/gamma"); raw(n + "/beta", n + "/bn/beta"); }
    }
    raw("vae_enc/conv1/raw", "vae_enc/conv1/w"); raw("vae_dec/deconv4/raw", "vae_dec/deconv4/w");
    struct Conv { const char* layer; int ci, co; bool tr; };  // forward conv [tap][ci][co]; transposed conv [tap][co][ci], B(k = ci, n = co)
    for (Conv c : {Conv{"vae_enc/conv2", 32, 64, false}, Conv{"vae_enc/conv3", 64, 128, false}, Conv{"vae_dec/deconv2", 128, 64, true},
                   Conv{"vae_dec/deconv3", 64, 32, true}}) {
        const std::string p = c.layer, w = p + "/w";
        const View fwd = taps(c.tr ? rowsT(c.ci, c.co) : rows(c.ci, c.co)), bwd = taps(c.tr ? rows(c.co, c.ci) : rowsT(c.co, c.ci));     // bwd: the other kind of conv, co -> ci
        f32(p + "/W", w, fwd); f32(p + "/Wbwd", w, bwd);
        w16(b16, p + "/W16", w, fwd, Enc::BF16);
        w16(x36 && c.tr, p + "/W6", w, fwd, Enc::SPLIT3);
        w16(x3 && c.tr, p + "/Wbwd16", w, bwd, Enc::SPLIT2);  // the two large data-gradient convolutions of the CVAE decoder (kernels_bwd_x3.hip)
    }
    {   // deconv1 as a GEMM: B(k = ci, n = (ky*4 + kx)*128 + co) = w[n*L + k]
        const std::string w1 = "vae_dec/deconv1/w";
        f32("vae_dec/deconv1/W", w1, rowsT(L, 2048)); f32("vae_dec/deconv1/WT", w1, rows(2048, L));
        w16(b16, "vae_dec/deconv1/W16", w1, rowsT(L, 2048), Enc::BF16); w16(x36, "vae_dec/deconv1/W6", w1, rowsT(L, 2048), Enc::SPLIT3);
    }
    // deconv4 as "tap products": A[m = tap][k = channel, chain order] = w4[tap][0][channel]
    w16(b16, "vae_dec/deconv4/W16", "vae_dec/deconv4/w", rowsT(32, 32).valid_n(25), Enc::BF16, Order::BF16_CHAIN);
    for (const char* n : {"scene_cnn/conv1/w", "scene_cnn/conv1/b", "scene_cnn/conv2/w", "scene_cnn/conv2/b", "scene_cnn/conv3/w",
                          "scene_cnn/conv3/b", "temporal/w", "temporal/b", "gauss_head/w", "gauss_head/b"}) raw(n, n);
    return t;
}

// slots of a gather operand whose source weight has n_src elements
inline size_t slots(const Operand& o, size_t n_src) {
    size_t n = 0;
    order_slots(o.order, o.v.K, o.v.N(), [&](int, int) { ++n; });
    return o.order == Order::RAW ? n_src : n * o.v.count;
}
inline size_t bytes(const Operand& o, size_t n_src) {
    const size_t n = slots(o, n_src), np = pieces(o.enc);
    return np ? (np * n + (np * n & 1)) / 2 * 4 : n * 4;
}
// put(j) for every slot of a gather operand, in order: j = 1 + index in the source weight, 0 = zero.  The one enumeration behind both consumers:
template <class F> void for_each_slot(const Operand& o, size_t n_src, F&& put) {
    if (o.order == Order::RAW) for (size_t i = 0; i < n_src; ++i) put((uint32_t)i + 1);
    const View::Lut t = o.v.lut();
    for (int s = 0; s < o.v.count; ++s) {
        const uint32_t b = (uint32_t)(s * o.v.block) - 1;    // (unsigned: b + k part + n part = 1 + index)
        order_slots(o.order, o.v.K, o.v.N(), [&](int k, int n) { const uint32_t a = t.k[k], c = t.n[n]; put(a && c ? b + a + c : 0); });
    }
}
// the device repack map (train.hip adds the source weight's offset in the flat buffers) ...
inline std::vector<uint32_t> gather_map(const Operand& o, size_t n_src) {
    std::vector<uint32_t> m(slots(o, n_src));
    uint32_t* p = m.data();
    for_each_slot(o, n_src, [&](uint32_t j) { *p++ = j; });
    return m;
}
// ... and the host pack: gather and encode
inline void encode(const Operand& o, const std::vector<float>& w, std::vector<float>& out) {
    const size_t n = slots(o, w.size()), np = pieces(o.enc);
    if (!np) {
        out.resize(n);
        float* p = out.data();
        for_each_slot(o, w.size(), [&](uint32_t j) { *p++ = j ? w[j - 1] : 0.f; });
        return;
    }
    std::vector<uint16_t> b(np * n + (np * n & 1));
    size_t i = 0;
    for_each_slot(o, w.size(), [&](uint32_t j) {
        float r = j ? w[j - 1] : 0.f;
        for (size_t pc = 0; pc < np; ++pc) {
            b[pc * n + i] = bf16_rne(r);
            r -= bf16_to_f32(b[pc * n + i]);
        }
        ++i;
    });
    out.resize(b.size() / 2);
    std::memcpy(out.data(), b.data(), out.size() * 4);
}
// one past the last element of its source that an operand reads
inline size_t reach(const Operand& o, size_t n_src) {
    if (o.order == Order::RAW) return n_src;
    const View::Lut t = o.v.lut();
    uint32_t k = 0, n = 0;
    for (uint32_t x : t.k) k = x > k ? x : k;
    for (uint32_t x : t.n) n = x > n ? x : n;
    return k && n ? (o.v.count - 1) * o.v.block + k + n - 1 : 0;
}

// The bytes of one operand.  find(name): the weight as a const std::vector<float>*, nullptr when it is not set.  Returns "" or what is wrong.
template <class Find> std::string build(const Operand& o, Find&& find, std::vector<float>& out) {
    if (o.kind != Kind::GATHER) {
        const std::vector<float>* p[5];
        const char* part[5] = {"/bn/gamma", "/bn/beta", "/bn/moving_mean", "/bn/moving_var", "/b"};
        for (int i = 0; i < 5; ++i) {
            p[i] = find(o.src + part[i]);
            if (!p[i] || p[i]->size() != p[0]->size()) return "weight not set: " + o.src + part[i];
        }
        std::vector<float> other;
        if (o.kind == Kind::SCALE) fold_bn(*p[0], *p[1], *p[2], *p[3], *p[4], out, other);
        else fold_bn(*p[0], *p[1], *p[2], *p[3], *p[4], other, out);
        return "";
    }
    const std::vector<float>* w = find(o.src);
    if (!w) return "weight not set: " + o.src;
    if (reach(o, w->size()) > w->size()) return "operand " + o.name + " reads past its source " + o.src;
    encode(o, *w, out);
    return "";
}

}  // namespace pack
