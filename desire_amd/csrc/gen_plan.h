// gen_plan.h -- which kernel family serves each stage of sample generation (desire_encode / desire_sample) and which packed operand it reads,
// decided in one place: gen_plan() and gen_operands() below.  Host code only and free of HIP headers (tests/test_gen_plan.py compiles it with
// g++, and checks every operand a plan reads against the operand table of pack.h); the launchers launch the family they are asked for.
#pragma once
#include "../../include/desire_hip.h"

#include <string>
#include <utility>
#include <vector>

// ---- the shapes the forms are instantiated for ----
// six-product row GEMMs (kernels_x6.hip: k_deconv1_x6 stages the whole [64, K] A tile once; NT n-tiles, four per wave quartet)
inline bool rows_x6_supported(int K, int NT) { return (K % 16) == 0 && K <= 128 && NT % 16 == 0; }
// six-product mask fc (k_mask_x6): one n-tile per wave, 128-column chunks of xhat
inline bool mask_x6_supported(int H, int V) { return (H == 64 || H == 128) && V % 128 == 0; }
// six-product GRU decoder (k_decoder_x6)
inline bool decoder_x6_supported(int H) { return H == 64 || H == 128 || H == 256; }
// plain-bf16 deconv1 (kernels_bf16.hip): whole bf16 k-groups of the latent, at most 512 of them columns
inline bool deconv1_bf16_supported(int L) { return L <= 512 && L % 16 == 0; }

// FP32: the fp32 kernels; BF16 (dims.bf16 = 1): plain bf16 operands; X6 (dims.bf16 = 2 / 3): kernels_x6.hip on three-piece packs
enum class GenForm { FP32, BF16, X6 };
enum class GenStage { ENC_X, ENC_Y, CONV2, CONV3, DECONV1, DECONV2, DECONV3, DECONV4, MASK, DECODER };

// The packed matrix operand(s) a stage reads under a form (b: the second one of a GRU, else nullptr); a form a stage does not have: {nullptr, nullptr}.
// DECONV4 has no packed fp32 operand: FP32 names its raw taps (k_deconv4_tp), BF16 the tap-product pack of the fused deconv3 + deconv4 kernel.
struct GenOps { const char* a; const char* b; };
inline GenOps gen_operands(GenStage st, GenForm f) {
    static const GenOps table[][3] = {
        /* ENC_X   */ {{"enc_x/Whg", "enc_x/Whc"}, {"enc_x/Whg16", "enc_x/Whc16"}, {nullptr, nullptr}},
        /* ENC_Y   */ {{"enc_y/Whg", "enc_y/Whc"}, {"enc_y/Whg16", "enc_y/Whc16"}, {nullptr, nullptr}},
        /* CONV2   */ {{"vae_enc/conv2/W", nullptr}, {"vae_enc/conv2/W16", nullptr}, {nullptr, nullptr}},
        /* CONV3   */ {{"vae_enc/conv3/W", nullptr}, {"vae_enc/conv3/W16", nullptr}, {nullptr, nullptr}},
        /* DECONV1 */ {{"vae_dec/deconv1/W", nullptr}, {"vae_dec/deconv1/W16", nullptr}, {"vae_dec/deconv1/W6", nullptr}},
        /* DECONV2 */ {{"vae_dec/deconv2/W", nullptr}, {"vae_dec/deconv2/W16", nullptr}, {"vae_dec/deconv2/W6", nullptr}},
        /* DECONV3 */ {{"vae_dec/deconv3/W", nullptr}, {"vae_dec/deconv3/W16", nullptr}, {"vae_dec/deconv3/W6", nullptr}},
        /* DECONV4 */ {{"vae_dec/deconv4/raw", nullptr}, {"vae_dec/deconv4/W16", nullptr}, {nullptr, nullptr}},
        /* MASK    */ {{"mask/W", nullptr}, {"mask/W16", nullptr}, {"mask/W6", nullptr}},
        /* DECODER */ {{"dec/Whg", "dec/Whc"}, {"dec/Whg16", "dec/Whc16"}, {"dec/Whg6", "dec/Whc6"}},
    };
    return table[(int)st][(int)f];
}

struct GenPlan {
    GenForm encoder = GenForm::FP32, conv23 = GenForm::FP32;              // the encoder stack: both GRU encoders; conv2 and conv3
    GenForm deconv1 = GenForm::FP32, deconv2 = GenForm::FP32, deconv3 = GenForm::FP32, mask = GenForm::FP32, decoder = GenForm::FP32;     // the sample stack
    bool fuse34 = false;                   // bf16 deconv3 + deconv4 in one kernel, d3 never written
    int np = 3;                            // pieces per operand of the X6 stages: 2 = the training forward under DESIRE_FLAG_TRAIN_FWD_3P (three products)
    bool batch_stats = false;              // dims.bn_mode != 0: linear epilogue, then a normalise + activate pass (fp32 stages only)
    int wgrad_pieces = 0;                  // backward: bf16 pieces per operand of the weight-gradient reductions (0: fp32)
    bool dgrad_split = false;              // backward: split-bf16 operands in the two large data-gradient convolutions
    GenForm deconv4() const { return fuse34 ? GenForm::BF16 : GenForm::FP32; }
    // every operand of gen_operands the plan reads (the encoder stack's as with dims.posterior = 1)
    std::vector<std::string> needs() const {
        const std::pair<GenStage, GenForm> stages[] = {
            {GenStage::ENC_X, encoder}, {GenStage::ENC_Y, encoder}, {GenStage::CONV2, conv23}, {GenStage::CONV3, conv23}, {GenStage::DECONV1, deconv1},
            {GenStage::DECONV2, deconv2}, {GenStage::DECONV3, deconv3}, {GenStage::DECONV4, deconv4()}, {GenStage::MASK, mask}, {GenStage::DECODER, decoder}};
        std::vector<std::string> n;
        for (const auto& s : stages) {
            const GenOps o = gen_operands(s.first, s.second);
            n.push_back(o.a);
            if (o.b) n.push_back(o.b);
        }
        return n;
    }
};

// The plan of a handle with dims d (d.H: the physical hidden width, as in pack.h) and V = S * S mask pixels, in inference or training mode
inline GenPlan gen_plan(const desire_dims& d, bool training, int V) {
    GenPlan p;
    const bool b16 = d.bf16 == 1;
    // six-product sample generation (the fp32 kernels' accuracy class on the bf16 matrix pipe): dims.bf16 = 3, and dims.bf16 = 2 as well -- two-piece
    // operands are an IOC-kernel matter (split operands: sample generation must not move Y0 by more than fp32 rounding) -- in
    // training unless dims.train_fp32_mask holds it back (bit 8); never with batch statistics or the reference's own graph
    const bool x6 = ((d.bf16 == 3 && !training) || (d.bf16 == 2 && (!training || !(d.train_fp32_mask & 8)))) && d.bn_mode == 0 && !d.ref_compat;
    auto form = [&](bool b16_served, bool x6_served) { return b16 && b16_served ? GenForm::BF16 : x6 && x6_served ? GenForm::X6 : GenForm::FP32; };
    p.encoder = p.conv23 = form(true, false);
    p.deconv1 = form(deconv1_bf16_supported(d.L), rows_x6_supported(d.L, 64));
    p.deconv2 = p.deconv3 = form(true, true);
    // (the six-product form of the deconv3 + deconv4 fusion was measured and dropped: 15.4 ms against 11.9 + 2.5 for the two kernels -- the tap
    //  products cost the contracting waves more than the d3 pass did)
    p.fuse34 = b16 && !(d.flags & DESIRE_FLAG_NO_FUSE34);
    p.mask = form(true, mask_x6_supported(d.H, V));
    p.decoder = form(true, decoder_x6_supported(d.H));
    p.np = training && (d.flags & DESIRE_FLAG_TRAIN_FWD_3P) ? 2 : 3;
    p.batch_stats = d.bn_mode != 0;
    // the training step under dims.bf16 = 2 uses split operands wherever dims.train_fp32_mask does not hold them back (1: weight-gradient
    // reductions, 2: data-gradient convolutions; 4, the IOC BPTT: ioc_plan.h)
    p.wgrad_pieces = d.bf16 == 2 && !(d.train_fp32_mask & 1) ? 2 : 0;
    p.dgrad_split = d.bf16 == 2 && !(d.train_fp32_mask & 2);
    return p;
}
