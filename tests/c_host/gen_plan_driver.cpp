// Reads one case per line from stdin and prints the sample-generation plan of desire_amd/csrc/gen_plan.h for it (tests/test_gen_plan.py):
//   in:  bf16 training flags train_fp32_mask bn_mode ref_compat H L V
//   out: encoder conv23 deconv1 deconv2 deconv3 mask decoder fuse34 np batch_stats wgrad_pieces dgrad_split
// gen_plan_driver needs: instead, every operand the plan reads with the number of times the operand table of pack.h (same dims) holds it: name=count ...
#include "gen_plan.h"
#include "pack.h"

#include <cstdio>
#include <cstring>

static const char* form_name(GenForm f) { return f == GenForm::FP32 ? "FP32" : f == GenForm::BF16 ? "BF16" : "X6"; }

int main(int argc, char** argv) {
    const bool needs = argc > 1 && !std::strcmp(argv[1], "needs");
    int bf16, training, flags, mask, bn_mode, ref_compat, H, L, V;
    while (std::scanf("%d %d %d %d %d %d %d %d %d", &bf16, &training, &flags, &mask, &bn_mode, &ref_compat, &H, &L, &V) == 9) {
        desire_dims d{};
        d.n_scenes = 1; d.mno = 32; d.K = 2; d.T_obs = 4; d.T_pred = 6; d.C = 32; d.E_v = 16; d.grid_size = 4;
        d.bf16 = bf16; d.flags = flags; d.train_fp32_mask = mask; d.bn_mode = bn_mode; d.ref_compat = ref_compat; d.H = H; d.L = L;
        const GenPlan p = gen_plan(d, training != 0, V);
        if (!needs) {
            std::printf("%s %s %s %s %s %s %s %d %d %d %d %d\n", form_name(p.encoder), form_name(p.conv23), form_name(p.deconv1), form_name(p.deconv2),
                        form_name(p.deconv3), form_name(p.mask), form_name(p.decoder), p.fuse34, p.np, p.batch_stats, p.wgrad_pieces, p.dgrad_split);
            continue;
        }
        const std::vector<pack::Operand> table = pack::operands(d, V, d.grid_size * d.grid_size);
        for (const std::string& n : p.needs()) {
            int count = 0;
            for (const pack::Operand& o : table) count += o.name == n;
            std::printf("%s=%d ", n.c_str(), count);
        }
        std::printf("\n");
    }
    return 0;
}
