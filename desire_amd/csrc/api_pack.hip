// api_pack.hip -- desire_pack_all: every device operand of pack.h's table rebuilt from the handle's host weights and uploaded.  Host code only.
#include "ctx.h"

int desire_pack_all(desire_ctx* h) {
    auto find = [h](const std::string& n) { const auto it = h->host_w.find(n); return it == h->host_w.end() ? nullptr : &it->second; };
    std::vector<float> bytes;
    for (const pack::Operand& o : pack::operands(h->d, h->V, h->B)) {
        const std::string err = pack::build(o, find, bytes);
        if (!err.empty()) return fail(DESIRE_ERR_STATE, err);
        if (desire_upload(h, o.name, bytes)) return fail(DESIRE_ERR_HIP, "weight upload failed: " + o.name);
    }
    HIPCHK(hipDeviceSynchronize());
    return DESIRE_OK;
}
