// Host-only driver of desire_amd/csrc/pack.h for tests/test_pack.py (g++, no ROCm header, no GPU).
//   pack_driver digests bf16 H grid_size L T_pred mno bn_mode   one line per operand: name, bytes, FNV-1a of the bytes, FNV-1a of the device repack
//                                                               map ("-" for the folded scale / shift, which have none)
//                                                               (a further argument names a weight to leave unset: the error text, exit code 1)
//   pack_driver time    bf16 H grid_size L T_pred mno bn_mode   milliseconds to build every operand once
//   pack_driver order   f32|lin|chain|c16 K N                   one line per slot of the fragment order: k * N + n, or -1 for a padding slot
// Weights come from a fixed integer generator (24-bit values / 2^20, exact in fp32 and in three bf16 pieces; moving_var made positive).
#include "pack.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

static uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
static void fill_weight(const std::string& name, std::vector<float>& w) {
    uint32_t s = (uint32_t)fnv1a(name.data(), name.size());
    const bool var = name.size() >= 10 && name.compare(name.size() - 10, 10, "moving_var") == 0;
    for (float& x : w) {
        s = s * 1664525u + 1013904223u;
        x = (float)((int32_t)(s >> 8) - (1 << 23)) / 1048576.f;
        if (var) x = std::fabs(x) + 0.5f;
    }
}

static int order(const std::string& which, int K, int N) {
    const pack::Order o = which == "f32" ? pack::Order::F32 : which == "lin" ? pack::Order::BF16_LIN : which == "chain" ? pack::Order::BF16_CHAIN
                        : which == "c16" ? pack::Order::F32_16x16x4 : pack::Order::RAW;
    if (o == pack::Order::RAW) return 2;
    const pack::Operand op{"order", "w", pack::rows(K, N), o};
    for (uint32_t j : pack::gather_map(op, (size_t)K * N)) std::printf("%ld\n", (long)j - 1);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "order" && argc == 5) return order(argv[2], std::atoi(argv[3]), std::atoi(argv[4]));
    if (!(mode == "digests" && argc == 10) && ((mode != "digests" && mode != "time") || argc != 9)) return 2;
    desire_dims d{};
    d.n_scenes = 1; d.K = 2; d.T_obs = 4; d.S = 32; d.C = 32; d.E_v = 16;
    d.bf16 = std::atoi(argv[2]); d.H = std::atoi(argv[3]); d.grid_size = std::atoi(argv[4]); d.L = std::atoi(argv[5]);
    d.T_pred = std::atoi(argv[6]); d.mno = std::atoi(argv[7]); d.bn_mode = std::atoi(argv[8]);
    const int V = d.S * d.S, B = d.grid_size * d.grid_size;
    std::map<std::string, size_t> want;
    pack::weight_shapes(d, d.H, V, B, want);
    std::map<std::string, std::vector<float>> w;
    std::map<std::string, size_t> off;                       // the flat training layout: name order, each weight padded to 4 floats
    size_t total = 0;
    for (auto& kv : want) {
        w[kv.first].resize(kv.second);
        fill_weight(kv.first, w[kv.first]);
        off[kv.first] = total; total += (kv.second + 3) / 4 * 4;
    }
    if (argc == 10) w.erase(argv[9]);
    auto find = [&](const std::string& n) { const auto it = w.find(n); return it == w.end() ? nullptr : &it->second; };
    std::vector<float> out;
    const auto t0 = std::chrono::steady_clock::now();
    for (const pack::Operand& o : pack::operands(d, V, B)) {
        const std::string err = pack::build(o, find, out);
        if (!err.empty()) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        if (mode == "time") continue;
        std::printf("%s %zu %016llx ", o.name.c_str(), out.size() * 4, (unsigned long long)fnv1a(out.data(), out.size() * 4));
        if (o.kind != pack::Kind::GATHER) { std::printf("-\n"); continue; }
        if (out.size() * 4 != pack::bytes(o, want.at(o.src))) { std::fprintf(stderr, "%s: bytes() disagrees with build()\n", o.name.c_str()); return 1; }
        std::vector<uint32_t> m = pack::gather_map(o, want.at(o.src));
        for (uint32_t& j : m) if (j) j += (uint32_t)off.at(o.src);
        std::printf("%016llx\n", (unsigned long long)fnv1a(m.data(), m.size() * 4));
    }
    if (mode == "time") std::printf("%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
