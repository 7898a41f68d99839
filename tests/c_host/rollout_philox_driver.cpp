// rollout_philox_driver.cpp -- the rollout counter of desire_amd/csrc/philox.h compiled with g++ (no ROCm header, no GPU) for
// tests/test_rollout_rng_cpu.py.  One request per line of standard input, numbers hexadecimal:
//   R draw scene_base scene k slot t seed_lo seed_hi -> the four counter words of the step's block (scene_base + scene is formed in 32 bits, as the
//                                                       kernels do), the four output words of that block under the key, and the bit patterns of
//                                                       the four fp32 normals philox_roll4 makes of it
// A malformed line ends the program with status 1.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "philox.h"

int main() {
    static_assert(PHILOX_ROLL == 2u && PHILOX_ROLL != PHILOX_EPS && PHILOX_ROLL != PHILOX_FILL, "c3 of the rollout blocks");
    static_assert(PHILOX_MAX_T == 2048, "steps the rollout packing holds");
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        uint64_t v[8];
        if (line[0] == 'R' && std::sscanf(line + 1, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64,
                                          v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7) == 8) {
            const uint32_t window = (uint32_t)v[1] + (uint32_t)v[2];
            const Philox4 c = philox_roll_counter((uint32_t)v[0], window, (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]);
            const Philox4 x = philox4x32_10(c, (uint32_t)v[6], (uint32_t)v[7]);
            float n[4];
            philox_roll4((uint32_t)v[6], (uint32_t)v[7], (uint32_t)v[0], window, (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], n);
            uint32_t b[4];
            std::memcpy(b, n, sizeof b);
            std::printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", c.v[0], c.v[1], c.v[2], c.v[3], x.v[0], x.v[1], x.v[2], x.v[3],
                        b[0], b[1], b[2], b[3]);
        } else {
            return 1;
        }
    }
    return 0;
}
