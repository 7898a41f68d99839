// philox_driver.cpp -- desire_amd/csrc/philox.h compiled with g++ (no ROCm header, no GPU) for tests/test_rng_cpu.py.  One request per line of standard input:
//   P c0 c1 c2 c3 k0 k1              -> the four output words of Philox4x32-10 and the bit patterns of the four fp32 normals made of them
//   E draw scene_base scene k slot l -> the four counter words of a latent (scene_base + scene is formed in 32 bits, as the kernels do)
//   F stream_id block                -> the four counter words of a fill block
// Numbers are hexadecimal.  A malformed line ends the program with status 1.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "philox.h"

int main() {
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        uint64_t v[6];
        if (line[0] == 'P' && std::sscanf(line + 1, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, v, v + 1, v + 2, v + 3, v + 4, v + 5) == 6) {
            const Philox4 c = {{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]}};
            const Philox4 x = philox4x32_10(c, (uint32_t)v[4], (uint32_t)v[5]);
            float n[4];
            philox_normal4(x, n);
            uint32_t b[4];
            std::memcpy(b, n, sizeof b);
            std::printf("%08x %08x %08x %08x %08x %08x %08x %08x\n", x.v[0], x.v[1], x.v[2], x.v[3], b[0], b[1], b[2], b[3]);
        } else if (line[0] == 'E' && std::sscanf(line + 1, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, v, v + 1, v + 2, v + 3, v + 4, v + 5) == 6) {
            const Philox4 c = philox_eps_counter((uint32_t)v[0], (uint32_t)v[1] + (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]);
            std::printf("%08x %08x %08x %08x\n", c.v[0], c.v[1], c.v[2], c.v[3]);
        } else if (line[0] == 'F' && std::sscanf(line + 1, "%" SCNx64 " %" SCNx64, v, v + 1) == 2) {
            const Philox4 c = philox_fill_counter((uint32_t)v[0], v[1]);
            std::printf("%08x %08x %08x %08x\n", c.v[0], c.v[1], c.v[2], c.v[3]);
        } else {
            return 1;
        }
    }
    return 0;
}
