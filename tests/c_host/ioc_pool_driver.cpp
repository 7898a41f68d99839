// Reads one request per line from stdin (tests/test_ioc_pool_plan.py) and answers from desire_amd/csrc/ioc_lds.h / ioc_tile.h (the part of
// ioc_tile.h in front of its HIP includes: plain C++):
//   in:  slots H TM           out: ioc_pool_slots(H, TM)  bytes of the AB region behind the slots  IOC_POOL_MAX_BINS
//   in:  src32 <hex mask>     out: ioc_row_source((unsigned)mask)               (-1 = the zero row, -2 = a sum slot, else the neighbour's slot)
//   in:  src64 <hex mask>     out: ioc_row_source((unsigned long long)mask)
//   in:  off code TM LDX E LDB lane15   out: ioc_row_offset(...)
#include "ioc_tile.h"

#include <cstdio>
#include <cstring>

static_assert(ioc_row_source(0u) == IOC_ROW_ZERO && ioc_row_source(0x80000000u) == 31 && ioc_row_source(3u) == IOC_ROW_SUM, "constexpr");

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "slots")) {
            int H, TM;
            if (std::scanf("%d %d", &H, &TM) != 2) return 1;
            const int n = ioc_pool_slots(H, TM);
            std::printf("%d %d %d\n", n, (2 * TM - n) * (H + 4) * 4, IOC_POOL_MAX_BINS);
            continue;
        }
        if (!std::strcmp(cmd, "off")) {
            int code, TM, LDX, E, LDB, l15;
            if (std::scanf("%d %d %d %d %d %d", &code, &TM, &LDX, &E, &LDB, &l15) != 6) return 1;
            std::printf("%d\n", ioc_row_offset(code, TM, LDX, E, LDB, l15));
            continue;
        }
        unsigned long long m;
        if (std::scanf("%llx", &m) != 1) return 1;
        if (!std::strcmp(cmd, "src32")) std::printf("%d\n", ioc_row_source((unsigned)m));
        else if (!std::strcmp(cmd, "src64")) std::printf("%d\n", ioc_row_source(m));
        else return 2;
    }
    return 0;
}
