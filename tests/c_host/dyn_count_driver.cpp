// Drives dyn_units of desire_amd/csrc/dyn_count.h (tests/test_dyn_count.py): no ROCm header, no GPU.  One request per line on stdin:
//   in:  worst hint mul has_cnt           out: dyn_units(worst, DynCount{has_cnt ? a device word's address : nullptr, mul, hint})
// The count word is never read on the host (it lives on the device in the library): its address only says that the launch carries one.
// A malformed line ends the driver with a non-zero status.
#include "dyn_count.h"

#include <cstdio>

int main() {
    static const int32_t word = 0;
    int worst, hint, mul, has_cnt, n;
    while ((n = std::scanf("%d %d %d %d", &worst, &hint, &mul, &has_cnt)) == 4) {
        const DynCount d{has_cnt ? &word : nullptr, mul, hint};
        std::printf("%d\n", dyn_units(worst, d));
    }
    return n == EOF ? 0 : 1;
}
