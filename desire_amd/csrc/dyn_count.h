// dyn_count.h -- the count of a launch whose rows are known on the device only, and the grid rule of the launches that stride over their tiles.
// No HIP include: tests/c_host/dyn_count_driver.cpp compiles it with g++ (tests/test_dyn_count.py).
#pragma once
#include <stdint.h>

// A launch whose row count is known on the DEVICE only (DESIRE_FLAG_COMPACT_*, inference: the present agents of a batch / the windows seated in a
// slot class, counted by kernels_compact.hip's scans).  The host sizes the grid -- and picks the kernel variant -- for the worst case and the kernel
// replaces its count by cnt[0] * mul in its first instructions; workgroups beyond it exit before they touch memory.  No read-back, no host wait, the
// call is hipGraph-capturable.  cnt == nullptr (every other launch): the count in the argument block stands.
// hint: a GUESS of cnt[0] (the previous call's count, read from the scans' mapped word without waiting; 0 = none).  It only ever shrinks a GRID: launchers of
// kernels that stride over their tiles size the grid for hint * 1.25 + slack instead of the worst case, and a count above that is still served -- more
// slowly -- by the stride loop (tests/test_gpu_count_hint.py).  The strided launchers:
//   launch_encoder_pair                     k_encoder_pair<64|128|256>
//   launch_deconv2, launch_deconv3          k_deconv2<FWD>, k_deconv3<FWD, 4>
//   launch_deconv2_x6, launch_deconv3_x6    k_deconv2_x6<3>, k_deconv3_x6i<3> -- and their np = 2 forms k_deconv2_x6<2>, k_deconv3_x6i<2>, which a device-side
//                                           count never reaches: np = 2 is the training-mode forward, and training keeps the read-back (cnt == nullptr)
struct DynCount { const int32_t* cnt; int mul; int hint; };
// units (rows / samples / agents) a strided launch is sized for: the worst case in the arguments, or the hinted count with a quarter of slack
inline int dyn_units(int worst, const DynCount& d) {
    if (!d.cnt || d.hint <= 0) return worst;
    const long g = (long)d.hint * d.mul, want = g + g / 4 + 256;
    return (int)(want < (long)worst ? want : (long)worst);
}
