// reequilibrate.hpp -- launchers of reequilibrate.hip: the device work chip_reequilibrate_problem /
// chip_reequilibrate_bdata add to the passes they reuse (equilibrate.hip's Ruiz loop, the refresh passes of the data
// updates).  Internal to the library: solver.cpp and batch.cpp include it.
#pragma once
#include <hip/hip_runtime.h>

namespace chip {
namespace dev {

// the load pass of one array: dst[i] = v and, when raw != nullptr, raw[i] = v, with v = src[i], or min(src[i], 1e20)
// when cap (b: problemdata.rs:125-127; a NaN stays a NaN, as std::min(v, 1e20) keeps it).  Two entries per lane with
// 16-byte accesses when every pointer is 16-byte aligned, one entry per lane otherwise
void re_load(hipStream_t s, double *dst, double *raw, const double *src, int len, bool cap);
// out[0] = max |v[0 .. len)| over the bit patterns of |x| (exact in any order; a NaN wins; 0 for len == 0): two fixed
// passes.  partials: re_absmax_partials() words
int re_absmax_partials();
void re_absmax(hipStream_t s, const double *v, int len, unsigned long long *partials, double *out);

} // namespace dev
} // namespace chip
