// reequilibrate.hip -- the device work of chip_reequilibrate_problem / chip_reequilibrate_bdata that no existing pass
// does: the load of the caller's raw P, A, q, b into the handle's arrays (b capped at the reference's infinity, as
// ProblemData::upload caps it at create; for the batch the unscaled copies of q and b in the same pass), and the norm
// of a raw vector.  The Ruiz loop itself is equilibrate.hip's (ProblemData::equilibrate), the refresh of K's store and
// of the L3 copies is the data updates' (problem_update.hip, kktsystem.cpp).
//
// Both passes are streaming and memory bound: grid-stride loops of 256-thread workgroups, no LDS beyond the reduction,
// no atomics.  The maximum is reduced over the bit patterns of |x| in two fixed passes (exact in any order, and the
// bits of a NaN exceed those of +inf, so a NaN propagates), as problem_update.hip's norms are.
#include "dev_common.hpp"
#include "reequilibrate.hpp"

namespace chip {
namespace dev {

namespace {

constexpr int ABSMAX_BLOCKS = 256; // fixed partition of the reduction
constexpr double B_INFINITY = 1e20; // get_infinity (problemdata.rs:125-127)

template <bool CAP> __device__ __forceinline__ double load_value(double v) {
    return CAP && v > B_INFINITY ? B_INFINITY : v; // (std::min(v, 1e20): a NaN stays)
}

// two entries per lane with 16-byte loads and stores when every pointer is 16-byte aligned
template <bool VEC, bool CAP, bool RAW>
__global__ __launch_bounds__(WG) void k_re_load(double *__restrict__ dst, double *__restrict__ raw,
                                                const double *__restrict__ src, int len) {
    if (VEC) {
        const int npair = len >> 1;
        const double2 *s2 = (const double2 *)src;
        double2 *d2 = (double2 *)dst, *r2 = (double2 *)raw;
        for (int p = blockIdx.x * WG + threadIdx.x; p < npair; p += gridDim.x * WG) {
            double2 v = s2[p];
            v.x = load_value<CAP>(v.x);
            v.y = load_value<CAP>(v.y);
            d2[p] = v;
            if (RAW) r2[p] = v;
        }
        if ((len & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            const double v = load_value<CAP>(src[len - 1]);
            dst[len - 1] = v;
            if (RAW) raw[len - 1] = v;
        }
    } else {
        for (int i = blockIdx.x * WG + threadIdx.x; i < len; i += gridDim.x * WG) {
            const double v = load_value<CAP>(src[i]);
            dst[i] = v;
            if (RAW) raw[i] = v;
        }
    }
}

template <bool VEC, bool CAP>
void launch_load(hipStream_t s, double *dst, double *raw, const double *src, int len) {
    const int g = stream_grid(VEC ? (len + 1) / 2 : len);
    if (raw) k_re_load<VEC, CAP, true><<<g, WG, 0, s>>>(dst, raw, src, len);
    else k_re_load<VEC, CAP, false><<<g, WG, 0, s>>>(dst, nullptr, src, len);
}

__global__ __launch_bounds__(WG) void k_re_absmax_partial(const double *__restrict__ v, int len,
                                                          unsigned long long *partials) {
    __shared__ unsigned long long red[WG];
    unsigned long long acc = 0;
    for (int i = blockIdx.x * WG + threadIdx.x; i < len; i += gridDim.x * WG) {
        const unsigned long long b = abs_bits(v[i]);
        acc = b > acc ? b : acc;
    }
    acc = block_max_u64(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}
__global__ __launch_bounds__(WG) void k_re_absmax_final(const unsigned long long *__restrict__ partials, double *out) {
    __shared__ unsigned long long red[WG];
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < ABSMAX_BLOCKS; i += WG) {
        const unsigned long long b = partials[i];
        acc = b > acc ? b : acc;
    }
    acc = block_max_u64(acc, red);
    if (threadIdx.x == 0) out[0] = __longlong_as_double((long long)acc);
}

} // namespace

void re_load(hipStream_t s, double *dst, double *raw, const double *src, int len, bool cap) {
    if (len <= 0) return;
    const bool vec = (((uintptr_t)dst | (uintptr_t)raw | (uintptr_t)src) & 15) == 0;
    if (vec) {
        if (cap) launch_load<true, true>(s, dst, raw, src, len);
        else launch_load<true, false>(s, dst, raw, src, len);
    } else {
        if (cap) launch_load<false, true>(s, dst, raw, src, len);
        else launch_load<false, false>(s, dst, raw, src, len);
    }
}

int re_absmax_partials() { return ABSMAX_BLOCKS; }

void re_absmax(hipStream_t s, const double *v, int len, unsigned long long *partials, double *out) {
    k_re_absmax_partial<<<ABSMAX_BLOCKS, WG, 0, s>>>(v, len, partials);
    k_re_absmax_final<<<1, WG, 0, s>>>(partials, out);
}

} // namespace dev
} // namespace chip
