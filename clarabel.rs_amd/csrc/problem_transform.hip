// problem_transform.hip -- the device reverse of the L4 solver's problem transforms (problem_transform.cpp): the
// original-sized x, s, z written straight from the SCALED internal variables, once per solve.
//
// One lane per output entry, in a grid-stride loop: entries [0, n) are x, entries [n, n + m) are the rows of s and z.
// Each source entry is unscaled with exactly the arithmetic of dev::unscale (equilibrate.hip) before it is summed or
// selected, so the result equals "unscale the internal variables, then apply transform_reverse_host" bit for bit:
//   x[i]  = (x2[i] * d[i]) * sx
//   s src = (s2[k] * einv[k]) * ss,  z src = (z2[k] * e[k]) * sz
// The source lists are walked in order by the lane that owns the row, so no atomics are needed and the sums are
// deterministic.  It is a gather: bound by HBM bandwidth, with 64-bit offsets into the lists.
#include "dev_common.hpp"
#include "problem_transform.hpp"

namespace chip {
namespace dev {

namespace {

__global__ __launch_bounds__(WG) void k_transform_reverse(const int32_t *__restrict__ mode, const int64_t *__restrict__ ptr,
                                                          const int64_t *__restrict__ src, int n, int m, double *xo,
                                                          const double *__restrict__ x2, const double *__restrict__ d,
                                                          double sx, double *so, const double *__restrict__ s2,
                                                          const double *__restrict__ einv, double ss, double *zo,
                                                          const double *__restrict__ z2, const double *__restrict__ e,
                                                          double sz) {
    const int64_t total = (int64_t)n + m;
    for (int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * WG) {
        if (t < n) {
            xo[t] = (x2[t] * d[t]) * sx;
            continue;
        }
        const int64_t i = t - n;
        const int32_t md = mode[i];
        const int64_t a = ptr[i], b = ptr[i + 1];
        double sv = 0.0, zv = 0.0;
        if (md == RV_CONST) {
            sv = 1e20;
        } else if (md == RV_COPY) {
            const int64_t k = src[a];
            sv = (s2[k] * einv[k]) * ss;
            zv = (z2[k] * e[k]) * sz;
        } else if (md == RV_COMPACT) {
            for (int64_t p = a; p < b; p++) {
                const int64_t k = src[p];
                sv += (s2[k] * einv[k]) * ss;
                zv = (z2[k] * e[k]) * sz;
            }
        } else {
            for (int64_t p = a; p < b; p++) {
                const int64_t k = src[p];
                sv += (s2[k] * einv[k]) * ss;
                zv += (z2[k] * e[k]) * sz;
            }
            if (b - a > 1) zv /= (double)(b - a);
        }
        so[i] = sv;
        zo[i] = zv;
    }
}

} // namespace

void transform_reverse(void *stream, const RvMaps &mp, int n, int m, double *xo, const double *x2, const double *d,
                       double sx, double *so, const double *s2, const double *einv, double ss, double *zo,
                       const double *z2, const double *e, double sz) {
    if (n + m == 0) return;
    k_transform_reverse<<<stream_grid(n + m), WG, 0, (hipStream_t)stream>>>(mp.mode, mp.ptr, mp.src, n, m, xo, x2, d,
                                                                             sx, so, s2, einv, ss, zo, z2, e, sz);
}

} // namespace dev
} // namespace chip
