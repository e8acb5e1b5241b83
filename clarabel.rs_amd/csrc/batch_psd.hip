// batch_psd.hip -- the per-member passes of PSDTriangle cones in the batched L4 solver (batch_psd.hpp): the fold of the
// per-cone eigenvalue results into the members' slots, and the unit-vector operations on the diagonal svec entries.
// Both kernels are 256 threads with __launch_bounds__(256), no LDS, no scratch and no atomics
// (tests/test_batch_psd_host.py audits the resources).
#include "batch_psd.hpp"
#include "dev_common.hpp"

namespace chip {
namespace dev {

namespace {

// one thread per member: its cones in order, so the result is the same bits on every run
__global__ __launch_bounds__(WG) void k_bp_fold(BatchPsdPlan p, int op, const double *__restrict__ a,
                                                const double *__restrict__ b, double *out_min, double *out_sum) {
    const int k = blockIdx.x * WG + threadIdx.x;
    if (k >= p.nprob) return;
    const int c0 = p.first[k], c1 = p.first[k + 1];
    if (c0 == c1) return; // (a member without PSD cones keeps cone_minima's bits)
    double mn = out_min[k], sm = op == BP_MARGINS ? out_sum[k] : 0.0;
    for (int c = c0; c < c1; c++) {
        const int v = p.view[c];
        mn = fmin(mn, a[v]);
        if (op == BP_INTERIOR) mn = fmin(mn, b[v]);
        else if (op == BP_MARGINS) sm += b[v];
    }
    out_min[k] = mn;
    if (op == BP_MARGINS) out_sum[k] = sm;
}

// one lane per diagonal entry.  mode 0: z += alpha_k where mask allows; mode 1: sv = z = 1 where flag asks.  The
// member's mask selects whether the entry is written at all: a masked entry is never multiplied by 0
__global__ __launch_bounds__(WG) void k_bp_diag(BatchPsdPlan p, int mode, double *z, double *sv,
                                                const double *__restrict__ alpha, const int *__restrict__ mask) {
    for (int t = blockIdx.x * WG + threadIdx.x; t < p.ndiag; t += gridDim.x * WG) {
        const int r = p.diag[t], k = p.zmem[r];
        if (mask && !mask[k]) continue;
        if (mode == 0) {
            z[r] += alpha[k];
        } else {
            sv[r] = 1.0;
            z[r] = 1.0;
        }
    }
}

} // namespace

void bp_fold(hipStream_t s, const BatchPsdPlan &p, int op, const double *a, const double *b, double *out_min,
             double *out_sum) {
    if (p.ncones) k_bp_fold<<<(p.nprob + WG - 1) / WG, WG, 0, s>>>(p, op, a, b, out_min, out_sum);
}

void bp_diag_shift(hipStream_t s, const BatchPsdPlan &p, double *z, const double *alpha, const int *mask) {
    if (p.ndiag) k_bp_diag<<<stream_grid(p.ndiag), WG, 0, s>>>(p, 0, z, nullptr, alpha, mask);
}

void bp_diag_unit(hipStream_t s, const BatchPsdPlan &p, double *sv, double *z, const int *flag) {
    if (p.ndiag) k_bp_diag<<<stream_grid(p.ndiag), WG, 0, s>>>(p, 1, z, sv, nullptr, flag);
}

} // namespace dev
} // namespace chip
