// batch_adjoint.hip -- the device work of the batched L4 solver's gradients (chip_bgrad_*): given dL/dx, dL/dz, dL/ds
// of every member's solution, dL/dq, dL/db, dL/dP, dL/dA of every member.
//
// The adjoint of a solved member is one KKT solve at its final iterate, K = [P A'; A -H] with H = diag(s/z) on the
// Nonnegative rows and 0 on the Zero rows: the scaling update, the refactor and the refined solve are chip_kkt's.
// What is here are the passes around it, all memory bound and entry-parallel (grid-stride loops, 256-thread
// workgroups, no LDS, no atomics: every output entry has one writer):
//   k_ba_rhs        the right-hand side in the equilibrated space and the point the cones are scaled at
//   k_ba_grad_vec   the adjoint variables multiplied back to the unscaled problem, dq and db
//   k_ba_grad_mat   dP and dA on the stored entries (the row / column / member gathers dominate, one entry per lane)
// The member of an entry is looked up through its column or row (xmem / zmem), as batch_update.hip does.  A member
// with valid[k] == 0 is selected out, never multiplied by 0: a NaN in its iterate or in its incoming gradient cannot
// reach an output, and its part of the right-hand side is an exact 0.
#include <cstdint>
#include <initializer_list>

#include "dev_common.hpp"
#include "batch_adjoint.hpp"

namespace chip {
namespace dev {

namespace {

__device__ __forceinline__ double ba_rx(const BaRhs &a, int v, int j) { return (v && a.gx) ? a.d[j] * a.gx[j] : 0.0; }
__device__ __forceinline__ void ba_rhs_row(const BatchPlan &p, const BaRhs &a, int i) {
    const int k = p.zmem[i], v = a.valid[k];
    const double e = a.e[i];
    a.ws[i] = (v && a.gs) ? a.gs[i] / e : 0.0;
    a.rz[i] = (v && a.gz) ? (e * a.gz[i]) / a.c[k] : 0.0;
    const int t = p.rtype[i];
    const double unit = (t == ROW_NN || t == ROW_SOC_HEAD) ? 1.0 : 0.0;
    a.ss[i] = v ? a.s[i] : unit;
    a.zs[i] = v ? a.z[i] : unit;
}

__global__ __launch_bounds__(WG) void k_ba_rhs(BatchPlan p, BaRhs a) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < p.n + p.m; i += gridDim.x * WG) {
        if (i < p.n) a.rx[i] = ba_rx(a, a.valid[p.xmem[i]], i);
        else ba_rhs_row(p, a, i - p.n);
    }
}

__device__ __forceinline__ void ba_vec_x(const BatchPlan &p, const BaGrad &a, int j) {
    const int k = p.xmem[j];
    const double u = a.valid[k] ? (a.c[k] * a.d[j]) * a.vx[j] : 0.0;
    a.ux[j] = u;
    a.dq[j] = 0.0 - u;
}
__device__ __forceinline__ void ba_vec_z(const BatchPlan &p, const BaGrad &a, int i) {
    const int v = a.valid[p.zmem[i]];
    const double u = v ? a.e[i] * a.vz[i] : 0.0;
    a.uz[i] = u;
    a.db[i] = (v && a.gs) ? u + a.gs[i] : u;
}

// VEC: two entries per lane with 16-byte loads and stores (the launcher checks every operand's alignment); the odd
// last entry of either space is left to one lane each
template <bool VEC> __global__ __launch_bounds__(WG) void k_ba_grad_vec(BatchPlan p, BaGrad a) {
    if (!VEC) {
        for (int i = blockIdx.x * WG + threadIdx.x; i < p.n + p.m; i += gridDim.x * WG) {
            if (i < p.n) ba_vec_x(p, a, i);
            else ba_vec_z(p, a, i - p.n);
        }
        return;
    }
    const int nx2 = p.n >> 1, nz2 = p.m >> 1;
    for (int t = blockIdx.x * WG + threadIdx.x; t < nx2 + nz2; t += gridDim.x * WG) {
        if (t < nx2) {
            const int2 mk = ((const int2 *)p.xmem)[t];
            const double2 d = ((const double2 *)a.d)[t], v = ((const double2 *)a.vx)[t];
            double2 u, q;
            u.x = a.valid[mk.x] ? (a.c[mk.x] * d.x) * v.x : 0.0;
            u.y = a.valid[mk.y] ? (a.c[mk.y] * d.y) * v.y : 0.0;
            q.x = 0.0 - u.x;
            q.y = 0.0 - u.y;
            ((double2 *)a.ux)[t] = u;
            ((double2 *)a.dq)[t] = q;
        } else {
            const int r = t - nx2;
            const int2 mk = ((const int2 *)p.zmem)[r];
            const double2 e = ((const double2 *)a.e)[r], v = ((const double2 *)a.vz)[r];
            const int v0 = a.valid[mk.x], v1 = a.valid[mk.y];
            double2 u, b;
            u.x = v0 ? e.x * v.x : 0.0;
            u.y = v1 ? e.y * v.y : 0.0;
            b = u;
            if (a.gs) {
                const double2 g = ((const double2 *)a.gs)[r];
                if (v0) b.x = u.x + g.x;
                if (v1) b.y = u.y + g.y;
            }
            ((double2 *)a.uz)[r] = u;
            ((double2 *)a.db)[r] = b;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (p.n & 1)) ba_vec_x(p, a, p.n - 1);
    if (blockIdx.x == 0 && threadIdx.x == 1 && (p.m & 1)) ba_vec_z(p, a, p.m - 1);
}

__global__ __launch_bounds__(WG) void k_ba_grad_mat(BatchPlan p, EqMats M, BaGrad a) {
    for (int t = blockIdx.x * WG + threadIdx.x; t < M.nnzP + M.nnzA; t += gridDim.x * WG) {
        if (t < M.nnzP) {
            const int i = M.Prow[t], j = M.Pcol[t];
            double g = 0.0;
            if (a.valid[p.xmem[j]]) {
                const double uxi = a.ux[i], xi = a.x[i];
                g = i == j ? 0.0 - uxi * xi : 0.0 - (uxi * a.x[j] + a.ux[j] * xi);
            }
            a.dP[t] = g;
        } else {
            const int q = t - M.nnzP;
            const int i = M.Arow[q], j = M.Acol[q];
            double g = 0.0;
            if (a.valid[p.xmem[j]]) {
                const double xj = a.x[j];
                g = 0.0 - (a.z[i] * a.ux[j] + a.uz[i] * xj);
                if (a.gs) g = g - a.gs[i] * xj;
            }
            a.dA[q] = g;
        }
    }
}

bool ba_aligned16(std::initializer_list<const void *> ptrs) {
    uintptr_t all = 0;
    for (const void *q : ptrs) all |= (uintptr_t)q;
    return (all & 15) == 0;
}

} // namespace

void ba_rhs(hipStream_t st, const BatchPlan &p, const BaRhs &a) {
    if (p.n + p.m) k_ba_rhs<<<stream_grid(p.n + p.m), WG, 0, st>>>(p, a);
}

void ba_grad_vectors(hipStream_t st, const BatchPlan &p, const BaGrad &a) {
    if (p.n + p.m == 0) return;
    const bool vec = ba_aligned16({a.d, a.vx, a.ux, a.dq, a.e, a.vz, a.uz, a.db, a.gs}) &&
                     (((uintptr_t)p.xmem | (uintptr_t)p.zmem) & 7) == 0;
    if (vec) k_ba_grad_vec<true><<<stream_grid((p.n + p.m + 1) / 2 + 1), WG, 0, st>>>(p, a);
    else k_ba_grad_vec<false><<<stream_grid(p.n + p.m), WG, 0, st>>>(p, a);
}

void ba_grad_matrices(hipStream_t st, const BatchPlan &p, const EqMats &M, const BaGrad &a) {
    if (M.nnzP + M.nnzA) k_ba_grad_mat<<<stream_grid(M.nnzP + M.nnzA), WG, 0, st>>>(p, M, a);
}

} // namespace dev
} // namespace chip
