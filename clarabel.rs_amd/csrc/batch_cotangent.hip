// batch_cotangent.hip -- the device work of the batched L4 solver's BLOCKS of gradients (chip_bvjp_*):
// the passes of batch_adjoint.hip for up to BC_MAX_DIR cotangents at once, and the right-hand sides of the unit
// cotangents the rows of a member Jacobian are made of.  Between them run chip_kkt's refined solves, one per cotangent
// and all enqueued before the one synchronisation of the call (batch_deriv.cpp).
//
// 256-thread workgroups, grid-stride loops, no LDS, no atomics, one writer per output entry, no scratch (the loops over
// the cotangents hold no private array at all: a cotangent's values live in scalars):
//   k_bc_rhs       k_ba_rhs for a block: an entry's member, flag, scalings and row type are loaded once
//   k_bc_units     the right-hand sides of unit cotangents, store only: no input is read
//   k_bc_grad_vec  k_ba_grad_vec over the cotangents, dq and / or db as wanted
//   k_bc_grad_mat  k_ba_grad_mat over the cotangents, dP and / or dA as wanted: the row / column / member gathers that
//                  dominate the single pass, and x[i], x[j], z[i], are paid once per stored entry; per cotangent only
//                  the gathers of the solve's result and of gs remain.  The adjoint variables of the unscaled problem
//                  (ux, uz) are formed in registers from the solve's result, by the single pass's expression
// Per cotangent the terms and their order are those of the single kernels, so given the same solve result cotangent t
// of a block is bit for bit the single pass on cotangent t.  A member with valid[k] == 0 is selected out, never
// multiplied by 0.
#include <cstdint>
#include <initializer_list>

#include "dev_common.hpp"
#include "batch_cotangent.hpp"

namespace chip {
namespace dev {

namespace {

// what the kernels read of the BatchPlan
struct BcPlan {
    int n, m;
    const int *xmem, *zmem, *rtype, *xoff, *zoff;
};

// the point the cones are scaled at, once per z row (batch_adjoint.hip: ba_rhs_row)
__device__ __forceinline__ void bc_scaling_point(const int *rtype, int i, int v, const double *s, const double *z,
                                                 double *ss, double *zs) {
    const int t = rtype[i];
    const double unit = (t == ROW_NN || t == ROW_SOC_HEAD) ? 1.0 : 0.0;
    ss[i] = v ? s[i] : unit;
    zs[i] = v ? z[i] : unit;
}

__global__ __launch_bounds__(WG) void k_bc_rhs(BcPlan p, BcRhs a) {
    for (int r = blockIdx.x * WG + threadIdx.x; r < p.n + p.m; r += gridDim.x * WG) {
        if (r < p.n) {
            const int j = r;
            const bool on = a.valid[p.xmem[j]] && a.gx;
            const double d = a.d[j];
            for (int t = 0; t < a.ndir; t++) a.rx[(size_t)t * a.srx + j] = on ? d * a.gx[(size_t)t * p.n + j] : 0.0;
        } else {
            const int i = r - p.n, k = p.zmem[i], v = a.valid[k];
            const double e = a.e[i], c = a.c[k];
            const bool ons = v && a.gs, onz = v && a.gz;
            for (int t = 0; t < a.ndir; t++) {
                const size_t at = (size_t)t * p.m + i;
                if (a.ws) a.ws[(size_t)t * a.sws + i] = ons ? a.gs[at] / e : 0.0;
                a.rz[(size_t)t * a.srz + i] = onz ? (e * a.gz[at]) / c : 0.0;
            }
            if (a.ss) bc_scaling_point(p.rtype, i, v, a.s, a.z, a.ss, a.zs);
        }
    }
}

__global__ __launch_bounds__(WG) void k_bc_units(BcPlan p, BcUnits a) {
    for (int r = blockIdx.x * WG + threadIdx.x; r < p.n + p.m; r += gridDim.x * WG) {
        if (r < p.n) {
            const int j = r, k = p.xmem[j];
            const bool mine = a.valid[k] && a.piece == 0;
            const long long at = (long long)(j - p.xoff[k]) - a.first; // the cotangent that hits entry j
            const double unit = mine ? a.d[j] * 1.0 : 0.0;
            for (int t = 0; t < a.ndir; t++) a.rx[(size_t)t * a.srx + j] = (mine && at == t) ? unit : 0.0;
        } else {
            const int i = r - p.n, k = p.zmem[i], v = a.valid[k];
            const long long at = (long long)(i - p.zoff[k]) - a.first;
            double uz = 0.0, us = 0.0;
            if (v && a.piece == 1) uz = (a.e[i] * 1.0) / a.c[k];
            if (v && a.piece == 2) us = 1.0 / a.e[i];
            for (int t = 0; t < a.ndir; t++) {
                const bool hit = v && at == t;
                if (a.ws) a.ws[(size_t)t * a.sws + i] = (hit && a.piece == 2) ? us : 0.0;
                a.rz[(size_t)t * a.srz + i] = (hit && a.piece == 1) ? uz : 0.0;
            }
            if (a.ss) bc_scaling_point(p.rtype, i, v, a.s, a.z, a.ss, a.zs);
        }
    }
}

// gs[t][i]: the given cotangent, or the unit vector of piece 2 (BcGrad)
__device__ __forceinline__ double bc_gs(const BcGrad &a, int m, int t, int i, long long at) {
    return a.gs ? a.gs[(size_t)t * m + i] : (at == t ? 1.0 : 0.0);
}

__device__ __forceinline__ void bc_vec_x(const BcPlan &p, const BcGrad &a, int j) {
    const int k = p.xmem[j], v = a.valid[k];
    const double cd = v ? a.c[k] * a.d[j] : 0.0;
    for (int t = 0; t < a.ndir; t++) {
        const double u = v ? cd * a.vx[(size_t)t * a.svx + j] : 0.0;
        a.dq[(size_t)t * p.n + j] = 0.0 - u;
    }
}
__device__ __forceinline__ void bc_vec_z(const BcPlan &p, const BcGrad &a, int i) {
    const int k = p.zmem[i], v = a.valid[k];
    const bool withgs = v && (a.gs || a.unit_s);
    const double e = a.e[i];
    const long long at = a.unit_s ? (long long)(i - p.zoff[k]) - a.first : -1;
    for (int t = 0; t < a.ndir; t++) {
        const double u = v ? e * a.vz[(size_t)t * a.svz + i] : 0.0;
        a.db[(size_t)t * p.m + i] = withgs ? u + bc_gs(a, p.m, t, i, at) : u;
    }
}

// VEC: two entries per lane with 16-byte loads and stores (the launcher checks every operand and every cotangent's
// slice); the odd last entry of either space is left to one lane each.  Only the wanted spaces are walked
template <bool VEC> __global__ __launch_bounds__(WG) void k_bc_grad_vec(BcPlan p, BcGrad a) {
    const int nx = (a.want & BC_WANT_Q) ? p.n : 0, nz = (a.want & BC_WANT_B) ? p.m : 0;
    if (!VEC) {
        for (int i = blockIdx.x * WG + threadIdx.x; i < nx + nz; i += gridDim.x * WG) {
            if (i < nx) bc_vec_x(p, a, i);
            else bc_vec_z(p, a, i - nx);
        }
        return;
    }
    const int nx2 = nx >> 1, nz2 = nz >> 1;
    for (int q = blockIdx.x * WG + threadIdx.x; q < nx2 + nz2; q += gridDim.x * WG) {
        if (q < nx2) {
            const int2 mk = ((const int2 *)p.xmem)[q];
            const double2 d = ((const double2 *)a.d)[q];
            const int v0 = a.valid[mk.x], v1 = a.valid[mk.y];
            const double cd0 = v0 ? a.c[mk.x] * d.x : 0.0, cd1 = v1 ? a.c[mk.y] * d.y : 0.0;
            for (int t = 0; t < a.ndir; t++) {
                const double2 v = ((const double2 *)(a.vx + (size_t)t * a.svx))[q];
                double2 o;
                o.x = 0.0 - (v0 ? cd0 * v.x : 0.0);
                o.y = 0.0 - (v1 ? cd1 * v.y : 0.0);
                ((double2 *)(a.dq + (size_t)t * p.n))[q] = o;
            }
        } else {
            const int r = q - nx2;
            const int2 mk = ((const int2 *)p.zmem)[r];
            const double2 e = ((const double2 *)a.e)[r];
            const int v0 = a.valid[mk.x], v1 = a.valid[mk.y];
            const bool withgs = a.gs || a.unit_s;
            const long long at0 = a.unit_s ? (long long)(2 * r - p.zoff[mk.x]) - a.first : -1;
            const long long at1 = a.unit_s ? (long long)(2 * r + 1 - p.zoff[mk.y]) - a.first : -1;
            for (int t = 0; t < a.ndir; t++) {
                const double2 v = ((const double2 *)(a.vz + (size_t)t * a.svz))[r];
                double2 b;
                b.x = v0 ? e.x * v.x : 0.0;
                b.y = v1 ? e.y * v.y : 0.0;
                if (withgs) {
                    double2 g;
                    if (a.gs) {
                        g = ((const double2 *)(a.gs + (size_t)t * p.m))[r];
                    } else {
                        g.x = at0 == t ? 1.0 : 0.0;
                        g.y = at1 == t ? 1.0 : 0.0;
                    }
                    if (v0) b.x = b.x + g.x;
                    if (v1) b.y = b.y + g.y;
                }
                ((double2 *)(a.db + (size_t)t * p.m))[r] = b;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (nx & 1)) bc_vec_x(p, a, nx - 1);
    if (blockIdx.x == 0 && threadIdx.x == 1 && (nz & 1)) bc_vec_z(p, a, nz - 1);
}

// one stored entry of P or A per lane; only the wanted matrices are walked
__global__ __launch_bounds__(WG) void k_bc_grad_mat(BcPlan p, EqMats M, BcGrad a) {
    const int nP = (a.want & BC_WANT_P) ? M.nnzP : 0, nA = (a.want & BC_WANT_A) ? M.nnzA : 0;
    for (int q = blockIdx.x * WG + threadIdx.x; q < nP + nA; q += gridDim.x * WG) {
        if (q < nP) {
            const int i = M.Prow[q], j = M.Pcol[q], k = p.xmem[j];
            if (!a.valid[k]) {
                for (int t = 0; t < a.ndir; t++) a.dP[(size_t)t * M.nnzP + q] = 0.0;
                continue;
            }
            const double c = a.c[k], cdi = c * a.d[i], xi = a.x[i];
            if (i == j) {
                for (int t = 0; t < a.ndir; t++) {
                    const double uxi = cdi * a.vx[(size_t)t * a.svx + i];
                    a.dP[(size_t)t * M.nnzP + q] = 0.0 - uxi * xi;
                }
            } else {
                const double cdj = c * a.d[j], xj = a.x[j];
                for (int t = 0; t < a.ndir; t++) {
                    const double *vx = a.vx + (size_t)t * a.svx;
                    const double uxi = cdi * vx[i], uxj = cdj * vx[j];
                    a.dP[(size_t)t * M.nnzP + q] = 0.0 - (uxi * xj + uxj * xi);
                }
            }
        } else {
            const int w = q - nP;
            const int i = M.Arow[w], j = M.Acol[w], k = p.xmem[j];
            if (!a.valid[k]) {
                for (int t = 0; t < a.ndir; t++) a.dA[(size_t)t * M.nnzA + w] = 0.0;
                continue;
            }
            const double cdj = a.c[k] * a.d[j], e = a.e[i], xj = a.x[j], zi = a.z[i];
            const bool withgs = a.gs || a.unit_s;
            const long long at = a.unit_s ? (long long)(i - p.zoff[k]) - a.first : -1;
            for (int t = 0; t < a.ndir; t++) {
                const double uxj = cdj * a.vx[(size_t)t * a.svx + j], uzi = e * a.vz[(size_t)t * a.svz + i];
                double g = 0.0 - (zi * uxj + uzi * xj);
                if (withgs) g = g - bc_gs(a, p.m, t, i, at) * xj;
                a.dA[(size_t)t * M.nnzA + w] = g;
            }
        }
    }
}

bool bc_aligned(std::initializer_list<const void *> ptrs, uintptr_t mask) {
    uintptr_t all = 0;
    for (const void *q : ptrs) all |= (uintptr_t)q;
    return (all & mask) == 0;
}

BcPlan bc_plan(const BatchPlan &p) { return BcPlan{p.n, p.m, p.xmem, p.zmem, p.rtype, p.xoff, p.zoff}; }

} // namespace

void bc_rhs(hipStream_t st, const BatchPlan &p, const BcRhs &a) {
    if (p.n + p.m && a.ndir > 0) k_bc_rhs<<<stream_grid(p.n + p.m), WG, 0, st>>>(bc_plan(p), a);
}

void bc_units(hipStream_t st, const BatchPlan &p, const BcUnits &a) {
    if (p.n + p.m && a.ndir > 0) k_bc_units<<<stream_grid(p.n + p.m), WG, 0, st>>>(bc_plan(p), a);
}

void bc_grad_vectors(hipStream_t st, const BatchPlan &p, const BcGrad &a) {
    const bool q = a.want & BC_WANT_Q, b = a.want & BC_WANT_B;
    const int nx = q ? p.n : 0, nz = b ? p.m : 0;
    if (nx + nz == 0 || a.ndir < 1) return;
    // (cotangent t of a result starts t * n or t * m entries on: an odd length leaves every other slice at 8 bytes)
    bool vec = bc_aligned({p.xmem, p.zmem}, 7);
    const bool one = a.ndir == 1;
    if (q) vec = vec && bc_aligned({a.d, a.vx, a.dq}, 15) && (one || ((p.n & 1) == 0 && (a.svx & 1) == 0));
    if (b) vec = vec && bc_aligned({a.e, a.vz, a.db, a.gs}, 15) && (one || ((p.m & 1) == 0 && (a.svz & 1) == 0));
    if (vec) k_bc_grad_vec<true><<<stream_grid((nx + nz + 1) / 2 + 1), WG, 0, st>>>(bc_plan(p), a);
    else k_bc_grad_vec<false><<<stream_grid(nx + nz), WG, 0, st>>>(bc_plan(p), a);
}

void bc_grad_matrices(hipStream_t st, const BatchPlan &p, const EqMats &M, const BcGrad &a) {
    const int nP = (a.want & BC_WANT_P) ? M.nnzP : 0, nA = (a.want & BC_WANT_A) ? M.nnzA : 0;
    if (nP + nA == 0 || a.ndir < 1) return;
    k_bc_grad_mat<<<stream_grid(nP + nA), WG, 0, st>>>(bc_plan(p), M, a);
}

} // namespace dev
} // namespace chip
