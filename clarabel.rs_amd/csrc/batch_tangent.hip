// batch_tangent.hip -- the device work of the batched L4 solver's forward-mode derivatives (chip_bjvp_*): given a
// direction (dq, db, dP, dA) in every member's data, the tangents (dx, dz, ds) of every member's solution
// (DESIGN.md 4.16).
//
// The tangent of a solved member is one KKT solve at its final iterate with the matrix the adjoint solves with
// (batch_adjoint.hip); the scaling update, the refactor and the refined solve are chip_kkt's.  What is here are the
// two passes around it (256-thread workgroups, no atomics: every output entry has one writer):
//   k_bt_rhs   the right-hand side in the equilibrated space.  Its three sparse products, dP_sym x, dA' z and dA x,
//              read the direction's values IN PLACE through the `map` arrays of the L3 handle's row forms (position
//              in the caller's nzval): no mirrored copy of dP / dA is written and read back.  A workgroup owns 256
//              consecutive rows of [x space; z space].  A row's entry count L (over its operators, 0 for an invalid
//              member) picks who sums it: L <= BT_THREAD its own lane, serially; L <= BT_WAVE its wavefront, lane l
//              taking the entries l, l + 64, ... and the 64 partial sums meeting in the fixed tree of wave_sum_all;
//              longer rows the whole workgroup, thread t taking t, t + 256, ..., then block_sum.  The order of every
//              sum depends on the pattern alone, so the pass is bit-reproducible.  LDS: the 16 doubles of block_sum
//              and one ballot word per wavefront.
//   k_bt_out   the solution of the system multiplied back to the unscaled problem: entry-parallel, memory bound.
// A member with valid[k] == 0 is selected out, never multiplied by 0: a NaN in its solution or in its part of the
// direction cannot reach an output, and its part of the right-hand side is an exact 0.
#include <cstdint>
#include <initializer_list>

#include "dev_common.hpp"
#include "batch_tangent.hpp"

namespace chip {
namespace dev {

namespace {

// what the kernels read of the BatchPlan (the whole plan as a kernel argument costs scalar registers for nothing)
struct BtPlan {
    int n, m;
    const int *xmem, *zmem, *rtype;
};

// one row of [x space; z space]: x row j sums Psym's row j against x and Acol's row j against z, z row i sums Arow's
// row i against x.  An absent direction (null dP / dA) leaves its range empty.
struct BtRow {
    int isx, j, k, v;     // j: the index in its own space; k: the member; v: valid[k]
    int b0, e0, b1, e1;   // x row: [b0, e0) of Psym, [b1, e1) of Acol; z row: [b0, e0) of Arow
};
__device__ __forceinline__ BtRow bt_row(const BtPlan &p, const SpPattern &Psym, const SpPattern &Acol,
                                        const SpPattern &Arow, const BtRhs &a, int r) {
    BtRow w;
    w.isx = r < p.n;
    w.j = w.isx ? r : r - p.n;
    w.k = w.isx ? p.xmem[w.j] : p.zmem[w.j];
    w.v = a.valid[w.k];
    w.b0 = w.e0 = w.b1 = w.e1 = 0;
    if (!w.v) return w;
    if (w.isx) {
        if (a.dP) w.b0 = Psym.ptr[w.j], w.e0 = Psym.ptr[w.j + 1];
        if (a.dA) w.b1 = Acol.ptr[w.j], w.e1 = Acol.ptr[w.j + 1];
    } else if (a.dA) {
        w.b0 = Arow.ptr[w.j], w.e0 = Arow.ptr[w.j + 1];
    }
    return w;
}
__device__ __forceinline__ double bt_seg(const SpPattern &M, const double *val, const double *vec, int beg, int end,
                                         int first, int step, double acc) {
    for (int t = beg + first; t < end; t += step) acc += val[M.map[t]] * vec[M.idx[t]];
    return acc;
}
// the entries first, first + step, ... of the row's ranges
__device__ __forceinline__ double bt_sum(const SpPattern &Psym, const SpPattern &Acol, const SpPattern &Arow,
                                         const BtRhs &a, const BtRow &w, int first, int step) {
    if (!w.isx) return bt_seg(Arow, a.dA, a.x, w.b0, w.e0, first, step, 0.0);
    const double acc = bt_seg(Psym, a.dP, a.x, w.b0, w.e0, first, step, 0.0);
    return bt_seg(Acol, a.dA, a.z, w.b1, w.e1, first, step, acc);
}
__device__ __forceinline__ void bt_write(const BtPlan &p, const BtRhs &a, const BtRow &w, double sum) {
    const int j = w.j;
    if (w.isx) {
        a.rx[j] = w.v ? (a.c[w.k] * a.d[j]) * (0.0 - ((a.dq ? a.dq[j] : 0.0) + sum)) : 0.0;
        return;
    }
    a.rz[j] = w.v ? a.e[j] * ((a.db ? a.db[j] : 0.0) - sum) : 0.0;
    if (a.ss) {
        const int t = p.rtype[j];
        const double unit = (t == ROW_NN || t == ROW_SOC_HEAD) ? 1.0 : 0.0;
        a.ss[j] = w.v ? a.s_int[j] : unit;
        a.zs[j] = w.v ? a.z_int[j] : unit;
    }
}

__global__ __launch_bounds__(WG) void k_bt_rhs(BtPlan p, SpPattern Psym, SpPattern Acol, SpPattern Arow, BtRhs a) {
    __shared__ double red[16];
    __shared__ unsigned long long heavy[WG / 64];
    const int total = p.n + p.m, base = blockIdx.x * WG;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // ---- the lane's own row: summed here when it is short (or empty, or its member invalid)
    const int r = base + threadIdx.x;
    const bool live = r < total;
    int len = 0;
    if (live) {
        const BtRow w = bt_row(p, Psym, Acol, Arow, a, r);
        len = (w.e0 - w.b0) + (w.e1 - w.b1);
        if (len <= BT_THREAD) bt_write(p, a, w, bt_sum(Psym, Acol, Arow, a, w, 0, 1));
    }
    // ---- the wavefront's medium rows, one after the other (wave-uniform loop: every lane takes part in the sum)
    unsigned long long mid = __ballot(len > BT_THREAD && len <= BT_WAVE);
    const unsigned long long big = __ballot(len > BT_WAVE);
    while (mid) {
        const int src = __ffsll((long long)mid) - 1;
        mid &= mid - 1;
        const BtRow w = bt_row(p, Psym, Acol, Arow, a, base + wv * 64 + src);
        const double sum = wave_sum_all(bt_sum(Psym, Acol, Arow, a, w, lane, 64));
        if (lane == 0) bt_write(p, a, w, sum);
    }
    // ---- the workgroup's long rows (workgroup-uniform loop)
    if (lane == 0) heavy[wv] = big;
    __syncthreads();
    for (int g = 0; g < WG / 64; g++) {
        unsigned long long mm = heavy[g];
        while (mm) {
            const int src = __ffsll((long long)mm) - 1;
            mm &= mm - 1;
            const BtRow w = bt_row(p, Psym, Acol, Arow, a, base + g * 64 + src);
            const double sum = block_sum(bt_sum(Psym, Acol, Arow, a, w, threadIdx.x, WG), red);
            if (threadIdx.x == 0) bt_write(p, a, w, sum);
        }
    }
}

__device__ __forceinline__ void bt_out_x(const BtPlan &p, const BtOut &a, int j) {
    a.dx[j] = a.valid[p.xmem[j]] ? a.d[j] * a.vx[j] : 0.0;
}
__device__ __forceinline__ void bt_out_z(const BtPlan &p, const BtOut &a, int i) {
    const int k = p.zmem[i], v = a.valid[k];
    a.dz[i] = v ? (a.e[i] * a.vz[i]) / a.c[k] : 0.0;
    a.ds[i] = (v && p.rtype[i] == ROW_NN) ? a.einv[i] * a.w[i] : 0.0;
}

// VEC: two entries per lane with 16-byte loads and stores (the launcher checks every operand's alignment); the odd
// last entry of either space is left to one lane each
template <bool VEC> __global__ __launch_bounds__(WG) void k_bt_out(BtPlan p, BtOut a) {
    if (!VEC) {
        for (int i = blockIdx.x * WG + threadIdx.x; i < p.n + p.m; i += gridDim.x * WG) {
            if (i < p.n) bt_out_x(p, a, i);
            else bt_out_z(p, a, i - p.n);
        }
        return;
    }
    const int nx2 = p.n >> 1, nz2 = p.m >> 1;
    for (int t = blockIdx.x * WG + threadIdx.x; t < nx2 + nz2; t += gridDim.x * WG) {
        if (t < nx2) {
            const int2 mk = ((const int2 *)p.xmem)[t];
            const double2 d = ((const double2 *)a.d)[t], v = ((const double2 *)a.vx)[t];
            double2 o;
            o.x = a.valid[mk.x] ? d.x * v.x : 0.0;
            o.y = a.valid[mk.y] ? d.y * v.y : 0.0;
            ((double2 *)a.dx)[t] = o;
        } else {
            const int r = t - nx2;
            const int2 mk = ((const int2 *)p.zmem)[r], ty = ((const int2 *)p.rtype)[r];
            const double2 e = ((const double2 *)a.e)[r], v = ((const double2 *)a.vz)[r];
            const double2 ei = ((const double2 *)a.einv)[r], w = ((const double2 *)a.w)[r];
            const int v0 = a.valid[mk.x], v1 = a.valid[mk.y];
            double2 z, s;
            z.x = v0 ? (e.x * v.x) / a.c[mk.x] : 0.0;
            z.y = v1 ? (e.y * v.y) / a.c[mk.y] : 0.0;
            s.x = (v0 && ty.x == ROW_NN) ? ei.x * w.x : 0.0;
            s.y = (v1 && ty.y == ROW_NN) ? ei.y * w.y : 0.0;
            ((double2 *)a.dz)[r] = z;
            ((double2 *)a.ds)[r] = s;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (p.n & 1)) bt_out_x(p, a, p.n - 1);
    if (blockIdx.x == 0 && threadIdx.x == 1 && (p.m & 1)) bt_out_z(p, a, p.m - 1);
}

bool bt_aligned(std::initializer_list<const void *> ptrs, uintptr_t mask) {
    uintptr_t all = 0;
    for (const void *q : ptrs) all |= (uintptr_t)q;
    return (all & mask) == 0;
}

} // namespace

void bt_rhs(hipStream_t st, const BatchPlan &p, const SpPattern &Psym, const SpPattern &Acol, const SpPattern &Arow,
            const BtRhs &a) {
    const int total = p.n + p.m;
    const BtPlan q{p.n, p.m, p.xmem, p.zmem, p.rtype};
    if (total) k_bt_rhs<<<(total + WG - 1) / WG, WG, 0, st>>>(q, Psym, Acol, Arow, a);
}

void bt_out(hipStream_t st, const BatchPlan &p, const BtOut &a) {
    if (p.n + p.m == 0) return;
    const bool vec = bt_aligned({a.d, a.vx, a.dx, a.e, a.vz, a.einv, a.w, a.dz, a.ds}, 15) &&
                     bt_aligned({p.xmem, p.zmem, p.rtype}, 7);
    const BtPlan q{p.n, p.m, p.xmem, p.zmem, p.rtype};
    if (vec) k_bt_out<true><<<stream_grid((p.n + p.m + 1) / 2 + 1), WG, 0, st>>>(q, a);
    else k_bt_out<false><<<stream_grid(p.n + p.m), WG, 0, st>>>(q, a);
}

} // namespace dev
} // namespace chip
