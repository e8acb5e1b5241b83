// batch_jacobian.hip -- the device work of the batched L4 solver's BLOCKS of forward-mode derivatives (chip_bjac_*;
// DESIGN.md 4.18): the passes of batch_tangent.hip for up to BJ_MAX_DIR directions at once, and the right-hand sides
// of the unit directions a member Jacobian is made of.  Between them run chip_kkt's refined solves, one per direction
// and all enqueued before the one synchronisation of the call (batch_deriv.cpp).
//
// 256-thread workgroups, no atomics, one writer per output entry, no scratch (the accumulators of a tile of
// directions are a fully unrolled, constant-indexed array):
//   k_bj_rhs    k_bt_rhs for a block.  Rows of [x space; z space] are owned as there -- by a lane, a wavefront or the
//               workgroup by the row's entry count (BT_THREAD, BT_WAVE) -- and the owner walks its row once per
//               BJ_TILE directions: idx[t], map[t] and vec[idx[t]] are loaded once and multiply the values of every
//               direction of the tile.  Per direction the terms, their order and the reduction trees (wave_sum_all,
//               block_sum) are k_bt_rhs's, so direction t of a block is bit for bit the single pass on direction t.
//   k_bj_units  the right-hand sides of unit directions, store only: no input is read.
//   k_bj_out    k_bt_out over the directions: an entry's scalings, member and validity are loaded once.
// A member with valid[k] == 0 is selected out, never multiplied by 0.
#include <cstdint>
#include <initializer_list>

#include "dev_common.hpp"
#include "batch_jacobian.hpp"

namespace chip {
namespace dev {

namespace {

// what the kernels read of the BatchPlan
struct BjPlan {
    int n, m;
    const int *xmem, *zmem, *rtype, *xoff, *zoff;
};

// one row of [x space; z space] and its entry ranges (batch_tangent.hip: BtRow)
struct BjRow {
    int isx, j, k, v;   // j: the index in its own space; k: the member; v: valid[k]
    int b0, e0, b1, e1; // x row: [b0, e0) of Psym, [b1, e1) of Acol; z row: [b0, e0) of Arow
};
__device__ __forceinline__ BjRow bj_row(const BjPlan &p, const SpPattern &Psym, const SpPattern &Acol,
                                        const SpPattern &Arow, const BtRhs &a, int r) {
    BjRow w;
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

// the entries first, first + step, ... of [beg, end) into the NT sums: val is direction 0 of the tile, stride apart
template <int NT>
__device__ __forceinline__ void bj_seg(const SpPattern &M, const double *val, size_t stride, const double *vec, int beg,
                                       int end, int first, int step, double (&acc)[NT]) {
    for (int t = beg + first; t < end; t += step) {
        const int at = M.map[t];
        const double v = vec[M.idx[t]];
#pragma unroll
        for (int u = 0; u < NT; u++) acc[u] += val[(size_t)u * stride + at] * v;
    }
}

enum { BJ_BY_LANE = 0, BJ_BY_WAVE = 1, BJ_BY_GROUP = 2 };

// the directions t0 .. t0 + NT - 1 of one row: summed by the row's owner, written by its first thread
template <int NT, int OWNER>
__device__ __forceinline__ void bj_tile(const SpPattern &Psym, const SpPattern &Acol, const SpPattern &Arow,
                                        const BjRhs &b, const BjRow &w, int t0, double *red) {
    const BtRhs &a = b.one;
    const int first = OWNER == BJ_BY_LANE ? 0 : OWNER == BJ_BY_WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int step = OWNER == BJ_BY_LANE ? 1 : OWNER == BJ_BY_WAVE ? 64 : WG;
    double acc[NT];
#pragma unroll
    for (int u = 0; u < NT; u++) acc[u] = 0.0;
    const double *dP = a.dP ? a.dP + (size_t)t0 * b.sP : nullptr;
    const double *dA = a.dA ? a.dA + (size_t)t0 * b.sA : nullptr;
    if (w.isx) {
        bj_seg<NT>(Psym, dP, b.sP, a.x, w.b0, w.e0, first, step, acc);
        bj_seg<NT>(Acol, dA, b.sA, a.z, w.b1, w.e1, first, step, acc);
    } else {
        bj_seg<NT>(Arow, dA, b.sA, a.x, w.b0, w.e0, first, step, acc);
    }
#pragma unroll
    for (int u = 0; u < NT; u++) {
        if (OWNER == BJ_BY_WAVE) acc[u] = wave_sum_all(acc[u]);
        if (OWNER == BJ_BY_GROUP) acc[u] = block_sum(acc[u], red);
    }
    if ((OWNER == BJ_BY_WAVE && (threadIdx.x & 63) != 0) || (OWNER == BJ_BY_GROUP && threadIdx.x != 0)) return;
    const int j = w.j;
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const size_t t = (size_t)(t0 + u);
        if (w.isx)
            a.rx[t * b.srx + j] = w.v ? (a.c[w.k] * a.d[j]) * (0.0 - ((a.dq ? a.dq[t * b.sq + j] : 0.0) + acc[u])) : 0.0;
        else
            a.rz[t * b.srz + j] = w.v ? a.e[j] * ((a.db ? a.db[t * b.sb + j] : 0.0) - acc[u]) : 0.0;
    }
}

// the point the cones are scaled at, once per z row (batch_tangent.hip: bt_write)
__device__ __forceinline__ void bj_scaling_point(const int *rtype, int i, int v, const double *s_int, const double *z_int,
                                                 double *ss, double *zs) {
    const int t = rtype[i];
    const double unit = (t == ROW_NN || t == ROW_SOC_HEAD) ? 1.0 : 0.0;
    ss[i] = v ? s_int[i] : unit;
    zs[i] = v ? z_int[i] : unit;
}

// every direction of one row, a tile at a time (the branches are uniform over the launch)
template <int OWNER>
__device__ __forceinline__ void bj_row_block(const BjPlan &p, const SpPattern &Psym, const SpPattern &Acol,
                                             const SpPattern &Arow, const BjRhs &b, const BjRow &w, double *red) {
    for (int t0 = 0; t0 < b.ndir; t0 += BJ_TILE) {
        switch (b.ndir - t0) {
        case 1: bj_tile<1, OWNER>(Psym, Acol, Arow, b, w, t0, red); break;
        case 2: bj_tile<2, OWNER>(Psym, Acol, Arow, b, w, t0, red); break;
        case 3: bj_tile<3, OWNER>(Psym, Acol, Arow, b, w, t0, red); break;
        default: bj_tile<BJ_TILE, OWNER>(Psym, Acol, Arow, b, w, t0, red); break;
        }
    }
    const bool writer = OWNER == BJ_BY_LANE || (OWNER == BJ_BY_WAVE ? (threadIdx.x & 63) == 0 : threadIdx.x == 0);
    if (writer && !w.isx && b.one.ss) bj_scaling_point(p.rtype, w.j, w.v, b.one.s_int, b.one.z_int, b.one.ss, b.one.zs);
}

__global__ __launch_bounds__(WG) void k_bj_rhs(BjPlan p, SpPattern Psym, SpPattern Acol, SpPattern Arow, BjRhs b) {
    __shared__ double red[16];
    __shared__ unsigned long long heavy[WG / 64];
    const int total = p.n + p.m, base = blockIdx.x * WG;
    const int wv = threadIdx.x >> 6;
    // ---- the lane's own row: summed here when it is short (or empty, or its member invalid)
    const int r = base + threadIdx.x;
    int len = 0;
    if (r < total) {
        const BjRow w = bj_row(p, Psym, Acol, Arow, b.one, r);
        len = (w.e0 - w.b0) + (w.e1 - w.b1);
        if (len <= BT_THREAD) bj_row_block<BJ_BY_LANE>(p, Psym, Acol, Arow, b, w, red);
    }
    // ---- the wavefront's medium rows, one after the other (wave-uniform loop)
    unsigned long long mid = __ballot(len > BT_THREAD && len <= BT_WAVE);
    const unsigned long long big = __ballot(len > BT_WAVE);
    while (mid) {
        const int src = __ffsll((long long)mid) - 1;
        mid &= mid - 1;
        const BjRow w = bj_row(p, Psym, Acol, Arow, b.one, base + wv * 64 + src);
        bj_row_block<BJ_BY_WAVE>(p, Psym, Acol, Arow, b, w, red);
    }
    // ---- the workgroup's long rows (workgroup-uniform loop)
    if ((threadIdx.x & 63) == 0) heavy[wv] = big;
    __syncthreads();
    for (int g = 0; g < WG / 64; g++) {
        unsigned long long mm = heavy[g];
        while (mm) {
            const int src = __ffsll((long long)mm) - 1;
            mm &= mm - 1;
            const BjRow w = bj_row(p, Psym, Acol, Arow, b.one, base + g * 64 + src);
            bj_row_block<BJ_BY_GROUP>(p, Psym, Acol, Arow, b, w, red);
        }
    }
}

__global__ __launch_bounds__(WG) void k_bj_units(BjPlan p, BjUnits a) {
    for (int r = blockIdx.x * WG + threadIdx.x; r < p.n + p.m; r += gridDim.x * WG) {
        const int isx = r < p.n, j = isx ? r : r - p.n;
        const int k = isx ? p.xmem[j] : p.zmem[j], v = a.valid[k];
        const long long at = (long long)(j - (isx ? p.xoff[k] : p.zoff[k])) - a.first; // the direction that hits entry j
        const bool mine = v && a.piece == (isx ? 0 : 1);
        double unit = 0.0;
        if (mine) unit = isx ? 0.0 - a.c[k] * a.d[j] : a.e[j];
        double *out = isx ? a.rx : a.rz;
        const size_t stride = isx ? a.srx : a.srz;
        for (int t = 0; t < a.ndir; t++) out[(size_t)t * stride + j] = (mine && at == t) ? unit : 0.0;
        if (!isx && a.ss) bj_scaling_point(p.rtype, j, v, a.s_int, a.z_int, a.ss, a.zs);
    }
}

__device__ __forceinline__ void bj_out_x(const BjPlan &p, const BjOut &b, int j) {
    const BtOut &a = b.one;
    const int v = a.valid[p.xmem[j]];
    const double d = a.d[j];
    for (int t = 0; t < b.ndir; t++) a.dx[(size_t)t * p.n + j] = v ? d * a.vx[(size_t)t * b.svx + j] : 0.0;
}
__device__ __forceinline__ void bj_out_z(const BjPlan &p, const BjOut &b, int i) {
    const BtOut &a = b.one;
    const int k = p.zmem[i], v = a.valid[k];
    const bool nn = v && p.rtype[i] == ROW_NN;
    const double e = a.e[i], ei = a.einv[i], c = a.c[k];
    for (int t = 0; t < b.ndir; t++) {
        a.dz[(size_t)t * p.m + i] = v ? (e * a.vz[(size_t)t * b.svz + i]) / c : 0.0;
        a.ds[(size_t)t * p.m + i] = nn ? ei * a.w[(size_t)t * b.svz + i] : 0.0;
    }
}

// VEC: two entries per lane with 16-byte loads and stores (the launcher checks every operand and every direction's
// slice); the odd last entry of either space is left to one lane each
template <bool VEC> __global__ __launch_bounds__(WG) void k_bj_out(BjPlan p, BjOut b) {
    if (!VEC) {
        for (int i = blockIdx.x * WG + threadIdx.x; i < p.n + p.m; i += gridDim.x * WG) {
            if (i < p.n) bj_out_x(p, b, i);
            else bj_out_z(p, b, i - p.n);
        }
        return;
    }
    const BtOut &a = b.one;
    const int nx2 = p.n >> 1, nz2 = p.m >> 1;
    for (int q = blockIdx.x * WG + threadIdx.x; q < nx2 + nz2; q += gridDim.x * WG) {
        if (q < nx2) {
            const int2 mk = ((const int2 *)p.xmem)[q];
            const double2 d = ((const double2 *)a.d)[q];
            const int v0 = a.valid[mk.x], v1 = a.valid[mk.y];
            for (int t = 0; t < b.ndir; t++) {
                const double2 v = ((const double2 *)(a.vx + (size_t)t * b.svx))[q];
                double2 o;
                o.x = v0 ? d.x * v.x : 0.0;
                o.y = v1 ? d.y * v.y : 0.0;
                ((double2 *)(a.dx + (size_t)t * p.n))[q] = o;
            }
        } else {
            const int r = q - nx2;
            const int2 mk = ((const int2 *)p.zmem)[r], ty = ((const int2 *)p.rtype)[r];
            const double2 e = ((const double2 *)a.e)[r], ei = ((const double2 *)a.einv)[r];
            const int v0 = a.valid[mk.x], v1 = a.valid[mk.y];
            const bool n0 = v0 && ty.x == ROW_NN, n1 = v1 && ty.y == ROW_NN;
            const double c0 = a.c[mk.x], c1 = a.c[mk.y];
            for (int t = 0; t < b.ndir; t++) {
                const double2 v = ((const double2 *)(a.vz + (size_t)t * b.svz))[r];
                const double2 w = ((const double2 *)(a.w + (size_t)t * b.svz))[r];
                double2 z, s;
                z.x = v0 ? (e.x * v.x) / c0 : 0.0;
                z.y = v1 ? (e.y * v.y) / c1 : 0.0;
                s.x = n0 ? ei.x * w.x : 0.0;
                s.y = n1 ? ei.y * w.y : 0.0;
                ((double2 *)(a.dz + (size_t)t * p.m))[r] = z;
                ((double2 *)(a.ds + (size_t)t * p.m))[r] = s;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (p.n & 1)) bj_out_x(p, b, p.n - 1);
    if (blockIdx.x == 0 && threadIdx.x == 1 && (p.m & 1)) bj_out_z(p, b, p.m - 1);
}

bool bj_aligned(std::initializer_list<const void *> ptrs, uintptr_t mask) {
    uintptr_t all = 0;
    for (const void *q : ptrs) all |= (uintptr_t)q;
    return (all & mask) == 0;
}

BjPlan bj_plan(const BatchPlan &p) { return BjPlan{p.n, p.m, p.xmem, p.zmem, p.rtype, p.xoff, p.zoff}; }

} // namespace

void bj_rhs(hipStream_t st, const BatchPlan &p, const SpPattern &Psym, const SpPattern &Acol, const SpPattern &Arow,
            const BjRhs &a) {
    const int total = p.n + p.m;
    if (total && a.ndir > 0) k_bj_rhs<<<(total + WG - 1) / WG, WG, 0, st>>>(bj_plan(p), Psym, Acol, Arow, a);
}

void bj_units(hipStream_t st, const BatchPlan &p, const BjUnits &a) {
    if (p.n + p.m && a.ndir > 0) k_bj_units<<<stream_grid(p.n + p.m), WG, 0, st>>>(bj_plan(p), a);
}

void bj_out(hipStream_t st, const BatchPlan &p, const BjOut &b) {
    if (p.n + p.m == 0 || b.ndir < 1) return;
    const BtOut &a = b.one;
    // (direction t of a result starts t * n or t * m entries on: an odd length leaves every other slice at 8 bytes)
    const bool slices = b.ndir == 1 || (((p.n | p.m) & 1) == 0 && ((b.svx | b.svz) & 1) == 0);
    const bool vec = slices && bj_aligned({a.d, a.vx, a.dx, a.e, a.vz, a.einv, a.w, a.dz, a.ds}, 15) &&
                     bj_aligned({p.xmem, p.zmem, p.rtype}, 7);
    if (vec) k_bj_out<true><<<stream_grid((p.n + p.m + 1) / 2 + 1), WG, 0, st>>>(bj_plan(p), b);
    else k_bj_out<false><<<stream_grid(p.n + p.m), WG, 0, st>>>(bj_plan(p), b);
}

} // namespace dev
} // namespace chip
