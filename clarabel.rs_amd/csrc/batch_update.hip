// batch_update.hip -- the device work of the batched L4 solver's data updates (default/data_updating.rs on a stack
// of independent problems): the new values of P, A, q or b scaled with the equilibration of the setup and the cost
// scale of the member that owns the entry, and the members' norms of the unscaled q and b.
//
// Every pass is memory bound and entry-parallel (grid-stride loops, 256-thread workgroups, no LDS beyond the
// reductions).  The products follow problem_update.hip's orders; what differs is the cost scale, one c_k per member
// (DESIGN.md 4.13), looked up per entry through the member of its column:
//   full    P = (v * (d[row] * d[col])) * c[xmem[col]],  A = v * (e[row] * d[col])
//   partial P = ((d[row] * d[col]) * c[xmem[col]]) * v,  A = (e[row] * d[col]) * v
//   vectors q = (v * d[j]) * c[xmem[j]],                 b = v * e[i]          (both forms)
// The vector passes also keep the unscaled value (the per-member norms are taken from it, as create takes them from
// the user's data) and refresh -q.  A partial update lets the last occurrence of a repeated index win as
// problem_update.hip does: claim by atomicMax of the position into an int scratch, write where the position matches,
// release the touched slots.  The passes of a partial update read the word the index check raised and write nothing
// when it is set, so the host needs no synchronisation between the check and the writes.
#include "dev_common.hpp"
#include "batch_update.hpp"

namespace chip {
namespace dev {

namespace {

__device__ __forceinline__ double bu_scale_full(const BuTarget &t, int i, double v) {
    if (t.row) {
        const int col = t.col[i];
        const double w = v * (t.l[t.row[i]] * t.r[col]);
        return t.c ? w * t.c[t.xmem[col]] : w;
    }
    const double w = v * t.l[i];
    return t.c ? w * t.c[t.xmem[i]] : w;
}
__device__ __forceinline__ double bu_scale_partial(const BuTarget &t, int i, double v) {
    if (t.row) {
        const int col = t.col[i];
        const double lr = t.l[t.row[i]] * t.r[col];
        return (t.c ? lr * t.c[t.xmem[col]] : lr) * v;
    }
    const double w = v * t.l[i];
    return t.c ? w * t.c[t.xmem[i]] : w;
}

// matrices: the row / column / member gathers dominate, one entry per lane
__global__ __launch_bounds__(WG) void k_bu_full_mat(BuTarget t, const double *__restrict__ vals) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < t.len; i += gridDim.x * WG) t.dst[i] = bu_scale_full(t, i, vals[i]);
}
// vectors: two entries per lane with 16-byte loads and stores when every operand is 16-byte aligned
template <bool VEC> __global__ __launch_bounds__(WG) void k_bu_full_vec(BuTarget t, const double *__restrict__ vals) {
    if (VEC) {
        const int npair = t.len >> 1;
        const double2 *v2 = (const double2 *)vals, *l2 = (const double2 *)t.l;
        const int2 *m2 = (const int2 *)t.xmem;
        double2 *d2 = (double2 *)t.dst, *r2 = (double2 *)t.raw, *n2 = (double2 *)t.neg;
        for (int p = blockIdx.x * WG + threadIdx.x; p < npair; p += gridDim.x * WG) {
            const double2 v = v2[p], l = l2[p];
            double2 o;
            o.x = v.x * l.x;
            o.y = v.y * l.y;
            if (t.c) {
                const int2 mk = m2[p];
                o.x = o.x * t.c[mk.x];
                o.y = o.y * t.c[mk.y];
            }
            d2[p] = o;
            r2[p] = v;
            if (t.neg) {
                double2 ng;
                ng.x = -1.0 * o.x;
                ng.y = -1.0 * o.y;
                n2[p] = ng;
            }
        }
        if (!(t.len & 1) || blockIdx.x != 0 || threadIdx.x != 0) return;
    }
    const int first = VEC ? t.len - 1 : blockIdx.x * WG + threadIdx.x;
    for (int i = first; i < t.len; i += gridDim.x * WG) {
        const double v = vals[i], o = bu_scale_full(t, i, v);
        t.dst[i] = o;
        t.raw[i] = v;
        if (t.neg) t.neg[i] = -1.0 * o;
    }
}

__global__ __launch_bounds__(WG) void k_bu_claim(const int64_t *__restrict__ idx, int k, int *pos,
                                                 const int *__restrict__ flag) {
    if (*flag) return; // (uniform: a refused update touches nothing, and a bad index is never used as an address)
    for (int t = blockIdx.x * WG + threadIdx.x; t < k; t += gridDim.x * WG) atomicMax(pos + idx[t], t);
}
__global__ __launch_bounds__(WG) void k_bu_write(BuTarget tg, const int64_t *__restrict__ idx,
                                                 const double *__restrict__ vals, int k, const int *__restrict__ pos,
                                                 const int *__restrict__ flag, int64_t *__restrict__ clean) {
    const bool bad = *flag != 0;
    for (int t = blockIdx.x * WG + threadIdx.x; t < k; t += gridDim.x * WG) {
        if (bad) {
            clean[t] = 0;
            continue;
        }
        const int64_t i64 = idx[t];
        const int i = (int)i64;
        clean[t] = i64;
        if (pos[i] != t) continue;
        const double v = vals[t], o = bu_scale_partial(tg, i, v);
        tg.dst[i] = o;
        if (tg.raw) tg.raw[i] = v;
        if (tg.neg) tg.neg[i] = -1.0 * o;
    }
}
__global__ __launch_bounds__(WG) void k_bu_release(const int64_t *__restrict__ idx, int k, int *pos,
                                                   const int *__restrict__ flag) {
    if (*flag) return;
    for (int t = blockIdx.x * WG + threadIdx.x; t < k; t += gridDim.x * WG) pos[idx[t]] = -1;
}

// one workgroup per chunk of the plan (chunk0: the first chunk of the space): the maximum of the bits of |raw|
__global__ __launch_bounds__(WG) void k_bu_norm_partial(const double *__restrict__ raw, const int *__restrict__ ch_beg,
                                                        const int *__restrict__ ch_end, int chunk0,
                                                        unsigned long long *__restrict__ partials) {
    __shared__ unsigned long long red[WG];
    const int ch = chunk0 + blockIdx.x;
    unsigned long long acc = 0;
    for (int i = ch_beg[ch] + threadIdx.x, e = ch_end[ch]; i < e; i += WG) {
        const unsigned long long v = abs_bits(raw[i]);
        acc = v > acc ? v : acc;
    }
    acc = block_max_u64(acc, red);
    if (threadIdx.x == 0) partials[ch] = acc;
}
// one thread per member: the maximum over its chunks (a member without entries: 0, as create's loop gives)
__global__ __launch_bounds__(WG) void k_bu_norm_final(const int *__restrict__ cfirst, int chunk0, int nprob,
                                                      const unsigned long long *__restrict__ partials,
                                                      double *__restrict__ out) {
    for (int k = blockIdx.x * WG + threadIdx.x; k < nprob; k += gridDim.x * WG) {
        unsigned long long acc = 0;
        for (int ch = chunk0 + cfirst[k], e = chunk0 + cfirst[k + 1]; ch < e; ch++) {
            const unsigned long long v = partials[ch];
            acc = v > acc ? v : acc;
        }
        out[k] = __longlong_as_double((long long)acc);
    }
}

} // namespace

void bu_write_full(hipStream_t s, const BuTarget &t, const double *vals) {
    if (t.len <= 0) return;
    if (t.row) {
        k_bu_full_mat<<<stream_grid(t.len), WG, 0, s>>>(t, vals);
        return;
    }
    const uintptr_t all = (uintptr_t)vals | (uintptr_t)t.l | (uintptr_t)t.dst | (uintptr_t)t.raw | (uintptr_t)t.neg;
    const bool vec = (all & 15) == 0 && ((uintptr_t)t.xmem & 7) == 0;
    if (vec) k_bu_full_vec<true><<<stream_grid((t.len + 1) / 2), WG, 0, s>>>(t, vals);
    else k_bu_full_vec<false><<<stream_grid(t.len), WG, 0, s>>>(t, vals);
}

void bu_write_partial(hipStream_t s, const BuTarget &t, const int64_t *idx, const double *vals, int k, int *pos,
                      const int *flag, int64_t *clean) {
    if (k <= 0) return;
    const int g = stream_grid(k);
    k_bu_claim<<<g, WG, 0, s>>>(idx, k, pos, flag);
    k_bu_write<<<g, WG, 0, s>>>(t, idx, vals, k, pos, flag, clean);
    k_bu_release<<<g, WG, 0, s>>>(idx, k, pos, flag);
}

void bu_norms(hipStream_t s, const BatchPlan &p, int space, const double *raw, unsigned long long *partials,
              double *out) {
    const int chunk0 = space == 0 ? 0 : p.ncx, nch = space == 0 ? p.ncx : p.ncz;
    if (nch > 0) k_bu_norm_partial<<<nch, WG, 0, s>>>(raw, p.ch_beg, p.ch_end, chunk0, partials);
    k_bu_norm_final<<<stream_grid(p.nprob), WG, 0, s>>>(space == 0 ? p.cx_first : p.cz_first, chunk0, p.nprob,
                                                        partials, out);
}

} // namespace dev
} // namespace chip
