// problem_update.hip -- the device work of the L4 solver's data updates (default/data_updating.rs): the new values of
// P, A, q or b scaled with the equilibration of the setup (never re-equilibrated) and written into the solver's own
// arrays, the scatter of P's and A's values into K, and the norms / max |P_ii| that setup derived from the values.
//
// Every pass is memory bound and entry-parallel (grid-stride loops over 64-wide waves, no LDS beyond the reductions).
// Products are taken in the reference's order, which differs between the two forms of a matrix update:
//   full    (update_matrix for [T]: lrscale, then scale(c))   P = (v * (d[row] * d[col])) * c,  A = v * (e[row] * d[col])
//   partial (update_matrix for Zip)                           P = ((d[row] * d[col]) * c) * v,  A = (e[row] * d[col]) * v
//   vectors (both forms)                                      q = (v * d[i]) * c,               b = v * e[i]
// A partial update lets the last occurrence of a repeated index win (the reference's sequential loop) without sorting:
// every occurrence t raises pos[i] to t (atomicMax on an int), the occurrence that holds pos[i] writes, and the touched
// slots go back to -1, so no clear of the whole scratch is needed per update.  These are the only atomics of the unit;
// the maxima are reduced over the bit patterns of |x| in two fixed passes (a maximum is exact in any order, and the
// bits of a NaN exceed those of +inf, so a NaN propagates).
#include "dev_common.hpp"
#include "problem_update.hpp"

namespace chip {
namespace dev {

namespace {

constexpr int NORM_BLOCKS = 256; // fixed partition of the reductions

__device__ __forceinline__ double scale_full(const PuTarget &t, int i, double v) {
    if (t.row) {
        const double w = v * (t.l[t.row[i]] * t.r[t.col[i]]);
        return t.has_c ? w * t.c : w;
    }
    const double w = v * t.l[i];
    return t.has_c ? w * t.c : w;
}
__device__ __forceinline__ double scale_partial(const PuTarget &t, int i, double v) {
    if (t.row) {
        const double lr = t.l[t.row[i]] * t.r[t.col[i]];
        return (t.has_c ? lr * t.c : lr) * v;
    }
    const double w = v * t.l[i]; // value * vscale[idx] * c
    return t.has_c ? w * t.c : w;
}

__global__ __launch_bounds__(WG) void k_pu_validate(const int64_t *__restrict__ idx, int k, int64_t len, int *flag) {
    bool bad = false;
    for (int t = blockIdx.x * WG + threadIdx.x; t < k; t += gridDim.x * WG) {
        const int64_t i = idx[t];
        bad |= i < 0 || i >= len;
    }
    if (bad) *flag = 1; // (a plain store: every writer stores the same word)
}

// matrices: the row / column gathers dominate, one entry per lane
__global__ __launch_bounds__(WG) void k_pu_full_mat(PuTarget t, const double *__restrict__ vals) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < t.len; i += gridDim.x * WG) t.dst[i] = scale_full(t, i, vals[i]);
}
// vectors: two entries per lane with 16-byte loads and stores when every operand is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(WG) void k_pu_full_vec(PuTarget t, const double *__restrict__ vals) {
    if (VEC) {
        const int npair = t.len >> 1;
        const double2 *v2 = (const double2 *)vals, *l2 = (const double2 *)t.l;
        double2 *d2 = (double2 *)t.dst;
        for (int p = blockIdx.x * WG + threadIdx.x; p < npair; p += gridDim.x * WG) {
            const double2 v = v2[p], l = l2[p];
            double2 o;
            o.x = v.x * l.x;
            o.y = v.y * l.y;
            if (t.has_c) {
                o.x = o.x * t.c;
                o.y = o.y * t.c;
            }
            d2[p] = o;
        }
        if ((t.len & 1) && blockIdx.x == 0 && threadIdx.x == 0) t.dst[t.len - 1] = scale_full(t, t.len - 1, vals[t.len - 1]);
    } else {
        for (int i = blockIdx.x * WG + threadIdx.x; i < t.len; i += gridDim.x * WG) t.dst[i] = scale_full(t, i, vals[i]);
    }
}

__global__ __launch_bounds__(WG) void k_pu_claim(const int64_t *__restrict__ idx, int k, int *pos) {
    for (int t = blockIdx.x * WG + threadIdx.x; t < k; t += gridDim.x * WG) atomicMax(pos + idx[t], t);
}
__global__ __launch_bounds__(WG) void k_pu_write(PuTarget tg, const int64_t *__restrict__ idx,
                                                 const double *__restrict__ vals, int k, const int *__restrict__ pos) {
    for (int t = blockIdx.x * WG + threadIdx.x; t < k; t += gridDim.x * WG) {
        const int i = (int)idx[t];
        if (pos[i] == t) tg.dst[i] = scale_partial(tg, i, vals[t]);
    }
}
__global__ __launch_bounds__(WG) void k_pu_release(const int64_t *__restrict__ idx, int k, int *pos) {
    for (int t = blockIdx.x * WG + threadIdx.x; t < k; t += gridDim.x * WG) pos[idx[t]] = -1;
}

__global__ __launch_bounds__(WG) void k_pu_scatter(double *Kx, const int *__restrict__ map, const double *__restrict__ src,
                                                   const int64_t *__restrict__ idx, int k) {
    for (int t = blockIdx.x * WG + threadIdx.x; t < k; t += gridDim.x * WG) {
        const int i = idx ? (int)idx[t] : t;
        Kx[map[i]] = src[i];
    }
}

// blockIdx.y: 0 = |q dinv|, 1 = |b einv|, 2 = |P_ii|
__global__ __launch_bounds__(WG) void k_pu_norm_partial(int mask, const double *__restrict__ q,
                                                        const double *__restrict__ dinv, int n,
                                                        const double *__restrict__ b, const double *__restrict__ einv,
                                                        int m, const int *__restrict__ Prow, const int *__restrict__ Pcol,
                                                        const double *__restrict__ Px, int nnzP,
                                                        unsigned long long *partials) {
    __shared__ unsigned long long red[WG];
    const int which = blockIdx.y;
    if (!((mask >> which) & 1)) return; // (uniform over the workgroup)
    unsigned long long acc = 0;
    const int len = which == 0 ? n : (which == 1 ? m : nnzP);
    for (int i = blockIdx.x * WG + threadIdx.x; i < len; i += gridDim.x * WG) {
        unsigned long long v = 0;
        if (which == 0) v = abs_bits(q[i] * dinv[i]);
        else if (which == 1) v = abs_bits(b[i] * einv[i]);
        else if (Prow[i] == Pcol[i]) v = abs_bits(Px[i]);
        acc = v > acc ? v : acc;
    }
    acc = block_max_u64(acc, red);
    if (threadIdx.x == 0) partials[which * NORM_BLOCKS + blockIdx.x] = acc;
}
__global__ __launch_bounds__(WG) void k_pu_norm_final(int mask, const unsigned long long *__restrict__ partials,
                                                      double *out) {
    __shared__ unsigned long long red[WG];
    const int which = blockIdx.x;
    if (!((mask >> which) & 1)) return;
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < NORM_BLOCKS; i += WG) {
        const unsigned long long v = partials[which * NORM_BLOCKS + i];
        acc = v > acc ? v : acc;
    }
    acc = block_max_u64(acc, red);
    if (threadIdx.x == 0) out[which] = __longlong_as_double((long long)acc);
}

} // namespace

void pu_validate(hipStream_t s, const int64_t *idx, int k, int64_t len, int *flag) {
    if (k > 0) k_pu_validate<<<stream_grid(k), WG, 0, s>>>(idx, k, len, flag);
}

void pu_write_full(hipStream_t s, const PuTarget &t, const double *vals) {
    if (t.len <= 0) return;
    if (t.row) {
        k_pu_full_mat<<<stream_grid(t.len), WG, 0, s>>>(t, vals);
        return;
    }
    const bool vec = (((uintptr_t)vals | (uintptr_t)t.l | (uintptr_t)t.dst) & 15) == 0;
    if (vec) k_pu_full_vec<true><<<stream_grid((t.len + 1) / 2), WG, 0, s>>>(t, vals);
    else k_pu_full_vec<false><<<stream_grid(t.len), WG, 0, s>>>(t, vals);
}

void pu_write_partial(hipStream_t s, const PuTarget &t, const int64_t *idx, const double *vals, int k, int *pos) {
    if (k <= 0) return;
    const int g = stream_grid(k);
    k_pu_claim<<<g, WG, 0, s>>>(idx, k, pos);
    k_pu_write<<<g, WG, 0, s>>>(t, idx, vals, k, pos);
    k_pu_release<<<g, WG, 0, s>>>(idx, k, pos);
}

void pu_scatter(hipStream_t s, double *Kx, const int *map, const double *src, const int64_t *idx, int k) {
    if (k > 0) k_pu_scatter<<<stream_grid(k), WG, 0, s>>>(Kx, map, src, idx, k);
}

int pu_norm_partials() { return 3 * NORM_BLOCKS; }

void pu_norms(hipStream_t s, int mask, const double *q, const double *dinv, int n, const double *b, const double *einv,
              int m, const int *Prow, const int *Pcol, const double *Px, int nnzP, unsigned long long *partials,
              double *out) {
    if (!mask) return;
    k_pu_norm_partial<<<dim3(NORM_BLOCKS, 3), WG, 0, s>>>(mask, q, dinv, n, b, einv, m, Prow, Pcol, Px, nnzP, partials);
    k_pu_norm_final<<<3, WG, 0, s>>>(mask, partials, out);
}

} // namespace dev
} // namespace chip
