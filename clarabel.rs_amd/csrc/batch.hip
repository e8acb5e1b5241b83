// batch.hip -- the per-member passes of the batched L4 solver (batch.cpp): segmented sums (the scaled norms of
// DefaultInfo::update, the dots of the residuals and of the tau direction, kktsystem.rs:170-186), the per-member step
// lengths, margins and interior checks of the Nonnegative and second-order cones, the vector updates with a scalar per
// member, and the Ruiz equilibration of the stack with one cost scaling per member (problemdata.rs:231-312).
//
// A batch is one block-diagonal stack: member k owns columns [xoff[k], xoff[k+1]) and rows [zoff[k], zoff[k+1]).
// Every pass covers all members in a fixed number of launches:
//   * sums: one workgroup per chunk of at most BATCH_CHUNK entries of one member (batch.hpp: BatchPlan), all specs of
//     the chunk's space in that workgroup; then one thread per (spec, member) adds the member's chunk partials in chunk
//     order.  The partition is fixed by the sizes alone, so the sums are deterministic whether the batch holds 1024
//     members of 6000 entries or 2 of 10^6 -- no floating-point atomics.
//   * minima: one workgroup per cone item (a slice of Nonnegative rows, or one second-order cone), then one thread per
//     member over its items.
//   * element-wise updates look the member up per entry (xmem / zmem) and read its scalar from a small device array.
// Every kernel is 256 threads (4 wave64s) with __launch_bounds__(256) and no LDS beyond the 16-slot reduction array:
// eight waves per SIMD, no scratch (tests/test_batch_host.py audits both).
#include <cfloat>

#include "batch.hpp"
#include "dev_common.hpp"

namespace chip {
namespace dev {

namespace {

__device__ __forceinline__ bool nonfinite(double v) { return !(fabs(v) <= DBL_MAX); }

__global__ __launch_bounds__(WG) void k_seg_partial(BatchPlan p, SegBatch bt, double *partial) {
    __shared__ double red[16];
    const int c = blockIdx.x, nch = p.ncx + p.ncz;
    const int space = c < p.ncx ? 0 : 1;
    const int beg = p.ch_beg[c], end = p.ch_end[c];
    for (int j = 0; j < bt.count; j++) {
        const SegSpec sp = bt.s[j];
        if (sp.space != space) continue; // uniform over the workgroup
        double acc = 0.0;
        for (int i = beg + threadIdx.x; i < end; i += WG) {
            if (sp.kind == SEG_DOT) {
                acc += sp.a[i] * sp.b[i];
            } else if (sp.kind == SEG_WSQ) {
                const double t = sp.a[i] * sp.b[i];
                acc += t * t;
            } else if (sp.kind == SEG_SUM) {
                acc += sp.a[i];
            } else {
                acc += (nonfinite(sp.a[i]) ? 1.0 : 0.0) + ((sp.b && nonfinite(sp.b[i])) ? 1.0 : 0.0);
            }
        }
        acc = block_sum(acc, red);
        if (threadIdx.x == 0) partial[(size_t)j * nch + c] = acc;
    }
}
__global__ __launch_bounds__(WG) void k_seg_final(BatchPlan p, SegBatch bt, const double *__restrict__ partial,
                                                  double *out) {
    const int t = blockIdx.x * WG + threadIdx.x;
    if (t >= bt.count * p.nprob) return;
    const int j = t / p.nprob, k = t - j * p.nprob;
    const SegSpec sp = bt.s[j];
    const int nch = p.ncx + p.ncz;
    const int c0 = sp.space == 0 ? p.cx_first[k] : p.ncx + p.cz_first[k];
    const int c1 = sp.space == 0 ? p.cx_first[k + 1] : p.ncx + p.cz_first[k + 1];
    double acc = 0.0;
    for (int c = c0; c < c1; c++) acc += partial[(size_t)j * nch + c];
    out[(size_t)sp.slot * p.nprob + k] = acc;
}

// overflow-safe 2-norm of x[1..n) over a workgroup (the scaled form of socone.rs's norms, as cones.hip)
__device__ __forceinline__ double block_norm_tail(const double *x, int n, double *red) {
    double amax = 0.0;
    for (int i = 1 + threadIdx.x; i < n; i += WG) amax = fmax(amax, fabs(x[i]));
    amax = block_max(amax, red);
    if (amax == 0.0) return 0.0;
    double ss = 0.0;
    for (int i = 1 + threadIdx.x; i < n; i += WG) {
        const double r = fabs(x[i]) / amax;
        ss += r * r;
    }
    ss = block_sum(ss, red);
    return amax * sqrt(ss);
}
__device__ __forceinline__ double block_dot_tail(const double *a, const double *b, int n, double *red) {
    double s = 0.0;
    for (int i = 1 + threadIdx.x; i < n; i += WG) s += a[i] * b[i];
    return block_sum(s, red);
}
// socone.rs:421-495 on quantities already reduced by the workgroup (the closed form of cones.hip)
__device__ __forceinline__ double soc_step_roots(double x0, double y0, double x1n, double y1n, double x1y1,
                                                 double amax) {
    if (x0 >= 0.0 && y0 < 0.0) amax = fmin(amax, -x0 / y0);
    const double a = (y0 - y1n) * (y0 + y1n);
    const double b = 2.0 * (x0 * y0 - x1y1);
    const double cres = (x0 - x1n) * (x0 + x1n);
    const double c = cres > 0.0 ? cres : 0.0;
    const double d = b * b - 4.0 * a * c;
    if ((a > 0.0 && b > 0.0) || d < 0.0) return amax;
    if (a == 0.0) return amax;
    if (c == 0.0) return a >= 0.0 ? amax : 0.0;
    const double t = (b >= 0.0) ? (-b - sqrt(d)) : (-b + sqrt(d));
    double r1 = (2.0 * c) / t, r2 = t / (2.0 * a);
    if (r1 < 0.0) r1 = INFINITY;
    if (r2 < 0.0) r2 = INFINITY;
    return fmin(amax, fmin(r1, r2));
}

// one workgroup per cone item -> (pmin, psum) of the item
__global__ __launch_bounds__(WG) void k_cone_items(BatchPlan p, int op, const double *__restrict__ dz,
                                                   const double *__restrict__ ds, const double *__restrict__ z,
                                                   const double *__restrict__ sv, const double *__restrict__ amax,
                                                   double *pmin, double *psum) {
    __shared__ double red[16];
    const int it = blockIdx.x;
    const int beg = p.it_beg[it], end = p.it_end[it];
    const int k = p.zmem[beg];
    double mn, sm = 0.0;
    if (p.it_type[it] == ITEM_NN) {
        double a = op == CONE_STEP ? amax[k] : DBL_MAX, b = 0.0;
        for (int i = beg + threadIdx.x; i < end; i += WG) {
            if (op == CONE_STEP) { // nonnegativecone.rs:128-153
                if (dz[i] < 0.0) a = fmin(a, -z[i] / dz[i]);
                if (ds[i] < 0.0) a = fmin(a, -sv[i] / ds[i]);
            } else if (op == CONE_MARGINS) { // nonnegativecone.rs:58-62
                a = fmin(a, z[i]);
                b += fmax(z[i], 0.0);
            } else {
                a = fmin(a, fmin(sv[i], z[i]));
            }
        }
        mn = -block_max(-a, red);
        sm = block_sum(b, red);
    } else {
        const int n = end - beg;
        if (op == CONE_STEP) { // socone.rs:289-302
            const double *zz = z + beg, *dd = dz + beg, *ss = sv + beg, *de = ds + beg;
            const double z1n = block_norm_tail(zz, n, red), dz1n = block_norm_tail(dd, n, red);
            const double zdz = block_dot_tail(zz, dd, n, red);
            const double s1n = block_norm_tail(ss, n, red), ds1n = block_norm_tail(de, n, red);
            const double sds = block_dot_tail(ss, de, n, red);
            const double am = amax[k];
            mn = fmin(soc_step_roots(zz[0], dd[0], z1n, dz1n, zdz, am), soc_step_roots(ss[0], de[0], s1n, ds1n, sds, am));
        } else if (op == CONE_MARGINS) { // socone.rs:104-108
            const double a = z[beg] - block_norm_tail(z + beg, n, red);
            mn = a;
            sm = fmax(0.0, a);
        } else {
            const double az = z[beg] - block_norm_tail(z + beg, n, red);
            const double as = sv[beg] - block_norm_tail(sv + beg, n, red);
            mn = fmin(az, as);
        }
    }
    if (threadIdx.x == 0) {
        pmin[it] = mn;
        psum[it] = sm;
    }
}
__global__ __launch_bounds__(WG) void k_cone_final(BatchPlan p, int op, const double *__restrict__ amax,
                                                   const double *__restrict__ pmin, const double *__restrict__ psum,
                                                   double *out_min, double *out_sum) {
    const int k = blockIdx.x * WG + threadIdx.x;
    if (k >= p.nprob) return;
    double mn = op == CONE_STEP ? amax[k] : DBL_MAX, sm = 0.0;
    for (int it = p.it_first[k]; it < p.it_first[k + 1]; it++) {
        mn = fmin(mn, pmin[it]);
        sm += psum[it];
    }
    out_min[k] = mn;
    if (out_sum) out_sum[k] = sm;
}

__global__ __launch_bounds__(WG) void k_blin(BatchPlan p, BLin a) {
    const int len = a.space ? p.m : p.n;
    const int *mem = a.space ? p.zmem : p.xmem;
    for (int i = blockIdx.x * WG + threadIdx.x; i < len; i += gridDim.x * WG) {
        const int k = mem[i];
        if (a.mask && !a.mask[k]) {
            if (a.mask_mode == MASK_ZERO) a.w[i] = 0.0;
            else if (a.mask_mode == MASK_Y) a.w[i] = a.y[i];
            continue;
        }
        const double ak = a.sa ? a.sa[k] : a.ca;
        if (a.y) {
            const double bk = a.sb ? a.sb[k] : a.cb;
            a.w[i] = ak * a.x[i] + bk * a.y[i];
        } else {
            a.w[i] = ak * a.x[i];
        }
    }
}

__global__ __launch_bounds__(WG) void k_bresid(BatchPlan p, double *rx, const double *__restrict__ rx_inf,
                                               const double *__restrict__ Px, const double *__restrict__ q, double *rz,
                                               const double *__restrict__ rz_inf, const double *__restrict__ b,
                                               const double *__restrict__ tau) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < p.n + p.m; i += gridDim.x * WG) {
        if (i < p.n) {
            rx[i] = 1.0 * rx_inf[i] + -1.0 * Px[i] + (-tau[p.xmem[i]]) * q[i]; // lin3's order (algebra.hip)
        } else {
            const int j = i - p.n;
            rz[j] = 1.0 * rz_inf[j] + (-tau[p.zmem[j]]) * b[j];
        }
    }
}

__global__ __launch_bounds__(WG) void k_bunit_shift(BatchPlan p, double *z, const double *__restrict__ alpha,
                                                    int primal, const int *__restrict__ mask) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < p.m; i += gridDim.x * WG) {
        const int k = p.zmem[i];
        if (mask && !mask[k]) continue;
        const int t = p.rtype[i];
        if (t == ROW_NN || t == ROW_SOC_HEAD) z[i] += alpha[k];
        else if (t == ROW_ZERO && primal) z[i] = 0.0;
    }
}

__global__ __launch_bounds__(WG) void k_bunit_reset(BatchPlan p, double *x, double *sv, double *z,
                                                    const int *__restrict__ flag) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < p.n + p.m; i += gridDim.x * WG) {
        if (i < p.n) {
            if (flag[p.xmem[i]]) x[i] = 0.0;
        } else {
            const int j = i - p.n;
            if (!flag[p.zmem[j]]) continue;
            const int t = p.rtype[j];
            const double e = (t == ROW_NN || t == ROW_SOC_HEAD) ? 1.0 : 0.0;
            sv[j] = e;
            z[j] = e;
        }
    }
}

__global__ __launch_bounds__(WG) void k_bunscale(BatchPlan p, double *xo, const double *__restrict__ x,
                                                 const double *__restrict__ d, double *zo, const double *__restrict__ z,
                                                 const double *__restrict__ e, double *so, const double *__restrict__ sv,
                                                 const double *__restrict__ einv, const double *__restrict__ sx,
                                                 const double *__restrict__ sz) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < p.n + 2 * p.m; i += gridDim.x * WG) {
        if (i < p.n) {
            xo[i] = (x[i] * d[i]) * sx[p.xmem[i]];
        } else if (i < p.n + p.m) {
            const int j = i - p.n;
            zo[j] = (z[j] * e[j]) * sz[p.zmem[j]];
        } else {
            const int j = i - p.n - p.m;
            so[j] = (sv[j] * einv[j]) * sx[p.zmem[j]];
        }
    }
}

// ---- Ruiz equilibration of the stack (equilibrate.hip's passes; the cost scaling per member) ----------------------
__device__ __forceinline__ void amax_bits(unsigned long long *p, double a) {
    if (!(a == a)) return; // f64::max ignores NaN
    const unsigned long long v = (unsigned long long)__double_as_longlong(a);
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}
__device__ __forceinline__ double bits_val(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ double clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// kkt_col_norms (problemdata.rs:316-325): the norms of a block-diagonal stack are already per member
__global__ __launch_bounds__(WG) void k_beq_norms(EqMats M, unsigned long long *dbits, unsigned long long *ebits) {
    const int total = M.nnzP + M.nnzA;
    for (int k = blockIdx.x * WG + threadIdx.x; k < total; k += gridDim.x * WG) {
        if (k < M.nnzP) {
            const double a = fabs(M.Px[k]);
            amax_bits(dbits + M.Pcol[k], a);
            amax_bits(dbits + M.Prow[k], a);
        } else {
            const int t = k - M.nnzP;
            const double a = fabs(M.Ax[t]);
            amax_bits(dbits + M.Acol[t], a);
            amax_bits(ebits + M.Arow[t], a);
        }
    }
}
// problemdata.rs:252-272 per element (k_eq_factors), ||q||inf of the scaled q per member into qinf[member]
__global__ __launch_bounds__(WG) void k_beq_factors(BatchPlan p, unsigned long long *dbits, unsigned long long *ebits,
                                                    double *q, double *b, double *d, double *e, double smin,
                                                    double smax, unsigned long long *qinf) {
    const int n = p.n, m = p.m;
    for (int i = blockIdx.x * WG + threadIdx.x; i < n + m; i += gridDim.x * WG) {
        const bool col = i < n;
        const int j = col ? i : i - n;
        unsigned long long *slot = col ? dbits + j : ebits + j;
        double *cum = col ? d + j : e + j;
        double x = bits_val(*slot);
        if (x == 0.0) x = 1.0;
        double w = 1.0 / sqrt(x);
        const double cj = *cum;
        w = clip(w, smin / cj, smax / cj);
        *(double *)slot = w;
        if (col) {
            const double qj = q[j] * w;
            q[j] = qj;
            const double aq = fabs(qj);
            if (aq > 0.0) amax_bits(qinf + p.xmem[j], aq);
        } else {
            b[j] = b[j] * w;
        }
        *cum = cj * w;
    }
}
// scale_data (problemdata.rs:330-349) and P.col_norms of the scaled P -> pcol (k_eq_scale)
__global__ __launch_bounds__(WG) void k_beq_scale(EqMats M, const double *__restrict__ dw, const double *__restrict__ ew,
                                                  unsigned long long *pcol) {
    const int total = M.nnzP + M.nnzA;
    for (int k = blockIdx.x * WG + threadIdx.x; k < total; k += gridDim.x * WG) {
        if (k < M.nnzP) {
            const int c = M.Pcol[k];
            const double v = M.Px[k] * (dw[M.Prow[k]] * dw[c]);
            M.Px[k] = v;
            amax_bits(pcol + c, fabs(v));
        } else {
            const int t = k - M.nnzP;
            M.Ax[t] = M.Ax[t] * (ew[M.Arow[t]] * dw[M.Acol[t]]);
        }
    }
}
// problemdata.rs:283-296 per member: the mean of its column norms, its ||q||inf, the decision and its c
__global__ __launch_bounds__(WG) void k_beq_cost_final(BatchPlan p, const double *__restrict__ colsum,
                                                       const unsigned long long *__restrict__ qinf, double *cstate,
                                                       double smin, double smax) {
    const int k = blockIdx.x * WG + threadIdx.x;
    if (k >= p.nprob) return;
    const int nk = p.xoff[k + 1] - p.xoff[k];
    const double mean = nk ? colsum[k] / (double)nk : 0.0;
    const double qn = bits_val(qinf[k]);
    double ctmp = 1.0;
    if (mean != 0.0 && qn != 0.0) {
        const double c = cstate[k];
        ctmp = clip(1.0 / fmax(qn, mean), smin / c, smax / c);
        cstate[k] = c * ctmp;
    }
    cstate[p.nprob + k] = ctmp;
}
// P.scale(ctmp_k), q.scale(ctmp_k) with the factor of the entry's member
__global__ __launch_bounds__(WG) void k_beq_cost_apply(BatchPlan p, double *Px, const int *__restrict__ Pcol, int nnzP,
                                                       double *q, const double *__restrict__ cstate) {
    const double *fac = cstate + p.nprob;
    for (int k = blockIdx.x * WG + threadIdx.x; k < nnzP + p.n; k += gridDim.x * WG) {
        if (k < nnzP) {
            const double c = fac[p.xmem[Pcol[k]]];
            if (c != 1.0) Px[k] = Px[k] * c;
        } else {
            const int j = k - nnzP;
            const double c = fac[p.xmem[j]];
            if (c != 1.0) q[j] = q[j] * c;
        }
    }
}

inline int per_member_grid(int count) { return (count + WG - 1) / WG; }

} // namespace

size_t seg_scratch_doubles(const BatchPlan &p) { return (size_t)SEG_MAX * (size_t)(p.ncx + p.ncz); }

void seg_reduce(hipStream_t s, const BatchPlan &p, const SegBatch &bt, double *out, double *scratch) {
    if (bt.count <= 0 || p.nprob <= 0) return;
    if (p.ncx + p.ncz) k_seg_partial<<<p.ncx + p.ncz, WG, 0, s>>>(p, bt, scratch);
    k_seg_final<<<per_member_grid(bt.count * p.nprob), WG, 0, s>>>(p, bt, scratch, out);
}

size_t cone_scratch_doubles(const BatchPlan &p) { return 2 * (size_t)std::max(p.nitems, 1); }

void cone_minima(hipStream_t s, const BatchPlan &p, int op, const double *dz, const double *ds, const double *z,
                 const double *sv, const double *amax, double *out_min, double *out_sum, double *scratch) {
    if (p.nprob <= 0) return;
    double *pmin = scratch, *psum = scratch + std::max(p.nitems, 1);
    if (p.nitems) k_cone_items<<<p.nitems, WG, 0, s>>>(p, op, dz, ds, z, sv, amax, pmin, psum);
    k_cone_final<<<per_member_grid(p.nprob), WG, 0, s>>>(p, op, amax, pmin, psum, out_min, out_sum);
}

void blin(hipStream_t s, const BatchPlan &p, const BLin &a) {
    const int len = a.space ? p.m : p.n;
    if (len) k_blin<<<stream_grid(len), WG, 0, s>>>(p, a);
}

void bresid(hipStream_t s, const BatchPlan &p, double *rx, const double *rx_inf, const double *Px, const double *q,
            double *rz, const double *rz_inf, const double *b, const double *tau) {
    if (p.n + p.m) k_bresid<<<stream_grid(p.n + p.m), WG, 0, s>>>(p, rx, rx_inf, Px, q, rz, rz_inf, b, tau);
}

void bunit_shift(hipStream_t s, const BatchPlan &p, double *z, const double *alpha, int primal, const int *mask) {
    if (p.m) k_bunit_shift<<<stream_grid(p.m), WG, 0, s>>>(p, z, alpha, primal, mask);
}

void bunit_reset(hipStream_t s, const BatchPlan &p, double *x, double *sv, double *z, const int *flag) {
    if (p.n + p.m) k_bunit_reset<<<stream_grid(p.n + p.m), WG, 0, s>>>(p, x, sv, z, flag);
}

void bunscale(hipStream_t s, const BatchPlan &p, double *xo, const double *x, const double *d, double *zo,
              const double *z, const double *e, double *so, const double *sv, const double *einv, const double *sx,
              const double *sz) {
    if (p.n + 2 * p.m) k_bunscale<<<stream_grid(p.n + 2 * p.m), WG, 0, s>>>(p, xo, x, d, zo, z, e, so, sv, einv, sx, sz);
}

size_t batch_eq_bits_words(int n, int m, int nprob) { return (size_t)2 * n + m + (size_t)nprob; }

void batch_eq_ruiz_step(hipStream_t s, const BatchPlan &p, const EqMats &M, double *q, double *b, double *d, double *e,
                        unsigned long long *bits, double *seg_scratch, double *colsum, double *cstate, double smin,
                        double smax) {
    const int n = p.n, m = p.m;
    unsigned long long *dbits = bits, *ebits = bits + n, *pcol = bits + n + m, *qinf = bits + 2 * (size_t)n + m;
    const int nnz = M.nnzP + M.nnzA;
    if (nnz) k_beq_norms<<<stream_grid(nnz), WG, 0, s>>>(M, dbits, ebits);
    if (n + m) k_beq_factors<<<stream_grid(n + m), WG, 0, s>>>(p, dbits, ebits, q, b, d, e, smin, smax, qinf);
    if (nnz) k_beq_scale<<<stream_grid(nnz), WG, 0, s>>>(M, (const double *)dbits, (const double *)ebits, pcol);
    SegBatch bt{};
    bt.s[0] = SegSpec{(const double *)pcol, nullptr, SEG_SUM, 0, 0}; // the column norms are non-negative doubles
    bt.count = 1;
    seg_reduce(s, p, bt, colsum, seg_scratch);
    k_beq_cost_final<<<per_member_grid(p.nprob), WG, 0, s>>>(p, colsum, qinf, cstate, smin, smax);
    if (M.nnzP + n) k_beq_cost_apply<<<stream_grid(M.nnzP + n), WG, 0, s>>>(p, M.Px, M.Pcol, M.nnzP, q, cstate);
}

} // namespace dev
} // namespace chip
