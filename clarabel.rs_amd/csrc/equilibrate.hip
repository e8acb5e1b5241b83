// equilibrate.hip -- the data-parallel work of the L4 solver (solver.cpp): Ruiz equilibration of (P, q, A, b)
// (default/problemdata.rs:231-312), the rectification of the cones that take a scalar scaling (compositecone.rs:183-195),
// the scaled norms of DefaultInfo::update (default/info.rs:142-165) and the unscaling of the solution
// (default/variables.rs:262-285).
//
// Every pass is memory bound.  The inf-norms are maxima over rows and columns of sparse matrices, computed entry-parallel
// with a 64-bit atomicMax on the bit pattern of |a| (finite non-negative doubles order like their bits, and a maximum is
// exact in any order); a lane first reads the slot and skips the atomic when it cannot raise it, so a dense row (the
// 10^6-entry budget row) costs a few atomics, not one per entry.  These are integer atomics: -munsafe-fp-atomics does
// not touch them.  The scaling factors use 1.0 / sqrt(x), the correctly rounded form of vecmath.rs:57-59, never the
// approximate hardware rsq, and every product is taken in the reference's order (CscMatrix::lrscale multiplies l[row] *
// r[col] first), so that with no cost scaling and no rectification d and e match a sequential restatement bit for bit.
#include "dev_common.hpp"
#include "equilibrate.hpp"

namespace chip {
namespace dev {

namespace {

constexpr int COST_BLOCKS = 256; // fixed partition of the mean of P's column norms (deterministic)
constexpr int WNORM_BLOCKS = 256;

__device__ __forceinline__ void amax_bits(unsigned long long *p, double a) {
    if (!(a == a)) return; // f64::max ignores NaN
    const unsigned long long v = (unsigned long long)__double_as_longlong(a);
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}
__device__ __forceinline__ double bits_val(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ double clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// kkt_col_norms (problemdata.rs:316-325): P.col_norms_sym -> dwork (each triu entry counts for its column and its row),
// A.col_norms_no_reset -> dwork, A.row_norms -> ework
__global__ __launch_bounds__(WG) void k_eq_norms(EqMats M, unsigned long long *dbits, unsigned long long *ebits) {
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

// problemdata.rs:252-272 per element: zero norm -> 1, 1/sqrt, clip against the cumulative scaling; then q <- D q,
// b <- E b (scale_data) and d <- d dwork, e <- e ework.  The factors overwrite the norm bits in place.  ||q||inf of the
// scaled q is reduced into *qinf (one atomic per workgroup).
__global__ __launch_bounds__(WG) void k_eq_factors(unsigned long long *dbits, unsigned long long *ebits, double *q,
                                                   double *b, double *d, double *e, int n, int m, double smin,
                                                   double smax, unsigned long long *qinf) {
    __shared__ double red[16];
    double qm = 0.0;
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
            qm = fmax(qm, fabs(qj));
        } else {
            b[j] = b[j] * w;
        }
        *cum = cj * w;
    }
    qm = block_max(qm, red);
    if (threadIdx.x == 0 && qm > 0.0) amax_bits(qinf, qm);
}

// scale_data (problemdata.rs:330-349): P <- D P D, A <- E A D as lrscale does it (val *= l[row] * r[col]); and
// P.col_norms of the scaled (triu) P -> pcol for the cost scaling (:278-281)
__global__ __launch_bounds__(WG) void k_eq_scale(EqMats M, const double *__restrict__ dw, const double *__restrict__ ew,
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

__global__ __launch_bounds__(WG) void k_eq_cost_partial(const unsigned long long *__restrict__ pcol, int n,
                                                        double *partials) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) acc += bits_val(pcol[i]);
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}
// the device-side tail of the cost scaling (problemdata.rs:283-296): mean of the column norms, ||q||inf, the decision
// and the update of c.  cstate[1] = this step's factor (1 = skipped)
__global__ __launch_bounds__(WG) void k_eq_cost_final(const double *__restrict__ partials, int n,
                                                      const unsigned long long *qinf, double *cstate, double smin,
                                                      double smax) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int i = threadIdx.x; i < COST_BLOCKS; i += WG) acc += partials[i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const double mean = n ? acc / (double)n : 0.0;
        const double qn = bits_val(*qinf);
        double ctmp = 1.0;
        if (mean != 0.0 && qn != 0.0) {
            const double c = cstate[0];
            ctmp = clip(1.0 / fmax(qn, mean), smin / c, smax / c);
            cstate[0] = c * ctmp;
        }
        cstate[1] = ctmp;
    }
}
// P.scale(ctmp), q.scale(ctmp)
__global__ __launch_bounds__(WG) void k_eq_cost_apply(double *Px, int nnzP, double *q, int n, const double *cstate) {
    const double c = cstate[1];
    if (c == 1.0) return;
    for (int k = blockIdx.x * WG + threadIdx.x; k < nnzP + n; k += gridDim.x * WG) {
        if (k < nnzP) Px[k] = Px[k] * c;
        else q[k - nnzP] = q[k - nnzP] * c;
    }
}

__global__ __launch_bounds__(WG) void k_eq_fill_one(double *w, int m) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < m; i += gridDim.x * WG) w[i] = 1.0;
}
// one workgroup per rectified cone: delta = recip(e) * mean(e) (socone.rs:97-101 and its siblings)
__global__ __launch_bounds__(WG) void k_eq_rect_seg(const int *__restrict__ beg, const int *__restrict__ end,
                                                    const double *__restrict__ e, double *delta) {
    __shared__ double red[16];
    const int b0 = beg[blockIdx.x], b1 = end[blockIdx.x];
    double acc = 0.0;
    for (int i = b0 + threadIdx.x; i < b1; i += WG) acc += e[i];
    acc = block_sum(acc, red);
    const double mean = acc / (double)(b1 - b0);
    for (int i = b0 + threadIdx.x; i < b1; i += WG) delta[i] = (1.0 / e[i]) * mean;
}
// A.lscale(delta), b <- b delta, e <- e delta (problemdata.rs:305-309)
__global__ __launch_bounds__(WG) void k_eq_rect_apply(EqMats M, double *b, double *e, int m,
                                                      const double *__restrict__ delta) {
    for (int k = blockIdx.x * WG + threadIdx.x; k < M.nnzA + m; k += gridDim.x * WG) {
        if (k < M.nnzA) {
            M.Ax[k] = M.Ax[k] * delta[M.Arow[k]];
        } else {
            const int i = k - M.nnzA;
            b[i] = b[i] * delta[i];
            e[i] = e[i] * delta[i];
        }
    }
}

__global__ __launch_bounds__(WG) void k_eq_invert(const double *__restrict__ d, double *dinv, int n,
                                                  const double *__restrict__ e, double *einv, int m) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < n + m; i += gridDim.x * WG) {
        if (i < n) dinv[i] = 1.0 / d[i];
        else einv[i - n] = 1.0 / e[i - n];
    }
}

__global__ __launch_bounds__(WG) void k_wnorm_partial(WNormBatch bt, double *partials) {
    __shared__ double red[16];
    const WNormSpec sp = bt.s[blockIdx.y];
    double acc = 0.0;
    for (int i = blockIdx.x * WG + threadIdx.x; i < sp.n; i += gridDim.x * WG) {
        const double t = sp.v[i] * sp.w[i];
        acc += t * t;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.y * WNORM_BLOCKS + blockIdx.x] = acc;
}
__global__ __launch_bounds__(WG) void k_wnorm_final(WNormBatch bt, const double *__restrict__ partials, double *out) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int i = threadIdx.x; i < WNORM_BLOCKS; i += WG) acc += partials[blockIdx.x * WNORM_BLOCKS + i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) out[bt.s[blockIdx.x].slot] = acc;
}

__global__ __launch_bounds__(WG) void k_unscale(double *xo, const double *__restrict__ x, const double *__restrict__ d,
                                                double sx, int n, double *zo, const double *__restrict__ z,
                                                const double *__restrict__ e, double sz, double *so,
                                                const double *__restrict__ sv, const double *__restrict__ einv,
                                                double ss, int m) {
    for (int i = blockIdx.x * WG + threadIdx.x; i < n + 2 * m; i += gridDim.x * WG) {
        if (i < n) {
            xo[i] = (x[i] * d[i]) * sx;
        } else if (i < n + m) {
            const int j = i - n;
            zo[j] = (z[j] * e[j]) * sz;
        } else {
            const int j = i - n - m;
            so[j] = (sv[j] * einv[j]) * ss;
        }
    }
}

} // namespace

size_t eq_bits_words(int n, int m) { return (size_t)2 * n + m + 1; }
int eq_cost_partials() { return COST_BLOCKS; }

void eq_ruiz_step(hipStream_t s, const EqMats &M, double *q, double *b, double *d, double *e, int n, int m,
                  unsigned long long *bits, double *partials, double *cstate, double smin, double smax) {
    unsigned long long *dbits = bits, *ebits = bits + n, *pcol = bits + n + m, *qinf = bits + 2 * (size_t)n + m;
    const int nnz = M.nnzP + M.nnzA;
    if (nnz) k_eq_norms<<<stream_grid(nnz), WG, 0, s>>>(M, dbits, ebits);
    if (n + m) k_eq_factors<<<stream_grid(n + m), WG, 0, s>>>(dbits, ebits, q, b, d, e, n, m, smin, smax, qinf);
    if (nnz) k_eq_scale<<<stream_grid(nnz), WG, 0, s>>>(M, (const double *)dbits, (const double *)ebits, pcol);
    k_eq_cost_partial<<<COST_BLOCKS, WG, 0, s>>>(pcol, n, partials);
    k_eq_cost_final<<<1, WG, 0, s>>>(partials, n, qinf, cstate, smin, smax);
    if (M.nnzP + n) k_eq_cost_apply<<<stream_grid(M.nnzP + n), WG, 0, s>>>(M.Px, M.nnzP, q, n, cstate);
}

void eq_rectify(hipStream_t s, const EqMats &M, double *b, double *e, int m, const int *seg_beg, const int *seg_end,
                int nseg, double *work) {
    if (!m || !nseg) return;
    k_eq_fill_one<<<stream_grid(m), WG, 0, s>>>(work, m);
    k_eq_rect_seg<<<nseg, WG, 0, s>>>(seg_beg, seg_end, e, work);
    k_eq_rect_apply<<<stream_grid(M.nnzA + m), WG, 0, s>>>(M, b, e, m, work);
}

void eq_invert(hipStream_t s, const double *d, double *dinv, int n, const double *e, double *einv, int m) {
    if (n + m) k_eq_invert<<<stream_grid(n + m), WG, 0, s>>>(d, dinv, n, e, einv, m);
}

int wnorm_scratch_doubles() { return WNORM_MAX * WNORM_BLOCKS; }
void wnorm_batch(hipStream_t s, const WNormBatch &bt, double *out, double *scratch) {
    if (bt.count <= 0) return;
    k_wnorm_partial<<<dim3(WNORM_BLOCKS, bt.count), WG, 0, s>>>(bt, scratch);
    k_wnorm_final<<<bt.count, WG, 0, s>>>(bt, scratch, out);
}

void unscale(hipStream_t s, double *xo, const double *x, const double *d, double sx, int n, double *zo, const double *z,
             const double *e, double sz, double *so, const double *sv, const double *einv, double ss, int m) {
    if (n + 2 * m) k_unscale<<<stream_grid(n + 2 * m), WG, 0, s>>>(xo, x, d, sx, n, zo, z, e, sz, so, sv, einv, ss, m);
}

} // namespace dev
} // namespace chip
