// equilibrate_debug.cpp -- the test hooks of equilibrate.hip's launchers (include/clarabel_hip_testing.h:
// chip_debug_eq_*, chip_debug_wnorm_batch, chip_debug_unscale), one launch of each on host arrays
// (tests/test_equilibrate_passes_gpu.py); empty in the build that ships
#include "debug_stage.hpp"
#include "problem_data.hpp"

#ifdef CHIP_TESTING
#include "../../include/clarabel_hip_testing.h"
using namespace chip;

namespace {
// a private stream for one runner call
struct DebugStream {
    hipStream_t s = nullptr;
    int open() {
        if (chip_device_count() < 1) return fail(CHIP_ERR_NO_DEVICE, "chip_debug_eq: no HIP device");
        CHIP_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return CHIP_OK;
    }
    ~DebugStream() {
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    }
};
bool colptr_ok(const uint64_t *p, int64_t n) {
    if (!p || p[0] != 0) return false;
    for (int64_t j = 0; j < n; j++)
        if (p[j + 1] < p[j]) return false;
    return true;
}
// the coordinate form setup builds (coordinate_form), with every index checked, and its upload
int upload_pattern(const char *fn, DebugStage &st, const ProblemArgs &a, CooPattern &co, double *Px, double *Ax,
                   dev::EqMats *M) {
    const std::string name(fn);
    if (a.n < 0 || a.m < 0 || a.n >= (1ll << 31) || a.m >= (1ll << 31) || !colptr_ok(a.Pcolptr, a.n) ||
        !colptr_ok(a.Acolptr, a.n))
        return fail(CHIP_ERR_ARG, name + ": bad argument");
    if (!a.fits_int32()) return fail(CHIP_ERR_DIM, name + ": sizes out of int32 range");
    if ((a.nnzP() && (!a.Prowval || !Px)) || (a.nnzA() && (!a.Arowval || !Ax)))
        return fail(CHIP_ERR_ARG, name + ": missing data");
    int rc = coordinate_form(a, co, [&](char, int64_t, int64_t r) {
        return r < 0 ? fail(CHIP_ERR_DIM, name + ": row index out of range") : 0;
    });
    if (rc) return rc;
    const int *dPr, *dPc, *dAr, *dAc;
    double *dPx, *dAx;
    if ((rc = st.in(co.Prow.data(), co.Prow.size(), &dPr)) || (rc = st.in(co.Pcol.data(), co.Pcol.size(), &dPc)) ||
        (rc = st.in(co.Arow.data(), co.Arow.size(), &dAr)) || (rc = st.in(co.Acol.data(), co.Acol.size(), &dAc)) ||
        (rc = st.out(Px, (size_t)a.nnzP(), &dPx)) || (rc = st.out(Ax, (size_t)a.nnzA(), &dAx)))
        return rc;
    *M = dev::EqMats{dPr, dPc, dPx, (int)a.nnzP(), dAr, dAc, dAx, (int)a.nnzA()};
    return CHIP_OK;
}
} // namespace

int32_t chip_debug_eq_ruiz_step(int64_t n, int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval, double *Px,
                                const uint64_t *Acolptr, const uint64_t *Arowval, double *Ax, double *q, double *b,
                                double *d, double *e, double *cstate, double min_scaling, double max_scaling) {
    if (!cstate || (n > 0 && (!q || !d)) || (m > 0 && (!b || !e)))
        return fail(CHIP_ERR_ARG, "chip_debug_eq_ruiz_step: bad argument");
    const ProblemArgs a{n, m, Pcolptr, Prowval, Px, q, Acolptr, Arowval, Ax, b, 0, nullptr, nullptr, nullptr};
    DebugStage st;
    DebugStream ds;
    CooPattern co;
    dev::EqMats M{};
    int rc;
    if ((rc = ds.open()) || (rc = upload_pattern("chip_debug_eq_ruiz_step", st, a, co, Px, Ax, &M))) return rc;
    double *dq, *db, *dd, *de, *dc, *partials;
    unsigned long long *bits;
    const size_t nbits = dev::eq_bits_words((int)n, (int)m);
    if ((rc = st.out(q, (size_t)n, &dq)) || (rc = st.out(b, (size_t)m, &db)) || (rc = st.out(d, (size_t)n, &dd)) ||
        (rc = st.out(e, (size_t)m, &de)) || (rc = st.out(cstate, 2, &dc)) || (rc = st.mem.alloc(&bits, nbits)) ||
        (rc = st.mem.alloc(&partials, (size_t)dev::eq_cost_partials())))
        return rc;
    CHIP_HIP(hipMemsetAsync(bits, 0, nbits * sizeof(unsigned long long), ds.s)); // as ProblemData::equilibrate does
    dev::eq_ruiz_step(ds.s, M, dq, db, dd, de, (int)n, (int)m, bits, partials, dc, min_scaling, max_scaling);
    return st.finish(ds.s);
}

int32_t chip_debug_eq_rectify(int64_t n, int64_t m, const uint64_t *Acolptr, const uint64_t *Arowval, double *Ax,
                              double *b, double *e, int32_t nseg, const int32_t *seg_beg, const int32_t *seg_end) {
    if (n < 0 || nseg < 0 || (nseg && (!seg_beg || !seg_end)) || (m > 0 && (!b || !e)))
        return fail(CHIP_ERR_ARG, "chip_debug_eq_rectify: bad argument");
    for (int k = 0; k < nseg; k++)
        if (seg_beg[k] < 0 || seg_beg[k] >= seg_end[k] || seg_end[k] > m)
            return fail(CHIP_ERR_ARG, "chip_debug_eq_rectify: bad segment");
    const std::vector<uint64_t> nop((size_t)n + 1, 0);
    const ProblemArgs a{n, m, nop.data(), nullptr, nullptr, nullptr, Acolptr, Arowval, Ax, b, 0, nullptr, nullptr, nullptr};
    DebugStage st;
    DebugStream ds;
    CooPattern co;
    dev::EqMats M{};
    int rc;
    if ((rc = ds.open()) || (rc = upload_pattern("chip_debug_eq_rectify", st, a, co, nullptr, Ax, &M))) return rc;
    double *db, *de, *work;
    const int *dsb, *dse;
    if ((rc = st.out(b, (size_t)m, &db)) || (rc = st.out(e, (size_t)m, &de)) || (rc = st.mem.alloc(&work, (size_t)m)) ||
        (rc = st.in((const int *)seg_beg, (size_t)nseg, &dsb)) || (rc = st.in((const int *)seg_end, (size_t)nseg, &dse)))
        return rc;
    dev::eq_rectify(ds.s, M, db, de, (int)m, dsb, dse, nseg, work);
    return st.finish(ds.s);
}

int32_t chip_debug_eq_invert(const double *d, double *dinv, int64_t n, const double *e, double *einv, int64_t m) {
    if (n < 0 || m < 0 || n + m >= (1ll << 31) || (n > 0 && (!d || !dinv)) || (m > 0 && (!e || !einv)))
        return fail(CHIP_ERR_ARG, "chip_debug_eq_invert: bad argument");
    DebugStage st;
    DebugStream ds;
    int rc;
    if ((rc = ds.open())) return rc;
    const double *dd, *de;
    double *ddi, *dei;
    if ((rc = st.in(d, (size_t)n, &dd)) || (rc = st.out(dinv, (size_t)n, &ddi)) || (rc = st.in(e, (size_t)m, &de)) ||
        (rc = st.out(einv, (size_t)m, &dei)))
        return rc;
    dev::eq_invert(ds.s, dd, ddi, (int)n, de, dei, (int)m);
    return st.finish(ds.s);
}

int32_t chip_debug_wnorm_batch(int32_t count, const double *const *v, const double *const *w, const int32_t *n,
                               const int32_t *slot, int32_t nslots, double *out) {
    if (count < 0 || count > dev::WNORM_MAX || nslots < 0 || (count && (!v || !w || !n || !slot || !out)))
        return fail(CHIP_ERR_ARG, "chip_debug_wnorm_batch: bad argument");
    for (int j = 0; j < count; j++)
        if (n[j] < 0 || slot[j] < 0 || slot[j] >= nslots || (n[j] > 0 && (!v[j] || !w[j])))
            return fail(CHIP_ERR_ARG, "chip_debug_wnorm_batch: bad spec");
    // (one device buffer per host array: an array that serves two specs must have one length)
    for (int j = 0; j < count; j++)
        for (int k = 0; k < count; k++)
            for (const double *p : {v[k], w[k]})
                if (n[j] > 0 && n[k] > 0 && n[j] != n[k] && (p == v[j] || p == w[j]))
                    return fail(CHIP_ERR_ARG, "chip_debug_wnorm_batch: one array with two lengths");
    DebugStage st;
    DebugStream ds;
    int rc;
    if ((rc = ds.open())) return rc;
    dev::WNormBatch bt{};
    bt.count = count;
    for (int j = 0; j < count; j++) {
        const double *dv = nullptr, *dw = nullptr;
        if (n[j] > 0 && ((rc = st.in(v[j], (size_t)n[j], &dv)) || (rc = st.in(w[j], (size_t)n[j], &dw)))) return rc;
        bt.s[j] = dev::WNormSpec{dv, dw, n[j], slot[j]};
    }
    double *dout, *scratch;
    if ((rc = st.out(out, (size_t)nslots, &dout)) || (rc = st.mem.alloc(&scratch, (size_t)dev::wnorm_scratch_doubles())))
        return rc;
    dev::wnorm_batch(ds.s, bt, dout, scratch);
    return st.finish(ds.s);
}

int32_t chip_debug_unscale(double *xo, const double *x, const double *d, double sx, int64_t n, double *zo,
                           const double *z, const double *e, double sz, double *so, const double *sv, const double *einv,
                           double ss, int64_t m) {
    if (n < 0 || m < 0 || n + 2 * m >= (1ll << 31) || (n > 0 && (!xo || !x || !d)) ||
        (m > 0 && (!zo || !z || !e || !so || !sv || !einv)))
        return fail(CHIP_ERR_ARG, "chip_debug_unscale: bad argument");
    DebugStage st;
    DebugStream ds;
    int rc;
    if ((rc = ds.open())) return rc;
    double *dxo, *dzo, *dso;
    const double *dx, *dd, *dz, *de, *dsv, *dei;
    if ((rc = st.out(xo, (size_t)n, &dxo)) || (rc = st.in(x, (size_t)n, &dx)) || (rc = st.in(d, (size_t)n, &dd)) ||
        (rc = st.out(zo, (size_t)m, &dzo)) || (rc = st.in(z, (size_t)m, &dz)) || (rc = st.in(e, (size_t)m, &de)) ||
        (rc = st.out(so, (size_t)m, &dso)) || (rc = st.in(sv, (size_t)m, &dsv)) || (rc = st.in(einv, (size_t)m, &dei)))
        return rc;
    dev::unscale(ds.s, dxo, dx, dd, sx, (int)n, dzo, dz, de, sz, dso, dsv, dei, ss, (int)m);
    return st.finish(ds.s);
}
#endif
