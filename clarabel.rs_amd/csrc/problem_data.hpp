// problem_data.hpp -- DefaultProblemData (default/problemdata.rs:59-312) as the two L4 handles share it: chip_solver
// and chip_batch each own one ProblemData and build it with the same steps: settings, coordinate form of the patterns,
// upload, Ruiz equilibration, the L2 / L3 handles of the equilibrated values.  Per handle: the transform and the GenPow
// powers (chip_solver); the partition, the members' cost scales and norms, uq / ub / negq and the rings (chip_batch).
// Plain host C++ over equilibrate.hpp's launchers; included by solver.cpp and batch.cpp only.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.hpp"
#include "equilibrate.hpp"
#include "host_util.hpp"
#include "ipm_info.hpp"
#include "reequilibrate.hpp"

namespace chip {

// the caller's settings (the defaults when null) with the two line-search fields chip_kkt reads copied into linsys
inline void create_settings(const chip_solver_settings *in, chip_solver_settings &st) {
    if (in) st = *in;
    else chip_solver_settings_default(&st);
    st.linsys.linesearch_backtrack_step = st.linesearch_backtrack_step;
    st.linsys.min_terminate_step_length = st.min_terminate_step_length;
}

// the problem as a create receives it (chip_solver_create: after the transform)
struct ProblemArgs {
    int64_t n, m;
    const uint64_t *Pcolptr, *Prowval;
    const double *Pnzval, *q;
    const uint64_t *Acolptr, *Arowval;
    const double *Anzval, *b;
    int64_t ncones;
    const int32_t *cone_tags;
    const int64_t *cone_dims, *cone_dims2;
    uint64_t nnzP() const { return Pcolptr[n]; }
    uint64_t nnzA() const { return Acolptr[n]; }
    // the entry-parallel passes of equilibrate.hip index P and A together, and A with b / e, in int32
    bool fits_int32() const {
        return n < (1ll << 31) && m < (1ll << 31) && nnzP() + nnzA() + (uint64_t)n + (uint64_t)m < (1ull << 31) &&
               n + 2 * m < (1ll << 31);
    }
};

// max |v[lo .. hi)|, NaN once one was met (the norms of q and b, problemdata.rs:168-189)
inline double absmax_nan(const double *v, int lo, int hi) {
    double r = 0.0;
    for (int i = lo; i < hi; i++) r = std::isnan(v[i]) ? v[i] : std::max(r, std::fabs(v[i]));
    return r;
}

// row and column of every stored entry of P and A, CSC order (dev::EqMats on the host)
struct CooPattern {
    std::vector<int> Prow, Pcol, Arow, Acol;
};
// Column by column, P's entries and then A's: refuses an entry of P below the diagonal and a row of A >= m; an entry
// that passes goes to extra(mat 'P' / 'A', column, row), whose non-zero return (its own fail()) ends the walk
template <typename Extra> int coordinate_form(const ProblemArgs &a, CooPattern &out, Extra extra) {
    const std::vector<int> zp(a.nnzP()), za(a.nnzA());
    out = {zp, zp, za, za};
    for (int64_t j = 0; j < a.n; j++) {
        for (uint64_t p = a.Pcolptr[j]; p < a.Pcolptr[j + 1]; p++) {
            const int64_t r = (int64_t)a.Prowval[p];
            if (r > j) return fail(CHIP_ERR_NOT_TRIU, "P is not upper triangular");
            if (int rc = extra('P', j, r)) return rc;
            out.Prow[p] = (int)r;
            out.Pcol[p] = (int)j;
        }
        for (uint64_t p = a.Acolptr[j]; p < a.Acolptr[j + 1]; p++) {
            const int64_t r = (int64_t)a.Arowval[p];
            if (r >= a.m) return fail(CHIP_ERR_DIM, "A row index out of range");
            if (int rc = extra('A', j, r)) return rc;
            out.Arow[p] = (int)r;
            out.Acol[p] = (int)j;
        }
    }
    return CHIP_OK;
}

// the data on the device, in the owning handle's DevPool: patterns in coordinate form, equilibrated values, scalings
struct ProblemData {
    int n = 0, m = 0, device = 0;
    dev::EqMats M{};
    double *q = nullptr, *b = nullptr, *d = nullptr, *e = nullptr, *dinv = nullptr, *einv = nullptr;
    int64_t update_len(int which) const {
        return which == UPD_P ? M.nnzP : which == UPD_A ? M.nnzA : which == UPD_Q ? n : m;
    }
    // problemdata.rs:86-160; b is capped at the reference's infinity (bcap: that b on the host, for the norms)
    int upload(DevPool &mem, const ProblemArgs &a, const CooPattern &co, std::vector<double> &bcap) {
        n = (int)a.n;
        m = (int)a.m;
        bcap.assign(a.b, a.b + m);
        for (double &v : bcap) v = std::min(v, 1e20); // problemdata.rs:125-127 (get_infinity)
        const size_t nnzP = a.nnzP(), nnzA = a.nnzA();
        int rc;
        int *dPr, *dPc, *dAr, *dAc;
        double *dPx, *dAx;
        if ((rc = mem.upload(&dPr, co.Prow.data(), nnzP)) || (rc = mem.upload(&dPc, co.Pcol.data(), nnzP)) ||
            (rc = mem.upload(&dPx, a.Pnzval, nnzP)) || (rc = mem.upload(&dAr, co.Arow.data(), nnzA)) ||
            (rc = mem.upload(&dAc, co.Acol.data(), nnzA)) || (rc = mem.upload(&dAx, a.Anzval, nnzA)) ||
            (rc = mem.upload(&q, a.q, (size_t)n)) || (rc = mem.upload(&b, bcap.data(), (size_t)m)))
            return rc;
        M = dev::EqMats{dPr, dPc, dPx, (int)nnzP, dAr, dAc, dAx, (int)nnzA};
        return CHIP_OK;
    }
    // (apart from upload: chip_batch places its unscaled copies of q and b between the two)
    int alloc_scalings(DevPool &mem) {
        int rc;
        if ((rc = mem.alloc(&d, (size_t)n)) || (rc = mem.alloc(&e, (size_t)m)) || (rc = mem.alloc(&dinv, (size_t)n)))
            return rc;
        return mem.alloc(&einv, (size_t)m);
    }

    // DefaultProblemData::equilibrate (problemdata.rs:231-312) on stream s: every Ruiz step enqueued without a host
    // synchronisation, the ncost cost scales (1, or one per member) on the device until the end, then in c_out.
    // ruiz_step(bits, cstate) enqueues one step on s: bits are nbits words, cleared here before every step; cstate is
    // [c_k][the step's factor_k], 2 ncost doubles starting at 1.  tail(cstate) runs once everything else is enqueued
    // and before the one synchronisation: what the caller wants done on s, and read back, in the same wait (a
    // re-equilibration's refresh passes; a create passes nothing).  Every write, the initial ones of d, e and cstate
    // included, is ordered on s, so work a live handle still has in flight on s is never overtaken
    template <typename RuizStep>
    int equilibrate(hipStream_t s, const chip_solver_settings &st, const std::vector<ConeSpec> &cones, int ncost,
                    size_t nbits, RuizStep ruiz_step, double *c_out) {
        return equilibrate(s, st, cones, ncost, nbits, ruiz_step, c_out, [](const double *) { return 0; });
    }
    template <typename RuizStep, typename Tail>
    int equilibrate(hipStream_t s, const chip_solver_settings &st, const std::vector<ConeSpec> &cones, int ncost,
                    size_t nbits, RuizStep ruiz_step, double *c_out, Tail tail) {
        const std::vector<double> ones((size_t)std::max({n, m, 2 * ncost}), 1.0);
        if (n) CHIP_HIP(hipMemcpyAsync(d, ones.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
        if (m) CHIP_HIP(hipMemcpyAsync(e, ones.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
        std::fill(c_out, c_out + ncost, 1.0);
        DevPool work;
        double *cstate = nullptr;
        int rc;
        if ((rc = work.alloc(&cstate, 2 * (size_t)ncost))) return rc;
        CHIP_HIP(hipMemcpyAsync(cstate, ones.data(), 2 * (size_t)ncost * 8, hipMemcpyHostToDevice, s));
        if (!st.equilibrate_enable) {
            if (n) CHIP_HIP(hipMemcpyAsync(dinv, ones.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
            if (m) CHIP_HIP(hipMemcpyAsync(einv, ones.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
            rc = tail(cstate);
            CHIP_HIP(hipStreamSynchronize(s));
            return rc;
        }
        unsigned long long *bits = nullptr;
        double *delta = nullptr;
        if ((rc = work.alloc(&bits, nbits)) || (rc = work.alloc(&delta, (size_t)m))) return rc;
        for (int it = 0; it < st.equilibrate_max_iter; it++) {
            CHIP_HIP(hipMemsetAsync(bits, 0, nbits * sizeof(unsigned long long), s));
            ruiz_step(bits, cstate);
        }
        // rectification (compositecone.rs:183-195): SOC, PSDTriangle, Exp, Pow, GenPow take mean(e) / e over their
        // range.  For a batch this is SOC only (it admits no cone past it), and per cone is per member already
        std::vector<int> sb, se;
        for (const ConeSpec &cs : cones)
            if (cs.tag >= CHIP_CONE_SECONDORDER && cs.numel > 0) {
                sb.push_back((int)cs.start);
                se.push_back((int)(cs.start + cs.numel));
            }
        int *dsb = nullptr, *dse = nullptr;
        if (!sb.empty()) {
            if ((rc = work.upload(&dsb, sb)) || (rc = work.upload(&dse, se))) return rc;
            dev::eq_rectify(s, M, b, e, m, dsb, dse, (int)sb.size(), delta);
        }
        dev::eq_invert(s, d, dinv, n, e, einv, m);
        CHIP_HIP(hipGetLastError());
        rc = tail(cstate);
        if (!rc) CHIP_HIP(hipMemcpyAsync(c_out, cstate, (size_t)ncost * 8, hipMemcpyDeviceToHost, s));
        CHIP_HIP(hipStreamSynchronize(s));
        return rc;
    }
    // the load pass of a re-equilibration (reequilibrate.hip), enqueued on s: the caller's raw values from device
    // memory into M.Px, M.Ax, q, b, with b capped as upload caps it; uq / ub (null: none): unscaled copies of q and b
    void reload(hipStream_t s, const double *P_dev, const double *q_dev, const double *A_dev, const double *b_dev,
                double *uq, double *ub) {
        dev::re_load(s, M.Px, nullptr, P_dev, M.nnzP, false);
        dev::re_load(s, M.Ax, nullptr, A_dev, M.nnzA, false);
        dev::re_load(s, q, uq, q_dev, n, false);
        dev::re_load(s, b, ub, b_dev, m, true);
    }
    // the scaled values as the handle holds them (null: not wanted), once the work on `stream` is done
    int get_scaled(hipStream_t stream, double *Px, double *Ax, double *qh, double *bh) const {
        CHIP_HIP(hipStreamSynchronize(stream));
        return copy_scaled(Px, Ax, qh, bh);
    }
    int copy_scaled(double *Px, double *Ax, double *qh, double *bh) const {
        if (Px && M.nnzP) CHIP_HIP(hipMemcpy(Px, M.Px, (size_t)M.nnzP * 8, hipMemcpyDeviceToHost));
        if (Ax && M.nnzA) CHIP_HIP(hipMemcpy(Ax, M.Ax, (size_t)M.nnzA * 8, hipMemcpyDeviceToHost));
        if (qh && n) CHIP_HIP(hipMemcpy(qh, q, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (bh && m) CHIP_HIP(hipMemcpy(bh, b, (size_t)m * 8, hipMemcpyDeviceToHost));
        return CHIP_OK;
    }
    // the KKT system of the equilibrated data: one copy of the scaled values to the host, then L2 and L3 as built from
    // host arrays (a's patterns); *stream: the L2 handle's.  between(kkt): what L2 still needs before L3 reads it
    template <typename Between>
    int create_kkt(const ProblemArgs &a, const double *cone_alphas_or_null, const chip_settings &linsys, chip_kkt **kkt,
                   chip_kktsystem **sys, hipStream_t *stream, Between between) const {
        std::vector<double> Px(M.nnzP), Ax(M.nnzA), qs(n), bs(m);
        int rc;
        if ((rc = copy_scaled(Px.data(), Ax.data(), qs.data(), bs.data()))) return rc;
        if ((rc = chip_kkt_create(kkt, n, m, a.Pcolptr, a.Prowval, Px.data(), a.Acolptr, a.Arowval, Ax.data(), a.ncones,
                                  a.cone_tags, a.cone_dims, a.cone_dims2, cone_alphas_or_null, &linsys, nullptr)))
            return rc;
        if ((rc = between(*kkt))) return rc;
        if ((rc = chip_kktsystem_create(sys, *kkt, a.Pcolptr, a.Prowval, Px.data(), a.Acolptr, a.Arowval, Ax.data(),
                                        qs.data(), bs.data())))
            return rc;
        *stream = (hipStream_t)chip_kkt_stream(*kkt);
        return CHIP_OK;
    }
};

// chip_solution_info of one problem.  Before the first finished solve the status is Unsolved and the other results are
// what the caller passes, zeros either way: chip_solver its own fields, zero-initialised (IpmInfo's initialisers,
// obj_val = obj_val_dual = 0) until a solve writes them; chip_batch, without per-member state yet, IpmInfo() and 0
inline void fill_solution_info(chip_solution_info *out, bool solved_once, const IpmInfo &info, double obj_val,
                               double obj_val_dual, double solve_time, double setup_time, double equilibration_time,
                               double iteration_time) {
    *out = chip_solution_info{solved_once ? info.status : CHIP_SOLVER_UNSOLVED, info.iterations, obj_val, obj_val_dual,
                              info.res_primal, info.res_dual, solve_time, setup_time, equilibration_time,
                              iteration_time};
}

} // namespace chip
