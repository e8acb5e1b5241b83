// solver.cpp -- L4 of the C ABI: DefaultSolver::new(P, q, A, b, cones, settings).solve() on one GPU.
//   setup: problem_data.hpp's steps, shared with batch.cpp: DefaultProblemData::new + equilibrate (default/
//          problemdata.rs:59-312) with the data on the device, then the L2 / L3 handles of the equilibrated values;
//   solve: the interior-point loop of core/solver.rs:242-464 over the L3 entry points, with DefaultInfo's update /
//          check_termination / post_process (default/info.rs:80-389) and DefaultSolution::post_process
//          (default/solution.rs:68-111) on the host: only scalars cross the boundary per iteration.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "engine.hpp"
#include "equilibrate.hpp"
#include "host_util.hpp"
#include "ipm_info.hpp"
#include "problem_data.hpp"
#include "problem_transform.hpp"
#include "problem_update.hpp"

using namespace chip;

namespace {
enum { PRIMAL_DUAL = 0, DUAL = 1 }; // ScalingStrategy (core/solver.rs:77-80)
} // namespace

struct chip_solver {
    chip_solver_settings st{};
    DevPool mem;
    ProblemData pd;
    double c = 1.0, normq = 0.0, normb = 0.0;
    chip_kkt *kkt = nullptr;
    chip_kktsystem *sys = nullptr;
    hipStream_t stream = nullptr;
    bool symmetric = true, allows_primal_dual = true;
    int64_t degree = 0;
    chip_vars vars{}, lhs{}, rhs{}, prev{};
    double *rx = nullptr, *rz = nullptr, *rx_inf = nullptr, *rz_inf = nullptr, *Pxv = nullptr;
    double *xo = nullptr, *so = nullptr, *zo = nullptr; // the unscaled solution (original sizes n_out, m_out)
    // presolve / chordal decomposition (problem_transform.cpp): tf is null unless one of them changed the problem; then
    // pd.n, pd.m are the internal sizes and the reverse maps live on the device
    std::unique_ptr<ProblemTransform> tf;
    int n_out = 0, m_out = 0;
    int32_t *rv_mode = nullptr;
    int64_t *rv_ptr = nullptr, *rv_src = nullptr;
    double transform_time = 0, completion_time = 0;
    IpmInfo info; // (its out5: r_tau, dot_qx, dot_bz, dot_sz, dot_xPx of the last residual update)
    double solve_time = 0;
    double setup_time = 0, equilibration_time = 0, iteration_time = 0;
    double obj_val = 0, obj_val_dual = 0;
    bool solved_once = false;
    // the data updates (problem_update.hip), allocated by the first one: host-form staging (grown to the longest
    // update), the last-occurrence scratch (-1 between updates), the index check's flag and the reductions
    UpdateStage stage;
    int *pos = nullptr, *flag = nullptr;
    unsigned long long *npart = nullptr;
    double *nout = nullptr;
    // a re-equilibration (chip_reequilibrate_problem) runs create's Ruiz loop again: the cones it rectifies, and the
    // cost partials of a Ruiz step, allocated by the first one
    std::vector<ConeSpec> cones;
    double *eq_partials = nullptr;
    long req_launches = 0, req_syncs = 0; // of the last re-equilibration

    ~chip_solver() {
        if (stream) (void)hipStreamSynchronize(stream);
        chip_kktsystem_destroy(sys);
        chip_kkt_destroy(kkt);
    }
    int alloc_vars(chip_vars &v) {
        int rc;
        if ((rc = mem.alloc(&v.x, (size_t)pd.n)) || (rc = mem.alloc(&v.z, (size_t)pd.m)) ||
            (rc = mem.alloc(&v.s, (size_t)pd.m)))
            return rc;
        v.tau = v.kappa = 1.0;
        return CHIP_OK;
    }
    int copy_vars(chip_vars &dst, const chip_vars &src) {
        if (pd.n) CHIP_HIP(hipMemcpyAsync(dst.x, src.x, (size_t)pd.n * 8, hipMemcpyDeviceToDevice, stream));
        if (pd.m) CHIP_HIP(hipMemcpyAsync(dst.z, src.z, (size_t)pd.m * 8, hipMemcpyDeviceToDevice, stream));
        if (pd.m) CHIP_HIP(hipMemcpyAsync(dst.s, src.s, (size_t)pd.m * 8, hipMemcpyDeviceToDevice, stream));
        dst.tau = src.tau;
        dst.kappa = src.kappa;
        return CHIP_OK;
    }
    int default_start();
    int residuals_and_info();
    int backtrack_step_to_barrier(double alpha_init, double *alpha_out);
    int post_process();
    int update_work();
    static constexpr const char *UPD_PREFIX = "chip_problem_update_";
    static int update_args(chip_solver *h, int which, const void *idx, const double *vals, int64_t k);
    int stage_upload(const uint64_t *idx, const double *vals, size_t k) { return stage.upload(stream, idx, vals, k); }
    int update(int which, const int64_t *idx_dev, const double *vals_dev, int k);
    int reequilibrate_gate(const char *fn);
    int stage_upload4(const double *const src[4], const size_t len[4], const double *at[4]) {
        return stage.upload4(stream, src, len, at, &req_launches, &req_syncs);
    }
    int reequilibrate(const double *P_dev, const double *q_dev, const double *A_dev, const double *b_dev);
    double t_solve0 = 0;
};

void chip_solver_settings_default(chip_solver_settings *s) {
    std::memset(s, 0, sizeof(*s));
    chip_settings_default(&s->linsys);
    s->max_iter = 200;
    s->time_limit = std::numeric_limits<double>::infinity();
    s->max_step_fraction = 0.99;
    s->tol_gap_abs = 1e-8;
    s->tol_gap_rel = 1e-8;
    s->tol_feas = 1e-8;
    s->tol_infeas_abs = 1e-8;
    s->tol_infeas_rel = 1e-8;
    s->tol_ktratio = 1e-6;
    s->reduced_tol_gap_abs = 5e-5;
    s->reduced_tol_gap_rel = 5e-5;
    s->reduced_tol_feas = 1e-4;
    s->reduced_tol_infeas_abs = 5e-12;
    s->reduced_tol_infeas_rel = 5e-5;
    s->reduced_tol_ktratio = 1e-4;
    s->equilibrate_enable = 1;
    s->equilibrate_max_iter = 10;
    s->equilibrate_min_scaling = 1e-4;
    s->equilibrate_max_scaling = 1e4;
    s->linesearch_backtrack_step = 0.8;
    s->min_switch_step_length = 0.1;
    s->min_terminate_step_length = 1e-4;
    // the reference enables presolve and chordal decomposition by default; here both stay off until measured, so that a
    // caller gets the problem it passes in
    s->presolve_enable = 0;
    s->chordal_decomposition_enable = 0;
    s->chordal_decomposition_merge_method = CHIP_MERGE_CLIQUE_GRAPH;
    s->chordal_decomposition_compact = 1;
    s->chordal_decomposition_complete_dual = 1;
}

int32_t chip_solver_create(chip_solver **out, int64_t n, int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval,
                           const double *Pnzval, const double *q, const uint64_t *Acolptr, const uint64_t *Arowval,
                           const double *Anzval, const double *b, int64_t ncones, const int32_t *cone_tags,
                           const int64_t *cone_dims, const int64_t *cone_dims2, const double *cone_alphas_or_null,
                           const double *genpow_alphas_or_null, const chip_solver_settings *settings) {
    if (!out || n < 0 || m < 0 || !Pcolptr || !Acolptr || ncones < 0 || (ncones && (!cone_tags || !cone_dims)))
        return fail(CHIP_ERR_ARG, "chip_solver_create: bad argument");
    *out = nullptr;
    const double t0 = now_s();
    std::unique_ptr<chip_solver> h(new chip_solver());
    chip_solver_settings &st = h->st;
    create_settings(settings, st);
    if (st.linsys.device == CHIP_DEVICE_HOST_ONLY || chip_device_count() < 1)
        return fail(CHIP_ERR_NO_DEVICE, "chip_solver_create: no HIP device (the product has no CPU fallback)");
    if ((Pcolptr[n] && (!Prowval || !Pnzval)) || (Acolptr[n] && (!Arowval || !Anzval)) || (n && !q) || (m && !b))
        return fail(CHIP_ERR_ARG, "chip_solver_create: missing data");
    h->n_out = (int)std::min<int64_t>(n, INT32_MAX);
    h->m_out = (int)std::min<int64_t>(m, INT32_MAX);
    // ---- presolve and chordal decomposition (problemdata.rs:59-165): everything below sees the transformed problem
    ProblemArgs a{n,      m,         Pcolptr,   Prowval,  Pnzval, q, Acolptr, Arowval, Anzval, b,
                  ncones, cone_tags, cone_dims, cone_dims2};
    if (st.presolve_enable || st.chordal_decomposition_enable) {
        if (n >= (1ll << 31) || m >= (1ll << 31)) return fail(CHIP_ERR_DIM, "chip_solver_create: sizes out of int32 range");
        for (uint64_t k = 0; k < Acolptr[n]; k++)
            if ((int64_t)Arowval[k] >= m) return fail(CHIP_ERR_DIM, "A row index out of range");
        std::unique_ptr<ProblemTransform> tf(new ProblemTransform());
        int rc0 = transform_build(n, m, Pcolptr, Prowval, Pnzval, q, Acolptr, Arowval, Anzval, b, ncones, cone_tags,
                                  cone_dims, cone_dims2, cone_alphas_or_null, transform_options(st), *tf);
        if (rc0) return rc0;
        h->transform_time = tf->transform_time;
        if (tf->active()) {
            const ProblemTransform &t = *tf;
            a = {t.n2,        t.m2,        t.Pp.data(), t.Pi.data(), t.Px.data(), t.q.data(), t.Ap.data(),
                 t.Ai.data(), t.Ax.data(), t.b.data(),  (int64_t)t.tags.size(), t.tags.data(), t.dims.data(),
                 t.dims2.data()};
            cone_alphas_or_null = t.alphas.data();
            h->tf = std::move(tf);
        }
    }
    if (!a.fits_int32()) return fail(CHIP_ERR_DIM, "chip_solver_create: sizes out of int32 range");
    std::vector<ConeSpec> &cones = h->cones;
    int64_t mm = 0, p = 0, nHs = 0;
    if (build_cone_specs(a.ncones, a.cone_tags, a.cone_dims, a.cone_dims2, cones, mm, p, nHs))
        return fail(CHIP_ERR_ARG, "chip_solver_create: bad cone");
    if (mm != a.m) return fail(CHIP_ERR_DIM, "chip_solver_create: cone dimensions do not add up to m");
    ProblemData &pd = h->pd;
    if (st.linsys.device >= 0) CHIP_HIP(hipSetDevice(st.linsys.device));
    CHIP_HIP(hipGetDevice(&pd.device));
    // ---- the data (problemdata.rs:86-160), the norms of the unequilibrated q and b, the equilibration (own stream)
    CooPattern co;
    std::vector<double> bcap;
    DevPool &mem = h->mem;
    int rc;
    if ((rc = coordinate_form(a, co, [](char, int64_t, int64_t) { return 0; })) || (rc = pd.upload(mem, a, co, bcap)) ||
        (rc = pd.alloc_scalings(mem)))
        return rc;
    h->normq = absmax_nan(a.q, 0, pd.n);
    h->normb = absmax_nan(bcap.data(), 0, pd.m);
    const double te = now_s();
    DevPool work;
    double *partials = nullptr;
    if ((rc = work.alloc(&partials, (size_t)dev::eq_cost_partials()))) return rc;
    hipStream_t s_eq = nullptr;
    CHIP_HIP(hipStreamCreateWithFlags(&s_eq, hipStreamNonBlocking));
    auto ruiz_step = [&](unsigned long long *bits, double *cstate) {
        dev::eq_ruiz_step(s_eq, pd.M, pd.q, pd.b, pd.d, pd.e, pd.n, pd.m, bits, partials, cstate,
                          st.equilibrate_min_scaling, st.equilibrate_max_scaling);
    };
    rc = pd.equilibrate(s_eq, st, cones, 1, dev::eq_bits_words(pd.n, pd.m), ruiz_step, &h->c);
    (void)hipStreamDestroy(s_eq);
    if (rc) return rc;
    h->equilibration_time = now_s() - te;
    // ---- the KKT system of the equilibrated data; the L2 handle takes the GenPow cones' powers before L3 reads it
    rc = pd.create_kkt(a, cone_alphas_or_null, st.linsys, &h->kkt, &h->sys, &h->stream, [&](chip_kkt *kkt) {
        const double *ga = genpow_alphas_or_null;
        for (int64_t i = 0; i < a.ncones; i++) {
            const int32_t tag = a.cone_tags[i];
            if (tag == CHIP_CONE_GENPOWER) {
                if (!ga) return fail(CHIP_ERR_ARG, "chip_solver_create: GenPow cone without its powers");
                if (int rc1 = chip_kkt_set_genpow_alpha(kkt, i, ga)) return rc1;
                ga += a.cone_dims[i];
            }
            if (tag == CHIP_CONE_EXPONENTIAL || tag == CHIP_CONE_POWER || tag == CHIP_CONE_GENPOWER)
                h->symmetric = false;
            if (tag == CHIP_CONE_GENPOWER) h->allows_primal_dual = false; // genpowcone.rs:96-98
        }
        return (int)CHIP_OK;
    });
    if (rc || (rc = chip_kkt_degree(h->kkt, &h->degree))) return rc;
    if ((rc = h->alloc_vars(h->vars)) || (rc = h->alloc_vars(h->lhs)) || (rc = h->alloc_vars(h->rhs)) ||
        (rc = h->alloc_vars(h->prev)))
        return rc;
    if ((rc = mem.alloc(&h->rx, (size_t)pd.n)) || (rc = mem.alloc(&h->rz, (size_t)pd.m)) ||
        (rc = mem.alloc(&h->rx_inf, (size_t)pd.n)) || (rc = mem.alloc(&h->rz_inf, (size_t)pd.m)) ||
        (rc = mem.alloc(&h->Pxv, (size_t)pd.n)) || (rc = mem.alloc(&h->xo, (size_t)h->n_out)) ||
        (rc = mem.alloc(&h->so, (size_t)h->m_out)) || (rc = mem.alloc(&h->zo, (size_t)h->m_out)))
        return rc;
    if (h->tf) {
        const ProblemTransform &t = *h->tf;
        if ((rc = mem.upload(&h->rv_mode, t.mode.data(), t.mode.size())) ||
            (rc = mem.upload(&h->rv_ptr, t.ptr.data(), t.ptr.size())) ||
            (rc = mem.upload(&h->rv_src, t.src.data(), t.src.size())))
            return rc;
    }
    h->setup_time = now_s() - t0;
    *out = h.release();
    return CHIP_OK;
}

void chip_solver_destroy(chip_solver *h) {
    if (!h) return;
    (void)hipSetDevice(h->pd.device);
    delete h;
}

// default_start (core/solver.rs:525-541)
int chip_solver::default_start() {
    int rc;
    if (symmetric) {
        // set_identity_scaling: the scaling at s = z = the cones' unit vector is the identity (W = I)
        if ((rc = chip_kkt_unit_initialization_dev(kkt, rhs.z, rhs.s))) return rc;
        if ((rc = chip_kkt_update_scaling_dev(kkt, rhs.z, rhs.z, 1.0, PRIMAL_DUAL)) < 0) return rc;
        if ((rc = chip_kktsystem_update(sys)) < 0) return rc; // (the reference ignores the bool here)
        if ((rc = chip_kktsystem_solve_initial_point(sys, &vars)) < 0) return rc;
        return chip_variables_symmetric_initialization(sys, &vars);
    }
    return chip_variables_unit_initialization(sys, &vars);
}

// Residuals::update + calc_mu's dot + DefaultInfo::update (info.rs:113-178) with ONE device-to-host copy
int chip_solver::residuals_and_info() {
    dev::WNormBatch wn{};
    const int n = pd.n, m = pd.m;
    const dev::WNormSpec specs[8] = {{vars.x, pd.d, n, 0},    {vars.z, pd.e, m, 1},  {vars.s, pd.einv, m, 2},
                                     {rx_inf, pd.dinv, n, 3}, {Pxv, pd.dinv, n, 4},  {rz_inf, pd.einv, m, 5},
                                     {rz, pd.einv, m, 6},     {rx, pd.dinv, n, 7}};
    for (int k = 0; k < 8; k++) wn.s[k] = specs[k];
    wn.count = 8;
    double sq[8];
    int rc = residuals_update_wnorms(sys, &vars, rx, rz, rx_inf, rz_inf, Pxv, info.out5, &wn, sq);
    if (rc) return rc;
    ipm_info_update(info, sq, vars.tau, vars.kappa, c, normq, normb);
    solve_time = setup_time + (now_s() - t_solve0);
    return CHIP_OK;
}

// backtrack_step_to_barrier (core/solver.rs:571-584)
int chip_solver::backtrack_step_to_barrier(double alpha_init, double *alpha_out) {
    double alpha = alpha_init;
    for (int k = 0; k < 50; k++) {
        double barrier = 0.0;
        int rc = chip_variables_barrier(sys, &vars, &lhs, alpha, &barrier);
        if (rc) return rc;
        if (barrier < 1.0) break;
        alpha *= st.linesearch_backtrack_step;
    }
    *alpha_out = alpha;
    return CHIP_OK;
}

// info.post_process (info.rs:95-105) + solution.post_process (solution.rs:68-111) with variables.unscale
int chip_solver::post_process() {
    double scaleinv, scale_z;
    ipm_post_process(info, st, vars.tau, vars.kappa, c, &obj_val, &obj_val_dual, &scaleinv, &scale_z);
    if (!tf) {
        dev::unscale(stream, xo, vars.x, pd.d, scaleinv, pd.n, zo, vars.z, pd.e, scale_z, so, vars.s, pd.einv, scaleinv,
                     pd.m);
    } else { // decomp_reverse + reverse_presolve (solution.rs:94-110) in one gather, straight from the scaled variables
        const dev::RvMaps mp{rv_mode, rv_ptr, rv_src};
        dev::transform_reverse(stream, mp, n_out, m_out, xo, vars.x, pd.d, scaleinv, so, vars.s, pd.einv, scaleinv, zo,
                               vars.z, pd.e, scale_z);
    }
    CHIP_HIP(hipGetLastError());
    CHIP_HIP(hipStreamSynchronize(stream));
    if (tf && tf->decomposed() && tf->opt.complete_dual) { // psd_completion on the host: a few dense blocks per solve
        const double tc = now_s();
        std::vector<double> zh((size_t)m_out);
        if (m_out) CHIP_HIP(hipMemcpy(zh.data(), zo, (size_t)m_out * 8, hipMemcpyDeviceToHost));
        transform_complete_dual(*tf, zh.data());
        if (m_out) CHIP_HIP(hipMemcpy(zo, zh.data(), (size_t)m_out * 8, hipMemcpyHostToDevice));
        completion_time = now_s() - tc;
    }
    solve_time = setup_time + (now_s() - t_solve0);
    return CHIP_OK;
}

// IPSolver::solve (core/solver.rs:242-464)
int32_t chip_solver_solve(chip_solver *h) {
    if (!h) return CHIP_ERR_ARG;
    CHIP_HIP(hipSetDevice(h->pd.device));
    IpmInfo &info = h->info;
    info = IpmInfo(); // info.reset; the previous-iterate scalars start from the same values on every solve
    h->solve_time = 0;
    h->t_solve0 = now_s();
    int rc;
    if ((rc = h->default_start()) < 0) return rc;
    CHIP_HIP(hipStreamSynchronize(h->stream));
    const double t_loop0 = now_s();
    int scaling = h->allows_primal_dual ? PRIMAL_DUAL : DUAL;
    int iter = 0;
    double sigma = 1.0, alpha = 0.0, mu = 0.0;
    const bool sym = h->symmetric;
    const chip_solver_settings &st = h->st;
    while (true) {
        if ((rc = h->residuals_and_info())) return rc;
        if ((rc = chip_variables_calc_mu(h->sys, &h->vars, info.out5[3], &mu))) return rc;
        info.iterations = iter; // save_scalars
        if (ipm_check_termination(info, st, iter, h->solve_time)) {
            // strategy_checkpoint_insufficient_progress (core/solver.rs:586-608)
            if (info.status != CHIP_SOLVER_INSUFFICIENT_PROGRESS) break;
            ipm_reset_to_prev(info);
            if ((rc = h->copy_vars(h->vars, h->prev))) return rc;
            if (!sym && scaling == PRIMAL_DUAL) { // Update(s) => {scaling = s; continue}: alpha is kept here
                info.status = CHIP_SOLVER_UNSOLVED; // (core/solver.rs:322), unlike the two checkpoints below
                scaling = DUAL;
                continue;
            }
            break;
        }
        // scale cones; the device verdict arrives with the KKT update below (strategy_checkpoint_is_scaling_success)
        if ((rc = chip_kkt_update_scaling_dev(h->kkt, h->vars.s, h->vars.z, mu, scaling)) < 0) return rc;
        iter++;
        rc = chip_kktsystem_update(h->sys);
        if (rc < 0) return rc;
        bool ok = rc == 1;
        if (!ok) {
            const int sc = chip_kkt_scaling_ok(h->kkt);
            if (sc < 0) return sc;
            if (sc == 0) { // the reference stops before counting the iteration
                iter--;
                info.status = CHIP_SOLVER_NUMERICAL_ERROR;
                break;
            }
        }
        if ((rc = chip_variables_affine_step_rhs(h->sys, &h->rhs, h->rx, h->rz, info.out5[0], &h->vars))) return rc;
        if (ok) {
            rc = chip_kktsystem_solve(h->sys, &h->lhs, &h->rhs, &h->vars, CHIP_STEP_AFFINE);
            if (rc < 0) return rc;
            ok = rc == 1;
        }
        if (ok) {
            if ((rc = chip_variables_calc_step_length(h->sys, &h->vars, &h->lhs, CHIP_STEP_AFFINE, st.max_step_fraction,
                                                      &alpha)))
                return rc;
            sigma = std::pow(1.0 - alpha, 3);
            const double mm = iter > 1 ? 1.0 : alpha;
            if ((rc = chip_variables_combined_step_rhs(h->sys, &h->rhs, h->rx, h->rz, info.out5[0], &h->vars, &h->lhs,
                                                       sigma, mu, mm)))
                return rc;
            rc = chip_kktsystem_solve(h->sys, &h->lhs, &h->rhs, &h->vars, CHIP_STEP_COMBINED);
            if (rc < 0) return rc;
            ok = rc == 1;
        }
        // strategy_checkpoint_numerical_error (core/solver.rs:610-628)
        if (!ok) {
            alpha = 0.0;
            if (!sym && scaling == PRIMAL_DUAL) {
                scaling = DUAL;
                continue;
            }
            info.status = CHIP_SOLVER_NUMERICAL_ERROR;
            break;
        }
        if ((rc = chip_variables_calc_step_length(h->sys, &h->vars, &h->lhs, CHIP_STEP_COMBINED, st.max_step_fraction,
                                                  &alpha)))
            return rc;
        if (!sym && scaling == DUAL && (rc = h->backtrack_step_to_barrier(alpha, &alpha))) return rc;
        // strategy_checkpoint_small_step (core/solver.rs:630-654)
        if (!sym && scaling == PRIMAL_DUAL && alpha < st.min_switch_step_length) {
            alpha = 0.0;
            scaling = DUAL;
            continue;
        } else if (alpha <= std::max(0.0, st.min_terminate_step_length)) {
            alpha = 0.0;
            info.status = CHIP_SOLVER_INSUFFICIENT_PROGRESS;
            break;
        }
        // save_prev_iterate (info.rs:233-242) + add_step (variables.rs:162-168): the new iterate is written into the
        // previous iterate's buffers (the arithmetic of chip_variables_add_step) and the two sets swap, so keeping the
        // previous iterate costs no copy
        ipm_save_prev(info);
        chip_vars &nv = h->prev, &v = h->vars, &st_ = h->lhs;
        dev::waxpby(h->stream, nv.x, alpha, st_.x, 1.0, v.x, h->pd.n);
        dev::waxpby(h->stream, nv.s, alpha, st_.s, 1.0, v.s, h->pd.m);
        dev::waxpby(h->stream, nv.z, alpha, st_.z, 1.0, v.z, h->pd.m);
        CHIP_HIP(hipGetLastError());
        nv.tau = v.tau;
        nv.tau += alpha * st_.tau;
        nv.kappa = v.kappa;
        nv.kappa += alpha * st_.kappa;
        std::swap(h->vars, h->prev);
    }
    h->iteration_time = now_s() - t_loop0;
    if (alpha == 0.0) info.iterations = iter;
    if ((rc = h->post_process())) return rc;
    h->solved_once = true;
    return CHIP_OK;
}

int32_t chip_solver_get_solution(chip_solver *h, double *x, double *s, double *z, chip_solution_info *out) {
    if (!h) return CHIP_ERR_ARG;
    CHIP_HIP(hipSetDevice(h->pd.device));
    if (h->solved_once) {
        if (x && h->n_out) CHIP_HIP(hipMemcpy(x, h->xo, (size_t)h->n_out * 8, hipMemcpyDeviceToHost));
        if (s && h->m_out) CHIP_HIP(hipMemcpy(s, h->so, (size_t)h->m_out * 8, hipMemcpyDeviceToHost));
        if (z && h->m_out) CHIP_HIP(hipMemcpy(z, h->zo, (size_t)h->m_out * 8, hipMemcpyDeviceToHost));
    } else {
        if (x) std::fill(x, x + h->n_out, 0.0);
        if (s) std::fill(s, s + h->m_out, 0.0);
        if (z) std::fill(z, z + h->m_out, 0.0);
    }
    if (out)
        fill_solution_info(out, h->solved_once, h->info, h->obj_val, h->obj_val_dual, h->solve_time, h->setup_time,
                           h->equilibration_time, h->iteration_time);
    return CHIP_OK;
}

int32_t chip_solver_get_solution_dev(chip_solver *h, double **x_dev, double **s_dev, double **z_dev) {
    if (!h) return CHIP_ERR_ARG;
    if (x_dev) *x_dev = h->xo;
    if (s_dev) *s_dev = h->so;
    if (z_dev) *z_dev = h->zo;
    return CHIP_OK;
}

int32_t chip_solver_get_equilibration(chip_solver *h, double *d, double *e, double *c) {
    if (!h) return CHIP_ERR_ARG;
    CHIP_HIP(hipSetDevice(h->pd.device));
    if (d && h->pd.n) CHIP_HIP(hipMemcpy(d, h->pd.d, (size_t)h->pd.n * 8, hipMemcpyDeviceToHost));
    if (e && h->pd.m) CHIP_HIP(hipMemcpy(e, h->pd.e, (size_t)h->pd.m * 8, hipMemcpyDeviceToHost));
    if (c) *c = h->c;
    return CHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Data updates (default/data_updating.rs): new values on the fixed patterns, scaled with the equilibration of the
// setup (d, e, c are never recomputed), written into the solver's arrays and from there, on the device, into K's
// store, the L3 mirrors and vectors, with the norms and max |P_ii| that setup derived from the values.  The host forms
// upload into the handle's staging and take the device path.
// ---------------------------------------------------------------------------------------------------------------
int chip_solver::update_work() {
    if (flag) return CHIP_OK;
    const size_t len = (size_t)std::max({pd.M.nnzP, pd.M.nnzA, pd.n, pd.m});
    int rc;
    if ((rc = mem.alloc(&pos, len)) || (rc = mem.alloc(&npart, (size_t)dev::pu_norm_partials())) ||
        (rc = mem.alloc(&nout, 3)) || (rc = mem.alloc(&flag, 1)))
        return rc;
    CHIP_HIP(hipMemset(pos, 0xff, std::max<size_t>(len, 1) * sizeof(int))); // every slot -1
    return CHIP_OK;
}

// one update of P, A, q or b: idx_dev == nullptr is the full form (k == the length, checked by the caller)
int chip_solver::update(int which, const int64_t *idx_dev, const double *vals_dev, int k) {
    int rc;
    if ((rc = update_work())) return rc;
    const int64_t len = pd.update_len(which);
    const dev::EqMats &M = pd.M;
    hipStream_t s = stream;
    if (idx_dev) { // the whole index list is checked before anything is written
        int bad = 0;
        CHIP_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
        dev::pu_validate(s, idx_dev, k, len, flag);
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s));
        CHIP_HIP(hipStreamSynchronize(s));
        if (bad) return fail(CHIP_ERR_DIM, update_fn(UPD_PREFIX, which) + ": an index is out of range (nothing changed)");
    }
    dev::PuTarget t{};
    switch (which) { // update_P / _A / _q / _b (data_updating.rs:96-170)
    case UPD_P: t = {M.Px, (int)len, M.Prow, M.Pcol, pd.d, pd.d, c, true}; break;
    case UPD_A: t = {M.Ax, (int)len, M.Arow, M.Acol, pd.e, pd.d, 1.0, false}; break;
    case UPD_Q: t = {pd.q, (int)len, nullptr, nullptr, pd.d, nullptr, c, true}; break;
    default: t = {pd.b, (int)len, nullptr, nullptr, pd.e, nullptr, 1.0, false}; break;
    }
    if (idx_dev) dev::pu_write_partial(s, t, idx_dev, vals_dev, k, pos);
    else dev::pu_write_full(s, t, vals_dev);
    CHIP_HIP(hipGetLastError());
    // the copies the loop reads: K's values (only the touched entries of a partial update), the L3 mirrors and vectors
    if (which == UPD_P || which == UPD_A) {
        const double *src = which == UPD_P ? M.Px : M.Ax;
        if ((rc = kkt_update_values_dev(kkt, which, src, idx_dev, idx_dev ? k : (int)len))) return rc;
    }
    if ((rc = kktsystem_update_data_dev(sys, which == UPD_P ? M.Px : nullptr, which == UPD_A ? M.Ax : nullptr,
                                        which == UPD_Q ? pd.q : nullptr, which == UPD_B ? pd.b : nullptr)))
        return rc;
    // the scalars setup derived from the values: normq / normb as the lazy getters recompute them (problemdata.rs:
    // 168-189) and max |P_ii| of the static regulariser; read back in the call's one synchronisation
    const int mask = which == UPD_Q ? 1 : which == UPD_B ? 2 : which == UPD_P ? 4 : 0;
    double hn[3] = {0, 0, 0};
    if (mask) {
        dev::pu_norms(s, mask, pd.q, pd.dinv, pd.n, pd.b, pd.einv, pd.m, M.Prow, M.Pcol, M.Px, M.nnzP, npart, nout);
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipMemcpyAsync(hn, nout, sizeof(hn), hipMemcpyDeviceToHost, s));
    }
    CHIP_HIP(hipStreamSynchronize(s));
    if (mask & 1) normq = hn[0] * (1.0 / c);
    if (mask & 2) normb = hn[1];
    if (mask & 4) kkt_set_static_diag_max(kkt, hn[2]);
    return CHIP_OK;
}

int chip_solver::update_args(chip_solver *h, int which, const void *idx, const double *vals, int64_t k) {
    const std::string fn = update_fn(UPD_PREFIX, which);
    return chip::update_args(fn, h, idx, vals, k, h ? h->pd.update_len(which) : 0, [&] {
        if (h->tf) // data_updating.rs: PresolveIsActive / ChordalDecompositionIsActive
            return fail(CHIP_ERR_UPDATE_NOT_ALLOWED, fn + ": presolve or chordal decomposition is active (nothing changed)");
        return 0;
    });
}

CHIP_UPDATE_ENTRIES(chip_problem_update_, chip_solver)

// ---------------------------------------------------------------------------------------------------------------
// Re-equilibration: new full data on the fixed patterns, equilibrated from d = e = 1, c = 1 by
// create's own ProblemData::equilibrate on the handle's stream, then every copy and derived value of the audit
// refreshed by the data updates' passes.  The symbolic side (chip_kkt, chip_kktsystem) is left alone.  One host
// synchronisation, equilibrate's own, in which c, the norms and max |P_ii| come back.
// ---------------------------------------------------------------------------------------------------------------
int chip_solver::reequilibrate_gate(const char *fn) {
    if (tf) // the rule of the updates (data_updating.rs: PresolveIsActive / ChordalDecompositionIsActive)
        return fail(CHIP_ERR_UPDATE_NOT_ALLOWED,
                    std::string(fn) + ": presolve or chordal decomposition is active (nothing changed)");
    req_launches = req_syncs = 0;
    return CHIP_OK;
}

int chip_solver::reequilibrate(const double *P_dev, const double *q_dev, const double *A_dev, const double *b_dev) {
    int rc;
    if ((rc = update_work())) return rc;
    if (!eq_partials && (rc = mem.alloc(&eq_partials, (size_t)dev::eq_cost_partials()))) return rc;
    const double te = now_s();
    hipStream_t s = stream;
    const dev::EqMats &M = pd.M;
    // the raw values, b capped, and the norms create takes from them (before the loop scales them in place)
    pd.reload(s, P_dev, q_dev, A_dev, b_dev, nullptr, nullptr);
    dev::re_absmax(s, pd.q, pd.n, npart, nout);
    dev::re_absmax(s, pd.b, pd.m, npart, nout + 1);
    CHIP_HIP(hipGetLastError());
    req_launches += 8;
    double hn[3] = {0, 0, 0};
    auto ruiz_step = [&](unsigned long long *bits, double *cstate) {
        dev::eq_ruiz_step(s, M, pd.q, pd.b, pd.d, pd.e, pd.n, pd.m, bits, eq_partials, cstate,
                          st.equilibrate_min_scaling, st.equilibrate_max_scaling);
        req_launches += 2; // (with the clear of bits)
    };
    rc = pd.equilibrate(s, st, cones, 1, dev::eq_bits_words(pd.n, pd.m), ruiz_step, &c, [&](const double *) -> int {
        // the copies the loop reads (4.11's audit), from the equilibrated arrays in place
        int rc1;
        if ((rc1 = kkt_update_values_dev(kkt, UPD_P, M.Px, nullptr, M.nnzP)) ||
            (rc1 = kkt_update_values_dev(kkt, UPD_A, M.Ax, nullptr, M.nnzA)) ||
            (rc1 = kktsystem_update_data_dev(sys, M.Px, M.Ax, pd.q, pd.b)))
            return rc1;
        dev::pu_norms(s, 4, nullptr, nullptr, 0, nullptr, nullptr, 0, M.Prow, M.Pcol, M.Px, M.nnzP, npart, nout);
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipMemcpyAsync(hn, nout, sizeof(hn), hipMemcpyDeviceToHost, s));
        req_launches += 2 + 5 + 2 + 1;
        return (int)CHIP_OK;
    });
    req_launches += 7; // d, e, cstate, the rectification, the inversion (or dinv, einv), c
    req_syncs++;
    if (rc) return rc;
    normq = hn[0];
    normb = hn[1];
    kkt_set_static_diag_max(kkt, hn[2]);
    equilibration_time = now_s() - te;
    return CHIP_OK;
}

int32_t chip_reequilibrate_problem(chip_solver *h, const double *Pnzval, const double *q, const double *Anzval,
                                   const double *b) {
    return reequilibrate_entry("chip_reequilibrate_problem", h, Pnzval, q, Anzval, b, true);
}
int32_t chip_reequilibrate_problem_dev(chip_solver *h, const double *Pnzval_dev, const double *q_dev,
                                       const double *Anzval_dev, const double *b_dev) {
    return reequilibrate_entry("chip_reequilibrate_problem_dev", h, Pnzval_dev, q_dev, Anzval_dev, b_dev, false);
}

// DefaultSolver::update_settings (core/solver.rs:207) with validate_as_update (settings.rs:307): the equilibration
// fields as in the reference, and every field chip_kkt keeps its own copy of (all of linsys, with the two line-search
// fields create copies into it)
int chip::validate_settings_update(const chip_solver_settings &o, chip_solver_settings &nw, const char *fn) {
    create_settings(&nw, nw); // (linsys' copies of the two line-search fields)
    const chip_settings &a = nw.linsys, &l = o.linsys;
#define IMMUTABLE(cond, name) \
    if (cond) return fail(CHIP_ERR_ARG, std::string(fn) + ": " name " cannot change after setup")
    IMMUTABLE(nw.equilibrate_enable != o.equilibrate_enable, "equilibrate_enable");
    IMMUTABLE(nw.equilibrate_max_iter != o.equilibrate_max_iter, "equilibrate_max_iter");
    IMMUTABLE(std::memcmp(&nw.equilibrate_min_scaling, &o.equilibrate_min_scaling, 8), "equilibrate_min_scaling");
    IMMUTABLE(std::memcmp(&nw.equilibrate_max_scaling, &o.equilibrate_max_scaling, 8), "equilibrate_max_scaling");
    IMMUTABLE(std::memcmp(&nw.linesearch_backtrack_step, &o.linesearch_backtrack_step, 8), "linesearch_backtrack_step");
    IMMUTABLE(std::memcmp(&nw.min_terminate_step_length, &o.min_terminate_step_length, 8), "min_terminate_step_length");
    IMMUTABLE(nw.presolve_enable != o.presolve_enable, "presolve_enable"); // settings.rs:317-325
    IMMUTABLE(nw.chordal_decomposition_enable != o.chordal_decomposition_enable, "chordal_decomposition_enable");
    IMMUTABLE(nw.chordal_decomposition_merge_method != o.chordal_decomposition_merge_method,
              "chordal_decomposition_merge_method");
    IMMUTABLE(nw.chordal_decomposition_compact != o.chordal_decomposition_compact, "chordal_decomposition_compact");
    IMMUTABLE(nw.chordal_decomposition_complete_dual != o.chordal_decomposition_complete_dual,
              "chordal_decomposition_complete_dual");
#define IMMUTABLE_LIN(f) IMMUTABLE(std::memcmp(&a.f, &l.f, sizeof(a.f)), "linsys." #f)
    IMMUTABLE_LIN(static_regularization_enable);
    IMMUTABLE_LIN(static_regularization_constant);
    IMMUTABLE_LIN(static_regularization_proportional);
    IMMUTABLE_LIN(dynamic_regularization_enable);
    IMMUTABLE_LIN(dynamic_regularization_eps);
    IMMUTABLE_LIN(dynamic_regularization_delta);
    IMMUTABLE_LIN(iterative_refinement_enable);
    IMMUTABLE_LIN(iterative_refinement_reltol);
    IMMUTABLE_LIN(iterative_refinement_abstol);
    IMMUTABLE_LIN(iterative_refinement_max_iter);
    IMMUTABLE_LIN(iterative_refinement_stop_ratio);
    IMMUTABLE_LIN(device);
    IMMUTABLE_LIN(amd_dense_scale);
    IMMUTABLE_LIN(use_graph);
#undef IMMUTABLE_LIN
#undef IMMUTABLE
    return CHIP_OK;
}

int32_t chip_problem_update_settings(chip_solver *h, const chip_solver_settings *settings) {
    if (!h || !settings) return fail(CHIP_ERR_ARG, "chip_problem_update_settings: bad argument");
    chip_solver_settings nw = *settings;
    if (int rc = validate_settings_update(h->st, nw, "chip_problem_update_settings")) return rc;
    h->st = nw;
    return CHIP_OK;
}

int32_t chip_problem_update_allowed(const chip_solver *h, int32_t *allowed) {
    if (!h || !allowed) return fail(CHIP_ERR_ARG, "chip_problem_update_allowed: bad argument");
    *allowed = h->tf ? 0 : 1; // an enabled transform that changed nothing keeps updates allowed (the reference's Option)
    return CHIP_OK;
}

int32_t chip_problem_get_scaled(chip_solver *h, double *Px, double *Ax, double *q, double *b) {
    if (!h) return fail(CHIP_ERR_ARG, "chip_problem_get_scaled: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    return h->pd.get_scaled(h->stream, Px, Ax, q, b);
}

int32_t chip_transform_get_info(const chip_solver *h, chip_transform_info *out) {
    if (!h || !out) return fail(CHIP_ERR_ARG, "chip_transform_get_info: bad argument");
    std::memset(out, 0, sizeof(*out));
    const ProblemTransform *t = h->tf.get();
    out->m_full = h->m_out;
    out->m_reduced = t ? t->m_reduced : h->m_out;
    out->n_internal = h->pd.n;
    out->m_internal = h->pd.m;
    out->nnzA_internal = h->pd.M.nnzA;
    out->psd_cones_decomposed = t ? (int64_t)t->patterns.size() : 0;
    out->psd_cones_added = t ? t->final_added : 0;
    out->psd_cones_added_premerge = t ? t->premerge_added : 0;
    out->largest_clique = t ? t->largest_clique : 0;
    out->transform_time = h->transform_time;
    out->completion_time = h->completion_time;
    return CHIP_OK;
}

#ifdef CHIP_TESTING
#include "../../include/clarabel_hip_testing.h"
int32_t chip_debug_solver_internal_solution(void *solver, double *x2, double *s2, double *z2) {
    chip_solver *h = (chip_solver *)solver;
    if (!h) return fail(CHIP_ERR_ARG, "chip_debug_solver_internal_solution: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    const ProblemData &pd = h->pd;
    const int n = pd.n, m = pd.m;
    const bool inf = ipm_is_infeasible(h->info.status);
    const chip_vars &v = h->vars;
    const double scaleinv = inf ? 1.0 / v.kappa : 1.0 / v.tau, cinv = 1.0 / h->c;
    DevPool tmp;
    double *xo, *so, *zo;
    int rc;
    if ((rc = tmp.alloc(&xo, (size_t)n)) || (rc = tmp.alloc(&so, (size_t)m)) || (rc = tmp.alloc(&zo, (size_t)m)))
        return rc;
    dev::unscale(h->stream, xo, v.x, pd.d, scaleinv, n, zo, v.z, pd.e, scaleinv * cinv, so, v.s, pd.einv, scaleinv, m);
    CHIP_HIP(hipGetLastError());
    CHIP_HIP(hipStreamSynchronize(h->stream));
    if (x2 && n) CHIP_HIP(hipMemcpy(x2, xo, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (s2 && m) CHIP_HIP(hipMemcpy(s2, so, (size_t)m * 8, hipMemcpyDeviceToHost));
    if (z2 && m) CHIP_HIP(hipMemcpy(z2, zo, (size_t)m * 8, hipMemcpyDeviceToHost));
    return CHIP_OK;
}

namespace {
// the flat form of an IpmInfo the two hooks below exchange (clarabel_hip_testing.h): these 15 scalars, then out5
constexpr double IpmInfo::*IPM_FIELD[15] = {
    &IpmInfo::cost_primal,      &IpmInfo::cost_dual,      &IpmInfo::res_primal,      &IpmInfo::res_dual,
    &IpmInfo::res_primal_inf,   &IpmInfo::res_dual_inf,   &IpmInfo::gap_abs,         &IpmInfo::gap_rel,
    &IpmInfo::ktratio,          &IpmInfo::prev_cost_primal, &IpmInfo::prev_cost_dual, &IpmInfo::prev_res_primal,
    &IpmInfo::prev_res_dual,    &IpmInfo::prev_gap_abs,   &IpmInfo::prev_gap_rel};
IpmInfo ipm_from_flat(const double *info) {
    IpmInfo I;
    for (int k = 0; k < 15; k++) I.*IPM_FIELD[k] = info[k];
    std::copy(info + 15, info + 20, I.out5);
    return I;
}
} // namespace
int32_t chip_debug_ipm_termination(const void *solver_settings, const double *info, int32_t iter, int32_t iterations,
                                   double solve_time, int32_t almost_post_process) {
    if (!solver_settings || !info) return fail(CHIP_ERR_ARG, "chip_debug_ipm_termination: bad argument");
    const chip_solver_settings &st = *(const chip_solver_settings *)solver_settings;
    IpmInfo I = ipm_from_flat(info);
    I.status = (int)info[20];
    I.iterations = iterations;
    double unused[4];
    if (almost_post_process) ipm_post_process(I, st, 1.0, 1.0, 1.0, &unused[0], &unused[1], &unused[2], &unused[3]);
    else ipm_check_termination(I, st, iter, solve_time);
    return I.status;
}
int32_t chip_debug_ipm_info_update(double *info, const double *sq, double tau, double kappa, double c, double normq,
                                   double normb) {
    if (!info || !sq) return fail(CHIP_ERR_ARG, "chip_debug_ipm_info_update: bad argument");
    IpmInfo I = ipm_from_flat(info);
    ipm_info_update(I, sq, tau, kappa, c, normq, normb);
    for (int k = 0; k < 9; k++) info[k] = I.*IPM_FIELD[k];
    return CHIP_OK;
}
int32_t chip_debug_solver_scaled_state(void *solver, double *x, double *s, double *z, double *tau_kappa, double *dinv,
                                       double *einv, double *info21) {
    chip_solver *h = (chip_solver *)solver;
    if (!h) return fail(CHIP_ERR_ARG, "chip_debug_solver_scaled_state: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    CHIP_HIP(hipStreamSynchronize(h->stream));
    const ProblemData &pd = h->pd;
    const size_t nb = (size_t)pd.n * 8, mb = (size_t)pd.m * 8;
    const chip_vars &v = h->vars;
    if (x && nb) CHIP_HIP(hipMemcpy(x, v.x, nb, hipMemcpyDeviceToHost));
    if (s && mb) CHIP_HIP(hipMemcpy(s, v.s, mb, hipMemcpyDeviceToHost));
    if (z && mb) CHIP_HIP(hipMemcpy(z, v.z, mb, hipMemcpyDeviceToHost));
    if (dinv && nb) CHIP_HIP(hipMemcpy(dinv, pd.dinv, nb, hipMemcpyDeviceToHost));
    if (einv && mb) CHIP_HIP(hipMemcpy(einv, pd.einv, mb, hipMemcpyDeviceToHost));
    if (tau_kappa) {
        tau_kappa[0] = v.tau;
        tau_kappa[1] = v.kappa;
    }
    if (info21) {
        for (int k = 0; k < 15; k++) info21[k] = h->info.*IPM_FIELD[k];
        std::copy(h->info.out5, h->info.out5 + 5, info21 + 15);
        info21[20] = (double)h->info.status;
    }
    return CHIP_OK;
}
#endif
