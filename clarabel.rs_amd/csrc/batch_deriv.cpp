// batch_deriv.cpp -- the derivative passes of the batched solver (chip_bgrad_*, chip_bjvp_*, chip_bjac_*, chip_bvjp_*)
// on the handle of batch_handle.hpp
#include "batch_adjoint.hpp"
#include "batch_cotangent.hpp"
#include "batch_handle.hpp"
#include "batch_jacobian.hpp"
#include "batch_tangent.hpp"

// ---------------------------------------------------------------------------------------------------------------
// The derivatives of the members' solutions: the gradients (chip_bgrad_*) and their exact transpose,
// the forward-mode derivatives (chip_bjvp_*).  Either is ONE refined KKT solve at the final iterates
// with K = [P A'; A -H], H = diag(s / z) on Nonnegative rows and 0 on Zero rows: the matrix chip_kkt factors after a
// scaling update with (s, z) of the internal iterate (tau cancels), in the equilibrated space of the stack
// (x = D x^, z = E z^ / c_k, s = E^-1 s^; P^ = c_k D P D, q^ = c_k D q, A^ = E A D, b^ = E b).  The steps below are
// shared; a pass itself is what differs mathematically: its right-hand side, its product with A' or A, its outputs.
// A derivative exists for the members that ended Solved and own only Zero / Nonnegative cones; every other member
// takes the cones' unit vector for (s, z), as a member that ended NumericalError does in the loop, and a zero
// right-hand side: its block of K stays well posed and its part of the solution is 0.
// Enqueues are counted as batch.cpp counts them everywhere (one per kernel, copy or call into the KKT layer, whatever
// that call launches itself); the synchronisations are chip_kkt_update's, chip_kkt_solve_dev's and one at the end.
// A pass overwrites work vectors and its own results only; chip_batch_solve starts from default_start, which rescales
// and refactors, so a following solve does not see it.
// ---------------------------------------------------------------------------------------------------------------
namespace {
typedef DerivPass chip_batch::*PassOf;

int deriv_alloc(chip_batch *h, DerivPass &p, std::initializer_list<size_t> in_len,
                std::initializer_list<size_t> out_len) {
    if (p.valid) return CHIP_OK;
    p.nin = (int)in_len.size();
    p.nout = (int)out_len.size();
    std::copy(in_len.begin(), in_len.end(), p.in_len);
    std::copy(out_len.begin(), out_len.end(), p.out_len);
    p.hvalid.assign((size_t)h->nprob, 0);
    int rc = CHIP_OK;
    for (int i = 0; i < p.nout && !rc; i++) rc = h->mem.alloc(&p.out[i], p.out_len[i]);
    for (int i = 0; i < p.nin && !rc; i++) rc = h->mem.alloc(&p.in[i], p.in_len[i]);
    return rc ? rc : h->mem.alloc(&p.valid, (size_t)h->nprob); // (last: it marks the allocation as done)
}

// the start of a pass's entry point `fn`: refused without a finished solve on the current data
int deriv_begin(chip_batch *h, const char *fn, PassOf which, int (chip_batch::*work)()) {
    if (!h) return fail(CHIP_ERR_ARG, std::string(fn) + ": bad argument");
    if (!h->solve_current)
        return fail(CHIP_ERR_ARG, std::string(fn) + ": needs a finished chip_batch_solve on the current data");
    CHIP_HIP(hipSetDevice(h->pd.device));
    (h->*which).syncs = (h->*which).launches = 0;
    return (h->*work)();
}

// the host form: a NULL input stays NULL, a given one becomes its staging buffer (one copy, none for an empty input)
int deriv_stage(chip_batch *h, DerivPass &p, const double **in) {
    for (int i = 0; i < p.nin; i++) {
        const double *src = in[i];
        if (!src) continue;
        in[i] = p.in[i];
        if (!p.in_len[i]) continue;
        CHIP_HIP(hipMemcpyAsync(p.in[i], src, p.in_len[i] * sizeof(double), hipMemcpyHostToDevice, h->stream));
        p.launches++;
    }
    return CHIP_OK;
}

int deriv_valid(chip_batch *h, DerivPass &p) {
    for (int k = 0; k < h->nprob; k++)
        p.hvalid[k] = h->info[k].status == CHIP_SOLVER_SOLVED && !h->has_soc[k] && !h->has_psd[k];
    CHIP_HIP(hipMemcpyAsync(p.valid, p.hvalid.data(), (size_t)h->nprob * sizeof(int), hipMemcpyHostToDevice, h->stream));
    p.launches++;
    return CHIP_OK;
}

// K at the final iterates: the scaling update with the (s, z) the right-hand side pass left in (ds, dz), the refactor
int deriv_factor(chip_batch *h, DerivPass &p) {
    int rc;
    h->kkt_final = false; // (a refactor that fails leaves nothing to reuse)
    if (h->psd.ncones) { // a member with a PSD cone is never valid: the pass wrote 0 on its PSD rows, the unit vector's
        dev::bp_diag_unit(h->stream, h->psd, h->ds, h->dz, nullptr); // diagonal is 1
        p.launches++;
    }
    if ((rc = chip_kkt_update_scaling_dev(h->kkt, h->ds, h->dz, 1.0, 0)) < 0) return rc;
    rc = chip_kkt_update(h->kkt, nullptr);
    p.syncs++;
    p.launches += 2;
    p.refactors++;
    if (rc < 0) return rc;
    if (rc != 1)
        return fail(CHIP_ERR_ZERO_PIVOT, std::string(p.name) + ": the factorisation at the final iterate failed");
    h->kkt_final = true; // (an apply after this solves with this factorisation)
    return CHIP_OK;
}

// [x1; z1] = K^-1 [workx; workz], refined
int deriv_solve(chip_batch *h, DerivPass &p) {
    int rc;
    if ((rc = chip_kkt_setrhs_dev(h->kkt, h->workx, h->workz))) return rc;
    rc = chip_kkt_solve_dev(h->kkt, h->x1, h->z1);
    p.syncs++;
    p.launches++;
    if (rc < 0) return rc;
    if (rc != 1) return fail(CHIP_ERR_ZERO_PIVOT, std::string(p.name) + ": the solve at the final iterate failed");
    return CHIP_OK;
}

int deriv_end(chip_batch *h, DerivPass &p) {
    CHIP_HIP(hipGetLastError());
    CHIP_HIP(hipStreamSynchronize(h->stream));
    p.syncs++;
    p.done = true;
    return CHIP_OK;
}

// the read-outs of entry point `fn`: refused without a pass since the last solve
int deriv_result(chip_batch *h, const char *fn, PassOf which) {
    if (!h) return fail(CHIP_ERR_ARG, std::string(fn) + ": bad argument");
    if (!(h->*which).done)
        return fail(CHIP_ERR_ARG, std::string(fn) + ": no " + (h->*which).name + " since the last solve");
    return CHIP_OK;
}

int deriv_get(chip_batch *h, const char *fn, PassOf which, std::initializer_list<double *> dst, int32_t *valid) {
    if (int rc = deriv_result(h, fn, which)) return rc;
    const DerivPass &p = h->*which;
    CHIP_HIP(hipSetDevice(h->pd.device));
    for (int i = 0; i < p.nout; i++)
        if (dst.begin()[i] && p.out_len[i])
            CHIP_HIP(hipMemcpy(dst.begin()[i], p.out[i], p.out_len[i] * 8, hipMemcpyDeviceToHost));
    if (valid) std::copy(p.hvalid.begin(), p.hvalid.end(), valid);
    return CHIP_OK;
}

int deriv_get_dev(chip_batch *h, const char *fn, PassOf which, std::initializer_list<double **> dst,
                  int32_t **valid_dev) {
    if (int rc = deriv_result(h, fn, which)) return rc;
    const DerivPass &p = h->*which;
    for (int i = 0; i < p.nout; i++)
        if (dst.begin()[i]) *dst.begin()[i] = p.out[i];
    if (valid_dev) *valid_dev = p.valid;
    return CHIP_OK;
}
} // namespace

// ---- the gradients.  With the incoming gradients (gx, gz, gs) of a member's unscaled (x, z, s), its adjoint is
//     [vx; vz] = K^-1 [gx - A' gs; gz].
// In the equilibrated space the incoming gradients are D gx, E gz / c_k and E^-1 gs; the solution multiplied back,
// ux = c_k D vx^ and uz = E vz^, is the adjoint pair of the unscaled problem, so the four gradients are the unscaled
// formulas on the unscaled solution the solve has already written (xo, zo).  A backward always refactors
int chip_batch::backward_work() {
    const size_t n = (size_t)pd.n, m = (size_t)pd.m;
    return deriv_alloc(this, grad, {n, m, m}, {n, m, (size_t)pd.M.nnzP, (size_t)pd.M.nnzA});
}

int chip_batch::backward(const double *gx, const double *gz, const double *gs) {
    int rc;
    grad.done = false; // (a backward that fails part-way leaves no result behind)
    if ((rc = deriv_valid(this, grad))) return rc;
    dev::ba_rhs(stream, plan, dev::BaRhs{grad.valid, gx, gz, gs, pd.d, pd.e, dc, vs, vz, wn, conicw, workz, ds, dz});
    grad.launches++;
    if ((rc = kktsystem_spmv(sys, 2, workx, wn, -1.0, conicw))) return rc; // D gx - A^' (gs / e)
    grad.launches++;
    if ((rc = deriv_factor(this, grad)) || (rc = deriv_solve(this, grad))) return rc;
    double *const *o = grad.out; // dq, db, dP, dA
    const dev::BaGrad g{grad.valid, x1, z1, gs, pd.d, pd.e, dc, xo, zo, x2, z2, o[0], o[1], o[2], o[3]};
    dev::ba_grad_vectors(stream, plan, g);
    dev::ba_grad_matrices(stream, plan, pd.M, g);
    grad.launches += 2;
    return deriv_end(this, grad);
}

int32_t chip_bgrad_backward(chip_batch *h, const double *gx, const double *gz, const double *gs) {
    const double *in[3] = {gx, gz, gs};
    int rc = deriv_begin(h, "chip_bgrad_backward", &chip_batch::grad, &chip_batch::backward_work);
    if (rc || (rc = deriv_stage(h, h->grad, in))) return rc;
    return h->backward(in[0], in[1], in[2]);
}

int32_t chip_bgrad_backward_dev(chip_batch *h, const double *gx_dev, const double *gz_dev, const double *gs_dev) {
    const int rc = deriv_begin(h, "chip_bgrad_backward_dev", &chip_batch::grad, &chip_batch::backward_work);
    return rc ? rc : h->backward(gx_dev, gz_dev, gs_dev);
}

int32_t chip_bgrad_get(chip_batch *h, double *dq, double *db, double *dPx, double *dAx, int32_t *valid) {
    return deriv_get(h, "chip_bgrad_get", &chip_batch::grad, {dq, db, dPx, dAx}, valid);
}

int32_t chip_bgrad_get_dev(chip_batch *h, double **dq_dev, double **db_dev, double **dPx_dev, double **dAx_dev,
                           int32_t **valid_dev) {
    return deriv_get_dev(h, "chip_bgrad_get_dev", &chip_batch::grad, {dq_dev, db_dev, dPx_dev, dAx_dev}, valid_dev);
}

// ---- the tangents.  Along a direction (dq, db, dP, dA) in a member's data its solution moves by
//     rx = -(dq + dP_sym x + dA' z),  rz = db - dA x,  [dx; dz] = K^-1 [rx; rz],  ds = rz - A dx (Nonnegative rows).
// In the equilibrated space the system is K^ [D^-1 dx; c_k E^-1 dz] = [c_k D rx; E rz] with rx, rz formed from the
// unscaled solution (xo, zo), so dx = D vx^, dz = E vz^ / c_k and ds = E^-1 (E rz - A^ vx^): the transposes of
// backward's scalings.  An apply refactors only when K is not factored at the final iterates already (kkt_final: set
// by a backward or an apply, cleared by an update and at the start of a solve)
int chip_batch::jvp_work() {
    const size_t n = (size_t)pd.n, m = (size_t)pd.m;
    return deriv_alloc(this, tan, {n, m, (size_t)pd.M.nnzP, (size_t)pd.M.nnzA}, {n, m, m});
}

int chip_batch::jvp_apply(const double *dq, const double *db, const double *dP, const double *dA) {
    int rc;
    tan.done = false; // (an apply that fails part-way leaves no result behind)
    dev::SpPattern Psym, Arow, Acol;
    if ((rc = kktsystem_pattern(sys, 0, &Psym)) || (rc = kktsystem_pattern(sys, 1, &Arow)) ||
        (rc = kktsystem_pattern(sys, 2, &Acol)) || (rc = deriv_valid(this, tan)))
        return rc;
    const bool refactor = !kkt_final;
    dev::bt_rhs(stream, plan, Psym, Acol, Arow,
                dev::BtRhs{tan.valid, xo, zo, dq, db, dP, dA, pd.d, pd.e, dc, workx, workz, vs, vz,
                           refactor ? ds : nullptr, refactor ? dz : nullptr});
    tan.launches++;
    if ((refactor && (rc = deriv_factor(this, tan))) || (rc = deriv_solve(this, tan))) return rc;
    if ((rc = kktsystem_spmv(sys, 1, conicw, workz, -1.0, x1))) return rc; // E rz - A^ vx^
    double *const *o = tan.out; // dx, dz, ds
    dev::bt_out(stream, plan, dev::BtOut{tan.valid, x1, z1, conicw, pd.d, pd.e, pd.einv, dc, o[0], o[1], o[2]});
    tan.launches += 2;
    return deriv_end(this, tan);
}

int32_t chip_bjvp_apply(chip_batch *h, const double *dq, const double *db, const double *dPx, const double *dAx) {
    const double *in[4] = {dq, db, dPx, dAx};
    int rc = deriv_begin(h, "chip_bjvp_apply", &chip_batch::tan, &chip_batch::jvp_work);
    if (rc || (rc = deriv_stage(h, h->tan, in))) return rc;
    return h->jvp_apply(in[0], in[1], in[2], in[3]);
}

int32_t chip_bjvp_apply_dev(chip_batch *h, const double *dq_dev, const double *db_dev, const double *dPx_dev,
                            const double *dAx_dev) {
    const int rc = deriv_begin(h, "chip_bjvp_apply_dev", &chip_batch::tan, &chip_batch::jvp_work);
    return rc ? rc : h->jvp_apply(dq_dev, db_dev, dPx_dev, dAx_dev);
}

int32_t chip_bjvp_get(chip_batch *h, double *dx, double *dz, double *ds, int32_t *valid) {
    return deriv_get(h, "chip_bjvp_get", &chip_batch::tan, {dx, dz, ds}, valid);
}

int32_t chip_bjvp_get_dev(chip_batch *h, double **dx_dev, double **dz_dev, double **ds_dev, int32_t **valid_dev) {
    return deriv_get_dev(h, "chip_bjvp_get_dev", &chip_batch::tan, {dx_dev, dz_dev, ds_dev}, valid_dev);
}

// ---- blocks of tangents (chip_bjac_*): up to CHIP_BJAC_MAX_DIR applies with ONE synchronisation.
// The mathematics of every direction is the apply's above.  What differs is the host sequence: one right-hand side
// launch for all directions, every direction's refined solve ENQUEUED (the refinement decisions are taken on the
// device), the products and one output launch behind them, and chip_kkt_collect as the one synchronisation, which
// brings all verdicts.  A solve that is pending borrows its right-hand side, so every direction owns its right-hand
// side, solution and product in jac_work: per direction [rx n' | rz m' | vx n' | vz m' | w m'] with n', m' the
// lengths rounded up to even (16-byte aligned slices)
namespace {
struct JacWork {
    size_t stride;
    double *rx, *rz, *vx, *vz, *w; // of direction 0; direction t: + t * stride
    explicit JacWork(const chip_batch *h) {
        const size_t np = ((size_t)h->pd.n + 1) & ~(size_t)1, mp = ((size_t)h->pd.m + 1) & ~(size_t)1;
        stride = 2 * np + 3 * mp;
        rx = h->jac_work;
        rz = rx + np;
        vx = rz + mp;
        vz = vx + np;
        w = vz + mp;
    }
};

// the two ends every block of pending solves shares (the tangents here, the cotangents below).
// block_solves: the refined solve of every direction t, ENQUEUED: [vx; vz] + t * stride = K^-1 ([rx; rz] + t * stride).
// (A system without the fused solve launch takes its refinement decisions on the host: its enqueue is a synchronous
// solve.)  A failure collects before it returns: no solve stays pending behind a failed call
int block_solves(chip_batch *h, DerivPass &p, int ndir, size_t stride, const double *rx, const double *rz, double *vx,
                 double *vz) {
    double model[8] = {};
    int rc;
    if ((rc = chip_kkt_work_model(h->kkt, model))) return rc;
    for (int t = 0; t < ndir && !rc; t++) {
        const size_t o = (size_t)t * stride;
        if (!(rc = chip_kkt_setrhs_dev(h->kkt, rx + o, rz + o))) rc = chip_kkt_solve_dev_enqueue(h->kkt, vx + o, vz + o);
        if (!rc) p.launches++, p.syncs += model[7] > 0.0 ? 0 : 1;
    }
    if (rc) (void)chip_kkt_collect(h->kkt, nullptr, nullptr, nullptr);
    return rc;
}

// block_finish: `outputs` enqueues what consumes the solutions; chip_kkt_collect behind it is the one synchronisation
// and brings all verdicts.  A solve that was repeated at the collect (verdict 2) means that what consumed its solution
// before that read garbage: the outputs are issued once more and the stream synchronised a second time
template <class Outputs> int block_finish(chip_batch *h, DerivPass &p, int ndir, long &repeats, Outputs outputs) {
    int rc = outputs();
    int32_t nsolves = 0, verdict[16] = {};
    const int rcc = chip_kkt_collect(h->kkt, nullptr, &nsolves, verdict);
    p.syncs++;
    if (rc || (rc = rcc) < 0) return rc;
    bool repeated = false;
    for (int t = 0; t < ndir; t++) {
        if (t >= nsolves || verdict[t] == 0)
            return fail(CHIP_ERR_ZERO_PIVOT, std::string(p.name) + ": a solve at the final iterate failed");
        repeated = repeated || verdict[t] == 2;
    }
    if (repeated) {
        repeats++;
        if ((rc = outputs())) return rc;
        CHIP_HIP(hipStreamSynchronize(h->stream));
        p.syncs++;
    }
    CHIP_HIP(hipGetLastError());
    p.done = true;
    return CHIP_OK;
}

int jac_begin(chip_batch *h, const char *fn, int32_t ndir) {
    if (!h) return fail(CHIP_ERR_ARG, std::string(fn) + ": bad argument");
    if (ndir < 1 || ndir > CHIP_BJAC_MAX_DIR)
        return fail(CHIP_ERR_ARG, std::string(fn) + ": a block holds 1 to CHIP_BJAC_MAX_DIR directions");
    return deriv_begin(h, fn, &chip_batch::jac, &chip_batch::jac_alloc);
}
} // namespace

int chip_batch::jac_alloc() {
    if (jac.valid) return CHIP_OK;
    const size_t n = (size_t)pd.n, m = (size_t)pd.m, K = CHIP_BJAC_MAX_DIR;
    int rc;
    if ((rc = mem.alloc(&jac_work, K * JacWork(this).stride))) return rc;
    return deriv_alloc(this, jac, {}, {K * n, K * m, K * m});
}

int chip_batch::jac_block(int ndir, int piece, long long first, const double *dq, const double *db, const double *dP,
                          const double *dA) {
    int rc;
    jac.done = false; // (a block that fails part-way leaves no result behind)
    jac_calls++;
    const size_t lens[3] = {(size_t)pd.n, (size_t)pd.m, (size_t)pd.m};
    for (int i = 0; i < 3; i++) jac.out_len[i] = (size_t)ndir * lens[i];
    const JacWork k(this);
    if ((rc = deriv_valid(this, jac))) return rc;
    const bool refactor = !kkt_final;
    double *ss = refactor ? ds : nullptr, *zs = refactor ? dz : nullptr;
    if (piece < 0) {
        dev::SpPattern Psym, Arow, Acol;
        if ((rc = kktsystem_pattern(sys, 0, &Psym)) || (rc = kktsystem_pattern(sys, 1, &Arow)) ||
            (rc = kktsystem_pattern(sys, 2, &Acol)))
            return rc;
        dev::bj_rhs(stream, plan, Psym, Acol, Arow,
                    dev::BjRhs{dev::BtRhs{jac.valid, xo, zo, dq, db, dP, dA, pd.d, pd.e, dc, k.rx, k.rz, vs, vz, ss, zs},
                               ndir, (size_t)pd.n, (size_t)pd.m, (size_t)pd.M.nnzP, (size_t)pd.M.nnzA, k.stride,
                               k.stride});
    } else {
        dev::bj_units(stream, plan,
                      dev::BjUnits{jac.valid, pd.d, pd.e, dc, k.rx, k.rz, k.stride, k.stride, piece, ndir, first, vs, vz,
                                   ss, zs});
    }
    jac.launches++;
    if (refactor && (rc = deriv_factor(this, jac))) return rc;
    if ((rc = block_solves(this, jac, ndir, k.stride, k.rx, k.rz, k.vx, k.vz))) return rc;
    // E rz - A^ vx^ of every direction, then all outputs in one launch
    return block_finish(this, jac, ndir, jac_repeats, [&]() -> int {
        for (int t = 0; t < ndir; t++) {
            const size_t o = (size_t)t * k.stride;
            if (int e = kktsystem_spmv(sys, 1, k.w + o, k.rz + o, -1.0, k.vx + o)) return e;
        }
        double *const *r = jac.out; // dx, dz, ds
        dev::bj_out(stream, plan,
                    dev::BjOut{dev::BtOut{jac.valid, k.vx, k.vz, k.w, pd.d, pd.e, pd.einv, dc, r[0], r[1], r[2]}, ndir,
                               k.stride, k.stride});
        jac.launches += ndir + 1;
        return CHIP_OK;
    });
}

int32_t chip_bjac_apply(chip_batch *h, int32_t ndir, const double *dq, const double *db, const double *dPx,
                        const double *dAx) {
    const double *in[4] = {dq, db, dPx, dAx};
    int rc = jac_begin(h, "chip_bjac_apply", ndir);
    if (rc) return rc;
    DerivPass &p = h->jac;
    const size_t lens[4] = {(size_t)h->pd.n, (size_t)h->pd.m, (size_t)h->pd.M.nnzP, (size_t)h->pd.M.nnzA};
    p.nin = 4;
    for (int i = 0; i < 4; i++) { // the staging of a full block, allocated by the first host form that gives the input
        if (in[i] && !p.in[i] && (rc = h->mem.alloc(&p.in[i], (size_t)CHIP_BJAC_MAX_DIR * lens[i]))) return rc;
        p.in_len[i] = (size_t)ndir * lens[i];
    }
    if ((rc = deriv_stage(h, p, in))) return rc;
    return h->jac_block(ndir, -1, 0, in[0], in[1], in[2], in[3]);
}

int32_t chip_bjac_apply_dev(chip_batch *h, int32_t ndir, const double *dq_dev, const double *db_dev,
                            const double *dPx_dev, const double *dAx_dev) {
    const int rc = jac_begin(h, "chip_bjac_apply_dev", ndir);
    return rc ? rc : h->jac_block(ndir, -1, 0, dq_dev, db_dev, dPx_dev, dAx_dev);
}

int32_t chip_bjac_units(chip_batch *h, int32_t piece, int64_t first, int32_t ndir) {
    if (h && ((piece != 0 && piece != 1) || first < 0))
        return fail(CHIP_ERR_ARG, "chip_bjac_units: piece is 0 (q) or 1 (b), first is not negative");
    const int rc = jac_begin(h, "chip_bjac_units", ndir);
    return rc ? rc : h->jac_block(ndir, piece, (long long)first, nullptr, nullptr, nullptr, nullptr);
}

int32_t chip_bjac_get(chip_batch *h, double *dx, double *dz, double *ds, int32_t *valid) {
    return deriv_get(h, "chip_bjac_get", &chip_batch::jac, {dx, dz, ds}, valid);
}

int32_t chip_bjac_get_dev(chip_batch *h, double **dx_dev, double **dz_dev, double **ds_dev, int32_t **valid_dev) {
    return deriv_get_dev(h, "chip_bjac_get_dev", &chip_batch::jac, {dx_dev, dz_dev, ds_dev}, valid_dev);
}

// ---- blocks of cotangents (chip_bvjp_*): up to CHIP_BVJP_MAX_DIR backwards with ONE synchronisation,
// and only the pieces of the result the caller wants.  The mathematics of every cotangent is the backward's above.
// What differs is the host sequence, which is jac_block's: one right-hand side launch for all cotangents, the A'
// products only when a gs is given, the refactor only when K is not factored at the final iterates yet (a backward
// always pays it), every cotangent's refined solve enqueued, the output launches behind them, and chip_kkt_collect as
// the one synchronisation.  Every cotangent owns its slices of vjp_work: [t n' | ws m' | rx n' | rz m' | vx n' | vz m']
// with n', m' the lengths rounded up to even (16-byte aligned slices); t = D gx and ws = gs / e are the operands of
// the A' product and stay unused without a gs, where the right-hand side pass writes D gx into rx itself
namespace {
struct VjpWork {
    size_t stride;
    double *t, *ws, *rx, *rz, *vx, *vz; // of cotangent 0; cotangent u: + u * stride
    explicit VjpWork(const chip_batch *h) {
        const size_t np = ((size_t)h->pd.n + 1) & ~(size_t)1, mp = ((size_t)h->pd.m + 1) & ~(size_t)1;
        stride = 3 * np + 3 * mp;
        t = h->vjp_work;
        ws = t + np;
        rx = ws + mp;
        rz = rx + np;
        vx = rz + mp;
        vz = vx + np;
    }
};

int vjp_begin(chip_batch *h, const char *fn, int32_t ndir, int32_t want) {
    if (!h) return fail(CHIP_ERR_ARG, std::string(fn) + ": bad argument");
    if (ndir < 1 || ndir > CHIP_BVJP_MAX_DIR)
        return fail(CHIP_ERR_ARG, std::string(fn) + ": a block holds 1 to CHIP_BVJP_MAX_DIR cotangents");
    if (want < 1 || want > dev::BC_WANT_ALL)
        return fail(CHIP_ERR_ARG, std::string(fn) + ": want holds bits 0 (dq), 1 (db), 2 (dP), 3 (dA), at least one");
    // the kernels index [x space; z space] and [P; A] together in int32 (chip_batch_create refuses a larger stack)
    const int64_t lim = 1ll << 31;
    if ((int64_t)h->pd.n + (int64_t)h->pd.m >= lim || (int64_t)h->pd.M.nnzP + (int64_t)h->pd.M.nnzA >= lim)
        return fail(CHIP_ERR_DIM, std::string(fn) + ": sizes out of int32 range");
    return deriv_begin(h, fn, &chip_batch::vjp, &chip_batch::vjp_alloc);
}
} // namespace

int chip_batch::vjp_alloc() {
    if (vjp.valid) return CHIP_OK;
    int rc;
    if ((rc = mem.alloc(&vjp_work, (size_t)CHIP_BVJP_MAX_DIR * VjpWork(this).stride))) return rc;
    rc = deriv_alloc(this, vjp, {}, {});
    vjp.nout = 4; // (allocated piece by piece, by the first block that wants the piece)
    return rc;
}

int chip_batch::vjp_block(int ndir, int want, int piece, long long first, const double *gx, const double *gz,
                          const double *gs) {
    int rc;
    vjp.done = false; // (a block that fails part-way leaves no result behind)
    vjp_calls++;
    const size_t lens[4] = {(size_t)pd.n, (size_t)pd.m, (size_t)pd.M.nnzP, (size_t)pd.M.nnzA};
    for (int i = 0; i < 4; i++) {
        const bool wanted = (want >> i) & 1;
        if (wanted && !vjp.out[i] && (rc = mem.alloc(&vjp.out[i], (size_t)CHIP_BVJP_MAX_DIR * lens[i]))) return rc;
        vjp.out_len[i] = wanted ? (size_t)ndir * lens[i] : 0;
    }
    vjp_want = want;
    const VjpWork k(this);
    if ((rc = deriv_valid(this, vjp))) return rc;
    const bool refactor = !kkt_final, with_gs = piece == 2 || (piece < 0 && gs);
    double *ss = refactor ? ds : nullptr, *zs = refactor ? dz : nullptr;
    // with a gs the pass writes the operands of the A' product, without one the right-hand side itself
    double *dgx = with_gs ? k.t : k.rx, *ws = with_gs ? k.ws : nullptr;
    if (piece < 0)
        dev::bc_rhs(stream, plan,
                    dev::BcRhs{vjp.valid, gx, gz, gs, pd.d, pd.e, dc, vs, vz, dgx, ws, k.rz, k.stride, k.stride, k.stride,
                               ndir, ss, zs});
    else
        dev::bc_units(stream, plan,
                      dev::BcUnits{vjp.valid, pd.d, pd.e, dc, vs, vz, dgx, ws, k.rz, k.stride, k.stride, k.stride, piece,
                                   ndir, first, ss, zs});
    vjp.launches++;
    for (int t = 0; t < ndir && with_gs; t++) { // D gx - A^' (gs / e), as the backward forms it
        const size_t o = (size_t)t * k.stride;
        if ((rc = kktsystem_spmv(sys, 2, k.rx + o, k.t + o, -1.0, k.ws + o))) return rc;
        vjp.launches++;
    }
    if (refactor && (rc = deriv_factor(this, vjp))) return rc;
    if ((rc = block_solves(this, vjp, ndir, k.stride, k.rx, k.rz, k.vx, k.vz))) return rc;
    // the wanted gradients of all cotangents: one launch for dq / db, one for dP / dA
    double *const *r = vjp.out; // dq, db, dP, dA
    const dev::BcGrad g{vjp.valid, k.vx, k.vz, piece < 0 ? gs : nullptr, pd.d, pd.e, dc, xo, zo, k.stride, k.stride, ndir,
                        want, piece == 2 ? 1 : 0, first, r[0], r[1], r[2], r[3]};
    return block_finish(this, vjp, ndir, vjp_repeats, [&]() -> int {
        if (want & (dev::BC_WANT_Q | dev::BC_WANT_B)) dev::bc_grad_vectors(stream, plan, g), vjp.launches++;
        if (want & (dev::BC_WANT_P | dev::BC_WANT_A)) dev::bc_grad_matrices(stream, plan, pd.M, g), vjp.launches++;
        return CHIP_OK;
    });
}

int32_t chip_bvjp_apply(chip_batch *h, int32_t ndir, int32_t want, const double *gx, const double *gz,
                        const double *gs) {
    const double *in[3] = {gx, gz, gs};
    int rc = vjp_begin(h, "chip_bvjp_apply", ndir, want);
    if (rc) return rc;
    DerivPass &p = h->vjp;
    const size_t lens[3] = {(size_t)h->pd.n, (size_t)h->pd.m, (size_t)h->pd.m};
    p.nin = 3;
    for (int i = 0; i < 3; i++) { // the staging of a full block, allocated by the first host form that gives the input
        if (in[i] && !p.in[i] && (rc = h->mem.alloc(&p.in[i], (size_t)CHIP_BVJP_MAX_DIR * lens[i]))) return rc;
        p.in_len[i] = (size_t)ndir * lens[i];
    }
    if ((rc = deriv_stage(h, p, in))) return rc;
    return h->vjp_block(ndir, want, -1, 0, in[0], in[1], in[2]);
}

int32_t chip_bvjp_apply_dev(chip_batch *h, int32_t ndir, int32_t want, const double *gx_dev, const double *gz_dev,
                            const double *gs_dev) {
    const int rc = vjp_begin(h, "chip_bvjp_apply_dev", ndir, want);
    return rc ? rc : h->vjp_block(ndir, want, -1, 0, gx_dev, gz_dev, gs_dev);
}

int32_t chip_bvjp_units(chip_batch *h, int32_t piece, int64_t first, int32_t ndir, int32_t want) {
    if (h && (piece < 0 || piece > 2 || first < 0))
        return fail(CHIP_ERR_ARG, "chip_bvjp_units: piece is 0 (x), 1 (z) or 2 (s), first is not negative");
    const int rc = vjp_begin(h, "chip_bvjp_units", ndir, want);
    return rc ? rc : h->vjp_block(ndir, want, piece, (long long)first, nullptr, nullptr, nullptr);
}

// (out_len of a piece the last block did not want is 0: nothing is written through its pointer)
int32_t chip_bvjp_get(chip_batch *h, double *dq, double *db, double *dPx, double *dAx, int32_t *valid) {
    return deriv_get(h, "chip_bvjp_get", &chip_batch::vjp, {dq, db, dPx, dAx}, valid);
}

int32_t chip_bvjp_get_dev(chip_batch *h, double **dq_dev, double **db_dev, double **dPx_dev, double **dAx_dev,
                          int32_t **valid_dev) {
    if (int rc = deriv_result(h, "chip_bvjp_get_dev", &chip_batch::vjp)) return rc;
    double **dst[4] = {dq_dev, db_dev, dPx_dev, dAx_dev};
    for (int i = 0; i < 4; i++)
        if (dst[i]) *dst[i] = ((h->vjp_want >> i) & 1) ? h->vjp.out[i] : nullptr;
    if (valid_dev) *valid_dev = h->vjp.valid;
    return CHIP_OK;
}
