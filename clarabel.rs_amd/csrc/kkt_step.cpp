// kkt_step.cpp -- everything an interior-point iteration calls on an L2 handle but the cone passes (kkt_cones.cpp): the
// KKT update, setrhs, the solves with their refinement, the fused launches and the collect.  One translation unit, so
// that no call on the per-step path crosses an object file.
#include <cstdio>

#include "kkt_handle.hpp"
#include "problem_update.hpp"

using namespace chip;

namespace {

// ---- the debug stamps of the persistent launches (CHIP_IR_DEBUG): the device buffers of the fused solve and the ONE
// writer of a stamp file -- int32 count, then count x 32 int64 (tools/ir_skew.py reads it)
struct IrStamps {
    long long *wg01 = nullptr; // CHIP_IR_DEBUG >= 1: 64 phase stamps of each of the first workgroups (256 words)
    long long *all = nullptr;  // CHIP_IR_DEBUG >= 2: 32 words of EVERY workgroup
    size_t all_len = 0;
    // the file CHIP_IR_DEBUG_FILE (default /tmp/chip_ir_stamps.bin) + suffix
    static std::string path(const char *suffix) {
        const std::string &p = switches().ir_debug_file;
        return (p.empty() ? std::string("/tmp/chip_ir_stamps.bin") : p) + suffix;
    }
    // waits for the stream, then writes `count` x 32 stamps of the device buffer
    static void write_file(const std::string &path, int count, const long long *stamps_dev, hipStream_t s) {
        (void)hipStreamSynchronize(s);
        std::vector<long long> t((size_t)count * 32);
        (void)hipMemcpy(t.data(), stamps_dev, t.size() * sizeof(long long), hipMemcpyDeviceToHost);
        if (FILE *f = std::fopen(path.c_str(), "wb")) {
            std::fwrite(&count, sizeof(int), 1, f);
            std::fwrite(t.data(), sizeof(long long), t.size(), f);
            std::fclose(f);
        }
    }
    // clears the buffers the switches ask for and hands them to the launch
    void attach(dev::IrView &ir, const Engine &E) {
        ir.dbg = ir.dbg_all = nullptr;
        if (switches().ir_debug > 0) {
            if (!wg01) (void)hipMalloc((void **)&wg01, 256 * sizeof(long long));
            (void)hipMemsetAsync(wg01, 0, 256 * sizeof(long long), E.stream);
            ir.dbg = wg01;
        }
        if (switches().ir_debug >= 2) {
            const size_t need = (size_t)E.ir_grid * 32;
            if (need > all_len) {
                if (all) (void)hipFree(all);
                (void)hipMalloc((void **)&all, need * sizeof(long long));
                all_len = need;
            }
            (void)hipMemsetAsync(all, 0, need * sizeof(long long), E.stream);
            ir.dbg_all = all;
        }
    }
    // after the launch: every workgroup's stamps to the file, or the first two workgroups' phase times to stderr
    void report(const Engine &E) const {
        if (switches().ir_debug >= 2) {
            write_file(path(""), E.ir_grid, all, E.stream);
        } else if (switches().ir_debug > 0) {
            long long t[256];
            (void)hipStreamSynchronize(E.stream);
            (void)hipMemcpy(t, wg01, sizeof(t), hipMemcpyDeviceToHost);
            for (int w = 0; w < 2; w++) {
                std::fprintf(stderr, "k_bundle_ir wg%d phases (us):", w);
                for (int i = 1; i < 64 && t[64 * w + i]; i++) std::fprintf(stderr, " %.1f", (t[64 * w + i] - t[64 * w + i - 1]) * 0.01);
                std::fprintf(stderr, "\n");
            }
        }
    }
} g_stamps;

int update_enqueue(chip_kkt *h, const double *hsblocks_or_null) {
    Engine &E = h->E;
    const KktLayout &K = h->K;
    KktCones &C = h->cones;
    CHIP_HIP(hipSetDevice(E.device));
    if (C.has_hostHs) {
        if (!hsblocks_or_null)
            return fail(CHIP_ERR_ARG, "update: Hs blocks are required for PSD cones");
        for (const ConeSpec &c : K.cones) {
            if (c.tag <= CHIP_CONE_PSDTRIANGLE) continue; // (held on the device)
            CHIP_HIP(hipMemcpyAsync(h->d_tmp + c.block_start, hsblocks_or_null + c.block_start,
                                    (size_t)c.block_len * sizeof(double), hipMemcpyHostToDevice, E.stream));
            dev::scatter_values(E.stream, E.Kx, h->mapHs + c.block_start, h->d_tmp + c.block_start,
                                (int)c.block_len, -1.0);
        }
    }
    // static regulariser eps = c + prop * max|diag K| (directldlkktsolver.rs:324-329): with Zero /
    // Nonnegative / SecondOrder cones only, the kernels that write the diagonal entries leave their maxima in
    // slots (no pass over the N diagonal entries); other cone kinds take the explicit reduction
    const bool slot_eps = C.sym_only();
    C.write_kkt(E, h->mapHs, slot_eps && E.st.static_regularization_enable ? E.diag_slots() : nullptr);
    return E.refactor_enqueue(h->E.st.static_regularization_enable != 0, slot_eps ? nullptr : h->diag_full,
                              h->static_diag_max);
}
// the verdict of the last enqueued update, from the mailbox (Engine::refactor_collect has copied it)
int update_verdict(chip_kkt *h, int ok) {
    Engine &E = h->E;
    if (ok < 0) return ok;
    h->last_eps = E.st.static_regularization_enable ? E.mb_host->eps : 0.0;
    if (h->scaling_pending_check) {
        h->scaling_pending_check = false;
        if (E.mb_host->soc_fail == h->cones.scaling_gen) return 0;
    }
    return ok;
}
// an update enqueued earlier whose verdict the host has not read: read it now (a solve whose refinement decisions need
// the host must not run on a failed factorisation).  A failed update answers the `nslots` solves of the caller: true
bool pending_update_failed(chip_kkt *h, int nslots) {
    if (!h->pend_update) return false;
    h->pend_update = 2; // collected, verdict kept
    h->pend_update_ok = update_verdict(h, h->E.refactor_collect());
    if (h->pend_update_ok == 1) return false;
    h->pend_slots.insert(h->pend_slots.end(), (size_t)nslots, -1);
    return true;
}

// one pass writes the permuted rhs twice into work vectors k: bp (kept for the residuals) and x (solved in place), and
// folds ||b||inf into norm set 0 of context k -- no separate copy / norm launches
int stage_rhs(chip_kkt *h, int k, const double *rhsx_dev, const double *rhsz_dev) {
    Engine &E = h->E;
    SolveCtx &c = E.ctx[k];
    int rc = E.zero_norm_sets(c);
    if (rc) return rc;
    dev::setrhs_perm(c.stream, h->wk[k].bp, h->wk[k].x, rhsx_dev, rhsz_dev, E.perm, (int)h->K.n, (int)h->K.m, E.N, c.norm_set(0),
                     c.norm_nan(0));
    return CHIP_OK;
}

// the pair form of refine_begin, for two solves that walk the levels together (Engine::pair_lockstep_ok): a in context
// 0, b in context 1
void refine_begin_pair(Engine &E, const SolveVecs &a, const SolveVecs &b) {
    const chip_settings &st = E.st;
    if (!st.iterative_refinement_enable) {
        refine_begin(E, E.ctx[0], a.bp, a.x, a.e, a.dx);
        refine_begin(E, E.ctx[1], b.bp, b.x, b.e, b.dx);
        return;
    }
    E.enqueue_residual_pair(a.e, a.bp, a.x, b.e, b.bp, b.x, 1);
    if (st.iterative_refinement_max_iter >= 1) {
        E.enqueue_solve_pair(a.e, a.x, b.e, b.x);
        E.enqueue_residual_pair(a.dx, a.bp, a.e, b.dx, b.bp, b.e, 2);
    }
}

// the solve of the right-hand side that work vectors k hold (or that setrhs noted), in solve context k
int solve_core(chip_kkt *h, int k) {
    Engine &E = h->E;
    SolveCtx &c = E.ctx[k];
    SolveVecs &w = h->wk[k];
    const int N = E.N;
    if (!E.factored) return fail(CHIP_ERR_NOT_FACTORED, "solve() before the first update()");
    int rc;
    if (h->bp_stale && !h->rhs_deferred) h->rhs_deferred = true; // (the last fused solve left no permuted copy of b)
    if (h->rhs_deferred) { // (fused path not taken for this solve: stage the noted right-hand side now)
        h->rhs_deferred = false;
        h->bp_stale = false;
        if ((rc = stage_rhs(h, k, h->rhs_x, h->rhs_z))) return rc;
        h->x_holds_b = true;
    }
    int ok = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        w.last_ir = 0;
        if (!h->x_holds_b) { // solve() again on the same right-hand side, a full-N rhs in bp, or the second attempt
            if ((rc = E.zero_norm_sets(c))) return rc;
            CHIP_HIP(hipMemcpyAsync(w.x, w.bp, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
            dev::norm_inf(c.stream, w.bp, N, c.norm_set(0), c.norm_nan(0));
        }
        h->x_holds_b = false;
        E.enqueue_solve_inplace(c, w.x);
        ok = refine_core(E, c, w.bp, w.x, w.e, w.dx, w.last_ir);
        // non-finite with persistent sweeps in use: possibly a level barrier that timed out -- once more on the per-level
        // launches (a genuinely non-finite system fails again, at the price of one more solve)
        if (ok != 0 || attempt == 1 || !E.sweeps_after_failure()) break;
    }
    return ok;
}

// ---- the whole solve (setrhs permutation, LDL' solve, refinement with its decisions, getlhs) as ONE persistent launch
// the launch's view of ring slot `slot`: buffers, tolerances, epoch and flags; which kernel reads it is fused_choose's
dev::IrView ir_view_fill(chip_kkt *h, double *lhsx_dev, double *lhsz_dev, int slot) {
    Engine &E = h->E;
    const chip_settings &st = E.st;
    dev::IrView ir{};
    ir.rx = h->rhs_x;
    ir.rz = h->rhs_z;
    ir.n = (int)h->K.n;
    ir.m = (int)h->K.m;
    ir.N = E.N;
    ir.perm = E.perm;
    ir.run_ptr = h->ir_run_ptr;
    ir.runs = h->ir_runs;
    ir.bp = h->wk[0].bp;
    ir.xa = h->wk[0].x;
    ir.xb = h->wk[0].e;
    ir.ebuf = h->wk[0].dx;
    ir.lhsx = lhsx_dev;
    ir.lhsz = lhsz_dev;
    ir.part = E.ir_part;
    ir.ctl = E.ir_ctl;
    ir.rel = E.ir_rel;
    ir.epoch = (E.ir_epoch = (E.ir_epoch + 1) & 0x3fffff); // (tags are epoch << 8 | barrier number)
    ir.res = E.ir_res + 4 * slot;
    ir.res_host = nullptr;
    ir.abstol = st.iterative_refinement_abstol;
    ir.reltol = st.iterative_refinement_reltol;
    ir.stopratio = st.iterative_refinement_stop_ratio;
    ir.maxiter = st.iterative_refinement_max_iter;
    ir.ir_enable = st.iterative_refinement_enable;
    g_stamps.attach(ir, E);
    ir.test_drop = h->ir_test_drop ? 1 : 0;
    ir.flat = switches().no_flat ? 0 : 1;
    // (the residual of the last round still reads the right-hand side when that round's candidate is written)
    auto overlap = [](const double *a, size_t na, const double *b_, size_t nb_) { return a && b_ && a < b_ + nb_ && b_ < a + na; };
    const size_t n = (size_t)h->K.n, m = (size_t)h->K.m;
    ir.sf_flags = (switches().irs_flags < 0 ? 3 : switches().irs_flags) & ~(dev::IRS_F_DESC | dev::IRS_F_REP);
    ir.spec_out = (ir.sf_flags & 2) && !(overlap(lhsx_dev, n, ir.rx, n) || overlap(lhsx_dev, n, ir.rz, m) ||
                                         overlap(lhsz_dev, m, ir.rx, n) || overlap(lhsz_dev, m, ir.rz, m));
    return ir;
}
// which kernel takes the launch; sets what depends on it: ir.sf (0: k_bundle_ir or the step kernel, 1: k_bundle_irs,
// 2: k_bundle_irs_fixed), ir.bp, ir.pat_off, ir.desc, ir.res_host, and the index arrays of lv
enum FusedKernel { FK_STEP, FK_IRS, FK_IR };
FusedKernel fused_choose(const chip_kkt *h, dev::IrView &ir, dev::LdlView &lv, int slot) {
    const Engine &E = h->E;
    // grouped fold with small bundles: the register-resident form of the same launch (bundle_gstep.hip)
    if (E.gstep_solve_on && !switches().no_step_kernel && ir.maxiter <= 30) return FK_STEP;
    if (!h->ir_sf) return FK_IR;
    ir.sf = 1;
    ir.bp = nullptr; // (k_bundle_irs reads b through the runs every time; see chip_kkt::bp_stale)
    // k_bundle_irs: identical bundles read ONE copy of their index pattern through per-bundle entry offsets
    // (host.hpp: PatternShare); the kernel has no residual spill, the table travels in that slot of the view
    ir.pat_off = nullptr;
    if (E.pat_off && !switches().no_shared_pattern) {
        lv.Li16 = E.pat_Li16;
        lv.Lj16 = E.pat_Lj16;
        lv.Ucol16 = E.pat_Ucol16;
        lv.Urow16 = E.pat_Urow16;
        ir.pat_off = E.pat_off;
    }
    // one record per bundle in the same slot (the offsets are inside) unless the chained prologue is asked for
    if (h->irs_desc && !(ir.sf_flags & (dev::IRS_F_CHAINED)) && h->irs_desc_shared == (ir.pat_off != nullptr)) {
        ir.desc = (const dev::IrsDesc *)h->irs_desc;
        ir.sf_flags |= dev::IRS_F_DESC;
        // (the shared copies of this handle carry replica ids and the words behind the records say where)
        if (h->irs_rep_bundles && ir.pat_off && !(ir.sf_flags & dev::IRS_F_NOREP)) ir.sf_flags |= dev::IRS_F_REP;
    }
    if (E.mirror_writes()) ir.res_host = E.mb_mirror->ring + 4 * slot; // (workgroup 0 writes the verdict there as well)
    // this launch's switches are the constants k_bundle_irs_fixed has folded: per launch, set_settings can switch
    // refinement between two solves
    if (h->irs_fixed_ok && dev::bundle_irs_takes_fixed(E.fold, ir)) ir.sf = 2;
    return FK_IRS;
}
// *slot = where the verdict will appear in the result ring
int fused_enqueue(chip_kkt *h, double *lhsx_dev, double *lhsz_dev, int *slot) {
    Engine &E = h->E;
    int rc0;
    if (!E.factored) return fail(CHIP_ERR_NOT_FACTORED, "solve() before the first update()");
    *slot = E.ir_next;
    E.ir_next = (E.ir_next + 1) % Engine::IR_RING;
    dev::IrView ir = ir_view_fill(h, lhsx_dev, lhsz_dev, *slot);
    dev::LdlView lv = E.view();
    const FusedKernel kernel = fused_choose(h, ir, lv, *slot);
    h->bp_stale = ir.sf != 0;
    if ((rc0 = E.wait_for_exchange())) return rc0; // (no foreign kernel of ours beside a persistent launch)
    h->fused_args[*slot] = {h->rhs_x, h->rhs_z, lhsx_dev, lhsz_dev};
    h->rhs_deferred = false;
    h->x_holds_b = false;
    E.prof_begin(PF_IR);
    int rc;
    if (kernel == FK_STEP) {
        E.gstep.epoch += 1;
        dev::GStepView gsv = E.gstep;
        if (!E.gstep_vals_valid) gsv.gsl = gsv.gsu = nullptr; // (gather L and K through the source positions instead)
        rc = dev::gstep_solve(E.stream, lv, E.bundles, ir, E.gfold, gsv);
    } else {
        if (ir.sf == 2) h->irs_fixed_launches += 1;
        rc = dev::bundle_ir(E.stream, lv, E.bundles, E.fold, ir, E.ir_grid, E.ir_tw, E.gfold);
    }
    E.prof_end(PF_IR);
    if (rc) return fail(CHIP_ERR_HIP, hip_err((hipError_t)rc, "fused solve launch"));
    E.note_mailbox_writer(ir.res_host != nullptr);
    g_stamps.report(E);
    return CHIP_OK;
}
// verdict of ring slot `slot` (after the stream has been synchronised and the ring copied to the host);
// FUSED_TIMEOUT: the grid barrier timed out (not all workgroups were resident), the counters have been cleared
constexpr int FUSED_TIMEOUT = -1000;
int fused_verdict(chip_kkt *h, int slot) {
    Engine &E = h->E;
    const int *r = E.ir_res_host + 4 * slot;
    if (r[2] || r[0] == 0) {
        (void)hipMemsetAsync(E.ir_ctl, 0, E.ir_ctl_len * sizeof(int), E.stream);
        return FUSED_TIMEOUT;
    }
    h->wk[0].last_ir = r[1];
    return r[0] > 0 ? 1 : 0;
}
// the solve of ring slot `slot` once more, one kernel per phase with the refinement decisions on the host
// (same results up to rounding); the slot's right-hand side buffers must still hold what was enqueued
int fused_retry_unfused(chip_kkt *h, int slot) {
    Engine &E = h->E;
    const chip_kkt::FusedArgs &a = h->fused_args[slot];
    h->fused_fallbacks += 1;
    h->rhs_x = a.rx;
    h->rhs_z = a.rz;
    h->rhs_deferred = true;
    h->x_holds_b = true;
    const int ok = solve_core(h, 0);
    if (ok != 1) return ok;
    dev::getlhs_perm(E.stream, a.lx, a.lz, h->wk[0].x, E.iperm, (int)h->K.n, (int)h->K.m);
    CHIP_HIP(hipGetLastError());
    CHIP_HIP(hipStreamSynchronize(E.stream));
    return 1;
}
int fused_read_ring(chip_kkt *h) { return h->E.read_mailbox(); } // (the ring lives in the mailbox)
// does the fused launch take the next solve?  (solve() again on the same right-hand side after k_bundle_irs: the noted
// vectors once more)
bool fused_takes_solve(chip_kkt *h) {
    const Engine &E = h->E;
    if (h->bp_stale && !h->rhs_deferred) {
        h->rhs_deferred = true;
        h->x_holds_b = true;
    }
    return E.ir_fused && h->rhs_deferred && (E.prof_family == PF_NONE || E.prof_family >= PF_IR);
}

int update_block(chip_kkt *h, const int *map, const std::vector<i64> &hmap, const double *vals, size_t k) {
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if (!k) return CHIP_OK;
    for (size_t i = 0; i < k; i++) h->K.nzval[(size_t)hmap[i]] = vals[i]; // host mirror (chip_kkt_get_matrix)
    CHIP_HIP(hipMemcpyAsync(h->d_tmp, vals, k * sizeof(double), hipMemcpyHostToDevice, E.stream));
    dev::scatter_values(E.stream, E.Kx, map, h->d_tmp, (int)k, 1.0);
    CHIP_HIP(hipStreamSynchronize(E.stream));
    return CHIP_OK;
}

} // namespace

namespace chip {

// x <- K^-1 bp with iterative refinement (directldlkktsolver.rs:168-189, :266-321);
// everything in the engine's permuted numbering.  Returns the reference's bool.
//
// Buffer rotation instead of copies: x (solution), e (residual, then solved IN PLACE into the
// correction, then turned into the candidate x + dx), w (next residual).  Accepting a round
// renames (x, e, w) <- (e, w, x): the reference's mem::swap(x, dx) without moving data.
// (the refinement loop itself, shared by the L2 handle and by chip_ldl_solve_refined: xio / eio / wio are the three work
// vectors and come back renamed; x holds K^-1 bp's first approximation on entry)
// (in two halves, so that two independent solves can be enqueued on two streams before either is waited for)
void refine_begin(Engine &E, SolveCtx &c, const double *bp, double *x, double *e, double *w) {
    const chip_settings &st = E.st;
    if (!st.iterative_refinement_enable) {
        dev::norm_inf(c.stream, x, E.N, c.norm_set(1), c.norm_nan(1));
        return;
    }
    // The first refinement round is enqueued SPECULATIVELY together with the initial residual,
    // so that one host synchronisation (one D2H copy of norm sets 0..2) serves both decisions of
    // directldlkktsolver.rs:288-318; if ||e0|| already meets the tolerance the speculative
    // candidate is simply never looked at.  Decisions are exactly the reference's.
    E.enqueue_residual(c, e, bp, x, 1);
    if (st.iterative_refinement_max_iter >= 1) {
        // w <- e0 is needed if the round is rejected?  No: a rejected round leaves x untouched and e
        // is dead afterwards, so e is solved in place.
        E.enqueue_solve_inplace(c, e, x); // e <- x + K^-1 e0   (the candidate; "+ x" fused into the sweep)
        E.enqueue_residual(c, w, bp, e, 2);
    }
}
int refine_finish(Engine &E, SolveCtx &c, const double *bp, double *&xio, double *&eio, double *&wio, int &last_ir) {
    const chip_settings &st = E.st;
    int rc;
    if (!st.iterative_refinement_enable) {
        double nx;
        if ((rc = E.read_norm(c, 1, &nx))) return rc;
        return std::isfinite(nx) ? 1 : 0; // x.is_finite(), directldlkktsolver.rs:180
    }
    double *x = xio, *e = eio, *w = wio;
    const double abstol = st.iterative_refinement_abstol, reltol = st.iterative_refinement_reltol;
    const double stopratio = st.iterative_refinement_stop_ratio;
    const int maxiter = st.iterative_refinement_max_iter;
    double nn[3] = {0, 0, 0};
    if ((rc = E.read_norms(c, 0, maxiter >= 1 ? 3 : 2, nn))) return rc;
    const double normb = nn[0];
    double norme = nn[1];
    if (!std::isfinite(norme)) return 0;
    int set = 2;
    for (int it = 0; it < maxiter; it++) {
        if (norme <= abstol + reltol * normb) break;
        const double lastnorme = norme;
        if (it == 0) {
            norme = nn[2]; // already computed above
        } else {
            E.enqueue_solve_inplace(c, e, x);
            set += 1;
            if (set >= NRM_SETS) set = 3;
            if (it + 2 >= NRM_SETS) // the set is being reused: clear it first
                CHIP_HIP(hipMemsetAsync(c.norm_set(set), 0, NRM_SET_WORDS * sizeof(unsigned long long), c.stream));
            E.enqueue_residual(c, w, bp, e, set);
            if ((rc = E.read_norm(c, set, &norme))) return rc;
        }
        last_ir += 1;
        if (!std::isfinite(norme)) return 0;
        const double improved = lastnorme / norme;
        const bool accept = !(improved < stopratio) || improved > 1.0;
        if (accept) { // (x, e, w) <- (candidate, its residual, free)
            double *t = x;
            x = e;
            e = w;
            w = t;
        }
        if (improved < stopratio) break;
    }
    xio = x;
    eio = e;
    wio = w;
    return 1;
}
int refine_core(Engine &E, SolveCtx &c, const double *bp, double *&xio, double *&eio, double *&wio, int &last_ir) {
    refine_begin(E, c, bp, xio, eio, wio);
    return refine_finish(E, c, bp, xio, eio, wio, last_ir);
}

// The exchange's completion as an event the HANDLE owns (recorded here on the communicator's stream): a communicator
// destroyed before the handle's next persistent launch takes nothing the handle waits on with it.
int kkt_note_exchange(::chip_kkt *h, hipStream_t comm_stream) {
    Engine &E = h->E;
    if (!E.exch_event && hipEventCreateWithFlags(&E.exch_event, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        E.exch_event = nullptr;
        return CHIP_ERR_HIP;
    }
    if (hipEventRecord(E.exch_event, comm_stream) != hipSuccess) {
        (void)hipGetLastError();
        return CHIP_ERR_HIP;
    }
    E.exch_pending = true;
    return CHIP_OK;
}
// the L4 data updates (solver.cpp): K's device store only -- nothing reads the host mirror K.nzval after create but
// chip_kkt_get_matrix and the host-array updates of this layer, which the L4 solver does not use
int kkt_update_values_dev(::chip_kkt *h, int block, const double *src_dev, const int64_t *idx_dev, int k) {
    Engine &E = h->E;
    NEED_DEVICE(E);
    dev::pu_scatter(E.stream, E.Kx, block == 0 ? h->mapP : h->mapA, src_dev, idx_dev, k);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
void kkt_set_static_diag_max(::chip_kkt *h, double v) { h->static_diag_max = v; }

} // namespace chip

extern "C" {

int32_t chip_kkt_update_scaling_dev(chip_kkt *h, const double *s_dev, const double *z_dev, double mu,
                                    int32_t strategy) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    h->cones.next_generation();
    h->cones.update_scaling(E, s_dev, z_dev, mu, strategy);
    CHIP_HIP(hipGetLastError());
    E.note_mailbox_writer(false); // (the cones' verdict is in the device mailbox alone)
    h->scaling_pending_check = h->cones.reports_failure(); // verdict folded into the next update()
    return 1;
}
int32_t chip_kkt_update_scaling(chip_kkt *h, const double *s, const double *z, double mu, int32_t strategy) {
    if (!h || !s || !z) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    const size_t bytes = (size_t)h->K.m * sizeof(double);
    if (bytes) {
        CHIP_HIP(hipMemcpyAsync(h->d_s, s, bytes, hipMemcpyHostToDevice, E.stream));
        CHIP_HIP(hipMemcpyAsync(h->d_z, z, bytes, hipMemcpyHostToDevice, E.stream));
    }
    int rc = chip_kkt_update_scaling_dev(h, h->d_s, h->d_z, mu, strategy);
    if (rc < 0) return rc;
    if (h->cones.reports_failure()) {
        rc = E.read_mailbox();
        if (rc) return rc;
        h->scaling_pending_check = false;
        return E.mb_host->soc_fail == h->cones.scaling_gen ? 0 : 1;
    }
    CHIP_HIP(hipStreamSynchronize(E.stream));
    return 1;
}
int32_t chip_kkt_scaling_ok(chip_kkt *h) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    if (!h->scaling_pending_check) return 1;
    CHIP_HIP(hipSetDevice(E.device));
    int rc = E.read_mailbox();
    if (rc) return rc;
    h->scaling_pending_check = false;
    return E.mb_host->soc_fail == h->cones.scaling_gen ? 0 : 1;
}

int32_t chip_kkt_update(chip_kkt *h, const double *hsblocks_or_null) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    int rc = update_enqueue(h, hsblocks_or_null);
    if (rc) return rc;
    h->pend_update = 0;
    return update_verdict(h, E.refactor_collect());
}
int32_t chip_kkt_update_enqueue(chip_kkt *h, const double *hsblocks_or_null) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    int rc = update_enqueue(h, hsblocks_or_null);
    if (rc) return rc;
    h->pend_update = 1;
    E.factored = true; // provisionally: the verdict arrives with chip_kkt_collect
    return CHIP_OK;
}

// solver.rs:334-352 as ONE enqueue: cones.update_scaling(s, z, mu, strategy), then kktsystem.update's KKT part
// (get_Hs scatter, static regularisation, numeric refactor).  With Zero / Nonnegative / SecondOrder cones only, the
// scaling and the Hs / sparse-cone writes of a cone run in one launch (dev::sym_scale_write) and -- where the bundle
// factorisation can take over the preparation work (Engine::fast_prep_ok) -- nothing else is launched ahead of it.
int32_t chip_kkt_update_scaled_enqueue(chip_kkt *h, const double *s_dev, const double *z_dev, double mu, int32_t strategy,
                                       const double *hsblocks_or_null) {
    if (!h || !s_dev || !z_dev) return CHIP_ERR_ARG;
    Engine &E = h->E;
    KktCones &C = h->cones;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if (!C.sym_only() || !E.st.static_regularization_enable || switches().no_step_kernel) {
        // (PSD blocks that go into L directly: the clear of L's fill-in range starts now, beside the scaling kernels)
        if (!C.has_hostHs && C.psd_direct_rows()) E.hs_direct_prefill_async();
        int rc = chip_kkt_update_scaling_dev(h, s_dev, z_dev, mu, strategy);
        if (rc < 0) return rc;
        return chip_kkt_update_enqueue(h, hsblocks_or_null);
    }
    C.next_generation();
    h->scaling_pending_check = C.soc.ncones > 0;
    // the cone launch clears the status words of the refactor -- when it launches anything at all (no SOC cones and no
    // Nonnegative rows: an empty grid) and when the factor kernel that reads the slots is the one that will run
    const bool cone_clears = E.fast_prep_ok && !switches().no_fast_prep && (C.soc.ncones + C.nn_count) > 0 &&
                             (E.gstep_factor_on || !switches().no_factor_flat);
    long long *sdbg = nullptr;
    if (switches().ir_debug >= 3 && C.soc.ncones > 0) { // stamps of every cone workgroup -> <CHIP_IR_DEBUG_FILE>.scale
        (void)hipMalloc((void **)&sdbg, (size_t)C.soc.ncones * 32 * sizeof(long long));
        (void)hipMemsetAsync(sdbg, 0, (size_t)C.soc.ncones * 32 * sizeof(long long), E.stream);
    }
    C.scale_write(E, s_dev, z_dev, h->mapHs, cone_clears ? E.mb_dev->status : nullptr, sdbg);
    if (sdbg) {
        IrStamps::write_file(IrStamps::path(".scale"), C.soc.ncones, sdbg, E.stream);
        (void)hipFree(sdbg);
    }
    CHIP_HIP(hipGetLastError());
    int rc = E.refactor_enqueue(true, nullptr, h->static_diag_max, cone_clears);
    if (rc) return rc;
    h->pend_update = 1;
    E.factored = true; // provisionally: the verdict arrives with chip_kkt_collect
    return CHIP_OK;
}

int32_t chip_kkt_setrhs_dev(chip_kkt *h, const double *rhsx_dev, const double *rhsz_dev) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if (E.ir_fused) { // the solve kernel reads (and permutes) the caller's buffers itself, see the header
        h->rhs_x = rhsx_dev;
        h->rhs_z = rhsz_dev;
        h->rhs_deferred = true;
        h->x_holds_b = true;
        return CHIP_OK;
    }
    int rc = stage_rhs(h, 0, rhsx_dev, rhsz_dev);
    if (rc) return rc;
    h->x_holds_b = true;
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_kkt_setrhs(chip_kkt *h, const double *rhsx, const double *rhsz) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    const size_t n = (size_t)h->K.n, m = (size_t)h->K.m;
    if (n) CHIP_HIP(hipMemcpyAsync(h->d_rhs, rhsx, n * sizeof(double), hipMemcpyHostToDevice, E.stream));
    if (m) CHIP_HIP(hipMemcpyAsync(h->d_rhs + n, rhsz, m * sizeof(double), hipMemcpyHostToDevice, E.stream));
    int rc = chip_kkt_setrhs_dev(h, h->d_rhs, h->d_rhs + n);
    if (rc) return rc;
    CHIP_HIP(hipStreamSynchronize(E.stream)); // the caller may reuse rhsx/rhsz (they were copied to d_rhs)
    return CHIP_OK;
}

int32_t chip_kkt_solve_dev(chip_kkt *h, double *lhsx_dev, double *lhsz_dev) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if (fused_takes_solve(h)) {
        int slot = 0;
        int rc = fused_enqueue(h, lhsx_dev, lhsz_dev, &slot);
        if (rc) return rc;
        if ((rc = fused_read_ring(h))) return rc;
        rc = fused_verdict(h, slot);
        return rc == FUSED_TIMEOUT ? fused_retry_unfused(h, slot) : rc;
    }
    int ok = solve_core(h, 0);
    if (ok != 1) return ok;
    dev::getlhs_perm(E.stream, lhsx_dev, lhsz_dev, h->wk[0].x, E.iperm, (int)h->K.n, (int)h->K.m);
    CHIP_HIP(hipGetLastError());
    return 1;
}
int32_t chip_kkt_solve_dev_enqueue(chip_kkt *h, double *lhsx_dev, double *lhsz_dev) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if ((int)h->pend_slots.size() >= Engine::IR_RING) return fail(CHIP_ERR_ARG, "solve_dev_enqueue: 16 solves pending, collect first");
    if (fused_takes_solve(h)) {
        int slot = 0;
        int rc = fused_enqueue(h, lhsx_dev, lhsz_dev, &slot);
        if (rc) return rc;
        h->pend_slots.push_back(slot);
        return CHIP_OK;
    }
    // no fused launch for this system: the refinement decisions need the host -- a pending update's verdict is
    // read first, then the solve runs synchronously
    if (pending_update_failed(h, 1)) return CHIP_OK;
    const int ok = chip_kkt_solve_dev(h, lhsx_dev, lhsz_dev);
    if (ok < 0) return ok;
    h->pend_slots.push_back(-1 - ok); // -1 = failed, -2 = succeeded (already known)
    return CHIP_OK;
}
// Two INDEPENDENT solves of one interior-point iteration -- K x = [-q; b] of kktsystem.rs:108-125 (it does not depend on
// the residuals) and the affine direction of core/solver.rs:351-361 -- as one call.  Systems whose top is level-scheduled
// (a sweep = a chain of small launches, refinement decisions on the host) run them on two streams: both chains are
// enqueued before either is waited for, and the device overlaps them; the third solve of the iteration (the combined
// direction) depends on the affine result and stays a call of its own.  Fused handles (one persistent launch per solve,
// which fills the chip) run the two launches one after the other.  Same results as two chip_kkt_solve_dev_enqueue calls;
// two verdicts are appended for chip_kkt_collect.
int32_t chip_kkt_solve2_dev_enqueue(chip_kkt *h, const double *rhsx_a, const double *rhsz_a, double *lhsx_a, double *lhsz_a,
                                    const double *rhsx_b, const double *rhsz_b, double *lhsx_b, double *lhsz_b) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if ((int)h->pend_slots.size() + 2 > Engine::IR_RING) return fail(CHIP_ERR_ARG, "solve2_dev_enqueue: 16 solves pending, collect first");
    int rc;
    if (E.ir_fused || !E.pair_ok() || switches().no_solve_pair || E.prof_family != PF_NONE) { // (one after the other)
        if ((rc = chip_kkt_setrhs_dev(h, rhsx_a, rhsz_a))) return rc;
        if ((rc = chip_kkt_solve_dev_enqueue(h, lhsx_a, lhsz_a))) return rc;
        if ((rc = chip_kkt_setrhs_dev(h, rhsx_b, rhsz_b))) return rc;
        return chip_kkt_solve_dev_enqueue(h, lhsx_b, lhsz_b);
    }
    if (pending_update_failed(h, 2)) return CHIP_OK; // (the refinement decisions need the host)
    if (!E.factored) return fail(CHIP_ERR_NOT_FACTORED, "solve() before the first update()");
    SolveVecs &wb = h->wk[1];
    if (!wb.bp && (rc = wb.alloc(E, (size_t)E.N))) return rc;
    if ((rc = E.pair_begin())) return rc;
    const int n = (int)h->K.n, m = (int)h->K.m;
    h->rhs_deferred = false;
    h->x_holds_b = false;
    h->bp_stale = false;
    const double *const rhsx[2] = {rhsx_a, rhsx_b}, *const rhsz[2] = {rhsz_a, rhsz_b};
    double *const lhsx[2] = {lhsx_a, lhsx_b}, *const lhsz[2] = {lhsz_a, lhsz_b};
    // ---- both chains enqueued before either is waited for: A in context 0 (the main stream), B in context 1.  Wide chain
    // supernodes with a form for two right-hand sides: the two chains walk the levels together (Engine::enqueue_solve_pair)
    const bool lockstep = E.pair_lockstep_ok();
    for (int k = 0; k < 2; k++) {
        SolveVecs &w = h->wk[k];
        w.last_ir = 0;
        if ((rc = stage_rhs(h, k, rhsx[k], rhsz[k]))) return rc;
        if (lockstep) continue;
        E.enqueue_solve_inplace(E.ctx[k], w.x);
        refine_begin(E, E.ctx[k], w.bp, w.x, w.e, w.dx);
    }
    if (lockstep) {
        E.enqueue_solve_pair(h->wk[0].x, nullptr, wb.x, nullptr);
        refine_begin_pair(E, h->wk[0], wb);
    }
    // ---- decisions (and any further rounds) of A, then of B
    int ok[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        SolveVecs &w = h->wk[k];
        ok[k] = refine_finish(E, E.ctx[k], w.bp, w.x, w.e, w.dx, w.last_ir);
        if (ok[k] == 1) dev::getlhs_perm(E.ctx[k].stream, lhsx[k], lhsz[k], w.x, E.iperm, n, m);
    }
    if (ok[0] == 0 || ok[1] == 0) (void)E.sweeps_after_failure(); // (stale barrier words must not outlive a failed solve)
    // (the second stream: its results are complete when this call returns)
    const hipError_t se = hipStreamSynchronize(E.ctx[1].stream);
    if (se != hipSuccess) return fail(CHIP_ERR_HIP, hip_err(se, "second solve stream"));
    for (int k = 0; k < 2; k++)
        if (ok[k] < 0) return ok[k];
    h->pend_slots.push_back(-1 - ok[0]);
    h->pend_slots.push_back(-1 - ok[1]);
    return CHIP_OK;
}
int32_t chip_kkt_collect(chip_kkt *h, int32_t *update_ok, int32_t *nsolves, int32_t solves_ok[16]) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    int rc;
    int uok = 1;
    bool ring = false;
    for (int sl : h->pend_slots) ring = ring || sl >= 0;
    // ONE device-to-host copy (the mailbox: refactor status, cone-scaling verdict, the solves' verdict ring)
    if (h->pend_update == 1) uok = update_verdict(h, E.refactor_collect());
    else {
        if (h->pend_update == 2) uok = h->pend_update_ok;
        if (ring && (rc = E.read_mailbox())) return rc;
        if (!ring) CHIP_HIP(hipStreamSynchronize(E.stream));
    }
    h->pend_update = 0;
    if (uok < 0) return uok;
    if (update_ok) *update_ok = uok;
    int n = 0;
    rc = CHIP_OK;
    bool suspect = false; // a timed-out launch leaves the barrier counters dirty for the launches queued behind it
    for (int sl : h->pend_slots) {
        int v;
        bool repeated = false;
        if (sl < 0) v = -1 - sl;
        else {
            v = fused_verdict(h, sl);
            if (v == FUSED_TIMEOUT || suspect) {
                suspect = true;
                repeated = true;
                v = fused_retry_unfused(h, sl);
            }
            if (v < 0) rc = v;
        }
        // (2: the lhs was garbage until this repeat -- whatever consumed it on the device must be re-issued)
        if (solves_ok && n < 16) solves_ok[n] = v > 0 ? (repeated ? 2 : 1) : 0;
        n++;
    }
    h->pend_slots.clear();
    if (nsolves) *nsolves = n;
    return rc;
}
int32_t chip_kkt_solve(chip_kkt *h, double *lhsx, double *lhsz) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    const size_t n = (size_t)h->K.n, m = (size_t)h->K.m;
    int ok = chip_kkt_solve_dev(h, h->d_lhs, h->d_lhs + n);
    if (ok != 1) return ok;
    if (lhsx && n) CHIP_HIP(hipMemcpyAsync(lhsx, h->d_lhs, n * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    if (lhsz && m) CHIP_HIP(hipMemcpyAsync(lhsz, h->d_lhs + n, m * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    CHIP_HIP(hipStreamSynchronize(E.stream));
    return 1;
}
int32_t chip_kkt_set_settings(chip_kkt *h, const chip_settings *s) {
    if (!h || !s) return CHIP_ERR_ARG;
    chip_settings &d = h->E.st;
    d.static_regularization_enable = s->static_regularization_enable;
    d.static_regularization_constant = s->static_regularization_constant;
    d.static_regularization_proportional = s->static_regularization_proportional;
    d.dynamic_regularization_enable = s->dynamic_regularization_enable;
    d.dynamic_regularization_eps = s->dynamic_regularization_eps;
    d.dynamic_regularization_delta = s->dynamic_regularization_delta;
    copy_refinement_settings(d, *s);
    d.linesearch_backtrack_step = s->linesearch_backtrack_step;
    d.min_terminate_step_length = s->min_terminate_step_length;
    return CHIP_OK;
}
int32_t chip_kkt_solve_full(chip_kkt *h, double *x, const double *b) {
    if (!h || !x || !b) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    const size_t bytes = (size_t)E.N * sizeof(double);
    CHIP_HIP(hipMemcpyAsync(h->d_tmp, b, bytes, hipMemcpyHostToDevice, E.stream));
    dev::permute_in(E.stream, h->wk[0].bp, h->d_tmp, E.perm, E.N);
    h->x_holds_b = false;
    // bp was written directly: a right-hand side noted by an earlier setrhs() (borrowed pointers) is void
    h->rhs_deferred = false;
    h->bp_stale = false;
    h->rhs_x = h->rhs_z = nullptr;
    int ok = solve_core(h, 0);
    if (ok != 1) return ok;
    dev::permute_out(E.stream, h->d_tmp, h->wk[0].x, E.perm, E.N);
    CHIP_HIP(hipMemcpyAsync(x, h->d_tmp, bytes, hipMemcpyDeviceToHost, E.stream));
    CHIP_HIP(hipStreamSynchronize(E.stream));
    return 1;
}

int32_t chip_kkt_update_P(chip_kkt *h, const double *Pnzval) {
    if (!h || !Pnzval) return CHIP_ERR_ARG;
    int rc = update_block(h, h->mapP, h->K.mapP, Pnzval, h->K.mapP.size() - 1);
    h->static_diag_max = diag_P_max(h->K);
    return rc;
}
int32_t chip_kkt_update_A(chip_kkt *h, const double *Anzval) {
    if (!h || !Anzval) return CHIP_ERR_ARG;
    return update_block(h, h->mapA, h->K.mapA, Anzval, h->K.mapA.size() - 1);
}

} // extern "C"
