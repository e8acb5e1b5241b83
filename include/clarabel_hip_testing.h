/* clarabel_hip_testing.h -- test hooks of libclarabel_hip.so.  NOT part of the drop-in boundary (clarabel_hip.h):
 * these entry points exist only in libraries built with -DCHIP_TESTING (the in-tree default of csrc/Makefile, which
 * the test-suite needs; `make TESTING=0` leaves them out). */
#ifndef CLARABEL_HIP_TESTING_H
#define CLARABEL_HIP_TESTING_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* launches a kernel of `blocks` x `threads` (+ lds_bytes of LDS per workgroup) that only spins for `usec`
 * microseconds, on a private stream of `device` -- the persistent launches (k_bundle_ir, k_gstep_*) must survive a
 * co-resident kernel (the RCCL ring of the sharded path).  blocks = 0: waits for the spinners launched so far.
 * The calling thread's current device is left as it was. */
int32_t chip_debug_spin(int32_t device, int32_t blocks, int32_t threads, int32_t lds_bytes, double usec);
/* sets (value != NULL) or clears one CHIP_* diagnostic switch by its environment name and re-parses the switch
 * table (csrc/switches.hpp) -- for flipping a switch on handles that already exist; switches given in the
 * environment are picked up whenever a handle is created.  Returns CHIP_ERR_ARG for an unknown name. */
int32_t chip_debug_set_switch(const char *name, const char *value_or_null);
/* one structural figure of a KKT handle (opaque chip_kkt *, clarabel_hip.h) by name, for tests that must know which
 * mechanism a handle ended up with: "dense_blocks" / "dense_block_rows" (dense diagonal blocks of the top that the
 * residual multiplies from K's values directly), "nnzS" (entries of the full-row copy of the top rows), "psd_hs_row_blocks" (> 0: the PSD cones write Hs row by row
 * of the value store, k_psd_write_hs_rows),
 * "assembled_levels" (unit levels whose ancestor updates can be assembled per target column), "assembled_targets",
 * "pattern_classes" / "pattern_bundles" / "pattern_index_bytes" / "pattern_full_index_bytes" / "pattern_verified_bundles" /
 * "pattern_mismatches" (host analysis, on host-only handles too: classes of bundles with byte-equal 16-bit index
 * slices, the bundles, bytes of the shared index arrays and of the full ones, bundles whose offsets were checked against
 * the full arrays and how many differed), "pattern_shared_bundles" (bundles whose fused solve launch reads a shared copy:
 * 0 on a host-only handle or with CHIP_NO_SHARED_PATTERN), "irs_desc_bundles" (bundles whose fused solve launch reads its
 * per-bundle record under the current switches: 0 with CHIP_IRS_FLAGS bit 4, the chained prologue),
 * "irs_fixed_launches" (fused solve launches of this handle that took k_bundle_irs_fixed, the instance with the usual
 * switches folded: it stays 0 with CHIP_IRS_FLAGS bit 8, without refinement, with more than one top row),
 * "irs_replica_bundles" / "irs_replica_nodes" (bundles whose fused solve launch adds into replica slots of their dense
 * targets under the current switches, and those targets over all bundles; host analysis, on host-only handles too: 0
 * with CHIP_IRS_FLAGS bit 16 or bit 4, with CHIP_NO_SHARED_PATTERN, without records),
 * "mailbox_mirror_on" (1: the handle's update and
 * solves end in launches that store their verdict words into the host mirror of the mailbox; 0 with
 * CHIP_NO_HOST_MAILBOX), "mailbox_copies" / "mailbox_mirror_reads" (collects that copied the mailbox / that only waited
 * for the stream and read the mirror).
 * Returns CHIP_ERR_ARG for an unknown name. */
int32_t chip_debug_counter(const void *kkt_handle, const char *name, double *out);
/* one int32 array of a KKT handle by name; *len <- its length; out (may be NULL) receives it.  "irs_desc": the fused
 * solve kernel's per-bundle records (csrc/kernels.hpp: IrsDesc, 128 ints each: s0, nloc, nleaf, levels, dl, du, fb, fe,
 * runs, 3 of padding, 20 level entries, 32 x 3 run entries; empty when some bundle does not fit), on host-only handles
 * too.  Host-only handles of systems that kernel can take also keep the arrays its chained prologue walks:
 * "bundle_ptr", "blvl_ptr", "blvl", "Lp", "Up", "run_ptr", "runs", "pat_off" (empty: every bundle reads its own copy of
 * the index arrays), and "factor_bundle_desc": the run-coded bundle factorisation's per-bundle records (csrc/host.hpp:
 * Symbolic::fr_bdesc, 64 ints each; empty: no runs) with the shared arrays they point into, one copy per class of
 * identical bundles: "factor_class_usr", "factor_class_col" (bit patterns of unsigned words), "factor_class_sgn",
 * "factor_class_desc" (8 ints per run), "factor_class_rec" (4 per record); chip_debug_counter: "factor_classes",
 * "factor_class_verified" (bundles compared with what their record reaches), "factor_class_mismatches".
 * Replica slots (csrc/kernels.hpp: IRS_REP_R): "irs_rep", 4 ints per bundle {ND | R << 8, first replicated node, fold
 * level, 0} as they travel behind the records; on host-only handles "pat_Li16" / "pat_Ucol16" / "pat_Urow16", the shared
 * index copies as the kernel reads them (replica id in the top 4 bits), "Li16" / "Ucol16", the bundles' own (small
 * problems only), and "replica_plan": the words of "irs_rep" by the rule alone, also for systems whose bundles the
 * kernel does not take.
 * Returns CHIP_ERR_ARG for an unknown name. */
int32_t chip_debug_kkt_ints(const void *kkt_handle, const char *name, int64_t *len, int32_t *out);
/* the update records of the flat bundle factorisation (csrc/host.hpp: Symbolic::fu_rec / fr_desc) of one bundle of a
 * HOST-ONLY KKT handle, levels in order; *len <- ints; out (may be NULL) receives them.  "records": every update,
 * 5 ints each {level, slot a, slot b, column k, target}; "runs": the affine runs the analysis coded, 10 ints each {level,
 * first a, first b, first k, first target, strides of a, b, k, target, count} (none: the handle keeps the plain records
 * alone); "leftover": the records outside runs, 5 ints each like "records".  chip_debug_counter has the handle's totals,
 * on device handles too: "factor_record_bundles" (bundles that have update records at all), "factor_runs", "factor_run_leftover", "factor_run_max_leftover" (most in one bundle),
 * "factor_run_invalid" (descriptors that failed their range check: the handle then has no runs), "factor_run_kernel" (1:
 * the refactor launches the run form), "factor_records_on_device" (1: the plain records were uploaded).
 * CHIP_ERR_ARG for an unknown name, a bundle out of range or a handle with a device. */
int32_t chip_debug_factor_updates(const void *kkt_handle, int32_t bundle, const char *what, int64_t *len, int32_t *out);
/* the factor of a KKT handle as the last refactor left it on the device, permuted numbering: Lx[nnzL] (CSC order of
 * chip_kkt_get_symbolic), D[N]; either may be NULL.  Waits for the handle's stream. */
int32_t chip_debug_kkt_factors(void *kkt_handle, double *Lx, double *D);
/* a spinner of `blocks` x `threads` for `usec` microseconds on the stream of a communicator (opaque chip_comm *), behind
 * the collective enqueued last; the communicator's completion event moves behind it.  On one GPU this stands in for
 * the time RCCL's ring kernel holds CUs when several ranks exchange (bench.py --coresident). */
int32_t chip_comm_debug_spin(void *comm, int32_t blocks, int32_t threads, double usec);
/* ---- the problem transforms of chip_solver_create (csrc/problem_transform.cpp), host only: no device is touched ----
 * chip_debug_transform_create takes chip_solver_create's arguments (only the five transform fields of the settings are
 * read) and returns a handle even when nothing is transformed (then "active" reads 0). */
int32_t chip_debug_transform_create(void **out, int64_t n, int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval,
                                    const double *Pnzval, const double *q, const uint64_t *Acolptr,
                                    const uint64_t *Arowval, const double *Anzval, const double *b, int64_t ncones,
                                    const int32_t *cone_tags, const int64_t *cone_dims, const int64_t *cone_dims2,
                                    const double *cone_alphas_or_null, const void *solver_settings);
void chip_debug_transform_destroy(void *h);
/* one array of the transform by name; *len <- its length; out (may be NULL) receives it.  int64 arrays: "sizes"
 * ({active, n, m, m_reduced, n2, m2, npatterns, premerge_added, final_added, largest_clique}), "keep", "Pp", "Pi", "Ap",
 * "Ai", "dims", "dims2", "mode", "ptr", "src", "H_row", "tags" (int32 values widened); double arrays: "Px", "q", "Ax",
 * "b", "alphas".  Pattern k: "pattern<k>.ordering", ".snode_start", ".snode_len", ".parent", ".info" ({cone, row_orig,
 * row_pre, side, premerge_cliques}), ".sep<j>".  CHIP_ERR_ARG for an unknown name. */
int32_t chip_debug_transform_get(const void *h, const char *name, int64_t *len, void *out);
/* the host restatement of the device reverse, from UNSCALED internal vectors x2[n2], s2[m2], z2[m2]: x[n], s[m], z[m],
 * with the PSD completion when complete_dual is set */
int32_t chip_debug_transform_reverse(const void *h, const double *x2, const double *s2, const double *z2, double *x,
                                     double *s, double *z);
/* the internal variables of a chip_solver's last solve unscaled (dev::unscale's arithmetic): x2[n_internal],
 * s2[m_internal], z2[m_internal] (any may be NULL) */
int32_t chip_debug_solver_internal_solution(void *solver, double *x2, double *s2, double *z2);
/* ---- the interior-point loop's scalar logic (csrc/ipm_info.hpp), host only: no device is touched ----
 * info[21]: cost_primal, cost_dual, res_primal, res_dual, res_primal_inf, res_dual_inf, gap_abs, gap_rel, ktratio; the six
 * prev_ scalars in the same order (cost_primal .. gap_rel); r_tau, q'x, b'z, s'z, x'Px of the residuals; the status.
 * chip_debug_ipm_termination returns the status after check_termination at iteration `iter` of an info with those
 * scalars whose iteration count is `iterations` and whose solve time so far is `solve_time` (almost_post_process == 0),
 * or after post_process alone (!= 0); CHIP_ERR_ARG (negative) for a NULL argument.
 * chip_debug_ipm_info_update: DefaultInfo::update from the SQUARED weighted norms sq[8] of (x, d), (z, e), (s, einv),
 * (rx_inf, dinv), (Px, dinv), (rz_inf, einv), (rz, einv), (rx, dinv) and the dots in info[15..19]; writes info[0..8]. */
int32_t chip_debug_ipm_termination(const void *solver_settings, const double *info, int32_t iter, int32_t iterations,
                                   double solve_time, int32_t almost_post_process);
int32_t chip_debug_ipm_info_update(double *info, const double *sq, double tau, double kappa, double c, double normq,
                                   double normb);
/* ---- the batched solver (csrc/batch.cpp) ----
 * chip_debug_batch_inject_nan: at the start of iteration `iteration` of the next solves, before the residual pass and
 * the pre-update check, z[first row of member `member`] of the stacked iterate becomes NaN (member < 0: off).
 * chip_debug_batch_counter: "host_syncs" / "launches" (host synchronisations / kernel and copy enqueues of the last
 * solve's iterations, default_start and post-processing excluded), "loop_iterations" (iterations run);
 * "update_launches" / "update_host_syncs" (kernel, memset and copy enqueues / host synchronisations of the last
 * chip_bdata_update_* call); "backward_launches" / "backward_host_syncs" (the same of the last chip_bgrad_backward*
 * call); "jvp_launches" / "jvp_host_syncs" (the same of the last chip_bjvp_apply* call) and "jvp_refactors" (the
 * scaling updates + refactors that applies have paid over the handle's life: an apply that finds K factored at the
 * final iterates pays none).
 * chip_debug_batch_jvp_rhs: the right-hand side pass of chip_bjvp_apply (csrc/batch_tangent.hip: bt_rhs) alone on a
 * created handle, on a private stream; no solve is needed.  HOST arrays: x[n], z[m] (the unscaled solution the pass
 * reads), valid[nprob], the direction dq[n], db[m], dPx[nnz(P)], dAx[nnz(A)] (any of the four may be NULL = zeros);
 * returns the SCALED right-hand side rx[n] = c_k d (-(dq + dP_sym x + dA' z)), rz[m] = e (db - dA x).
 * Of the blocks (chip_bjac_*): the counters "jac_launches" / "jac_host_syncs" (of the last block call), "jac_refactors"
 * (scaling updates + refactors that blocks have paid), "jac_repeats" (blocks whose outputs were issued again because
 * chip_kkt_collect repeated a solve) and "jac_calls" (block calls that passed the argument checks).
 * chip_debug_batch_jac_rhs: the block form of chip_debug_batch_jvp_rhs (csrc/batch_jacobian.hip: bj_rhs): the inputs
 * hold ndir directions (direction-major, any of the four may be NULL), the results are rx[ndir][n], rz[ndir][m].
 * chip_debug_batch_jac_units: the unit right-hand sides (bj_units) of piece / first / ndir alone, the same results. */
int32_t chip_debug_batch_jac_rhs(void *batch, int32_t ndir, const double *x, const double *z, const int32_t *valid,
                                 const double *dq, const double *db, const double *dPx, const double *dAx, double *rx,
                                 double *rz);
int32_t chip_debug_batch_jac_units(void *batch, int32_t piece, int64_t first, int32_t ndir, const int32_t *valid,
                                   double *rx, double *rz);
/* Of the blocks of cotangents (chip_bvjp_*): the counters "vjp_launches" / "vjp_host_syncs" (of the last block call),
 * "vjp_refactors" (scaling updates + refactors that blocks have paid), "vjp_repeats" (blocks whose outputs were issued
 * again because chip_kkt_collect repeated a solve) and "vjp_calls" (block calls that passed the argument checks).
 * The three passes of a block alone on a created handle, on a private stream; no solve is needed; HOST arrays; the
 * valid flags are given.  form = 1 runs the block launcher (csrc/batch_cotangent.hip) ONCE; form = 0 runs the single
 * launchers of chip_bgrad_backward (csrc/batch_adjoint.hip) once per cotangent on that cotangent's slices.
 * chip_debug_batch_vjp_rhs: s[m], z[m] (the internal iterate the scaling point is read from), gx[ndir][n], gz[ndir][m],
 * gs[ndir][m] (any of the three may be NULL = zeros) -> rx[ndir][n] = d gx, ws[ndir][m] = gs / e,
 * rz[ndir][m] = e gz / c_k (the A' product is not part of the pass).
 * chip_debug_batch_vjp_units: the unit right-hand sides (bc_units) of piece / first / ndir alone, the same results.
 * chip_debug_batch_vjp_out: x[n], z[m] (the unscaled solution), the solves' results vx[ndir][n], vz[ndir][m] and
 * gs[ndir][m] (may be NULL) -> dq[ndir][n], db[ndir][m], dP[ndir][nnz(P)], dA[ndir][nnz(A)]; only the pieces in `want`
 * (bit 0 dq .. bit 3 dA) are written, in either form, and only their pointers are needed. */
int32_t chip_debug_batch_vjp_rhs(void *batch, int32_t form, int32_t ndir, const double *s, const double *z,
                                 const int32_t *valid, const double *gx, const double *gz, const double *gs, double *rx,
                                 double *ws, double *rz);
int32_t chip_debug_batch_vjp_units(void *batch, int32_t piece, int64_t first, int32_t ndir, const int32_t *valid,
                                   double *rx, double *ws, double *rz);
int32_t chip_debug_batch_vjp_out(void *batch, int32_t form, int32_t ndir, int32_t want, const double *x, const double *z,
                                 const int32_t *valid, const double *vx, const double *vz, const double *gs, double *dq,
                                 double *db, double *dP, double *dA);
int32_t chip_debug_batch_inject_nan(void *batch, int64_t member, int32_t iteration);
int32_t chip_debug_batch_counter(void *batch, const char *name, double *out);
int32_t chip_debug_batch_jvp_rhs(void *batch, const double *x, const double *z, const int32_t *valid, const double *dq,
                                 const double *db, const double *dPx, const double *dAx, double *rx, double *rz);
/* ---- the batched solver's partition and its device passes (csrc/batch.hpp), each alone ----
 * chip_debug_bplan_create: the partition chip_batch_create builds for nprob members of n_part[k] columns and m_part[k]
 * rows with the given cones (Zero / Nonnegative / SecondOrder), by the same code and with the same refusals; host only,
 * no device is touched.  chip_debug_bplan_get: one int32 array by name; *len <- its length; out (may be NULL) receives
 * it: "xoff", "zoff", "xmem", "zmem", "ch_beg", "ch_end", "cx_first", "cz_first", "it_beg", "it_end", "it_type",
 * "it_first", "rtype", and "sizes" = {nprob, n, m, ncx, ncz, nitems}.
 * The runners (one per launcher of batch.hpp) take HOST arrays of the stack's lengths (n, m, or nprob for the
 * per-member scalars, masks and outputs): the first one uploads the plan to the current device; each copies its
 * arrays to device buffers (one buffer per distinct host pointer, so aliased operands stay aliased; arrays written by
 * the pass are uploaded as well, so entries a pass leaves alone come back unchanged), calls the launcher ONCE on a
 * private stream, synchronises and copies the written arrays back.  NULL operands the launcher accepts are passed on
 * as NULL (y, sa, sb, mask, out_sum, b[j] of a sum); a NULL the kernel would read is refused with CHIP_ERR_ARG.
 * seg_reduce: `count` <= 16 specs (kind / space / slot / a / b per spec) into out[nslots * nprob]. */
int32_t chip_debug_bplan_create(void **out, int64_t nprob, const int64_t *n_part, const int64_t *m_part, int64_t ncones,
                                const int32_t *cone_tags, const int64_t *cone_dims);
/* the plan chip_bsym_create builds: PSDTriangle cones (cone_dims: the side) are accepted as well.  The handle is a
 * chip_debug_bplan handle (destroy, get and the runners take it).  Its rows of PSD cones have rtype 4 (ROW_PSD) and no
 * item; chip_debug_bplan_get knows, for either create, "degree" (per member), "psd_sizes" = {PSD cones of side > 0,
 * their diagonal entries, all PSD cones} and per PSD cone of side > 0, in row order, "psd_mem" (owner), "psd_start"
 * (first row), "psd_dim" (side), "psd_view" (index among all PSD cones, side 0 included), with "psd_first" (nprob + 1:
 * the member's first cone) and "psd_diag" (the rows of the diagonal svec entries, cone after cone). */
int32_t chip_debug_bsymplan_create(void **out, int64_t nprob, const int64_t *n_part, const int64_t *m_part,
                                   int64_t ncones, const int32_t *cone_tags, const int64_t *cone_dims);
void chip_debug_bplan_destroy(void *h);
int32_t chip_debug_bplan_get(const void *h, const char *name, int64_t *len, int32_t *out);
int32_t chip_debug_bplan_seg_reduce(void *h, int32_t count, const int32_t *kind, const int32_t *space,
                                    const int32_t *slot, const double *const *a, const double *const *b,
                                    int32_t nslots, double *out);
int32_t chip_debug_bplan_cone_minima(void *h, int32_t op, const double *dz, const double *ds, const double *z,
                                     const double *sv, const double *amax, double *out_min, double *out_sum_or_null);
int32_t chip_debug_bplan_blin(void *h, double *w, const double *x, const double *y, const double *sa, const double *sb,
                              double ca, double cb, int32_t space, const int32_t *mask, int32_t mask_mode);
int32_t chip_debug_bplan_bresid(void *h, double *rx, const double *rx_inf, const double *Px, const double *q,
                                double *rz, const double *rz_inf, const double *b, const double *tau);
int32_t chip_debug_bplan_bunit_shift(void *h, double *z, const double *alpha, int32_t primal, const int32_t *mask);
int32_t chip_debug_bplan_bunit_reset(void *h, double *x, double *sv, double *z, const int32_t *flag);
int32_t chip_debug_bplan_bunscale(void *h, double *xo, const double *x, const double *d, double *zo, const double *z,
                                  const double *e, double *so, const double *sv, const double *einv, const double *sx,
                                  const double *sz);
/* ---- the re-equilibration (csrc/reequilibrate.hip, chip_reequilibrate_problem / chip_reequilibrate_bdata) ----
 * chip_debug_reload_pass: the load pass (re_load) alone on `len` values.  HOST arrays: src[len]; dst[len + 4] and raw
 * (may be NULL) [len + 4] are uploaded whole, written at [o, o + len) and copied back whole, so the caller sees that
 * nothing around the range was touched.  o = 2 (a 16-byte boundary) for every array, or 1 (8 bytes past one) for the
 * arrays whose bit of `misalign` is set: 1 = dst, 2 = raw, 4 = src (src sits at its own o in a device buffer).  cap:
 * values above 1e20 become 1e20.
 * chip_debug_create_count: how often this process entered chip_kkt_create (which = 0) / chip_kktsystem_create (1). */
int32_t chip_debug_reload_pass(double *dst, double *raw_or_null, const double *src, int64_t len, int32_t cap,
                               int32_t misalign);
int32_t chip_debug_create_count(int32_t which, double *out);
/* ---- the passes of csrc/equilibrate.hip (the five launchers of csrc/equilibrate.hpp), each alone ----
 * The runners take HOST arrays, copy them to device buffers (one buffer per distinct host pointer, so aliased operands
 * stay aliased; arrays the pass writes are uploaded as well, so entries it leaves alone come back unchanged), call the
 * launcher ONCE on a private stream, synchronise and copy the written arrays back.  Sizes must fit the int32 indexing
 * of the passes (CHIP_ERR_DIM otherwise); every index is checked before anything is launched.
 * chip_debug_eq_ruiz_step: ONE Ruiz step from the state (Px, Ax, q, b, d, e, cstate = {c, the last factor}): P (n x n,
 * upper triangle) and A (m x n) are the caller's CSC triplets, turned into coordinate form by the function setup uses;
 * the norm words are zeroed as the equilibration loop zeroes them.  Px, Ax, q, b, d, e and cstate[0..1] are updated in place.
 * chip_debug_eq_rectify: the rectification over the row ranges [seg_beg[k], seg_end[k]) (0 <= beg < end <= m); Ax, b and
 * e are updated in place.  chip_debug_eq_invert: dinv[n] = 1 / d, einv[m] = 1 / e.
 * chip_debug_wnorm_batch: `count` <= 8 specs (v[j], w[j] of n[j] entries, into out[slot[j]], slot[j] < nslots); out is
 * uploaded and copied back whole.  chip_debug_unscale: xo[n] = (x d) sx, zo[m] = (z e) sz, so[m] = (sv einv) ss.
 * chip_debug_solver_scaled_state reads a chip_solver after a solve: the SCALED iterate x[n], s[m], z[m] and
 * tau_kappa[2], its dinv[n], einv[m] (internal sizes), and its info in the 21-double form above (info21[20] = status);
 * any may be NULL. */
int32_t chip_debug_eq_ruiz_step(int64_t n, int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval, double *Px,
                                const uint64_t *Acolptr, const uint64_t *Arowval, double *Ax, double *q, double *b,
                                double *d, double *e, double *cstate, double min_scaling, double max_scaling);
int32_t chip_debug_eq_rectify(int64_t n, int64_t m, const uint64_t *Acolptr, const uint64_t *Arowval, double *Ax,
                              double *b, double *e, int32_t nseg, const int32_t *seg_beg, const int32_t *seg_end);
int32_t chip_debug_eq_invert(const double *d, double *dinv, int64_t n, const double *e, double *einv, int64_t m);
int32_t chip_debug_wnorm_batch(int32_t count, const double *const *v, const double *const *w, const int32_t *n,
                               const int32_t *slot, int32_t nslots, double *out);
int32_t chip_debug_unscale(double *xo, const double *x, const double *d, double sx, int64_t n, double *zo,
                           const double *z, const double *e, double sz, double *so, const double *sv, const double *einv,
                           double ss, int64_t m);
int32_t chip_debug_solver_scaled_state(void *solver, double *x, double *s, double *z, double *tau_kappa, double *dinv,
                                       double *einv, double *info21);
/* ---- the PSD cone kernels (csrc/cones.hip: k_psd_update_scaling, k_psd_ops<0..6>) alone ----
 * chip_debug_psd_create: a bare view over a vector that holds only the svec ranges of `ncones` PSD triangle cones of
 * sides dims[] (0 .. 1024), in order: rows = sum n (n + 1) / 2.  The sizing is the function chip_kkt_create calls (state
 * of 3 n^2 + 2 n doubles per cone, maxdim, the maxdim > 64 scratch decision for ALL cones of the view and its stride);
 * host only, no device is touched until the first runner uploads it to the current device.
 * chip_debug_psd_counter: "gs" (1: work matrices in an HBM scratch slice, 0: in LDS), "jacobi_lds" (doubles of dynamic
 * LDS the last update_scaling / step_length / margins launch staged its SVD / eigenvalue iteration in; 0: not staged, or
 * gs == 0), "maxdim", "rows", "scratch_stride", "state_doubles".
 * The runners (one per launcher of cones.hip) take HOST arrays of `rows` entries (per-cone outputs: ncones), copy them to
 * device buffers (arrays the pass writes are uploaded as well), call the launcher ONCE on a private stream, synchronise
 * and copy the written arrays back.  update_scaling: *ok <- 0 when a cone's S or Z has no Cholesky factor (the flag
 * chip_kkt_update_scaling reads), 1 otherwise.  state: the state of cone `cone` as the kernels keep it, B (n x n, column
 * major) | lambda (n) | lambda^-1/2 (n) | R (n x n) | Rinv (n x n).  combined_ds_shift updates step_z (<- W step_z) and
 * step_s (<- W^-T step_s) in place, like the launcher. */
int32_t chip_debug_psd_create(void **out, int64_t ncones, const int64_t *dims);
void chip_debug_psd_destroy(void *h);
int32_t chip_debug_psd_counter(const void *h, const char *name, double *out);
int32_t chip_debug_psd_update_scaling(void *h, const double *s, const double *z, int32_t *ok);
int32_t chip_debug_psd_state(void *h, int64_t cone, double *out);
int32_t chip_debug_psd_mul_hs(void *h, double *y, const double *x);
int32_t chip_debug_psd_affine_ds(void *h, double *ds);
int32_t chip_debug_psd_combined_ds_shift(void *h, double *shift, double *step_z, double *step_s, double sigma_mu);
int32_t chip_debug_psd_ds_from_dz_offset(void *h, double *out, const double *ds);
int32_t chip_debug_psd_step_length(void *h, const double *dz, const double *ds, double amax, double *partial);
int32_t chip_debug_psd_margins(void *h, const double *z, double *pmin, double *psum);
int32_t chip_debug_psd_barrier(void *h, const double *z, const double *s, const double *dz, const double *ds,
                               double alpha, double *partial);
#ifdef __cplusplus
}
#endif
#endif
