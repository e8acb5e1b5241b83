// kkt_handle.hpp -- the L1 and L2 handles behind include/clarabel_hip.h and the few internal functions that cross
// their translation units.  Private to capi.cpp, capi_ldl.cpp, kkt_create.cpp, kkt_cones.cpp, kkt_step.cpp and
// capi_debug.cpp; the layers above reach a chip_kkt through the chip::kkt_* functions only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"
#include "kkt_cones.hpp"
#include "../../include/clarabel_hip_testing.h"

namespace chip {

inline const i64 *as_i64(const uint64_t *p) { return reinterpret_cast<const i64 *>(p); }

inline void fill_info(const Engine &E, chip_info *info) {
    std::memset(info, 0, sizeof(*info));
    std::strncpy(info->name, "hip", sizeof(info->name) - 1);
    info->threads = 1;
    info->direct = 1;
    info->nnzA = E.nnzK;
    info->nnzL = E.nnzL;
    info->n = E.N;
    info->n_levels = E.tree_depth;
    info->amd_lnz = E.amd.lnz;
    info->amd_ndiv = E.amd.ndiv;
    info->amd_nmultsubs_ldl = E.amd.nmultsubs_ldl;
    info->regularize_count = E.last_regularize_count;
    info->positive_inertia = -1;
}
int count_positive(Engine &E, i64 *out); // capi.cpp: positive entries of D
// diagnostics: the chain supernodes chosen by the symbolic analysis (capi.cpp)
int32_t get_supernodes(const Engine &E, int64_t *count, uint64_t *ptr, uint64_t *cols);

// the five refinement fields of the settings, the ones a solve may change per call
inline void copy_refinement_settings(chip_settings &d, const chip_settings &s) {
    d.iterative_refinement_enable = s.iterative_refinement_enable;
    d.iterative_refinement_reltol = s.iterative_refinement_reltol;
    d.iterative_refinement_abstol = s.iterative_refinement_abstol;
    d.iterative_refinement_max_iter = s.iterative_refinement_max_iter;
    d.iterative_refinement_stop_ratio = s.iterative_refinement_stop_ratio;
}

// the part of diag K no cone kernel writes: max |P_ii| (kkt_assembly.rs:120-121); a NaN entry makes it NaN
inline double diag_P_max(const KktLayout &K) {
    double mx = 0.0;
    for (i64 i = 0; i < K.n; i++) {
        const double a = K.nzval[(size_t)K.diagP[(size_t)i]];
        if (a != a) mx = a;
        else if (mx == mx) mx = std::max(mx, std::fabs(a));
    }
    return mx;
}

// the work vectors of one solve (N, permuted numbering): right-hand side, iterate, residual, correction
struct SolveVecs {
    double *bp = nullptr, *x = nullptr, *e = nullptr, *dx = nullptr;
    int last_ir = 0;
    int alloc(Engine &E, size_t N) {
        int rc;
        if ((rc = E.alloc(&bp, N)) || (rc = E.alloc(&x, N)) || (rc = E.alloc(&e, N))) return rc;
        return E.alloc(&dx, N);
    }
};

// x <- K^-1 bp with iterative refinement (kkt_step.cpp), shared by the L2 handle and chip_ldl_solve_refined
void refine_begin(Engine &E, SolveCtx &c, const double *bp, double *x, double *e, double *w);
int refine_finish(Engine &E, SolveCtx &c, const double *bp, double *&xio, double *&eio, double *&wio, int &last_ir);
int refine_core(Engine &E, SolveCtx &c, const double *bp, double *&xio, double *&eio, double *&wio, int &last_ir);

} // namespace chip

#define NEED_DEVICE(E) \
    if ((E).host_only) return chip::fail(CHIP_ERR_NO_DEVICE, "host-only handle: no numeric work without a GPU")

struct chip_ldl {
    chip::Engine E;
    std::vector<double> hK; // host mirror of the caller's K.nzval (update/scale/offset land here)
    bool dirty = true;
    double *d_b = nullptr, *d_x = nullptr, *d_y = nullptr;
    // ---- fast path of the strict drop-in (round 5) ----
    // registered index sets: the reference's update_values / scale_values / offset_values always come with one of a few
    // FIXED index vectors of the LDLDataMap (Hsblocks, diag_full, the sparse cones' u / v / D: datamaps.rs:350-362);
    // registered once, a set lives on the device as positions in the value store and an update moves 8 bytes per entry
    struct IndexSet {
        int *pos = nullptr;      // device: position of entry t in the device's value order
        int8_t *signs = nullptr; // device (or nullptr): the signs of offset_values
        chip::i64 k = 0;
    };
    std::vector<IndexSet> sets;
    double *d_vals = nullptr; // staging of one update's values
    chip::i64 d_vals_cap = 0;
    // once an update went to the device copy directly, THAT copy is the caller's K.nzval (the host mirror is stale and
    // chip_ldl_refactor no longer uploads it); chip_ldl_set_values makes the host mirror current again
    bool dev_values = false;
    chip::SolveVecs r; // device-resident refinement (chip_ldl_solve_refined), allocated by its first call
    std::vector<void *> pinned; // caller buffers registered with chip_ldl_pin_buffer
    ~chip_ldl() {
        for (void *p : pinned) (void)hipHostUnregister(p);
    }
};

struct chip_kkt {
    chip::KktLayout K;
    chip::Engine E;
    // int32 device copies of the LDLDataMap pieces the kernels index with
    int *mapHs = nullptr, *diag_full = nullptr, *mapP = nullptr, *mapA = nullptr;
    chip::KktCones cones;
    double *d_s = nullptr, *d_z = nullptr;
    double *d_rhs = nullptr, *d_lhs = nullptr; // n+m staging
    // wk[k] goes with the engine's solve context k; wk[1] is allocated by the first pair of solves
    // (chip_kkt_solve2_dev_enqueue)
    chip::SolveVecs wk[2];
    double *d_tmp = nullptr;                                         // max(N, nHs, nnzP, nnzA) staging
    size_t tmp_len = 0;
    double last_eps = 0;
    bool scaling_pending_check = false;
    bool x_holds_b = false; // x was initialised with the rhs by setrhs (skips a D2D copy)
    double static_diag_max = 0.0; // max |P_ii|: the diagonal entries of K that no cone kernel writes
    // fused solve path (Engine::ir_fused): setrhs only notes the caller's device buffers, the solve kernel
    // permutes them in; results of enqueued solves / updates not yet collected
    const double *rhs_x = nullptr, *rhs_z = nullptr;
    bool rhs_deferred = false;
    int *ir_run_ptr = nullptr, *ir_runs = nullptr; // run-length form of the permutation inside the bundles (dev::IrView)
    // k_bundle_irs takes this handle's fused solves (checked once at creation: every bundle qualifies, the grid is
    // co-resident).  That kernel does NOT leave the permuted right-hand side in bp: bp_stale says so, and a solve() that
    // follows without a new setrhs() reads the noted vectors (rhs_x / rhs_z) again -- they stay borrowed until the next
    // setrhs (include/clarabel_hip.h)
    bool ir_sf = false, bp_stale = false;
    bool irs_fixed_ok = false;       // k_bundle_irs_fixed is co-resident for this handle's grid (the launch decides, see fused_choose)
    long long irs_fixed_launches = 0; // test hook: fused solve launches that took k_bundle_irs_fixed
    // k_bundle_irs: one dev::IrsDesc per bundle (kkt_create.cpp: irs_descriptors), built once here because nothing in it
    // changes after creation; empty / nullptr: some bundle does not fit the record, the kernel keeps its chained prologue.
    // The host copy is there on host-only handles too (tests read it back: chip_debug_kkt_ints).
    std::vector<int> h_irs_desc;
    // the bundles' replica slots (kernels.hpp: IRS_REP_INTS per bundle, behind the records on the device; all zero: none)
    // and what the test hooks count: bundles with replicated nodes, replicated nodes over all bundles
    std::vector<int> h_irs_rep;
    int irs_rep_bundles = 0, irs_rep_nodes = 0;
    int *irs_desc = nullptr;
    bool irs_desc_shared = false; // the records on the device carry offsets into the SHARED index arrays
#ifdef CHIP_TESTING
    // host-only handles: the arrays the chained prologue walks, kept so that a test can walk them itself
    std::vector<int> t_bundle_ptr, t_blvl_ptr, t_blvl, t_Lp, t_Up, t_run_ptr, t_runs, t_pat_off;
    std::vector<int> t_pat_Li16, t_pat_Ucol16, t_pat_Urow16, t_Li16, t_Ucol16, t_rep_plan; // the shared index copies as the kernel reads them, the bundles' own
    // ... and the update records of the flat bundle factorisation, plain and run-coded (chip_debug_factor_updates)
    std::vector<uint16_t> t_fu_rec, t_fr_rec;
    std::vector<int> t_fu_ptr, t_fr_desc, t_fr_ptr, t_fr_rptr, t_fu_lvl_ptr, t_fr_bdesc, t_fc_usr, t_fc_col, t_fc_sgn, t_fc_desc, t_fc_rec;
#endif
    int pend_update = 0;             // 1: an update has been enqueued and its verdict not read; 2: read, kept
    int pend_update_ok = 1;
    std::vector<int> pend_slots;     // ring slots of the solves enqueued since the last collect
    // arguments of the fused launches by ring slot: a launch whose grid barrier timed out (its workgroups were not
    // co-resident: another long-running kernel held their slots) is repeated on the one-kernel-per-phase path
    struct FusedArgs {
        const double *rx, *rz;
        double *lx, *lz;
    } fused_args[chip::Engine::IR_RING] = {};
    int fused_fallbacks = 0;
#ifdef CHIP_TESTING
    bool ir_test_drop = chip::switches().ir_test_drop; // (tests, read when the handle is created)
#else
    static constexpr bool ir_test_drop = false;
#endif
    int world = 1;               // ranks sharing the problem (chip_kkt_attach_comm)
};
