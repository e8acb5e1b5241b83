// ir_refine.hpp -- what the three fused-solve kernels (k_bundle_ir, k_bundle_irs: bundle_ir.hip; k_gstep_solve:
// bundle_gstep.hip) share: the right-hand side / result through the permutation, the reference's refinement decisions,
// the k x k top part of the sweeps.  The kernels differ in where the vectors live and in how the grid synchronises;
// what is decided, and in which operation order, is written once, here.
#pragma once
#include "dev_common.hpp"

namespace chip {
namespace dev {

namespace {

// entry o of the right-hand side in the caller's order (directldlkktsolver.rs:160-166: the sparse-cone rows are zero)
__device__ __forceinline__ double ir_rhs(const IrView &ir, int o) {
    return o < ir.n ? ir.rx[o] : (o < ir.n + ir.m ? ir.rz[o - ir.n] : 0.0);
}
// ... and entry o of the result (directldlkktsolver.rs:205-215; either output may be absent)
__device__ __forceinline__ void ir_put(const IrView &ir, int o, double val) {
    if (o < ir.n) {
        if (ir.lhsx) ir.lhsx[o] = val;
    } else if (o < ir.n + ir.m) {
        if (ir.lhsz) ir.lhsz[o - ir.n] = val;
    }
}
// original index of bundle-local node i through the runs (LDS); successive calls with ascending i: one monotone walk
struct RunWalk {
    const int *runs;
    int r;
    __device__ __forceinline__ int orig(int i) {
        while (i >= runs[3 * r] + runs[3 * r + 2]) ++r; // (runs ascend in the local index)
        return runs[3 * r + 1] + (i - runs[3 * r]);
    }
};

// a thread's part of an inf-norm: NaNs are kept out of the maximum and flagged instead
__device__ __forceinline__ void norm_take(double val, double &m, bool &nan) {
    if (val != val) nan = true;
    else m = fmax(m, fabs(val));
}
// ... and the workgroup's: the maximum, or NaN if any thread flagged one (in every thread)
__device__ __forceinline__ double block_norm_or_nan(double m, bool nan, double *red) {
    m = block_max(m, red);
    const bool anynan = __syncthreads_or(nan);
    return norm_or_nan(m, anynan);
}

// the refinement state the decisions read and write (one copy per workgroup, in LDS, written by thread 0)
struct IrVerdict {
    double normb, norme, lastnorme;
    int rounds, ok, done, sel, accept; // sel: which of the two iterate slots holds the accepted x; accept: the last verdict
};
__device__ __forceinline__ void ir_verdict_init(IrVerdict &s) {
    s.normb = s.norme = s.lastnorme = 0.0;
    s.rounds = 0;
    s.ok = 1;
    s.done = 0;
    s.sel = 0;
    s.accept = 0;
}
// The reference's decisions (directldlkktsolver.rs:284-318) about the candidate of round `round`, whose residual has the
// norm `newnorm` (no refinement: the norm of the candidate itself -- only x.is_finite() is asked for, :180); s.normb is
// the caller's to set in round 0.  Returns whether the candidate is accepted: the caller then copies its top entries to
// its accepted slot (s.sel has been flipped).  One thread.  (k_bundle_irs keeps a copy of the body, see there.)
__device__ __forceinline__ bool ir_verdict(IrVerdict &s, const IrView &ir, int round, double newnorm) {
    const double tol = ir.abstol + ir.reltol * s.normb;
    bool accept, done = false;
    if (round == 0) {
        accept = true;
        s.norme = newnorm;
        if (!(newnorm - newnorm == 0.0)) { // non-finite (:284-286; without refinement: x.is_finite(), :180)
            s.ok = 0;
            done = true;
        } else if (!ir.ir_enable || ir.maxiter <= 0 || newnorm <= tol) {
            done = true;
        }
    } else {
        s.rounds += 1;
        if (!(newnorm - newnorm == 0.0)) { // :305-307
            s.ok = 0;
            accept = false;
            done = true;
        } else {
            const double improved = s.lastnorme / newnorm;
            accept = !(improved < ir.stopratio) || improved > 1.0; // :309-318
            if (improved < ir.stopratio) done = true;
            if (accept) s.norme = newnorm;
        }
    }
    s.accept = accept ? 1 : 0;
    if (accept) s.sel ^= 1;
    if (!done && (s.rounds >= ir.maxiter || s.norme <= tol)) done = true; // :288-293
    s.lastnorme = s.norme;
    s.done = done ? 1 : 0;
    return accept;
}

// The k x k top part of both sweeps (k <= 8): y0(i) = the right-hand side of top row i less the bundles' forward shares;
// forward with L(top, top) (ltt, rows of 8), 1 / d, backward; the result in dxt.  One thread.
// (y in LDS, dxt: a private array indexed by a loop variable lives in scratch memory, and its reloads sat on the
// critical path right behind the barrier.  k_bundle_ir keeps two copies of the body, see there.)
template <class Y0>
__device__ __forceinline__ void ir_top_solve(int k, Y0 y0, const double *ltt, const double *dinvt, double *dxt) {
    for (int i = 0; i < k; ++i) {
        double sacc = y0(i);
        for (int j = 0; j < i; ++j) sacc -= ltt[i * 8 + j] * dxt[j];
        dxt[i] = sacc;
    }
    for (int i = k - 1; i >= 0; --i) {
        double sacc = dxt[i] * dinvt[i];
        for (int j = i + 1; j < k; ++j) sacc -= ltt[j * 8 + i] * dxt[j];
        dxt[i] = sacc;
    }
}
// a top entry of the candidate: x (round 0) or x + dx (directldlkktsolver.rs:300 axpby(1, x, 1), in that operation order)
__device__ __forceinline__ double ir_top_cand(int round, double cur, double dx) {
    return round == 0 ? dx : 1.0 * cur + 1.0 * dx;
}

} // namespace

} // namespace dev
} // namespace chip
