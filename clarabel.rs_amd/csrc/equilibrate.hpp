// equilibrate.hpp -- launchers of equilibrate.hip (the L4 solver's data-parallel work) and the internal residual pass
// with the scaled norms of DefaultInfo::update.  Internal to the library: solver.cpp and kktsystem.cpp include it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/clarabel_hip.h"

namespace chip {
namespace dev {

// problem data in the coordinate form the entry-parallel passes walk: for every stored entry its row and column
// (CSC order, so the values line up with the caller's nzval)
struct EqMats {
    const int *Prow, *Pcol;
    double *Px;
    int nnzP;
    const int *Arow, *Acol;
    double *Ax;
    int nnzA;
};

// bits: [dwork n][ework m][pcol n][qinf 1] as the bit patterns of non-negative doubles (atomicMax on u64), zeroed by
// the caller before every Ruiz step (one memset)
size_t eq_bits_words(int n, int m);
int eq_cost_partials();
// one Ruiz step (problemdata.rs:246-297) without a host synchronisation: column / row inf-norms of [P A; A' 0],
// the scaling factors (zeros -> 1, 1/sqrt, clipped against the cumulative d / e), D P D, E A D, D q, E b, d, e, and the
// cost scaling decided on the device: cstate[0] = c, cstate[1] = the factor of this step (1 when skipped)
void eq_ruiz_step(hipStream_t s, const EqMats &M, double *q, double *b, double *d, double *e, int n, int m,
                  unsigned long long *bits, double *partials, double *cstate, double min_scaling, double max_scaling);
// compositecone.rs:183-195: delta = mean(e over the cone) / e on the ranges [seg_beg, seg_end) of the cones that
// take a scalar equilibration, 1 elsewhere; then A <- diag(delta) A, b <- delta b, e <- delta e.  work: m doubles
void eq_rectify(hipStream_t s, const EqMats &M, double *b, double *e, int m, const int *seg_beg, const int *seg_end,
                int nseg, double *work);
// dinv = 1 / d, einv = 1 / e
void eq_invert(hipStream_t s, const double *d, double *dinv, int n, const double *e, double *einv, int m);

// sum of (v w)^2 for up to WNORM_MAX (v, w) pairs, out[slot] (deterministic fixed partition); scratch:
// wnorm_scratch_doubles()
constexpr int WNORM_MAX = 8;
struct WNormSpec {
    const double *v, *w;
    int n, slot;
};
struct WNormBatch {
    WNormSpec s[WNORM_MAX];
    int count;
};
int wnorm_scratch_doubles();
void wnorm_batch(hipStream_t s, const WNormBatch &bt, double *out, double *scratch);

// variables.rs:262-285: xo = (x d) sx, zo = (z e) sz, so = (s einv) ss
void unscale(hipStream_t s, double *xo, const double *x, const double *d, double sx, int n, double *zo, const double *z,
             const double *e, double sz, double *so, const double *sv, const double *einv, double ss, int m);

} // namespace dev

// Residuals::update (residuals.rs:69-111) as chip_residuals_update does it, plus the weighted squared norms of
// `wn` (DefaultInfo::update's scaled norms, info.rs:142-165) reduced in the same launches and returned, as sums of
// squares, in wsq[0 .. wn->count) by the same single device-to-host copy.  Slots 0-7 of the handle's dot buffer.
int residuals_update_wnorms(chip_kktsystem *h, const chip_vars *variables, double *rx_dev, double *rz_dev,
                            double *rx_inf_dev, double *rz_inf_dev, double *Px_dev, double out5[5],
                            const dev::WNormBatch *wn, double *wsq);

} // namespace chip
