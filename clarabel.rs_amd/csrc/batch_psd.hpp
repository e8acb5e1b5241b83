// batch_psd.hpp -- launchers of batch_psd.hip: the per-member side of PSDTriangle cones in the batched L4 solver
// (chip_bsym_create, batch.cpp), and the L2 accessors through which the batch runs the PSD cone
// reductions of its chip_kkt.  The cones themselves (scaling, Hs blocks, products) are the L2 handle's and run on the
// whole stack; what is per member is the fold of the per-cone results of cones.hip's k_psd_ops<4> / <5> into the
// member's slot, and the unit-vector operations on the diagonal svec entries.  BatchPlan (batch.hpp) knows nothing of
// PSD cones: their rows are ROW_PSD there, which every kernel of batch.hip leaves alone (bunit_reset writes its 0).
// Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

struct chip_kkt;

namespace chip {
namespace dev {

// the PSD cones of side > 0 in row order, hence sorted by member: member k owns the cones [first[k], first[k + 1]).
// view[c]: the cone's index among ALL PSDTriangle cones of the stack (the order of the L2 handle's PsdView, which
// also holds the cones of side 0).  diag: the rows of the diagonal svec entries k (k + 1) / 2 + k of every cone, cone
// after cone.  ncones == 0: the handle has no PSD cone and none of the launchers below is called
struct BatchPsdPlan {
    int nprob, ncones, ndiag;
    const int *first; // [nprob + 1]
    const int *view;  // [ncones]
    const int *diag;  // [ndiag]
    const int *zmem;  // member of every row (BatchPlan's)
};

// folds the per-cone results a[view[c]] (and b[view[c]]) into the member's slot behind cone_minima, one thread per
// member over its cones in order (deterministic; fmin as k_cone_final):
//   BP_INTERIOR  a = min eig of s, b = min eig of z:  out_min[k] = min(out_min[k], a, b)
//   BP_MARGINS   a = min eig, b = sum of positive eigs: out_min[k] = min(out_min[k], a), out_sum[k] += b
//   BP_STEP      a = the cone's step length (taken with alpha_max = 1): out_min[k] = min(out_min[k], a)
enum { BP_INTERIOR = 0, BP_MARGINS = 1, BP_STEP = 2 };
void bp_fold(hipStream_t s, const BatchPsdPlan &p, int op, const double *a, const double *b, double *out_min,
             double *out_sum);
// z += alpha_k e on the PSD diagonals (bunit_shift's part of these cones); mask (may be null): members with
// mask[k] == 0 are left alone
void bp_diag_shift(hipStream_t s, const BatchPsdPlan &p, double *z, const double *alpha, const int *mask);
// s = z = 1 on the PSD diagonals of the members with flag[k] != 0 (flag == null: of every member).  With the 0 that
// bunit_reset, or a derivative pass's scaling point, has written on every PSD row this is the cones' unit vector
void bp_diag_unit(hipStream_t s, const BatchPsdPlan &p, double *sv, double *z, const int *flag);

} // namespace dev

// L2 (kkt_cones.cpp): dev::psd_margins / dev::psd_step_length on the handle's PsdView and stream, one result per PSD cone
// of the stack (kkt_psd_cones of them) into device arrays of the caller.  Enqueued only: no copy, no synchronisation.
// The step length is that of the scaling the handle holds (chip_kkt_update_scaling_dev)
int kkt_psd_cones(const ::chip_kkt *h);
int kkt_psd_margins_dev(::chip_kkt *h, const double *z_dev, double *pmin_dev, double *psum_dev);
int kkt_psd_step_length_dev(::chip_kkt *h, const double *dz_dev, const double *ds_dev, double alpha_max,
                            double *alpha_dev);

} // namespace chip
