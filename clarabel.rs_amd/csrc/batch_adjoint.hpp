// batch_adjoint.hpp -- launchers of batch_adjoint.hip: the gradients of the batched L4 solver's solutions with respect
// to P, q, A and b (chip_bgrad_*, batch.cpp).  Every launcher covers all members at once; a member
// whose valid[k] is 0 contributes zeros and nothing of it is read as a number.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "batch.hpp"

namespace chip {
namespace dev {

// the right-hand side of the adjoint system in the solver's equilibrated space, and the point (s, z) the cones are
// scaled at.  gx / gz / gs: the incoming gradients of the UNSCALED solution (any may be null = zeros).
//   rx[j] = d[j] gx[j]                 (the caller subtracts A_int' ws)
//   ws[i] = gs[i] / e[i]
//   rz[i] = e[i] gz[i] / c[k]
//   ss[i], zs[i] = s[i], z[i] of the final iterate; for an invalid member the cones' unit vector
struct BaRhs {
    const int *valid;
    const double *gx, *gz, *gs, *d, *e, *c, *s, *z;
    double *rx, *ws, *rz, *ss, *zs;
};
void ba_rhs(hipStream_t st, const BatchPlan &p, const BaRhs &a);

// the gradients from the solution (vx, vz) of the adjoint system and the unscaled solution (x, z) of the solve:
//   ux[j] = (c[k] d[j]) vx[j],  uz[i] = e[i] vz[i]        (the adjoint variables of the unscaled problem)
//   dq[j] = -ux[j],  db[i] = uz[i] + gs[i]
//   dP[p] = -(ux[i] x[j] + ux[j] x[i])  (i < j),  -(ux[i] x[i])  (i == j)        on P's stored entries
//   dA[p] = -(z[i] ux[j] + uz[i] x[j]) - gs[i] x[j]                              on A's stored entries
// every output entry of an invalid member is an exact 0
struct BaGrad {
    const int *valid;
    const double *vx, *vz, *gs, *d, *e, *c, *x, *z;
    double *ux, *uz, *dq, *db, *dP, *dA;
};
void ba_grad_vectors(hipStream_t st, const BatchPlan &p, const BaGrad &a);
void ba_grad_matrices(hipStream_t st, const BatchPlan &p, const EqMats &M, const BaGrad &a);

} // namespace dev
} // namespace chip
