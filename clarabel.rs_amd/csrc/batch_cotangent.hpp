// batch_cotangent.hpp -- launchers of batch_cotangent.hip: BLOCKS of gradients of the batched L4 solver's solutions
// (chip_bvjp_*, batch_deriv.cpp): up to BC_MAX_DIR cotangents (gx, gz, gs) of every member's solution
// in one pass each, and the unit cotangents the ROWS of a member Jacobian are made of.  The passes are those of
// batch_adjoint.hpp with a cotangent index: given the same solve result, cotangent t of a block is, bit for bit, what
// the single pass computes on that cotangent.  A member whose valid[k] is 0 contributes zeros and nothing of it is read
// as a number.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "equilibrate.hpp"

namespace chip {
namespace dev {

// cotangents per block (the pending-solve limit of chip_kkt_collect)
constexpr int BC_MAX_DIR = 16;
// the pieces of a result a call wants
enum { BC_WANT_Q = 1, BC_WANT_B = 2, BC_WANT_P = 4, BC_WANT_A = 8, BC_WANT_ALL = 15 };

// the right-hand sides of ndir cotangents: BaRhs with cotangent t of an input at gx + t * n, gz + t * m, gs + t * m
// (a null input = zeros in every cotangent) and of the results at rx + t * srx, ws + t * sws, rz + t * srz:
//   rx[t][j] = d[j] gx[t][j]                 (the caller subtracts A_int' ws[t] when gs is given)
//   ws[t][i] = gs[t][i] / e[i]               (ws null: not written)
//   rz[t][i] = e[i] gz[t][i] / c[k]
//   ss[i], zs[i] = s[i], z[i] of the final iterate, for an invalid member the cones' unit vector; written once, and
//   only when ss is not null (K is not factored at the final iterates yet)
// An entry's member, flag, scalings and row type are loaded once for all cotangents
struct BcRhs {
    const int *valid;
    const double *gx, *gz, *gs, *d, *e, *c, *s, *z;
    double *rx, *ws, *rz;
    size_t srx, sws, srz;
    int ndir;
    double *ss, *zs;
};
void bc_rhs(hipStream_t st, const BatchPlan &p, const BcRhs &a);

// the right-hand sides of ndir UNIT cotangents, store only: cotangent t is, for every member, the unit vector at local
// position first + t of its own x (piece 0), z (piece 1) or s (piece 2); a member with fewer entries, or an invalid
// one, gets zeros.  What bc_rhs writes for these cotangents given explicitly:
//   piece 0: rx[t][j] = d[j] at j - xoff[k] == first + t
//   piece 1: rz[t][i] = e[i] / c[k] at i - zoff[k] == first + t
//   piece 2: ws[t][i] = 1 / e[i] at i - zoff[k] == first + t
// +0.0 everywhere else; ws null: not written; (ss, zs) as in BcRhs
struct BcUnits {
    const int *valid;
    const double *d, *e, *c, *s, *z;
    double *rx, *ws, *rz;
    size_t srx, sws, srz;
    int piece, ndir;
    long long first;
    double *ss, *zs;
};
void bc_units(hipStream_t st, const BatchPlan &p, const BcUnits &a);

// the gradients of ndir cotangents from the solutions (vx, vz) of their adjoint systems (cotangent t at vx + t * svx,
// vz + t * svz) and the unscaled solution (x, z) of the solve; with ux = (c[k] d) vx[t], uz = e vz[t]:
//   dq[t][j] = -ux[j],  db[t][i] = uz[i] + gs[t][i]
//   dP[t][p] = -(ux[i] x[j] + ux[j] x[i])  (i < j),  -(ux[i] x[i])  (i == j)      on P's stored entries
//   dA[t][p] = -(z[i] ux[j] + uz[i] x[j]) - gs[t][i] x[j]                          on A's stored entries
// cotangent t of a result at dq + t * n, db + t * m, dP + t * nnz(P), dA + t * nnz(A).  gs: cotangent t at gs + t * m;
// null with unit_s == 0: zeros; null with unit_s != 0: the unit vectors of bc_units' piece 2 (gs[t][i] = 1 at
// i - zoff[k] == first + t).  want: only the pieces whose bit is set are computed and stored; the others' pointers
// are not touched.  bc_grad_vectors covers dq and db (two entries per lane with 16-byte accesses when every operand and
// every cotangent's slice is 16-byte aligned, one entry per lane otherwise), bc_grad_matrices dP and dA (one stored
// entry per lane: its row, column, member, flag, scalings and x[i], x[j], z[i] are loaded once, only the gathers of
// vx[t], vz[t] and gs[t] repeat per cotangent).  Either launches nothing when want holds none of its pieces
struct BcGrad {
    const int *valid;
    const double *vx, *vz, *gs, *d, *e, *c, *x, *z;
    size_t svx, svz;
    int ndir, want, unit_s;
    long long first;
    double *dq, *db, *dP, *dA;
};
void bc_grad_vectors(hipStream_t st, const BatchPlan &p, const BcGrad &a);
void bc_grad_matrices(hipStream_t st, const BatchPlan &p, const EqMats &M, const BcGrad &a);

} // namespace dev
} // namespace chip
