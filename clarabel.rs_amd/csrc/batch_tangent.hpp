// batch_tangent.hpp -- launchers of batch_tangent.hip: the forward-mode derivatives of the batched L4 solver's
// solutions (chip_bjvp_*, batch.cpp): how x, z, s of every member move when q, b, P, A move along a
// direction (dq, db, dP, dA).  Every launcher covers all members at once; a member whose valid[k] is 0 contributes
// zeros and nothing of it is read as a number.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "batch.hpp"

namespace chip {
namespace dev {

// one of the L3 handle's sparse operators as rows: row r holds the entries [ptr[r], ptr[r + 1]), entry t multiplies
// the vector at idx[t] and its value sits at position map[t] of the CALLER's nzval (P's stored triu / A's CSC order)
struct SpPattern {
    int rows;
    const int *ptr, *idx, *map;
};

// the right-hand side of the tangent system in the solver's equilibrated space, from the UNSCALED solution (x, z) of
// the solve and the direction (dq, db, dP, dA; any may be null = zeros), dP / dA read in place through the maps:
//   rx[j] = (c[k] d[j]) * -(dq[j] + sum_Psym dP[map] x[idx] + sum_Acol dA[map] z[idx])
//   rz[i] = e[i] * (db[i] - sum_Arow dA[map] x[idx])
// and, when ss is not null, the point (ss, zs) the cones are scaled at: s_int, z_int of the final iterate, for an
// invalid member the cones' unit vector (as ba_rhs writes it).  Every entry has one writer and a summation order
// that depends on the pattern alone.  Rows of the three operators are taken by their total entry count L:
// L <= BT_THREAD by one lane, L <= BT_WAVE by one wavefront, longer ones by the whole workgroup.
constexpr int BT_THREAD = 32, BT_WAVE = 16384;
struct BtRhs {
    const int *valid;
    const double *x, *z, *dq, *db, *dP, *dA, *d, *e, *c;
    double *rx, *rz;
    const double *s_int, *z_int;
    double *ss, *zs;
};
void bt_rhs(hipStream_t st, const BatchPlan &p, const SpPattern &Psym, const SpPattern &Acol, const SpPattern &Arow,
            const BtRhs &a);

// the tangents from the solution (vx, vz) of the tangent system and w = E rz - A^ vx:
//   dx[j] = d[j] vx[j],  dz[i] = e[i] vz[i] / c[k],  ds[i] = einv[i] w[i] on Nonnegative rows, +0.0 on Zero rows
// every output entry of an invalid member is an exact +0.0
struct BtOut {
    const int *valid;
    const double *vx, *vz, *w, *d, *e, *einv, *c;
    double *dx, *dz, *ds;
};
void bt_out(hipStream_t st, const BatchPlan &p, const BtOut &a);

} // namespace dev

// the row form of the L3 handle's operator `which` (0 = P symmetric, 1 = A by rows, 2 = A by columns; kktsystem.cpp)
int kktsystem_pattern(chip_kktsystem *h, int which, dev::SpPattern *out);

} // namespace chip
