// batch_jacobian.hpp -- launchers of batch_jacobian.hip: BLOCKS of forward-mode derivatives of the batched L4 solver's
// solutions (chip_bjac_*, batch_deriv.cpp): up to BJ_MAX_DIR directions (dq, db, dP, dA) of every
// member's data in one pass each, and the unit directions a member Jacobian is made of.  The passes are those of
// batch_tangent.hpp with a direction index: direction t of a block is, bit for bit, what the single pass computes
// on that direction.  A member whose valid[k] is 0 contributes zeros and nothing of it is read as a number.
// Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "batch.hpp"
#include "batch_tangent.hpp"

namespace chip {
namespace dev {

// directions per block (the pending-solve limit of chip_kkt_collect) and per walk of a row
constexpr int BJ_MAX_DIR = 16, BJ_TILE = 4;

// the right-hand sides of ndir directions: BtRhs with direction t of an input at in + t * its stride (sq, sb, sP, sA;
// a null input = zeros for every direction) and direction t of the results at rx + t * srx, rz + t * srz.  A row's
// owner (lane, wavefront or workgroup by the row's entry count, as in bt_rhs) walks the row once per BJ_TILE
// directions: idx, map and the vector's entry are loaded once and used for every direction of the tile, and every
// direction's sum runs in bt_rhs's order.  (ss, zs) as in BtRhs, written once
struct BjRhs {
    BtRhs one; // direction 0 and what the directions share
    int ndir;
    size_t sq, sb, sP, sA, srx, srz;
};
void bj_rhs(hipStream_t st, const BatchPlan &p, const SpPattern &Psym, const SpPattern &Acol, const SpPattern &Arow,
            const BjRhs &a);

// the right-hand sides of ndir UNIT directions, store only: direction t is, for every member, the unit vector at
// local position first + t of its own q (piece 0) or b (piece 1); a member with fewer entries, or an invalid one,
// gets zeros.  What bj_rhs writes for these directions given explicitly:
//   piece 0: rx[t][j] = -(c[k] d[j]) at j - xoff[k] == first + t, +0.0 elsewhere; rz = +0.0
//   piece 1: rz[t][i] = e[i] at i - zoff[k] == first + t, +0.0 elsewhere; rx = +0.0
// and (ss, zs) as in BtRhs when ss is not null
struct BjUnits {
    const int *valid;
    const double *d, *e, *c;
    double *rx, *rz;
    size_t srx, srz;
    int piece, ndir;
    long long first;
    const double *s_int, *z_int;
    double *ss, *zs;
};
void bj_units(hipStream_t st, const BatchPlan &p, const BjUnits &a);

// the tangents of ndir directions: BtOut with direction t of the solutions and products at vx + t * svx, vz + t * svz,
// w + t * svz and of the results at dx + t * n, dz + t * m, ds + t * m.  An entry's scalings, member and flag are
// loaded once for all directions.  Two entries per lane with 16-byte accesses when every operand and every direction's
// slice is 16-byte aligned, one entry per lane otherwise
struct BjOut {
    BtOut one; // direction 0 and what the directions share
    int ndir;
    size_t svx, svz;
};
void bj_out(hipStream_t st, const BatchPlan &p, const BjOut &a);

} // namespace dev
} // namespace chip
