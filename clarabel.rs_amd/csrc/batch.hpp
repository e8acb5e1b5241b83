// batch.hpp -- launchers of batch.hip: the per-member reductions and vector updates of the batched L4 solver
// (batch.cpp).  A batch is ONE block-diagonal stack: member k owns the columns [xoff[k], xoff[k+1]) and the rows
// [zoff[k], zoff[k+1]).  Every launcher covers all members at once; the number of launches never depends on nprob.
// Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "equilibrate.hpp"

struct chip_kktsystem;

namespace chip {
namespace dev {

// the fixed partition of the segmented reductions: every member's x range and z range cut into chunks of at most
// BATCH_CHUNK entries (chunks [0, ncx) cover x space, [ncx, ncx + ncz) z space).  The partial sum of a chunk is taken
// by one workgroup; a member's total adds its chunks' partials in chunk order, so results are deterministic.
constexpr int BATCH_CHUNK = 4096;
struct BatchPlan {
    int nprob, n, m;
    const int *xoff, *zoff;         // [nprob + 1] each: the members' column / row ranges
    const int *xmem, *zmem;         // member of every column / row
    const int *ch_beg, *ch_end;     // [ncx + ncz] entry ranges of the chunks
    const int *cx_first, *cz_first; // [nprob + 1] each: the member's chunks (z: relative to ncx)
    int ncx, ncz;
    // cone items for the minima / margins: a slice of at most BATCH_CHUNK Nonnegative rows, or one second-order cone
    const int *it_beg, *it_end, *it_type, *it_first; // it_first: [nprob + 1]
    int nitems;
    const int *rtype; // per row: ROW_ZERO / ROW_NN / ROW_SOC_HEAD / ROW_SOC_TAIL / ROW_PSD
};
// ROW_PSD (only in a plan of chip_bsym_create): a row of a PSDTriangle cone.  The kernels of this unit and of the
// derivative units take it for a row that carries no unit-vector entry and is not a Zero row either: no item covers it,
// bunit_shift leaves it alone (its primal form zeroes Zero rows only), bunit_reset and the scaling points write 0.
// batch_psd.hpp holds the cones' own description and adds the 1 of their diagonals
enum { ROW_ZERO = 0, ROW_NN = 1, ROW_SOC_HEAD = 2, ROW_SOC_TAIL = 3, ROW_PSD = 4 };
enum { ITEM_NN = 0, ITEM_SOC = 1 };

// segmented sums: out[slot * nprob + k] = the member-k part of the spec
enum { SEG_DOT = 0, SEG_WSQ = 1, SEG_SUM = 2, SEG_NONFINITE = 3 };
constexpr int SEG_MAX = 16;
struct SegSpec {
    const double *a, *b; // SEG_DOT: a.b   SEG_WSQ: sum (a b)^2   SEG_SUM: sum a   SEG_NONFINITE: #non-finite in a (and b)
    int kind, space, slot; // space 0: x (n), 1: z (m)
};
struct SegBatch {
    SegSpec s[SEG_MAX];
    int count;
};
size_t seg_scratch_doubles(const BatchPlan &p);
void seg_reduce(hipStream_t s, const BatchPlan &p, const SegBatch &bt, double *out, double *scratch);

// per-member minima over the cone items (one workgroup per item), then one thread per member:
//   CONE_STEP      (nonnegativecone.rs:128-153, socone.rs:289-302,421-495) of (dz, ds) at (z, s), capped by amax[k]:
//                  out_min[k] = the member's step length (amax[k] when it has no Nonnegative / SOC rows)
//   CONE_MARGINS   of z (compositecone.rs:197-206): out_min[k] = min margin (DBL_MAX without cones), out_sum[k] = the
//                  sum of the positive margins
//   CONE_INTERIOR  of s and z: out_min[k] = min(margin(s), margin(z)); > 0 iff strictly interior
enum { CONE_STEP = 0, CONE_MARGINS = 1, CONE_INTERIOR = 2 };
size_t cone_scratch_doubles(const BatchPlan &p);
void cone_minima(hipStream_t s, const BatchPlan &p, int op, const double *dz, const double *ds, const double *z,
                 const double *sv, const double *amax, double *out_min, double *out_sum, double *scratch);

// w = a_k x + b_k y over one space with a_k = sa ? sa[k] : ca, b_k = sb ? sb[k] : cb (y may be null: w = a_k x).
// mask (may be null): where mask[k] == 0 the entry becomes 0 (MASK_ZERO), y (MASK_Y) or stays (MASK_KEEP)
enum { MASK_ZERO = 0, MASK_Y = 1, MASK_KEEP = 2 };
struct BLin {
    double *w;
    const double *x, *y, *sa, *sb;
    double ca, cb;
    int space;
    const int *mask;
    int mask_mode;
};
void blin(hipStream_t s, const BatchPlan &p, const BLin &a);
// rx = rx_inf - Px - tau_k q, rz = rz_inf - tau_k b (residuals.rs:69-111 with the member's tau)
void bresid(hipStream_t s, const BatchPlan &p, double *rx, const double *rx_inf, const double *Px, const double *q,
            double *rz, const double *rz_inf, const double *b, const double *tau);
// z += alpha_k e (e: the cones' unit vector); primal: Zero rows set to 0 (scaled_unit_shift, compositecone.rs:208-214).
// mask (may be null): members with mask[k] == 0 are left alone
void bunit_shift(hipStream_t s, const BatchPlan &p, double *z, const double *alpha, int primal, const int *mask);
// members with flag[k] != 0: x = 0, s = z = e (unit_initialization, compositecone.rs:208-214)
void bunit_reset(hipStream_t s, const BatchPlan &p, double *x, double *sv, double *z, const int *flag);
// variables.rs:262-285 per member: xo = (x d) sx_k, zo = (z e) sz_k, so = (s einv) sx_k
void bunscale(hipStream_t s, const BatchPlan &p, double *xo, const double *x, const double *d, double *zo,
              const double *z, const double *e, double *so, const double *sv, const double *einv, const double *sx,
              const double *sz);

// one Ruiz step (problemdata.rs:246-297) of the stack with a cost scaling per member: bits as eq_bits_words(n, m)
// with one qinf word per member at the end (batch_eq_bits_words); cstate: [c_k][factor_k] (2 nprob doubles); seg: the
// scratch of seg_reduce plus nprob doubles for the column-norm sums
size_t batch_eq_bits_words(int n, int m, int nprob);
void batch_eq_ruiz_step(hipStream_t s, const BatchPlan &p, const EqMats &M, double *q, double *b, double *d, double *e,
                        unsigned long long *bits, double *seg_scratch, double *colsum, double *cstate, double min_scaling,
                        double max_scaling);

} // namespace dev

// y = aux + alpha * M x with the sparse operators of the L3 handle: which 0 = P (symmetric), 1 = A, 2 = A'
// (kktsystem.cpp).  Enqueued on the handle's stream.
int kktsystem_spmv(chip_kktsystem *h, int which, double *y, const double *aux, double alpha, const double *x);

} // namespace chip
