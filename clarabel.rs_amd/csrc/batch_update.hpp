// batch_update.hpp -- launchers of batch_update.hip: the data updates of the batched L4 solver (chip_bdata_*,
// batch.cpp).  The stack's cost scale is one c_k per member, so every entry of P and q looks its scale up through the
// member of its column (c[xmem[col]]), and the norms of q and b are kept per member.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "batch.hpp"

namespace chip {
namespace dev {

// one piece of the stack's data and its equilibration (data_updating.rs with a cost scale per member):
//   matrices (row != nullptr)  full: dst = (v * (l[row] * r[col])) * c_k    partial: dst = ((l[row] * r[col]) * c_k) * v
//   vectors                    both: dst = (v * l[i]) * c_k
// with c_k = c[xmem[col]] (vectors: c[xmem[i]]); c == nullptr: no cost scale (A, b).  Vectors also keep the unscaled
// value in raw[i] (the norms are taken from it) and, when neg != nullptr, neg[i] = -dst[i]
struct BuTarget {
    double *dst, *raw, *neg;
    int len;
    const int *row, *col;
    const double *l, *r, *c;
    const int *xmem;
};

// the full form: one streaming pass over the len entries
void bu_write_full(hipStream_t s, const BuTarget &t, const double *vals);
// the partial form, the last occurrence of an index winning (pos[len] is -1 on entry and on return).  flag: the word
// pu_validate raised for a bad index -- when it is set nothing is written and clean[t] = 0 for every t, else
// clean[t] = idx[t]: the index list the later scatter into K may read without a host check in between
void bu_write_partial(hipStream_t s, const BuTarget &t, const int64_t *idx, const double *vals, int k, int *pos,
                      const int *flag, int64_t *clean);
// out[k] = max |raw[i]| over member k's entries of one space (0: x, 1: z), over the bit patterns of |x| (exact in any
// order; a NaN wins): one workgroup per chunk of the plan, then one thread per member.  partials: ncx + ncz words
void bu_norms(hipStream_t s, const BatchPlan &p, int space, const double *raw, unsigned long long *partials,
              double *out);

} // namespace dev
} // namespace chip
