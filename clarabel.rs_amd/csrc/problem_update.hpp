// problem_update.hpp -- launchers of problem_update.hip (the L4 solver's data updates, default/data_updating.rs) and
// the internal device-value entry points of L2 (kkt_step.cpp) and L3 (kktsystem.cpp) they feed.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/clarabel_hip.h"

namespace chip {
namespace dev {

// one piece of the solver's data and its equilibration: dst[i] = the new value v scaled as update_matrix /
// update_vector do it (data_updating.rs), with l = lscale, r = rscale (matrices: row / column of every entry),
// c = cscale (has_c = false: None)
struct PuTarget {
    double *dst;
    int len;
    const int *row, *col; // nullptr for a vector
    const double *l, *r;  // vectors: l = vscale, r unused
    double c;
    bool has_c;
};

// flag <- 1 when some idx[t] (t < k) is negative or >= len; the caller zeroes flag first
void pu_validate(hipStream_t s, const int64_t *idx, int k, int64_t len, int *flag);
// the full form: dst[t] = scaled(vals[t]) for t < k == len (one streaming pass)
void pu_write_full(hipStream_t s, const PuTarget &t, const double *vals);
// the partial form, the last occurrence of an index winning: pos[len] is -1 on entry and on return (only the touched
// entries are written back)
void pu_write_partial(hipStream_t s, const PuTarget &t, const int64_t *idx, const double *vals, int k, int *pos);
// Kx[map[i]] = src[i] for i = t (idx == nullptr) or i = idx[t], t < k (a repeated i writes the same value twice)
void pu_scatter(hipStream_t s, double *Kx, const int *map, const double *src, const int64_t *idx, int k);
// the stored norms (problemdata.rs:168-189) and max |P_ii| (kkt_handle.hpp: diag_P_max), as maxima of |x| over the bit
// patterns (a NaN wins).  mask bit 0: out[0] = max |q dinv|; bit 1: out[1] = max |b einv|; bit 2: out[2] = max over
// the diagonal entries of P (Prow == Pcol).  partials: pu_norm_partials() words
int pu_norm_partials();
void pu_norms(hipStream_t s, int mask, const double *q, const double *dinv, int n, const double *b, const double *einv,
              int m, const int *Prow, const int *Pcol, const double *Px, int nnzP, unsigned long long *partials,
              double *out);

} // namespace dev

// L2: new values of P's (block 0) or A's (block 1) entries into K's device store: src_dev holds the whole block in the
// caller's nzval order; idx_dev == nullptr: all k entries, else only the k entries idx_dev[0 .. k) (duplicates allowed).
// Enqueued on the handle's stream.  K's host mirror (chip_kkt_get_matrix) is not touched.
int kkt_update_values_dev(::chip_kkt *h, int block, const double *src_dev, const int64_t *idx_dev, int k);
// the max |P_ii| the static regulariser reads (chip_kkt_update_P computes it from the host mirror)
void kkt_set_static_diag_max(::chip_kkt *h, double v);
// L3: the mirrors of P and A (full re-gather from device arrays in the caller's nzval order), q with -q, and b from
// device vectors; any pointer may be nullptr.  Enqueued on the handle's stream.
int kktsystem_update_data_dev(::chip_kktsystem *h, const double *P_dev, const double *A_dev, const double *q_dev,
                              const double *b_dev);

} // namespace chip
