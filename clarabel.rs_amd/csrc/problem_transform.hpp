// problem_transform.hpp -- presolve and chordal decomposition of the L4 solver's problem (default/presolver.rs,
// src/solver/chordal/): the host transform built at setup, its reverse maps, the PSD completion, and the launcher of
// the device reverse (problem_transform.hip).  Internal to the library.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/clarabel_hip.h"

namespace chip {

enum { MERGE_NONE = 0, MERGE_PARENT_CHILD = 1, MERGE_CLIQUE_GRAPH = 2 };

// reverse-map modes of one original row
enum { RV_CONST = 0,    // removed by presolve: s = 1e20, z = 0
       RV_COPY = 1,     // one source, copied
       RV_COMPACT = 2,  // s = +0.0 + the sources in order, z = the last source (0 without one)
       RV_STANDARD = 3  // s = +0.0 + the sources, z = the same sum divided by the count when it exceeds 1
};

struct TransformOptions {
    bool presolve = false, chordal = false, compact = true, complete_dual = true;
    int merge = MERGE_CLIQUE_GRAPH;
};

// the five transform fields of chip_solver_settings
TransformOptions transform_options(const chip_solver_settings &st);

// one decomposed PSDTriangle cone.  Internal vertex v stands for original vertex ordering[v]; cliques are listed in
// post order (the last one is the root), clique k = snode k (the consecutive internal vertices
// [snode_start[k], snode_start[k] + snode_len[k])) followed by its separator sep[k] (internal vertices, sorted)
struct CliquePattern {
    int64_t cone = 0;       // index among the presolved problem's cones
    int64_t row_orig = 0;   // first row of the cone in the ORIGINAL problem
    int64_t row_pre = 0;    // the same in the presolved problem
    int64_t side = 0;
    int64_t premerge_cliques = 0;
    std::vector<int64_t> ordering, snode_start, snode_len, parent;
    std::vector<std::vector<int64_t>> sep;
    int64_t ncliques() const { return (int64_t)snode_start.size(); }
    int64_t nblk(int64_t k) const { return snode_len[k] + (int64_t)sep[k].size(); }
    // the clique's vertices in ORIGINAL labels, sorted
    std::vector<int64_t> clique_orig(int64_t k) const;
};

struct ProblemTransform {
    TransformOptions opt;
    int64_t n = 0, m = 0;             // original sizes
    int64_t m_reduced = 0;            // after presolve
    bool presolved = false;           // a row was removed
    std::vector<uint8_t> keep;        // presolve: keep[i] for each original row (when presolved)
    std::vector<CliquePattern> patterns;
    // the problem the solver runs on
    int64_t n2 = 0, m2 = 0;
    std::vector<uint64_t> Pp, Pi, Ap, Ai;
    std::vector<double> Px, q, Ax, b;
    std::vector<int32_t> tags;
    std::vector<int64_t> dims, dims2;
    std::vector<double> alphas;
    // standard form: H (one entry per column: the original row of column c is H_row[c]; -1 none)
    std::vector<int64_t> H_row;
    // the reverse: per original row i, mode[i] and the internal rows src[ptr[i] .. ptr[i+1])
    std::vector<int32_t> mode;
    std::vector<int64_t> ptr, src;
    int64_t premerge_added = 0, final_added = 0, largest_clique = 0;
    double transform_time = 0;

    bool decomposed() const { return !patterns.empty(); }
    bool active() const { return presolved || decomposed(); }
};

// builds the transform of (P, q, A, b, cones) (P triu CSC, A CSC, cones as chip_solver_create).  Returns 0, or a
// negative chip_status with the error set.  When nothing is removed nor decomposed, out.active() is false and the
// transformed arrays are left empty.
int transform_build(int64_t n, int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval, const double *Pnzval,
                    const double *q, const uint64_t *Acolptr, const uint64_t *Arowval, const double *Anzval,
                    const double *b, int64_t ncones, const int32_t *tags, const int64_t *dims, const int64_t *dims2,
                    const double *alphas_or_null, const TransformOptions &opt, ProblemTransform &out);

// the reverse on the host from already-unscaled internal vectors: x[n], s[m], z[m] of the original problem
void transform_reverse_host(const ProblemTransform &t, const double *x2, const double *s2, const double *z2, double *x,
                            double *s, double *z);

// psd_completion (psd_completion.rs): completes z (original-sized) over every decomposed cone in place
void transform_complete_dual(const ProblemTransform &t, double *z);

namespace dev {
// the reverse on the device from the SCALED internal variables, with the arithmetic of dev::unscale per source:
// (stream: a hipStream_t; this header is also read by host-only translation units)
// x[i] = (x2[i] * d[i]) * sx; source k of s: (s2[k] * einv[k]) * ss; source k of z: (z2[k] * e[k]) * sz
struct RvMaps {
    const int32_t *mode;
    const int64_t *ptr, *src;
};
void transform_reverse(void *stream, const RvMaps &mp, int n, int m, double *xo, const double *x2, const double *d,
                       double sx, double *so, const double *s2, const double *einv, double ss, double *zo,
                       const double *z2, const double *e, double sz);
} // namespace dev

} // namespace chip
