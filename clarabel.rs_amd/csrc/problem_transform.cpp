// problem_transform.cpp -- the L4 solver's problem transforms, built once at setup on the host:
//   presolve              default/presolver.rs: Nonnegative rows whose b exceeds (1 - 10 eps) * 1e20 are dropped,
//                         an emptied Nonnegative cone disappears;
//   chordal decomposition src/solver/chordal/: the aggregate sparsity pattern of each PSDTriangle cone of side > 3
//                         in [A b], a chordal extension from a minimum-degree elimination (amd_order.cpp), the
//                         fundamental supernodes and their cliques, one of three clique-merge strategies, and the
//                         compact (augment_compact.rs) or standard (augment_standard.rs) augmentation;
//   the reverse           per original row, the internal rows it is gathered from (decomp_reverse + reverse_presolve
//                         composed into one map), and the PSD completion of the dual (psd_completion.rs).
// Unlike the reference, the chordal analysis runs on the PRESOLVED problem, so that the two steps compose when
// presolve removes a row in front of a decomposable cone.
#include "problem_transform.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <map>
#include <numeric>
#include <set>

#include "../../include/clarabel_hip.h"
#include "host.hpp"

namespace chip {

namespace {

using Set = std::vector<int64_t>; // sorted vertex sets

inline int64_t tri(int64_t k) { return k * (k + 1) / 2; }
inline int64_t triu_index(int64_t r, int64_t c) { return tri(c) + r; } // r <= c, column-major upper triangle

int64_t cone_numel(int32_t tag, int64_t dim, int64_t dim2) {
    switch (tag) {
    case CHIP_CONE_EXPONENTIAL:
    case CHIP_CONE_POWER: return 3;
    case CHIP_CONE_GENPOWER: return dim + dim2;
    case CHIP_CONE_PSDTRIANGLE: return tri(dim);
    default: return dim;
    }
}

Set set_union(const Set &a, const Set &b) {
    Set o;
    o.reserve(a.size() + b.size());
    std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(o));
    return o;
}
Set set_inter(const Set &a, const Set &b) {
    Set o;
    std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(o));
    return o;
}
Set set_minus(const Set &a, const Set &b) {
    Set o;
    std::set_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(o));
    return o;
}
int64_t union_size(const Set &a, const Set &b) { return (int64_t)(a.size() + b.size() - set_inter(a, b).size()); }

// a clique tree under construction: cliques (sorted vertex sets; empty = merged away) and their parents (-1: root)
struct CliqueTree {
    std::vector<Set> C;
    std::vector<int64_t> parent;
};

// children lists and a post order (children before parents, children in index order) of a rooted forest
std::vector<int64_t> post_order(const std::vector<int64_t> &parent, const std::vector<uint8_t> &alive) {
    const int64_t k = (int64_t)parent.size();
    std::vector<std::vector<int64_t>> ch((size_t)k);
    std::vector<int64_t> roots;
    for (int64_t i = 0; i < k; i++) {
        if (!alive[i]) continue;
        if (parent[i] < 0) roots.push_back(i);
        else ch[parent[i]].push_back(i);
    }
    std::vector<int64_t> post;
    std::vector<std::pair<int64_t, size_t>> stack;
    for (int64_t r : roots) {
        stack.push_back({r, 0});
        while (!stack.empty()) {
            auto &top = stack.back();
            if (top.second < ch[top.first].size()) {
                const int64_t c = ch[top.first][top.second++];
                stack.push_back({c, 0});
            } else {
                post.push_back(top.first);
                stack.pop_back();
            }
        }
    }
    return post;
}

// ---- the chordal extension and its supernodal clique tree (sparsity_pattern.rs, supernode_tree.rs) ---------------
// graph: the mask over the upper triangle of an N x N matrix (diagonal set).  Returns the cliques over internal
// labels 0..N-1 (elimination order: label = position in the minimum-degree order) and perm (perm[label] = vertex).
int chordal_cliques(int64_t N, const std::vector<uint8_t> &mask, CliqueTree &T, std::vector<int64_t> &perm) {
    std::vector<i64> Ap((size_t)N + 1, 0), Ai;
    for (int64_t c = 0; c < N; c++) {
        for (int64_t r = 0; r <= c; r++)
            if (mask[(size_t)triu_index(r, c)]) Ai.push_back(r);
        Ap[(size_t)c + 1] = (i64)Ai.size();
    }
    AmdInfo info;
    std::vector<i64> p;
    if (amd_order(N, Ap.data(), Ai.data(), 1.0, p, &info)) return CHIP_ERR_BAD_PERM;
    perm.assign(p.begin(), p.end());
    std::vector<int64_t> pinv((size_t)N);
    for (int64_t k = 0; k < N; k++) pinv[(size_t)perm[k]] = k;
    // the higher neighbours of every label, then the column patterns of the logical Cholesky factor
    std::vector<Set> L((size_t)N);
    for (int64_t c = 0; c < N; c++)
        for (i64 k = Ap[c]; k < Ap[c + 1]; k++) {
            const int64_t r = Ai[k];
            if (r == c) continue;
            const int64_t a = pinv[(size_t)r], b2 = pinv[(size_t)c];
            L[(size_t)std::min(a, b2)].push_back(std::max(a, b2));
        }
    std::vector<int64_t> parent((size_t)N, -1);
    std::vector<std::vector<int64_t>> children((size_t)N);
    for (int64_t j = 0; j < N; j++) {
        Set &Lj = L[(size_t)j];
        std::sort(Lj.begin(), Lj.end());
        Lj.erase(std::unique(Lj.begin(), Lj.end()), Lj.end());
        for (int64_t c : children[(size_t)j]) {
            Set rest(std::upper_bound(L[(size_t)c].begin(), L[(size_t)c].end(), j), L[(size_t)c].end());
            Lj = set_union(Lj, rest);
        }
        // connect_graph: a column without a higher neighbour is linked to the next label, so the tree is connected
        if (Lj.empty() && j + 1 < N) Lj.push_back(j + 1);
        if (!Lj.empty()) {
            parent[(size_t)j] = Lj[0];
            children[(size_t)Lj[0]].push_back(j);
        }
    }
    // fundamental supernodes (Pothen & Sun): in post order, a parent joins its child's supernode when its column is
    // the child's minus the parent itself and no other child claimed it
    std::vector<uint8_t> all((size_t)N, 1);
    const std::vector<int64_t> post = post_order(parent, all);
    std::vector<int64_t> rep((size_t)N, -1); // supernode representative (its first vertex) of every vertex
    for (int64_t v : post) {
        if (rep[(size_t)v] < 0) rep[(size_t)v] = v;
        const int64_t p2 = parent[(size_t)v];
        if (p2 >= 0 && rep[(size_t)p2] < 0 && L[(size_t)v].size() == L[(size_t)p2].size() + 1)
            rep[(size_t)p2] = rep[(size_t)v];
    }
    std::vector<int64_t> sn_of((size_t)N, -1);
    T.C.clear();
    for (int64_t v = 0; v < N; v++) {
        const int64_t r = rep[(size_t)v];
        if (r == v) {
            sn_of[(size_t)v] = (int64_t)T.C.size();
            Set c{v};
            c.insert(c.end(), L[(size_t)v].begin(), L[(size_t)v].end());
            T.C.push_back(c);
        }
        sn_of[(size_t)v] = sn_of[(size_t)r];
    }
    T.parent.assign(T.C.size(), -1);
    // the parent of a supernode: the supernode of the elimination-tree parent of its last vertex
    for (int64_t v = 0; v < N; v++) {
        const int64_t p2 = parent[(size_t)v];
        if (p2 >= 0 && sn_of[(size_t)p2] != sn_of[(size_t)v]) T.parent[(size_t)sn_of[(size_t)v]] = sn_of[(size_t)p2];
    }
    return 0;
}

// ---- merge strategies (merge/) -----------------------------------------------------------------------------------
// parent_child.rs: in descending post order, a clique merges into its parent when the fill-in is at most 8 or both
// supernodes have at most 8 vertices
void merge_parent_child(CliqueTree &T) {
    const int64_t k = (int64_t)T.C.size();
    std::vector<uint8_t> alive((size_t)k, 1);
    const std::vector<int64_t> post = post_order(T.parent, alive);
    auto snode_size = [&](int64_t c) {
        const int64_t p = T.parent[(size_t)c];
        return (int64_t)T.C[(size_t)c].size() - (p < 0 ? 0 : (int64_t)set_inter(T.C[(size_t)c], T.C[(size_t)p]).size());
    };
    for (int64_t idx = (int64_t)post.size() - 2; idx >= 0; idx--) {
        const int64_t c = post[(size_t)idx], p = T.parent[(size_t)c];
        if (p < 0) continue;
        const int64_t sep = (int64_t)set_inter(T.C[(size_t)c], T.C[(size_t)p]).size();
        const int64_t fill = ((int64_t)T.C[(size_t)p].size() - sep) * ((int64_t)T.C[(size_t)c].size() - sep);
        const int64_t max_snode = std::max(snode_size(c), snode_size(p));
        if (fill <= 8 || max_snode <= 8) {
            T.C[(size_t)p] = set_union(T.C[(size_t)p], T.C[(size_t)c]);
            T.C[(size_t)c].clear();
            alive[(size_t)c] = 0;
            for (int64_t j = 0; j < k; j++)
                if (T.parent[(size_t)j] == c) T.parent[(size_t)j] = p;
        }
    }
}

// clique_graph.rs: the cliques joined by the edges of the clique graph whose intersection is a separator of the
// clique tree; repeatedly the permissible edge of largest weight |Ci|^3 + |Cj|^3 - |Ci u Cj|^3 is merged while that
// weight is >= 0 (permissible: every common neighbour meets both cliques in the same set); the clique tree is then
// rebuilt as a maximum-weight spanning tree (weight |Ci n Cj|, Kruskal with a disjoint-set union)
void merge_clique_graph(CliqueTree &T) {
    const int64_t k = (int64_t)T.C.size();
    std::set<Set> separators;
    for (int64_t c = 0; c < k; c++)
        if (T.parent[(size_t)c] >= 0) separators.insert(set_inter(T.C[(size_t)c], T.C[(size_t)T.parent[(size_t)c]]));
    int64_t nv = 0;
    for (const Set &c : T.C)
        if (!c.empty()) nv = std::max(nv, c.back() + 1);
    std::vector<std::vector<int64_t>> of_vertex((size_t)nv);
    for (int64_t c = 0; c < k; c++)
        for (int64_t v : T.C[(size_t)c]) of_vertex[(size_t)v].push_back(c);
    std::vector<std::set<int64_t>> adj((size_t)k);
    for (const auto &cl : of_vertex)
        for (size_t a = 0; a < cl.size(); a++)
            for (size_t b = a + 1; b < cl.size(); b++) {
                const int64_t i = cl[a], j = cl[b];
                if (adj[(size_t)i].count(j)) continue;
                if (separators.count(set_inter(T.C[(size_t)i], T.C[(size_t)j]))) {
                    adj[(size_t)i].insert(j);
                    adj[(size_t)j].insert(i);
                }
            }
    auto cube = [](int64_t x) { return x * x * x; };
    auto weight = [&](int64_t i, int64_t j) {
        return cube((int64_t)T.C[(size_t)i].size()) + cube((int64_t)T.C[(size_t)j].size()) -
               cube(union_size(T.C[(size_t)i], T.C[(size_t)j]));
    };
    std::map<std::pair<int64_t, int64_t>, int64_t> w; // i < j
    for (int64_t i = 0; i < k; i++)
        for (int64_t j : adj[(size_t)i])
            if (i < j) w[{i, j}] = weight(i, j);
    auto permissible = [&](int64_t i, int64_t j) {
        for (int64_t nb : adj[(size_t)i]) {
            if (nb == j || !adj[(size_t)j].count(nb)) continue;
            if (set_inter(T.C[(size_t)i], T.C[(size_t)nb]) != set_inter(T.C[(size_t)j], T.C[(size_t)nb])) return false;
        }
        return true;
    };
    while (!w.empty()) {
        std::vector<std::pair<int64_t, std::pair<int64_t, int64_t>>> order;
        order.reserve(w.size());
        for (const auto &kv : w) order.push_back({kv.second, kv.first});
        // largest weight first; ties: the smaller pair
        std::stable_sort(order.begin(), order.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
        int64_t ci = -1, cj = -1;
        for (const auto &o : order) {
            if (o.first < 0) break;
            if (permissible(o.second.first, o.second.second)) {
                ci = o.second.first;
                cj = o.second.second;
                break;
            }
        }
        if (ci < 0) break;
        // merge cj into ci; cj's edges move to ci
        T.C[(size_t)ci] = set_union(T.C[(size_t)ci], T.C[(size_t)cj]);
        T.C[(size_t)cj].clear();
        for (int64_t nb : adj[(size_t)cj]) {
            w.erase({std::min(nb, cj), std::max(nb, cj)});
            adj[(size_t)nb].erase(cj);
            if (nb != ci) {
                adj[(size_t)nb].insert(ci);
                adj[(size_t)ci].insert(nb);
            }
        }
        adj[(size_t)cj].clear();
        for (int64_t nb : adj[(size_t)ci]) w[{std::min(nb, ci), std::max(nb, ci)}] = weight(ci, nb);
    }
    // the clique tree: maximum-weight spanning tree of what is left of the graph
    std::vector<std::pair<int64_t, std::pair<int64_t, int64_t>>> edges;
    for (int64_t i = 0; i < k; i++)
        for (int64_t j : adj[(size_t)i])
            if (i < j) edges.push_back({(int64_t)set_inter(T.C[(size_t)i], T.C[(size_t)j]).size(), {i, j}});
    std::stable_sort(edges.begin(), edges.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    std::vector<int64_t> dsu((size_t)k);
    std::iota(dsu.begin(), dsu.end(), 0);
    auto find = [&](int64_t x) {
        while (dsu[(size_t)x] != x) x = dsu[(size_t)x] = dsu[(size_t)dsu[(size_t)x]];
        return x;
    };
    std::vector<std::vector<int64_t>> tadj((size_t)k);
    for (const auto &e : edges) {
        const int64_t a = find(e.second.first), b = find(e.second.second);
        if (a == b) continue;
        dsu[(size_t)a] = b;
        tadj[(size_t)e.second.first].push_back(e.second.second);
        tadj[(size_t)e.second.second].push_back(e.second.first);
    }
    // root: the clique holding the last vertex; components left apart hang below it with an empty separator
    int64_t root = -1;
    for (int64_t c = 0; c < k; c++)
        if (!T.C[(size_t)c].empty() && (root < 0 || T.C[(size_t)c].back() > T.C[(size_t)root].back())) root = c;
    T.parent.assign((size_t)k, -1);
    std::vector<uint8_t> seen((size_t)k, 0);
    auto bfs = [&](int64_t r) {
        std::vector<int64_t> q{r};
        seen[(size_t)r] = 1;
        for (size_t h = 0; h < q.size(); h++)
            for (int64_t nb : tadj[(size_t)q[h]])
                if (!seen[(size_t)nb]) {
                    seen[(size_t)nb] = 1;
                    T.parent[(size_t)nb] = q[h];
                    q.push_back(nb);
                }
    };
    if (root >= 0) bfs(root);
    for (int64_t c = 0; c < k; c++)
        if (!T.C[(size_t)c].empty() && !seen[(size_t)c]) {
            bfs(c);
            T.parent[(size_t)c] = root;
        }
}

// reorder_snode_consecutively + calculate_block_dimensions: the live cliques in post order, snode = clique minus its
// parent, the vertices relabelled so that every snode is a consecutive range
void finalize(const CliqueTree &T, const std::vector<int64_t> &perm, CliquePattern &pat) {
    const int64_t k = (int64_t)T.C.size();
    std::vector<uint8_t> alive((size_t)k);
    for (int64_t c = 0; c < k; c++) alive[(size_t)c] = !T.C[(size_t)c].empty();
    const std::vector<int64_t> post = post_order(T.parent, alive);
    std::vector<int64_t> pos((size_t)k, -1);
    for (size_t i = 0; i < post.size(); i++) pos[(size_t)post[i]] = (int64_t)i;
    const int64_t N = (int64_t)perm.size();
    std::vector<int64_t> relabel((size_t)N, -1);
    std::vector<Set> seps;
    int64_t next = 0;
    pat.snode_start.clear();
    pat.snode_len.clear();
    pat.parent.clear();
    for (int64_t c : post) {
        const int64_t p = T.parent[(size_t)c];
        const Set sep = p < 0 ? Set{} : set_inter(T.C[(size_t)c], T.C[(size_t)p]);
        const Set sn = set_minus(T.C[(size_t)c], sep);
        pat.snode_start.push_back(next);
        pat.snode_len.push_back((int64_t)sn.size());
        pat.parent.push_back(p < 0 ? -1 : pos[(size_t)p]);
        for (int64_t v : sn) relabel[(size_t)v] = next++;
        seps.push_back(sep);
    }
    pat.sep.clear();
    for (const Set &s : seps) {
        Set r;
        for (int64_t v : s) r.push_back(relabel[(size_t)v]);
        std::sort(r.begin(), r.end());
        pat.sep.push_back(r);
    }
    pat.ordering.assign((size_t)N, 0);
    for (int64_t v = 0; v < N; v++) pat.ordering[(size_t)relabel[(size_t)v]] = perm[(size_t)v];
}

struct Triplet {
    int64_t row, col;
    double v;
};

void to_csc(int64_t ncols, std::vector<Triplet> &t, std::vector<uint64_t> &cp, std::vector<uint64_t> &ri,
            std::vector<double> &vx) {
    std::stable_sort(t.begin(), t.end(), [](const Triplet &a, const Triplet &b) {
        return a.col != b.col ? a.col < b.col : a.row < b.row;
    });
    cp.assign((size_t)ncols + 1, 0);
    ri.resize(t.size());
    vx.resize(t.size());
    for (size_t k = 0; k < t.size(); k++) {
        cp[(size_t)t[k].col + 1]++;
        ri[k] = (uint64_t)t[k].row;
        vx[k] = t[k].v;
    }
    for (int64_t j = 0; j < ncols; j++) cp[(size_t)j + 1] += cp[(size_t)j];
}

} // namespace

TransformOptions transform_options(const chip_solver_settings &st) {
    TransformOptions o;
    o.presolve = st.presolve_enable != 0;
    o.chordal = st.chordal_decomposition_enable != 0;
    o.merge = st.chordal_decomposition_merge_method;
    o.compact = st.chordal_decomposition_compact != 0;
    o.complete_dual = st.chordal_decomposition_complete_dual != 0;
    return o;
}

std::vector<int64_t> CliquePattern::clique_orig(int64_t k) const {
    std::vector<int64_t> c;
    for (int64_t v = snode_start[k]; v < snode_start[k] + snode_len[k]; v++) c.push_back(ordering[(size_t)v]);
    for (int64_t v : sep[k]) c.push_back(ordering[(size_t)v]);
    std::sort(c.begin(), c.end());
    return c;
}

int transform_build(int64_t n, int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval, const double *Pnzval,
                    const double *q, const uint64_t *Acolptr, const uint64_t *Arowval, const double *Anzval,
                    const double *b, int64_t ncones, const int32_t *tags, const int64_t *dims, const int64_t *dims2,
                    const double *alphas_or_null, const TransformOptions &opt, ProblemTransform &out) {
    const double t0 = now_s();
    out = ProblemTransform();
    if (opt.merge < MERGE_NONE || opt.merge > MERGE_CLIQUE_GRAPH) {
        set_error("problem transform: unknown chordal_decomposition_merge_method");
        return CHIP_ERR_ARG;
    }
    out.opt = opt;
    out.n = n;
    out.m = m;
    out.m_reduced = m;
    // ---- presolve (make_reduction_map): Nonnegative rows with an "infinite" b
    std::vector<int64_t> start((size_t)ncones + 1, 0);
    for (int64_t c = 0; c < ncones; c++)
        start[(size_t)c + 1] = start[(size_t)c] + cone_numel(tags[c], dims[c], dims2 ? dims2[c] : 0);
    if (start[(size_t)ncones] != m) {
        set_error("problem transform: cone dimensions do not add up to m");
        return CHIP_ERR_DIM;
    }
    std::vector<uint8_t> keep((size_t)m, 1);
    if (opt.presolve) {
        const double infbound = (1.0 - std::numeric_limits<double>::epsilon() * 10.0) * 1e20;
        for (int64_t c = 0; c < ncones; c++)
            if (tags[c] == CHIP_CONE_NONNEGATIVE)
                for (int64_t i = start[(size_t)c]; i < start[(size_t)c + 1]; i++)
                    if (b[i] > infbound) {
                        keep[(size_t)i] = 0;
                        out.m_reduced--;
                    }
        out.presolved = out.m_reduced < m;
    }
    std::vector<int64_t> pre_of((size_t)m, -1); // original row -> presolved row
    {
        int64_t r = 0;
        for (int64_t i = 0; i < m; i++)
            if (keep[(size_t)i]) pre_of[(size_t)i] = r++;
    }
    const int64_t m1 = out.m_reduced;
    // the presolved cones (cone index map, first rows) and b
    std::vector<int32_t> tg1;
    std::vector<int64_t> d1, d21, orig_cone1, start1;
    std::vector<double> al1;
    for (int64_t c = 0; c < ncones; c++) {
        int64_t dim = dims[c];
        if (tags[c] == CHIP_CONE_NONNEGATIVE) {
            dim = 0;
            for (int64_t i = start[(size_t)c]; i < start[(size_t)c + 1]; i++) dim += keep[(size_t)i];
            if (dim == 0 && dims[c] > 0) continue; // an emptied Nonnegative cone disappears
        }
        tg1.push_back(tags[c]);
        d1.push_back(dim);
        d21.push_back(dims2 ? dims2[c] : 0);
        al1.push_back(alphas_or_null ? alphas_or_null[c] : 0.5);
        orig_cone1.push_back(c);
    }
    start1.assign(tg1.size() + 1, 0);
    for (size_t c = 0; c < tg1.size(); c++) start1[c + 1] = start1[c] + cone_numel(tg1[c], d1[c], d21[c]);
    std::vector<double> b1((size_t)m1);
    for (int64_t i = 0; i < m; i++)
        if (keep[(size_t)i]) b1[(size_t)pre_of[(size_t)i]] = b[i];
    // A by rows of the presolved problem: (col, value) lists in column order
    std::vector<std::vector<std::pair<int64_t, double>>> arow((size_t)m1);
    for (int64_t j = 0; j < n; j++)
        for (uint64_t k = Acolptr[j]; k < Acolptr[j + 1]; k++) {
            const int64_t r = pre_of[(size_t)Arowval[k]];
            if (r >= 0) arow[(size_t)r].push_back({j, Anzval[k]});
        }
    // ---- chordal analysis on the presolved problem (chordal_info.rs)
    if (opt.chordal) {
        std::vector<uint8_t> active((size_t)m1, 0);
        for (int64_t r = 0; r < m1; r++) active[(size_t)r] = !arow[(size_t)r].empty() || b1[(size_t)r] != 0.0;
        for (size_t c = 0; c < tg1.size(); c++) {
            if (tg1[c] != CHIP_CONE_PSDTRIANGLE || d1[c] <= 3) continue;
            const int64_t N = d1[c];
            std::vector<uint8_t> mask(active.begin() + start1[c], active.begin() + start1[c + 1]);
            for (int64_t i = 0; i < N; i++) mask[(size_t)triu_index(i, i)] = 1;
            if (std::all_of(mask.begin(), mask.end(), [](uint8_t x) { return x != 0; })) continue; // dense
            CliqueTree T;
            std::vector<int64_t> perm;
            int rc = chordal_cliques(N, mask, T, perm);
            if (rc) return rc;
            CliquePattern pat;
            pat.premerge_cliques = (int64_t)T.C.size();
            if (T.C.size() > 1) {
                if (opt.merge == MERGE_PARENT_CHILD) merge_parent_child(T);
                else if (opt.merge == MERGE_CLIQUE_GRAPH) merge_clique_graph(T);
            }
            finalize(T, perm, pat);
            if (pat.ncliques() <= 1) continue; // not decomposed, or merged back into one
            pat.cone = (int64_t)c;
            pat.side = N;
            pat.row_pre = start1[c];
            pat.row_orig = start[(size_t)orig_cone1[c]];
            out.premerge_added += pat.premerge_cliques - 1;
            out.final_added += pat.ncliques() - 1;
            for (int64_t k = 0; k < pat.ncliques(); k++) out.largest_clique = std::max(out.largest_clique, pat.nblk(k));
            out.patterns.push_back(std::move(pat));
        }
    }
    if (!out.active()) {
        out.transform_time = now_s() - t0;
        return CHIP_OK;
    }
    out.keep = keep;
    // ---- augmentation.  rows_of[r]: the internal rows that presolved row r is gathered from, in reverse order
    std::vector<std::vector<int64_t>> rows_of((size_t)m1);
    std::vector<int32_t> mode_pre((size_t)m1, RV_COPY);
    std::vector<Triplet> At;
    std::vector<double> b2;
    auto pattern_for = [&](size_t c) -> const CliquePattern * {
        for (const CliquePattern &p : out.patterns)
            if (p.cone == (int64_t)c) return &p;
        return nullptr;
    };
    int64_t nadd = 0;
    if (!out.decomposed()) { // presolve alone
        for (int64_t r = 0; r < m1; r++) {
            for (const auto &e : arow[(size_t)r]) At.push_back({r, e.first, e.second});
            rows_of[(size_t)r].push_back(r);
        }
        b2 = b1;
        for (size_t c = 0; c < tg1.size(); c++) {
            out.tags.push_back(tg1[c]);
            out.dims.push_back(d1[c]);
            out.dims2.push_back(d21[c]);
            out.alphas.push_back(al1[c]);
        }
        out.m2 = m1;
    } else if (opt.compact) { // augment_compact.rs
        int64_t row = 0;
        for (size_t c = 0; c < tg1.size(); c++) {
            const CliquePattern *p = pattern_for(c);
            const int64_t r0 = start1[c];
            if (!p) {
                for (int64_t r = r0; r < start1[c + 1]; r++) {
                    for (const auto &e : arow[(size_t)r]) At.push_back({row + r - r0, e.first, e.second});
                    b2.push_back(b1[(size_t)r]);
                    rows_of[(size_t)r].push_back(row + r - r0);
                }
                out.tags.push_back(tg1[c]);
                out.dims.push_back(d1[c]);
                out.dims2.push_back(d21[c]);
                out.alphas.push_back(al1[c]);
                row += start1[c + 1] - r0;
                continue;
            }
            for (int64_t r = r0; r < start1[c + 1]; r++) mode_pre[(size_t)r] = RV_COMPACT;
            // the cliques root first; the rows of each clique in column-major upper-triangle order of its sorted
            // original vertices
            const int64_t K = p->ncliques();
            std::vector<int64_t> crow((size_t)K);
            {
                int64_t rr = row;
                for (int64_t k = K - 1; k >= 0; k--) {
                    crow[(size_t)k] = rr;
                    rr += tri(p->nblk(k));
                }
            }
            for (int64_t k = K - 1; k >= 0; k--) {
                const std::vector<int64_t> vo = p->clique_orig(k);
                std::vector<uint8_t> in_sep(vo.size(), 0);
                std::vector<int64_t> sep_o;
                for (int64_t v : p->sep[(size_t)k]) sep_o.push_back(p->ordering[(size_t)v]);
                std::sort(sep_o.begin(), sep_o.end());
                for (size_t a = 0; a < vo.size(); a++) in_sep[a] = std::binary_search(sep_o.begin(), sep_o.end(), vo[a]);
                std::vector<int64_t> par;
                if (p->parent[(size_t)k] >= 0) par = p->clique_orig(p->parent[(size_t)k]);
                int64_t cnt = 0;
                for (size_t jb = 0; jb < vo.size(); jb++)
                    for (size_t ia = 0; ia <= jb; ia++, cnt++) {
                        const int64_t nr = crow[(size_t)k] + cnt;
                        const int64_t pr = r0 + triu_index(vo[ia], vo[jb]);
                        rows_of[(size_t)pr].push_back(nr);
                        if (in_sep[ia] && in_sep[jb]) { // an overlap: +y here, -y in the parent's entry
                            const int64_t pi = std::lower_bound(par.begin(), par.end(), vo[ia]) - par.begin();
                            const int64_t pj = std::lower_bound(par.begin(), par.end(), vo[jb]) - par.begin();
                            At.push_back({nr, n + nadd, 1.0});
                            At.push_back({crow[(size_t)p->parent[(size_t)k]] + triu_index(pi, pj), n + nadd, -1.0});
                            nadd++;
                        } else {
                            for (const auto &e : arow[(size_t)pr]) At.push_back({nr, e.first, e.second});
                        }
                    }
                out.tags.push_back(CHIP_CONE_PSDTRIANGLE);
                out.dims.push_back(p->nblk(k));
                out.dims2.push_back(0);
                out.alphas.push_back(0.5);
            }
            // b: the non-overlap entries take b of their original row
            b2.resize((size_t)(crow[0] + tri(p->nblk(0))), 0.0);
            for (int64_t k = K - 1; k >= 0; k--) {
                const std::vector<int64_t> vo = p->clique_orig(k);
                std::vector<int64_t> sep_o;
                for (int64_t v : p->sep[(size_t)k]) sep_o.push_back(p->ordering[(size_t)v]);
                std::sort(sep_o.begin(), sep_o.end());
                int64_t cnt = 0;
                for (size_t jb = 0; jb < vo.size(); jb++)
                    for (size_t ia = 0; ia <= jb; ia++, cnt++) {
                        const bool ov = std::binary_search(sep_o.begin(), sep_o.end(), vo[ia]) &&
                                        std::binary_search(sep_o.begin(), sep_o.end(), vo[jb]);
                        if (!ov) b2[(size_t)(crow[(size_t)k] + cnt)] = b1[(size_t)(r0 + triu_index(vo[ia], vo[jb]))];
                    }
            }
            row = crow[0] + tri(p->nblk(0));
        }
        out.m2 = row;
    } else { // augment_standard.rs: [A H; 0 -I], a zero cone over the presolved rows
        std::vector<int64_t> Hrow;
        for (size_t c = 0; c < tg1.size(); c++) {
            const CliquePattern *p = pattern_for(c);
            const int64_t r0 = start1[c];
            if (!p) {
                for (int64_t r = r0; r < start1[c + 1]; r++) Hrow.push_back(r);
                continue;
            }
            for (int64_t k = 0; k < p->ncliques(); k++) {
                const std::vector<int64_t> vo = p->clique_orig(k);
                for (size_t jb = 0; jb < vo.size(); jb++)
                    for (size_t ia = 0; ia <= jb; ia++) Hrow.push_back(r0 + triu_index(vo[ia], vo[jb]));
            }
        }
        nadd = (int64_t)Hrow.size();
        for (int64_t r = 0; r < m1; r++) {
            for (const auto &e : arow[(size_t)r]) At.push_back({r, e.first, e.second});
            mode_pre[(size_t)r] = RV_STANDARD;
        }
        for (int64_t c2 = 0; c2 < nadd; c2++) {
            At.push_back({Hrow[(size_t)c2], n + c2, 1.0});
            At.push_back({m1 + c2, n + c2, -1.0});
            rows_of[(size_t)Hrow[(size_t)c2]].push_back(m1 + c2);
        }
        b2 = b1;
        b2.resize((size_t)(m1 + nadd), 0.0);
        out.tags.push_back(CHIP_CONE_ZERO);
        out.dims.push_back(m1);
        out.dims2.push_back(0);
        out.alphas.push_back(0.5);
        for (size_t c = 0; c < tg1.size(); c++) {
            const CliquePattern *p = pattern_for(c);
            if (!p) {
                out.tags.push_back(tg1[c]);
                out.dims.push_back(d1[c]);
                out.dims2.push_back(d21[c]);
                out.alphas.push_back(al1[c]);
                continue;
            }
            for (int64_t k = 0; k < p->ncliques(); k++) {
                out.tags.push_back(CHIP_CONE_PSDTRIANGLE);
                out.dims.push_back(p->nblk(k));
                out.dims2.push_back(0);
                out.alphas.push_back(0.5);
            }
        }
        out.H_row = Hrow;
        out.m2 = m1 + nadd;
    }
    out.n2 = n + nadd;
    // P' = blockdiag(P, 0), q' = [q; 0]
    out.Pp.assign(Pcolptr, Pcolptr + n + 1);
    out.Pp.resize((size_t)out.n2 + 1, Pcolptr[n]);
    out.Pi.assign(Prowval, Prowval + Pcolptr[n]);
    out.Px.assign(Pnzval, Pnzval + Pcolptr[n]);
    out.q.assign(q, q + n);
    out.q.resize((size_t)out.n2, 0.0);
    to_csc(out.n2, At, out.Ap, out.Ai, out.Ax);
    out.b = b2;
    // ---- the reverse maps over the original rows
    out.mode.assign((size_t)m, RV_CONST);
    out.ptr.assign((size_t)m + 1, 0);
    for (int64_t i = 0; i < m; i++) {
        const int64_t r = pre_of[(size_t)i];
        if (r >= 0) {
            out.mode[(size_t)i] = mode_pre[(size_t)r];
            out.src.insert(out.src.end(), rows_of[(size_t)r].begin(), rows_of[(size_t)r].end());
        }
        out.ptr[(size_t)i + 1] = (int64_t)out.src.size();
    }
    out.transform_time = now_s() - t0;
    return CHIP_OK;
}

void transform_reverse_host(const ProblemTransform &t, const double *x2, const double *s2, const double *z2, double *x,
                            double *s, double *z) {
    for (int64_t i = 0; i < t.n; i++) x[i] = x2[i];
    for (int64_t i = 0; i < t.m; i++) {
        const int64_t a = t.ptr[(size_t)i], e = t.ptr[(size_t)i + 1];
        switch (t.mode[(size_t)i]) {
        case RV_CONST:
            s[i] = 1e20;
            z[i] = 0.0;
            break;
        case RV_COPY:
            s[i] = s2[t.src[(size_t)a]];
            z[i] = z2[t.src[(size_t)a]];
            break;
        case RV_COMPACT: {
            double ss = 0.0, zz = 0.0;
            for (int64_t k = a; k < e; k++) {
                ss += s2[t.src[(size_t)k]];
                zz = z2[t.src[(size_t)k]];
            }
            s[i] = ss;
            z[i] = zz;
            break;
        }
        default: {
            double ss = 0.0, zz = 0.0;
            for (int64_t k = a; k < e; k++) {
                ss += s2[t.src[(size_t)k]];
                zz += z2[t.src[(size_t)k]];
            }
            if (e - a > 1) zz /= (double)(e - a);
            s[i] = ss;
            z[i] = zz;
        }
        }
    }
}

// ---- psd_completion.rs --------------------------------------------------------------------------------------------
namespace {

// y <- A^{-1} y for symmetric A (n x n, row-major) and Y with ncol columns: Cholesky, or when that fails a
// pseudo-inverse from a Jacobi eigendecomposition
void spd_solve(std::vector<double> A, int64_t n, std::vector<double> &Y, int64_t ncol) {
    std::vector<double> Lm = A;
    bool ok = true;
    for (int64_t j = 0; j < n && ok; j++) {
        double d = Lm[(size_t)(j * n + j)];
        for (int64_t k = 0; k < j; k++) d -= Lm[(size_t)(j * n + k)] * Lm[(size_t)(j * n + k)];
        if (!(d > 0.0)) {
            ok = false;
            break;
        }
        d = std::sqrt(d);
        Lm[(size_t)(j * n + j)] = d;
        for (int64_t i = j + 1; i < n; i++) {
            double v = Lm[(size_t)(i * n + j)];
            for (int64_t k = 0; k < j; k++) v -= Lm[(size_t)(i * n + k)] * Lm[(size_t)(j * n + k)];
            Lm[(size_t)(i * n + j)] = v / d;
        }
    }
    if (ok) {
        for (int64_t c = 0; c < ncol; c++) {
            for (int64_t i = 0; i < n; i++) {
                double v = Y[(size_t)(i * ncol + c)];
                for (int64_t k = 0; k < i; k++) v -= Lm[(size_t)(i * n + k)] * Y[(size_t)(k * ncol + c)];
                Y[(size_t)(i * ncol + c)] = v / Lm[(size_t)(i * n + i)];
            }
            for (int64_t i = n - 1; i >= 0; i--) {
                double v = Y[(size_t)(i * ncol + c)];
                for (int64_t k = i + 1; k < n; k++) v -= Lm[(size_t)(k * n + i)] * Y[(size_t)(k * ncol + c)];
                Y[(size_t)(i * ncol + c)] = v / Lm[(size_t)(i * n + i)];
            }
        }
        return;
    }
    // cyclic Jacobi: A = V diag(w) V'
    std::vector<double> V((size_t)(n * n), 0.0);
    for (int64_t i = 0; i < n; i++) V[(size_t)(i * n + i)] = 1.0;
    for (int sweep = 0; sweep < 100; sweep++) {
        double off = 0.0;
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = i + 1; j < n; j++) off += A[(size_t)(i * n + j)] * A[(size_t)(i * n + j)];
        if (off < 1e-30) break;
        for (int64_t p = 0; p < n; p++)
            for (int64_t qq = p + 1; qq < n; qq++) {
                const double apq = A[(size_t)(p * n + qq)];
                if (apq == 0.0) continue;
                const double th = (A[(size_t)(qq * n + qq)] - A[(size_t)(p * n + p)]) / (2.0 * apq);
                const double tt = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double cs = 1.0 / std::sqrt(tt * tt + 1.0), sn = tt * cs;
                for (int64_t k = 0; k < n; k++) {
                    const double akp = A[(size_t)(k * n + p)], akq = A[(size_t)(k * n + qq)];
                    A[(size_t)(k * n + p)] = cs * akp - sn * akq;
                    A[(size_t)(k * n + qq)] = sn * akp + cs * akq;
                }
                for (int64_t k = 0; k < n; k++) {
                    const double apk = A[(size_t)(p * n + k)], aqk = A[(size_t)(qq * n + k)];
                    A[(size_t)(p * n + k)] = cs * apk - sn * aqk;
                    A[(size_t)(qq * n + k)] = sn * apk + cs * aqk;
                }
                for (int64_t k = 0; k < n; k++) {
                    const double vkp = V[(size_t)(k * n + p)], vkq = V[(size_t)(k * n + qq)];
                    V[(size_t)(k * n + p)] = cs * vkp - sn * vkq;
                    V[(size_t)(k * n + qq)] = sn * vkp + cs * vkq;
                }
            }
    }
    double wmax = 0.0;
    for (int64_t i = 0; i < n; i++) wmax = std::max(wmax, std::fabs(A[(size_t)(i * n + i)]));
    const double tol = wmax * (double)n * std::numeric_limits<double>::epsilon();
    std::vector<double> out((size_t)(n * ncol), 0.0);
    for (int64_t e = 0; e < n; e++) {
        const double w = A[(size_t)(e * n + e)];
        if (std::fabs(w) <= tol) continue;
        for (int64_t c = 0; c < ncol; c++) {
            double proj = 0.0;
            for (int64_t k = 0; k < n; k++) proj += V[(size_t)(k * n + e)] * Y[(size_t)(k * ncol + c)];
            proj /= w;
            for (int64_t k = 0; k < n; k++) out[(size_t)(k * ncol + c)] += V[(size_t)(k * n + e)] * proj;
        }
    }
    Y = out;
}

} // namespace

void transform_complete_dual(const ProblemTransform &t, double *z) {
    const double r2 = std::sqrt(2.0);
    for (const CliquePattern &p : t.patterns) {
        const int64_t N = p.side;
        double *zc = z + p.row_orig;
        // W = Z[ordering, ordering] with Z the symmetric matrix of the scaled triangle (off-diagonals / sqrt 2)
        std::vector<double> W((size_t)(N * N));
        for (int64_t a = 0; a < N; a++)
            for (int64_t b2 = 0; b2 < N; b2++) {
                const int64_t i = p.ordering[(size_t)a], j = p.ordering[(size_t)b2];
                const double v = zc[triu_index(std::min(i, j), std::max(i, j))];
                W[(size_t)(a * N + b2)] = i == j ? v : v / r2;
            }
        std::vector<uint8_t> mark((size_t)N);
        for (int64_t k = p.ncliques() - 2; k >= 0; k--) {
            const int64_t i0 = p.snode_start[(size_t)k], nn = p.snode_len[(size_t)k];
            const std::vector<int64_t> &al = p.sep[(size_t)k];
            std::fill(mark.begin(), mark.end(), 0);
            for (int64_t v : al) mark[(size_t)v] = 1;
            for (int64_t v = i0; v < i0 + nn; v++) mark[(size_t)v] = 1;
            std::vector<int64_t> eta;
            for (int64_t v = i0 + 1; v < N; v++)
                if (!mark[(size_t)v]) eta.push_back(v);
            const int64_t na = (int64_t)al.size(), ne = (int64_t)eta.size();
            if (ne == 0) continue;
            std::vector<double> Waa((size_t)(na * na)), Y((size_t)(na * nn));
            for (int64_t a = 0; a < na; a++) {
                for (int64_t b2 = 0; b2 < na; b2++) Waa[(size_t)(a * na + b2)] = W[(size_t)(al[a] * N + al[b2])];
                for (int64_t c = 0; c < nn; c++) Y[(size_t)(a * nn + c)] = W[(size_t)(al[a] * N + i0 + c)];
            }
            if (na) spd_solve(Waa, na, Y, nn);
            for (int64_t e = 0; e < ne; e++)
                for (int64_t c = 0; c < nn; c++) {
                    double v = 0.0;
                    for (int64_t a = 0; a < na; a++) v += W[(size_t)(eta[e] * N + al[a])] * Y[(size_t)(a * nn + c)];
                    W[(size_t)(eta[e] * N + i0 + c)] = v;
                    W[(size_t)((i0 + c) * N + eta[e])] = v;
                }
        }
        for (int64_t a = 0; a < N; a++)
            for (int64_t b2 = 0; b2 < N; b2++) {
                const int64_t i = p.ordering[(size_t)a], j = p.ordering[(size_t)b2];
                if (i > j) continue;
                const double v = W[(size_t)(a * N + b2)];
                zc[triu_index(i, j)] = i == j ? v : v * r2;
            }
    }
}

} // namespace chip

#ifdef CHIP_TESTING
// ---- test hooks (include/clarabel_hip_testing.h): the transform alone, on the host --------------------------------
#include <cstring>
#include <string>

#include "../../include/clarabel_hip_testing.h"

using chip::ProblemTransform;

int32_t chip_debug_transform_create(void **out, int64_t n, int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval,
                                    const double *Pnzval, const double *q, const uint64_t *Acolptr,
                                    const uint64_t *Arowval, const double *Anzval, const double *b, int64_t ncones,
                                    const int32_t *cone_tags, const int64_t *cone_dims, const int64_t *cone_dims2,
                                    const double *cone_alphas_or_null, const void *solver_settings) {
    if (!out || !solver_settings || n < 0 || m < 0 || !Pcolptr || !Acolptr) return CHIP_ERR_ARG;
    *out = nullptr;
    for (uint64_t k = 0; k < Acolptr[n]; k++)
        if ((int64_t)Arowval[k] >= m) return CHIP_ERR_DIM;
    ProblemTransform *t = new ProblemTransform();
    const int rc = chip::transform_build(n, m, Pcolptr, Prowval, Pnzval, q, Acolptr, Arowval, Anzval, b, ncones,
                                         cone_tags, cone_dims, cone_dims2, cone_alphas_or_null,
                                         chip::transform_options(*(const chip_solver_settings *)solver_settings), *t);
    if (rc) {
        delete t;
        return rc;
    }
    *out = t;
    return CHIP_OK;
}

void chip_debug_transform_destroy(void *h) { delete (ProblemTransform *)h; }

int32_t chip_debug_transform_get(const void *h, const char *name, int64_t *len, void *out) {
    if (!h || !name || !len) return CHIP_ERR_ARG;
    const ProblemTransform &t = *(const ProblemTransform *)h;
    std::vector<int64_t> iv;
    const std::vector<double> *dv = nullptr;
    const std::string nm(name);
    auto widen = [&](const auto &v) { iv.assign(v.begin(), v.end()); };
    if (nm == "sizes")
        iv = {t.active() ? 1 : 0, t.n, t.m, t.m_reduced, t.n2, t.m2, (int64_t)t.patterns.size(), t.premerge_added,
              t.final_added, t.largest_clique};
    else if (nm == "keep") widen(t.keep);
    else if (nm == "Pp") widen(t.Pp);
    else if (nm == "Pi") widen(t.Pi);
    else if (nm == "Ap") widen(t.Ap);
    else if (nm == "Ai") widen(t.Ai);
    else if (nm == "dims") iv = t.dims;
    else if (nm == "dims2") iv = t.dims2;
    else if (nm == "tags") widen(t.tags);
    else if (nm == "mode") widen(t.mode);
    else if (nm == "ptr") iv = t.ptr;
    else if (nm == "src") iv = t.src;
    else if (nm == "H_row") iv = t.H_row;
    else if (nm == "Px") dv = &t.Px;
    else if (nm == "q") dv = &t.q;
    else if (nm == "Ax") dv = &t.Ax;
    else if (nm == "b") dv = &t.b;
    else if (nm == "alphas") dv = &t.alphas;
    else if (nm.rfind("pattern", 0) == 0) {
        const size_t dot = nm.find('.');
        if (dot == std::string::npos) return CHIP_ERR_ARG;
        const size_t k = (size_t)std::stoul(nm.substr(7, dot - 7));
        if (k >= t.patterns.size()) return CHIP_ERR_ARG;
        const chip::CliquePattern &p = t.patterns[k];
        const std::string f = nm.substr(dot + 1);
        if (f == "ordering") iv = p.ordering;
        else if (f == "snode_start") iv = p.snode_start;
        else if (f == "snode_len") iv = p.snode_len;
        else if (f == "parent") iv = p.parent;
        else if (f == "info") iv = {p.cone, p.row_orig, p.row_pre, p.side, p.premerge_cliques};
        else if (f.rfind("sep", 0) == 0) {
            const size_t j = (size_t)std::stoul(f.substr(3));
            if (j >= p.sep.size()) return CHIP_ERR_ARG;
            iv = p.sep[j];
        } else return CHIP_ERR_ARG;
    } else return CHIP_ERR_ARG;
    if (dv) {
        *len = (int64_t)dv->size();
        if (out && !dv->empty()) std::memcpy(out, dv->data(), dv->size() * sizeof(double));
    } else {
        *len = (int64_t)iv.size();
        if (out && !iv.empty()) std::memcpy(out, iv.data(), iv.size() * sizeof(int64_t));
    }
    return CHIP_OK;
}

int32_t chip_debug_transform_reverse(const void *h, const double *x2, const double *s2, const double *z2, double *x,
                                     double *s, double *z) {
    if (!h || !x || !s || !z) return CHIP_ERR_ARG;
    const ProblemTransform &t = *(const ProblemTransform *)h;
    if (!t.active()) { // the identity
        std::memcpy(x, x2, (size_t)t.n * sizeof(double));
        std::memcpy(s, s2, (size_t)t.m * sizeof(double));
        std::memcpy(z, z2, (size_t)t.m * sizeof(double));
        return CHIP_OK;
    }
    chip::transform_reverse_host(t, x2, s2, z2, x, s, z);
    if (t.decomposed() && t.opt.complete_dual) chip::transform_complete_dual(t, z);
    return CHIP_OK;
}
#endif
