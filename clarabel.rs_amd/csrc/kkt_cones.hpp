// kkt_cones.hpp -- the cones of one L2 handle (chip_kkt): their device tables, built once at creation, and one method
// per cone pass of an interior-point iteration.  Internal to the library (kkt_create.cpp, kkt_cones.cpp, kkt_step.cpp,
// capi.cpp, capi_debug.cpp).
#pragma once
#include <algorithm>
#include <vector>

#include "engine.hpp"

namespace chip {

// ---- the PSD cones' device view (dev::PsdView, kernels.hpp) -- one function for KktCones::build and the test runners
// (chip_debug_psd_*).  PsdSizing is host arithmetic only: per cone its first row, side, Hs block and the offset of its
// state (3 n^2 + 2 n doubles: B | lambda | lambda^-1/2 | R | Rinv), the largest side, and the decision that holds for
// ALL cones of the view: a largest side above 64 puts the kernels' work matrices into a scratch slice per cone in HBM
// (4 maxdim^2 + 4 maxdim + 16 doubles each) instead of LDS.
struct PsdSizing {
    std::vector<int> start, dim, hs, off;
    i64 state = 0;
    int maxdim = 0;
    long long scratch_stride = 0; // 0: work matrices in LDS
    void add(i64 start_row, i64 side, i64 hs_start) {
        start.push_back((int)start_row);
        dim.push_back((int)side);
        hs.push_back((int)hs_start);
        off.push_back((int)state);
        state += 3 * side * side + 2 * side;
        maxdim = std::max<int>(maxdim, (int)side);
        scratch_stride = maxdim > 64 ? 4LL * maxdim * maxdim + 4LL * maxdim + 16 : 0;
    }
};
// uploads the sizing through `mem` (Engine or DevPool: alloc(T **, n)) and fills the view; rows_nblk and its arrays
// (the dense-block analysis of KktCones::build) are left as they are
template <typename Mem>
int psd_view_build(Mem &mem, dev::PsdView &pv, const PsdSizing &sz, const int *mapHs, int *fail_flag) {
    int rc;
    const size_t nc = sz.start.size();
    int *q[4] = {nullptr, nullptr, nullptr, nullptr};
    const std::vector<int> *src[4] = {&sz.start, &sz.dim, &sz.hs, &sz.off};
    for (int k = 0; k < 4; k++) {
        if ((rc = mem.alloc(&q[k], nc))) return rc;
        if (nc) CHIP_HIP(hipMemcpy(q[k], src[k]->data(), nc * sizeof(int), hipMemcpyHostToDevice));
    }
    double *qs;
    if ((rc = mem.alloc(&qs, (size_t)(sz.state ? sz.state : 1)))) return rc;
    pv.ncones = (int)nc;
    pv.maxdim = sz.maxdim;
    pv.scratch = nullptr;
    pv.scratch_stride = sz.scratch_stride;
    if (sz.scratch_stride) // beyond the LDS budget of three / four n x n matrices: work matrices in HBM
        if ((rc = mem.alloc(&pv.scratch, (size_t)sz.scratch_stride * nc))) return rc;
    pv.start = q[0];
    pv.dim = q[1];
    pv.hs_start = q[2];
    pv.state_off = q[3];
    pv.state = qs;
    pv.mapHs = mapHs;
    pv.fail = fail_flag;
    return CHIP_OK;
}

struct KktCones {
    int nn_count = 0, zero_count = 0;
    const int *nn_rows = nullptr, *nn_hsidx = nullptr, *zero_rows = nullptr;
    dev::SocView soc{};
    dev::Ns3View ns3{};      // Exponential / Power cones
    dev::GpwView gpw{};      // generalised power cones
    std::vector<int> gpw_cone_index, gpw_state_off, gpw_dim1; // host copies (alpha setter)
    dev::PsdView psd{};      // PSD triangle cones (any matrix side)
    bool psd_rows_all_blocks = false; // every dense diagonal block of the top is a PSD cone's Hs block (k_psd_write_hs_rows)
    bool has_hostHs = false; // cones whose Hs must come from the host (none of the SupportedConeT kinds any more)
    double *d_w = nullptr, *d_lam = nullptr;
    double *d_partial = nullptr; // per-block partial minima / sums of the cone reductions
    int partial_cap = 0;
    std::vector<double> h_partial;
    int scaling_gen = 0; // generation of the last update_scaling: a failing cone writes it into mailbox.soc_fail

    // the device tables of K.cones; k2v: position of an entry of K in the device's value order, mapHs: the device copy of
    // the Hs map, alphas: one exponent per cone or nullptr, n: the first cone row of K
    int build(Engine &E, const KktLayout &K, const bigvec &k2v, const int *mapHs, const double *alphas, i64 n);

    // what the entry points refuse
    bool symmetric() const { return !(has_hostHs || ns3.ncones || gpw.ncones); } // margins / scaled_unit_shift
    bool sym_only() const { return symmetric() && !psd.ncones; }                 // Zero / Nonnegative / SecondOrder alone
    bool reports_failure() const { return soc.ncones > 0 || psd.ncones > 0; }    // update_scaling can fail

    // ---- the cone passes: each launches on E.stream, in the order of the reference's composite cone ----
    void next_generation() { // (no memset of the failure flag: a failure is recognised by its generation)
        scaling_gen += 1;
        soc.fail_gen = psd.fail_gen = scaling_gen;
    }
    void update_scaling(Engine &E, const double *s_dev, const double *z_dev, double mu, int strategy);
    void mul_Hs(Engine &E, double *y_dev, const double *x_dev);
    void unit_shift(Engine &E, double *z_dev, double alpha, int primal_cone);
    void affine_ds(Engine &E, double *ds_dev, const double *s_dev);
    void combined_ds_shift(Engine &E, double *shift_dev, double *step_z_dev, double *step_s_dev, double sigma_mu);
    void ds_from_dz_offset(Engine &E, double *out_dev, const double *ds_dev, const double *z_dev);
    int step_length(Engine &E, const double *dz_dev, const double *ds_dev, const double *z_dev, const double *s_dev,
                    double alpha_max, double *alpha_out);
    int barrier(Engine &E, const double *z_dev, const double *s_dev, const double *dz_dev, const double *ds_dev,
                double alpha, double *barrier_out);
    void unit_initialization(Engine &E, double *z_dev, double *s_dev, int m);
    int margins(Engine &E, const double *z_dev, double *alpha_out, double *beta_out);
    // the writes of an update into K (and, for PSD blocks that are dense diagonal blocks of the top, into L)
    bool psd_direct_rows() const { return psd_rows_all_blocks && dev::psd_write_hs_rows_active(psd); }
    void write_kkt(Engine &E, const int *mapHs, unsigned long long *dslots);
    // scaling and writes of the symmetric cones in one launch (dev::sym_scale_write); dbg: stamps or nullptr
    void scale_write(Engine &E, const double *s_dev, const double *z_dev, const int *mapHs, int *status_or_null,
                     long long *dbg);
    int set_genpow_alpha(Engine &E, const KktLayout &K, int64_t cone_index, const double *alpha);

private:
    using ConeList = std::vector<const ConeSpec *>; // the cones of one kind, in K's order
    int build_genpow(Engine &E, const KktLayout &K, const ConeList &cones, const bigvec &k2v, const int *mapHs);
    int build_psd(Engine &E, const PsdSizing &pd, const int *mapHs, i64 n);
    int psd_dense_blocks(Engine &E, const PsdSizing &pd, i64 n);
    int build_ns3(Engine &E, const KktLayout &K, const ConeList &cones, const double *alphas, const int *mapHs);
    int build_soc(Engine &E, const KktLayout &K, const ConeList &cones, const bigvec &k2v, const int *mapHs);
    int ensure_partials(Engine &E);
    int fetch_partials(Engine &E, int used, int halves);
};

} // namespace chip
