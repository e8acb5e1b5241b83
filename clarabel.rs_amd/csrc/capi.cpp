// capi.cpp -- the parts of the C ABI of include/clarabel_hip.h that belong to no layer: default settings, ordering,
// the last error, and what a handle tells about itself (dimensions, maps, diagnostics, profiling).
//   chip_ldl_*  : capi_ldl.cpp
//   chip_kkt_*  : KKTSolver<f64> as implemented by DirectLDLKKTSolver (quasidef/directldlkktsolver.rs:18-405), device
//                 resident -- kkt_create.cpp (creation), kkt_step.cpp (update, solves), kkt_cones.cpp (cone passes)
#include "kkt_handle.hpp"

using namespace chip;

namespace {
thread_local std::string g_last;
}

namespace chip {

int count_positive(Engine &E, i64 *out) {
    std::vector<double> d((size_t)E.N);
    if (E.N) CHIP_HIP(hipMemcpy(d.data(), E.D, (size_t)E.N * sizeof(double), hipMemcpyDeviceToHost));
    i64 c = 0;
    for (double v : d) c += v > 0.0;
    *out = c;
    return CHIP_OK;
}
int32_t get_supernodes(const Engine &E, int64_t *count, uint64_t *ptr, uint64_t *cols) {
    if (!count) return CHIP_ERR_ARG;
    *count = E.nsn > 0 ? E.nsn : 0;
    if (ptr)
        for (size_t i = 0; i < E.h_sn_ptr.size(); i++) ptr[i] = (uint64_t)E.h_sn_ptr[i];
    if (cols)
        for (size_t i = 0; i < E.h_sn_col.size(); i++) cols[i] = (uint64_t)E.h_sn_col[i];
    return CHIP_OK;
}
// for the layers above, which otherwise only use the public chip_kkt_* entry points
int kkt_device(const ::chip_kkt *h) { return h->E.device; }
hipStream_t kkt_stream(::chip_kkt *h) { return h->E.host_only ? nullptr : h->E.stream; }
void kkt_set_world(::chip_kkt *h, int world) { h->world = world; }
bool kkt_host_only(const ::chip_kkt *h) { return h->E.host_only; }

} // namespace chip

extern "C" {

void chip_settings_default(chip_settings *s) {
    std::memset(s, 0, sizeof(*s));
    s->static_regularization_enable = 1;
    s->static_regularization_constant = 1e-8;
    s->static_regularization_proportional = 2.220446049250313e-16 * 2.220446049250313e-16;
    s->dynamic_regularization_enable = 1;
    s->dynamic_regularization_eps = 1e-13;
    s->dynamic_regularization_delta = 2e-7;
    s->iterative_refinement_enable = 1;
    s->iterative_refinement_reltol = 1e-13;
    s->iterative_refinement_abstol = 1e-12;
    s->iterative_refinement_max_iter = 10;
    s->iterative_refinement_stop_ratio = 5.0;
    s->device = -1;
    s->amd_dense_scale = 1.5;
    s->use_graph = 0;
    s->linesearch_backtrack_step = 0.8;
    s->min_terminate_step_length = 1e-4;
}

int32_t chip_auto_select(double lnz, double n_div, double n_mult_subs_ldl) {
    const double flops = n_div + n_mult_subs_ldl, thresh = 40.0; // auto.rs:72-79
    return (flops / lnz) < thresh ? 0 : 1;
}

const char *chip_last_error(void) {
    g_last = get_error();
    return g_last.c_str();
}

int32_t chip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int32_t chip_amd_order(int64_t n, const uint64_t *colptr, const uint64_t *rowval, double dense_scale,
                       uint64_t *perm, uint64_t *iperm, double *info3) {
    if (n < 0 || !colptr || !perm) return fail(CHIP_ERR_ARG, "chip_amd_order: bad argument");
    for (i64 c = 0; c < n; c++)
        for (uint64_t p = colptr[c]; p < colptr[c + 1]; p++)
            if (rowval[p] > (uint64_t)c) return fail(CHIP_ERR_NOT_TRIU, "matrix is not upper triangular");
    std::vector<i64> p;
    AmdInfo info;
    int rc = amd_order(n, as_i64(colptr), as_i64(rowval), dense_scale, p, &info);
    if (rc) return fail(CHIP_ERR_ARG, "amd_order failed");
    for (i64 k = 0; k < n; k++) {
        perm[k] = (uint64_t)p[k];
        if (iperm) iperm[p[k]] = (uint64_t)k;
    }
    if (info3) {
        info3[0] = info.lnz;
        info3[1] = info.ndiv;
        info3[2] = info.nmultsubs_ldl;
    }
    return CHIP_OK;
}

int32_t chip_kkt_dims(const chip_kkt *h, int64_t out[8]) {
    if (!h) return CHIP_ERR_ARG;
    out[0] = h->K.n;
    out[1] = h->K.m;
    out[2] = h->K.p;
    out[3] = h->K.N;
    out[4] = h->K.nnz;
    out[5] = h->K.nHs;
    out[6] = h->E.NF;
    out[7] = h->E.nnzU;
    return CHIP_OK;
}
// CompositeCone::degree (compositecone.rs:106-108): zerocone.rs:36-38 (0), nonnegativecone.rs:39-41 (dim),
// socone.rs:74-77 (1), psdtrianglecone.rs:77-79 (n), expcone.rs:55-57 / powcone.rs:48-50 (3),
// genpowcone.rs:84-86 (dim1 + 1)
int32_t chip_kkt_degree(const chip_kkt *h, int64_t *degree) {
    if (!h || !degree) return CHIP_ERR_ARG;
    i64 d = 0;
    for (const ConeSpec &c : h->K.cones) {
        switch (c.tag) {
        case CHIP_CONE_ZERO: break;
        case CHIP_CONE_NONNEGATIVE: d += c.dim; break;
        case CHIP_CONE_SECONDORDER: d += 1; break;
        case CHIP_CONE_PSDTRIANGLE: d += c.dim; break;
        case CHIP_CONE_EXPONENTIAL:
        case CHIP_CONE_POWER: d += 3; break;
        case CHIP_CONE_GENPOWER: d += c.dim + 1; break;
        default: break;
        }
    }
    *degree = d;
    return CHIP_OK;
}
int32_t chip_kkt_get_supernodes(const chip_kkt *h, int64_t *count, uint64_t *ptr, uint64_t *cols) {
    return h ? get_supernodes(h->E, count, ptr, cols) : CHIP_ERR_ARG;
}
int32_t chip_kkt_get_matrix(const chip_kkt *h, uint64_t *colptr, uint64_t *rowval, double *nzval) {
    if (!h) return CHIP_ERR_ARG;
    const KktLayout &K = h->K;
    if (colptr)
        for (i64 i = 0; i <= K.N; i++) colptr[i] = (uint64_t)K.colptr[i];
    if (rowval)
        for (i64 i = 0; i < K.nnz; i++) rowval[i] = (uint64_t)K.rowval[i];
    if (nzval) std::memcpy(nzval, K.nzval.data(), (size_t)K.nnz * sizeof(double));
    return CHIP_OK;
}
int32_t chip_kkt_get_map(const chip_kkt *h, uint64_t *mapP, uint64_t *mapA, uint64_t *mapHs, uint64_t *diagP,
                         uint64_t *diag_full, int8_t *dsigns) {
    if (!h) return CHIP_ERR_ARG;
    const KktLayout &K = h->K;
    auto cp = [](uint64_t *dst, const auto &src, size_t n) {
        if (dst)
            for (size_t i = 0; i < n; i++) dst[i] = (uint64_t)src[i];
    };
    cp(mapP, K.mapP, K.mapP.size() - 1);
    cp(mapA, K.mapA, K.mapA.size() - 1);
    cp(mapHs, K.mapHs, (size_t)K.nHs);
    cp(diagP, K.diagP, (size_t)K.n);
    cp(diag_full, K.diag_full, (size_t)K.N);
    if (dsigns) std::memcpy(dsigns, K.dsigns.data(), (size_t)K.N);
    return CHIP_OK;
}

int32_t chip_kkt_info(const chip_kkt *h, chip_info *info) {
    if (!h || !info) return CHIP_ERR_ARG;
    fill_info(h->E, info);
    info->threads = h->world;
    info->last_ir_iterations = h->wk[0].last_ir;
    info->last_regularizer = h->last_eps;
    if (h->E.factored && !h->E.host_only) {
        i64 c = 0;
        int rc = count_positive(const_cast<Engine &>(h->E), &c);
        if (rc) return rc;
        info->positive_inertia = c;
    }
    return CHIP_OK;
}
int32_t chip_kkt_get_perm(const chip_kkt *h, uint64_t *perm) {
    if (!h || !perm) return CHIP_ERR_ARG;
    for (int i = 0; i < h->E.N; i++) perm[i] = (uint64_t)h->E.h_perm[i];
    return CHIP_OK;
}
int32_t chip_kkt_get_symbolic(const chip_kkt *h, uint64_t *etree, uint64_t *Lp, uint64_t *Li,
                              uint64_t *lvlptr) {
    if (!h) return CHIP_ERR_ARG;
    return h->E.get_symbolic(etree, Lp, Li, lvlptr);
}
int32_t chip_kkt_get_values(chip_kkt *h, double *nzval) {
    if (!h || !nzval) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    return E.download_values(nzval); // back in the caller's K.nzval order
}
int32_t chip_kkt_synchronize(chip_kkt *h) {
    if (!h) return CHIP_ERR_ARG;
    NEED_DEVICE(h->E);
    CHIP_HIP(hipStreamSynchronize(h->E.stream));
    return CHIP_OK;
}
void *chip_kkt_stream(chip_kkt *h) { return (h && !h->E.host_only) ? (void *)h->E.stream : nullptr; }
int32_t chip_kkt_profile(chip_kkt *h, int32_t family) {
    if (!h) return CHIP_ERR_ARG;
    h->E.prof_collect();
    h->E.prof_family = family;
    h->E.prof_ms_total = 0;
    h->E.prof_launches = 0;
    return CHIP_OK;
}
int32_t chip_kkt_profile_read(chip_kkt *h, double out[8]) {
    if (!h) return CHIP_ERR_ARG;
    h->E.prof_collect();
    std::memset(out, 0, 8 * sizeof(double));
    out[0] = (double)h->E.prof_launches;
    out[1] = h->E.prof_ms_total;
    out[2] = (double)h->E.prof_family;
    return CHIP_OK;
}
int32_t chip_kkt_step_kernels(const chip_kkt *h) {
    if (!h) return CHIP_ERR_ARG;
    const bool on = !switches().no_step_kernel;
    return (on && h->E.gstep_solve_on ? 1 : 0) | (on && h->E.gstep_factor_on ? 2 : 0) | (h->ir_sf && !(on && h->E.gstep_solve_on) ? 4 : 0);
}
int32_t chip_kkt_fused_fallbacks(const chip_kkt *h) { return h ? h->fused_fallbacks : CHIP_ERR_ARG; }
int32_t chip_kkt_work_model(const chip_kkt *h, double out[8]) {
    if (!h || !out) return CHIP_ERR_ARG;
    std::memcpy(out, h->E.sn_model, 8 * sizeof(double));
    out[5] = h->E.gfold.ng;    // groups of a grouped fold in use (0: none)
    out[6] = h->E.bundles.nb;  // subtree bundles
    out[7] = h->E.ir_fused ? h->E.ir_tw : 0; // threads per workgroup of the fused solve launch (0: not fused)
    return CHIP_OK;
}
int32_t chip_kkt_sweep_model(const chip_kkt *h, double out[4]) {
    if (!h || !out) return CHIP_ERR_ARG;
    const Engine &E = h->E;
    int gl = 0, sl = 0;
    for (char f : E.sn_lvl_g) gl += f != 0;
    for (size_t l = 0; l + 1 < E.sn_lvl_ptr.size(); l++) sl += E.sn_lvl_ptr[l + 1] > E.sn_lvl_ptr[l];
    out[0] = E.sn_g_ntasks > 0 ? E.sn_g_entries : 0.0;
    out[1] = E.sn_g_ntasks > 0 ? gl : 0;
    out[2] = sl;
    out[3] = E.sn_g_ntasks > 0 ? 1 : 0;
    return CHIP_OK;
}

} // extern "C"
