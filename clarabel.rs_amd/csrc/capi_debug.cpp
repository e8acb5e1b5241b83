// capi_debug.cpp -- the test hooks of include/clarabel_hip_testing.h on the L2 handle and the PSD cone kernels
// (chip_debug_*); empty without TESTING=1
#ifdef CHIP_TESTING
#include <memory>

#include "host_util.hpp"
#include "kkt_handle.hpp"

using namespace chip;

namespace {

// a bare PsdView over a vector that holds only these cones' svec ranges (chip_debug_psd_*): the sizing is host only, the
// first runner uploads it to the current device
struct DebugPsd {
    PsdSizing sz;
    i64 m = 0; // rows of the vector (sum of the cones' n (n + 1) / 2)
    DevPool mem;
    dev::PsdView pv{};
    int *fail_flag = nullptr;
    int gen = 0, last_jacobi_lds = 0;
    bool uploaded = false;
    int device = 0;
    hipStream_t stream = nullptr;
    ~DebugPsd() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
    int ready() {
        if (uploaded) {
            CHIP_HIP(hipSetDevice(device));
            return CHIP_OK;
        }
        if (chip_device_count() < 1) return fail(CHIP_ERR_NO_DEVICE, "chip_debug_psd: no HIP device");
        CHIP_HIP(hipGetDevice(&device));
        int rc;
        if ((rc = mem.alloc(&fail_flag, 1))) return rc;
        CHIP_HIP(hipMemset(fail_flag, 0, sizeof(int)));
        if ((rc = psd_view_build(mem, pv, sz, nullptr, fail_flag))) return rc;
        CHIP_HIP(hipMemset(pv.state, 0, (size_t)(sz.state ? sz.state : 1) * sizeof(double)));
        CHIP_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        uploaded = true;
        return CHIP_OK;
    }
};
// the device copies of one runner call; out arrays are uploaded too (entries a pass leaves alone come back unchanged)
struct DebugPsdStage {
    DevPool mem;
    struct Buf {
        void *host, *dev;
        size_t bytes;
    };
    std::vector<Buf> outs;
    int in(const double *host, size_t len, const double **devp) {
        double *d = nullptr;
        *devp = nullptr;
        if (!host) return CHIP_OK;
        int rc = mem.upload(&d, host, len);
        *devp = d;
        return rc;
    }
    int out(double *host, size_t len, double **devp) {
        *devp = nullptr;
        if (!host) return CHIP_OK;
        int rc = mem.upload(devp, (const double *)host, len);
        if (rc) return rc;
        outs.push_back(Buf{host, *devp, len * sizeof(double)});
        return CHIP_OK;
    }
    int finish(hipStream_t s) {
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipStreamSynchronize(s));
        for (const Buf &b : outs)
            if (b.bytes) CHIP_HIP(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
        return CHIP_OK;
    }
};

} // namespace

extern "C" {

// test hooks (include/clarabel_hip_testing.h): a kernel that only spins, on a stream of its own (co-residency tests of
// the persistent launches); a switch of csrc/switches.hpp set or cleared by name
int32_t chip_debug_spin(int32_t device, int32_t blocks, int32_t threads, int32_t lds_bytes, double usec) {
    static hipStream_t spin_stream[16] = {};
    if (device < 0 || device >= 16 || blocks < 0 || threads <= 0 || threads > 1024 || lds_bytes < 0 || lds_bytes > 160 * 1024)
        return CHIP_ERR_ARG;
    int prev = -1;
    (void)hipGetDevice(&prev);
    struct Restore { // the caller's current device is left as it was
        int d;
        ~Restore() {
            if (d >= 0) (void)hipSetDevice(d);
        }
    } restore{prev};
    CHIP_HIP(hipSetDevice(device));
    if (blocks == 0) { // wait for the spinners launched so far
        if (spin_stream[device]) CHIP_HIP(hipStreamSynchronize(spin_stream[device]));
        return CHIP_OK;
    }
    if (!spin_stream[device]) CHIP_HIP(hipStreamCreateWithFlags(&spin_stream[device], hipStreamNonBlocking));
    dev::debug_spin(spin_stream[device], blocks, threads, lds_bytes, usec);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_debug_set_switch(const char *name, const char *value_or_null) {
    return switches_set(name, value_or_null) ? CHIP_OK : fail(CHIP_ERR_ARG, "chip_debug_set_switch: unknown switch");
}
int32_t chip_debug_counter(const void *kkt_handle, const char *name, double *out) {
    const chip_kkt *h = (const chip_kkt *)kkt_handle;
    if (!h || !name || !out) return CHIP_ERR_ARG;
    const std::string k(name);
    const Engine &E = h->E;
    if (k == "dense_blocks") *out = E.dblk.nblk;
    else if (k == "dense_block_rows") *out = E.dblk.nrows;
    else if (k == "nnzS") *out = (double)E.nnzS;
    else if (k == "psd_hs_row_blocks") *out = h->cones.psd.rows_nblk;
    else if (k == "assembled_levels") {
        int c = 0;
        for (size_t l = 0; l + 1 < E.asm_lvl_ptr.size(); l++) c += E.asm_lvl_ptr[l + 1] > E.asm_lvl_ptr[l];
        *out = c;
    } else if (k == "assembled_targets") *out = E.asm_lvl_ptr.empty() ? 0 : E.asm_lvl_ptr.back();
    else if (k == "g_levels") { // unit levels whose supernodes use the one-pass substitution matrices (snode_g.hip)
        int c = 0;
        for (char f : E.sn_lvl_g) c += f != 0;
        *out = E.sn_g_ntasks > 0 ? c : 0;
    } else if (k == "sn_levels") {
        int c = 0;
        for (size_t l = 0; l + 1 < E.sn_lvl_ptr.size(); l++) c += E.sn_lvl_ptr[l + 1] > E.sn_lvl_ptr[l];
        *out = c;
    } else if (k == "g_entries") *out = E.sn_g_entries;
    else if (k == "gsweep_runs") *out = (double)E.gs_runs.size(); // runs of unit levels taken by one persistent launch per sweep (after the first solve)
    else if (k == "gsweep_launches") *out = E.gs_launches;
    else if (k == "gsweep_recoveries") *out = E.gs_recoveries;
    else if (k == "tri2_launches") *out = E.tri2_launches;
    else if (k == "dblk2_launches") *out = (double)E.dblk2_launches;
    else if (k == "dblk_blocks") *out = E.dblk.nblk;
    else if (k == "hs_direct_refactors") *out = (double)E.hs_direct_refactors;
    else if (k == "gsweep_levels") {
        int c = 0;
        for (const auto &r : E.gs_runs) c += r.nlev;
        *out = c;
    }
    // pattern classes of the bundles (host.hpp: PatternShare): all but the last are host analysis, on host-only handles too
    else if (k == "pattern_classes") *out = E.pat_classes;
    else if (k == "pattern_index_bytes") *out = (double)E.pat_index_bytes;
    else if (k == "pattern_bundles") *out = E.pat_bundles;
    else if (k == "pattern_full_index_bytes") *out = (double)E.pat_full_bytes;
    else if (k == "pattern_verified_bundles") *out = E.pat_verified;
    else if (k == "pattern_mismatches") *out = E.pat_mismatches;
    else if (k == "pattern_shared_bundles") // bundles whose fused solve launch reads a shared copy
        *out = (h->ir_sf && E.pat_off && !switches().no_shared_pattern) ? E.bundles.nb : 0;
    // run-coded update records of the flat bundle factorisation (host.hpp: Symbolic::fr_desc): host analysis, on host-only
    // handles too; "factor_run_kernel": 1 when the refactor of this handle launches the run form (device handles)
    else if (k == "factor_runs") *out = E.fr_runs;
    else if (k == "factor_record_bundles") *out = E.fr_bundles;
    else if (k == "factor_classes") *out = E.fc_classes;
    else if (k == "factor_class_verified") *out = E.fc_verified;
    else if (k == "factor_class_mismatches") *out = E.fc_mismatches;
    else if (k == "factor_run_leftover") *out = E.fr_left;
    else if (k == "factor_run_max_leftover") *out = E.fr_max_left;
    else if (k == "factor_run_invalid") *out = E.fr_invalid;
    else if (k == "factor_run_kernel") *out = (E.fr_desc && E.factor_lds_doubles > 0 && !switches().no_factor_flat && !(E.gstep_factor_on && !switches().no_step_kernel)) ? 1 : 0;
    else if (k == "factor_records_on_device") *out = E.fu_rec ? 1 : 0;
    else if (k == "irs_desc_bundles") { // bundles whose fused solve launch reads its record (dev::IrsDesc) under the current switches
        const bool shared = E.pat_off && !switches().no_shared_pattern;
        const int flags = switches().irs_flags < 0 ? 3 : switches().irs_flags;
        *out = (h->ir_sf && h->irs_desc && !(flags & dev::IRS_F_CHAINED) && h->irs_desc_shared == shared) ? E.bundles.nb : 0;
    }
    // bundles whose fused solve launch adds into replica slots under the current switches / their replicated nodes
    else if (k == "irs_replica_bundles" || k == "irs_replica_nodes") {
        const int flags = switches().irs_flags < 0 ? 3 : switches().irs_flags;
        const bool on = h->irs_rep_bundles && !(flags & (dev::IRS_F_CHAINED | dev::IRS_F_NOREP)) && !switches().no_shared_pattern &&
                        (h->E.host_only || (h->ir_sf && h->irs_desc));
        *out = !on ? 0 : k == "irs_replica_bundles" ? h->irs_rep_bundles : h->irs_rep_nodes;
    }
    else if (k == "irs_fixed_launches") *out = (double)h->irs_fixed_launches; // fused solve launches that took k_bundle_irs_fixed
    else if (k == "mailbox_mirror_on") *out = E.mirror_writes() ? 1 : 0;   // update and solves end in launches that write the host mirror
    else if (k == "mailbox_copies") *out = (double)E.mailbox_copies;       // collects that copied the mailbox
    else if (k == "mailbox_mirror_reads") *out = (double)E.mailbox_mirror_reads; // ... that read the host mirror the kernels wrote
    else return fail(CHIP_ERR_ARG, "chip_debug_counter: unknown name");
    return CHIP_OK;
}
int32_t chip_debug_kkt_ints(const void *handle, const char *name, int64_t *len, int32_t *out) {
    const chip_kkt *h = (const chip_kkt *)handle;
    if (!h || !name || !len) return fail(CHIP_ERR_ARG, "chip_debug_kkt_ints: bad argument");
    const std::string k(name);
    const std::vector<int> *v = nullptr;
    if (k == "irs_desc") v = &h->h_irs_desc;
    else if (k == "bundle_ptr") v = &h->t_bundle_ptr;
    else if (k == "blvl_ptr") v = &h->t_blvl_ptr;
    else if (k == "blvl") v = &h->t_blvl;
    else if (k == "Lp") v = &h->t_Lp;
    else if (k == "Up") v = &h->t_Up;
    else if (k == "run_ptr") v = &h->t_run_ptr;
    else if (k == "runs") v = &h->t_runs;
    else if (k == "pat_off") v = &h->t_pat_off;
    else if (k == "irs_rep") v = &h->h_irs_rep;
    else if (k == "replica_plan") v = &h->t_rep_plan;
    else if (k == "pat_Li16") v = &h->t_pat_Li16;
    else if (k == "pat_Ucol16") v = &h->t_pat_Ucol16;
    else if (k == "pat_Urow16") v = &h->t_pat_Urow16;
    else if (k == "Li16") v = &h->t_Li16;
    else if (k == "Ucol16") v = &h->t_Ucol16;
    else if (k == "factor_bundle_desc") v = &h->t_fr_bdesc;
    else if (k == "factor_class_usr") v = &h->t_fc_usr;
    else if (k == "factor_class_col") v = &h->t_fc_col;
    else if (k == "factor_class_sgn") v = &h->t_fc_sgn;
    else if (k == "factor_class_desc") v = &h->t_fc_desc;
    else if (k == "factor_class_rec") v = &h->t_fc_rec;
    else return fail(CHIP_ERR_ARG, "chip_debug_kkt_ints: unknown name");
    *len = (int64_t)v->size();
    if (out) std::copy(v->begin(), v->end(), out);
    return CHIP_OK;
}
int32_t chip_debug_kkt_factors(void *handle, double *Lx, double *D) {
    chip_kkt *h = (chip_kkt *)handle;
    if (!h) return fail(CHIP_ERR_ARG, "chip_debug_kkt_factors: bad argument");
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    CHIP_HIP(hipStreamSynchronize(E.stream));
    if (Lx && E.nnzL) CHIP_HIP(hipMemcpy(Lx, E.Lx, (size_t)E.nnzL * sizeof(double), hipMemcpyDeviceToHost));
    if (D && E.N) CHIP_HIP(hipMemcpy(D, E.D, (size_t)E.N * sizeof(double), hipMemcpyDeviceToHost));
    return CHIP_OK;
}
int32_t chip_debug_factor_updates(const void *handle, int32_t bundle, const char *what, int64_t *len, int32_t *out) {
    const chip_kkt *h = (const chip_kkt *)handle;
    if (!h || !what || !len) return fail(CHIP_ERR_ARG, "chip_debug_factor_updates: bad argument");
    const std::string k(what);
    const int nb = h->t_fu_lvl_ptr.empty() ? 0 : (int)h->t_fu_lvl_ptr.size() - 1;
    if (bundle < 0 || bundle >= nb) return fail(CHIP_ERR_ARG, "chip_debug_factor_updates: no such bundle (host-only handles)");
    const int lb0 = h->t_fu_lvl_ptr[(size_t)bundle], nl = h->t_fu_lvl_ptr[(size_t)bundle + 1] - lb0 - 1;
    std::vector<int32_t> res;
    auto records = [&](const std::vector<uint16_t> &rec, const std::vector<int> &ptr) {
        if (ptr.empty()) return;
        for (int l = 0; l < nl; l++)
            for (int t = ptr[(size_t)lb0 + l]; t < ptr[(size_t)lb0 + l + 1]; t++) {
                res.push_back(l);
                for (int f = 0; f < 4; f++) res.push_back(rec[(size_t)t * 4 + f]);
            }
    };
    if (k == "records") records(h->t_fu_rec, h->t_fu_ptr);
    else if (k == "leftover") records(h->t_fr_rec, h->t_fr_rptr);
    else if (k == "runs") {
        if (!h->t_fr_ptr.empty())
            for (int l = 0; l < nl; l++)
                for (int d = h->t_fr_ptr[(size_t)lb0 + l]; d < h->t_fr_ptr[(size_t)lb0 + l + 1]; d++) {
                    const int *e = h->t_fr_desc.data() + (size_t)d * 8;
                    const int32_t row[10] = {l, e[0], e[1], e[2], e[3], (int16_t)(e[4] & 0xFFFF), (int16_t)(e[4] >> 16),
                                             (int16_t)(e[5] & 0xFFFF), (int16_t)(e[5] >> 16), e[6]};
                    res.insert(res.end(), row, row + 10);
                }
    } else return fail(CHIP_ERR_ARG, "chip_debug_factor_updates: unknown name");
    *len = (int64_t)res.size();
    if (out) std::copy(res.begin(), res.end(), out);
    return CHIP_OK;
}
// ---- the PSD cone kernels of cones.hip alone, one launch per call on host arrays (tests/test_psd_passes_gpu.py) ----
int32_t chip_debug_psd_create(void **out, int64_t ncones, const int64_t *dims) {
    if (!out) return fail(CHIP_ERR_ARG, "chip_debug_psd_create: bad argument");
    *out = nullptr;
    if (ncones < 1 || !dims) return fail(CHIP_ERR_ARG, "chip_debug_psd_create: bad argument");
    // the cone constructor of chip_kkt_create (build_cone_specs): rows, Hs block starts and refusals are its own
    std::vector<i32> tags((size_t)ncones, CHIP_CONE_PSDTRIANGLE);
    std::vector<ConeSpec> specs;
    i64 m = 0, p = 0, nHs = 0;
    if (build_cone_specs(ncones, tags.data(), dims, nullptr, specs, m, p, nHs))
        return fail(CHIP_ERR_ARG, "chip_debug_psd_create: cones refused");
    for (const ConeSpec &c : specs)
        if (c.dim < 0 || c.dim > 1024) return fail(CHIP_ERR_ARG, "chip_debug_psd_create: side out of range (0 .. 1024)");
    std::unique_ptr<DebugPsd> h(new DebugPsd());
    for (const ConeSpec &c : specs) h->sz.add(c.start, c.dim, c.block_start);
    h->m = m;
    *out = h.release();
    return CHIP_OK;
}
void chip_debug_psd_destroy(void *h) { delete (DebugPsd *)h; }
int32_t chip_debug_psd_counter(const void *handle, const char *name, double *out) {
    const DebugPsd *h = (const DebugPsd *)handle;
    if (!h || !name || !out) return fail(CHIP_ERR_ARG, "chip_debug_psd_counter: bad argument");
    const std::string k(name);
    if (k == "gs") *out = h->sz.scratch_stride ? 1 : 0;
    else if (k == "jacobi_lds") *out = h->last_jacobi_lds;
    else if (k == "maxdim") *out = h->sz.maxdim;
    else if (k == "rows") *out = (double)h->m;
    else if (k == "scratch_stride") *out = (double)h->sz.scratch_stride;
    else if (k == "state_doubles") *out = (double)h->sz.state;
    else return fail(CHIP_ERR_ARG, "chip_debug_psd_counter: unknown name");
    return CHIP_OK;
}
int32_t chip_debug_psd_update_scaling(void *handle, const double *s, const double *z, int32_t *ok) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !s || !z || !ok) return fail(CHIP_ERR_ARG, "chip_debug_psd_update_scaling: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugPsdStage st;
    const double *ds, *dz;
    if ((rc = st.in(s, (size_t)h->m, &ds)) || (rc = st.in(z, (size_t)h->m, &dz))) return rc;
    h->pv.fail_gen = ++h->gen; // (the generation a failing cone leaves in the flag, as chip_kkt_update_scaling does)
    dev::psd_update_scaling(h->stream, h->pv, ds, dz);
    h->last_jacobi_lds = dev::psd_last_jacobi_lds();
    if ((rc = st.finish(h->stream))) return rc;
    int flag = 0;
    CHIP_HIP(hipMemcpy(&flag, h->fail_flag, sizeof(int), hipMemcpyDeviceToHost));
    *ok = flag == h->gen ? 0 : 1;
    return CHIP_OK;
}
int32_t chip_debug_psd_state(void *handle, int64_t cone, double *out) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !out || cone < 0 || cone >= (int64_t)h->sz.dim.size())
        return fail(CHIP_ERR_ARG, "chip_debug_psd_state: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    const size_t n = (size_t)h->sz.dim[(size_t)cone];
    CHIP_HIP(hipStreamSynchronize(h->stream));
    CHIP_HIP(hipMemcpy(out, h->pv.state + h->sz.off[(size_t)cone], (3 * n * n + 2 * n) * sizeof(double),
                       hipMemcpyDeviceToHost));
    return CHIP_OK;
}
int32_t chip_debug_psd_mul_hs(void *handle, double *y, const double *x) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !y || !x) return fail(CHIP_ERR_ARG, "chip_debug_psd_mul_hs: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugPsdStage st;
    double *dy;
    const double *dx;
    if ((rc = st.out(y, (size_t)h->m, &dy)) || (rc = st.in(x, (size_t)h->m, &dx))) return rc;
    dev::psd_mul_hs(h->stream, h->pv, dy, dx);
    return st.finish(h->stream);
}
int32_t chip_debug_psd_affine_ds(void *handle, double *ds) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !ds) return fail(CHIP_ERR_ARG, "chip_debug_psd_affine_ds: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugPsdStage st;
    double *dds;
    if ((rc = st.out(ds, (size_t)h->m, &dds))) return rc;
    dev::psd_affine_ds(h->stream, h->pv, dds);
    return st.finish(h->stream);
}
int32_t chip_debug_psd_combined_ds_shift(void *handle, double *shift, double *step_z, double *step_s, double sigma_mu) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !shift || !step_z || !step_s || step_z == step_s || shift == step_z || shift == step_s)
        return fail(CHIP_ERR_ARG, "chip_debug_psd_combined_ds_shift: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugPsdStage st;
    double *d0, *d1, *d2;
    if ((rc = st.out(shift, (size_t)h->m, &d0)) || (rc = st.out(step_z, (size_t)h->m, &d1)) ||
        (rc = st.out(step_s, (size_t)h->m, &d2)))
        return rc;
    dev::psd_combined_ds_shift(h->stream, h->pv, d0, d1, d2, sigma_mu);
    return st.finish(h->stream);
}
int32_t chip_debug_psd_ds_from_dz_offset(void *handle, double *out, const double *ds) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !out || !ds) return fail(CHIP_ERR_ARG, "chip_debug_psd_ds_from_dz_offset: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugPsdStage st;
    double *d0;
    const double *d1;
    if ((rc = st.out(out, (size_t)h->m, &d0)) || (rc = st.in(ds, (size_t)h->m, &d1))) return rc;
    dev::psd_ds_from_dz_offset(h->stream, h->pv, d0, d1);
    return st.finish(h->stream);
}
int32_t chip_debug_psd_step_length(void *handle, const double *dz, const double *ds, double amax, double *partial) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !dz || !ds || !partial) return fail(CHIP_ERR_ARG, "chip_debug_psd_step_length: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugPsdStage st;
    const double *d0, *d1;
    double *dp;
    if ((rc = st.in(dz, (size_t)h->m, &d0)) || (rc = st.in(ds, (size_t)h->m, &d1)) ||
        (rc = st.out(partial, h->sz.dim.size(), &dp)))
        return rc;
    (void)dev::psd_step_length(h->stream, h->pv, d0, d1, amax, dp);
    h->last_jacobi_lds = dev::psd_last_jacobi_lds();
    return st.finish(h->stream);
}
int32_t chip_debug_psd_margins(void *handle, const double *z, double *pmin, double *psum) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !z || !pmin || !psum) return fail(CHIP_ERR_ARG, "chip_debug_psd_margins: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugPsdStage st;
    const double *d0;
    double *dmin, *dsum;
    if ((rc = st.in(z, (size_t)h->m, &d0)) || (rc = st.out(pmin, h->sz.dim.size(), &dmin)) ||
        (rc = st.out(psum, h->sz.dim.size(), &dsum)))
        return rc;
    (void)dev::psd_margins(h->stream, h->pv, d0, dmin, dsum);
    h->last_jacobi_lds = dev::psd_last_jacobi_lds();
    return st.finish(h->stream);
}
int32_t chip_debug_psd_barrier(void *handle, const double *z, const double *s, const double *dz, const double *ds,
                               double alpha, double *partial) {
    DebugPsd *h = (DebugPsd *)handle;
    if (!h || !z || !s || !dz || !ds || !partial) return fail(CHIP_ERR_ARG, "chip_debug_psd_barrier: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugPsdStage st;
    const double *d0, *d1, *d2, *d3;
    double *dp;
    const size_t m = (size_t)h->m;
    if ((rc = st.in(z, m, &d0)) || (rc = st.in(s, m, &d1)) || (rc = st.in(dz, m, &d2)) || (rc = st.in(ds, m, &d3)) ||
        (rc = st.out(partial, h->sz.dim.size(), &dp)))
        return rc;
    (void)dev::psd_barrier(h->stream, h->pv, d0, d1, d2, d3, alpha, dp);
    return st.finish(h->stream);
}

} // extern "C"
#endif
