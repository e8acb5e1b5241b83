// batch_debug.cpp -- the test hooks of the batched solver (include/clarabel_hip_testing.h: chip_debug_batch_*,
// chip_debug_bplan_*); empty in the build that ships
#include "batch_adjoint.hpp"
#include "batch_cotangent.hpp"
#include "batch_handle.hpp"
#include "batch_jacobian.hpp"
#include "batch_tangent.hpp"
#include "debug_stage.hpp"

#ifdef CHIP_TESTING
#include "../../include/clarabel_hip_testing.h"
int32_t chip_debug_batch_inject_nan(void *batch, int64_t member, int32_t iteration) {
    chip_batch *h = (chip_batch *)batch;
    if (!h) return fail(CHIP_ERR_ARG, "chip_debug_batch_inject_nan: bad argument");
    h->nan_member = member;
    h->nan_iter = iteration;
    return CHIP_OK;
}
int32_t chip_debug_batch_counter(void *batch, const char *name, double *out) {
    chip_batch *h = (chip_batch *)batch;
    if (!h || !name || !out) return fail(CHIP_ERR_ARG, "chip_debug_batch_counter: bad argument");
    const std::string nm(name);
    if (nm == "host_syncs") *out = (double)h->syncs;
    else if (nm == "launches") *out = (double)h->launches;
    else if (nm == "loop_iterations") *out = (double)h->loop_iters;
    else if (nm == "update_launches") *out = (double)h->upd_launches;
    else if (nm == "update_host_syncs") *out = (double)h->upd_syncs;
    else if (nm == "backward_launches") *out = (double)h->grad.launches;
    else if (nm == "backward_host_syncs") *out = (double)h->grad.syncs;
    else if (nm == "jvp_launches") *out = (double)h->tan.launches;
    else if (nm == "jvp_host_syncs") *out = (double)h->tan.syncs;
    else if (nm == "jvp_refactors") *out = (double)h->tan.refactors;
    else if (nm == "jac_launches") *out = (double)h->jac.launches;
    else if (nm == "jac_host_syncs") *out = (double)h->jac.syncs;
    else if (nm == "jac_refactors") *out = (double)h->jac.refactors;
    else if (nm == "jac_repeats") *out = (double)h->jac_repeats;
    else if (nm == "jac_calls") *out = (double)h->jac_calls;
    else if (nm == "vjp_launches") *out = (double)h->vjp.launches;
    else if (nm == "vjp_host_syncs") *out = (double)h->vjp.syncs;
    else if (nm == "vjp_refactors") *out = (double)h->vjp.refactors;
    else if (nm == "vjp_repeats") *out = (double)h->vjp_repeats;
    else if (nm == "vjp_calls") *out = (double)h->vjp_calls;
    else return fail(CHIP_ERR_ARG, "chip_debug_batch_counter: unknown name");
    return CHIP_OK;
}

// ---- the partition alone, and one launch of every launcher of batch.hpp on host arrays (tests/test_batch_plan_host.py,
// tests/test_batch_passes_gpu.py).  The plan is the one chip_batch_create builds (host_plan_build / host_plan_upload)
namespace {
struct DebugPlan {
    HostPlan hp;
    DevPool mem;
    dev::BatchPlan plan{};
    bool uploaded = false;
    int device = 0;
    hipStream_t stream = nullptr;
    double *seg_scr = nullptr, *cone_scr = nullptr;
    ~DebugPlan() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
    int ready() { // the first runner uploads the plan; chip_debug_bplan_create itself touches no device
        if (uploaded) {
            CHIP_HIP(hipSetDevice(device));
            return CHIP_OK;
        }
        if (chip_device_count() < 1) return fail(CHIP_ERR_NO_DEVICE, "chip_debug_bplan: no HIP device");
        CHIP_HIP(hipGetDevice(&device));
        int rc;
        if ((rc = host_plan_upload(mem, hp, &plan)) || (rc = mem.alloc(&seg_scr, dev::seg_scratch_doubles(plan))) ||
            (rc = mem.alloc(&cone_scr, dev::cone_scratch_doubles(plan))))
            return rc;
        CHIP_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        uploaded = true;
        return CHIP_OK;
    }
};
} // namespace

int32_t chip_debug_batch_jvp_rhs(void *batch, const double *x, const double *z, const int32_t *valid, const double *dq,
                                 const double *db, const double *dPx, const double *dAx, double *rx, double *rz) {
    chip_batch *h = (chip_batch *)batch;
    if (!h || !valid || (h->pd.n && (!x || !rx)) || (h->pd.m && (!z || !rz)))
        return fail(CHIP_ERR_ARG, "chip_debug_batch_jvp_rhs: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    int rc;
    dev::SpPattern Psym, Arow, Acol;
    if ((rc = kktsystem_pattern(h->sys, 0, &Psym)) || (rc = kktsystem_pattern(h->sys, 1, &Arow)) ||
        (rc = kktsystem_pattern(h->sys, 2, &Acol)))
        return rc;
    DebugStage st;
    const size_t n = (size_t)h->pd.n, m = (size_t)h->pd.m;
    const double *dx_, *dz_, *ddq, *ddb, *ddP, *ddA;
    const int32_t *dvalid;
    double *drx, *drz;
    if ((rc = st.in(x, n, &dx_)) || (rc = st.in(z, m, &dz_)) || (rc = st.in(valid, (size_t)h->nprob, &dvalid)) ||
        (rc = st.in(dq, n, &ddq)) || (rc = st.in(db, m, &ddb)) || (rc = st.in(dPx, (size_t)h->pd.M.nnzP, &ddP)) ||
        (rc = st.in(dAx, (size_t)h->pd.M.nnzA, &ddA)) || (rc = st.out(rx, n, &drx)) || (rc = st.out(rz, m, &drz)))
        return rc;
    hipStream_t s = nullptr;
    CHIP_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    dev::bt_rhs(s, h->plan, Psym, Acol, Arow,
                dev::BtRhs{dvalid, dx_, dz_, ddq, ddb, ddP, ddA, h->pd.d, h->pd.e, h->dc, drx, drz, nullptr, nullptr,
                           nullptr, nullptr});
    rc = st.finish(s);
    (void)hipStreamDestroy(s);
    return rc;
}

int32_t chip_debug_batch_jac_rhs(void *batch, int32_t ndir, const double *x, const double *z, const int32_t *valid,
                                 const double *dq, const double *db, const double *dPx, const double *dAx, double *rx,
                                 double *rz) {
    chip_batch *h = (chip_batch *)batch;
    if (!h || ndir < 1 || ndir > CHIP_BJAC_MAX_DIR || !valid || (h->pd.n && (!x || !rx)) || (h->pd.m && (!z || !rz)))
        return fail(CHIP_ERR_ARG, "chip_debug_batch_jac_rhs: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    int rc;
    dev::SpPattern Psym, Arow, Acol;
    if ((rc = kktsystem_pattern(h->sys, 0, &Psym)) || (rc = kktsystem_pattern(h->sys, 1, &Arow)) ||
        (rc = kktsystem_pattern(h->sys, 2, &Acol)))
        return rc;
    DebugStage st;
    const size_t n = (size_t)h->pd.n, m = (size_t)h->pd.m, nP = (size_t)h->pd.M.nnzP, nA = (size_t)h->pd.M.nnzA;
    const size_t K = (size_t)ndir;
    const double *dx_, *dz_, *ddq, *ddb, *ddP, *ddA;
    const int32_t *dvalid;
    double *drx, *drz;
    if ((rc = st.in(x, n, &dx_)) || (rc = st.in(z, m, &dz_)) || (rc = st.in(valid, (size_t)h->nprob, &dvalid)) ||
        (rc = st.in(dq, K * n, &ddq)) || (rc = st.in(db, K * m, &ddb)) || (rc = st.in(dPx, K * nP, &ddP)) ||
        (rc = st.in(dAx, K * nA, &ddA)) || (rc = st.out(rx, K * n, &drx)) || (rc = st.out(rz, K * m, &drz)))
        return rc;
    hipStream_t s = nullptr;
    CHIP_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    dev::bj_rhs(s, h->plan, Psym, Acol, Arow,
                dev::BjRhs{dev::BtRhs{dvalid, dx_, dz_, ddq, ddb, ddP, ddA, h->pd.d, h->pd.e, h->dc, drx, drz, nullptr,
                                      nullptr, nullptr, nullptr},
                           ndir, n, m, nP, nA, n, m});
    rc = st.finish(s);
    (void)hipStreamDestroy(s);
    return rc;
}

int32_t chip_debug_batch_jac_units(void *batch, int32_t piece, int64_t first, int32_t ndir, const int32_t *valid,
                                   double *rx, double *rz) {
    chip_batch *h = (chip_batch *)batch;
    if (!h || ndir < 1 || ndir > CHIP_BJAC_MAX_DIR || (piece != 0 && piece != 1) || first < 0 || !valid ||
        (h->pd.n && !rx) || (h->pd.m && !rz))
        return fail(CHIP_ERR_ARG, "chip_debug_batch_jac_units: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    int rc;
    DebugStage st;
    const size_t n = (size_t)h->pd.n, m = (size_t)h->pd.m, K = (size_t)ndir;
    const int32_t *dvalid;
    double *drx, *drz;
    if ((rc = st.in(valid, (size_t)h->nprob, &dvalid)) || (rc = st.out(rx, K * n, &drx)) || (rc = st.out(rz, K * m, &drz)))
        return rc;
    hipStream_t s = nullptr;
    CHIP_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    dev::bj_units(s, h->plan,
                  dev::BjUnits{dvalid, h->pd.d, h->pd.e, h->dc, drx, drz, n, m, piece, ndir, (long long)first, nullptr,
                               nullptr, nullptr, nullptr});
    rc = st.finish(s);
    (void)hipStreamDestroy(s);
    return rc;
}

// ---- the passes of a block of cotangents alone (batch_cotangent.hip), or the single launchers once per cotangent
int32_t chip_debug_batch_vjp_rhs(void *batch, int32_t form, int32_t ndir, const double *s, const double *z,
                                 const int32_t *valid, const double *gx, const double *gz, const double *gs, double *rx,
                                 double *ws, double *rz) {
    chip_batch *h = (chip_batch *)batch;
    if (!h || (form != 0 && form != 1) || ndir < 1 || ndir > CHIP_BVJP_MAX_DIR || !valid || (h->pd.n && !rx) ||
        (h->pd.m && (!s || !z || !ws || !rz)))
        return fail(CHIP_ERR_ARG, "chip_debug_batch_vjp_rhs: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    int rc;
    DebugStage st;
    const size_t n = (size_t)h->pd.n, m = (size_t)h->pd.m, K = (size_t)ndir;
    const double *ds_, *dz_, *dgx, *dgz, *dgs;
    const int32_t *dvalid;
    double *drx, *dws, *drz, *dss, *dzs;
    if ((rc = st.in(s, m, &ds_)) || (rc = st.in(z, m, &dz_)) || (rc = st.in(valid, (size_t)h->nprob, &dvalid)) ||
        (rc = st.in(gx, K * n, &dgx)) || (rc = st.in(gz, K * m, &dgz)) || (rc = st.in(gs, K * m, &dgs)) ||
        (rc = st.out(rx, K * n, &drx)) || (rc = st.out(ws, K * m, &dws)) || (rc = st.out(rz, K * m, &drz)) ||
        (rc = st.mem.alloc(&dss, m)) || (rc = st.mem.alloc(&dzs, m)))
        return rc;
    hipStream_t q = nullptr;
    CHIP_HIP(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    if (form == 1) {
        dev::bc_rhs(q, h->plan,
                    dev::BcRhs{dvalid, dgx, dgz, dgs, h->pd.d, h->pd.e, h->dc, ds_, dz_, drx, dws, drz, n, m, m, ndir, dss, dzs});
    } else {
        for (size_t t = 0; t < K; t++)
            dev::ba_rhs(q, h->plan,
                        dev::BaRhs{dvalid, dgx ? dgx + t * n : nullptr, dgz ? dgz + t * m : nullptr,
                                   dgs ? dgs + t * m : nullptr, h->pd.d, h->pd.e, h->dc, ds_, dz_, drx + t * n, dws + t * m,
                                   drz + t * m, dss, dzs});
    }
    rc = st.finish(q);
    (void)hipStreamDestroy(q);
    return rc;
}

int32_t chip_debug_batch_vjp_units(void *batch, int32_t piece, int64_t first, int32_t ndir, const int32_t *valid,
                                   double *rx, double *ws, double *rz) {
    chip_batch *h = (chip_batch *)batch;
    if (!h || ndir < 1 || ndir > CHIP_BVJP_MAX_DIR || piece < 0 || piece > 2 || first < 0 || !valid || (h->pd.n && !rx) ||
        (h->pd.m && (!ws || !rz)))
        return fail(CHIP_ERR_ARG, "chip_debug_batch_vjp_units: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    int rc;
    DebugStage st;
    const size_t n = (size_t)h->pd.n, m = (size_t)h->pd.m, K = (size_t)ndir;
    const int32_t *dvalid;
    double *drx, *dws, *drz;
    if ((rc = st.in(valid, (size_t)h->nprob, &dvalid)) || (rc = st.out(rx, K * n, &drx)) ||
        (rc = st.out(ws, K * m, &dws)) || (rc = st.out(rz, K * m, &drz)))
        return rc;
    hipStream_t q = nullptr;
    CHIP_HIP(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    dev::bc_units(q, h->plan,
                  dev::BcUnits{dvalid, h->pd.d, h->pd.e, h->dc, nullptr, nullptr, drx, dws, drz, n, m, m, piece, ndir,
                               (long long)first, nullptr, nullptr});
    rc = st.finish(q);
    (void)hipStreamDestroy(q);
    return rc;
}

int32_t chip_debug_batch_vjp_out(void *batch, int32_t form, int32_t ndir, int32_t want, const double *x, const double *z,
                                 const int32_t *valid, const double *vx, const double *vz, const double *gs, double *dq,
                                 double *db, double *dP, double *dA) {
    chip_batch *h = (chip_batch *)batch;
    const size_t n = h ? (size_t)h->pd.n : 0, m = h ? (size_t)h->pd.m : 0;
    const size_t nP = h ? (size_t)h->pd.M.nnzP : 0, nA = h ? (size_t)h->pd.M.nnzA : 0;
    if (!h || (form != 0 && form != 1) || ndir < 1 || ndir > CHIP_BVJP_MAX_DIR || want < 1 || want > dev::BC_WANT_ALL ||
        !valid || (n && (!x || !vx)) || (m && (!z || !vz)) || ((want & 1) && n && !dq) || ((want & 2) && m && !db) ||
        ((want & 4) && nP && !dP) || ((want & 8) && nA && !dA))
        return fail(CHIP_ERR_ARG, "chip_debug_batch_vjp_out: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    int rc;
    DebugStage st;
    const size_t K = (size_t)ndir, lens[4] = {n, m, nP, nA};
    const double *dx_, *dz_, *dvx, *dvz, *dgs;
    const int32_t *dvalid;
    double *host[4] = {dq, db, dP, dA}, *o[4], *dux, *duz;
    if ((rc = st.in(x, n, &dx_)) || (rc = st.in(z, m, &dz_)) || (rc = st.in(valid, (size_t)h->nprob, &dvalid)) ||
        (rc = st.in(vx, K * n, &dvx)) || (rc = st.in(vz, K * m, &dvz)) || (rc = st.in(gs, K * m, &dgs)) ||
        (rc = st.mem.alloc(&dux, n)) || (rc = st.mem.alloc(&duz, m)))
        return rc;
    for (int i = 0; i < 4; i++) { // an unwanted piece: the block form gets no buffer, the single launchers a private one
        if ((want >> i) & 1) rc = st.out(host[i], K * lens[i], &o[i]);
        else if (form == 0) rc = st.mem.alloc(&o[i], K * lens[i]);
        else o[i] = nullptr;
        if (rc) return rc;
    }
    hipStream_t q = nullptr;
    CHIP_HIP(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    if (form == 1) {
        const dev::BcGrad g{dvalid, dvx, dvz, dgs, h->pd.d, h->pd.e, h->dc, dx_, dz_, n, m, ndir, want, 0, 0, o[0], o[1],
                            o[2], o[3]};
        dev::bc_grad_vectors(q, h->plan, g);
        dev::bc_grad_matrices(q, h->plan, h->pd.M, g);
    } else {
        for (size_t t = 0; t < K; t++) {
            const dev::BaGrad g{dvalid, dvx + t * n, dvz + t * m, dgs ? dgs + t * m : nullptr, h->pd.d, h->pd.e, h->dc,
                                dx_, dz_, dux, duz, o[0] + t * n, o[1] + t * m, o[2] + t * nP, o[3] + t * nA};
            dev::ba_grad_vectors(q, h->plan, g);
            dev::ba_grad_matrices(q, h->plan, h->pd.M, g);
        }
    }
    rc = st.finish(q);
    (void)hipStreamDestroy(q);
    return rc;
}

static int32_t debug_plan_create(const std::string &fn, const BatchEntry &entry, void **out, int64_t nprob,
                                 const int64_t *n_part, const int64_t *m_part, int64_t ncones, const int32_t *cone_tags,
                                 const int64_t *cone_dims) {
    if (!out) return fail(CHIP_ERR_ARG, fn + ": bad argument");
    *out = nullptr;
    if (nprob < 1 || !n_part || !m_part || ncones < 0 || (ncones && (!cone_tags || !cone_dims)))
        return fail(CHIP_ERR_ARG, fn + ": bad argument");
    if (int rc = batch_cones_supported(entry, ncones, cone_tags)) return rc;
    if (nprob >= (1ll << 31)) return fail(CHIP_ERR_DIM, fn + ": sizes out of int32 range");
    int64_t n = 0, m = 0;
    for (int64_t k = 0; k < nprob; k++) {
        if (n_part[k] < 0 || m_part[k] < 0) return fail(CHIP_ERR_ARG, fn + ": negative part");
        n += n_part[k];
        m += m_part[k];
        if (n >= (1ll << 31) || m >= (1ll << 31) || n + 2 * m >= (1ll << 31))
            return fail(CHIP_ERR_DIM, fn + ": sizes out of int32 range");
    }
    std::unique_ptr<DebugPlan> h(new DebugPlan());
    h->hp.fn = entry.fn;
    std::vector<int64_t> dims2((size_t)ncones, 0);
    if (int rc = host_plan_build(h->hp, nprob, n_part, m_part, n, m, ncones, cone_tags, cone_dims, dims2.data()))
        return rc;
    *out = h.release();
    return CHIP_OK;
}
int32_t chip_debug_bplan_create(void **out, int64_t nprob, const int64_t *n_part, const int64_t *m_part, int64_t ncones,
                                const int32_t *cone_tags, const int64_t *cone_dims) {
    return debug_plan_create("chip_debug_bplan_create", BATCH_ENTRY_BASIC, out, nprob, n_part, m_part, ncones, cone_tags,
                             cone_dims);
}
int32_t chip_debug_bsymplan_create(void **out, int64_t nprob, const int64_t *n_part, const int64_t *m_part,
                                   int64_t ncones, const int32_t *cone_tags, const int64_t *cone_dims) {
    return debug_plan_create("chip_debug_bsymplan_create", BATCH_ENTRY_SYMMETRIC, out, nprob, n_part, m_part, ncones,
                             cone_tags, cone_dims);
}
void chip_debug_bplan_destroy(void *h) { delete (DebugPlan *)h; }

int32_t chip_debug_bplan_get(const void *handle, const char *name, int64_t *len, int32_t *out) {
    const DebugPlan *h = (const DebugPlan *)handle;
    if (!h || !name || !len) return fail(CHIP_ERR_ARG, "chip_debug_bplan_get: bad argument");
    const HostPlan &hp = h->hp;
    const std::string nm(name);
    const std::vector<int> sizes{hp.nprob, hp.n, hp.m, hp.ncx, hp.ncz, (int)hp.it_beg.size()};
    const std::vector<int> degree(hp.degree.begin(), hp.degree.end()); // (at most m each)
    const std::vector<int> psd_sizes{(int)hp.psd_view.size(), (int)hp.psd_diag.size(), hp.psd_total};
    const std::vector<int> *v = nm == "sizes"      ? &sizes
                                : nm == "degree"    ? &degree
                                : nm == "psd_sizes" ? &psd_sizes
                                : nm == "psd_mem"   ? &hp.psd_mem
                                : nm == "psd_start" ? &hp.psd_start
                                : nm == "psd_dim"   ? &hp.psd_dim
                                : nm == "psd_view"  ? &hp.psd_view
                                : nm == "psd_first" ? &hp.psd_first
                                : nm == "psd_diag"  ? &hp.psd_diag
                                : nm == "xoff"     ? &hp.xoff
                                : nm == "zoff"     ? &hp.zoff
                                : nm == "xmem"     ? &hp.xmem
                                : nm == "zmem"     ? &hp.zmem
                                : nm == "ch_beg"   ? &hp.ch_beg
                                : nm == "ch_end"   ? &hp.ch_end
                                : nm == "cx_first" ? &hp.cx_first
                                : nm == "cz_first" ? &hp.cz_first
                                : nm == "it_beg"   ? &hp.it_beg
                                : nm == "it_end"   ? &hp.it_end
                                : nm == "it_type"  ? &hp.it_type
                                : nm == "it_first" ? &hp.it_first
                                : nm == "rtype"    ? &hp.rtype
                                                   : nullptr;
    if (!v) return fail(CHIP_ERR_ARG, "chip_debug_bplan_get: unknown name");
    *len = (int64_t)v->size();
    if (out && !v->empty()) std::memcpy(out, v->data(), v->size() * sizeof(int));
    return CHIP_OK;
}

int32_t chip_debug_bplan_seg_reduce(void *handle, int32_t count, const int32_t *kind, const int32_t *space,
                                    const int32_t *slot, const double *const *a, const double *const *b,
                                    int32_t nslots, double *out) {
    DebugPlan *h = (DebugPlan *)handle;
    if (!h || count < 0 || count > dev::SEG_MAX || nslots < 0 || (count && (!kind || !space || !slot || !a || !b || !out)))
        return fail(CHIP_ERR_ARG, "chip_debug_bplan_seg_reduce: bad argument");
    for (int j = 0; j < count; j++)
        if (kind[j] < dev::SEG_DOT || kind[j] > dev::SEG_NONFINITE || (space[j] != 0 && space[j] != 1) || slot[j] < 0 ||
            slot[j] >= nslots || !a[j] || (!b[j] && (kind[j] == dev::SEG_DOT || kind[j] == dev::SEG_WSQ)))
            return fail(CHIP_ERR_ARG, "chip_debug_bplan_seg_reduce: bad spec");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugStage st;
    dev::SegBatch bt{};
    bt.count = count;
    for (int j = 0; j < count; j++) {
        const size_t len = space[j] ? (size_t)h->hp.m : (size_t)h->hp.n;
        const double *da, *db;
        if ((rc = st.in(a[j], len, &da)) || (rc = st.in(b[j], len, &db))) return rc;
        bt.s[j] = dev::SegSpec{da, db, kind[j], space[j], slot[j]};
    }
    double *dout;
    if ((rc = st.out(out, (size_t)nslots * h->hp.nprob, &dout))) return rc;
    dev::seg_reduce(h->stream, h->plan, bt, dout, h->seg_scr);
    return st.finish(h->stream);
}

int32_t chip_debug_bplan_cone_minima(void *handle, int32_t op, const double *dz, const double *ds, const double *z,
                                     const double *sv, const double *amax, double *out_min, double *out_sum_or_null) {
    DebugPlan *h = (DebugPlan *)handle;
    const bool step = op == dev::CONE_STEP;
    if (!h || op < dev::CONE_STEP || op > dev::CONE_INTERIOR || !z || !out_min || (step && (!dz || !ds || !sv || !amax)) ||
        (op == dev::CONE_INTERIOR && !sv))
        return fail(CHIP_ERR_ARG, "chip_debug_bplan_cone_minima: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugStage st;
    const size_t m = (size_t)h->hp.m, np = (size_t)h->hp.nprob;
    const double *ddz, *dds, *dzz, *dsv, *dam;
    double *dmin, *dsum;
    if ((rc = st.in(dz, m, &ddz)) || (rc = st.in(ds, m, &dds)) || (rc = st.in(z, m, &dzz)) || (rc = st.in(sv, m, &dsv)) ||
        (rc = st.in(amax, np, &dam)) || (rc = st.out(out_min, np, &dmin)) || (rc = st.out(out_sum_or_null, np, &dsum)))
        return rc;
    dev::cone_minima(h->stream, h->plan, op, ddz, dds, dzz, dsv, dam, dmin, dsum, h->cone_scr);
    return st.finish(h->stream);
}

int32_t chip_debug_bplan_blin(void *handle, double *w, const double *x, const double *y, const double *sa,
                              const double *sb, double ca, double cb, int32_t space, const int32_t *mask,
                              int32_t mask_mode) {
    DebugPlan *h = (DebugPlan *)handle;
    if (!h || !w || !x || (space != 0 && space != 1) || mask_mode < dev::MASK_ZERO || mask_mode > dev::MASK_KEEP ||
        (mask && mask_mode == dev::MASK_Y && !y))
        return fail(CHIP_ERR_ARG, "chip_debug_bplan_blin: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugStage st;
    const size_t len = space ? (size_t)h->hp.m : (size_t)h->hp.n, np = (size_t)h->hp.nprob;
    double *dw;
    const double *dx, *dy, *dsa, *dsb;
    const int *dmask;
    if ((rc = st.out(w, len, &dw)) || (rc = st.in(x, len, &dx)) || (rc = st.in(y, len, &dy)) ||
        (rc = st.in(sa, np, &dsa)) || (rc = st.in(sb, np, &dsb)) || (rc = st.in((const int *)mask, np, &dmask)))
        return rc;
    dev::blin(h->stream, h->plan, dev::BLin{dw, dx, dy, dsa, dsb, ca, cb, space, dmask, mask_mode});
    return st.finish(h->stream);
}

int32_t chip_debug_bplan_bresid(void *handle, double *rx, const double *rx_inf, const double *Px, const double *q,
                                double *rz, const double *rz_inf, const double *b, const double *tau) {
    DebugPlan *h = (DebugPlan *)handle;
    if (!h || !rx || !rx_inf || !Px || !q || !rz || !rz_inf || !b || !tau)
        return fail(CHIP_ERR_ARG, "chip_debug_bplan_bresid: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugStage st;
    const size_t n = (size_t)h->hp.n, m = (size_t)h->hp.m, np = (size_t)h->hp.nprob;
    double *drx, *drz;
    const double *drxi, *dPx, *dq, *drzi, *db, *dtau;
    if ((rc = st.out(rx, n, &drx)) || (rc = st.in(rx_inf, n, &drxi)) || (rc = st.in(Px, n, &dPx)) ||
        (rc = st.in(q, n, &dq)) || (rc = st.out(rz, m, &drz)) || (rc = st.in(rz_inf, m, &drzi)) ||
        (rc = st.in(b, m, &db)) || (rc = st.in(tau, np, &dtau)))
        return rc;
    dev::bresid(h->stream, h->plan, drx, drxi, dPx, dq, drz, drzi, db, dtau);
    return st.finish(h->stream);
}

int32_t chip_debug_bplan_bunit_shift(void *handle, double *z, const double *alpha, int32_t primal,
                                     const int32_t *mask) {
    DebugPlan *h = (DebugPlan *)handle;
    if (!h || !z || !alpha) return fail(CHIP_ERR_ARG, "chip_debug_bplan_bunit_shift: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugStage st;
    double *dz;
    const double *dal;
    const int *dmask;
    if ((rc = st.out(z, (size_t)h->hp.m, &dz)) || (rc = st.in(alpha, (size_t)h->hp.nprob, &dal)) ||
        (rc = st.in((const int *)mask, (size_t)h->hp.nprob, &dmask)))
        return rc;
    dev::bunit_shift(h->stream, h->plan, dz, dal, primal, dmask);
    return st.finish(h->stream);
}

int32_t chip_debug_bplan_bunit_reset(void *handle, double *x, double *sv, double *z, const int32_t *flag) {
    DebugPlan *h = (DebugPlan *)handle;
    if (!h || !x || !sv || !z || !flag) return fail(CHIP_ERR_ARG, "chip_debug_bplan_bunit_reset: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugStage st;
    double *dx, *dsv, *dz;
    const int *dflag;
    if ((rc = st.out(x, (size_t)h->hp.n, &dx)) || (rc = st.out(sv, (size_t)h->hp.m, &dsv)) ||
        (rc = st.out(z, (size_t)h->hp.m, &dz)) || (rc = st.in((const int *)flag, (size_t)h->hp.nprob, &dflag)))
        return rc;
    dev::bunit_reset(h->stream, h->plan, dx, dsv, dz, dflag);
    return st.finish(h->stream);
}

int32_t chip_debug_bplan_bunscale(void *handle, double *xo, const double *x, const double *d, double *zo,
                                  const double *z, const double *e, double *so, const double *sv, const double *einv,
                                  const double *sx, const double *sz) {
    DebugPlan *h = (DebugPlan *)handle;
    if (!h || !xo || !x || !d || !zo || !z || !e || !so || !sv || !einv || !sx || !sz)
        return fail(CHIP_ERR_ARG, "chip_debug_bplan_bunscale: bad argument");
    int rc;
    if ((rc = h->ready())) return rc;
    DebugStage st;
    const size_t n = (size_t)h->hp.n, m = (size_t)h->hp.m, np = (size_t)h->hp.nprob;
    double *dxo, *dzo, *dso;
    const double *dx, *dd, *dz, *de, *dsv, *dei, *dsx, *dsz;
    if ((rc = st.out(xo, n, &dxo)) || (rc = st.in(x, n, &dx)) || (rc = st.in(d, n, &dd)) || (rc = st.out(zo, m, &dzo)) ||
        (rc = st.in(z, m, &dz)) || (rc = st.in(e, m, &de)) || (rc = st.out(so, m, &dso)) || (rc = st.in(sv, m, &dsv)) ||
        (rc = st.in(einv, m, &dei)) || (rc = st.in(sx, np, &dsx)) || (rc = st.in(sz, np, &dsz)))
        return rc;
    dev::bunscale(h->stream, h->plan, dxo, dx, dd, dzo, dz, de, dso, dsv, dei, dsx, dsz);
    return st.finish(h->stream);
}

// ---- the re-equilibration's load pass (reequilibrate.hip: re_load) alone, and the create counters
int32_t chip_debug_reload_pass(double *dst, double *raw_or_null, const double *src, int64_t len, int32_t cap,
                               int32_t misalign) {
    if (!dst || !src || len < 0 || len >= (1ll << 31) || misalign < 0 || misalign > 7)
        return fail(CHIP_ERR_ARG, "chip_debug_reload_pass: bad argument");
    if (chip_device_count() < 1) return fail(CHIP_ERR_NO_DEVICE, "chip_debug_reload_pass: no HIP device");
    const size_t n = (size_t)len, full = n + 4;
    DevPool mem;
    double *ddst, *draw = nullptr, *dsrc;
    int rc;
    if ((rc = mem.upload(&ddst, dst, full)) || (rc = mem.alloc(&dsrc, full))) return rc;
    if (raw_or_null && (rc = mem.upload(&draw, raw_or_null, full))) return rc;
    const size_t od = misalign & 1 ? 1 : 2, orw = misalign & 2 ? 1 : 2, os = misalign & 4 ? 1 : 2;
    if (n) CHIP_HIP(hipMemcpy(dsrc + os, src, n * 8, hipMemcpyHostToDevice));
    dev::re_load(nullptr, ddst + od, draw ? draw + orw : nullptr, dsrc + os, (int)len, cap != 0);
    CHIP_HIP(hipGetLastError());
    CHIP_HIP(hipDeviceSynchronize());
    CHIP_HIP(hipMemcpy(dst, ddst, full * 8, hipMemcpyDeviceToHost));
    if (draw) CHIP_HIP(hipMemcpy(raw_or_null, draw, full * 8, hipMemcpyDeviceToHost));
    return CHIP_OK;
}

int32_t chip_debug_create_count(int32_t which, double *out) {
    if (which < 0 || which > 1 || !out) return fail(CHIP_ERR_ARG, "chip_debug_create_count: bad argument");
    *out = (double)create_count(which);
    return CHIP_OK;
}
#endif
