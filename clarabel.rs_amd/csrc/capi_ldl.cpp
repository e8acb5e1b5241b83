// capi_ldl.cpp -- chip_ldl_*: DirectLDLSolver<f64> (quasidef/mod.rs:14-26; behaviour of ldlsolvers/qdldl.rs) and the
// fast path of the strict drop-in (registered index sets, device-resident refinement, pinned caller buffers)
#include <memory>

#include "kkt_handle.hpp"

using namespace chip;

namespace {

// ---- L1 fast path (round 5): registered index sets, device-resident refinement, pinned caller buffers -----------------
// The strict drop-in moved 352 MB over PCIe per interior-point iteration of config 3 (all of K.nzval per refactor, b and x
// of every LDL' solve of every refinement round).  What the reference's DirectLDLKKTSolver actually changes per
// iteration are the entries of a few fixed index vectors (directldlkktsolver.rs:143,245; datamaps.rs:213-219), and its
// refinement (:266-321) needs nothing from the host but b.
int ldl_values_to_device(chip_ldl *h) { // first direct update: the device copy becomes the caller's K.nzval
    Engine &E = h->E;
    if (h->dev_values) return CHIP_OK;
    if (h->dirty && E.nnzK) {
        int rc = E.upload_values(h->hK.data());
        if (rc) return rc;
    }
    h->dev_values = true;
    return CHIP_OK;
}
int ldl_stage(chip_ldl *h, i64 k) {
    if (k <= h->d_vals_cap) return CHIP_OK;
    int rc = h->E.alloc(&h->d_vals, (size_t)k); // (the engine frees it with the handle; earlier, smaller ones too)
    if (rc) return rc;
    h->d_vals_cap = k;
    return CHIP_OK;
}
// a plain (index-carrying) update on a handle whose device copy is authoritative: index translated and shipped each time
int ldl_plain_on_device(chip_ldl *h, int kind, const uint64_t *index, const double *values, double scalar,
                        const int8_t *signs, int64_t k) {
    Engine &E = h->E;
    NEED_DEVICE(E);
    if (k <= 0) return CHIP_OK;
    CHIP_HIP(hipSetDevice(E.device));
    std::vector<i32> pos((size_t)k);
    for (i64 i = 0; i < k; i++) {
        if (index[i] >= (uint64_t)E.nnzK) return fail(CHIP_ERR_ARG, "values update: index out of range");
        pos[(size_t)i] = E.h_k2v[(size_t)index[i]];
    }
    int *dpos = nullptr;
    int8_t *dsg = nullptr;
    int rc = CHIP_OK;
    // (every HIP call checked; the two temporaries are released on every path)
    auto hipok = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == CHIP_OK) rc = fail(CHIP_ERR_HIP, hip_err(e, what));
        return e == hipSuccess;
    };
    if (hipok(hipMalloc((void **)&dpos, (size_t)k * sizeof(int)), "values update: index buffer") &&
        hipok(hipMemcpyAsync(dpos, pos.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice, E.stream), "values update: index copy")) {
        if (kind == 0) {
            if ((rc = ldl_stage(h, k)) == CHIP_OK &&
                hipok(hipMemcpyAsync(h->d_vals, values, (size_t)k * sizeof(double), hipMemcpyHostToDevice, E.stream), "values update: value copy"))
                dev::scatter_values(E.stream, E.Kx, dpos, h->d_vals, (int)k, 1.0);
        } else if (kind == 1) {
            dev::scale_values(E.stream, E.Kx, dpos, (int)k, scalar);
        } else if (hipok(hipMalloc((void **)&dsg, (size_t)k), "values update: sign buffer") &&
                   hipok(hipMemcpyAsync(dsg, signs, (size_t)k, hipMemcpyHostToDevice, E.stream), "values update: sign copy")) {
            dev::offset_values(E.stream, E.Kx, dpos, dsg, (int)k, scalar);
        }
        (void)hipok(hipGetLastError(), "values update: launch");
    }
    (void)hipok(hipStreamSynchronize(E.stream), "values update: synchronise");
    if (dpos) (void)hipFree(dpos);
    if (dsg) (void)hipFree(dsg);
    E.sx_valid = false;
    h->dirty = true;
    return rc;
}
int ldl_set_of(chip_ldl *h, int32_t id, chip_ldl::IndexSet **st) {
    if (!h || id < 0 || (size_t)id >= h->sets.size()) return fail(CHIP_ERR_ARG, "unknown index set");
    *st = &h->sets[(size_t)id];
    return CHIP_OK;
}

} // namespace

extern "C" {

int32_t chip_ldl_create(chip_ldl **out, int64_t n, const uint64_t *colptr, const uint64_t *rowval,
                        const double *nzval, const int8_t *dsigns, const uint64_t *perm_or_null,
                        const chip_settings *settings) {
    if (!out || n < 0 || !colptr || !rowval || !nzval) return fail(CHIP_ERR_ARG, "chip_ldl_create: bad argument");
    *out = nullptr;
    switches_reload(); // the CHIP_* diagnostic switches are read from the environment here, never in a launch loop
    chip_settings st;
    if (settings) st = *settings;
    else chip_settings_default(&st);
    std::vector<i64> perm0;
    if (perm_or_null) perm0.assign(as_i64(perm_or_null), as_i64(perm_or_null) + n);
    Symbolic S;
    // (target_wg = 0: L1 handles never take the fused launches, so a forest is not cut finer for them -- the grouped
    // fold's extra top nodes would only add level-scheduled launches to every solve)
    int rc = analyse(n, as_i64(colptr), as_i64(rowval), dsigns, perm0, st.amd_dense_scale, S, 0);
    if (rc) return rc;
    std::unique_ptr<chip_ldl> h(new chip_ldl());
    h->hK.assign(nzval, nzval + S.nnzK);
    if (st.device == CHIP_DEVICE_HOST_ONLY) {
        h->E.init_host_only(S, st);
        *out = h.release();
        return CHIP_OK;
    }
    rc = h->E.init(S, st);
    if (rc) return rc;
    h->dirty = true;
    if ((rc = h->E.alloc(&h->d_b, (size_t)n))) return rc;
    if ((rc = h->E.alloc(&h->d_x, (size_t)n))) return rc;
    if ((rc = h->E.alloc(&h->d_y, (size_t)n))) return rc;
    *out = h.release();
    return CHIP_OK;
}

void chip_ldl_destroy(chip_ldl *h) { delete h; }

int32_t chip_ldl_update_values(chip_ldl *h, const uint64_t *index, const double *values, int64_t k) {
    if (!h) return CHIP_ERR_ARG;
    if (h->dev_values) return ldl_plain_on_device(h, 0, index, values, 0.0, nullptr, k);
    for (i64 i = 0; i < k; i++) {
        if (index[i] >= (uint64_t)h->E.nnzK) return fail(CHIP_ERR_ARG, "update_values: index out of range");
        h->hK[index[i]] = values[i];
    }
    h->dirty = true;
    return CHIP_OK;
}
int32_t chip_ldl_scale_values(chip_ldl *h, const uint64_t *index, double scale, int64_t k) {
    if (!h) return CHIP_ERR_ARG;
    if (h->dev_values) return ldl_plain_on_device(h, 1, index, nullptr, scale, nullptr, k);
    for (i64 i = 0; i < k; i++) {
        if (index[i] >= (uint64_t)h->E.nnzK) return fail(CHIP_ERR_ARG, "scale_values: index out of range");
        h->hK[index[i]] *= scale;
    }
    h->dirty = true;
    return CHIP_OK;
}
int32_t chip_ldl_offset_values(chip_ldl *h, const uint64_t *index, double offset, const int8_t *signs,
                               int64_t k) {
    if (!h) return CHIP_ERR_ARG;
    if (h->dev_values) return ldl_plain_on_device(h, 2, index, nullptr, offset, signs, k);
    for (i64 i = 0; i < k; i++) {
        if (index[i] >= (uint64_t)h->E.nnzK) return fail(CHIP_ERR_ARG, "offset_values: index out of range");
        if (signs[i] > 0) h->hK[index[i]] += offset;
        else if (signs[i] < 0) h->hK[index[i]] -= offset;
    }
    h->dirty = true;
    return CHIP_OK;
}
int32_t chip_ldl_set_values(chip_ldl *h, const double *kkt_nzval) {
    if (!h || !kkt_nzval) return CHIP_ERR_ARG;
    std::memcpy(h->hK.data(), kkt_nzval, (size_t)h->E.nnzK * sizeof(double));
    h->dirty = true;
    h->dev_values = false; // (the host mirror is the caller's K.nzval again; the next refactor uploads it)
    return CHIP_OK;
}

int32_t chip_ldl_get_symbolic(const chip_ldl *h, uint64_t *etree, uint64_t *Lp, uint64_t *Li,
                              uint64_t *lvlptr) {
    if (!h) return CHIP_ERR_ARG;
    return h->E.get_symbolic(etree, Lp, Li, lvlptr);
}

int32_t chip_ldl_refactor(chip_ldl *h) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if (h->dirty && !h->dev_values && E.nnzK) {
        int rc = E.upload_values(h->hK.data());
        if (rc) return rc;
    }
    h->dirty = false;
    return E.refactor(false, nullptr);
}
int32_t chip_ldl_solve_dev(chip_ldl *h, double *x_dev, const double *b_dev) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    if (!E.factored) return fail(CHIP_ERR_NOT_FACTORED, "solve() before the first refactor()");
    CHIP_HIP(hipSetDevice(E.device));
    dev::permute_in(E.stream, h->d_y, b_dev, E.perm, E.N);
    E.enqueue_solve_inplace(E.ctx[0], h->d_y);
    dev::permute_out(E.stream, x_dev, h->d_y, E.perm, E.N);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_ldl_solve(chip_ldl *h, double *x, const double *b) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    if (!E.factored) return fail(CHIP_ERR_NOT_FACTORED, "solve() before the first refactor()");
    CHIP_HIP(hipSetDevice(E.device));
    const size_t bytes = (size_t)E.N * sizeof(double);
    if (E.N) CHIP_HIP(hipMemcpyAsync(h->d_b, b, bytes, hipMemcpyHostToDevice, E.stream));
    int rc = chip_ldl_solve_dev(h, h->d_x, h->d_b);
    if (rc) return rc;
    if (E.N) CHIP_HIP(hipMemcpyAsync(x, h->d_x, bytes, hipMemcpyDeviceToHost, E.stream));
    CHIP_HIP(hipStreamSynchronize(E.stream));
    return CHIP_OK;
}
int32_t chip_ldl_info(const chip_ldl *h, chip_info *info) {
    if (!h || !info) return CHIP_ERR_ARG;
    fill_info(h->E, info);
    if (h->E.factored && !h->E.host_only) {
        i64 c = 0;
        int rc = count_positive(const_cast<Engine &>(h->E), &c);
        if (rc) return rc;
        info->positive_inertia = c;
    }
    return CHIP_OK;
}
int32_t chip_ldl_get_perm(const chip_ldl *h, uint64_t *perm) {
    if (!h || !perm) return CHIP_ERR_ARG;
    for (int i = 0; i < h->E.N; i++) perm[i] = (uint64_t)h->E.h_perm[i];
    return CHIP_OK;
}
int32_t chip_ldl_get_supernodes(const chip_ldl *h, int64_t *count, uint64_t *ptr, uint64_t *cols) {
    return h ? get_supernodes(h->E, count, ptr, cols) : CHIP_ERR_ARG;
}
int32_t chip_ldl_get_factors(chip_ldl *h, uint64_t *Lp, uint64_t *Li, double *Lx, double *D, double *Dinv) {
    if (!h) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    CHIP_HIP(hipStreamSynchronize(E.stream));
    const size_t n = (size_t)E.N, nl = (size_t)E.nnzL;
    std::vector<int> tmp;
    if (Lp) {
        tmp.resize(n + 1);
        CHIP_HIP(hipMemcpy(tmp.data(), E.Lp, (n + 1) * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i <= n; i++) Lp[i] = (uint64_t)tmp[i];
    }
    if (Li && nl) {
        tmp.resize(nl);
        CHIP_HIP(hipMemcpy(tmp.data(), E.Li, nl * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nl; i++) Li[i] = (uint64_t)tmp[i];
    }
    if (Lx && nl) CHIP_HIP(hipMemcpy(Lx, E.Lx, nl * sizeof(double), hipMemcpyDeviceToHost));
    if (D && n) CHIP_HIP(hipMemcpy(D, E.D, n * sizeof(double), hipMemcpyDeviceToHost));
    if (Dinv && n) CHIP_HIP(hipMemcpy(Dinv, E.Dinv, n * sizeof(double), hipMemcpyDeviceToHost));
    return CHIP_OK;
}

int32_t chip_ldl_register_index(chip_ldl *h, const uint64_t *index, int64_t k, const int8_t *signs_or_null, int32_t *id_out) {
    if (!h || !id_out || k < 0 || (k > 0 && !index)) return fail(CHIP_ERR_ARG, "chip_ldl_register_index: bad argument");
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    std::vector<i32> pos((size_t)k);
    for (i64 i = 0; i < k; i++) {
        if (index[i] >= (uint64_t)E.nnzK) return fail(CHIP_ERR_ARG, "chip_ldl_register_index: index out of range");
        pos[(size_t)i] = E.h_k2v[(size_t)index[i]];
    }
    chip_ldl::IndexSet st;
    st.k = k;
    int rc;
    if ((rc = E.upload(&st.pos, pos, (size_t)k))) return rc;
    if (signs_or_null) {
        std::vector<int8_t> sg(signs_or_null, signs_or_null + k);
        if ((rc = E.upload(&st.signs, sg, (size_t)k))) return rc;
    }
    h->sets.push_back(st);
    *id_out = (int32_t)h->sets.size() - 1;
    return CHIP_OK;
}
int32_t chip_ldl_update_values_id(chip_ldl *h, int32_t id, const double *values) {
    chip_ldl::IndexSet *st;
    int rc = ldl_set_of(h, id, &st);
    if (rc) return rc;
    Engine &E = h->E;
    NEED_DEVICE(E);
    if (st->k == 0) return CHIP_OK;
    if (!values) return CHIP_ERR_ARG;
    CHIP_HIP(hipSetDevice(E.device));
    if ((rc = ldl_values_to_device(h))) return rc;
    if ((rc = ldl_stage(h, st->k))) return rc;
    CHIP_HIP(hipMemcpyAsync(h->d_vals, values, (size_t)st->k * sizeof(double), hipMemcpyHostToDevice, E.stream));
    dev::scatter_values(E.stream, E.Kx, st->pos, h->d_vals, (int)st->k, 1.0);
    // (the caller may reuse `values` at once: the reference's update_values copies; a pinned source is read by the DMA
    // engine asynchronously, so wait for the copy -- not for the kernel)
    CHIP_HIP(hipStreamSynchronize(E.stream));
    E.sx_valid = false;
    h->dirty = true;
    return CHIP_OK;
}
int32_t chip_ldl_scale_values_id(chip_ldl *h, int32_t id, double scale) {
    chip_ldl::IndexSet *st;
    int rc = ldl_set_of(h, id, &st);
    if (rc) return rc;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if ((rc = ldl_values_to_device(h))) return rc;
    dev::scale_values(E.stream, E.Kx, st->pos, (int)st->k, scale);
    E.sx_valid = false;
    h->dirty = true;
    return CHIP_OK;
}
int32_t chip_ldl_offset_values_id(chip_ldl *h, int32_t id, double offset) {
    chip_ldl::IndexSet *st;
    int rc = ldl_set_of(h, id, &st);
    if (rc) return rc;
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    if ((rc = ldl_values_to_device(h))) return rc;
    dev::offset_values(E.stream, E.Kx, st->pos, st->signs, (int)st->k, offset);
    E.sx_valid = false;
    h->dirty = true;
    return CHIP_OK;
}
int32_t chip_ldl_pin_buffer(chip_ldl *h, void *ptr, uint64_t bytes) {
    if (!h || !ptr || !bytes) return CHIP_ERR_ARG;
    NEED_DEVICE(h->E);
    CHIP_HIP(hipSetDevice(h->E.device));
    for (void *p : h->pinned)
        if (p == ptr) return CHIP_OK;
    CHIP_HIP(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
    h->pinned.push_back(ptr);
    return CHIP_OK;
}
// solve + iterative refinement of directldlkktsolver.rs:266-321 with the handle's CURRENT values as K (the caller has
// restored the unregularised diagonal after refactor, :255-261): b in, x out, everything in between on the device
int32_t chip_ldl_solve_refined(chip_ldl *h, double *x, const double *b, const chip_settings *ir_settings, int32_t *iterations) {
    if (!h || !x || !b) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    if (!E.factored) return fail(CHIP_ERR_NOT_FACTORED, "solve() before the first refactor()");
    CHIP_HIP(hipSetDevice(E.device));
    int rc;
    const size_t N = (size_t)E.N;
    SolveVecs &r = h->r;
    if (!r.bp && (rc = r.alloc(E, N))) return rc;
    if (h->dirty && !h->dev_values && E.nnzK) { // plain updates since the refactor (the restored diagonal): the residual reads them
        if ((rc = E.upload_values(h->hK.data()))) return rc;
        E.sx_valid = false;
        h->dirty = false;
    }
    struct RestoreSettings { // (every return below leaves the handle with its own refinement settings)
        Engine &E;
        chip_settings saved;
        ~RestoreSettings() { E.st = saved; }
    } restore{E, E.st};
    if (ir_settings) copy_refinement_settings(E.st, *ir_settings);
    if (N) CHIP_HIP(hipMemcpyAsync(h->d_b, b, N * sizeof(double), hipMemcpyHostToDevice, E.stream));
    SolveCtx &c = E.ctx[0];
    if ((rc = E.zero_norm_sets(c))) return rc;
    dev::permute_in(E.stream, r.bp, h->d_b, E.perm, E.N);
    if (N) CHIP_HIP(hipMemcpyAsync(r.x, r.bp, N * sizeof(double), hipMemcpyDeviceToDevice, E.stream));
    dev::norm_inf(E.stream, r.bp, E.N, c.norm_set(0), c.norm_nan(0));
    E.enqueue_solve_inplace(c, r.x);
    int its = 0;
    const int ok = refine_core(E, c, r.bp, r.x, r.e, r.dx, its);
    if (ok == 0) (void)E.sweeps_after_failure(); // (stale barrier words must not outlive a failed solve)
    if (iterations) *iterations = its;
    if (ok != 1) return ok;
    dev::permute_out(E.stream, h->d_x, r.x, E.perm, E.N);
    if (N) CHIP_HIP(hipMemcpyAsync(x, h->d_x, N * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    CHIP_HIP(hipStreamSynchronize(E.stream));
    return 1;
}

} // extern "C"
