// host_util.hpp -- host-side helpers the L3 / L4 handles share (kktsystem.cpp, solver.cpp, batch.cpp): the owning pool
// of device allocations, and the front end of the data updates (chip_problem_update_* of chip_solver, chip_bdata_update_*
// of chip_batch): argument check, staging of the host forms, the ABI wrappers, the settings validator.  The problem data
// the two L4 handles are set up with, and whose length an update is checked against, is problem_data.hpp's.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "engine.hpp"

namespace chip {

// device allocations freed together with their owner; a zero-length request still yields a valid pointer
struct DevPool {
    std::vector<void *> ptrs;
    template <typename T> int alloc(T **dst, size_t n) {
        *dst = nullptr;
        void *p = nullptr;
        CHIP_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        ptrs.push_back(p);
        *dst = (T *)p;
        return CHIP_OK;
    }
    template <typename T> int upload(T **dst, const T *src, size_t n) {
        int rc = alloc(dst, n);
        if (rc) return rc;
        if (n) CHIP_HIP(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
        return CHIP_OK;
    }
    template <typename T> int upload(T **dst, const std::vector<T> &src) { return upload(dst, src.data(), src.size()); }
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() {
        for (void *p : ptrs) (void)hipFree(p);
    }
};

// a device buffer that grows on demand.  Work enqueued earlier may still read the old buffer, so the stream is
// synchronised before it is freed (counted in *syncs when given)
template <typename T> int grow_dev(T **buf, size_t *cap, size_t need, hipStream_t stream, long *syncs = nullptr) {
    if (need <= *cap) return CHIP_OK;
    if (*buf) {
        CHIP_HIP(hipStreamSynchronize(stream));
        if (syncs) ++*syncs;
        (void)hipFree(*buf);
        *buf = nullptr;
        *cap = 0;
    }
    CHIP_HIP(hipMalloc((void **)buf, need * sizeof(T)));
    *cap = need;
    return CHIP_OK;
}

#ifdef CHIP_TESTING
// test build only: how often chip_kkt_create (0) and chip_kktsystem_create (1) were entered in this process
// (chip_debug_create_count: a re-equilibration must make neither)
inline long &create_count(int which) {
    static long counts[2] = {0, 0};
    return counts[which];
}
#endif

// ---- the data updates' front end ------------------------------------------------------------------------------------
enum { UPD_P = 0, UPD_A = 1, UPD_Q = 2, UPD_B = 3 };
// the entry point's name in error texts: prefix "chip_problem_update_" or "chip_bdata_update_" + P / A / q / b
inline std::string update_fn(const char *prefix, int which) { return std::string(prefix) + "PAqb"[which]; }

// the staging of the host forms: the values and (partial forms) the indices, uploaded on the handle's stream
struct UpdateStage {
    double *v = nullptr;
    int64_t *i = nullptr;
    size_t v_cap = 0, i_cap = 0;
    // launches / syncs (when given) count the copies enqueued and the synchronisations of a growth
    int upload(hipStream_t s, const uint64_t *idx, const double *vals, size_t k, long *launches = nullptr,
               long *syncs = nullptr) {
        int rc;
        if ((rc = grow_dev(&v, &v_cap, k, s, syncs))) return rc;
        if (idx && (rc = grow_dev(&i, &i_cap, k, s, syncs))) return rc;
        CHIP_HIP(hipMemcpyAsync(v, vals, k * sizeof(double), hipMemcpyHostToDevice, s));
        // (an index past 2^63 - 1 reads as negative and is refused like any other out-of-range index)
        if (idx) CHIP_HIP(hipMemcpyAsync(i, idx, k * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (launches) *launches += idx ? 2 : 1;
        return CHIP_OK;
    }
    // the host form of a re-equilibration: the four arrays P, q, A, b one after the other in v, each starting on a
    // 16-byte boundary; at[j]: where array j went.  One enqueue per non-empty array
    int upload4(hipStream_t s, const double *const src[4], const size_t len[4], const double *at[4],
                long *launches = nullptr, long *syncs = nullptr) {
        size_t off[4], total = 0;
        for (int j = 0; j < 4; j++) {
            off[j] = total;
            total += (len[j] + 1) & ~(size_t)1;
        }
        if (int rc = grow_dev(&v, &v_cap, std::max<size_t>(total, 2), s, syncs)) return rc;
        for (int j = 0; j < 4; j++) {
            at[j] = v + off[j];
            if (!len[j]) continue;
            CHIP_HIP(hipMemcpyAsync(v + off[j], src[j], len[j] * sizeof(double), hipMemcpyHostToDevice, s));
            if (launches) ++*launches;
        }
        return CHIP_OK;
    }
    UpdateStage() = default;
    UpdateStage(const UpdateStage &) = delete;
    UpdateStage &operator=(const UpdateStage &) = delete;
    ~UpdateStage() { // (the owner has synchronised its stream)
        (void)hipFree(v);
        (void)hipFree(i);
    }
};

// the checks of every update entry point, both forms: CHIP_ERR_ARG before any device is touched, k == 0 a no-op
// (returns 1), the 2^31 limit, the full form's length (len: the target's).  gate() runs between the argument check
// and the rest, on a handle that is not null: what the handle itself refuses or resets on every call
template <typename Gate>
int update_args(const std::string &fn, const void *h, const void *idx, const double *vals, int64_t k, int64_t len,
                Gate gate) {
    if (!h || k < 0 || (k > 0 && !vals)) return fail(CHIP_ERR_ARG, fn + ": bad argument");
    if (int rc = gate()) return rc;
    if (k == 0) return 1;
    if (k >= (1ll << 31)) return fail(CHIP_ERR_DIM, fn + ": more than 2^31 values");
    if (!idx && k != len) return fail(CHIP_ERR_DIM, fn + ": the full form needs one value per entry");
    return 0;
}

// the two forms of one update of handle type H, which provides: static update_args(h, which, idx, vals, k) (the check
// above with the handle's own refusals), pd (its ProblemData, for the device), stage_upload(idx, vals, k)
// (UpdateStage::upload on its stream with its counters), stage and update(which, idx_dev, vals_dev, k)
template <typename H> int update_host(H *h, int which, const uint64_t *idx, const double *vals, int64_t k) {
    int rc = H::update_args(h, which, idx, vals, k);
    if (rc) return rc < 0 ? rc : CHIP_OK;
    CHIP_HIP(hipSetDevice(h->pd.device));
    if ((rc = h->stage_upload(idx, vals, (size_t)k))) return rc;
    return h->update(which, idx ? h->stage.i : nullptr, h->stage.v, (int)k);
}
template <typename H> int update_dev(H *h, int which, const int64_t *idx, const double *vals, int64_t k) {
    int rc = H::update_args(h, which, idx, vals, k);
    if (rc) return rc < 0 ? rc : CHIP_OK;
    CHIP_HIP(hipSetDevice(h->pd.device));
    return h->update(which, idx, vals, (int)k);
}

// the eight exported entry points of one handle type: prefix##P / A / q / b and their _dev forms
#define CHIP_UPDATE_ENTRY(prefix, H, X, which)                                                                  \
    int32_t prefix##X(H *h, const uint64_t *index_or_null, const double *values, int64_t k) {                   \
        return chip::update_host(h, which, index_or_null, values, k);                                           \
    }                                                                                                           \
    int32_t prefix##X##_dev(H *h, const int64_t *index_dev_or_null, const double *values_dev, int64_t k) {      \
        return chip::update_dev(h, which, index_dev_or_null, values_dev, k);                                    \
    }
#define CHIP_UPDATE_ENTRIES(prefix, H)              \
    CHIP_UPDATE_ENTRY(prefix, H, P, chip::UPD_P)    \
    CHIP_UPDATE_ENTRY(prefix, H, A, chip::UPD_A)    \
    CHIP_UPDATE_ENTRY(prefix, H, q, chip::UPD_Q)    \
    CHIP_UPDATE_ENTRY(prefix, H, b, chip::UPD_B)

// the two forms of a re-equilibration of handle type H (chip_reequilibrate_problem / chip_reequilibrate_bdata and their
// _dev forms): CHIP_ERR_ARG before any device is touched, the handle's own refusal (reequilibrate_gate(fn), which also
// resets its counters), the host form's upload into the handle's staging (stage_upload4), then the device path
// h->reequilibrate(P, q, A, b).  The lengths are those of the handle's patterns
template <typename H>
int reequilibrate_entry(const char *fn, H *h, const double *P, const double *q, const double *A, const double *b,
                        bool host) {
    if (!h || !P || !q || !A || !b) return fail(CHIP_ERR_ARG, std::string(fn) + ": bad argument");
    if (int rc = h->reequilibrate_gate(fn)) return rc;
    CHIP_HIP(hipSetDevice(h->pd.device));
    const double *src[4] = {P, q, A, b}, *at[4] = {P, q, A, b};
    if (host) {
        const size_t len[4] = {(size_t)h->pd.update_len(UPD_P), (size_t)h->pd.update_len(UPD_Q),
                               (size_t)h->pd.update_len(UPD_A), (size_t)h->pd.update_len(UPD_B)};
        if (int rc = h->stage_upload4(src, len, at)) return rc;
    }
    return h->reequilibrate(at[0], at[1], at[2], at[3]);
}

// validate_as_update (settings.rs:307) for chip_problem_update_settings / chip_bdata_update_settings (fn: the caller's
// name in the error text): copies the two line-search fields into nw.linsys as create does (create_settings,
// problem_data.hpp), then CHIP_ERR_ARG if a field that setup consumed differs from old.  Defined in solver.cpp
int validate_settings_update(const chip_solver_settings &old, chip_solver_settings &nw, const char *fn);

} // namespace chip
