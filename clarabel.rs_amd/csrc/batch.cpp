// batch.cpp -- the batched L4 solver (chip_batch_*): nprob independent problems of Zero / Nonnegative / SecondOrder
// cones, stacked block-diagonally, solved by ONE interior-point loop whose scalars are kept per member:
//   setup: problem_data.hpp's steps, shared with solver.cpp, on the stack: Ruiz equilibration with one cost scale per
//          member (batch.hip), one L2 chip_kkt (block-diagonal K: one tree per member); per member norms and degrees;
//   solve: core/solver.rs:242-464 with tau, kappa, mu, sigma, the step length, DefaultInfo's scalars, the iteration
//          count and the status of every member on the host, read back from one device-to-host copy per reduction
//          pass.  Members that terminate are frozen: their step length is 0, selected per entry, and their part of
//          every right-hand side is 0.  The per-member passes are segmented kernels (batch.hip), so the number of
//          launches and host synchronisations per iteration does not depend on nprob.
// The L2 cone operations without a scalar (affine ds, ds from dz, Hs products, scaling update, unit initialisation)
// run on the whole stack as they are; combined_ds_shift runs with sigma mu = 0 and the member's sigma mu is then
// subtracted at the unit vector's entries, which is the same arithmetic for Nonnegative and SecondOrder cones.
// Members with PSDTriangle cones come in through chip_bsym_create, the same body with another mask of accepted cones:
// the L2 handle's per-cone eigenvalue results are folded per member on the device and the unit-vector operations run
// on the cones' diagonal entries (batch_psd.hpp).  A handle without PSD cones runs none of that.
// This file: the partition, create / destroy, the loop, the getters and the data updates.  The handle itself is in
// batch_handle.hpp, the derivative passes in batch_deriv.cpp, the test hooks in batch_debug.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "batch_handle.hpp"
#include "batch_update.hpp"

namespace {
// per-member device scalars (slot * nprob + k) and masks
enum { S_TAU, S_INVTAU, S_DTAU, S_OMS, S_ALPHA, S_AMAX, S_SHIFT1, S_SHIFT2, S_NEGSM, S_SX, S_SZ, S_COUNT };
enum { M_ACTIVE, M_QP, M_LP, M_SEL, M_SEL2, M_COUNT };
// slots of the reduction output: the residual pass
enum { R_QX, R_XPX, R_NX, R_NRXI, R_NPX, R_NRX, R_BADX, R_BZ, R_SZ, R_NZ, R_NS, R_NRZI, R_NRZ, R_BADSZ, R_COUNT };
// the direction passes
enum { D_QX1, D_BZ1, D_XIPX1, D_DPD, D_BAD, D_COUNT };
} // namespace

const BatchEntry BATCH_ENTRY_BASIC{"chip_batch_create", BATCH_CONES_BASIC, "only Zero, Nonnegative and SecondOrder cones"};
const BatchEntry BATCH_ENTRY_SYMMETRIC{"chip_bsym_create", BATCH_CONES_SYMMETRIC,
                                       "only Zero, Nonnegative, SecondOrder and PSDTriangle cones"};

int batch_cones_supported(const BatchEntry &entry, int64_t ncones, const int32_t *cone_tags) {
    for (int64_t i = 0; i < ncones; i++)
        if (cone_tags[i] < 0 || cone_tags[i] >= 32 || !((entry.accepted >> cone_tags[i]) & 1u))
            return fail(CHIP_ERR_UNSUPPORTED, std::string(entry.fn) + ": " + entry.only);
    return CHIP_OK;
}

// the partition of nprob members with n_part[k] columns and m_part[k] rows (sizes already within int32), and the
// checks that the parts add up and that every cone stays inside its member
int host_plan_build(HostPlan &hp, int64_t nprob, const int64_t *n_part, const int64_t *m_part, int64_t n, int64_t m,
                    int64_t ncones, const int32_t *cone_tags, const int64_t *cone_dims, const int64_t *cone_dims2) {
    const int np = (int)nprob;
    const std::string fn(hp.fn);
    hp.nprob = np;
    hp.n = (int)n;
    hp.m = (int)m;
    std::vector<int> &xoff = hp.xoff, &zoff = hp.zoff, &xmem = hp.xmem, &zmem = hp.zmem;
    xoff.assign((size_t)np + 1, 0);
    zoff.assign((size_t)np + 1, 0);
    for (int k = 0; k < np; k++) {
        if (n_part[k] < 0 || m_part[k] < 0) return fail(CHIP_ERR_ARG, fn + ": negative part");
        const int64_t xn = (int64_t)xoff[k] + n_part[k], zn = (int64_t)zoff[k] + m_part[k];
        if (xn > n || zn > m) return fail(CHIP_ERR_ARG, fn + ": the parts exceed n or m");
        xoff[k + 1] = (int)xn;
        zoff[k + 1] = (int)zn;
    }
    if (xoff[np] != n || zoff[np] != m) return fail(CHIP_ERR_ARG, fn + ": the parts do not add up to n, m");
    xmem.assign((size_t)n, 0);
    zmem.assign((size_t)m, 0);
    for (int k = 0; k < np; k++) {
        for (int j = xoff[k]; j < xoff[k + 1]; j++) xmem[j] = k;
        for (int i = zoff[k]; i < zoff[k + 1]; i++) zmem[i] = k;
    }
    hp.parts_ok = true;
    int64_t mm = 0, pdim = 0, nHs = 0;
    if (build_cone_specs(ncones, cone_tags, cone_dims, cone_dims2, hp.cones, mm, pdim, nHs))
        return fail(CHIP_ERR_ARG, fn + ": bad cone");
    if (mm != m) return fail(CHIP_ERR_DIM, fn + ": cone dimensions do not add up to m");
    hp.rtype.assign((size_t)m, dev::ROW_ZERO);
    hp.degree.assign((size_t)np, 0);
    hp.has_soc.assign((size_t)np, 0);
    hp.has_psd.assign((size_t)np, 0);
    hp.psd_total = 0;
    std::vector<int> &it_beg = hp.it_beg, &it_end = hp.it_end, &it_type = hp.it_type, it_mem;
    for (const ConeSpec &cs : hp.cones) {
        const int view = cs.tag == CHIP_CONE_PSDTRIANGLE ? hp.psd_total++ : -1; // (a cone of side 0 counts there too)
        if (cs.numel == 0) continue;
        const int r0 = (int)cs.start, r1 = (int)(cs.start + cs.numel), k = zmem[r0];
        if (zmem[r1 - 1] != k) return fail(CHIP_ERR_ARG, fn + ": a cone crosses a member's rows");
        if (cs.tag == CHIP_CONE_NONNEGATIVE) {
            for (int i = r0; i < r1; i++) hp.rtype[i] = dev::ROW_NN;
            hp.degree[k] += cs.numel;
            for (int i = r0; i < r1; i += dev::BATCH_CHUNK) {
                it_beg.push_back(i);
                it_end.push_back(std::min(r1, i + dev::BATCH_CHUNK));
                it_type.push_back(dev::ITEM_NN);
                it_mem.push_back(k);
            }
        } else if (cs.tag == CHIP_CONE_SECONDORDER) {
            hp.has_soc[k] = 1;
            hp.rtype[r0] = dev::ROW_SOC_HEAD;
            for (int i = r0 + 1; i < r1; i++) hp.rtype[i] = dev::ROW_SOC_TAIL;
            hp.degree[k] += 1;
            it_beg.push_back(r0);
            it_end.push_back(r1);
            it_type.push_back(dev::ITEM_SOC);
            it_mem.push_back(k);
        } else if (cs.tag == CHIP_CONE_PSDTRIANGLE) { // no item: its reductions are the L2 handle's (batch_psd.hpp)
            const int side = (int)cs.dim;
            hp.has_psd[k] = 1;
            for (int i = r0; i < r1; i++) hp.rtype[i] = dev::ROW_PSD;
            hp.degree[k] += side; // psdtrianglecone.rs:77-79
            hp.psd_mem.push_back(k);
            hp.psd_start.push_back(r0);
            hp.psd_dim.push_back(side);
            hp.psd_view.push_back(view);
            for (int j = 0; j < side; j++) hp.psd_diag.push_back(r0 + j * (j + 1) / 2 + j);
        }
    }
    // cones are in row order, so the items are sorted by member
    hp.it_first.assign((size_t)np + 1, 0);
    for (int k : it_mem) hp.it_first[k + 1]++;
    for (int k = 0; k < np; k++) hp.it_first[k + 1] += hp.it_first[k];
    hp.psd_first.assign((size_t)np + 1, 0);
    for (int k : hp.psd_mem) hp.psd_first[k + 1]++;
    for (int k = 0; k < np; k++) hp.psd_first[k + 1] += hp.psd_first[k];
    std::vector<int> &ch_beg = hp.ch_beg, &ch_end = hp.ch_end;
    hp.cx_first.assign((size_t)np + 1, 0);
    hp.cz_first.assign((size_t)np + 1, 0);
    for (int k = 0; k < np; k++) {
        for (int j = xoff[k]; j < xoff[k + 1]; j += dev::BATCH_CHUNK) {
            ch_beg.push_back(j);
            ch_end.push_back(std::min(xoff[k + 1], j + dev::BATCH_CHUNK));
        }
        hp.cx_first[k + 1] = (int)ch_beg.size();
    }
    hp.ncx = (int)ch_beg.size();
    for (int k = 0; k < np; k++) {
        for (int i = zoff[k]; i < zoff[k + 1]; i += dev::BATCH_CHUNK) {
            ch_beg.push_back(i);
            ch_end.push_back(std::min(zoff[k + 1], i + dev::BATCH_CHUNK));
        }
        hp.cz_first[k + 1] = (int)ch_beg.size() - hp.ncx;
    }
    hp.ncz = (int)ch_beg.size() - hp.ncx;
    return CHIP_OK;
}

// the device copy of a HostPlan, owned by `mem`
int host_plan_upload(DevPool &mem, const HostPlan &hp, dev::BatchPlan *pl) {
    int rc;
    int *d_xoff, *d_zoff, *d_xmem, *d_zmem, *d_chb, *d_che, *d_cxf, *d_czf, *d_itb, *d_ite, *d_itt, *d_itf, *d_rt;
    if ((rc = mem.upload(&d_xoff, hp.xoff)) || (rc = mem.upload(&d_zoff, hp.zoff)) ||
        (rc = mem.upload(&d_xmem, hp.xmem)) || (rc = mem.upload(&d_zmem, hp.zmem)) ||
        (rc = mem.upload(&d_chb, hp.ch_beg)) || (rc = mem.upload(&d_che, hp.ch_end)) ||
        (rc = mem.upload(&d_cxf, hp.cx_first)) || (rc = mem.upload(&d_czf, hp.cz_first)) ||
        (rc = mem.upload(&d_itb, hp.it_beg)) || (rc = mem.upload(&d_ite, hp.it_end)) ||
        (rc = mem.upload(&d_itt, hp.it_type)) || (rc = mem.upload(&d_itf, hp.it_first)) ||
        (rc = mem.upload(&d_rt, hp.rtype)))
        return rc;
    *pl = dev::BatchPlan{hp.nprob, hp.n, hp.m, d_xoff, d_zoff, d_xmem, d_zmem, d_chb,  d_che, d_cxf,
                         d_czf,    hp.ncx, hp.ncz, d_itb, d_ite, d_itt, d_itf, (int)hp.it_beg.size(), d_rt};
    return CHIP_OK;
}

// the device copy of the plan's PSD cones, owned by `mem`; zmem is the uploaded plan's
int host_plan_upload_psd(DevPool &mem, const HostPlan &hp, const dev::BatchPlan &pl, dev::BatchPsdPlan *pp) {
    int rc;
    int *d_first, *d_view, *d_diag;
    if ((rc = mem.upload(&d_first, hp.psd_first)) || (rc = mem.upload(&d_view, hp.psd_view)) ||
        (rc = mem.upload(&d_diag, hp.psd_diag)))
        return rc;
    *pp = dev::BatchPsdPlan{hp.nprob, (int)hp.psd_view.size(), (int)hp.psd_diag.size(), d_first, d_view, d_diag, pl.zmem};
    return CHIP_OK;
}

// chip_batch_create and chip_bsym_create: one body, the entry decides which cones pass
static int32_t batch_create(const BatchEntry &entry, chip_batch **out, int64_t nprob, const int64_t *n_part,
                            const int64_t *m_part, int64_t n, int64_t m, const uint64_t *Pcolptr,
                            const uint64_t *Prowval, const double *Pnzval, const double *q, const uint64_t *Acolptr,
                            const uint64_t *Arowval, const double *Anzval, const double *b, int64_t ncones,
                            const int32_t *cone_tags, const int64_t *cone_dims, const int64_t *cone_dims2,
                            const chip_solver_settings *settings) {
    const std::string fn(entry.fn);
    if (!out) return fail(CHIP_ERR_ARG, fn + ": bad argument");
    *out = nullptr;
    if (nprob < 1 || !n_part || !m_part || n < 0 || m < 0 || !Pcolptr || !Acolptr || ncones < 0 ||
        (ncones && (!cone_tags || !cone_dims)))
        return fail(CHIP_ERR_ARG, fn + ": bad argument");
    if ((Pcolptr[n] && (!Prowval || !Pnzval)) || (Acolptr[n] && (!Arowval || !Anzval)) || (n && !q) || (m && !b))
        return fail(CHIP_ERR_ARG, fn + ": missing data");
    const double t0 = now_s();
    std::unique_ptr<chip_batch> h(new chip_batch());
    chip_solver_settings &st = h->st;
    create_settings(settings, st);
    if (st.presolve_enable || st.chordal_decomposition_enable)
        return fail(CHIP_ERR_UNSUPPORTED, fn + ": presolve and chordal decomposition are not supported");
    if (int rc = batch_cones_supported(entry, ncones, cone_tags)) return rc;
    const ProblemArgs a{n,      m,         Pcolptr,   Prowval,  Pnzval, q, Acolptr, Arowval, Anzval, b,
                        ncones, cone_tags, cone_dims, cone_dims2};
    if (nprob >= (1ll << 31) || !a.fits_int32()) return fail(CHIP_ERR_DIM, fn + ": sizes out of int32 range");
    // ---- the partition and the checks that every entry and cone stays inside its member
    const int np = (int)nprob;
    HostPlan hp;
    hp.fn = entry.fn;
    const int plan_rc = host_plan_build(hp, nprob, n_part, m_part, n, m, ncones, cone_tags, cone_dims, cone_dims2);
    if (plan_rc && !hp.parts_ok) return plan_rc;
    const std::vector<int> &xoff = hp.xoff, &zoff = hp.zoff, &zmem = hp.zmem, &xmem = hp.xmem;
    CooPattern co;
    std::vector<int> lp_init((size_t)np, 1);
    int rc = coordinate_form(a, co, [&](char mat, int64_t j, int64_t r) {
        const int k = xmem[j];
        if (mat == 'P') {
            if (r < xoff[k]) return fail(CHIP_ERR_ARG, fn + ": an entry of P crosses two members' blocks");
            lp_init[k] = 0;
        } else if (zmem[r] != k) {
            return fail(CHIP_ERR_ARG, fn + ": an entry of A crosses two members' blocks");
        }
        return (int)CHIP_OK;
    });
    if (rc) return rc;
    if (plan_rc) return plan_rc; // a refused cone: reported after the entries of P and A, its text still the last error
    // ---- the device
    if (st.linsys.device == CHIP_DEVICE_HOST_ONLY || chip_device_count() < 1)
        return fail(CHIP_ERR_NO_DEVICE, fn + ": no HIP device (the product has no CPU fallback)");
    ProblemData &pd = h->pd;
    if (st.linsys.device >= 0) CHIP_HIP(hipSetDevice(st.linsys.device));
    CHIP_HIP(hipGetDevice(&pd.device));
    h->nprob = np;
    h->xoff = xoff;
    h->zoff = zoff;
    h->degree = hp.degree;
    h->has_soc = hp.has_soc;
    h->has_psd = hp.has_psd;
    h->cones = hp.cones;
    h->lp_init = lp_init;
    h->anyP = a.nnzP() > 0;
    h->anyLP = std::find(lp_init.begin(), lp_init.end(), 1) != lp_init.end();
    DevPool &mem = h->mem;
    dev::BatchPlan &pl = h->plan;
    if ((rc = host_plan_upload(mem, hp, &pl))) return rc;
    if (!hp.psd_view.empty()) { // (a handle without a PSD cone of side > 0 carries nothing of them)
        h->psd_total = hp.psd_total;
        if ((rc = host_plan_upload_psd(mem, hp, pl, &h->psd)) || (rc = mem.alloc(&h->psd_res, 4 * (size_t)hp.psd_total)))
            return rc;
    }
    // ---- the data, with the unscaled q and (capped) b kept beside it; per member the norms of the two
    std::vector<double> bcap;
    if ((rc = pd.upload(mem, a, co, bcap)) || (rc = mem.upload(&h->uq, q, (size_t)n)) ||
        (rc = mem.upload(&h->ub, bcap.data(), (size_t)m)) || (rc = pd.alloc_scalings(mem)) ||
        (rc = mem.alloc(&h->negq, (size_t)n)))
        return rc;
    for (int k = 0; k < np; k++) {
        h->normq.push_back(absmax_nan(q, xoff[k], xoff[k + 1]));
        h->normb.push_back(absmax_nan(bcap.data(), zoff[k], zoff[k + 1]));
    }
    // ---- its equilibration on a stream of its own (the handle's is the KKT handle's, built below)
    DevPool work;
    double *colsum = nullptr, *scr = nullptr;
    if ((rc = work.alloc(&colsum, (size_t)np)) || (rc = work.alloc(&scr, dev::seg_scratch_doubles(pl)))) return rc;
    hipStream_t s_eq = nullptr;
    CHIP_HIP(hipStreamCreateWithFlags(&s_eq, hipStreamNonBlocking));
    const double te = now_s();
    h->c.assign((size_t)np, 1.0);
    auto ruiz_step = [&](unsigned long long *bits, double *cstate) {
        dev::batch_eq_ruiz_step(s_eq, pl, pd.M, pd.q, pd.b, pd.d, pd.e, bits, scr, colsum, cstate,
                                st.equilibrate_min_scaling, st.equilibrate_max_scaling);
    };
    rc = pd.equilibrate(s_eq, st, hp.cones, np, dev::batch_eq_bits_words(pd.n, pd.m, np), ruiz_step, h->c.data());
    (void)hipStreamDestroy(s_eq);
    if (rc) return rc;
    h->equilibration_time = now_s() - te;
    if ((rc = mem.upload(&h->dc, h->c.data(), (size_t)np))) return rc;
    // ---- one KKT system of the equilibrated stack (block-diagonal K)
    if ((rc = pd.create_kkt(a, nullptr, st.linsys, &h->kkt, &h->sys, &h->stream, [](chip_kkt *) { return 0; })))
        return rc;
    if (h->psd.ncones && kkt_psd_cones(h->kkt) != h->psd_total) // (view[] indexes the L2 handle's per-cone results)
        return fail(CHIP_ERR_ARG, fn + ": the PSD cones of the plan are not those of the KKT handle");
    const size_t N = (size_t)n, Mm = (size_t)m;
    if ((rc = mem.alloc(&h->vx, N)) || (rc = mem.alloc(&h->vs, Mm)) || (rc = mem.alloc(&h->vz, Mm)) ||
        (rc = mem.alloc(&h->px, N)) || (rc = mem.alloc(&h->ps, Mm)) || (rc = mem.alloc(&h->pz, Mm)) ||
        (rc = mem.alloc(&h->hx, N)) || (rc = mem.alloc(&h->hs, Mm)) || (rc = mem.alloc(&h->hz, Mm)) ||
        (rc = mem.alloc(&h->lx, N)) || (rc = mem.alloc(&h->ls, Mm)) || (rc = mem.alloc(&h->lz, Mm)) ||
        (rc = mem.alloc(&h->dx, N)) || (rc = mem.alloc(&h->ds, Mm)) || (rc = mem.alloc(&h->dz, Mm)) ||
        (rc = mem.alloc(&h->x1, N)) || (rc = mem.alloc(&h->z1, Mm)) || (rc = mem.alloc(&h->x2, N)) ||
        (rc = mem.alloc(&h->z2, Mm)) || (rc = mem.alloc(&h->workx, N)) || (rc = mem.alloc(&h->workx2, N)) ||
        (rc = mem.alloc(&h->wn, N)) || (rc = mem.alloc(&h->wn2, N)) || (rc = mem.alloc(&h->wn3, N)) || (rc = mem.alloc(&h->workz, Mm)) ||
        (rc = mem.alloc(&h->conicw, Mm)) || (rc = mem.alloc(&h->rx, N)) || (rc = mem.alloc(&h->rz, Mm)) ||
        (rc = mem.alloc(&h->rx_inf, N)) || (rc = mem.alloc(&h->rz_inf, Mm)) || (rc = mem.alloc(&h->Pxv, N)) ||
        (rc = mem.alloc(&h->xo, N)) || (rc = mem.alloc(&h->so, Mm)) || (rc = mem.alloc(&h->zo, Mm)))
        return rc;
    const size_t red_len = (size_t)(R_COUNT + 2) * np; // + the interior minima
    if ((rc = mem.alloc(&h->dsc_ring, (size_t)chip_batch::RING * S_COUNT * np)) ||
        (rc = mem.alloc(&h->dmask_ring, (size_t)chip_batch::RING * M_COUNT * np)) ||
        (rc = mem.alloc(&h->dred, red_len)) || (rc = mem.alloc(&h->seg_scr, dev::seg_scratch_doubles(pl))) ||
        (rc = mem.alloc(&h->cone_scr, dev::cone_scratch_doubles(pl))))
        return rc;
    h->hsc.assign((size_t)S_COUNT * np, 0.0);
    h->hmask.assign((size_t)M_COUNT * np, 0);
    h->hred.assign(red_len, 0.0);
    h->hsc_ring.assign((size_t)chip_batch::RING * S_COUNT * np, 0.0);
    h->hmask_ring.assign((size_t)chip_batch::RING * M_COUNT * np, 0);
    h->dsc = h->dsc_ring;
    h->dmask = h->dmask_ring;
    dev::waxpby(h->stream, h->negq, -1.0, pd.q, 0.0, nullptr, pd.n);
    CHIP_HIP(hipGetLastError());
    CHIP_HIP(hipStreamSynchronize(h->stream));
    h->setup_time = now_s() - t0;
    *out = h.release();
    return CHIP_OK;
}

int32_t chip_batch_create(chip_batch **out, int64_t nprob, const int64_t *n_part, const int64_t *m_part, int64_t n,
                          int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval, const double *Pnzval,
                          const double *q, const uint64_t *Acolptr, const uint64_t *Arowval, const double *Anzval,
                          const double *b, int64_t ncones, const int32_t *cone_tags, const int64_t *cone_dims,
                          const int64_t *cone_dims2, const double *cone_alphas_or_null,
                          const double *genpow_alphas_or_null, const chip_solver_settings *settings) {
    (void)cone_alphas_or_null;
    (void)genpow_alphas_or_null;
    return batch_create(BATCH_ENTRY_BASIC, out, nprob, n_part, m_part, n, m, Pcolptr, Prowval, Pnzval, q, Acolptr, Arowval,
                        Anzval, b, ncones, cone_tags, cone_dims, cone_dims2, settings);
}

int32_t chip_bsym_create(chip_batch **out, int64_t nprob, const int64_t *n_part, const int64_t *m_part, int64_t n,
                         int64_t m, const uint64_t *Pcolptr, const uint64_t *Prowval, const double *Pnzval,
                         const double *q, const uint64_t *Acolptr, const uint64_t *Arowval, const double *Anzval,
                         const double *b, int64_t ncones, const int32_t *cone_tags, const int64_t *cone_dims,
                         const int64_t *cone_dims2, const double *cone_alphas_or_null,
                         const double *genpow_alphas_or_null, const chip_solver_settings *settings) {
    (void)cone_alphas_or_null;
    (void)genpow_alphas_or_null;
    return batch_create(BATCH_ENTRY_SYMMETRIC, out, nprob, n_part, m_part, n, m, Pcolptr, Prowval, Pnzval, q, Acolptr,
                        Arowval, Anzval, b, ncones, cone_tags, cone_dims, cone_dims2, settings);
}

void chip_batch_destroy(chip_batch *h) {
    if (!h) return;
    (void)hipSetDevice(h->pd.device);
    delete h;
}

// default_start (core/solver.rs:525-541) for symmetric cones, per member: the initial point of kktsystem.rs:197-231
// (QP members from [-q; b], LP members from [0; b] and [-q; 0]) and _shift_to_cone_interior (variables.rs:231-256)
// with the member's margins and degree
int chip_batch::default_start() {
    int rc;
    hipStream_t s = stream;
    const int n = pd.n, m = pd.m;
    if ((rc = chip_kkt_unit_initialization_dev(kkt, dz, ds))) return rc;
    if ((rc = chip_kkt_update_scaling_dev(kkt, dz, dz, 1.0, 0)) < 0) return rc;
    if ((rc = chip_kkt_update(kkt, nullptr)) < 0) return rc; // (the reference ignores the bool here)
    for (int k = 0; k < nprob; k++) {
        hm(M_QP, k) = !lp_init[k];
        hm(M_LP, k) = lp_init[k];
    }
    if ((rc = push_masks())) return rc;
    lin(workx, negq, nullptr, nullptr, nullptr, 1.0, 0.0, 0, mk(M_QP), dev::MASK_ZERO); // QP: -q, LP: 0
    if ((rc = chip_kkt_setrhs_dev(kkt, workx, pd.b))) return rc;
    if ((rc = chip_kkt_solve_dev(kkt, vx, vz)) < 0) return rc;
    dev::waxpby(s, vs, -1.0, vz, 0.0, nullptr, m); // QP: s = -z; LP: s = -(the z part of [0; b])
    if (anyLP) {
        lin(workx, negq, nullptr, nullptr, nullptr, 1.0, 0.0, 0, mk(M_LP), dev::MASK_ZERO);
        CHIP_HIP(hipMemsetAsync(workz, 0, std::max<size_t>((size_t)m, 1) * 8, s));
        if ((rc = chip_kkt_setrhs_dev(kkt, workx, workz))) return rc;
        if ((rc = chip_kkt_solve_dev(kkt, x1, z1)) < 0) return rc;
        lin(vz, z1, nullptr, nullptr, nullptr, 1.0, 0.0, 1, mk(M_LP), dev::MASK_KEEP);
    }
    // the shifts of s (primal) and z (dual)
    for (int pass = 0; pass < 2; pass++) {
        double *v = pass == 0 ? vs : vz;
        dev::cone_minima(s, plan, dev::CONE_MARGINS, nullptr, nullptr, v, nullptr, nullptr, dred, dred + nprob,
                         cone_scr);
        if (psd.ncones) { // the PSD cones' margins (psdtrianglecone.rs:104-121) join the member's on the device
            if ((rc = kkt_psd_margins_dev(kkt, v, pres(0), pres(1)))) return rc;
            dev::bp_fold(s, psd, dev::BP_MARGINS, pres(0), pres(1), dred, dred + nprob);
        }
        if ((rc = read_red(2 * (size_t)nprob))) return rc;
        for (int k = 0; k < nprob; k++) {
            const double mn = red(0, k), pos = red(1, k);
            const double target = std::max(1.0, (pos * 0.1) / (double)degree[k]);
            double a1 = 0.0, a2 = 0.0;
            if (mn <= 0.0) {
                a1 = -mn;
                a2 = target;
            } else if (mn < target) {
                a1 = target - mn;
            }
            hs_(S_SHIFT1, k) = a1;
            hs_(S_SHIFT2, k) = a2;
        }
        if ((rc = push_scalars())) return rc;
        dev::bunit_shift(s, plan, v, sc(S_SHIFT1), pass == 0, nullptr);
        dev::bunit_shift(s, plan, v, sc(S_SHIFT2), pass == 0, nullptr);
        if (psd.ncones) {
            dev::bp_diag_shift(s, psd, v, sc(S_SHIFT1), nullptr);
            dev::bp_diag_shift(s, psd, v, sc(S_SHIFT2), nullptr);
        }
    }
    for (int k = 0; k < nprob; k++) tau[k] = kappa[k] = 1.0;
    // the previous iterate starts as the initial one (a member that fails before its first step reports it)
    if (n) CHIP_HIP(hipMemcpyAsync(px, vx, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    if (m) CHIP_HIP(hipMemcpyAsync(ps, vs, (size_t)m * 8, hipMemcpyDeviceToDevice, s));
    if (m) CHIP_HIP(hipMemcpyAsync(pz, vz, (size_t)m * 8, hipMemcpyDeviceToDevice, s));
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}

// Residuals::update + DefaultInfo::update's norms and dots for every member, the finiteness counts and the interior
// minima of (s, z): one segmented pass, one cone pass, ONE device-to-host copy
int chip_batch::residual_pass() {
    int rc;
    for (int k = 0; k < nprob; k++) hs_(S_TAU, k) = tau[k];
    if ((rc = push_scalars())) return rc;
    if (anyP) {
        if ((rc = spmv(0, Pxv, nullptr, 1.0, vx))) return rc;
    } else if (pd.n) {
        CHIP_HIP(hipMemsetAsync(Pxv, 0, (size_t)pd.n * 8, stream));
    }
    if ((rc = spmv(2, rx_inf, nullptr, -1.0, vz))) return rc; // rx_inf = -A' z
    if ((rc = spmv(1, rz_inf, vs, 1.0, vx))) return rc;       // rz_inf = A x + s
    dev::bresid(stream, plan, rx, rx_inf, Pxv, pd.q, rz, rz_inf, pd.b, sc(S_TAU));
    dev::SegBatch bt{};
    auto add = [&](const double *a, const double *w, int kind, int space, int slot) {
        bt.s[bt.count++] = dev::SegSpec{a, w, kind, space, slot};
    };
    add(pd.q, vx, dev::SEG_DOT, 0, R_QX);
    add(vx, Pxv, dev::SEG_DOT, 0, R_XPX);
    add(vx, pd.d, dev::SEG_WSQ, 0, R_NX);
    add(rx_inf, pd.dinv, dev::SEG_WSQ, 0, R_NRXI);
    add(Pxv, pd.dinv, dev::SEG_WSQ, 0, R_NPX);
    add(rx, pd.dinv, dev::SEG_WSQ, 0, R_NRX);
    add(vx, nullptr, dev::SEG_NONFINITE, 0, R_BADX);
    add(pd.b, vz, dev::SEG_DOT, 1, R_BZ);
    add(vs, vz, dev::SEG_DOT, 1, R_SZ);
    add(vz, pd.e, dev::SEG_WSQ, 1, R_NZ);
    add(vs, pd.einv, dev::SEG_WSQ, 1, R_NS);
    add(rz_inf, pd.einv, dev::SEG_WSQ, 1, R_NRZI);
    add(rz, pd.einv, dev::SEG_WSQ, 1, R_NRZ);
    add(vs, vz, dev::SEG_NONFINITE, 1, R_BADSZ);
    dev::seg_reduce(stream, plan, bt, dred, seg_scr);
    dev::cone_minima(stream, plan, dev::CONE_INTERIOR, nullptr, nullptr, vz, vs, nullptr, dred + (size_t)R_COUNT * nprob,
                     nullptr, cone_scr);
    launches += 4;
    if (psd.ncones) { // the smallest eigenvalues of the PSD cones' s and z, folded behind the other cones' minima
        int rc2;
        if ((rc2 = kkt_psd_margins_dev(kkt, vs, pres(0), pres(1))) || (rc2 = kkt_psd_margins_dev(kkt, vz, pres(2), pres(3))))
            return rc2;
        dev::bp_fold(stream, psd, dev::BP_INTERIOR, pres(0), pres(2), dred + (size_t)R_COUNT * nprob, nullptr);
        launches += 3;
    }
    return read_red((size_t)(R_COUNT + 1) * nprob);
}

// the dots and squared norms of member k from the residual pass into DefaultInfo::update (ipm_info.hpp), and its mu
void chip_batch::member_info(int k) {
    IpmInfo &I = info[k];
    const double qx = red(R_QX, k), bz = red(R_BZ, k), sz = red(R_SZ, k), xPx = anyP ? red(R_XPX, k) : 0.0;
    I.out5[0] = qx + bz + kappa[k] + xPx / tau[k];
    I.out5[1] = qx;
    I.out5[2] = bz;
    I.out5[3] = sz;
    I.out5[4] = xPx;
    const int slots[8] = {R_NX, R_NZ, R_NS, R_NRXI, R_NPX, R_NRZI, R_NRZ, R_NRX};
    double sq[8];
    for (int j = 0; j < 8; j++) sq[j] = red(slots[j], k);
    ipm_info_update(I, sq, tau[k], kappa[k], c[k], normq[k], normb[k]);
    mu[k] = (sz + tau[k] * kappa[k]) / (double)(degree[k] + 1); // variables.rs:63-66
}

// member k ends NumericalError: its reported solution is its last finite iterate (the previous one when the current
// one is not finite), held aside; its s and z become the cones' unit vector so that its block of K stays well posed
int chip_batch::end_member(int k, int status, int iterations, bool from_prev) {
    info[k].status = status;
    info[k].iterations = iterations;
    active[k] = 0;
    held[k] = from_prev ? 2 : 1;
    return CHIP_OK;
}

// the KKT solve of one direction with the member-wise tau step (kktsystem.rs:127-195): right-hand side (dx, ds, dz)
// and rtau / rkappa per member; the result in (lx, ls, lz) and dtau / lkappa per member.  conic: the constant term of
// Hs dz + ds = -conic.  Members whose part of the solution is not finite end NumericalError; *global_ok is the
// engine's verdict
int chip_batch::solve_direction(const double *conic, const std::vector<double> &rtau, const std::vector<double> &rkap,
                                std::vector<double> &lkappa, bool *global_ok, int iter) {
    int rc;
    hipStream_t s = stream;
    // frozen members contribute a zero right-hand side, so their part of the solution is 0 and stays finite
    lin(workz, conic, dz, nullptr, nullptr, 1.0, -1.0, 1, mk(M_ACTIVE), dev::MASK_ZERO);
    lin(workx, dx, nullptr, nullptr, nullptr, 1.0, 0.0, 0, mk(M_ACTIVE), dev::MASK_ZERO);
    if ((rc = chip_kkt_setrhs_dev(kkt, workx, workz))) return rc;
    rc = chip_kkt_solve_dev(kkt, x1, z1);
    syncs++;
    launches++;
    if (rc < 0) return rc;
    *global_ok = rc == 1;
    // the dots of the tau numerator and denominator per member and the finiteness of (x1, z1), one copy
    for (int k = 0; k < nprob; k++) hs_(S_INVTAU, k) = 1.0 / tau[k];
    if ((rc = push_scalars())) return rc;
    dev::SegBatch bt{};
    bt.s[bt.count++] = dev::SegSpec{pd.q, x1, dev::SEG_DOT, 0, D_QX1};
    bt.s[bt.count++] = dev::SegSpec{pd.b, z1, dev::SEG_DOT, 1, D_BZ1};
    if (anyP) {
        lin(wn2, vx, nullptr, sc(S_INVTAU), nullptr, 1.0, 0.0, 0, nullptr, 0); // xi = x / tau
        if ((rc = spmv(0, wn, nullptr, 1.0, x1))) return rc;                   // P x1
        dev::waxpby(s, workx2, -1.0, x2, 1.0, wn2, pd.n);                      // xi - x2
        if ((rc = spmv(0, wn3, nullptr, 1.0, workx2))) return rc;
        launches++;
        bt.s[bt.count++] = dev::SegSpec{wn2, wn, dev::SEG_DOT, 0, D_XIPX1};
        bt.s[bt.count++] = dev::SegSpec{workx2, wn3, dev::SEG_DOT, 0, D_DPD};
    }
    bt.s[bt.count++] = dev::SegSpec{x1, nullptr, dev::SEG_NONFINITE, 0, D_BAD};
    bt.s[bt.count++] = dev::SegSpec{z1, nullptr, dev::SEG_NONFINITE, 1, D_BAD + 1};
    dev::seg_reduce(s, plan, bt, dred, seg_scr);
    launches += 2;
    if ((rc = read_red((size_t)(D_COUNT + 1) * nprob))) return rc;
    for (int k = 0; k < nprob; k++) {
        dtau[k] = 0.0;
        lkappa[k] = 0.0;
        if (!active[k]) continue;
        const double t = tau[k], kp = kappa[k];
        const double xiPx1 = anyP ? red(D_XIPX1, k) : 0.0, dPd = anyP ? red(D_DPD, k) : 0.0;
        const double tau_num = rtau[k] - rkap[k] / t + red(D_QX1, k) + red(D_BZ1, k) + 2.0 * xiPx1;
        double tau_den = kp / t - qx2[k] - bz2[k];
        tau_den += dPd - x2Px2[k];
        const double lt = tau_num / tau_den;
        if (red(D_BAD, k) != 0.0 || red(D_BAD + 1, k) != 0.0 || !std::isfinite(lt)) {
            end_member(k, CHIP_SOLVER_NUMERICAL_ERROR, iter, false);
            continue;
        }
        dtau[k] = lt;
        lkappa[k] = -(rkap[k] + kp * lt) / t;
    }
    for (int k = 0; k < nprob; k++) {
        hs_(S_DTAU, k) = dtau[k];
        hm(M_ACTIVE, k) = active[k];
    }
    if ((rc = push_scalars()) || (rc = push_masks())) return rc;
    lin(lx, x1, x2, nullptr, sc(S_DTAU), 1.0, 0.0, 0, nullptr, 0); // x1 + dtau x2
    lin(lz, z1, z2, nullptr, sc(S_DTAU), 1.0, 0.0, 1, nullptr, 0);
    if ((rc = chip_kkt_mul_Hs_dev(kkt, ls, lz))) return rc; // ds = -(Hs dz + conic)
    dev::waxpby(s, ls, -1.0, conic, -1.0, ls, pd.m);
    launches += 2;
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}

// calc_step_length (variables.rs:120-160) per member: the tau / kappa bounds on the host, the cones on the device
int chip_batch::step_length(const std::vector<double> &lkappa, bool combined) {
    int rc;
    const double big = std::numeric_limits<double>::max();
    for (int k = 0; k < nprob; k++) {
        const double a_tau = dtau[k] < 0.0 ? -tau[k] / dtau[k] : big;
        const double a_kap = lkappa[k] < 0.0 ? -kappa[k] / lkappa[k] : big;
        hs_(S_AMAX, k) = std::min(std::min(a_tau, a_kap), 1.0);
    }
    if ((rc = push_scalars())) return rc;
    dev::cone_minima(stream, plan, dev::CONE_STEP, lz, ls, vz, vs, sc(S_AMAX), dred, nullptr, cone_scr);
    launches += 2;
    if (psd.ncones) { // psdtrianglecone.rs:235-279 per cone with alpha_max = 1: the member's S_AMAX <= 1 is in its slot
        if ((rc = kkt_psd_step_length_dev(kkt, lz, ls, 1.0, pres(0)))) return rc;
        dev::bp_fold(stream, psd, dev::BP_STEP, pres(0), nullptr, dred, nullptr);
        launches += 2;
    }
    if ((rc = read_red((size_t)nprob))) return rc;
    for (int k = 0; k < nprob; k++) {
        double a = red(0, k);
        if (combined) a *= st.max_step_fraction;
        alpha[k] = active[k] ? a : 0.0;
    }
    return CHIP_OK;
}

// the constant right-hand side [-q; b] after each KKT update (kktsystem.rs:108-125) and its dots per member
int chip_batch::constant_rhs(bool *global_ok, int iter) {
    int rc;
    if ((rc = chip_kkt_setrhs_dev(kkt, negq, pd.b))) return rc;
    rc = chip_kkt_solve_dev(kkt, x2, z2);
    syncs++;
    launches++;
    if (rc < 0) return rc;
    *global_ok = rc == 1;
    dev::SegBatch bt{};
    bt.s[bt.count++] = dev::SegSpec{pd.q, x2, dev::SEG_DOT, 0, 0};
    bt.s[bt.count++] = dev::SegSpec{pd.b, z2, dev::SEG_DOT, 1, 1};
    if (anyP) {
        if ((rc = spmv(0, wn, nullptr, 1.0, x2))) return rc;
        bt.s[bt.count++] = dev::SegSpec{x2, wn, dev::SEG_DOT, 0, 2};
    }
    bt.s[bt.count++] = dev::SegSpec{x2, nullptr, dev::SEG_NONFINITE, 0, 3};
    bt.s[bt.count++] = dev::SegSpec{z2, nullptr, dev::SEG_NONFINITE, 1, 4};
    dev::seg_reduce(stream, plan, bt, dred, seg_scr);
    launches += 2;
    if ((rc = read_red(5 * (size_t)nprob))) return rc;
    for (int k = 0; k < nprob; k++) {
        qx2[k] = red(0, k);
        bz2[k] = red(1, k);
        x2Px2[k] = anyP ? red(2, k) : 0.0;
        if (active[k] && (red(3, k) != 0.0 || red(4, k) != 0.0)) end_member(k, CHIP_SOLVER_NUMERICAL_ERROR, iter, false);
    }
    return CHIP_OK;
}

// the held iterates of the members that ended NumericalError this iteration (the current one, or the previous one
// when the current one is not finite), then their s and z reset to the unit vector
int chip_batch::hold_and_reset() {
    bool any = false;
    for (int k = 0; k < nprob; k++) {
        hm(M_SEL, k) = held[k] == 1 && !held_done[k];
        hm(M_SEL2, k) = held[k] == 2 && !held_done[k];
        any = any || hm(M_SEL, k) || hm(M_SEL2, k);
    }
    if (!any) return CHIP_OK;
    for (int k = 0; k < nprob; k++) {
        if (!hm(M_SEL, k) && !hm(M_SEL2, k)) continue;
        const bool prev = hm(M_SEL2, k);
        htau[k] = prev ? ptau[k] : tau[k];
        hkappa[k] = prev ? pkappa[k] : kappa[k];
        const int status = info[k].status, iterations = info[k].iterations;
        hinfo[k] = prev ? pinfo[k] : info[k];
        hinfo[k].status = status;
        hinfo[k].iterations = iterations;
        held_done[k] = 1;
    }
    int rc;
    if ((rc = push_masks())) return rc;
    copy_members(hx, hs, hz, vx, vs, vz, mk(M_SEL));
    copy_members(hx, hs, hz, px, ps, pz, mk(M_SEL2));
    for (int k = 0; k < nprob; k++) hm(M_SEL, k) = hm(M_SEL, k) || hm(M_SEL2, k);
    if ((rc = push_masks())) return rc;
    dev::bunit_reset(stream, plan, vx, vs, vz, mk(M_SEL));
    launches++;
    if (psd.ncones) { // (bunit_reset has written 0 on every PSD row of these members)
        dev::bp_diag_unit(stream, psd, vs, vz, mk(M_SEL));
        launches++;
    }
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}

// info.post_process (info.rs:95-105) and solution.post_process (solution.rs:68-111) per member, one segmented unscale
int chip_batch::post_process() {
    int rc;
    for (int k = 0; k < nprob; k++) {
        hm(M_SEL, k) = held[k] != 0;
        if (held[k]) {
            info[k] = hinfo[k];
            tau[k] = htau[k];
            kappa[k] = hkappa[k];
        }
    }
    if ((rc = push_masks())) return rc;
    copy_members(vx, vs, vz, hx, hs, hz, mk(M_SEL));
    for (int k = 0; k < nprob; k++)
        ipm_post_process(info[k], st, tau[k], kappa[k], c[k], &obj_val[k], &obj_val_dual[k], &hs_(S_SX, k), &hs_(S_SZ, k));
    if ((rc = push_scalars())) return rc;
    dev::bunscale(stream, plan, xo, vx, pd.d, zo, vz, pd.e, so, vs, pd.einv, sc(S_SX), sc(S_SZ));
    CHIP_HIP(hipGetLastError());
    CHIP_HIP(hipStreamSynchronize(stream));
    return CHIP_OK;
}

// IPSolver::solve (core/solver.rs:242-464) with every scalar indexed by member
int32_t chip_batch_solve(chip_batch *h) {
    if (!h) return fail(CHIP_ERR_ARG, "chip_batch_solve: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    const int np = h->nprob;
    const chip_solver_settings &st = h->st;
    auto zeros = [np](std::vector<double> &v) { v.assign((size_t)np, 0.0); };
    for (auto *v : {&h->tau, &h->kappa, &h->ptau, &h->pkappa, &h->htau, &h->hkappa, &h->mu, &h->sigma, &h->alpha,
                    &h->dtau, &h->obj_val, &h->obj_val_dual, &h->qx2, &h->bz2, &h->x2Px2})
        zeros(*v);
    h->info.assign((size_t)np, IpmInfo());
    h->pinfo.assign((size_t)np, IpmInfo());
    h->hinfo.assign((size_t)np, IpmInfo());
    h->active.assign((size_t)np, 1);
    h->held.assign((size_t)np, 0);
    h->held_done.assign((size_t)np, 0);
    h->t_solve0 = now_s();
    h->solve_time = h->setup_time;
    h->solve_current = h->kkt_final = h->grad.done = h->tan.done = h->jac.done = h->vjp.done = false;
    int rc;
    if ((rc = h->default_start())) return rc;
    for (int k = 0; k < np; k++) h->hm(M_ACTIVE, k) = 1;
    if ((rc = h->push_masks())) return rc;
    CHIP_HIP(hipStreamSynchronize(h->stream));
    h->syncs = h->launches = h->loop_iters = 0;
    const double t_loop0 = now_s();
    int iter = 0;
    std::vector<double> rtau((size_t)np), rkap((size_t)np), lkappa((size_t)np);
    std::vector<char> restore((size_t)np);
    while (true) {
#ifdef CHIP_TESTING
        if (h->nan_member >= 0 && h->nan_member < np && iter == h->nan_iter && h->zoff[h->nan_member + 1] > h->zoff[h->nan_member]) {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            CHIP_HIP(hipMemcpyAsync(h->vz + h->zoff[h->nan_member], &nan, 8, hipMemcpyHostToDevice, h->stream));
            CHIP_HIP(hipStreamSynchronize(h->stream));
        }
#endif
        if ((rc = h->residual_pass())) return rc;
        h->solve_time = h->setup_time + (now_s() - h->t_solve0);
        bool any_restore = false;
        for (int k = 0; k < np; k++) {
            if (!h->active[k]) continue;
            IpmInfo &I = h->info[k];
            h->member_info(k);
            I.iterations = iter;
            if (ipm_check_termination(I, st, iter, h->solve_time)) {
                h->active[k] = 0;
                if (I.status == CHIP_SOLVER_INSUFFICIENT_PROGRESS) { // reset_to_prev_iterate (info.rs:244-253)
                    ipm_reset_to_prev(I);
                    restore[k] = 1;
                    any_restore = true;
                    h->tau[k] = h->ptau[k];
                    h->kappa[k] = h->pkappa[k];
                }
                // a member with PSD cones leaves the stack at its final iterate: the last step can take s or z to
                // the cones' boundary within rounding (mu of 1e-16), where the Cholesky factors of the next scaling
                // update -- which the single solver never takes at its final iterate -- break down and no member
                // would account for it.  Its iterate is held aside as it is (restored first, if it is to be) and
                // its s and z become the unit vector; post_process puts it back unchanged
                if (h->has_psd[k]) h->held[k] = 1;
                continue;
            }
            // the pre-update check: s and z finite and strictly interior, x finite
            const bool nonfin = h->red(R_BADX, k) != 0.0 || h->red(R_BADSZ, k) != 0.0;
            const double margin = h->red(R_COUNT, k);
            if (nonfin || !(margin > 0.0)) h->end_member(k, CHIP_SOLVER_NUMERICAL_ERROR, iter, nonfin);
        }
        if (any_restore) {
            for (int k = 0; k < np; k++) h->hm(M_SEL, k) = restore[k];
            if ((rc = h->push_masks())) return rc;
            h->copy_members(h->vx, h->vs, h->vz, h->px, h->ps, h->pz, h->mk(M_SEL));
            std::fill(restore.begin(), restore.end(), 0);
        }
        if ((rc = h->hold_and_reset())) return rc;
        bool any_active = false;
        for (int k = 0; k < np; k++) {
            h->hm(M_ACTIVE, k) = h->active[k];
            any_active = any_active || h->active[k];
        }
        if (!any_active) break;
        if ((rc = h->push_masks())) return rc;
        h->loop_iters++;
        // scale cones and refactor (NN and SOC scalings do not read mu)
        if ((rc = chip_kkt_update_scaling_dev(h->kkt, h->vs, h->vz, 1.0, 0)) < 0) return rc;
        iter++;
        rc = chip_kkt_update(h->kkt, nullptr);
        h->syncs++;
        h->launches++;
        if (rc < 0) return rc;
        bool ok = rc == 1;
        if (ok && (rc = h->constant_rhs(&ok, iter))) return rc;
        if (!ok) { // a failed factorisation that no member accounts for (the reference stops before counting it)
            for (int k = 0; k < np; k++)
                if (h->active[k]) h->end_member(k, CHIP_SOLVER_NUMERICAL_ERROR, iter - 1, false);
            if ((rc = h->hold_and_reset())) return rc;
            break;
        }
        if ((rc = h->hold_and_reset())) return rc;
        // affine step rhs (variables.rs:68-79)
        for (int k = 0; k < np; k++) {
            h->hm(M_ACTIVE, k) = h->active[k];
            rtau[k] = h->info[k].out5[0];
            rkap[k] = h->tau[k] * h->kappa[k];
        }
        if ((rc = h->push_masks())) return rc;
        h->lin(h->dx, h->rx, nullptr, nullptr, nullptr, 1.0, 0.0, 0, nullptr, 0);
        h->lin(h->dz, h->rz, nullptr, nullptr, nullptr, 1.0, 0.0, 1, nullptr, 0);
        if ((rc = chip_kkt_affine_ds_dev(h->kkt, h->ds, h->vs))) return rc;
        ok = true;
        if ((rc = h->solve_direction(h->vs, rtau, rkap, lkappa, &ok, iter))) return rc;
        bool any_flag = false;
        for (int k = 0; k < np; k++) any_flag = any_flag || (h->held[k] && !h->held_done[k]);
        if (!ok && !any_flag) {
            for (int k = 0; k < np; k++)
                if (h->active[k]) h->end_member(k, CHIP_SOLVER_NUMERICAL_ERROR, iter, false);
            if ((rc = h->hold_and_reset())) return rc;
            break;
        }
        if ((rc = h->hold_and_reset())) return rc;
        if ((rc = h->step_length(lkappa, false))) return rc;
        // combined step rhs (variables.rs:81-118)
        for (int k = 0; k < np; k++) {
            const double a = h->alpha[k];
            h->sigma[k] = std::pow(1.0 - a, 3);
            const double mscale = iter > 1 ? 1.0 : a;
            const double sm = h->sigma[k] * h->mu[k];
            h->hs_(S_OMS, k) = 1.0 - h->sigma[k];
            h->hs_(S_ALPHA, k) = mscale;
            h->hs_(S_NEGSM, k) = -sm;
            rkap[k] = -sm + mscale * h->dtau[k] * lkappa[k] + h->tau[k] * h->kappa[k];
            rtau[k] = (1.0 - h->sigma[k]) * h->info[k].out5[0];
        }
        if ((rc = h->push_scalars())) return rc;
        h->lin(h->dx, h->rx, nullptr, h->sc(S_OMS), nullptr, 1.0, 0.0, 0, nullptr, 0);
        if (iter == 1) h->lin(h->lz, h->lz, nullptr, h->sc(S_ALPHA), nullptr, 1.0, 0.0, 1, nullptr, 0);
        if ((rc = chip_kkt_combined_ds_shift_dev(h->kkt, h->dz, h->lz, h->ls, 0.0))) return rc; // dz is work
        dev::bunit_shift(h->stream, h->plan, h->dz, h->sc(S_NEGSM), 0, nullptr);                 // - sigma_mu e
        if (h->psd.ncones) { // (0.5 (Z + Z') - 0 and then - sigma_mu on the diagonal: the single kernel's bits)
            dev::bp_diag_shift(h->stream, h->psd, h->dz, h->sc(S_NEGSM), nullptr);
            h->launches++;
        }
        dev::waxpby(h->stream, h->ds, 1.0, h->ds, 1.0, h->dz, h->pd.m);
        h->lin(h->dz, h->rz, nullptr, h->sc(S_OMS), nullptr, 1.0, 0.0, 1, nullptr, 0);
        if ((rc = chip_kkt_ds_from_dz_offset_dev(h->kkt, h->conicw, h->ds, h->vz))) return rc;
        h->launches += 4;
        ok = true;
        if ((rc = h->solve_direction(h->conicw, rtau, rkap, lkappa, &ok, iter))) return rc;
        any_flag = false;
        for (int k = 0; k < np; k++) any_flag = any_flag || (h->held[k] && !h->held_done[k]);
        if (!ok && !any_flag) {
            for (int k = 0; k < np; k++)
                if (h->active[k]) h->end_member(k, CHIP_SOLVER_NUMERICAL_ERROR, iter, false);
            if ((rc = h->hold_and_reset())) return rc;
            break;
        }
        if ((rc = h->hold_and_reset())) return rc;
        if ((rc = h->step_length(lkappa, true))) return rc;
        // strategy_checkpoint_small_step (core/solver.rs:630-654) per member
        for (int k = 0; k < np; k++) {
            if (!h->active[k]) {
                h->alpha[k] = 0.0;
                continue;
            }
            if (h->alpha[k] <= std::max(0.0, st.min_terminate_step_length)) {
                h->alpha[k] = 0.0;
                h->info[k].status = CHIP_SOLVER_INSUFFICIENT_PROGRESS;
                h->info[k].iterations = iter;
                h->active[k] = 0;
            }
        }
        // save_prev_iterate + add_step: the new iterate goes into the previous iterate's buffers and the two swap;
        // frozen members copy their iterate (a select, never 0 * step)
        for (int k = 0; k < np; k++) {
            h->hm(M_ACTIVE, k) = h->active[k];
            h->hs_(S_ALPHA, k) = h->alpha[k];
            if (!h->active[k]) continue;
            IpmInfo &I = h->info[k];
            h->pinfo[k] = I;
            ipm_save_prev(I);
            h->ptau[k] = h->tau[k];
            h->pkappa[k] = h->kappa[k];
            h->tau[k] = h->tau[k] + h->alpha[k] * h->dtau[k];
            h->kappa[k] = h->kappa[k] + h->alpha[k] * lkappa[k];
        }
        if ((rc = h->push_scalars()) || (rc = h->push_masks())) return rc;
        h->lin(h->px, h->lx, h->vx, h->sc(S_ALPHA), nullptr, 1.0, 1.0, 0, h->mk(M_ACTIVE), dev::MASK_Y);
        h->lin(h->ps, h->ls, h->vs, h->sc(S_ALPHA), nullptr, 1.0, 1.0, 1, h->mk(M_ACTIVE), dev::MASK_Y);
        h->lin(h->pz, h->lz, h->vz, h->sc(S_ALPHA), nullptr, 1.0, 1.0, 1, h->mk(M_ACTIVE), dev::MASK_Y);
        CHIP_HIP(hipGetLastError());
        std::swap(h->vx, h->px);
        std::swap(h->vs, h->ps);
        std::swap(h->vz, h->pz);
    }
    h->iteration_time = now_s() - t_loop0;
    if ((rc = h->post_process())) return rc;
    h->solve_time = h->setup_time + (now_s() - h->t_solve0);
    h->solved_once = true;
    h->solve_current = true;
    return CHIP_OK;
}

static void fill_info(const chip_batch *h, int k, chip_solution_info *out) {
    const bool done = h->solved_once; // (the per-member vectors are empty before the first solve)
    fill_solution_info(out, done, done ? h->info[k] : IpmInfo(), done ? h->obj_val[k] : 0.0,
                       done ? h->obj_val_dual[k] : 0.0, h->solve_time, h->setup_time, h->equilibration_time,
                       h->iteration_time);
}

int32_t chip_batch_get_info(chip_batch *h, chip_solution_info *infos) {
    if (!h || !infos) return fail(CHIP_ERR_ARG, "chip_batch_get_info: bad argument");
    for (int k = 0; k < h->nprob; k++) fill_info(h, k, infos + k);
    return CHIP_OK;
}

int32_t chip_batch_get_solution(chip_batch *h, int64_t k, double *x, double *s, double *z, chip_solution_info *info) {
    if (!h || k < 0 || k >= h->nprob) return fail(CHIP_ERR_ARG, "chip_batch_get_solution: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    const int x0 = h->xoff[k], nk = h->xoff[k + 1] - x0, z0 = h->zoff[k], mk_ = h->zoff[k + 1] - z0;
    if (h->solved_once) {
        if (x && nk) CHIP_HIP(hipMemcpy(x, h->xo + x0, (size_t)nk * 8, hipMemcpyDeviceToHost));
        if (s && mk_) CHIP_HIP(hipMemcpy(s, h->so + z0, (size_t)mk_ * 8, hipMemcpyDeviceToHost));
        if (z && mk_) CHIP_HIP(hipMemcpy(z, h->zo + z0, (size_t)mk_ * 8, hipMemcpyDeviceToHost));
    } else {
        if (x) std::fill(x, x + nk, 0.0);
        if (s) std::fill(s, s + mk_, 0.0);
        if (z) std::fill(z, z + mk_, 0.0);
    }
    if (info) fill_info(h, (int)k, info);
    return CHIP_OK;
}

int32_t chip_batch_get_solution_dev(chip_batch *h, double **x_dev, double **s_dev, double **z_dev) {
    if (!h) return fail(CHIP_ERR_ARG, "chip_batch_get_solution_dev: bad argument");
    if (x_dev) *x_dev = h->xo;
    if (s_dev) *s_dev = h->so;
    if (z_dev) *z_dev = h->zo;
    return CHIP_OK;
}

int32_t chip_batch_get_equilibration(chip_batch *h, int64_t k, double *d, double *e, double *c) {
    if (!h || k < 0 || k >= h->nprob) return fail(CHIP_ERR_ARG, "chip_batch_get_equilibration: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    const int x0 = h->xoff[k], nk = h->xoff[k + 1] - x0, z0 = h->zoff[k], mk_ = h->zoff[k + 1] - z0;
    if (d && nk) CHIP_HIP(hipMemcpy(d, h->pd.d + x0, (size_t)nk * 8, hipMemcpyDeviceToHost));
    if (e && mk_) CHIP_HIP(hipMemcpy(e, h->pd.e + z0, (size_t)mk_ * 8, hipMemcpyDeviceToHost));
    if (c) *c = h->c[k];
    return CHIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Data updates of the stack (chip_bdata_*; default/data_updating.rs with one cost scale per member): new values on the
// fixed patterns, scaled on the device with the setup's d, e and the members' c_k, then every copy the loop reads is
// refreshed.  What create derives from the values and the loop reads: the scaled M.Px / M.Ax, q, b
// and negq; K's device store; the L3 handle's mirrors of P and A (kktsystem_spmv) and its q, b; max |P_ii| of the
// static regulariser over the whole stack; normq[k] and normb[k] of the members' UNSCALED q and b.  One call is a
// fixed number of launches and ONE host synchronisation: a partial form's writes read the word the index check
// raised on the device, so a refused call has written nothing when the host learns of it.
// ---------------------------------------------------------------------------------------------------------------
int chip_batch::update_work() {
    if (uflag) return CHIP_OK;
    const size_t len = (size_t)std::max({pd.M.nnzP, pd.M.nnzA, pd.n, pd.m, 1});
    int rc;
    if ((rc = mem.alloc(&upos, len)) || (rc = mem.alloc(&unpart, (size_t)dev::pu_norm_partials())) ||
        (rc = mem.alloc(&unout, 3)) || (rc = mem.alloc(&ubpart, (size_t)(plan.ncx + plan.ncz))) ||
        (rc = mem.alloc(&ubout, (size_t)nprob)) || (rc = mem.alloc(&uflag, 1)))
        return rc;
    unorm.assign((size_t)nprob, 0.0);
    CHIP_HIP(hipMemsetAsync(upos, 0xff, len * sizeof(int), stream)); // every slot -1
    CHIP_HIP(hipMemsetAsync(uflag, 0, sizeof(int), stream));
    upd_launches += 2;
    return CHIP_OK;
}

// one update of P, A, q or b: idx_dev == nullptr is the full form (k == the length, checked by the caller)
int chip_batch::update(int which, const int64_t *idx_dev, const double *vals_dev, int k) {
    int rc;
    if ((rc = update_work())) return rc;
    // from the first write on the last solve's iterate no longer belongs to the data: no gradient until the next solve
    // (chip_bgrad_*).  Only the refusal that has changed nothing puts the flag back; a call that fails on the way does not
    // K's factorisation is not vouched for either (chip_bjvp_*); that flag stays down even after such a refusal, which
    // costs the next apply one refactor
    const bool was_current = solve_current;
    solve_current = kkt_final = false;
    const int len = (int)pd.update_len(which);
    const dev::EqMats &M = pd.M;
    hipStream_t s = stream;
    if (idx_dev) { // the whole index list is checked on the device before any pass writes
        if ((rc = grow_dev(&clean, &clean_cap, (size_t)k, s, &upd_syncs))) return rc;
        CHIP_HIP(hipMemsetAsync(uflag, 0, sizeof(int), s));
        dev::pu_validate(s, idx_dev, k, len, uflag);
        upd_launches += 2;
    }
    dev::BuTarget t{};
    switch (which) {
    case UPD_P: t = {M.Px, nullptr, nullptr, len, M.Prow, M.Pcol, pd.d, pd.d, dc, plan.xmem}; break;
    case UPD_A: t = {M.Ax, nullptr, nullptr, len, M.Arow, M.Acol, pd.e, pd.d, nullptr, plan.xmem}; break;
    case UPD_Q: t = {pd.q, uq, negq, len, nullptr, nullptr, pd.d, nullptr, dc, plan.xmem}; break;
    default: t = {pd.b, ub, nullptr, len, nullptr, nullptr, pd.e, nullptr, nullptr, plan.zmem}; break;
    }
    if (idx_dev) {
        dev::bu_write_partial(s, t, idx_dev, vals_dev, k, upos, uflag, clean);
        upd_launches += 3;
    } else {
        dev::bu_write_full(s, t, vals_dev);
        upd_launches++;
    }
    CHIP_HIP(hipGetLastError());
    // the copies the loop reads: K's values (only the touched entries of a partial form; a refused one rewrites
    // entry 0 with its own value), the L3 mirrors and vectors
    if (which == UPD_P || which == UPD_A) {
        const double *src = which == UPD_P ? M.Px : M.Ax;
        if ((rc = kkt_update_values_dev(kkt, which, src, idx_dev ? clean : nullptr, idx_dev ? k : len))) return rc;
        upd_launches++;
    }
    if ((rc = kktsystem_update_data_dev(sys, which == UPD_P ? M.Px : nullptr, which == UPD_A ? M.Ax : nullptr,
                                        which == UPD_Q ? pd.q : nullptr, which == UPD_B ? pd.b : nullptr)))
        return rc;
    upd_launches += (which == UPD_A || which == UPD_Q) ? 2 : 1; // A: two mirrors; q: the copy and its negation
    // the scalars create derived from the values: the members' norms of the unscaled q / b, max |P_ii| of the stack
    double pmax[3] = {0, 0, 0};
    if (which == UPD_Q || which == UPD_B) {
        dev::bu_norms(s, plan, which == UPD_Q ? 0 : 1, which == UPD_Q ? uq : ub, ubpart, ubout);
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipMemcpyAsync(unorm.data(), ubout, (size_t)nprob * 8, hipMemcpyDeviceToHost, s));
        upd_launches += 3;
    } else if (which == UPD_P) {
        dev::pu_norms(s, 4, nullptr, nullptr, 0, nullptr, nullptr, 0, M.Prow, M.Pcol, M.Px, M.nnzP, unpart, unout);
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipMemcpyAsync(pmax, unout, sizeof(pmax), hipMemcpyDeviceToHost, s));
        upd_launches += 3;
    }
    int bad = 0;
    if (idx_dev) {
        CHIP_HIP(hipMemcpyAsync(&bad, uflag, sizeof(int), hipMemcpyDeviceToHost, s));
        upd_launches++;
    }
    CHIP_HIP(hipStreamSynchronize(s));
    upd_syncs++;
    if (bad) {
        solve_current = was_current;
        return fail(CHIP_ERR_DIM, update_fn(UPD_PREFIX, which) + ": an index is out of range (nothing changed)");
    }
    if (which == UPD_Q) normq = unorm;
    if (which == UPD_B) normb = unorm;
    if (which == UPD_P) kkt_set_static_diag_max(kkt, pmax[2]);
    return CHIP_OK;
}

int chip_batch::update_args(chip_batch *h, int which, const void *idx, const double *vals, int64_t k) {
    const std::string fn = update_fn(UPD_PREFIX, which);
    const int64_t len = h ? h->pd.update_len(which) : 0;
    const int rc = chip::update_args(fn, h, idx, vals, k, len, [&] {
        h->upd_syncs = h->upd_launches = 0;
        return 0;
    });
    if (rc == 0 && idx && len == 0) // (every index is out of range)
        return fail(CHIP_ERR_DIM, fn + ": an index is out of range (nothing changed)");
    return rc;
}

CHIP_UPDATE_ENTRIES(chip_bdata_update_, chip_batch)

// ---------------------------------------------------------------------------------------------------------------
// Re-equilibration of the stack: new full data on the fixed patterns, equilibrated from d = e = 1,
// c_k = 1 by create's own ProblemData::equilibrate on the handle's stream, then every copy and derived value of the
// audit refreshed by the data updates' passes; the partition, chip_kkt and chip_kktsystem are left alone.  The number
// of enqueues does not depend on nprob, and the one host synchronisation is equilibrate's own: the members' c_k, their
// norms and max |P_ii| come back in it.
// ---------------------------------------------------------------------------------------------------------------
int chip_batch::reequilibrate_gate(const char *) {
    upd_syncs = upd_launches = 0;
    return CHIP_OK;
}

int chip_batch::reequilibrate(const double *P_dev, const double *q_dev, const double *A_dev, const double *b_dev) {
    int rc;
    if ((rc = update_work())) return rc;
    const size_t np = (size_t)nprob;
    if (!req_out && ((rc = mem.alloc(&eq_colsum, np)) || (rc = mem.alloc(&req_out, 2 * np + 3)))) return rc;
    req_host.assign(2 * np + 3, 0.0);
    // as after an update that changed something: no gradient and no reuse of K's factorisation until the next solve
    solve_current = kkt_final = grad.done = tan.done = jac.done = vjp.done = false;
    const double te = now_s();
    hipStream_t s = stream;
    const dev::EqMats &M = pd.M;
    // the raw values with the unscaled copies of q and (capped) b, and the members' norms of those copies
    pd.reload(s, P_dev, q_dev, A_dev, b_dev, uq, ub);
    dev::bu_norms(s, plan, 0, uq, ubpart, req_out);
    dev::bu_norms(s, plan, 1, ub, ubpart, req_out + np);
    CHIP_HIP(hipGetLastError());
    upd_launches += 8;
    auto ruiz_step = [&](unsigned long long *bits, double *cstate) {
        dev::batch_eq_ruiz_step(s, plan, M, pd.q, pd.b, pd.d, pd.e, bits, seg_scr, eq_colsum, cstate,
                                st.equilibrate_min_scaling, st.equilibrate_max_scaling);
        upd_launches += 2; // (with the clear of bits)
    };
    rc = pd.equilibrate(s, st, cones, nprob, dev::batch_eq_bits_words(pd.n, pd.m, nprob), ruiz_step, c.data(),
                        [&](const double *cstate) -> int {
        // the members' cost scales on the device, then the copies the loop reads (4.14's audit), from the
        // equilibrated arrays in place
        CHIP_HIP(hipMemcpyAsync(dc, cstate, np * 8, hipMemcpyDeviceToDevice, s));
        int rc1;
        if ((rc1 = kkt_update_values_dev(kkt, UPD_P, M.Px, nullptr, M.nnzP)) ||
            (rc1 = kkt_update_values_dev(kkt, UPD_A, M.Ax, nullptr, M.nnzA)) ||
            (rc1 = kktsystem_update_data_dev(sys, M.Px, M.Ax, pd.q, pd.b)))
            return rc1;
        dev::waxpby(s, negq, -1.0, pd.q, 0.0, nullptr, pd.n);
        dev::pu_norms(s, 4, nullptr, nullptr, 0, nullptr, nullptr, 0, M.Prow, M.Pcol, M.Px, M.nnzP, unpart,
                      req_out + 2 * np);
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipMemcpyAsync(req_host.data(), req_out, req_host.size() * 8, hipMemcpyDeviceToHost, s));
        upd_launches += 1 + 2 + 5 + 1 + 2 + 1;
        return (int)CHIP_OK;
    });
    upd_launches += 7; // d, e, cstate, the rectification, the inversion (or dinv, einv), the c_k
    upd_syncs++;
    if (rc) return rc;
    normq.assign(req_host.begin(), req_host.begin() + nprob);
    normb.assign(req_host.begin() + nprob, req_host.begin() + 2 * nprob);
    kkt_set_static_diag_max(kkt, req_host[2 * np + 2]);
    equilibration_time = now_s() - te;
    return CHIP_OK;
}

int32_t chip_reequilibrate_bdata(chip_batch *h, const double *Pnzval, const double *q, const double *Anzval,
                                 const double *b) {
    return reequilibrate_entry("chip_reequilibrate_bdata", h, Pnzval, q, Anzval, b, true);
}
int32_t chip_reequilibrate_bdata_dev(chip_batch *h, const double *Pnzval_dev, const double *q_dev,
                                     const double *Anzval_dev, const double *b_dev) {
    return reequilibrate_entry("chip_reequilibrate_bdata_dev", h, Pnzval_dev, q_dev, Anzval_dev, b_dev, false);
}

// update_settings with validate_as_update (settings.rs:307): the immutable fields of chip_problem_update_settings
int32_t chip_bdata_update_settings(chip_batch *h, const chip_solver_settings *settings) {
    if (!h || !settings) return fail(CHIP_ERR_ARG, "chip_bdata_update_settings: bad argument");
    chip_solver_settings nw = *settings;
    if (int rc = validate_settings_update(h->st, nw, "chip_bdata_update_settings")) return rc;
    h->st = nw;
    return CHIP_OK;
}

int32_t chip_bdata_get_scaled(chip_batch *h, double *Px, double *Ax, double *q, double *b, double *normq,
                              double *normb) {
    if (!h) return fail(CHIP_ERR_ARG, "chip_bdata_get_scaled: bad argument");
    CHIP_HIP(hipSetDevice(h->pd.device));
    if (int rc = h->pd.get_scaled(h->stream, Px, Ax, q, b)) return rc;
    if (normq) std::copy(h->normq.begin(), h->normq.end(), normq);
    if (normb) std::copy(h->normb.begin(), h->normb.end(), normb);
    return CHIP_OK;
}
