// kkt_cones.cpp -- the cones of an L2 handle: the device tables (KktCones::build), the cone passes and their entry
// points chip_kkt_*_dev of include/clarabel_hip.h
#include <cmath>

#include "batch_psd.hpp"
#include "kkt_handle.hpp"

namespace chip {

// uploads v through the engine (which owns the allocation) and stores the pointer in a view's field
template <typename T> static int up(Engine &E, const T *&field, const std::vector<T> &v) {
    T *p = nullptr;
    const int rc = E.upload(&p, v, v.size());
    field = p;
    return rc;
}
// `count` doubles of state, cleared; an allocation of its own (a kernel that runs past its tables faults instead of
// reading a neighbour's)
static int zeroed(Engine &E, double *&field, size_t count) {
    int rc = E.alloc(&field, count);
    if (rc) return rc;
    CHIP_HIP(hipMemset(field, 0, (count ? count : 1) * sizeof(double)));
    return CHIP_OK;
}

int KktCones::build(Engine &E, const KktLayout &K, const bigvec &k2v, const int *mapHs, const double *alphas, i64 n) {
    std::vector<int> nn, nn_hs, zero;
    ConeList socs, ns3s, gpws;
    PsdSizing pd;
    for (const ConeSpec &c : K.cones) {
        switch (c.tag) {
        case CHIP_CONE_NONNEGATIVE:
            for (i64 k = 0; k < c.numel; k++) {
                nn.push_back((int)(c.start + k));
                nn_hs.push_back((int)(c.block_start + k));
            }
            break;
        case CHIP_CONE_ZERO:
            for (i64 k = 0; k < c.numel; k++) zero.push_back((int)(c.start + k));
            break;
        case CHIP_CONE_SECONDORDER: socs.push_back(&c); break;
        case CHIP_CONE_POWER:
            if (const double al = alphas ? alphas[(size_t)(&c - K.cones.data())] : 0.5; !(al > 0.0 && al < 1.0))
                return fail(CHIP_ERR_ARG, "PowerConeT exponent must lie in (0,1)");
            [[fallthrough]];
        case CHIP_CONE_EXPONENTIAL: ns3s.push_back(&c); break;
        case CHIP_CONE_GENPOWER: gpws.push_back(&c); break;
        case CHIP_CONE_PSDTRIANGLE: pd.add(c.start, c.dim, c.block_start); break;
        default: has_hostHs = true;
        }
    }
    int rc;
    if ((rc = build_genpow(E, K, gpws, k2v, mapHs))) return rc;
    if ((rc = build_psd(E, pd, mapHs, n))) return rc;
    if ((rc = build_ns3(E, K, ns3s, alphas, mapHs))) return rc;
    nn_count = (int)nn.size();
    zero_count = (int)zero.size();
    if ((rc = up(E, nn_rows, nn))) return rc;
    if ((rc = up(E, nn_hsidx, nn_hs))) return rc;
    if ((rc = up(E, zero_rows, zero))) return rc;
    return build_soc(E, K, socs, k2v, mapHs);
}

int KktCones::build_genpow(Engine &E, const KktLayout &K, const ConeList &cones, const bigvec &k2v, const int *mapHs) {
    std::vector<int> start, d1, d2, hs, off, mapptr, map, mapD;
    i64 state = 0;
    for (const ConeSpec *cp : cones) {
        const ConeSpec &c = *cp;
        start.push_back((int)c.start);
        d1.push_back((int)c.dim);
        d2.push_back((int)c.dim2);
        hs.push_back((int)c.block_start);
        off.push_back((int)state);
        state += 6 * c.dim + 4 * c.dim2 + 3;
        mapptr.push_back((int)map.size());
        const i64 sidx = c.sparse_idx;
        for (i64 k = 0; k < c.dim; k++) map.push_back(k2v[(size_t)K.sp_q[K.sp_q_ptr[sidx] + k]]);
        for (i64 k = 0; k < c.dim2; k++) map.push_back(k2v[(size_t)K.sp_r[K.sp_r_ptr[sidx] + k]]);
        for (i64 k = 0; k < c.numel; k++) map.push_back(k2v[(size_t)K.sp_u[K.sp_ptr[sidx] + k]]);
        for (int k = 0; k < 3; k++) mapD.push_back(k2v[(size_t)K.sp_D[3 * sidx + k]]);
        gpw_cone_index.push_back((int)(&c - K.cones.data()));
    }
    int rc;
    gpw.ncones = (int)start.size();
    if ((rc = up(E, gpw.start, start))) return rc;
    if ((rc = up(E, gpw.dim1, d1))) return rc;
    if ((rc = up(E, gpw.dim2, d2))) return rc;
    if ((rc = up(E, gpw.hs_start, hs))) return rc;
    if ((rc = up(E, gpw.state_off, off))) return rc;
    if ((rc = up(E, gpw.map_ptr, mapptr))) return rc;
    if ((rc = up(E, gpw.mapQRP, map))) return rc;
    if ((rc = up(E, gpw.mapD, mapD))) return rc;
    // state: alpha defaults to 1/dim1 with psi = 1 / sum alpha^2 until chip_kkt_set_genpow_alpha
    std::vector<double> st0((size_t)(state ? state : 1), 0.0);
    for (size_t c = 0; c < start.size(); c++) {
        double *st = st0.data() + off[c];
        for (int k = 0; k < d1[c]; k++) st[k] = 1.0 / d1[c];
        st[6 * d1[c] + 4 * d2[c] + 1] = 1.0;            // mu
        st[6 * d1[c] + 4 * d2[c] + 2] = (double)d1[c]; // psi
    }
    if ((rc = E.upload(&gpw.state, st0, st0.size()))) return rc;
    gpw.mapHs = mapHs;
    gpw_state_off = off;
    gpw_dim1 = d1;
    return CHIP_OK;
}

// entry t of a cone's svec (column-major upper triangle) as i | j << 16
static i32 svec_ij(i64 t) {
    i32 j = (i32)((std::sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((i64)j * (j + 1) / 2 > t) j--;
    while ((i64)(j + 1) * (j + 2) / 2 <= t) j++;
    return (i32)(t - (i64)j * (j + 1) / 2) | (j << 16);
}
// every cone's Hs block one of the dense diagonal blocks of the top?  Then Hs is written row by row of the device's
// value order (k_psd_write_hs_rows) instead of through mapHs
int KktCones::psd_dense_blocks(Engine &E, const PsdSizing &pd, i64 n) {
    const int nblk = E.dblk.nblk;
    std::vector<i32> blk_cone((size_t)nblk, -1), row_ij(E.h_dblk_node.size(), 0);
    std::vector<char> covered(pd.start.size(), 0);
    size_t nc = 0;
    for (int b = 0, o = 0; b < nblk; o += E.h_dblk_m[(size_t)b], b++) {
        const i32 mb = E.h_dblk_m[(size_t)b];
        const i64 z0 = (i64)E.h_perm[(size_t)E.h_dblk_node[(size_t)o]] - n;
        if (z0 < 0) continue;
        // the cone that holds z0 (cones ascend by start)
        const size_t c = (size_t)(std::upper_bound(pd.start.begin(), pd.start.end(), (i32)z0) - pd.start.begin());
        if (c == 0) continue;
        const i32 st = pd.start[c - 1], nd = pd.dim[c - 1], numel = nd * (nd + 1) / 2;
        if (mb != numel || covered[c - 1]) continue;
        bool ok = true;
        for (i32 a = 0; a < mb && ok; a++) {
            const i64 t = (i64)E.h_perm[(size_t)E.h_dblk_node[(size_t)(o + a)]] - n - st;
            ok = t >= 0 && t < numel;
            if (ok) row_ij[(size_t)(o + a)] = svec_ij(t);
        }
        if (!ok) continue;
        blk_cone[(size_t)b] = (i32)(c - 1);
        covered[c - 1] = 1;
        nc++;
    }
    if (nc != pd.start.size()) return CHIP_OK;
    // (every dense block belongs to a cone: the blocks may be written into L directly, Engine::hs_direct_begin)
    psd_rows_all_blocks = std::all_of(blk_cone.begin(), blk_cone.end(), [](i32 c) { return c >= 0; });
    int rc;
    if ((rc = up(E, psd.blk_cone, blk_cone))) return rc;
    if ((rc = up(E, psd.row_ij, row_ij))) return rc;
    psd.rows_nblk = nblk;
    psd.blk_m = E.dblk.m;
    psd.blk_rowbase = E.dblk.rowbase;
    psd.blk_start = E.dblk.start;
    return CHIP_OK;
}
int KktCones::build_psd(Engine &E, const PsdSizing &pd, const int *mapHs, i64 n) {
    int rc = psd_view_build(E, psd, pd, mapHs, &E.mb_dev->soc_fail);
    if (rc) return rc;
    if (psd.ncones > 0 && pd.maxdim <= 64 && E.dblk.nblk > 0) return psd_dense_blocks(E, pd, n);
    return CHIP_OK;
}

int KktCones::build_ns3(Engine &E, const KktLayout &K, const ConeList &cones, const double *alphas, const int *mapHs) {
    std::vector<int> start, hs, tag;
    std::vector<double> alpha;
    for (const ConeSpec *c : cones) {
        start.push_back((int)c->start);
        hs.push_back((int)c->block_start);
        tag.push_back((int)c->tag);
        alpha.push_back(alphas ? alphas[(size_t)(c - K.cones.data())] : 0.5);
    }
    int rc;
    ns3.ncones = (int)start.size();
    if ((rc = up(E, ns3.start, start))) return rc;
    if ((rc = up(E, ns3.hs_start, hs))) return rc;
    if ((rc = up(E, ns3.tag, tag))) return rc;
    if ((rc = up(E, ns3.alpha, alpha))) return rc;
    if ((rc = zeroed(E, ns3.state, (size_t)(ns3.ncones ? ns3.ncones : 1) * 18))) return rc;
    ns3.mapHs = mapHs;
    return CHIP_OK;
}

int KktCones::build_soc(Engine &E, const KktLayout &K, const ConeList &cones, const bigvec &k2v, const int *mapHs) {
    std::vector<int> start, dim, hs, sidx, ptr, mapU, mapV, mapD;
    for (const ConeSpec *c : cones) {
        start.push_back((int)c->start);
        dim.push_back((int)c->numel);
        hs.push_back((int)c->block_start);
        sidx.push_back((int)c->sparse_idx);
    }
    // the sparse cones' extra columns (u, v, D of every sparse cone of K, SecondOrder and GenPow alike)
    const size_t nsp = K.sp_ptr.size() ? K.sp_ptr.size() - 1 : 0, nuv = (size_t)(nsp ? K.sp_ptr[nsp] : 0);
    for (size_t s = 0; s <= nsp; s++) ptr.push_back((int)K.sp_ptr[s]);
    for (size_t k = 0; k < nuv; k++) {
        mapU.push_back(k2v[(size_t)K.sp_u[k]]);
        mapV.push_back(k2v[(size_t)K.sp_v[k]]);
    }
    for (size_t s = 0; s < nsp; s++) {
        mapD.push_back(k2v[(size_t)K.sp_D[3 * s]]);
        mapD.push_back(k2v[(size_t)K.sp_D[3 * s + 1]]);
    }
    int rc;
    soc.ncones = (int)start.size();
    if ((rc = up(E, soc.start, start))) return rc;
    if ((rc = up(E, soc.dim, dim))) return rc;
    if ((rc = up(E, soc.hs_start, hs))) return rc;
    if ((rc = up(E, soc.sparse_idx, sidx))) return rc;
    if ((rc = up(E, soc.sp_ptr, ptr))) return rc;
    if ((rc = up(E, soc.mapU, mapU))) return rc;
    if ((rc = up(E, soc.mapV, mapV))) return rc;
    if ((rc = up(E, soc.mapD, mapD))) return rc;
    soc.mapHs = mapHs;
    if ((rc = zeroed(E, d_w, (size_t)K.m))) return rc;
    if ((rc = zeroed(E, d_lam, (size_t)K.m))) return rc;
    soc.w = d_w;
    soc.lam = d_lam;
    if ((rc = zeroed(E, soc.eta, (size_t)(soc.ncones ? soc.ncones : 1) * 8))) return rc;
    soc.d = soc.eta;
    soc.fail = &E.mb_dev->soc_fail;
    return CHIP_OK;
}

// ---- the cone passes ------------------------------------------------------------------------------------------------
void KktCones::update_scaling(Engine &E, const double *s_dev, const double *z_dev, double mu, int strategy) {
    dev::sym_update_scaling(E.stream, soc, nn_rows, nn_count, s_dev, z_dev, d_w, d_lam);
    dev::ns3_update_scaling(E.stream, ns3, s_dev, z_dev, mu, strategy);
    dev::gpw_update_scaling(E.stream, gpw, z_dev, mu);
    dev::psd_update_scaling(E.stream, psd, s_dev, z_dev);
}
void KktCones::write_kkt(Engine &E, const int *mapHs, unsigned long long *dslots) {
    dev::sym_write_kkt(E.stream, soc, nn_rows, nn_hsidx, nn_count, d_w, mapHs, E.Kx, dslots);
    dev::ns3_write_hs(E.stream, ns3, E.Kx);
    dev::gpw_write_kkt(E.stream, gpw, E.Kx);
    // PSD blocks that are dense diagonal blocks of the top, contiguous in L too: written into K AND L by the one kernel
    const bool direct = psd_direct_rows() && E.hs_direct_begin();
    dev::psd_write_hs(E.stream, psd, E.Kx, direct ? E.Lx : nullptr, direct ? E.dblk_l0 : nullptr);
}
void KktCones::scale_write(Engine &E, const double *s_dev, const double *z_dev, const int *mapHs, int *status_or_null,
                           long long *dbg) {
    dev::SocView sview = soc;
    sview.dbg = dbg;
    dev::sym_scale_write(E.stream, sview, nn_rows, nn_hsidx, nn_count, s_dev, z_dev, d_w, d_lam, mapHs, E.Kx,
                         E.diag_slots(), status_or_null);
}
void KktCones::mul_Hs(Engine &E, double *y_dev, const double *x_dev) {
    dev::cones_mul_Hs(E.stream, nn_rows, nn_count, soc, zero_rows, zero_count, y_dev, x_dev);
    dev::ns3_mul_hs(E.stream, ns3, y_dev, x_dev);
    dev::gpw_mul_hs(E.stream, gpw, y_dev, x_dev);
    dev::psd_mul_hs(E.stream, psd, y_dev, x_dev);
}
void KktCones::unit_shift(Engine &E, double *z_dev, double alpha, int primal_cone) {
    dev::cone_unit_shift(E.stream, nn_rows, nn_count, zero_rows, zero_count, soc, z_dev, alpha, primal_cone ? 1 : 0);
    dev::psd_unit_shift(E.stream, psd, z_dev, alpha);
}
void KktCones::affine_ds(Engine &E, double *ds_dev, const double *s_dev) {
    dev::cone_affine_ds(E.stream, nn_rows, nn_count, zero_rows, zero_count, soc, ds_dev);
    dev::ns3_affine_ds(E.stream, ns3, ds_dev, s_dev);
    dev::gpw_copy(E.stream, gpw, ds_dev, s_dev);
    dev::psd_affine_ds(E.stream, psd, ds_dev);
}
void KktCones::combined_ds_shift(Engine &E, double *shift_dev, double *step_z_dev, double *step_s_dev, double sigma_mu) {
    dev::cone_combined_ds_shift(E.stream, nn_rows, nn_count, zero_rows, zero_count, soc, shift_dev, step_z_dev,
                                step_s_dev, sigma_mu);
    dev::ns3_combined_ds_shift(E.stream, ns3, shift_dev, step_z_dev, step_s_dev, sigma_mu);
    dev::gpw_combined_ds_shift(E.stream, gpw, shift_dev, sigma_mu);
    dev::psd_combined_ds_shift(E.stream, psd, shift_dev, step_z_dev, step_s_dev, sigma_mu);
}
void KktCones::ds_from_dz_offset(Engine &E, double *out_dev, const double *ds_dev, const double *z_dev) {
    dev::cone_ds_from_dz_offset(E.stream, nn_rows, nn_count, zero_rows, zero_count, soc, out_dev, ds_dev, z_dev);
    dev::ns3_ds_from_dz_offset(E.stream, ns3, out_dev, ds_dev);
    dev::gpw_copy(E.stream, gpw, out_dev, ds_dev);
    dev::psd_ds_from_dz_offset(E.stream, psd, out_dev, ds_dev);
}
void KktCones::unit_initialization(Engine &E, double *z_dev, double *s_dev, int m) {
    dev::cone_unit_initialization(E.stream, nn_rows, nn_count, soc, ns3, z_dev, s_dev, m);
    dev::psd_unit_initialization(E.stream, psd, z_dev, s_dev);
    dev::gpw_unit_initialization(E.stream, gpw, z_dev, s_dev);
}

int KktCones::ensure_partials(Engine &E) {
    if (d_partial) return CHIP_OK;
    partial_cap = 1024 + soc.ncones + psd.ncones + gpw.ncones + (ns3.ncones + 255) / 256 + 8;
    int rc = E.alloc(&d_partial, (size_t)partial_cap * 2);
    if (rc) return rc;
    h_partial.resize((size_t)partial_cap * 2);
    return CHIP_OK;
}
// the first `used` partials of each of the `halves` halves of d_partial -> the same places of h_partial, then the host
// waits for the stream
int KktCones::fetch_partials(Engine &E, int used, int halves) {
    for (int k = 0; k < halves; k++)
        CHIP_HIP(hipMemcpyAsync(h_partial.data() + (size_t)k * partial_cap, d_partial + (size_t)k * partial_cap,
                                (size_t)used * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    CHIP_HIP(hipStreamSynchronize(E.stream));
    return CHIP_OK;
}
int KktCones::step_length(Engine &E, const double *dz_dev, const double *ds_dev, const double *z_dev, const double *s_dev,
                          double alpha_max, double *alpha_out) {
    int rc = ensure_partials(E);
    if (rc) return rc;
    // symmetric cones first (compositecone.rs:326-327)
    int used = dev::cone_step_length(E.stream, nn_rows, nn_count, soc, dz_dev, ds_dev, z_dev, s_dev, alpha_max, d_partial, 1024);
    used += dev::psd_step_length(E.stream, psd, dz_dev, ds_dev, alpha_max, d_partial + used);
    double a = alpha_max;
    if (used) {
        if ((rc = fetch_partials(E, used, 1))) return rc;
        for (int i = 0; i < used; i++) a = std::min(a, h_partial[i]); // T::min: NaN-ignoring like f64::min
    }
    if (ns3.ncones || gpw.ncones) { // back off from the boundary, then the nonsymmetric cones (:329-337)
        a = std::min(a, 1.0 - std::sqrt(2.220446049250313e-16));
        used = dev::ns3_step_length(E.stream, ns3, dz_dev, ds_dev, z_dev, s_dev, a, E.st.min_terminate_step_length,
                                    E.st.linesearch_backtrack_step, d_partial);
        used += dev::gpw_step_length(E.stream, gpw, dz_dev, ds_dev, z_dev, s_dev, a, E.st.min_terminate_step_length,
                                     E.st.linesearch_backtrack_step, d_partial + used);
        if ((rc = fetch_partials(E, used, 1))) return rc;
        for (int i = 0; i < used; i++) a = std::min(a, h_partial[i]);
    }
    *alpha_out = a;
    return CHIP_OK;
}
int KktCones::barrier(Engine &E, const double *z_dev, const double *s_dev, const double *dz_dev, const double *ds_dev,
                      double alpha, double *barrier_out) {
    int rc = ensure_partials(E);
    if (rc) return rc;
    int used = dev::cone_barrier(E.stream, nn_rows, nn_count, soc, ns3, z_dev, s_dev, dz_dev, ds_dev, alpha, d_partial);
    used += dev::psd_barrier(E.stream, psd, z_dev, s_dev, dz_dev, ds_dev, alpha, d_partial + used);
    // scratch for the GenPow primal gradients: the cones' own slices of the (otherwise NN / SOC) w state
    used += dev::gpw_barrier(E.stream, gpw, z_dev, s_dev, dz_dev, ds_dev, alpha, d_partial + used, d_w);
    double b = 0.0;
    if (used) {
        if ((rc = fetch_partials(E, used, 1))) return rc;
        for (int i = 0; i < used; i++) b += h_partial[i];
    }
    *barrier_out = b;
    return CHIP_OK;
}
int KktCones::margins(Engine &E, const double *z_dev, double *alpha_out, double *beta_out) {
    int rc = ensure_partials(E);
    if (rc) return rc;
    double *pmin = d_partial, *psum = d_partial + partial_cap;
    int used = dev::cone_margins(E.stream, nn_rows, nn_count, soc, z_dev, pmin, psum, 1024);
    used += dev::psd_margins(E.stream, psd, z_dev, pmin + used, psum + used);
    double a = 1.7976931348623157e308, b = 0.0; // T::max_value(), compositecone.rs:198
    if (used) {
        if ((rc = fetch_partials(E, used, 2))) return rc;
        for (int i = 0; i < used; i++) {
            a = std::min(a, h_partial[i]);
            b += h_partial[partial_cap + i];
        }
    }
    *alpha_out = a;
    *beta_out = b;
    return CHIP_OK;
}

int KktCones::set_genpow_alpha(Engine &E, const KktLayout &K, int64_t cone_index, const double *alpha) {
    for (size_t g = 0; g < gpw_cone_index.size(); g++) {
        if (gpw_cone_index[g] != cone_index) continue;
        const int d1 = gpw_dim1[g];
        double sum = 0.0, sq = 0.0;
        for (int k = 0; k < d1; k++) {
            if (!(alpha[k] > 0.0)) return fail(CHIP_ERR_ARG, "GenPowerConeT: powers must be positive"); // genpowcone.rs:27
            sum += alpha[k];
            sq += alpha[k] * alpha[k];
        }
        if (std::fabs(1.0 - sum) >= 2.220446049250313e-16 * d1 * 0.5 + 1e-15)
            return fail(CHIP_ERR_ARG, "GenPowerConeT: powers must sum to one"); // genpowcone.rs:28
        CHIP_HIP(hipSetDevice(E.device));
        double *st = gpw.state + gpw_state_off[g];
        const int d2 = (int)K.cones[(size_t)cone_index].dim2;
        const double psi = 1.0 / sq;
        CHIP_HIP(hipMemcpyAsync(st, alpha, (size_t)d1 * sizeof(double), hipMemcpyHostToDevice, E.stream));
        CHIP_HIP(hipMemcpyAsync(st + 6 * d1 + 4 * d2 + 2, &psi, sizeof(double), hipMemcpyHostToDevice, E.stream));
        CHIP_HIP(hipStreamSynchronize(E.stream));
        return CHIP_OK;
    }
    return fail(CHIP_ERR_ARG, "cone_index is not a GenPowerConeT");
}

// the batched solver's PSD members (batch_psd.hpp): the per-cone reductions of the handle's PsdView, enqueued on its
// stream into the caller's device arrays and left there -- the batch folds them per member without a host round trip
int kkt_psd_cones(const ::chip_kkt *h) { return h->cones.psd.ncones; }
int kkt_psd_margins_dev(::chip_kkt *h, const double *z_dev, double *pmin_dev, double *psum_dev) {
    Engine &E = h->E;
    NEED_DEVICE(E);
    (void)dev::psd_margins(E.stream, h->cones.psd, z_dev, pmin_dev, psum_dev);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int kkt_psd_step_length_dev(::chip_kkt *h, const double *dz_dev, const double *ds_dev, double alpha_max,
                            double *alpha_dev) {
    Engine &E = h->E;
    NEED_DEVICE(E);
    (void)dev::psd_step_length(E.stream, h->cones.psd, dz_dev, ds_dev, alpha_max, alpha_dev);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}

} // namespace chip

using namespace chip;

#define NEED_SYMMETRIC(h) \
    if (!(h)->cones.symmetric()) return fail(CHIP_ERR_UNSUPPORTED, "margins / scaled_unit_shift: symmetric, device-held cones only")
#define NEED_STEP_OPS(h) \
    if ((h)->cones.has_hostHs) return fail(CHIP_ERR_UNSUPPORTED, "cone step operations: a cone kind that is not held on the device")

extern "C" {

int32_t chip_kkt_mul_Hs_dev(chip_kkt *h, double *y_dev, const double *x_dev) {
    if (!h) return CHIP_ERR_ARG;
    if (h->cones.has_hostHs) return fail(CHIP_ERR_UNSUPPORTED, "mul_Hs: a cone kind that is not held on the device");
    Engine &E = h->E;
    NEED_DEVICE(E);
    CHIP_HIP(hipSetDevice(E.device));
    h->cones.mul_Hs(E, y_dev, x_dev);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_kkt_scaled_unit_shift_dev(chip_kkt *h, double *z_dev, double alpha, int32_t primal_cone) {
    if (!h || !z_dev) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    NEED_SYMMETRIC(h);
    CHIP_HIP(hipSetDevice(E.device));
    h->cones.unit_shift(E, z_dev, alpha, primal_cone);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_kkt_affine_ds_dev(chip_kkt *h, double *ds_dev, const double *s_dev) {
    if (!h || !ds_dev) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    NEED_STEP_OPS(h);
    if ((h->cones.ns3.ncones || h->cones.gpw.ncones) && !s_dev) return CHIP_ERR_ARG;
    CHIP_HIP(hipSetDevice(E.device));
    h->cones.affine_ds(E, ds_dev, s_dev);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_kkt_combined_ds_shift_dev(chip_kkt *h, double *shift_dev, double *step_z_dev, double *step_s_dev,
                                       double sigma_mu) {
    if (!h || !shift_dev || !step_z_dev || !step_s_dev) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    NEED_STEP_OPS(h);
    CHIP_HIP(hipSetDevice(E.device));
    h->cones.combined_ds_shift(E, shift_dev, step_z_dev, step_s_dev, sigma_mu);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_kkt_ds_from_dz_offset_dev(chip_kkt *h, double *out_dev, const double *ds_dev, const double *z_dev) {
    if (!h || !out_dev || !ds_dev || !z_dev) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    NEED_STEP_OPS(h);
    CHIP_HIP(hipSetDevice(E.device));
    h->cones.ds_from_dz_offset(E, out_dev, ds_dev, z_dev);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_kkt_step_length_dev(chip_kkt *h, const double *dz_dev, const double *ds_dev, const double *z_dev,
                                 const double *s_dev, double alpha_max, double *alpha_out) {
    if (!h || !alpha_out) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    NEED_STEP_OPS(h);
    CHIP_HIP(hipSetDevice(E.device));
    return h->cones.step_length(E, dz_dev, ds_dev, z_dev, s_dev, alpha_max, alpha_out);
}
int32_t chip_kkt_set_genpow_alpha(chip_kkt *h, int64_t cone_index, const double *alpha) {
    if (!h || !alpha) return CHIP_ERR_ARG;
    NEED_DEVICE(h->E);
    return h->cones.set_genpow_alpha(h->E, h->K, cone_index, alpha);
}
int32_t chip_kkt_compute_barrier_dev(chip_kkt *h, const double *z_dev, const double *s_dev, const double *dz_dev,
                                     const double *ds_dev, double alpha, double *barrier_out) {
    if (!h || !barrier_out || !z_dev || !s_dev || !dz_dev || !ds_dev) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    NEED_STEP_OPS(h);
    CHIP_HIP(hipSetDevice(E.device));
    return h->cones.barrier(E, z_dev, s_dev, dz_dev, ds_dev, alpha, barrier_out);
}
int32_t chip_kkt_unit_initialization_dev(chip_kkt *h, double *z_dev, double *s_dev) {
    if (!h || !z_dev || !s_dev) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    NEED_STEP_OPS(h);
    CHIP_HIP(hipSetDevice(E.device));
    h->cones.unit_initialization(E, z_dev, s_dev, (int)h->K.m);
    CHIP_HIP(hipGetLastError());
    return CHIP_OK;
}
int32_t chip_kkt_margins_dev(chip_kkt *h, const double *z_dev, double *alpha_out, double *beta_out) {
    if (!h || !alpha_out || !beta_out) return CHIP_ERR_ARG;
    Engine &E = h->E;
    NEED_DEVICE(E);
    NEED_SYMMETRIC(h);
    CHIP_HIP(hipSetDevice(E.device));
    return h->cones.margins(E, z_dev, alpha_out, beta_out);
}

} // extern "C"
