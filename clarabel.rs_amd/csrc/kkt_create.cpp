// kkt_create.cpp -- chip_kkt_create as a sequence of stages: assembly and analysis, the host's plan for the fused solve
// kernels, the host-only exit, then the device side (values, index maps, cone tables, work vectors, fused binding)
#include <memory>

#include "host_util.hpp"
#include "kkt_handle.hpp"

using namespace chip;

namespace {

// workgroups the device keeps resident for the fused solve kernel (4 x 256 threads per CU): a forest with fewer
// bundles than that is cut finer by the analysis (grouped fold).  Host-only handles: an MI355X's 256 CUs.
int target_workgroups(const chip_settings &st) {
    if (switches().has_target_wg) return switches().target_wg; // (tests; 0 = never refine)
    if (st.device == CHIP_DEVICE_HOST_ONLY) return 1024;
    int dev = st.device, cus = 0;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return 1024;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        return 1024;
    }
    return 4 * cus;
}

// the permutation inside every bundle as maximal ascending runs that stay inside one of the ranges
// [0, n) (rhsx), [n, n + m) (rhsz), [n + m, N) (zeros): run r = {first local index, first original index, length};
// bundle b owns runs [rp[b], rp[b + 1])
void bundle_perm_runs(const Symbolic &S, i64 n, i64 m, std::vector<int> &rp, std::vector<int> &runs) {
    rp.assign(1, 0);
    runs.clear();
    const std::vector<i32> &pm = S.perm;
    const i64 n1 = n, n2 = n + m;
    auto range_of = [&](i64 o) { return o < n1 ? 0 : (o < n2 ? 1 : 2); };
    const int nb = S.bundle_ptr.empty() ? 0 : (int)S.bundle_ptr.size() - 1;
    for (int b = 0; b < nb; b++) {
        const int s0 = S.bundle_ptr[(size_t)b], s1 = S.bundle_ptr[(size_t)b + 1];
        int t = s0;
        while (t < s1) {
            int e = t + 1;
            while (e < s1 && pm[(size_t)e] == pm[(size_t)e - 1] + 1 && range_of(pm[(size_t)e]) == range_of(pm[(size_t)t])) e++;
            runs.push_back(t - s0);
            runs.push_back(pm[(size_t)t]);
            runs.push_back(e - t);
            t = e;
        }
        rp.push_back((int)(runs.size() / 3));
    }
}
// One dev::IrsDesc per bundle for k_bundle_irs: what its prologue would chase through bundle_ptr, blvl_ptr -> blvl ->
// Lp, Up, run_ptr -> runs and the pattern offsets (pat_off: 2 per bundle, or nullptr: every bundle reads its own copy of
// the index arrays, offsets 0).  Empty when some bundle does not fit the record.
std::vector<int> irs_descriptors(const Symbolic &S, const std::vector<int> &rp, const std::vector<int> &runs,
                                 const std::vector<i32> *pat_off) {
    static_assert(dev::IRS_REP_R == 8 && dev::IRS_REP_MAXND == 4 && dev::IRS_NODE_BITS == 12, "symbolic.cpp: REP_R, REP_MAXND, NODE_BITS");
    const int nb = S.bundle_ptr.empty() ? 0 : (int)S.bundle_ptr.size() - 1;
    std::vector<int> out;
    if (nb <= 0 || (int)rp.size() != nb + 1) return out;
    for (int b = 0; b < nb; b++)
        if (!dev::irs_desc_fits(S.blvl_ptr[(size_t)b + 1] - S.blvl_ptr[(size_t)b] - 1, rp[(size_t)b + 1] - rp[(size_t)b])) return out;
    out.assign((size_t)nb * dev::IRS_DESC_INTS, 0);
    for (int b = 0; b < nb; b++) {
        dev::IrsDesc d{};
        const i32 *lv = S.blvl.data() + S.blvl_ptr[(size_t)b];
        d.s0 = S.bundle_ptr[(size_t)b];
        d.nloc = S.bundle_ptr[(size_t)b + 1] - d.s0;
        d.nleaf = lv[1] - d.s0;
        d.nl = S.blvl_ptr[(size_t)b + 1] - S.blvl_ptr[(size_t)b] - 1;
        d.dl = pat_off ? (*pat_off)[2 * (size_t)b] : 0;
        d.du = pat_off ? (*pat_off)[2 * (size_t)b + 1] : 0;
        d.fb = S.Up[(size_t)(d.s0 + d.nleaf)];
        d.fe = S.Up[(size_t)(d.s0 + d.nloc)];
        d.nruns = rp[(size_t)b + 1] - rp[(size_t)b];
        for (int l = 0; l <= d.nl; l++) d.lev_e[l] = S.Lp[(size_t)lv[l]];
        std::copy_n(&runs[3 * (size_t)rp[(size_t)b]], 3 * (size_t)d.nruns, d.runs);
        std::memcpy(&out[(size_t)b * dev::IRS_DESC_INTS], &d, sizeof d);
    }
    return out;
}
// the classes' replica slots (host.hpp: PatternShare::Rep) per bundle, the words that travel behind the records
// (kernels.hpp: IRS_REP_INTS); all zero when no class has any
std::vector<int> irs_replica_words(const PatternShare &pat, int nb) {
    std::vector<int> out((size_t)nb * dev::IRS_REP_INTS, 0);
    if (pat.rep.empty()) return out;
    for (int b = 0; b < nb; b++) {
        const PatternShare::Rep &r = pat.rep[(size_t)pat.cls[(size_t)b]];
        if (!r.nd) continue;
        int *w = &out[(size_t)b * dev::IRS_REP_INTS];
        w[0] = r.nd | dev::IRS_REP_R << 8, w[1] = r.first, w[2] = r.fold;
    }
    return out;
}

// what the stages after the analysis hand on: the host's plan for k_bundle_irs
struct FusedPlan {
    PatternShare pat;
    bool pat_cand = false;   // an arrow system whose every bundle is within the kernel's limits
    bool pat_shared = false; // ... and whose bundles read one shared copy of their index pattern
    std::vector<int> run_ptr, runs;
};

// stage 1: cone specs, K, the cliques of the dense cone blocks, the analysis
int assemble_and_analyse(chip_kkt *h, i64 n, i64 m, const uint64_t *Pcolptr, const uint64_t *Prowval, const double *Pnzval,
                         const uint64_t *Acolptr, const uint64_t *Arowval, const double *Anzval, i64 ncones,
                         const int32_t *cone_tags, const int64_t *cone_dims, const int64_t *cone_dims2,
                         const uint64_t *perm_or_null, const chip_settings &st, Symbolic &S, PhaseClock &clk) {
    KktLayout &K = h->K;
    i64 mm = 0;
    int rc = build_cone_specs(ncones, cone_tags, cone_dims, cone_dims2, K.cones, mm, K.p, K.nHs);
    if (rc) return CHIP_ERR_ARG;
    if (mm != m) return fail(CHIP_ERR_DIM, "cone dimensions do not add up to m");
    rc = assemble_kkt_triu(n, m, as_i64(Pcolptr), as_i64(Prowval), Pnzval, as_i64(Acolptr), as_i64(Arowval), Anzval, K);
    if (rc) return rc;
    clk("KKT assembly");
    std::vector<i64> perm0;
    if (perm_or_null) perm0.assign(as_i64(perm_or_null), as_i64(perm_or_null) + K.N);
    // dense cone blocks (the Hs block of a cone that is not diagonal: its rows are a clique of K) enter the ordering as
    // one weighted node each -- worth it from a few dozen rows per block (PSD cones; not the 3 x 3 / 4 x 4 blocks)
    std::vector<i32> clique_of;
    i32 g = 0;
    for (const ConeSpec &c : K.cones)
        if (!c.hs_diag && c.numel >= 16) {
            if (clique_of.empty()) clique_of.assign((size_t)K.N, -1);
            for (i64 r = 0; r < c.numel; r++) clique_of[(size_t)(n + c.start + r)] = g;
            g++;
        }
    rc = analyse(K.N, K.colptr.data(), K.rowval.data(), K.dsigns.data(), perm0, st.amd_dense_scale, S, target_workgroups(st),
                 clique_of.empty() ? nullptr : &clique_of);
    if (rc) return rc;
    clk("analysis (total)");
    return CHIP_OK;
}

// every bundle within the limits of k_bundle_irs (dev::irs_bundle_ok)?  runs_of(b): the runs bundle b brings
template <typename Runs> bool irs_bundles_ok(const Symbolic &S, Runs runs_of) {
    const i32 nbun = S.bundle_ptr.empty() ? 0 : (i32)S.bundle_ptr.size() - 1;
    bool ok = true;
    for (i32 b = 0; b < nbun && ok; b++) {
        const i32 s0 = S.bundle_ptr[(size_t)b], nloc = S.bundle_ptr[(size_t)b + 1] - s0;
        const i32 nleaf = S.blvl[(size_t)S.blvl_ptr[(size_t)b] + 1] - s0;
        ok = dev::irs_bundle_ok(nloc, nleaf, S.blvl_ptr[(size_t)b + 1] - S.blvl_ptr[(size_t)b] - 1, runs_of(b));
    }
    return ok;
}

// stage 2 (host only): pattern classes of the bundles and the kernel's per-bundle records, only for systems whose
// solves k_bundle_irs can take (an arrow system, every bundle within that kernel's limits: the host's part of the ir_sf
// conditions of fused_bind); host analysis, so the figures are there on a host-only handle too.  Every other system (a
// grouped fold, a level-scheduled top) skips all of it.
void fused_plan(chip_kkt *h, const Symbolic &S, FusedPlan &fp, PhaseClock &clk) {
    const bool nonempty = !S.bundle_ptr.empty() && S.bundle_ptr.size() > 1;
    fp.pat_cand = !S.Li16.empty() && S.gf_ng == 0 && S.nfold >= 1 && nonempty && irs_bundles_ok(S, [](i32) { return 1; });
    if (fp.pat_cand) {
        // (replica ids only where the records can say where they are: a shared pattern, no CHIP_IRS_FLAGS bit 16)
        const bool no_rep = switches().no_shared_pattern || (switches().irs_flags >= 0 && (switches().irs_flags & dev::IRS_F_NOREP));
        bundle_pattern_classes(S, fp.pat, !no_rep);
        h->E.note_patterns(fp.pat);
        clk("pattern classes");
    }
    // (what decides whether the kernel takes the solves at all is in fused_bind, on the device)
    fp.pat_shared = !fp.pat.off.empty() && !fp.pat.mismatches && !switches().no_shared_pattern;
    if (!fp.pat_cand) return;
    bundle_perm_runs(S, h->K.n, h->K.m, fp.run_ptr, fp.runs);
    bool fit = true;
    for (size_t b = 0; b + 1 < fp.run_ptr.size() && fit; b++) fit = fp.run_ptr[b + 1] - fp.run_ptr[b] <= dev::IRS_DESC_RUNS;
    if (fit) h->h_irs_desc = irs_descriptors(S, fp.run_ptr, fp.runs, fp.pat_shared ? &fp.pat.off : nullptr);
    if (h->h_irs_desc.empty() || !fp.pat_shared) fp.pat.strip_replicas(); // (a bundle of more than 19 levels: the chained prologue)
    if (!h->h_irs_desc.empty()) h->h_irs_rep = irs_replica_words(fp.pat, (int)(h->h_irs_desc.size() / dev::IRS_DESC_INTS));
    h->irs_rep_bundles = fp.pat.rep_bundles, h->irs_rep_nodes = fp.pat.rep_nodes;
    clk("bundle descriptors");
}

// stage 3: a handle without a device -- the analysis alone (and, in test builds, the arrays the tests walk)
void finish_host_only(chip_kkt *h, Symbolic &S, const chip_settings &st, const FusedPlan &fp) {
#ifdef CHIP_TESTING
    if (fp.pat_cand) {
        h->t_bundle_ptr = S.bundle_ptr, h->t_blvl_ptr = S.blvl_ptr, h->t_blvl = S.blvl;
        h->t_Lp = S.Lp, h->t_Up = S.Up, h->t_run_ptr = fp.run_ptr, h->t_runs = fp.runs;
        if (fp.pat_shared) {
            h->t_pat_off = fp.pat.off;
            h->t_pat_Li16.assign(fp.pat.Li16.begin(), fp.pat.Li16.end()), h->t_pat_Ucol16.assign(fp.pat.Ucol16.begin(), fp.pat.Ucol16.end());
            h->t_pat_Urow16.assign(fp.pat.Urow16.begin(), fp.pat.Urow16.end());
            if (S.Li16.size() + S.Ucol16.size() <= ((size_t)1 << 21)) // (the bundles' own slices, for small problems)
                h->t_Li16.assign(S.Li16.begin(), S.Li16.end()), h->t_Ucol16.assign(S.Ucol16.begin(), S.Ucol16.end());
        }
    }
    // what the replica rule (host.hpp: PatternShare::Rep) says about this system's bundles whether or not k_bundle_irs can
    // take them (bundles under its 512 nodes: the rule's threshold of 64 entries lies there), for the tests of the rule
    if (!S.Li16.empty() && S.gf_ng == 0 && S.nfold >= 1 && S.bundle_ptr.size() > 1) {
        PatternShare plan;
        bundle_pattern_classes(S, plan, true);
        if (!plan.off.empty()) h->t_rep_plan = irs_replica_words(plan, (int)S.bundle_ptr.size() - 1);
    }
#else
    (void)fp;
#endif
    h->E.init_host_only(S, st);
#ifdef CHIP_TESTING
    h->t_fu_lvl_ptr = S.blvl_ptr;
    h->t_fu_rec = std::move(S.fu_rec), h->t_fu_ptr = std::move(S.fu_ptr);
    h->t_fr_rec = std::move(S.fr_rec), h->t_fr_desc = std::move(S.fr_desc);
    h->t_fr_ptr = std::move(S.fr_ptr), h->t_fr_rptr = std::move(S.fr_rptr);
    h->t_fr_bdesc = std::move(S.fr_bdesc);
    h->t_fc_usr.assign(S.fc_usr.begin(), S.fc_usr.end()), h->t_fc_col.assign(S.fc_col.begin(), S.fc_col.end()); // (bit patterns)
    h->t_fc_sgn.assign(S.fc_sgn.begin(), S.fc_sgn.end()), h->t_fc_rec.assign(S.fc_rec.begin(), S.fc_rec.end());
    h->t_fc_desc = std::move(S.fc_desc);
#endif
}

// stage 4: the engine and K's values, which the device keeps in T order (host.hpp: Symbolic::k2v)
int init_engine(chip_kkt *h, const Symbolic &S, const chip_settings &st, PhaseClock &clk) {
    const KktLayout &K = h->K;
    int rc = h->E.init(S, st);
    if (rc) return rc;
    clk("engine init (uploads)");
    if (K.nnz) {
        rawvec<double> vx((size_t)K.nnz);
        run_threads(K.nnz >= (i64)1 << 22 ? host_threads() : 1, [&](int t, int TT) {
            for (i64 u = K.nnz * t / TT; u < K.nnz * (t + 1) / TT; u++) vx[(size_t)u] = K.nzval[(size_t)S.v2k[(size_t)u]];
        });
        CHIP_HIP(hipMemcpy(h->E.Kx, vx.data(), (size_t)K.nnz * sizeof(double), hipMemcpyHostToDevice));
    }
    h->static_diag_max = diag_P_max(K);
    return CHIP_OK;
}

// stage 5: every LDLDataMap index the kernels use is translated ONCE into a position of the device's value store
// (by host threads when the map is long: config 5's mapHs has 1.6e8 entries)
template <typename V> int upload_map(Engine &E, int **dst, const V &v, size_t cnt, const bigvec &k2v) {
    rawvec<int> o(cnt);
    run_threads(cnt >= (size_t)1 << 22 ? host_threads() : 1, [&](int t, int TT) {
        for (size_t i = cnt * (size_t)t / (size_t)TT; i < cnt * (size_t)(t + 1) / (size_t)TT; i++) o[i] = k2v[(size_t)v[i]];
    });
    return E.upload(dst, o, cnt);
}
int upload_index_maps(chip_kkt *h, const bigvec &k2v, size_t nnzP, size_t nnzA) {
    const KktLayout &K = h->K;
    int rc;
    if ((rc = upload_map(h->E, &h->mapHs, K.mapHs, (size_t)K.nHs, k2v))) return rc;
    if ((rc = upload_map(h->E, &h->diag_full, K.diag_full, (size_t)K.N, k2v))) return rc;
    if ((rc = upload_map(h->E, &h->mapP, K.mapP, nnzP, k2v))) return rc;
    return upload_map(h->E, &h->mapA, K.mapA, nnzA, k2v);
}

// stage 7: the staging and work vectors
int alloc_vectors(chip_kkt *h, size_t nnzP, size_t nnzA) {
    Engine &E = h->E;
    const KktLayout &K = h->K;
    int rc;
    if ((rc = E.alloc(&h->d_s, (size_t)K.m))) return rc;
    if ((rc = E.alloc(&h->d_z, (size_t)K.m))) return rc;
    if ((rc = E.alloc(&h->d_rhs, (size_t)(K.n + K.m)))) return rc;
    if ((rc = E.alloc(&h->d_lhs, (size_t)(K.n + K.m)))) return rc;
    if ((rc = h->wk[0].alloc(E, (size_t)K.N))) return rc;
    h->tmp_len = std::max<size_t>({(size_t)K.N, (size_t)K.nHs, nnzP, nnzA, 1});
    if ((rc = E.alloc(&h->d_tmp, h->tmp_len))) return rc;
    CHIP_HIP(hipMemset(h->wk[0].bp, 0, (size_t)(K.N ? K.N : 1) * sizeof(double)));
    return CHIP_OK;
}

// stage 8 (device side of fused_plan): which of k_bundle_irs / k_bundle_irs_fixed / the mailbox mirror apply to this
// handle, and the uploads they read
int fused_bind(chip_kkt *h, const Symbolic &S, FusedPlan &fp) {
    Engine &E = h->E;
    if (!E.ir_fused) return CHIP_OK;
    int rc;
    // the permutation inside every bundle as runs (bundle_perm_runs); used when they are long on average
    if (fp.run_ptr.empty()) bundle_perm_runs(S, h->K.n, h->K.m, fp.run_ptr, fp.runs);
    const std::vector<int> &rp = fp.run_ptr;
    if (fp.runs.empty() || (i64)(fp.runs.size() / 3) * 64 > (i64)E.NF) return CHIP_OK;
    if ((rc = E.upload(&h->ir_run_ptr, rp, rp.size()))) return rc;
    if ((rc = E.upload(&h->ir_runs, fp.runs, fp.runs.size()))) return rc;
    // (arrow systems only: a forest without top rows whose bundles qualify did not occur in any test problem -- block-diagonal
    // problems become grouped folds --, so that path of the kernel stays unreachable rather than untested)
    const bool sf = E.gfold.ng == 0 && E.fold.k >= 1 && E.ir_tw == 256 && E.bundles.symv_split && E.bundles.nb == E.ir_grid &&
                    !switches().no_ir_sf && !switches().no_flat &&
                    irs_bundles_ok(S, [&rp](i32 b) { return rp[(size_t)b + 1] - rp[(size_t)b]; });
    h->ir_sf = sf && dev::bundle_irs_capacity_ok(E.bundles);
    h->irs_fixed_ok = h->ir_sf && E.fold.k == 1 && dev::bundle_irs_fixed_capacity_ok(E.bundles);
    // replica slots: only when every kernel that can take the launch is still co-resident with the larger LDS request
    if (fp.pat.rep_bundles && !(h->ir_sf && dev::bundle_irs_capacity_ok(E.bundles, true) &&
                                (!h->irs_fixed_ok || dev::bundle_irs_fixed_capacity_ok(E.bundles, true)))) {
        fp.pat.strip_replicas();
        std::fill(h->h_irs_rep.begin(), h->h_irs_rep.end(), 0);
        h->irs_rep_bundles = h->irs_rep_nodes = 0;
    }
    // (update and solves each end in a launch that can leave its verdict in the host's mirror of the mailbox)
    E.mb_mirror_on = h->ir_sf && E.fold.k == 1 && E.fast_prep_ok;
    if (h->ir_sf && !switches().no_shared_pattern && (rc = E.upload_patterns(fp.pat))) return rc;
    // (the records carry the offsets of the shared arrays: only beside them, or with offsets 0 without them)
    if (h->ir_sf && !h->h_irs_desc.empty() && (E.pat_off != nullptr) == fp.pat_shared) {
        std::vector<int> table = h->h_irs_desc; // (the records, then the replica words of every bundle)
        table.insert(table.end(), h->h_irs_rep.begin(), h->h_irs_rep.end());
        if ((rc = E.upload(&h->irs_desc, table, table.size()))) return rc;
    }
    h->irs_desc_shared = fp.pat_shared;
    return CHIP_OK;
}

} // namespace

extern "C" {

int32_t chip_kkt_create(chip_kkt **out, int64_t n, int64_t m, const uint64_t *Pcolptr,
                        const uint64_t *Prowval, const double *Pnzval, const uint64_t *Acolptr,
                        const uint64_t *Arowval, const double *Anzval, int64_t ncones,
                        const int32_t *cone_tags, const int64_t *cone_dims, const int64_t *cone_dims2,
                        const double *cone_alphas_or_null, const chip_settings *settings,
                        const uint64_t *perm_or_null) {
    if (!out || n < 0 || m < 0 || !Pcolptr || !Acolptr) return fail(CHIP_ERR_ARG, "chip_kkt_create: bad argument");
    *out = nullptr;
#ifdef CHIP_TESTING
    create_count(0)++;
#endif
    switches_reload(); // the CHIP_* diagnostic switches are read from the environment here, never in a launch loop
    chip_settings st;
    if (settings) st = *settings;
    else chip_settings_default(&st);
    std::unique_ptr<chip_kkt> h(new chip_kkt()); // (every error path below frees the handle and what its engine owns)
    PhaseClock clk;
    clk.tag = "kkt_create";
    Symbolic S;
    FusedPlan fp;
    int rc;
    if ((rc = assemble_and_analyse(h.get(), n, m, Pcolptr, Prowval, Pnzval, Acolptr, Arowval, Anzval, ncones, cone_tags,
                                   cone_dims, cone_dims2, perm_or_null, st, S, clk)))
        return rc;
    fused_plan(h.get(), S, fp, clk);
    if (st.device == CHIP_DEVICE_HOST_ONLY) {
        finish_host_only(h.get(), S, st, fp);
        *out = h.release();
        return CHIP_OK;
    }
    const size_t nnzP = (size_t)Pcolptr[n], nnzA = (size_t)Acolptr[n];
    if ((rc = init_engine(h.get(), S, st, clk))) return rc;
    if ((rc = upload_index_maps(h.get(), S.k2v, nnzP, nnzA))) return rc;
    if ((rc = h->cones.build(h->E, h->K, S.k2v, h->mapHs, cone_alphas_or_null, n))) return rc;
    if ((rc = alloc_vectors(h.get(), nnzP, nnzA))) return rc;
    if ((rc = fused_bind(h.get(), S, fp))) return rc;
    clk("maps, cone tables");
    *out = h.release();
    return CHIP_OK;
}

void chip_kkt_destroy(chip_kkt *h) { delete h; }

} // extern "C"
