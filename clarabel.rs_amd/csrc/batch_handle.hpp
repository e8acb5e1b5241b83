// batch_handle.hpp -- the handle of the batched solver (struct chip_batch) and the host partition it is built from,
// for the translation units that work on it: batch.cpp (plan, create / destroy, the IPM loop, getters, data updates),
// batch_deriv.cpp (chip_bgrad_*, chip_bjvp_*, chip_bjac_*, chip_bvjp_*) and batch_debug.cpp (the test hooks).
// Internal: nothing here is part of the C ABI, and no other translation unit includes it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "batch.hpp"
#include "batch_psd.hpp"
#include "engine.hpp"
#include "host_util.hpp"
#include "ipm_info.hpp"
#include "problem_data.hpp"
#include "problem_update.hpp"

using namespace chip;

// what is shared between translation units without being part of the library's symbol table
#define CHIP_INTERNAL __attribute__((visibility("hidden")))

// the fixed partition of a batch on the host (dev::BatchPlan, batch.hpp, is its device copy), with what the cones give
// per member.  parts_ok: the parts themselves were accepted, so xoff / zoff / xmem / zmem are filled even when a cone
// was refused after them
struct CHIP_INTERNAL HostPlan {
    int nprob = 0, n = 0, m = 0, ncx = 0, ncz = 0;
    std::vector<int> xoff, zoff, xmem, zmem, ch_beg, ch_end, cx_first, cz_first, it_beg, it_end, it_type, it_first, rtype;
    std::vector<int64_t> degree;
    std::vector<char> has_soc;
    std::vector<ConeSpec> cones;
    bool parts_ok = false;
    const char *fn = "chip_batch_create"; // the entry point the messages name
    // the PSDTriangle cones of side > 0 (dev::BatchPsdPlan, batch_psd.hpp, is the device copy), in row order and so
    // sorted by member: owner, first row, side, index among all PSD cones of the stack (the L2 handle's PsdView
    // order, which counts the cones of side 0 too), the member's first cone, and the rows of the diagonal entries
    std::vector<int> psd_mem, psd_start, psd_dim, psd_view, psd_first, psd_diag;
    std::vector<char> has_psd;
    int psd_total = 0; // all PSD cones of the stack, side 0 included
};

// the two entry points of create and the cones each takes (bit t: cone tag t)
struct CHIP_INTERNAL BatchEntry {
    const char *fn;    // as the messages name it
    unsigned accepted; // mask of the cone tags
    const char *only;  // the refusal of any other cone
};
constexpr unsigned BATCH_CONES_BASIC =
    (1u << CHIP_CONE_ZERO) | (1u << CHIP_CONE_NONNEGATIVE) | (1u << CHIP_CONE_SECONDORDER);
constexpr unsigned BATCH_CONES_SYMMETRIC = BATCH_CONES_BASIC | (1u << CHIP_CONE_PSDTRIANGLE);
extern CHIP_INTERNAL const BatchEntry BATCH_ENTRY_BASIC, BATCH_ENTRY_SYMMETRIC;

// the partition itself and its device copies (batch.cpp); batch_cones_supported: only the cones the entry takes.
// host_plan_build describes every cone it is given (the caller has refused the others) and names hp.fn in its messages
CHIP_INTERNAL int batch_cones_supported(const BatchEntry &entry, int64_t ncones, const int32_t *cone_tags);
CHIP_INTERNAL int host_plan_build(HostPlan &hp, int64_t nprob, const int64_t *n_part, const int64_t *m_part, int64_t n,
                                  int64_t m, int64_t ncones, const int32_t *cone_tags, const int64_t *cone_dims,
                                  const int64_t *cone_dims2);
CHIP_INTERNAL int host_plan_upload(DevPool &mem, const HostPlan &hp, dev::BatchPlan *pl);
CHIP_INTERNAL int host_plan_upload_psd(DevPool &mem, const HostPlan &hp, const dev::BatchPlan &pl,
                                       dev::BatchPsdPlan *pp);

// one derivative pass of the handle (the gradients, the tangents, the blocks of tangents or of cotangents): what the
// shared steps of the passes work on.  Each pass owns its valid flags and its results, so none disturbs what another's
// get_dev handed out.  The buffers are allocated by the pass's first call
struct CHIP_INTERNAL DerivPass {
    const char *name;             // the call that runs the pass, as the messages name it
    bool done = false;            // the results hold a pass since the last solve
    long syncs = 0, launches = 0; // of the last call
    long refactors = 0;           // of the handle's life
    std::vector<int32_t> hvalid;  // the member has a derivative: it ended Solved and owns no SecondOrder or PSD cone
    int *valid = nullptr;         // ... on the device
    int nin = 0, nout = 0;
    size_t in_len[4] = {}, out_len[4] = {};
    double *in[4] = {};  // the staging of the host form's inputs
    double *out[4] = {}; // the results
};

struct chip_batch {
    int nprob = 0;
    chip_solver_settings st{};
    DevPool mem;
    std::vector<int> xoff, zoff;
    dev::BatchPlan plan{};
    // the PSDTriangle cones of a handle of chip_bsym_create (ncones == 0: none, and no pass of batch_psd.hpp runs);
    // psd_res: four arrays of one double per PSD cone of the stack for the per-cone results the L2 handle leaves
    dev::BatchPsdPlan psd{};
    double *psd_res = nullptr;
    int psd_total = 0;
    double *pres(int j) { return psd_res + (size_t)j * psd_total; }
    ProblemData pd; // the whole stack
    double *negq = nullptr;
    // for the data updates (chip_bdata_*): the unscaled q and b (the members' norms are taken from them, as create
    // takes them from the user's data) and the members' cost scales on the device
    double *uq = nullptr, *ub = nullptr, *dc = nullptr;
    std::vector<double> c, normq, normb;
    std::vector<int64_t> degree;
    std::vector<int> lp_init; // the member's P has no stored entry: the LP initial point (kktsystem.rs:197-215)
    bool anyP = false, anyLP = false;
    chip_kkt *kkt = nullptr;
    chip_kktsystem *sys = nullptr; // its sparse operators only (kktsystem_spmv)
    hipStream_t stream = nullptr;
    // iterates: the current and previous one (swapped by the step), the held last finite iterate of members that ended
    // NumericalError, the direction and right-hand side
    double *vx = nullptr, *vs = nullptr, *vz = nullptr, *px = nullptr, *ps = nullptr, *pz = nullptr;
    double *hx = nullptr, *hs = nullptr, *hz = nullptr;
    double *lx = nullptr, *ls = nullptr, *lz = nullptr, *dx = nullptr, *ds = nullptr, *dz = nullptr;
    double *x1 = nullptr, *z1 = nullptr, *x2 = nullptr, *z2 = nullptr, *workx = nullptr, *workx2 = nullptr,
           *wn = nullptr, *wn2 = nullptr, *wn3 = nullptr, *workz = nullptr, *conicw = nullptr;
    double *rx = nullptr, *rz = nullptr, *rx_inf = nullptr, *rz_inf = nullptr, *Pxv = nullptr;
    double *xo = nullptr, *so = nullptr, *zo = nullptr;
    double *dsc = nullptr, *dred = nullptr, *seg_scr = nullptr, *cone_scr = nullptr;
    int *dmask = nullptr;
    std::vector<double> hsc, hred;
    std::vector<int> hmask;
    // per member on the host
    std::vector<double> tau, kappa, ptau, pkappa, htau, hkappa, mu, sigma, alpha, dtau, qx2, bz2, x2Px2;
    std::vector<IpmInfo> info, pinfo, hinfo; // (out5 of a member: the dots of its last residual pass)
    std::vector<char> active, held, held_done; // held: 1 = the current iterate, 2 = the previous one
    std::vector<double> obj_val, obj_val_dual;
    double setup_time = 0, equilibration_time = 0, iteration_time = 0, solve_time = 0;
    double t_solve0 = 0;
    bool solved_once = false;
    // test hooks and counters
    int64_t nan_member = -1;
    int nan_iter = -1;
    long syncs = 0, launches = 0, loop_iters = 0;
    // work buffers of the data updates, allocated by the first one; the staging of the host forms grows on demand
    int *upos = nullptr, *uflag = nullptr;
    unsigned long long *unpart = nullptr, *ubpart = nullptr;
    double *unout = nullptr, *ubout = nullptr;
    UpdateStage stage;
    int64_t *clean = nullptr;
    size_t clean_cap = 0;
    std::vector<double> unorm;
    long upd_syncs = 0, upd_launches = 0; // of the last update or re-equilibration call
    // a re-equilibration (chip_reequilibrate_bdata) runs create's Ruiz loop again: the cones it rectifies, the column
    // sums of a Ruiz step, and what its one synchronisation reads back ([normq nprob][normb nprob][-, -, max |P_ii|]);
    // the two buffers are allocated by the first one
    std::vector<ConeSpec> cones;
    double *eq_colsum = nullptr, *req_out = nullptr;
    std::vector<double> req_host;
    // the derivatives (chip_bgrad_*, chip_bjvp_*).  solve_current: the last solve ran on the data
    // the handle holds now; kkt_final: K is factored at the final iterates of that solve (by a backward or an apply),
    // so an apply needs no scaling update and no refactor
    std::vector<char> has_soc; // the member owns a SecondOrder cone: no derivative
    std::vector<char> has_psd; // ... a PSDTriangle cone: no derivative either; held aside when it terminates
    bool solve_current = false, kkt_final = false;
    DerivPass grad{"chip_bgrad_backward"}; // gx, gz, gs -> dq, db, dP, dA
    DerivPass tan{"chip_bjvp_apply"};      // dq, db, dP, dA -> dx, dz, ds
    // blocks of up to CHIP_BJAC_MAX_DIR tangents with one synchronisation (chip_bjac_*).  in / out hold
    // the directions one after the other (in_len / out_len: those of the last block; the staging is allocated by the
    // first host form); jac_work holds, per direction, its own right-hand side, solution and A product: a solve that
    // is pending borrows its right-hand side until the collect
    DerivPass jac{"chip_bjac_apply"};
    double *jac_work = nullptr;
    long jac_calls = 0, jac_repeats = 0; // blocks run / blocks whose outputs were issued again after the collect
    // blocks of up to CHIP_BVJP_MAX_DIR cotangents with one synchronisation (chip_bvjp_*).  out holds
    // the cotangents one after the other; a piece's buffer is allocated by the first block that wants it (vjp_want:
    // the pieces the last block computed); vjp_work holds, per cotangent, D gx and gs / e (the operands of the A'
    // product), its own right-hand side and its solution
    DerivPass vjp{"chip_bvjp_apply"};
    double *vjp_work = nullptr;
    int vjp_want = 0;
    long vjp_calls = 0, vjp_repeats = 0;

    ~chip_batch() {
        if (stream) (void)hipStreamSynchronize(stream);
        (void)hipFree(clean);
        chip_kktsystem_destroy(sys);
        chip_kkt_destroy(kkt);
    }
    double *sc(int slot) { return dsc + (size_t)slot * nprob; }
    double &hs_(int slot, int k) { return hsc[(size_t)slot * nprob + k]; }
    int *mk(int slot) { return dmask + (size_t)slot * nprob; }
    int &hm(int slot, int k) { return hmask[(size_t)slot * nprob + k]; }
    // the per-member scalars and masks travel in a ring of device (and host staging) slots: a kernel enqueued before
    // the next upload keeps reading its own slot, and the loop synchronises far more often than the ring wraps
    static constexpr int RING = 32;
    double *dsc_ring = nullptr;
    int *dmask_ring = nullptr;
    std::vector<double> hsc_ring;
    std::vector<int> hmask_ring;
    int ring_s = 0, ring_m = 0;
    int push_scalars() {
        const size_t len = hsc.size();
        ring_s = (ring_s + 1) % RING;
        double *src = hsc_ring.data() + (size_t)ring_s * len;
        std::memcpy(src, hsc.data(), len * 8);
        dsc = dsc_ring + (size_t)ring_s * len;
        launches++;
        CHIP_HIP(hipMemcpyAsync(dsc, src, len * 8, hipMemcpyHostToDevice, stream));
        return CHIP_OK;
    }
    int push_masks() {
        const size_t len = hmask.size();
        ring_m = (ring_m + 1) % RING;
        int *src = hmask_ring.data() + (size_t)ring_m * len;
        std::memcpy(src, hmask.data(), len * sizeof(int));
        dmask = dmask_ring + (size_t)ring_m * len;
        launches++;
        CHIP_HIP(hipMemcpyAsync(dmask, src, len * sizeof(int), hipMemcpyHostToDevice, stream));
        return CHIP_OK;
    }
    // one device-to-host copy of `count` doubles of the reduction output and one synchronisation
    int read_red(size_t count) {
        CHIP_HIP(hipGetLastError());
        CHIP_HIP(hipMemcpyAsync(hred.data(), dred, count * 8, hipMemcpyDeviceToHost, stream));
        CHIP_HIP(hipStreamSynchronize(stream));
        launches++;
        syncs++;
        return CHIP_OK;
    }
    double red(int slot, int k) const { return hred[(size_t)slot * nprob + k]; }
    void lin(double *w, const double *x, const double *y, const double *sa, const double *sb, double ca, double cb,
             int space, const int *mask, int mode) {
        dev::blin(stream, plan, dev::BLin{w, x, y, sa, sb, ca, cb, space, mask, mode});
        launches++;
    }
    void copy_members(double *wx, double *ws, double *wz, const double *x, const double *s, const double *z,
                      const int *mask) { // masked copy: members with mask[k] != 0 take (x, s, z)
        lin(wx, x, nullptr, nullptr, nullptr, 1.0, 0.0, 0, mask, dev::MASK_KEEP);
        lin(ws, s, nullptr, nullptr, nullptr, 1.0, 0.0, 1, mask, dev::MASK_KEEP);
        lin(wz, z, nullptr, nullptr, nullptr, 1.0, 0.0, 1, mask, dev::MASK_KEEP);
    }
    int spmv(int which, double *y, const double *aux, double alpha_, const double *x) {
        launches++;
        return kktsystem_spmv(sys, which, y, aux, alpha_, x);
    }
    int default_start();
    int residual_pass();
    void member_info(int k);
    int solve_direction(const double *conic, const std::vector<double> &rtau, const std::vector<double> &rkap,
                        std::vector<double> &lkappa, bool *global_ok, int iter);
    int step_length(const std::vector<double> &lkappa, bool combined);
    int constant_rhs(bool *global_ok, int iter);
    int hold_and_reset();
    int post_process();
    int end_member(int k, int status, int iterations, bool from_prev);
    int update_work();
    static constexpr const char *UPD_PREFIX = "chip_bdata_update_";
    static int update_args(chip_batch *h, int which, const void *idx, const double *vals, int64_t k);
    int stage_upload(const uint64_t *idx, const double *vals, size_t k) {
        return stage.upload(stream, idx, vals, k, &upd_launches, &upd_syncs);
    }
    int update(int which, const int64_t *idx_dev, const double *vals_dev, int k);
    int reequilibrate_gate(const char *fn);
    int stage_upload4(const double *const src[4], const size_t len[4], const double *at[4]) {
        return stage.upload4(stream, src, len, at, &upd_launches, &upd_syncs);
    }
    int reequilibrate(const double *P_dev, const double *q_dev, const double *A_dev, const double *b_dev);
    int backward_work();
    int backward(const double *gx_dev, const double *gz_dev, const double *gs_dev);
    int jvp_work();
    int jvp_apply(const double *dq_dev, const double *db_dev, const double *dP_dev, const double *dA_dev);
    int jac_alloc();
    int jac_block(int ndir, int piece, long long first, const double *dq_dev, const double *db_dev, const double *dP_dev,
                  const double *dA_dev);
    int vjp_alloc();
    int vjp_block(int ndir, int want, int piece, long long first, const double *gx_dev, const double *gz_dev,
                  const double *gs_dev);
};
