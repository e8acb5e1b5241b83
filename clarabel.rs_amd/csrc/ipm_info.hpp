// ipm_info.hpp -- DefaultInfo (default/info.rs:12-389) as plain host C++: the scalars the interior-point loop keeps
// per problem, their update from the residual norms and dots, the termination checks and post_process' status /
// objective / scale decision.  No device code: chip_solver keeps one IpmInfo, chip_batch one per member, and both call
// the same functions.  Included by solver.cpp and batch.cpp only, whose build keeps fp contraction off (the
// reference's operation order).
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/clarabel_hip.h"

namespace chip {

struct IpmInfo {
    double cost_primal = 0, cost_dual = 0, res_primal = 0, res_dual = 0, res_primal_inf = 0, res_dual_inf = 0;
    double gap_abs = 0, gap_rel = 0, ktratio = 0;
    double prev_cost_primal = 0, prev_cost_dual = 0, prev_res_primal = 0, prev_res_dual = 0, prev_gap_abs = 0,
           prev_gap_rel = 0;
    double out5[5] = {0, 0, 0, 0, 0}; // r_tau, q'x, b'z, s'z, x'Px of the last residual update
    int iterations = 0;
    int status = CHIP_SOLVER_UNSOLVED;
};

// DefaultInfo::update (info.rs:113-178) from I.out5 and the SQUARED weighted norms of, in this order,
// (x, d), (z, e), (s, einv), (rx_inf, dinv), (Px, dinv), (rz_inf, einv), (rz, einv), (rx, dinv)
inline void ipm_info_update(IpmInfo &I, const double sq[8], double tau, double kappa, double c, double normq,
                            double normb) {
    double nrm[8];
    for (int k = 0; k < 8; k++) nrm[k] = std::sqrt(sq[k]);
    const double tinv = 1.0 / tau, cinv = 1.0 / c;
    const double dot_qx = I.out5[1], dot_bz = I.out5[2], dot_xPx = I.out5[4];
    const double xPx2 = dot_xPx * tinv * tinv / 2.0;
    I.cost_primal = (dot_qx * tinv + xPx2) * cinv;
    I.cost_dual = (-dot_bz * tinv - xPx2) * cinv;
    double normx = nrm[0], normz = nrm[1] * cinv, norms = nrm[2];
    I.res_primal_inf = (nrm[3] * cinv) / std::max(1.0, normz);
    I.res_dual_inf = std::max(nrm[4] / std::max(1.0, normx), nrm[5] / std::max(1.0, normx + norms));
    normx *= tinv;
    normz *= tinv;
    norms *= tinv;
    I.res_primal = nrm[6] * tinv / std::max(1.0, normb + normx + norms);
    I.res_dual = nrm[7] * tinv * cinv / std::max(1.0, normq + normx + normz);
    I.gap_abs = std::fabs(I.cost_primal - I.cost_dual);
    I.gap_rel = I.gap_abs / std::max(1.0, std::min(std::fabs(I.cost_primal), std::fabs(I.cost_dual)));
    I.ktratio = kappa * tinv;
}

// check_convergence_full / _almost (info.rs:277-389)
inline void ipm_check_convergence(IpmInfo &I, const chip_solver_settings &st, bool almost) {
    const double tga = almost ? st.reduced_tol_gap_abs : st.tol_gap_abs;
    const double tgr = almost ? st.reduced_tol_gap_rel : st.tol_gap_rel;
    const double tf = almost ? st.reduced_tol_feas : st.tol_feas;
    const double tia = almost ? st.reduced_tol_infeas_abs : st.tol_infeas_abs;
    const double tir = almost ? st.reduced_tol_infeas_rel : st.tol_infeas_rel;
    const double tkt = almost ? st.reduced_tol_ktratio : st.tol_ktratio;
    const double dot_qx = I.out5[1], dot_bz = I.out5[2];
    if (I.ktratio <= 1.0 && (I.gap_abs < tga || I.gap_rel < tgr) && I.res_primal < tf && I.res_dual < tf) {
        I.status = almost ? CHIP_SOLVER_ALMOST_SOLVED : CHIP_SOLVER_SOLVED;
    } else if (I.ktratio > (1.0 / tkt) * 1000.0) {
        if (dot_bz < -tia && I.res_primal_inf < -tir * dot_bz)
            I.status = almost ? CHIP_SOLVER_ALMOST_PRIMAL_INFEASIBLE : CHIP_SOLVER_PRIMAL_INFEASIBLE;
        else if (dot_qx < -tia && I.res_dual_inf < -tir * dot_qx)
            I.status = almost ? CHIP_SOLVER_ALMOST_DUAL_INFEASIBLE : CHIP_SOLVER_DUAL_INFEASIBLE;
    }
}

// check_termination (info.rs:182-231); solve_time: the time so far, setup included
inline bool ipm_check_termination(IpmInfo &I, const chip_solver_settings &st, int iter, double solve_time) {
    ipm_check_convergence(I, st, false);
    if (I.status == CHIP_SOLVER_UNSOLVED && iter > 1 && (I.res_dual > I.prev_res_dual || I.res_primal > I.prev_res_primal)) {
        if (I.ktratio < std::numeric_limits<double>::epsilon() * 100.0 &&
            (I.prev_gap_abs < st.tol_gap_abs || I.prev_gap_rel < st.tol_gap_rel))
            I.status = CHIP_SOLVER_INSUFFICIENT_PROGRESS;
        if (I.ktratio < 1.0) {
            if ((I.res_dual > st.tol_feas * 100.0 && I.res_dual > I.prev_res_dual * 100.0) ||
                (I.res_primal > st.tol_feas * 100.0 && I.res_primal > I.prev_res_primal * 100.0))
                I.status = CHIP_SOLVER_INSUFFICIENT_PROGRESS;
        }
    }
    if (I.status == CHIP_SOLVER_UNSOLVED) {
        if (st.max_iter == I.iterations) I.status = CHIP_SOLVER_MAX_ITERATIONS;
        else if (solve_time > st.time_limit) I.status = CHIP_SOLVER_MAX_TIME;
    }
    return I.status != CHIP_SOLVER_UNSOLVED;
}

// save_prev_iterate (info.rs:233-242) and reset_to_prev_iterate (info.rs:244-253): the scalars; the callers move the
// variables
inline void ipm_save_prev(IpmInfo &I) {
    I.prev_cost_primal = I.cost_primal;
    I.prev_cost_dual = I.cost_dual;
    I.prev_res_primal = I.res_primal;
    I.prev_res_dual = I.res_dual;
    I.prev_gap_abs = I.gap_abs;
    I.prev_gap_rel = I.gap_rel;
}
inline void ipm_reset_to_prev(IpmInfo &I) {
    I.cost_primal = I.prev_cost_primal;
    I.cost_dual = I.prev_cost_dual;
    I.res_primal = I.prev_res_primal;
    I.res_dual = I.prev_res_dual;
    I.gap_abs = I.prev_gap_abs;
    I.gap_rel = I.prev_gap_rel;
}

inline bool ipm_is_infeasible(int s) {
    return s == CHIP_SOLVER_PRIMAL_INFEASIBLE || s == CHIP_SOLVER_DUAL_INFEASIBLE ||
           s == CHIP_SOLVER_ALMOST_PRIMAL_INFEASIBLE || s == CHIP_SOLVER_ALMOST_DUAL_INFEASIBLE;
}

// info.post_process (info.rs:95-105) and the scalar part of solution.post_process (solution.rs:68-93): the reduced
// tolerances for a solve that ended in an error or at a limit, NaN objectives for an infeasible status, and the
// factors that unscale x and s (*scale_x) and z (*scale_z)
inline void ipm_post_process(IpmInfo &I, const chip_solver_settings &st, double tau, double kappa, double c,
                             double *obj_val, double *obj_val_dual, double *scale_x, double *scale_z) {
    const int s = I.status;
    if (s == CHIP_SOLVER_NUMERICAL_ERROR || s == CHIP_SOLVER_INSUFFICIENT_PROGRESS || s == CHIP_SOLVER_MAX_ITERATIONS ||
        s == CHIP_SOLVER_MAX_TIME)
        ipm_check_convergence(I, st, true);
    const bool inf = ipm_is_infeasible(I.status);
    *obj_val = inf ? std::numeric_limits<double>::quiet_NaN() : I.cost_primal;
    *obj_val_dual = inf ? std::numeric_limits<double>::quiet_NaN() : I.cost_dual;
    const double scaleinv = inf ? 1.0 / kappa : 1.0 / tau;
    *scale_x = scaleinv;
    *scale_z = scaleinv * (1.0 / c);
}

} // namespace chip
