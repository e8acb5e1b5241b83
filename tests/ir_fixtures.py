"""Systems on which the iterative refinement of the KKT solve (directldlkktsolver.rs:266-321) takes every decision it can
take, with margins: shared by tests/test_ir_ref_host.py (CPU: the conditions, against the oracle) and
tests/test_ir_decisions_gpu.py (every solve path against the traces of tests/ir_ref.py).

The lever is the static regulariser.  With static_regularization_constant = EPS and the proportional part 0 the factor
is that of K + EPS * diag(signs); refinement against the unregularised K contracts a mode of generalised eigenvalue mu by
EPS / (mu + EPS) per round, and a diagonal entry P_ii = -P_NEG with P_NEG < EPS < 2 P_NEG GROWS by EPS / (EPS - P_NEG)
instead (the pivot EPS - P_NEG keeps its sign: no dynamic regularisation).  grow() gives a problem of the generators an
explicit diagonal P = I with that one entry, and scales column i of A so that x_i is all but decoupled from the rest;
the scale of b_i then places the round at which the growing mode takes over:
    rhs "late"   b_i = LATE[problem]: a few rounds improve by the contraction of the other modes, then one worsens by GROWTH
    rhs "first"  b_i = 1: the growing mode leads from round 1 on, every round worsens by GROWTH
    rhs "other"  another vector of the kind of "late" (the solve after each scenario; the member of a pair that stops at once)
    rhs "big"    2^20 * "late": the same trace scaled, beside "other" in a pair under one abstol
scenarios() turns the all-accepting trace of "late" (stop_ratio = 0, no tolerance, 17 rounds) into the settings of the
issue's table: thresholds are placed at the geometric mean of the two numbers they have to separate."""
import math

import numpy as np
import scipy.sparse as sp

from tests import ir_ref

TOL = 1e-8  # tests/test_bundle_pattern_gpu.py
EPS = 0.01
P_NEG = 0.007
GROWTH = EPS / (EPS - P_NEG)  # 3.33 per round
COL_SCALE = 1e-9
# b_i of rhs "late" per problem: chosen with the oracle so that two rounds improve and the third worsens, every decision a
# factor 2.7 or more from its threshold (a scan over 1e-5 .. 1e-8; conditions asserted in tests/test_ir_ref_host.py)
LATE = {"socp_5x170": 1e-6, "socp_19x341": 3e-6, "socp_3x200": 1e-6, "socp_12x300": 3e-6, "three_row_top": 3e-6,
        "ragged_forest": 3e-6, "qp_3000": 3e-6}
MANY = 17
# problem "qp_3000_slow": P_ii = +P_SLOW instead, b_i = 1: that mode CONTRACTS by EPS / (P_SLOW + EPS) = 0.714 per round and leads
# every norm, so 17 rounds improve by 1.4 each and the norms of rounds 15 - 17 are 100 times smaller than those of rounds
# 2 - 4 whose norm sets the host path reuses (NRM_SETS = 16): a set that is not cleared first makes round 15 look 70 times worse
P_SLOW = 0.004
SLOW_IR = dict(reltol=0.0, abstol=0.0, stop_ratio=0.6, max_iter=MANY)
BIG = 2.0 ** 20  # rhs "big" = BIG * "late" (exact scaling): the member of a pair that must NOT stop on the shared abstol
REG = dict(static_regularization_enable=1, static_regularization_constant=EPS, static_regularization_proportional=0.0)
DEFAULT_IR = dict(enable=True, max_iter=10, reltol=1e-13, abstol=1e-12, stop_ratio=5.0)  # settings.rs:160-181


def _csc(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return (M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64))


def grow(pr, late, var=None, diag=-P_NEG):
    """`pr` with P = I except P[var, var] = diag, column `var` of A scaled by COL_SCALE"""
    n, m = pr["n"], pr["m"]
    var = n // 2 if var is None else var
    d = np.ones(n)
    d[var] = diag
    A = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n)).copy()
    A.data[A.indptr[var]:A.indptr[var + 1]] *= COL_SCALE
    out = dict(pr)
    out.update(P=_csc(sp.diags(d)), A=_csc(A), var=var, late=late)
    return out


def rhs(pr, kind):
    """(rhsx, rhsz) of the kind named in the module docstring"""
    rng = np.random.default_rng(dict(late=3, first=3, other=4, big=3)[kind])
    rx, rz = rng.standard_normal(pr["n"]), rng.standard_normal(pr["m"])
    rx[pr["var"]] = 1.0 if kind == "first" else pr["late"]
    if kind == "big":
        return BIG * rx, BIG * rz
    return rx, rz


def pair_settings(ref):
    """ONE setting under which rhs "other" stops on tolerance in round 0 and rhs "big" goes through the rounds of "late"
    to its rejection: abstol at the geometric mean of other's first norm and the smallest norm big's loop looks at"""
    other, big = ref.base("other"), ref.base("big")
    imp = [r[1] for r in big["rounds_list"]]
    k = next(i for i, v in enumerate(imp) if v < 1.0)
    norms = [big["norme0"]] + [r[0] for r in big["rounds_list"]]
    return dict(reltol=0.0, abstol=_mid(other["norme0"], min(norms[:k + 1]))), k


def hip_settings(hip, ir=None, **kw):
    ir = dict(DEFAULT_IR, **(ir or {}))
    return hip.Settings.default(iterative_refinement_enable=int(ir["enable"]), iterative_refinement_max_iter=ir["max_iter"],
                                iterative_refinement_reltol=ir["reltol"], iterative_refinement_abstol=ir["abstol"],
                                iterative_refinement_stop_ratio=ir["stop_ratio"], **dict(REG, **kw))


def oracle_settings(oracle, ir=None):
    ir = dict(DEFAULT_IR, **(ir or {}))
    st = oracle.Settings.default()
    st.static_reg_enable, st.static_reg_constant, st.static_reg_proportional = 1, EPS, 0.0
    st.ir_enable, st.ir_max_iter, st.ir_reltol = int(ir["enable"]), ir["max_iter"], ir["reltol"]
    st.ir_abstol, st.ir_stop_ratio = ir["abstol"], ir["stop_ratio"]
    return st


class Reference:
    """the oracle's KKTSolver of a problem at its scaling point (permutation `perm`), K's rows, and traces by settings"""

    def __init__(self, oracle, pr, perm=None):
        self.oracle, self.pr, self.perm = oracle, pr, perm
        self.cones = oracle.Cones(pr["cones"])
        self.raw = oracle_settings(oracle, dict(enable=False))
        self.ko = oracle.KKTSolver(pr["n"], pr["m"], pr["P"], pr["A"], self.cones, settings=self.raw, perm=perm)
        assert self.cones.update_scaling(pr["s"], pr["z"]) and self.ko.update()
        self.N, self.nvis = self.ko.N, pr["n"] + pr["m"]
        km = self.ko.kkt
        self.triu = (km.colptr, km.rowval, km.nzval)
        self.rows = ir_ref.full_rows(self.N, *self.triu)
        self.dsigns = self.ko.dsigns
        self._base = {}

    def ko_perm(self, hip):
        """the permutation this reference was factored under"""
        return self.perm if self.perm is not None else host_perm(hip, self.pr)

    def full(self, rx, rz):
        return np.concatenate([rx, rz, np.zeros(self.N - self.nvis)])

    def solve_raw(self, b):
        """the oracle's factor of the regularised matrix, no refinement"""
        self.ko.settings = self.raw
        ok, x = self.ko.solve_full(b)
        assert ok
        return x

    def trace(self, b, ir):
        return ir_ref.trace(self.rows, self.solve_raw, b, **dict(DEFAULT_IR, **ir))

    def base(self, kind):
        """the all-accepting trace of rhs `kind`: every iterate the loop can reach under any settings"""
        if kind not in self._base:
            self._base[kind] = self.trace(self.full(*rhs(self.pr, kind)), dict(max_iter=MANY, reltol=0.0, abstol=0.0, stop_ratio=0.0))
        return self._base[kind]

    def oracle_solve(self, b, ir):
        """the oracle's own solve() with its own refinement -> (x full, rounds)"""
        self.ko.settings = oracle_settings(self.oracle, ir)
        ok, x = self.ko.solve_full(b)
        assert ok
        # (the oracle's counter is written by its refinement alone: switched off, it keeps the last solve's)
        return x, self.ko.last_ir_iters if dict(DEFAULT_IR, **ir)["enable"] else 0


def host_perm(hip, pr):
    """the fill-reducing permutation a handle of the package takes for `pr` (a host-only handle: no GPU needed)"""
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    return hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=hip_settings(hip, device=hip.DEVICE_HOST_ONLY)).perm


def _mid(a, b):
    return math.sqrt(a * b)


def scenarios(ref):
    """-> {id: (rhs kind, refinement settings)} from the all-accepting traces; what each must do: expected()"""
    late, first = ref.base("late"), ref.base("first")
    # (reject_first and worse_accepted rest on it: on "first" every round worsens, by about GROWTH)
    assert all(r[1] < 0.5 for r in first["rounds_list"]), [r[1] for r in first["rounds_list"]]
    nb = late["normb"]
    norms = [late["norme0"]] + [r[0] for r in late["rounds_list"]]
    imp = [r[1] for r in late["rounds_list"]]
    k = next(i for i, v in enumerate(imp) if v < 1.0)  # rounds 1 .. k improve, round k + 1 worsens
    assert k >= 2, imp
    zero = dict(reltol=0.0, abstol=0.0)
    sc = {
        "tol0": ("late", dict(reltol=100.0 * norms[0] / nb, abstol=0.0)),
        "tol_late": ("late", dict(reltol=_mid(norms[k - 1], norms[k]) / nb, abstol=0.0)),
        "accept_stop": ("late", dict(zero, stop_ratio=4.0 * imp[0])),
        "reject": ("late", dict(zero)),
        "reject_first": ("first", dict(zero, max_iter=1)),
        "reject_at_limit": ("late", dict(zero, max_iter=k + 1)),
        "worse_accepted": ("first", dict(zero, stop_ratio=0.0, max_iter=6)),
        "many_rounds": ("late", dict(zero, stop_ratio=0.0, max_iter=MANY)),
        "limit_30": ("late", dict(zero, max_iter=30)),
        "limit_31": ("late", dict(zero, max_iter=31)),
        "off": ("late", dict(enable=False)),
        "zero_iter": ("late", dict(max_iter=0)),
    }
    return sc, k


def expected(k):
    """{id: (rounds, accepted iterate, why_stopped)} with k the number of improving rounds of rhs "late" """
    return {"tol0": (0, 0, "tolerance"), "tol_late": (k, k, "tolerance"), "accept_stop": (1, 1, "stop_ratio"),
            "reject": (k + 1, k, "stop_ratio"), "reject_first": (1, 0, "stop_ratio"), "reject_at_limit": (k + 1, k, "stop_ratio"),
            "worse_accepted": (6, 6, "limit"), "many_rounds": (MANY, MANY, "limit"), "limit_30": (k + 1, k, "stop_ratio"),
            "limit_31": (k + 1, k, "stop_ratio"), "off": (0, 0, "disabled"), "zero_iter": (0, 0, "limit")}


def check_conditions(ref, name, kind, ir, tr, want):
    """the hard conditions of a fixture on the reference trace `tr` of scenario `name`; -> (decision margin, rounding
    ratio, separation) for the record"""
    assert tr["ok"], name
    assert (tr["rounds"], tr["accepted"], tr["why_stopped"]) == want, (name, tr["rounds"], tr["accepted"], tr["why_stopped"], want)
    dec, rnd = ir_ref.margins(tr, **dict(DEFAULT_IR, **ir))
    assert dec >= 2.0, (name, dec)
    assert rnd >= 1e3, (name, rnd)
    # the accepted iterate against every OTHER iterate the loop can reach on this right-hand side, on the visible part
    base = ref.base(kind)["iterates"]
    sep = ir_ref.separation(base, tr["accepted"], visible=ref.nvis)
    assert sep >= 100.0 * TOL, (name, sep)
    assert float(np.max(np.abs(base[tr["accepted"]] - tr["iterates"][tr["accepted"]]))) == 0.0, name
    assert ref.ko.ldl_regularize_count() == 0, name
    return dec, rnd, sep


# ---- the problems, as the existing tests of each solve path build them ---------------------------------------------------
def problem(name):
    from tests import problems
    if name.startswith("socp_"):
        nb, bs = (int(v) for v in name[5:].split("x"))
        seed = 3 if (nb, bs) == (12, 300) else 11
        return grow(problems.portfolio_socp(nb, bs, seed=seed), LATE[name])
    if name == "three_row_top":  # tests/test_ldl_backward_gpu.py: _three_row_top
        pr = problems.portfolio_socp(12, 600, seed=21)
        n, m = pr["n"], pr["m"]
        rng = np.random.default_rng(2)
        A = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n))
        A2 = sp.vstack([A, sp.csc_matrix(rng.uniform(0.5, 1.5, (2, n)))], format="csc")
        return grow(dict(n=n, m=m + 2, P=pr["P"], A=_csc(A2), cones=list(pr["cones"]) + [(0, 2)],
                         s=np.concatenate([pr["s"], np.zeros(2)]), z=np.concatenate([pr["z"], np.zeros(2)])), LATE[name])
    if name == "ragged_forest":  # tests/test_gpu_parity.py: test_grouped_fold_ragged_forest
        parts = [problems.portfolio_socp(2 + (i % 3), 120 + 40 * (i % 4), seed=100 + i) for i in range(14)]
        parts.append(problems.portfolio_socp(1, 20, seed=300))
        return grow(problems.blockdiag(parts), LATE[name])
    if name == "qp_3000_slow":
        return grow(problems.random_qp(3000, 6000, band=30, seed=2), 1.0, diag=P_SLOW)
    if name == "qp_3000":
        return grow(problems.random_qp(3000, 6000, band=30, seed=2), LATE[name])
    raise KeyError(name)


FAMILIES = {"socp": ["socp_5x170", "socp_19x341", "socp_3x200", "socp_12x300", "three_row_top", "ragged_forest"],
            "qp": ["qp_3000"]}
