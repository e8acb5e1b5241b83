"""tests/nonsym_ref.py checked on the CPU by means that do not share its formulas: the gradients, Hessians and the
third-order correction against mp.diff of the barrier functions written out here, the identities <s, g(s)> = -nu and
g*(-g(s)) = -s of a conjugate pair, the secant equations of the primal-dual scaling, Hs = mu Hd on the fallback and dual
branches, the GenPow primal gradient with a w part through the exact root of mp.findroot, the step-length references
of all three cones against a bisection for the exact boundary crossing, and every condition of the
module docstring of nonsym_ref (E <= E_CAP, the branch margins, the step-length margins, finite barriers) for every input
tests/test_nonsym_passes_gpu.py uses, with each E printed (pytest -s)."""
import mpmath as mp
import numpy as np
import pytest

from tests import nonsym_ref as R

EXP, POW = R.EXP, R.POW
TINY = mp.mpf(10) ** -40  # agreement asked of two 60-digit evaluations (mp.diff steps at 10^-20 .. 10^-30 of the point)


# ---- the barrier functions, written out separately -------------------------------------------------------------------
def f_dual(isexp, a, z):
    """the dual barriers (expcone.rs:245-254, powcone.rs:249-261)"""
    if isexp:
        return -mp.log(-z[2] * z[0]) - mp.log(z[1] - z[0] - z[0] * mp.log(-z[2] / z[0]))
    return (-mp.log((z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a) - z[2] ** 2) - (1 - a) * mp.log(z[0])
            - a * mp.log(z[1]))


def f_dual_genpow(alpha, z):
    d1 = len(alpha)
    phi = mp.mpf(1)
    for a, x in zip(alpha, z[:d1]):
        phi *= (x / a) ** (2 * a)
    return -mp.log(phi - sum(w * w for w in z[d1:])) - sum((1 - a) * mp.log(x) for a, x in zip(alpha, z[:d1]))


def partial(f, x, orders):
    return mp.diff(lambda *v: f(list(v)), tuple(x), tuple(orders))


def unit(n, *idx):
    o = [0] * n
    for i in idx:
        o[i] += 1
    return o


def close(a, b, scale=1):
    return abs(a - b) <= mp.mpf(10) ** -25 * max(abs(mp.mpf(scale)), abs(b))


POINTS = [(kind, j) for kind in (EXP, POW) for j in (0, 1, 2)]


@pytest.mark.parametrize("kind,j", POINTS)
def test_dual_gradient_and_hessian_against_mp_diff(kind, j):
    pt = R.late_point(kind, 1e-2, 1e-3, j)
    with mp.workdps(R.DPS):
        z, a = R.mpv(pt["z"]), mp.mpf(pt["a"])
        grad, Hd = R.ns3_dual_grad_hess(pt["isexp"], pt["a"], pt["z"])
        f = lambda v: f_dual(pt["isexp"], a, v)  # noqa: E731
        for i in range(3):
            assert close(grad[i], partial(f, z, unit(3, i))), ("grad", i)
            for k in range(i, 3):
                assert close(Hd[R.IDX[i][k]], partial(f, z, unit(3, i, k))), ("Hd", i, k)


@pytest.mark.parametrize("kind,j", POINTS)
def test_third_order_correction_against_mp_diff(kind, j):
    """eta = 1/2 D^3 f*(z)[u, v] with Hd u = ds (expcone.rs:256-328, powcone.rs:263-352): the mixed second derivative of
    the gradient along u and v"""
    c = R.ns3_case("late 1", kind, j, 0)
    pt, ref = c["pt"], c["ref"]
    with mp.workdps(R.DPS):
        z, a = R.mpv(pt["z"]), mp.mpf(pt["a"])
        eta, pivot = ref.higher_correction(c["step_s"], c["step_z"])
        assert pivot > 0
        Hd = mp.matrix([[ref.Hd[R.IDX[i][k]] for k in range(3)] for i in range(3)])
        u = list(mp.lu_solve(Hd, mp.matrix(R.mpv(c["step_s"]))))
        v = R.mpv(c["step_z"])
        f = lambda p: f_dual(pt["isexp"], a, p)  # noqa: E731
        for i in range(3):
            gi = lambda t, r, i=i: partial(f, [z[k] + t * u[k] + r * v[k] for k in range(3)], unit(3, i))  # noqa: E731
            third = mp.diff(gi, (0, 0), (1, 1))
            assert abs(eta[i] - third / 2) <= mp.mpf(10) ** -12 * max(abs(e) for e in eta), (i, eta[i], third)


@pytest.mark.parametrize("kind,j", POINTS + [(POW, 3), (POW, 5)])
def test_conjugate_gradient_identities(kind, j):
    """<s, g(s)> = -3 and g*(-g(s)) = -s for the exact primal gradient; the reference's own (one-sided Newton) iterate is
    printed beside it: for the power cone with alpha != 0.5 it is the starting point, up to 0.20 away (1.96e-1 at alpha 0.1, s2 = +-v)"""
    for name in R.BRANCH_POINTS[kind]:
        pt = R.branch_point(name, j)
        with mp.workdps(R.DPS):
            s = R.mpv(pt["s"])
            g = R.ns3_primal_grad(pt["isexp"], pt["a"], pt["s"], exact=True)[0]
            gref = R.ns3_primal_grad(pt["isexp"], pt["a"], pt["s"])[0]
            print("  %-36s alpha %.2f: reference's g against the conjugate gradient %.2e" % (name, pt["a"], R.rel_vec([float(x) for x in gref], g)))
            assert abs(R.mp_dot(s, g) + 3) <= TINY
            back, _ = R.ns3_dual_grad_hess(pt["isexp"], pt["a"], [-x for x in g])
            assert all(abs(b + x) <= TINY * (1 + abs(x)) for b, x in zip(back, s))


@pytest.mark.parametrize("d1,d2", [(2, 0), (2, 1), (5, 3)])
def test_genpow_gradient_hessian_and_identities(d1, d2):
    pt = R.gpw_point(d1, d2, 1e-2, 1e-3)
    mu = 0.7
    ref = R.GpwScaling(pt["alpha"], d2, pt["z"], mu)
    n = d1 + d2
    with mp.workdps(R.DPS):
        z, al = R.mpv(pt["z"]), [mp.mpf(a) for a in pt["alpha"]]
        f = lambda v: f_dual_genpow(al, v)  # noqa: E731
        for i in range(n):
            assert close(ref.grad[i], partial(f, z, unit(n, i)))
            e = [mp.mpf(1 if k == i else 0) for k in range(n)]
            col = ref.mul_hs(e)  # mu (D + p p' - q q' - r r') e_i = mu Hess f*(z) e_i
            for k in range(n):
                assert close(col[k], mu * partial(f, z, unit(n, i, k)), scale=max(abs(c) for c in col)), (i, k)
        assert abs(R.mp_dot(z, ref.grad) + (d1 + 1)) <= 1e-13  # <z, g*(z)> = -nu (alpha sums to one in double only)
        assert R.gpw_feasibility(pt["alpha"], False, [-g for g in ref.grad])[0]  # -g*(z) is primal-interior
    if d2 == 0:  # <s, g(s)> = -(dim1 + 1) and g*(-g(s)) = -s: the primal gradient without a w part is in closed form
        with mp.workdps(R.DPS):
            s = R.mpv(pt["s"])
            g = [-(1 + a) / p for a, p in zip(al, s)]
            assert abs(R.mp_dot(s, g) + (d1 + 1)) <= 1e-13
            back = R.GpwScaling(pt["alpha"], 0, [-x for x in g], mu).grad
            assert all(abs(b + x) <= TINY * (1 + abs(x)) for b, x in zip(back, s))


@pytest.mark.parametrize("d1,d2", [(2, 1), (5, 3), (3, 40)])
def test_genpow_conjugate_gradient_with_a_w_part(d1, d2):
    """dim2 > 0: the primal gradient with the exact root of the reference's f (mp.findroot) and the w part along s_w
    satisfies <s, g(s)> = -(dim1 + 1) and g*(-g(s)) = -s, with g* the dual gradient of GpwScaling, whose formula is
    checked against mp.diff above.  Neither identity uses f.  The reference's own one-sided iterate is printed beside
    the exact root"""
    for delta, mu in ((1e-2, 1e-3), (0.5, 1.0)):
        pt = R.gpw_point(d1, d2, delta, mu)
        with mp.workdps(R.DPS):
            s = R.mpv(pt["s"])
            g, margin, _ = R.gpw_primal_grad(pt["alpha"], pt["s"], exact=True)
            gref, _, newton = R.gpw_primal_grad(pt["alpha"], pt["s"])
            print("  (%d, %d) delta %.0e: reference's g against the conjugate gradient %.2e (Newton margin %.1e)" % (
                d1, d2, delta, R.rel_vec([float(x) for x in gref], g), float(newton)))
            assert margin >= R.MARGIN  # (the Newton branch, norm_r > eps)
            assert abs(R.mp_dot(s, g) + (d1 + 1)) <= 1e-13  # (alpha sums to one in double only)
            back = R.GpwScaling(pt["alpha"], d2, [-x for x in g], 1.0).grad
            assert all(abs(b + x) <= TINY * (1 + abs(x)) for b, x in zip(back, s))


@pytest.mark.parametrize("kind,j", POINTS + [(POW, 4)])
def test_secant_equations_and_fallback(kind, j):
    """primal-dual branch: Hs z = s and Hs zt = st (zt the exact primal gradient, st the dual gradient) -- the two secant
    equations the BFGS-style update is built to satisfy; central pair and strategy 1: Hs = mu Hd, with mu = <s, z> / 3 for
    the fallback and the mu passed in for the dual strategy"""
    pt = R.late_point(kind, 1e-2, 1e-3, j)
    with mp.workdps(R.DPS):
        ref = R.Ns3Scaling(pt["isexp"], pt["a"], pt["s"], pt["z"], 0.123, 0, exact=True)
        assert ref.branch == "primal-dual"
        s, z = R.mpv(pt["s"]), R.mpv(pt["z"])
        hz, hzt = ref.mul_hs(z), ref.mul_hs(ref.zt)
        assert all(abs(a - b) <= TINY * (1 + abs(b)) for a, b in zip(hz, s))
        assert all(abs(a - b) <= TINY * (1 + abs(b)) for a, b in zip(hzt, ref.grad))
        cen = R.late_point(kind, 1e-2, 1e-3, j, central=True)
        fb = R.Ns3Scaling(cen["isexp"], cen["a"], cen["s"], cen["z"], 0.123, 0)
        assert fb.branch == "fallback" and abs(fb.de1) < mp.mpf(10) ** -12
        mu = R.mp_dot(R.mpv(cen["s"]), R.mpv(cen["z"])) / 3
        assert all(h == mu * d for h, d in zip(fb.Hs, fb.Hd)) and abs(mu / mp.mpf(cen["mu"]) - 1) < mp.mpf(10) ** -12
        du = R.Ns3Scaling(pt["isexp"], pt["a"], pt["s"], pt["z"], 0.123, 1)
        assert du.branch == "dual" and all(h == mp.mpf(0.123) * d for h, d in zip(du.Hs, du.Hd))


def test_step_length_reference_against_bisection():
    """the accepted candidate lies below the exact boundary crossing and the rejected one before it above; 0.0 only where
    the crossing is below every candidate down to 1e-4"""
    a0 = R.first_candidate(1.0)
    for kind in (EXP, POW):
        for j in range(R.POOL):
            pt = R.ns3_pool_point("late 0", kind, j)
            for coef, side in ((-2.2, "z"), (-2.2, "s"), (-1e5, "z"), (0.3, "s")):
                dz, ds = R.ns3_step_direction(pt, kind, j, coef, side)
                got, margin = R.ns3_step(pt["isexp"], pt["a"], dz, ds, pt["z"], pt["s"], a0)
                assert margin >= R.STEP_MARGIN
                crossing = mp.inf
                for dual, q, dq in ((True, pt["z"], dz), (False, pt["s"], ds)):
                    feas = lambda p, dual=dual: R.ns3_feasibility(pt["isexp"], dual, pt["a"], p)  # noqa: E731
                    with mp.workdps(R.DPS):
                        if not feas([mp.mpf(float(x)) + mp.mpf(a0) * mp.mpf(float(d)) for x, d in zip(q, dq)])[0]:
                            crossing = min(crossing, R.step_boundary_bisect(feas, q, dq, a0))
                if crossing == mp.inf:
                    assert got == a0
                elif got == 0.0:
                    assert crossing < R.MIN_STEP / R.BACKTRACK
                else:
                    assert got < crossing < got / R.BACKTRACK * (1 + 1e-15), (got, float(crossing))
    for d1, d2 in ((2, 1), (64, 64), (3, 300)):  # gpw_step, the cases of the GPU file
        alpha = R.gpw_set_point(d1, d2, R.GPW_STEP_SET)["alpha"]
        for case in R.GPW_STEP_CASES:
            dz, ds, z, s, amax = R.gpw_step_case(d1, d2, R.GPW_STEP_SET, case)
            got, margin = R.gpw_step_expected(d1, d2, R.GPW_STEP_SET, case)
            assert margin >= R.STEP_MARGIN
            crossing = mp.inf
            for dual, q, dq in ((True, z, dz), (False, s, ds)):
                feas = lambda p, dual=dual: R.gpw_feasibility(alpha, dual, p)  # noqa: E731
                with mp.workdps(R.DPS):
                    if not feas([mp.mpf(float(x)) + mp.mpf(a0) * mp.mpf(float(d)) for x, d in zip(q, dq)])[0]:
                        crossing = min(crossing, R.step_boundary_bisect(feas, q, dq, a0))
            print("  genpow (%d, %d) %-16s -> %.17g, exact crossing %s" % (d1, d2, case, got, mp.nstr(crossing, 12)))
            if crossing == mp.inf:
                assert got == a0 and case == "stays feasible"
            elif got == 0.0:
                assert crossing < R.MIN_STEP / R.BACKTRACK and case == "ends at 0"
            else:
                assert got < crossing < got / R.BACKTRACK * (1 + 1e-15), (got, float(crossing))
    # the candidates are the kernel's own products
    c = [a0]
    while c[-1] * R.BACKTRACK >= R.MIN_STEP:
        c.append(c[-1] * R.BACKTRACK)
    assert R.ns3_step_expected(1, "late 0", "backtracks")[0] in c and len(c) == 42


# ---- the conditions of every input the GPU file uses --------------------------------------------------------------
@pytest.mark.parametrize("set_name", R.NS3_SETS)
def test_conditions_of_the_exp_pow_inputs(set_name):
    worst = {}
    for kind in (EXP, POW):
        for j in range(R.POOL):
            for strategy in (0, 1):
                c = R.ns3_case(set_name, kind, j, strategy)
                print("  %-10s %s point %d strategy %d: %-11s margin %.1e Newton margin %.1e kappa %.1e  E %s" % (
                    set_name, "exp" if kind == EXP else "pow", j, strategy, c["branch"], c["margin"], c["newton_margin"], c["kappa"],
                    " ".join("%s %.1e" % kv for kv in sorted(c["E"].items()))))
                assert max(c["E"].values()) <= R.E_CAP
                assert c["margin"] >= R.MARGIN
                assert c["newton_margin"] >= R.NEWTON_MARGIN
                want = "dual" if strategy == 1 else R.STRATEGY0_BRANCH.get(set_name.split()[0])
                assert want is None or c["branch"] == want  # (late and inward sets: primal-dual, exp and pow alike)
                assert ("shift" in c["E"]) == (set_name not in R.THIRD_ORDER_MOVED_FROM)
                for k, v in c["E"].items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print("  %s: largest E %s" % (set_name, " ".join("%s %.1e" % kv for kv in sorted(worst.items()))))


def test_branch_points_take_their_branches():
    with mp.workdps(R.DPS):
        for j in range(R.POOL):
            lo = R.wright_argument(R.branch_point(R.BRANCH_POINTS[EXP][0], j)["s"])
            hi = R.wright_argument(R.branch_point(R.BRANCH_POINTS[EXP][1], j)["s"])
            assert lo < 1 + mp.pi < hi
            assert R.branch_point("pow s2 = 0", j)["s"][2] == 0.0
            assert R.branch_point("pow s2 = +v", j)["s"][2] > 0.1 and R.branch_point("pow s2 = -v", j)["s"][2] < -0.1
            a = R.branch_point("pow alpha away from 0.5", j)["a"]
            assert a == R.POW_ALPHAS[j] and (abs(a - 0.5) > 0.09 if j else a == 0.5)
    pts = R.ns3_handle_points(257, "late 1")
    assert all(pts[c]["s"].tobytes() != pts[c - 256]["s"].tobytes() for c in range(256, 257))
    assert len({(p["tag"], p["s"].tobytes()) for p in pts}) == 2 * R.POOL


@pytest.mark.parametrize("set_name", R.STEP_SETS)
def test_conditions_of_the_exp_pow_step_cases(set_name):
    a0 = R.first_candidate(1.0)
    for n in R.NS3_SIZES:
        for case in R.STEP_CASES:
            want, margin = R.ns3_step_expected(n, set_name, case)
            print("  %s, %d cones, %-16s -> %.17g (margin %.1e)" % (set_name, n, case, want, margin))
            assert margin >= R.STEP_MARGIN
            assert want == {"stays feasible": a0, "ends at 0": 0.0}.get(case, a0 * 0.8 * 0.8 * 0.8 * 0.8)
    # "last cone limits": without the last cone the step is the full one
    dz, ds, z, s, amax, coefs = R.ns3_step_case(257, set_name, "last cone limits")
    assert coefs.count(-2.2) == 1 and coefs[-1] == -2.2


@pytest.mark.parametrize("set_name", R.BARRIER_SETS)
def test_conditions_of_the_exp_pow_barrier_cases(set_name):
    for alpha in R.BARRIER_ALPHAS:
        for kind in (EXP, POW):
            for j in range(R.POOL):
                b, kap, margin, newton = R.ns3_barrier_case(set_name, kind, j, alpha)
                assert mp.isfinite(b) and margin >= R.MARGIN and newton >= R.NEWTON_MARGIN, (set_name, kind, j, alpha, float(margin), float(newton))
        for n in R.NS3_SIZES:  # E of the whole handle's barrier, as the GPU file takes it
            cones = R.oracle_mod().Cones(R.ns3_specs(n))
            cat = lambda name: R.tile_cones(n, lambda kind, j: R.ns3_case(set_name, kind, j, 0)[name] if name in ("step_z", "step_s")  # noqa: E731
                                            else R.ns3_pool_point(set_name, kind, j)[name])
            with mp.workdps(R.DPS):
                ref = mp.fsum(R.ns3_barrier_case(set_name, EXP if c % 2 == 0 else POW, c % R.POOL, alpha)[0] for c in range(n))
            E = float(abs(mp.mpf(cones.compute_barrier(cat("z"), cat("s"), cat("step_z"), cat("step_s"), alpha)) - ref)) / max(1.0, abs(float(ref)))
            print("  %s, %d cones, barrier at alpha %.1f: %.12g  E %.1e" % (set_name, n, alpha, float(ref), E))
            assert E <= R.E_CAP


@pytest.mark.parametrize("d1,d2", R.GPW_SIZES)
def test_conditions_of_the_genpow_inputs(d1, d2):
    for set_name in R.GPW_SETS:
        c = R.gpw_case(d1, d2, set_name)
        print("  (%d, %d) %s: kappa %.1e  E %s" % (d1, d2, set_name, c["kappa"], " ".join("%s %.1e" % kv for kv in sorted(c["E"].items()))))
        assert max(c["E"].values()) <= R.E_CAP
        a = c["pt"]["alpha"]
        assert abs(a.sum() - 1.0) < 1e-15 and a.max() / a.min() > 1.5  # normalised, not uniform
        if d2:
            sw, zw = c["pt"]["s"][d1:], c["pt"]["z"][d1:]
            assert abs(abs(sw @ zw) - np.linalg.norm(sw) * np.linalg.norm(zw)) <= 1e-14 * np.linalg.norm(sw) * np.linalg.norm(zw)
    a0 = R.first_candidate(1.0)
    for case in R.GPW_STEP_CASES:
        if d2 == 0 and case == "last w leaves":
            continue
        want, margin = R.gpw_step_expected(d1, d2, R.GPW_STEP_SET, case)
        print("  (%d, %d) step %-16s -> %.17g (margin %.1e)" % (d1, d2, case, want, margin))
        assert margin >= R.STEP_MARGIN
        if case == "stays feasible":
            assert want == a0
        elif case == "ends at 0":
            assert want == 0.0
        else:
            assert 0.0 < want < a0
    for alpha in R.BARRIER_ALPHAS:
        b, kap, margin, newton, pt, dz, ds = R.gpw_barrier_case(d1, d2, alpha)
        orc = R.GpwOracle(pt)
        assert orc.cones.update_scaling(pt["s"], pt["z"], 1.0, 1)
        E = abs(orc.cones.compute_barrier(pt["z"], pt["s"], dz, ds, alpha) - float(b)) / max(1.0, abs(float(b)))
        print("  (%d, %d) barrier at alpha %.1f: %.12g  E %.1e kappa %.1e margin %.1e Newton margin %.1e" % (d1, d2, alpha, float(b), E, kap, float(margin), float(newton)))
        assert mp.isfinite(b) and E <= R.E_CAP and margin >= R.MARGIN and newton >= R.NEWTON_MARGIN
        if d2:  # the Newton branch is the one taken
            assert np.linalg.norm(pt["s"][d1:]) > 1e-3


def test_the_split_of_write_hs_falls_inside_a_cone():
    """k_ns3_write_hs: thread t writes entry t - 6 (t / 6) of cone t / 6.  With 43 cones the first workgroup ends at t = 255 =
    6 * 42 + 3, so cone 42 has entries 0..3 in workgroup 0 and 4, 5 in workgroup 1; with 42 cones (252 threads) there is no
    second workgroup.  `t >> 3` instead of `t / 6` sends thread t to cone t / 8 with k = t - 6 (t / 8) up to 71: of 43 cones
    only cones 0..32 are addressed at all (257 / 8 = 32), each through entries of its neighbours' maps and states, and cones
    33..42 keep what the scramble's pair left.  Their pool points differ from the scramble's, so
    test_exp_pow_scaling[43-*] compares stale entries with the reference of other inputs and fails; this mutant is argued
    here, on the CPU, and not run."""
    n = 43
    threads = 6 * n
    assert (threads + 255) // 256 == 2 and 255 // 6 == 42 and 255 - 6 * 42 == 3
    assert (6 * 42 + 255) // 256 == 1
    wrong = {t >> 3 for t in range(threads)}
    assert max(wrong) == 32 and len(wrong) < n
    pts, scr = R.ns3_handle_points(n, "late 1"), R.ns3_handle_points(n, "late 0")
    assert all(pts[c]["s"].tobytes() != scr[c]["s"].tobytes() for c in range(33, n))
