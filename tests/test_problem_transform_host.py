"""Presolve and chordal decomposition on the host (no GPU needed): the new settings and their refusals, the transform
of chip_solver_create through the test hooks (presolve.rs's cases, the clique structure on banded, block-arrow and
random patterns under every merge method, both augmentations), and the equivalence of the transformed problem solved by
the CPU oracle's interior-point loop and reversed, with the untransformed solve."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import ipm_driver as ipm
from tests.test_solver_host import HIPCC, ROOT, _resources

ZERO, NN, SOC, EXP, POW, GENPOW, PSD = 0, 1, 2, 3, 4, 5, 6
SQ2 = np.sqrt(2.0)
MERGES = ["none", "parent_child", "clique_graph"]
TRANSFORM_FIELDS = ["presolve_enable", "chordal_decomposition_enable", "chordal_decomposition_merge_method",
                    "chordal_decomposition_compact", "chordal_decomposition_complete_dual"]
HOOKS = ["chip_debug_transform_create", "chip_debug_transform_destroy", "chip_debug_transform_get",
         "chip_debug_transform_reverse", "chip_debug_solver_internal_solution"]


def tri(k):
    return k * (k + 1) // 2


def triu_index(r, c):
    return tri(c) + r


# ---- problems ------------------------------------------------------------------------------------------------------
def csc(hip, M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return hip.CscMatrix(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def presolve_data():
    # presolve.rs:8-25: min 0.5 x'x + c'x s.t. 2x <= 1, -2x <= 1 (two NN(3) cones)
    P = sp.identity(3, format="csc")
    A = 2.0 * sp.vstack([sp.identity(3), -sp.identity(3)]).tocsc()
    return P, np.array([3.0, -2.0, 1.0]), A, np.ones(6), [(NN, 3), (NN, 3)]


def sdp_chordal_data():
    # sdp_chordal.rs:9-80 (numbers of the fixture)
    A = sp.csc_matrix((np.array([-1.0, -SQ2, -1.0, -1.0, -SQ2, -SQ2, -1.0, -1.0, -SQ2, -SQ2, -SQ2, -1.0, -1.0, -1.0,
                                 -1.0, -1.0]),
                       np.array([24, 7, 10, 22, 8, 12, 15, 25, 9, 13, 18, 21, 26, 0, 23, 27]),
                       np.array([0, 1, 4, 5, 8, 9, 10, 13, 16])), shape=(28, 8))
    b = np.zeros(28)
    b[1:7] = [3.0, 2 * SQ2, 2.0, SQ2, SQ2, 3.0]
    q = np.zeros(8)
    q[0] = -1.0
    return sp.csc_matrix((8, 8)), q, A, b, [(NN, 1), (PSD, 6), (POW, 3, 0, 1.0 / 3.0), (POW, 3, 0, 0.5)]


def mask_sdp(mask_pairs, N, seed=0, extra_nn=False):
    """min <C, X> + 0.5 |x|^2 over the entries x of the pattern, X = B - sum x_k E_k PSD with B = N I + pattern
    noise: one variable per off-diagonal pattern entry, one per diagonal; s = svec(X) in the PSD cone"""
    rng = np.random.default_rng(seed)
    m = tri(N)
    rows, cols, vals = [], [], []
    b = np.zeros(m)
    q = []
    j = 0
    for (r, c) in sorted(set(mask_pairs) | {(i, i) for i in range(N)}, key=lambda t: (t[1], t[0])):
        k = triu_index(r, c)
        rows.append(k)
        cols.append(j)
        vals.append(1.0 if r == c else SQ2)
        b[k] = float(N) if r == c else SQ2 * rng.uniform(-0.5, 0.5)
        q.append(rng.uniform(-1, 1))
        j += 1
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, j))
    cones = [(PSD, N)]
    if extra_nn:  # an infinite-bound NN row in front of the PSD cone, and a finite bound x_0 <= 10
        A = sp.vstack([sp.csc_matrix(([1.0, 1.0], ([0, 1], [0, 0])), shape=(2, j)), A]).tocsc()
        b = np.concatenate([[1e30, 10.0], b])
        cones = [(NN, 2)] + cones
    return sp.identity(j, format="csc") * 0.5, np.array(q), A, b, cones


def banded(N, w):
    return [(r, c) for c in range(N) for r in range(max(0, c - w), c)]


def block_arrow(N, blk, arrow):
    pairs = []
    for s0 in range(0, N - arrow, blk):
        for c in range(s0, min(s0 + blk, N - arrow)):
            pairs += [(r, c) for r in range(s0, c)]
    pairs += [(r, c) for c in range(N - arrow, N) for r in range(c)]
    return pairs


def random_pattern(N, p, seed):
    rng = np.random.default_rng(seed)
    return [(r, c) for c in range(N) for r in range(c) if rng.uniform() < p]


def transform(hip, P, q, A, b, cones, **kw):
    s = hip.SolverSettings.default(**kw)
    return hip.TransformDebug(csc(hip, sp.triu(P)), q, csc(hip, A), b, cones, s)


# ---- 1. settings -----------------------------------------------------------------------------------------------------
def test_transform_settings_defaults_and_refusals(hip):
    s = hip.SolverSettings.default()
    assert (s.presolve_enable, s.chordal_decomposition_enable) == (0, 0)  # off here (the reference: on)
    assert s.chordal_decomposition_merge_method == hip.MERGE_CLIQUE_GRAPH
    assert (s.chordal_decomposition_compact, s.chordal_decomposition_complete_dual) == (1, 1)
    assert C.sizeof(hip.SolverSettings) % 8 == 0
    assert hip.SolverSettings.presolve_enable.offset > hip.SolverSettings.min_terminate_step_length.offset
    for name, val in (("none", 0), ("parent_child", 1), ("clique_graph", 2)):
        s = hip.SolverSettings.default(chordal_decomposition_enable=1, chordal_decomposition_merge_method=name)
        assert s.chordal_decomposition_merge_method == val and s.chordal_decomposition_enable == 1
    with pytest.raises(ValueError):
        hip.SolverSettings.default(chordal_decomposition_merge_method="cliquegraph")
    with pytest.raises(ValueError):
        hip.SolverSettings.default(chordal_decomposition_merge_method=7)
    assert hip.ERR_UPDATE_NOT_ALLOWED == -11 and hip.STATUS_NAMES[-11] == "UpdateNotAllowed"


def test_transform_header_declares_the_new_abi():
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    assert "CHIP_ERR_UPDATE_NOT_ALLOWED = -11" in hdr
    assert re.search(r"int32_t chip_transform_get_info\(const chip_solver \*h, chip_transform_info \*out\);", hdr)
    body = re.search(r"typedef struct \{([^}]*)\} chip_solver_settings;", hdr, flags=re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names[names.index("min_terminate_step_length") + 1:] == TRANSFORM_FIELDS + ["reserved1"]


def test_transform_symbols_test_build_only(hip):
    L = C.CDLL(hip.LIB_PATH)
    assert hasattr(L, "chip_transform_get_info")
    for sym in HOOKS:
        assert hasattr(L, sym), sym
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    S = C.CDLL(hip.SHIP_LIB_PATH)
    assert hasattr(S, "chip_transform_get_info")
    for sym in HOOKS:
        assert not hasattr(S, sym), sym
    info = hip.TransformInfo()
    assert L.chip_transform_get_info(None, C.byref(info)) == hip.ERR_ARG


# ---- 2. presolve -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["single", "single_2", "cone", "all", "inf"])
def test_presolve_reduction(hip, case):
    P, q, A, b, cones = presolve_data()
    removed = {"single": [3], "single_2": [4], "cone": [0, 1, 2], "all": list(range(6)), "inf": [5]}[case]
    if case == "single_2":
        cones = [(ZERO, 2), (NN, 4)]
    for i in removed:
        b[i] = np.inf if case == "inf" else 1e30
    t = transform(hip, P, q, A, b, cones, presolve_enable=1)
    assert t.active and t.m_reduced == 6 - len(removed) and t.m2 == t.m_reduced and t.n2 == 3
    Pt, qt, At, bt, ct = t.problem()
    keep = [i for i in range(6) if i not in removed]
    assert np.array_equal(At.m and sp.csc_matrix((At.nzval, At.rowval, At.colptr), shape=(At.m, 3)).toarray(),
                          A.toarray()[keep]) if keep else At.m == 0
    assert np.array_equal(bt, b[keep])
    want = {"single": [(NN, 3), (NN, 2)], "single_2": [(ZERO, 2), (NN, 3)], "cone": [(NN, 3)], "all": [],
            "inf": [(NN, 3), (NN, 2)]}[case]
    assert ct == want
    x2, s2, z2 = np.arange(3.0), np.arange(t.m2) + 0.5, -np.arange(t.m2) - 0.25
    x, s, z = t.reverse(x2, s2, z2)
    assert np.array_equal(x, x2)
    assert np.array_equal(s[removed], np.full(len(removed), 1e20)) and np.array_equal(z[removed], np.zeros(len(removed)))
    assert np.array_equal(s[keep], s2) and np.array_equal(z[keep], z2)


def test_presolve_disabled_or_nothing_to_remove_is_inactive(hip):
    P, q, A, b, cones = presolve_data()
    assert not transform(hip, P, q, A, b, cones, presolve_enable=1).active
    b[3] = 1e30
    assert not transform(hip, P, q, A, b, cones).active
    assert not transform(hip, P, q, A, b, [(ZERO, 6)], presolve_enable=1).active  # only NN rows are reduced


# ---- 3. chordal structure ----------------------------------------------------------------------------------------------
def _check_structure(hip, N, pairs, merge, compact):
    P, q, A, b, cones = mask_sdp(pairs, N, seed=N)
    t = transform(hip, P, q, A, b, cones, chordal_decomposition_enable=1, chordal_decomposition_merge_method=merge,
                  chordal_decomposition_compact=int(compact))
    if not t.active:
        return None
    (p,) = t.patterns()
    cl = [set(c) for c in p["cliques"]]
    assert sorted(p["ordering"]) == list(range(N))
    # every mask entry (and every diagonal) lies in some clique
    for (r, c) in set(pairs) | {(i, i) for i in range(N)}:
        assert any(r in C_ and c in C_ for C_ in cl), (r, c)
    # the clique tree: parents later in post order, the root last, and the running-intersection property
    par = p["parent"]
    assert par[-1] == -1 and all(par[k] > k for k in range(len(par) - 1))
    for k in range(len(par) - 1):
        assert set(int(p["ordering"][v]) for v in p["sep"][k]) == cl[k] & cl[par[k]]
    for v in range(N):
        holders = [k for k in range(len(cl)) if v in cl[k]]
        tops = [k for k in holders if par[k] < 0 or v not in cl[par[k]]]
        assert len(tops) == 1, (v, holders)  # the cliques holding v form one subtree
    Pt, qt, At, bt, ct = t.problem()
    Ad = sp.csc_matrix((At.nzval, At.rowval, At.colptr), shape=(At.m, At.n)).toarray()
    A0 = A.toarray()
    nx = A.shape[1]
    sizes = [len(c) for c in p["cliques"]]
    if compact:
        assert ct == [(PSD, s) for s in reversed(sizes)]  # root first
        # every original row of the cone: its A row and b land on exactly one clique row (the others are overlaps)
        src, ptr = t.get("src"), t.get("ptr")
        for i in range(tri(N)):
            rows = src[ptr[i]:ptr[i + 1]]
            carrying = [r for r in rows if np.any(Ad[r, :nx] != 0) or bt[r] != 0]
            if np.any(A0[i] != 0) or b[i] != 0:
                assert len(carrying) == 1
                assert np.array_equal(Ad[carrying[0], :nx], A0[i]) and bt[carrying[0]] == b[i]
        # each overlap column: +1 in the child's entry, -1 in the parent's (same original row)
        for c in range(nx, At.n):
            nz = np.nonzero(Ad[:, c])[0]
            assert sorted(Ad[nz, c]) == [-1.0, 1.0]
    else:
        Hrow = t.get("H_row")
        assert ct == [(ZERO, tri(N))] + [(PSD, s) for s in sizes]
        assert len(Hrow) == sum(tri(s) for s in sizes) == t.m2 - tri(N)
        # H: one 1 per (clique entry, original row) pair
        want = [triu_index(cc[a], cc[bb]) for cc in p["cliques"] for bb in range(len(cc)) for a in range(bb + 1)]
        assert list(Hrow) == want
        assert np.array_equal(Ad[:tri(N), nx:], np.eye(tri(N))[:, Hrow])
        assert np.array_equal(Ad[tri(N):, nx:], -np.eye(len(Hrow)))
    return t


PATTERNS = {"banded": lambda: (40, banded(40, 3)), "block_arrow": lambda: (30, block_arrow(30, 6, 3)),
            "random": lambda: (25, random_pattern(25, 0.08, 3))}


@pytest.mark.parametrize("merge", MERGES)
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("compact", [True, False])
def test_chordal_structure(hip, pattern, merge, compact):
    N, pairs = PATTERNS[pattern]()
    t = _check_structure(hip, N, pairs, merge, compact)
    assert t is not None and t.npatterns == 1
    assert t.final_added <= t.premerge_added
    if merge == "none":
        assert t.final_added == t.premerge_added


def test_dense_or_small_cone_is_not_decomposed(hip):
    P, q, A, b, cones = mask_sdp(banded(6, 5), 6)  # dense
    assert not transform(hip, P, q, A, b, cones, chordal_decomposition_enable=1).active
    P, q, A, b, cones = mask_sdp([], 3)  # side 3
    assert not transform(hip, P, q, A, b, cones, chordal_decomposition_enable=1).active


# ---- 4. / 5. equivalence through the oracle's interior-point loop -------------------------------------------------------
def _oracle_solve(oracle, P, q, A, b, cones):
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    A = sp.csc_matrix(A)
    for M in (Pt, A):
        M.sort_indices()
    tup = lambda M: (M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64))
    bcap = np.minimum(np.asarray(b, float), 1e20)
    be = ipm.OracleBackend(oracle, Pt.shape[0], A.shape[0], tup(Pt), tup(A), np.asarray(q, float), bcap, cones)
    return ipm.solve(be, cones, q, bcap, max_iter=100)


def _check_equivalent(hip, oracle, P, q, A, b, cones, complete_dual=True, may_stay=False, ref_problem=None, **kw):
    # (ref_problem: the same problem for the reference solve, e.g. without a row the equilibration-free oracle loop
    # cannot carry at 1e20)
    ref = _oracle_solve(oracle, *(ref_problem or (P, q, A, b, cones)))
    assert ref["status"] == "Solved"
    t = transform(hip, P, q, A, b, cones, chordal_decomposition_complete_dual=int(complete_dual), **kw)
    if may_stay and not t.active:
        return t, None, None, None
    assert t.active
    Pt, qt, At, bt, ct = t.problem()
    Ps = sp.csc_matrix((Pt.nzval, Pt.rowval, Pt.colptr), shape=(Pt.m, Pt.n))
    As = sp.csc_matrix((At.nzval, At.rowval, At.colptr), shape=(At.m, At.n))
    out = _oracle_solve(oracle, Ps + sp.triu(Ps, 1).T, qt, As, bt, ct)
    assert out["status"] == "Solved"
    x, s, z = t.reverse(out["x"], out["s"], out["z"])
    x_ref = ref["x"]
    obj = lambda xx: 0.5 * xx @ (P @ xx) + q @ xx
    assert abs(obj(x) - obj(x_ref)) <= 1e-6 * max(1.0, abs(obj(x_ref)))
    fin = np.asarray(b) < 1e19
    assert np.linalg.norm((A @ x + s - b)[fin], np.inf) <= 1e-7 * max(1.0, np.linalg.norm(b[fin], np.inf))
    row = 0
    for c in cones:
        k = tri(c[1]) if c[0] == PSD else (3 if c[0] in (POW, EXP) else c[1])
        if c[0] == PSD:
            Ns = c[1]
            S, Z = np.zeros((Ns, Ns)), np.zeros((Ns, Ns))
            for cc in range(Ns):
                for r in range(cc + 1):
                    f = 1.0 if r == cc else 1.0 / SQ2
                    S[r, cc] = S[cc, r] = s[row + triu_index(r, cc)] * f
                    Z[r, cc] = Z[cc, r] = z[row + triu_index(r, cc)] * f
            assert np.linalg.eigvalsh(S).min() >= -1e-7 * max(1.0, np.linalg.norm(S))
            if complete_dual:
                assert np.linalg.eigvalsh(Z).min() >= -1e-7 * max(1.0, np.linalg.norm(Z))
                assert abs(s[row:row + k] @ z[row:row + k]) <= 1e-5 * max(1.0, np.linalg.norm(Z))
        row += k
    return t, x, s, z


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("complete_dual", [True, False])
@pytest.mark.parametrize("merge", MERGES)
def test_sdp_chordal_equivalent_through_oracle(hip, oracle, compact, complete_dual, merge):
    P, q, A, b, cones = sdp_chordal_data()
    # (parent_child merges the side-6 cone's cliques back into one: then nothing is decomposed, as in the reference)
    t, *_ = _check_equivalent(hip, oracle, P, q, A, b, cones, complete_dual, may_stay=merge == "parent_child",
                              chordal_decomposition_enable=1, chordal_decomposition_compact=int(compact),
                              chordal_decomposition_merge_method=merge)
    assert t.active or merge == "parent_child"


@pytest.mark.parametrize("compact", [True, False])
def test_banded_sdp_equivalent_through_oracle(hip, oracle, compact):
    P, q, A, b, cones = mask_sdp(banded(12, 2), 12, seed=5)
    t, *_ = _check_equivalent(hip, oracle, P, q, A, b, cones, True, chordal_decomposition_enable=1,
                              chordal_decomposition_compact=int(compact))
    assert t.npatterns == 1 and t.final_added >= 1


@pytest.mark.parametrize("compact", [True, False])
def test_presolve_in_front_of_a_decomposed_cone(hip, oracle, compact):
    """an infinite-bound NN row ahead of a decomposable PSD cone: the chordal analysis of the presolved problem"""
    P, q, A, b, cones = mask_sdp(banded(10, 2), 10, seed=2, extra_nn=True)
    plain = (P, q, A[1:], b[1:], [(NN, 1)] + cones[1:])
    t, x, s, z = _check_equivalent(hip, oracle, P, q, A, b, cones, True, ref_problem=plain, presolve_enable=1,
                                   chordal_decomposition_enable=1, chordal_decomposition_compact=int(compact))
    assert t.m_reduced == t.m - 1 and t.npatterns == 1
    (p,) = t.patterns()
    assert p["row_orig"] == 2 and p["row_pre"] == 1
    assert s[0] == 1e20 and z[0] == 0.0


# ---- the spill audit of problem_transform.hip --------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_problem_transform_kernels_do_not_spill():
    res = _resources("problem_transform.hip")
    assert "k_transform_reverse" in " ".join(res), sorted(res)
    for name, r in res.items():
        assert r.get("ScratchSize", 0) == 0, (name, r)
        assert r.get("SGPRs Spill", 0) == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
