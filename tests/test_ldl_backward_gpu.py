"""-m gpu: the LDL' factorisation and the substitutions of the handles (bundle_factor.hip, bundle_solve.hip, bundle_ir.hip,
bundle_gstep.hip, snode.hip, snode_g.hip) held entry by entry to the backward-error bounds of tests/ldl_ref.py
(tests/test_ldl_ref_host.py checks those on the CPU):

    factor   the handle's own L^, D^ against the K it was given: |K - L^ D^ L^'|_ij <= (c_ij + 2) u T_ij at every stored
             position, two refactors at different values per case
    solve    the handle's unrefined x^ against its own L^, D^: |b - L^ D^ L^' x^|_i <= (rmax + cmax + 4) u t_i per row
             (full-length sweeps), the visible rows of the same with the hidden components re-solved (fused launches on
             handles with sparse second-order cones), three right-hand sides, two of them over eight decades

No flat tolerance, no oracle: a lost, doubled or misplaced term shows as soon as it exceeds about 1e-15 of the absolute
term sum of its own entry.  Every case builds its handle as the existing test of that path does, asserts by that test's
counter that the path ran and that no pivot was regularised, and prints its worst ratio before it asserts (pytest -s).
Shapes: the smallest the path's counter accepts (random_qp(3000, 6000, band=30) where the existing tests take
(20000, 40000, band=50): 15 chain supernodes up to 263 wide, a top of 1486 rows on 784 levels; cliques of 29 and 30 where
they take 40).  batched_socp(129, 4000, 2) stays: 512 threads are chosen by the LDS a bundle of 6000 nodes needs.
Left out: handles whose PSD cones write Hs straight into the factor storage (their K is not in the value store); the
chordal SDPs are factored through the L1 handle on the KKT handle's values, as their existing tests do, and the tile
cases on the KKT handle's own factor as well (hs_direct_refactors == 0 asserted: its K is in the value store).  Of the
existing tests' variants only banded_qp_graph of the persistent sweeps (a replay of the same launches) has no case here.

Paths that multiply by an explicitly inverted block instead of substituting (read from the kernels, not from their ratios):
k_topblk_build / k_topblk_step (bundle_solve.hip: T_b = (I + L_bb)^-1 per 128 rows of a tall top; cases sweep-*-tall_top)
and the one-pass matrices G = [I; L_B] T^-1 of snode_g.hip (k_snode_ginv, k_snode_gfwd / gbwd / gsweep; cases snode-g-*,
snode-persistent*, snode-per_level, pair-banded_qp).  The substitution bound is not derived for them; they stay below 1
on every fixture (worst 0.53, late-iterate scaling through the persistent sweeps), so they are left on the derived bound and
no measured constant is in this module.  The factorisation has no such path: k_snode_rows, k_snode_panel and k_snode_panel2
substitute against the diagonal block.  k_snode_rows scales x_q first and multiplies by the staged d_q L_jq (two roundings per
term); k_snode_panel and k_snode_panel2 carry the UNSCALED u_ik = L_ik D_k through a column, so a term of T holds three
roundings where ldl_ref.py counts two -- (c - 1) + 3 = c + 2, the constant as it stands.
The tall top has no counter: _tall_top restates the selection rule of symbolic.cpp (at least 4 blocks of 128 top rows, 256
levels, three blocks per level saved) from n_levels, N - NF and supernodes(), and has to follow that rule if it changes.

Worst ratio of error to bound on one MI355X, per family (120 cases, 50 s in all; the slowest, a fuzz matrix, 2 s):
    factor   bundle (LDS, flat, run-coded, plain records) 0.26 - 0.36    folded top 0.35 - 0.40    grouped fold 0.36 - 0.38
             general fill 0.30 - 0.38, dense front (bound doubled) 0.17    chain supernodes, every switch 0.32 - 0.47
             wide and narrow tiles, L1 handle 0.25 - 0.29, the KKT handle's own factor 0.29    structure fuzz 0.35 - 0.39
    solve    flat / row bundle sweeps 0.0015 - 0.0043, late iterate 0.24 - 0.35    folded and grouped tops 0.0002 - 0.0018
             block-by-block supernode sweeps 0.003 - 0.006    one-pass matrices 0.003, late iterate 0.29 - 0.53
             tall top (inverted blocks) 0.0035    fused k_bundle_irs / k_bundle_ir / k_gstep_solve 0.0007 - 0.0020, pairs 0.0035
(the factor's worst entries have c = 1 or 2: two or three roundings of the three or four allowed.)

Wrong kernels, each a one-line arithmetic change that stays in bounds, built in a scratch copy and run once on the MI355X
against this module and against the existing tests of the same path (the module then had 108 cases; the update tiles were
run once more against the factor test as it stands, 72 cases):
    * k_bundle_factor_runs, a reduction run skipping products below 1e-9 of its target: bundle-bs200-runs, bundle-bs1100-runs,
      fold-arrow, fold-arrow_late, general-chunked_row, gfold-off, gfold-three_launches(_late) fail (ratios 6e3 - 1.3e5; the
      blocks of 63 - 65 and 20 have no such product and pass); tests/test_factor_runs_gpu.py, test_c3_portfolio_socp,
      test_c3_several_dense_top_rows, test_fused_solve_iterates_on_chip, test_ir_fixed_one_round: 19 passed
    * k_bundle_sweep_flat, the forward sweep skipping contributions below 1e-10 of the row's running value: sweep-flat-chordal_sdp,
      snode-g-chordal_sdp, snode-g-wide_psd, snode-blocks-chordal_sdp, snode-blocks-wide_psd, snode-no_lds_rows-chordal_sdp fail
      (1.7 - 160; the banded QPs have no such contribution); test_bundle_sweeps_entry_parallel_against_row_form[band20,
      band50_late, chordal_sdp], test_c2_random_qp, test_c2_solve_sequence_as_hipgraph: 6 passed
    * snode_tiles, the staged operand d_k L_jk taken as 0 where |L_jk| < 1e-10: all 50 cases with chain supernodes fail
      (snode-*, the sixteen tile cases among them, fuzz-*, general-dense_front_2300, general-quasidef_400_300; ratios up to
      1.4e14 = 1 / ((c + 2) u): entries whose terms are all that small are lost whole); test_chain_supernodes_factor_parity, test_ancestor_updates_assembled_per_
      target_column, test_ldl_structure_fuzz_with_supernodes, test_ldl_supernode_trees, test_c2_random_qp,
      test_run_coded_factorisation_...[irregular]: 23 passed
    * k_gstep_factor skipping update records below 1e-9 of their target: gfold-step, gfold-step_late fail (1.1e4, 1.4e5);
      test_grouped_fold_ragged_forest[False], test_full_scale_parity_c4_share_grouped_fold, test_update_scaled_enqueue_matches_
      the_two_calls pass, test_grouped_fold_ragged_forest[True] fails (3e-6 at its unrefined solve held to 1e-8)
    * bundle_sweep_flat_ahead (the fused kernels' backward sweep) skipping contributions below 1e-10 of the running value: nothing
      fails, here or there -- the arrow columns have three entries and no contribution that small; below 1e-6: fused-irs (all
      four), fused-ir, fused-ir_1024, fused-ir_grouped, pair-arrow fail (1.4e5 - 1.5e6), and so do 5 of 24 existing cases
      (test_fused_solve_iterates_on_chip by its refinement round count, 2 for 1; one unrefined case at 2.5e-7)"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import ldl_ref as R
from tests import problems
from tests.test_gpu_parity import _arrow_of_bands, _rand_quasidef

pytestmark = pytest.mark.gpu


# ---- fixtures ----------------------------------------------------------------------------------------------------------
def _banded_qp(late=False):
    return problems.random_qp(3000, 6000, band=30, seed=1, late=late)


def _ragged_forest(late=False):
    """tests/test_gpu_parity.py: test_grouped_fold_ragged_forest"""
    parts = [problems.portfolio_socp(2 + (i % 3), 120 + 40 * (i % 4), seed=100 + i, late=late) for i in range(14)]
    parts.append(problems.portfolio_socp(1, 20, seed=300, late=late))
    return problems.blockdiag(parts)


def _three_row_top():
    """tests/test_gpu_parity.py: test_c3_several_dense_top_rows"""
    pr = problems.portfolio_socp(12, 600, seed=21)
    n, m = pr["n"], pr["m"]
    rng = np.random.default_rng(2)
    A = sp.csc_matrix((pr["A"][2], pr["A"][1], pr["A"][0]), shape=(m, n))
    A2 = sp.vstack([A, sp.csc_matrix(rng.uniform(0.5, 1.5, (2, n)))], format="csc")
    A2.sort_indices()
    return dict(n=n, m=m + 2, P=pr["P"], A=problems._csc(A2), cones=list(pr["cones"]) + [(0, 2)],
                s=np.concatenate([pr["s"], np.zeros(2)]), z=np.concatenate([pr["z"], np.zeros(2)]))


def _dense_front():
    """tests/test_gpu_parity.py: test_ldl_dense_front_beyond_lds"""
    rng = np.random.default_rng(3)
    n1, n2 = 2200, 100
    M = rng.standard_normal((n1, 40))
    A = rng.standard_normal((n2, n1))
    K = np.block([[M @ M.T + n1 * np.eye(n1), A.T], [A, -(n2 * np.eye(n2))]])
    K = sp.triu(sp.csc_matrix(K), format="csc")
    K.sort_indices()
    return K, np.array([1] * n1 + [-1] * n2, dtype=np.int8)


def _structure_fuzz(seed):
    """tests/test_gpu_parity.py: test_ldl_structure_fuzz_with_supernodes"""
    rng = np.random.default_rng(1000 + seed)
    n1 = int(rng.integers(300, 1500))
    n2 = int(rng.integers(300, 2500))
    rs = np.random.RandomState(seed)
    band = int(rng.integers(2, 40))
    diags = [rng.standard_normal(n1 - k) * 0.3 for k in range(1, band)]
    H = sp.diags(diags, list(range(1, band)), shape=(n1, n1), format="csc")
    H = H + H.T + sp.diags(rng.uniform(2.0, 4.0, n1) * band)
    B = sp.random(n2, n1, density=float(rng.uniform(0.5, 4.0)) / n1, random_state=rs, format="csc")
    nblk = int(rng.integers(0, 4))
    G = sp.diags(rng.uniform(0.5, 2.0, n2)).tolil()
    pos = 0
    for _ in range(nblk):
        w = int(rng.integers(20, 180))
        if pos + w > n2:
            break
        M = rng.standard_normal((w, w))
        G[pos:pos + w, pos:pos + w] = M @ M.T / w + np.eye(w)
        pos += w + int(rng.integers(0, 50))
    K = sp.triu(sp.bmat([[H, B.T], [B, -G.tocsc()]], format="csc"), format="csc")
    K.sort_indices()
    return K, np.array([1] * n1 + [-1] * n2, dtype=np.int8)


def _kkt_handle(hip, pr, settings=None):
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    return hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"], settings=settings)


def _scalings(pr, it):
    """the two scaling points of tests/test_factor_runs_gpu.py: _walk"""
    return pr["s"] * (1.0 + 0.3 * it), pr["z"] / (1.0 + 0.2 * it)


def _rhs(N, rng, k):
    """right-hand side k of a case: the first plain, the others with entries spread over eight decades"""
    b = rng.standard_normal(N)
    return b if k == 0 else b * 10.0 ** rng.uniform(-4.0, 4.0, N)


# ---- the path each case must have taken, by the counters of the existing tests --------------------------------------------
def _runs(expect):
    return lambda hip, ks: int(hip.debug_counter(ks, "factor_run_kernel")) == expect


def _top_rows(k):
    return lambda hip, ks: ks.N - ks.NF == k and not ks.supernodes()


def _grouped(step, groups=True):
    return lambda hip, ks: (ks.work_model()["fold_groups"] >= 10) == groups and ks.step_kernels() == step


def _snodes(hip, ks):
    return len(ks.supernodes()) > 0


def _widest(w):
    return lambda hip, ks: max(len(c) for c in ks.supernodes()) > w


def _rows_of_B(k):
    def check(hip, ks):
        cnt = np.diff(ks.symbolic()[1])
        return max(int(cnt[c[-1]]) for c in ks.supernodes()) > k
    return check


def _assembled(hip, ks):
    """(the counter is the KKT handle's: the L1 handle built on its values is held to the structural part)"""
    return len(ks.supernodes()) > 1 and (not hasattr(ks, "nnzK") or hip.debug_counter(ks, "assembled_levels") > 0)


def _several(hip, ks):
    return len(ks.supernodes()) > 1


def _long_columns(hip, ks):
    return len(ks.supernodes()) > 1 and np.diff(ks.symbolic()[1]).max() > 300


def _long_row(hip, ks):
    return int(np.bincount(ks.symbolic()[2], minlength=ks.N).max()) > 16384  # (the B-chunk threshold)


# ---- factor cases ------------------------------------------------------------------------------------------------------
# name -> (kind, fixture, environment of the handle, path check).  kind "kkt": the KKT handle's own factor
# (debug_kkt_factors) against its value store + static regulariser; "l1_hs": the L1 handle on the values of a KKT handle
# with host-supplied Hs blocks, as tests/test_gpu_parity.py: test_chain_supernodes_factor_parity; "l1": an L1 handle on a
# matrix; "kkt_hs": the own factor of a KKT handle with host-supplied Hs blocks, the same point twice; "+dense": R in float64
# BLAS, the bound doubled (tests/ldl_ref.py) -- the dense front of order 2300 alone
FACTOR = {}
for _name, _mk, _env, _has in (("bs63", lambda: problems.portfolio_socp(3, 63, seed=3), {}, 0),
                               ("bs64", lambda: problems.portfolio_socp(3, 64, seed=3), {}, 1),
                               ("bs65", lambda: problems.portfolio_socp(3, 65, seed=3), {}, 1),
                               ("bs200", lambda: problems.portfolio_socp(4, 200, seed=3), {}, 1),
                               ("bs1100", lambda: problems.portfolio_socp(2, 1100, seed=3), {"CHIP_TARGET_WG": "0"}, 1),
                               ("bs20_min4", lambda: problems.portfolio_socp(3, 20, seed=3), {"CHIP_FACTOR_RUN_MIN": "4"}, 1)):
    FACTOR["bundle-%s-runs" % _name] = ("kkt", _mk, _env, _runs(_has))
    FACTOR["bundle-%s-records" % _name] = ("kkt", _mk, dict(_env, CHIP_NO_FACTOR_RUNS="1"), _runs(0))
FACTOR.update({
    "fold-arrow": ("kkt", lambda: problems.portfolio_socp(12, 300, seed=3), {}, _top_rows(1)),
    "fold-arrow_late": ("kkt", lambda: problems.portfolio_socp(12, 300, seed=3, late=True), {}, _top_rows(1)),
    "fold-three_row_top": ("kkt", _three_row_top, {}, _top_rows(3)),
    "gfold-step": ("kkt", _ragged_forest, {}, _grouped(3)),
    "gfold-step_late": ("kkt", lambda: _ragged_forest(True), {}, _grouped(3)),
    "gfold-three_launches": ("kkt", _ragged_forest, {"CHIP_NO_STEP_KERNEL": "1"}, _grouped(0)),
    "gfold-three_launches_late": ("kkt", lambda: _ragged_forest(True), {"CHIP_NO_STEP_KERNEL": "1"}, _grouped(0)),
    "gfold-off": ("kkt", _ragged_forest, {"CHIP_NO_GROUPFOLD": "1"}, _grouped(0, False)),
    "general-quasidef_30_20": ("l1", lambda: _rand_quasidef(np.random.default_rng(0), 30, 20, 0.1), {}, lambda hip, f: not f.supernodes()),  # (the column kernels alone)
    "general-quasidef_400_300": ("l1", lambda: _rand_quasidef(np.random.default_rng(1), 400, 300, 0.01), {}, _snodes),
    "general-dense_front_2300": ("l1+dense", _dense_front, {}, lambda hip, f: np.diff(f.symbolic()[1]).max() > 2048),
    "general-chunked_row": ("kkt", lambda: problems.portfolio_socp(40, 500, seed=9), {}, _long_row),
    "snode-banded_qp": ("kkt", _banded_qp, {}, _snodes),
    "snode-banded_qp_late": ("kkt", lambda: _banded_qp(True), {}, _snodes),
    "snode-chordal_sdp": ("l1_hs", lambda: problems.chordal_sdp(8, 20, 4, 8, 9, seed=5), {}, _snodes),
    "snode-wide_psd": ("l1_hs", lambda: problems.chordal_sdp(2, 29, 6, 1, 5, seed=7), {}, _widest(416)),
    "snode-asm-banded_qp": ("kkt", _banded_qp, {"CHIP_EXTEND_ASM_MIN": "2"}, _assembled),
    "snode-asm_off-banded_qp": ("kkt", _banded_qp, {"CHIP_NO_EXTEND_ASM": "1"}, _several),
    "snode-asm-chordal_sdp": ("l1_hs", lambda: problems.chordal_sdp(8, 20, 4, 8, 9, seed=5), {"CHIP_EXTEND_ASM_MIN": "2"}, _assembled),
    "snode-asm_off-chordal_sdp": ("l1_hs", lambda: problems.chordal_sdp(8, 20, 4, 8, 9, seed=5), {"CHIP_NO_EXTEND_ASM": "1"}, _several),
    "snode-asm-long_columns": ("l1_hs", lambda: problems.chordal_sdp(4, 26, 8, 2, 9, seed=3),
                               {"CHIP_EXTEND_ASM_MIN": "2", "CHIP_SN_ASM_CAP": "100"},
                               lambda hip, ks: _assembled(hip, ks) and _long_columns(hip, ks)),
    "snode-asm_off-long_columns": ("l1_hs", lambda: problems.chordal_sdp(4, 26, 8, 2, 9, seed=3),
                                   {"CHIP_NO_EXTEND_ASM": "1", "CHIP_SN_ASM_CAP": "100"}, _long_columns),
})
for _form in ("CHIP_NO_SNODE_PANEL", "CHIP_NO_PANEL_MFMA", "CHIP_NO_PANEL_DIAG_MFMA", "CHIP_SN_PANEL_SLOTS", "CHIP_NO_PANEL_OVERLAP",
              "CHIP_NO_PANEL_OVERLAP+CHIP_SN_PANEL_SLOTS", "CHIP_NO_PANEL_UNIFORM", "CHIP_NO_FACTOR_OVERLAP"):
    _env = {k: "1" for k in _form.split("+")}
    FACTOR["snode-%s-banded_qp" % _form] = ("kkt", _banded_qp, _env, _snodes)
    FACTOR["snode-%s-chordal_sdp" % _form] = ("l1_hs", lambda: problems.chordal_sdp(8, 20, 4, 8, 9, seed=5), _env, _snodes)
for _emit in ("atomics", "assembled"):
    for _waves in ("4", "8"):
        for _form in ("wide", "narrow"):
            _env = {"CHIP_SN_WIDE_MIN_COUNT": "1", "CHIP_SN_WIDE_WAVES": _waves}
            _env.update({"CHIP_NO_EXTEND_ASM": "1"} if _emit == "atomics" else {"CHIP_EXTEND_ASM_MIN": "2"})
            if _form == "narrow":
                _env["CHIP_NO_SN_WIDE"] = "1"
            # (two supernodes of 461 columns with 284 rows of B: more than one wide column block, the last one narrower
            # than 256, row groups that end inside a tile; tests/test_gpu_parity.py takes four cliques of 40, 820 columns --
            # 29 s per refactor for the longdouble residual against 1.6 s here)
            FACTOR["snode-tiles_%s_%s_%s" % (_form, _emit, _waves)] = ("l1_hs", lambda: problems.chordal_sdp(2, 30, 23, 1, 5, seed=11),
                                                                      _env, _rows_of_B(256))
            FACTOR["snode-tileskkt_%s_%s_%s" % (_form, _emit, _waves)] = ("kkt_hs", lambda: problems.chordal_sdp(2, 30, 23, 1, 5, seed=11),
                                                                         _env, _rows_of_B(256))


def _trees(seed):
    """tests/test_gpu_parity.py: test_ldl_supernode_trees"""
    rng = np.random.default_rng(77 + seed)
    K, ds, _ = _arrow_of_bands(rng, int(rng.integers(3, 6)), int(rng.integers(40, 400)))
    return K, ds


for _seed in range(3):
    FACTOR["fuzz-structure_%d" % _seed] = ("l1", lambda s=_seed: _structure_fuzz(s), {}, _snodes)
    FACTOR["fuzz-trees_%d" % _seed] = ("l1", lambda s=_seed: _trees(s), {}, lambda hip, f: len(f.supernodes()) >= 2)


def _report(label, it, fc, Lx, D):
    i, j = fc["at"]
    print("%s refactor %d: worst ratio %.3f at (%d, %d) [c %d, T %.3e, R %.3e]; %d positions, max|L| %.2e, max|D| / min|D| %.1e"
          % (label, it, fc["worst"], i, j, fc["c"][np.argmax(fc["ratio"])], fc["T"][np.argmax(fc["ratio"])], fc["R"][np.argmax(fc["ratio"])],
             len(fc["ratio"]), np.abs(Lx).max(initial=0.0), np.abs(D).max() / np.abs(D).min()))


def _second_values(N, colptr, rowval, nzval):
    """the values of an L1 handle's second refactor: 0.9 K + 0.4 diag(K), quasidefinite like K"""
    v = 0.9 * np.asarray(nzval, dtype=np.float64)
    diag = np.asarray(rowval, dtype=np.int64) == np.repeat(np.arange(N), np.diff(np.asarray(colptr, dtype=np.int64)))
    v[diag] = 1.3 * np.asarray(nzval, dtype=np.float64)[diag]
    return v


def _l1_refactors(hip, f, N, colptr, rowval, values, dense, label):
    """the L1 handle's factor of every set of values against those values; -> worst ratios"""
    worst = []
    for it, v in enumerate(values):
        f.set_values(v)
        assert f.refactor()
        assert f.linear_solver_info().regularize_count == 0, label
        Lp, Li, Lx, D, _ = f.factors()
        fc = R.factor_check(N, Lp, Li, Lx, D, R.lower_permuted(N, colptr, rowval, v, f.perm), dense=dense)
        _report(label, it, fc, Lx, D)
        worst.append(fc["worst"])
    return worst


@pytest.mark.parametrize("case", sorted(FACTOR))
def test_factor_within_componentwise_bound(hip, case, monkeypatch):
    kind, mk, env, path = FACTOR[case]
    dense = kind.endswith("+dense")
    kind = kind.split("+")[0]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read when a handle is created)
    if kind == "l1":
        K, ds = mk()
        N = K.shape[0]
        Kc = hip.CscMatrix.from_scipy(K)
        f = hip.HipDirectLDLSolver(Kc, ds)
        assert path(hip, f), case
        print("%s: N %d, %d chain supernodes" % (case, N, len(f.supernodes())))
        worst = _l1_refactors(hip, f, N, Kc.colptr, Kc.rowval, [np.array(Kc.nzval), _second_values(N, Kc.colptr, Kc.rowval, Kc.nzval)], dense, case)
    elif kind == "l1_hs":
        pr = mk()
        ks = _kkt_handle(hip, pr)
        assert path(hip, ks), case
        assert ks.update_scaling(pr["s"], pr["z"]) and ks.update(pr["hsblocks"])
        K = ks.kkt_matrix()
        values = [np.array(ks.values()), _second_values(ks.N, K.colptr, K.rowval, ks.values())]
        f = hip.HipDirectLDLSolver(hip.CscMatrix(ks.N, ks.N, K.colptr, K.rowval, values[0]), ks.maps()["dsigns"], hip.Settings.default(), perm=ks.perm)
        assert len(f.supernodes()) > 0 and path(hip, f), case
        print("%s: N %d, chain supernodes (columns, rows of B): %s" % (case, ks.N, [(len(c), int(np.diff(f.symbolic()[1])[c[-1]])) for c in f.supernodes()]))
        worst = _l1_refactors(hip, f, ks.N, K.colptr, K.rowval, values, dense, case)
    else:
        pr = mk()
        ks = _kkt_handle(hip, pr)
        assert path(hip, ks), case
        _, Lp, Li, _ = ks.symbolic()
        worst = []
        for it in range(2):
            if kind == "kkt_hs":  # (host-supplied Hs blocks belong to the problem's own (s, z): the same point twice)
                assert ks.update_scaling(pr["s"], pr["z"]) and ks.update(pr["hsblocks"])
                assert hip.debug_counter(ks, "hs_direct_refactors") == 0, case  # (K is in the value store)
            else:
                s_, z_ = _scalings(pr, it)
                assert ks.update_scaling(s_, z_) and ks.update()
            assert ks.linear_solver_info().regularize_count == 0, case
            Lx, D = hip.debug_kkt_factors(ks)
            fc = R.factor_check(ks.N, Lp, Li, Lx, D, R.kkt_lower(ks), dense=dense)
            _report(case, it, fc, Lx, D)
            worst.append(fc["worst"])
        assert path(hip, ks), case
    assert max(worst) < 1.0, (case, worst)


# ---- solve cases -------------------------------------------------------------------------------------------------------
def _counter(name, test):
    return lambda hip, ks: test(hip.debug_counter(ks, name))


def _g_levels(all_of_them):
    def check(hip, ks):
        ng, nl = hip.debug_counter(ks, "g_levels"), hip.debug_counter(ks, "sn_levels")
        return ng >= 1 and (ng == nl if all_of_them else ng < nl)
    return check


def _persistent(hip, ks):
    runs, lv = hip.debug_counter(ks, "gsweep_runs"), hip.debug_counter(ks, "gsweep_levels")
    return runs >= 2 and lv >= 2 * runs and hip.debug_counter(ks, "gsweep_launches") >= runs


def _tall_top(hip, ks):
    """symbolic.cpp: the blocked substitution of the top is taken without supernodes from 4 blocks of 128 rows and 256
    levels on, when it saves two thirds of the dependent steps"""
    ntop, nlev = ks.N - ks.NF, ks.linear_solver_info().n_levels
    return not ks.supernodes() and ntop >= 4 * 128 and nlev >= 256 and 3 * ((ntop + 127) // 128) < nlev


def _irs(desc=True, shared=True):
    def check(hip, ks):
        nb = ks.work_model()["n_bundles"]
        return (ks.step_kernels() & 4 and nb > 0 and hip.debug_counter(ks, "irs_desc_bundles") == (nb if desc else 0)
                and hip.debug_counter(ks, "pattern_shared_bundles") == (nb if shared else 0))
    return check


def _wide(threads, groups):
    def check(hip, ks):
        wm = ks.work_model()
        return wm["fused_threads"] == threads and wm["fold_groups"] == groups and ks.step_kernels() == 0
    return check


_SDP = lambda: problems.chordal_sdp(8, 20, 4, 8, 9, seed=5)
_ARROW = lambda: problems.portfolio_socp(6, 700, seed=11)
# name -> (how, fixture, environment, path check).  how: "full" solve_full on the KKT handle, "l1" solve of the L1 handle on
# the KKT handle's matrix, values and permutation, "fused" setrhs + solve (the visible components), "pair" both results of
# one solve2_dev_enqueue
SOLVE = {
    "sweep-flat-band20": ("full", lambda: problems.random_qp(3000, 6000, band=20, seed=1), {}, _snodes),
    "sweep-rows-band20": ("full", lambda: problems.random_qp(3000, 6000, band=20, seed=1), {"CHIP_NO_BUNDLE_FLAT_SWEEP": "1"}, _snodes),
    "sweep-flat-banded_qp_late": ("full", lambda: _banded_qp(True), {}, _snodes),
    "sweep-rows-banded_qp_late": ("full", lambda: _banded_qp(True), {"CHIP_NO_BUNDLE_FLAT_SWEEP": "1"}, _snodes),
    "sweep-flat-chordal_sdp": ("full", _SDP, {}, _snodes),
    "sweep-rows-chordal_sdp": ("full", _SDP, {"CHIP_NO_BUNDLE_FLAT_SWEEP": "1"}, _snodes),
    "sweep-flat-tall_top": ("full", _banded_qp, {"CHIP_NO_SNODE": "1"}, _tall_top),
    "sweep-rows-tall_top": ("full", _banded_qp, {"CHIP_NO_SNODE": "1", "CHIP_NO_BUNDLE_FLAT_SWEEP": "1"}, _tall_top),
    "sweep-level_top": ("full", _banded_qp, {"CHIP_NO_SNODE": "1", "CHIP_NO_TOPBLK": "1"}, lambda hip, ks: not ks.supernodes() and ks.NF < ks.N),
    "top-fold-arrow": ("full", lambda: problems.portfolio_socp(12, 300, seed=3), {}, _top_rows(1)),
    "top-fold-arrow_late": ("full", lambda: problems.portfolio_socp(12, 300, seed=3, late=True), {}, _top_rows(1)),
    "top-fold-three_rows": ("full", _three_row_top, {}, _top_rows(3)),
    "top-gfold": ("full", _ragged_forest, {}, _grouped(3)),
    "top-gfold_late": ("full", lambda: _ragged_forest(True), {}, _grouped(3)),
    "snode-g-banded_qp": ("full", _banded_qp, {}, _g_levels(True)),
    "snode-g-banded_qp_late": ("full", lambda: _banded_qp(True), {}, _g_levels(True)),
    "snode-g-chordal_sdp": ("full", _SDP, {}, _g_levels(True)),
    "snode-g-wide_psd": ("full", lambda: problems.chordal_sdp(2, 29, 6, 1, 5, seed=7), {}, lambda hip, ks: _widest(416)(hip, ks) and hip.debug_counter(ks, "g_levels") >= 1),
    "snode-g-mixed_widths": ("full", _banded_qp, {"CHIP_SN_G_MAXW": "250"}, _g_levels(False)),
    "snode-g-no_merge": ("full", _banded_qp, {"CHIP_NO_SWEEP_MERGE": "1"}, _g_levels(True)),
    "snode-g-l1": ("l1", _banded_qp, {}, _snodes),
    "snode-blocks-banded_qp": ("full", _banded_qp, {"CHIP_NO_SNODE_G": "1"}, _counter("g_levels", lambda c: c == 0)),
    "snode-blocks-banded_qp_late": ("full", lambda: _banded_qp(True), {"CHIP_NO_SNODE_G": "1"}, _counter("g_levels", lambda c: c == 0)),
    "snode-blocks-chordal_sdp": ("full", _SDP, {"CHIP_NO_SNODE_G": "1"}, _counter("g_levels", lambda c: c == 0)),
    "snode-blocks-wide_psd": ("full", lambda: problems.chordal_sdp(2, 29, 6, 1, 5, seed=7), {"CHIP_NO_SNODE_G": "1"}, _widest(416)),
    "snode-blocks-l1": ("l1", _banded_qp, {"CHIP_NO_SNODE_G": "1"}, _snodes),
    "snode-no_lds_rows-banded_qp": ("full", _banded_qp, {"CHIP_SN_XB_CAP": "16", "CHIP_NO_SNODE_G": "1"}, _snodes),
    "snode-no_lds_rows-chordal_sdp": ("full", _SDP, {"CHIP_SN_XB_CAP": "16", "CHIP_NO_SNODE_G": "1"}, _snodes),
    "snode-persistent": ("full", _banded_qp, {}, _persistent),
    "snode-persistent_late": ("full", lambda: _banded_qp(True), {}, _persistent),
    "snode-persistent_grid1": ("full", _banded_qp, {"CHIP_GSWEEP_GRID": "1"}, _persistent),
    "snode-persistent_grid3": ("full", _banded_qp, {"CHIP_GSWEEP_GRID": "3"}, _persistent),
    "snode-persistent_narrow_grid2": ("full", lambda: problems.random_qp(12000, 24000, band=30, seed=4), {"CHIP_GSWEEP_GRID": "2"}, _persistent),
    "snode-persistent_mixed": ("full", _banded_qp, {"CHIP_SN_G_MAXW": "250"}, _persistent),
    "snode-per_level": ("full", _banded_qp, {"CHIP_NO_SWEEP_PERSIST": "1"}, _counter("gsweep_launches", lambda c: c == 0)),
    "fused-irs": ("fused", _ARROW, {}, _irs()),
    "fused-irs_flags0": ("fused", _ARROW, {"CHIP_IRS_FLAGS": "0"}, _irs()),
    "fused-irs_chained": ("fused", _ARROW, {"CHIP_IRS_FLAGS": "7"}, _irs(desc=False)),
    "fused-irs_own_patterns": ("fused", _ARROW, {"CHIP_NO_SHARED_PATTERN": "1"}, _irs(shared=False)),
    "fused-ir": ("fused", _ARROW, {"CHIP_NO_IR_SF": "1"}, lambda hip, ks: not ks.step_kernels() & 4 and ks.work_model()["fused_threads"] > 0),
    "fused-ir_1024": ("fused", lambda: problems.batched_socp(4, 2000, 2, seed=100), {"CHIP_NO_GROUPFOLD": "1"}, _wide(1024, 0)),
    "fused-ir_512_grouped": ("fused", lambda: problems.batched_socp(129, 4000, 2, seed=100), {}, _wide(512, 129)),
    "fused-gstep": ("fused", _ragged_forest, {}, _grouped(3)),
    "fused-gstep_late": ("fused", lambda: _ragged_forest(True), {}, _grouped(3)),
    "fused-ir_grouped": ("fused", _ragged_forest, {"CHIP_NO_STEP_KERNEL": "1"}, _grouped(0)),
    "pair-arrow": ("pair", lambda: problems.portfolio_socp(12, 300, seed=3), {}, _top_rows(1)),
    "pair-forest": ("pair", _ragged_forest, {}, _grouped(3)),
    "pair-banded_qp": ("pair", _banded_qp, {}, _snodes),
}


def _visible_check(ks, factor, vis, perm, iperm, b, got):
    """the n + m components `got` a fused launch returns for b = (rhsx, rhsz), zeros in the hidden rows"""
    n, m, N = ks.n, ks.m, ks.N
    bp = np.concatenate([b, np.zeros(N - n - m)])[perm]
    if vis is None:
        return R.solve_check(N, *factor, bp, got[perm])
    xp = np.zeros(N)
    xp[iperm[:n + m]] = got
    return vis.check(bp, xp[vis.V])


@pytest.mark.parametrize("case", sorted(SOLVE))
def test_unrefined_solve_within_componentwise_bound(hip, case, monkeypatch):
    how, mk, env, path = SOLVE[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read when a handle is created)
    pr = mk()
    hs = pr.get("hsblocks")
    st = hip.Settings.default(iterative_refinement_enable=0)
    ks = _kkt_handle(hip, pr, st)
    n, m, N = ks.n, ks.m, ks.N
    rng = np.random.default_rng(31)
    worst = []
    for it in range(2 if hs is None else 1):
        s_, z_ = _scalings(pr, it)
        assert ks.update_scaling(s_, z_) and ks.update(hs)
        assert ks.linear_solver_info().regularize_count == 0, case
        if how == "l1":
            K = ks.kkt_matrix()
            f = hip.HipDirectLDLSolver(hip.CscMatrix(N, N, K.colptr, K.rowval, ks.values()), ks.maps()["dsigns"], hip.Settings.default(), perm=ks.perm)
            assert f.refactor() and f.linear_solver_info().regularize_count == 0 and path(hip, f), case
            Lp, Li, Lx, D, _ = f.factors()
            perm = f.perm  # (the L1 handle renumbers the permutation it is given once more)
        else:
            _, Lp, Li, _ = ks.symbolic()
            Lx, D = hip.debug_kkt_factors(ks)
            perm = ks.perm
        iperm = np.empty(N, dtype=np.int64)
        iperm[perm] = np.arange(N)
        factor = (Lp, Li, Lx, D)
        # (one M = L^ D^ L^' and one |M_HH^-1| per refactor for the fused launches of handles with hidden rows)
        vis = R.VisibleSolveCheck(N, *factor, iperm[n + m:]) if how in ("fused", "pair") and N > n + m else None
        for k in range(3):
            if how in ("full", "l1"):
                b = _rhs(N, rng, k)
                if how == "full":
                    ok, x = ks.solve_full(b)
                    assert ok
                else:
                    x = np.zeros(N)
                    f.solve(None, x, b)
                checks = [R.solve_check(N, *factor, b[perm], x[perm])]
            elif how == "fused":
                b = _rhs(n + m, rng, k)
                ks.setrhs(b[:n], b[n:])
                x, z = np.zeros(n), np.zeros(m)
                assert ks.solve(x, z)
                checks = [_visible_check(ks, factor, vis, perm, iperm, b, np.concatenate([x, z]))]
            else:
                rhs = [_rhs(n + m, rng, k), _rhs(n + m, rng, (k + 1) % 3)]
                dev = [(hip.DeviceArray(b[:n]), hip.DeviceArray(b[n:]), hip.DeviceArray(n + m)) for b in rhs]
                (ra, za, la), (rb, zb, lb) = dev
                ks.solve2_dev_enqueue(ra.ptr, za.ptr, la.ptr, la.ptr + 8 * n, rb.ptr, zb.ptr, lb.ptr, lb.ptr + 8 * n)
                uok, sok = ks.collect()
                assert uok and sok == [True, True]
                checks = [_visible_check(ks, factor, vis, perm, iperm, b, out.numpy()) for b, (_, _, out) in zip(rhs, dev)]
            for c in checks:
                print("%s refactor %d rhs %d: worst ratio %.4f at row %d (N %d, hidden %d)" % (case, it, k, c["worst"], c["at"], N, N - n - m))
                worst.append(c["worst"])
        assert ks.linear_solver_info().last_ir_iterations == 0, case
    assert path(hip, ks), case  # (after the solves: the counters of the persistent sweeps count launches)
    if how in ("fused", "pair"):
        assert ks.fused_fallbacks() == 0, case
    assert max(worst) < 1.0, (case, worst)
