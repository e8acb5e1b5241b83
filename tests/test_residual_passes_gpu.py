"""The residual pass of the single solver (clarabel.rs_amd/csrc/kktsystem.cpp residuals_pass) on the MI355X through the
public HipKKTSolver + HipKKTSystem.residuals_update(..., norms=True) and vec_norms, against the references of
tests/spmv_ref.py (tests/test_spmv_ref_host.py checks those on the CPU), on both sides of every row length and vector
size at which the pass changes its code path.  No factorisation: handles are created and residuals_update is called.

Paths (WG = 256, wavefront 64):

    row length 32 | 33        thread per row | wavefront per row (kktsystem.cpp:50 `len > T_MAX`)
    row length 0              a thread row that must still write aux or 0 (kktsystem.cpp:53; bundle_solve.hip:384-389)
    192 | 193, 256 | 257,     wavefront row: tail loop only | one unrolled trip | unrolled trip + tail; 64 | 65 a second
    448 | 449                 trip of the tail (bundle_solve.hip:426 `t + 192 < e`, :434)
    16384 | 16385             wavefront row | k_gather_Bprep + chunks of 4096 added by atomicAdd (kktsystem.cpp:43
                              `len > B_MIN`, :45-48; bundle_solve.hip:366, :415); 16385 ends in a chunk of ONE entry
    chunk 4096 | 1023, 1119   unrolled trips only (row 20480) | `t += WG` tail with lanes beyond the end (rows 21503 and
                              the symmetric row 0 of P, 21599) (bundle_solve.hip:404 `t + 3 * WG < ce`, :412)
    thread slab behind off8   21598 thread rows of the symmetric P (85 workgroups rounded to 88) behind 6 chunk blocks and
                              one wavefront block, off8 = 8: the XCD map `(lb0 & 7) * per + (lb0 >> 3)`
                              (bundle_solve.hip:379-382, :790-793).  Arow of the columns layout is 21600 thread rows with
                              off8 = 0, its Acol 2 thread rows behind 11 chunk blocks and one wavefront block, off8 = 16
    store_row<SPMV>           aux == nullptr, alpha = -1 (A'z) | aux = s, alpha = 1 (A x + s) | alpha = 1, no aux (P x)
                              (bundle_solve.hip:239; kktsystem.cpp:409, :413, :414)
    Psym                      an off-diagonal entry serves two rows; an empty row and column (kktsystem.cpp:174-193)
    k_multi_dot_*             n = 1, 255 | 256 | 257: one block | two; 131072 | 131073: the 512-block cap, a second trip
                              of stride nb * WG (algebra.hip:295-300, :308-310)
    stream_grid               524288 | 524289: the 2048-block cap, a second grid-stride trip of k_lin3 and k_waxpby
                              (dev_common.hpp:64-67; algebra.hip:271, :317)

Layouts, one handle each for the whole module: (rows) spmv_ref.rows_problem -- every row length above in A, the
workgroup, wavefront and empty rows of the symmetric P; its row 0 has n - 1 = 21599 entries, not n, because row and
column 7777 are empty; (cols) spmv_ref.cols_problem -- every class in A', P without entries; (vector, n) P diagonal, A one
entry per row, n = m.  A handle is created with one set of integer values; every test loads its own values through
update_data first, so no test depends on another.  Before every call the five output arrays hold NaN: a row that the pass
does not write shows.

Both families of spmv_ref on every layout: the integer family must come back bit for bit (vectors, dots, rtau, norms),
the wide family within (L + 4) 2^-53 fsum|terms| per entry; no flat tolerance.  Every test prints the largest ratio of
error to bound per output before it asserts (pytest -s).

Largest ratio of the wide family on one MI355X (integer family: 0 everywhere, every output bit for bit):
                     Px      rx_inf  rz_inf  rx      rz      dots     norms, vec_norms
    rows             0.29    0.41    0.22    0.36    0.24    0.051    < 1e-3
    columns          0 (=)   0.015   0.29    0.014   0.29    < 1e-3   < 1e-3
    n = m, all eight 0 (=)   0 (=)   0 (=)   0.29    0.29    0.006    0.014
(0 (=): one product per entry, or none -- the reference's bits.  0.29 = 2 / 7: rx and rz of three terms are two roundings
of the seven allowed.  The dots and norms of the long vectors err by a few roundings where the bound allows n + 4 of them.)

Wrong kernels (each a one-line change that stays in bounds, built in a scratch copy and run on the MI355X unless marked):
    * the wavefront tail `for (; t < e; t += 64)` bounded by `t + 64 < e`: run -- test_rows_of_every_length[integer, wide]
      (first Px[100], 302 entries: 199 for 210; rz_inf of the row of 33), test_columns_of_every_length[integer, wide]
      (rx_inf of the column of 33 is 0 for -80), test_same_answers_twice_and_after_update_data fail; the vector sizes pass
    * build_spmat emitting chunks only while `b + B_CHUNK <= ptr[r + 1]` (the ragged last chunk dropped): run -- the same
      five fail (Px[0], 21599 entries: -350 for -279; rz_inf[24], the row of 21503; rx_inf[5], the column of 21503)
    * k_gather_Bprep<SPMV> writing 0 where aux is given: run -- test_rows_of_every_length[integer, wide] and
      test_same_answers_twice_and_after_update_data fail (rz_inf[21], the row of 16385 entries: off by s = 4); the columns
      pass, as they must: A'z has no aux and A x + s has no workgroup row there
    * empty rows left out of the thread list: run -- the same five as the first fail (Px[7777], rz_inf[0], rx_inf of the empty
      column are the NaN the buffers held)
    * k_multi_dot_partial striding by `gridDim.x * WG` instead of `nb * WG`: run -- nothing fails, and nothing can: the
      stride is only taken when nb * WG < n, that is at nb = 512, and then gridDim.x, the largest nb of the batch, is 512
      too; with nb < 512 no thread makes a second trip under either stride.  Not a gap of the tests: the same function
    * store_row<SPMV> ignoring alpha: run -- all 21 cases fail (rx_inf has the wrong sign wherever A'z is not 0)
A k_gather_Bprep that does not reset its rows (argued, not run) adds every call's chunks onto the NaN, or onto the first
call's result: the first and the second call of test_same_answers_twice_and_after_update_data fail."""
import time

import numpy as np
import pytest

from tests import spmv_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hipdev(hip):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    return hip


class Handle:
    """HipKKTSolver + HipKKTSystem over one pattern, the device arrays of a point and of the five outputs"""

    def __init__(self, hip, pr):
        self.hip, self.pr = hip, pr
        n, m = pr["n"], pr["m"]
        v = R.integer_point(pr, 0)
        t0 = time.perf_counter()
        P = hip.CscMatrix(n, n, pr["P"][0], pr["P"][1], v["Pv"])
        A = hip.CscMatrix(m, n, pr["A"][0], pr["A"][1], v["Av"])
        self.ks = hip.HipKKTSolver(P, A, pr["cones"], m, n)
        self.sys = hip.HipKKTSystem(self.ks, P, A, v["q"], v["b"])
        self.create_seconds = time.perf_counter() - t0
        self.vars = hip.DeviceVariables(n, m)
        self.out = {k: hip.DeviceArray(n if k in ("Px", "rx_inf", "rx") else m) for k in R.OUTPUTS}
        self.nan = {k: np.full(a.n, np.nan) for k, a in self.out.items()}

    def load(self, v, P=True, A=True, q=True, b=True):
        """the values of v through update_data (P only where it has entries)"""
        self.sys.update_data(P=v["Pv"] if P and len(v["Pv"]) else None, A=v["Av"] if A else None,
                             q=v["q"] if q else None, b=v["b"] if b else None)

    def run(self, v):
        """residuals_update(norms=True) at the point of v -> what spmv_ref.compare takes"""
        d, o = self.vars, self.out
        d.x.copy_from(v["x"])
        d.z.copy_from(v["z"])
        d.s.copy_from(v["s"])
        d.tau, d.kappa = v["tau"], v["kappa"]
        for k, a in o.items():
            a.copy_from(self.nan[k])
        res = self.sys.residuals_update(d, o["rx"], o["rz"], o["rx_inf"], o["rz_inf"], o["Px"], norms=True)
        got = {k: a.numpy() for k, a in o.items()}
        got.update(res)
        return got


_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def release_handles():
    """the handles cached for the module are released with it, not at interpreter exit"""
    yield
    _HANDLES.clear()


def handle(hip, key):
    if key not in _HANDLES:
        pr = R.rows_problem() if key == "rows" else R.cols_problem() if key == "cols" else R.vector_problem(key, key)
        _HANDLES[key] = Handle(hip, pr)
        print("  (handle %s: n = %d, m = %d, %.3f s)" % (key, pr["n"], pr["m"], _HANDLES[key].create_seconds))
    return _HANDLES[key]


def check(label, h, v, got, exact):
    ratios, fails = R.compare(h.pr, v, got, exact)
    print("  %s, %s family: largest error / bound  %s" % (label, "integer" if exact else "wide", "  ".join(
        "%s %.3g" % (k, r) for k, r in ratios.items())))
    assert not fails, (label, fails)
    return ratios


def point(pr, family, seed):
    return R.integer_point(pr, seed) if family == "integer" else R.wide_point(pr, seed)


FAMILIES = ("integer", "wide")


# ---- 1. rows of A and of the symmetric P ------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_rows_of_every_length(hipdev, family):
    """thread, wavefront and workgroup rows of Arow and Psym in the same k_gather_merged launches, every edge of the
    wavefront and chunk loops, the empty rows; per entry"""
    h = handle(hipdev, "rows")
    pr = h.pr
    assert list(R.a_row_lengths(pr)) == R.ROW_LENGTHS
    ps = R.psym_row_lengths(pr)
    assert (ps[0], ps[R.P_WAVE_ROW], ps[R.P_EMPTY]) == (pr["n"] - 1, 302, 0)
    v = point(pr, family, 21)
    h.load(v)
    got = h.run(v)
    check("rows", h, v, got, family == "integer")
    # the empty rows hold exactly aux (A x + s) or +0 (P x)
    assert got["rz_inf"][0] == v["s"][0] and R.same_bits(got["Px"][R.P_EMPTY:R.P_EMPTY + 1], [0.0])


# ---- 2. columns of A ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_columns_of_every_length(hipdev, family):
    """Acol with alpha = -1 and no aux on every class, 21600 thread rows of Arow (many empty), no P: Px = +0, x.Px = 0"""
    h = handle(hipdev, "cols")
    pr = h.pr
    assert list(R.a_col_lengths(pr)) == R.COL_LENGTHS and len(pr["P"][1]) == 0
    v = point(pr, family, 22)
    h.load(v)
    got = h.run(v)
    check("columns", h, v, got, family == "integer")
    assert R.same_bits(got["Px"], np.zeros(pr["n"])) and R.same_bits([got["dot_xPx"]], [0.0])
    assert R.same_bits(got["rx_inf"][:1], [0.0])  # the empty column
    empty = R.a_row_lengths(pr) == 0
    assert int(np.sum(empty)) > 0 and R.same_bits(got["rz_inf"][empty], v["s"][empty])


# ---- 3. vector sizes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", R.VECTOR_SIZES)
def test_vector_sizes(hipdev, n, family):
    """the block counts of the dot products and the grid-stride trips of k_lin3 / k_waxpby: every output vector, the
    four dots, rtau, the five norms and vec_norms of three arrays"""
    h = handle(hipdev, n)
    pr = h.pr
    v = point(pr, family, 23)
    h.load(v)
    got = h.run(v)
    exact = family == "integer"
    check("n = m = %d" % n, h, v, got, exact)
    o = h.out
    nrm = h.sys.vec_norms(o["Px"], o["rx_inf"], o["rz_inf"])
    worst = 0.0
    for have, key in zip(nrm, ("Px", "rx_inf", "rz_inf")):
        want, bound = R.norm_ref(got[key])
        worst = max(worst, abs(have - want) / bound)
        assert abs(have - want) <= bound and (not exact or have == want), (key, have, want, bound)
    print("  n = m = %d, %s family: vec_norms largest error / bound %.3g" % (n, family, worst))
    assert h.sys.vec_norms() == []
    # one array, and the same array three times: the slots do not depend on what shares the launch
    assert h.sys.vec_norms(o["rz_inf"]) == [nrm[2]] and h.sys.vec_norms(o["Px"], o["Px"], o["Px"]) == [nrm[0]] * 3


# ---- 4. the same answers twice, and new values on the long rows ---------------------------------------------------------
def test_same_answers_twice_and_after_update_data(hipdev):
    """a second call must not see what the first left in the targets of the chunks' atomic adds (k_gather_Bprep resets
    them); update_data(A=, P=) refreshes the row-ordered copies through their maps (k_gather_values), long rows included"""
    h = handle(hipdev, "rows")
    pr = h.pr
    v = R.integer_point(pr, 31)
    h.load(v)
    first = h.run(v)
    check("rows, first call", h, v, first, True)
    # the second call without NaN in the outputs: they hold the first call's results
    res = h.sys.residuals_update(h.vars, h.out["rx"], h.out["rz"], h.out["rx_inf"], h.out["rz_inf"], h.out["Px"], norms=True)
    second = dict({k: a.numpy() for k, a in h.out.items()}, **res)
    check("rows, second call", h, v, second, True)
    for k in R.OUTPUTS:
        assert R.same_bits(first[k], second[k]), k
    w = R.integer_point(pr, 32)
    assert np.any(w["Av"] != v["Av"]) and np.any(w["Pv"] != v["Pv"])
    new = dict(v, Pv=w["Pv"], Av=w["Av"])  # new matrices, the same q, b and point
    h.load(new, q=False, b=False)
    third = h.run(new)
    check("rows, new P and A", h, new, third, True)
    assert not R.same_bits(third["Px"], first["Px"]) and not R.same_bits(third["rz_inf"], first["rz_inf"])
    wide = dict(R.wide_point(pr, 33), q=v["q"], b=v["b"])
    h.load(wide, q=False, b=False)
    check("rows, new wide P and A", h, wide, h.run(wide), False)
