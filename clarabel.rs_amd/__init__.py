"""clarabel.rs_amd -- host-side mirror (Python/ctypes) of the MI355X-native KKT
backend's C ABI (include/clarabel_hip.h).

The reference's host language is Rust (absent from this image), so the mirror of
its operator interface is written in Python over the C ABI, keeping the
reference's names, argument meaning and error behaviour:

  HipDirectLDLSolver   <->  trait DirectLDLSolver<f64>
                            (src/solver/core/kktsolvers/direct/quasidef/mod.rs:14-26,
                             reference engine ldlsolvers/qdldl.rs:18-107)
  HipKKTSolver         <->  trait KKTSolver<f64> / DirectLDLKKTSolver
                            (src/solver/core/kktsolvers/mod.rs:7-18,
                             quasidef/directldlkktsolver.rs:18-405)

There is NO CPU fallback: every numeric call runs hand-written HIP kernels from
csrc/ through libclarabel_hip.so, and the import fails loudly when that library
is missing.  (The CPU oracle under /oracle is test infrastructure and is never
imported from here.)

Because the directory name contains a dot it cannot be imported with a plain
`import`; use `__graft_entry__.load_package()` (or tests/conftest.py's `hip`
fixture), which loads it under the module name `clarabel_rs_amd`.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CLARABEL_HIP_LIB: another build of the same ABI -- tests load the library as it ships, libclarabel_hip_ship.so, through it)
LIB_PATH = os.environ.get("CLARABEL_HIP_LIB") or os.path.join(_HERE, "libclarabel_hip.so")
SHIP_LIB_PATH = os.path.join(_HERE, "libclarabel_hip_ship.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "clarabel_hip.h")

u64 = np.uint64
f64 = np.float64
P_U64 = C.POINTER(C.c_uint64)
P_I64 = C.POINTER(C.c_int64)
P_F64 = C.POINTER(C.c_double)
P_I8 = C.POINTER(C.c_int8)
P_I32 = C.POINTER(C.c_int32)

# chip_status
OK, ERR_DIM, ERR_EMPTY_COLUMN, ERR_NOT_TRIU, ERR_ZERO_PIVOT, ERR_BAD_PERM = 0, -1, -2, -3, -4, -5
ERR_NOT_FACTORED, ERR_NO_DEVICE, ERR_HIP, ERR_ARG, ERR_UNSUPPORTED = -6, -7, -8, -9, -10
ERR_UPDATE_NOT_ALLOWED = -11
STATUS_NAMES = {0: "ok", -1: "IncompatibleDimension", -2: "EmptyColumn", -3: "NotUpperTriangular",
                -4: "ZeroPivot", -5: "InvalidPermutation", -6: "NotFactored", -7: "NoDevice", -8: "HipError",
                -9: "BadArgument", -10: "Unsupported", -11: "UpdateNotAllowed"}
DEVICE_HOST_ONLY = -2
BJAC_MAX_DIR = 16  # CHIP_BJAC_MAX_DIR: the directions of one chip_bjac_* call
BVJP_MAX_DIR = 16  # CHIP_BVJP_MAX_DIR: the cotangents of one chip_bvjp_* call

# SupportedConeT tags
ZeroConeT, NonnegativeConeT, SecondOrderConeT, ExponentialConeT, PowerConeT, GenPowerConeT, PSDTriangleConeT = range(7)

# profile families of chip_kkt_profile
PF_NONE, PF_SYMV_T, PF_BWD_T, PF_FWD_T, PF_FACTOR_T = range(5)


class ChipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = ""
        try:
            msg = lib().chip_last_error().decode()
        except Exception:
            pass
        super().__init__("%s: %s (%d) %s" % (where, STATUS_NAMES.get(code, "?"), code, msg))


class Settings(C.Structure):
    """chip_settings == the CoreSettings fields the path consumes
    (src/solver/implementations/default/settings.rs:126-181) + engine knobs."""
    _fields_ = [("static_regularization_enable", C.c_int32), ("static_regularization_constant", C.c_double),
                ("static_regularization_proportional", C.c_double), ("dynamic_regularization_enable", C.c_int32),
                ("dynamic_regularization_eps", C.c_double), ("dynamic_regularization_delta", C.c_double),
                ("iterative_refinement_enable", C.c_int32), ("iterative_refinement_reltol", C.c_double),
                ("iterative_refinement_abstol", C.c_double), ("iterative_refinement_max_iter", C.c_int32),
                ("iterative_refinement_stop_ratio", C.c_double), ("device", C.c_int32),
                ("amd_dense_scale", C.c_double), ("use_graph", C.c_int32), ("reserved0", C.c_int32),
                ("linesearch_backtrack_step", C.c_double), ("min_terminate_step_length", C.c_double),
                ("reserved", C.c_int32 * 2)]

    @staticmethod
    def default(**kw):
        s = Settings()
        lib().chip_settings_default(C.byref(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s


class Info(C.Structure):
    """chip_info == LinearSolverInfo (src/solver/core/kktsolvers/mod.rs:27-38) + factor statistics."""
    _fields_ = [("name", C.c_char * 16), ("threads", C.c_int64), ("direct", C.c_int32), ("nnzA", C.c_int64),
                ("nnzL", C.c_int64), ("positive_inertia", C.c_int64), ("regularize_count", C.c_int64),
                ("n", C.c_int64), ("n_levels", C.c_int64), ("amd_lnz", C.c_double), ("amd_ndiv", C.c_double),
                ("amd_nmultsubs_ldl", C.c_double), ("last_ir_iterations", C.c_int32),
                ("last_regularizer", C.c_double)]


_LIB = None


def build(verbose=False, testing=True):
    """Compile csrc/ into libclarabel_hip.so for gfx950 (hipcc cross-compiles without a GPU).  testing: with the
    hooks of include/clarabel_hip_testing.h (what the test suite needs; the Makefile's own default leaves them out)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8", "TESTING=%d" % (1 if testing else 0)]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def build_ship(verbose=False):
    """the library as it ships (TESTING=0: no test hooks) beside the test build: libclarabel_hip_ship.so"""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8", "ship"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return SHIP_LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: the HIP extension is mandatory (no CPU fallback). "
                              "Run `python -c 'import __graft_entry__ as g; g.build()'`." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.chip_last_error.restype = C.c_char_p
        L.chip_kkt_stream.restype = C.c_void_p
        _LIB = L
    return _LIB


def device_count():
    return int(lib().chip_device_count())


def _u(a):
    return np.ascontiguousarray(a, dtype=u64)


def _f(a):
    return np.ascontiguousarray(a, dtype=f64)


def _pu(a):
    return a.ctypes.data_as(P_U64)


def _pf(a):
    return a.ctypes.data_as(P_F64)


class UpdateNotAllowedError(ChipError):
    """a data update refused because presolve or chordal decomposition changed the problem (the reference's
    DataUpdateError::PresolveIsActive / ChordalDecompositionIsActive); code == ERR_UPDATE_NOT_ALLOWED"""


def _check(rc, where):
    if rc == ERR_UPDATE_NOT_ALLOWED:
        raise UpdateNotAllowedError(rc, where)
    if rc < 0:
        raise ChipError(rc, where)
    return rc


def _status(rc, where):
    """1 / 0 -> bool (the reference's is_success), negative -> ChipError"""
    return bool(_check(rc, where))


def auto_select(lnz, n_div, n_mult_subs_ldl):
    """ldl_auto_select's rule (ldlsolvers/auto.rs:62-87): 'qdldl' (simplicial) or 'faer' (supernodal)"""
    return "faer" if lib().chip_auto_select(C.c_double(lnz), C.c_double(n_div), C.c_double(n_mult_subs_ldl)) else "qdldl"


def amd_order(n, colptr, rowval, dense_scale=1.5):
    """AMD ordering of the symmetric matrix with upper triangle (colptr,rowval).
    Replaces `amd::order` at src/qdldl/qdldl.rs:905-917.  Returns (perm, iperm, info3)."""
    colptr, rowval = _u(colptr), _u(rowval)
    perm = np.zeros(n, dtype=u64)
    iperm = np.zeros(n, dtype=u64)
    info = np.zeros(3)
    _check(lib().chip_amd_order(C.c_int64(n), _pu(colptr), _pu(rowval), C.c_double(dense_scale), _pu(perm),
                                _pu(iperm), _pf(info)), "chip_amd_order")
    return perm.astype(np.int64), iperm.astype(np.int64), info


def _supernodes(fn, h):
    cnt = C.c_int64()
    _check(fn(h, C.byref(cnt), None, None), "get_supernodes")
    if cnt.value == 0:
        return []
    ptr = np.zeros(cnt.value + 1, dtype=u64)
    _check(fn(h, C.byref(cnt), _pu(ptr), None), "get_supernodes")
    cols = np.zeros(max(int(ptr[-1]), 1), dtype=u64)
    _check(fn(h, C.byref(cnt), _pu(ptr), _pu(cols)), "get_supernodes")
    return [cols[int(ptr[i]):int(ptr[i + 1])].astype(np.int64) for i in range(cnt.value)]


class CscMatrix:
    """CscMatrix<f64> (src/algebra/csc/core.rs:45-60): m, n, colptr, rowval, nzval."""

    def __init__(self, m, n, colptr, rowval, nzval):
        self.m, self.n = int(m), int(n)
        self.colptr = _u(colptr)
        self.rowval = _u(rowval)
        self.nzval = _f(nzval)
        assert len(self.colptr) == self.n + 1 and len(self.rowval) == len(self.nzval)

    @property
    def nnz(self):
        return int(self.colptr[-1])

    @staticmethod
    def from_scipy(M):
        M = M.tocsc()
        M.sort_indices()
        return CscMatrix(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


class HipDirectLDLSolver:
    """`direct_solve_method = "hip"`: DirectLDLSolver<f64> on the MI355X.

    new(KKT, Dsigns, settings, perm)  -- ldlsolvers/config.rs:21-22
    required_matrix_shape() = Triu     -- quasidef/mod.rs:14-16"""

    def __init__(self, KKT, Dsigns, settings=None, perm=None):
        assert KKT.m == KKT.n, "KKT matrix is not square"  # ldlsolvers/qdldl.rs:24
        self.settings = settings or Settings.default()
        self.n = KKT.n
        self._h = C.c_void_p()
        ds = np.ascontiguousarray(Dsigns, dtype=np.int8)
        pp = None
        if perm is not None:
            perm = _u(perm)
            pp = _pu(perm)
        _check(lib().chip_ldl_create(C.byref(self._h), C.c_int64(self.n), _pu(KKT.colptr), _pu(KKT.rowval),
                                     _pf(KKT.nzval), ds.ctypes.data_as(P_I8), pp, C.byref(self.settings)),
               "chip_ldl_create")

    @staticmethod
    def required_matrix_shape():
        return "triu"

    def __del__(self):
        if getattr(self, "_h", None):
            lib().chip_ldl_destroy(self._h)
            self._h = None

    def update_values(self, index, values):
        index, values = _u(index), _f(values)
        _check(lib().chip_ldl_update_values(self._h, _pu(index), _pf(values), C.c_int64(len(index))), "update_values")

    def scale_values(self, index, scale):
        index = _u(index)
        _check(lib().chip_ldl_scale_values(self._h, _pu(index), C.c_double(scale), C.c_int64(len(index))),
               "scale_values")

    def offset_values(self, index, offset, signs):
        index = _u(index)
        signs = np.ascontiguousarray(signs, dtype=np.int8)
        assert len(index) == len(signs)  # qdldl.rs:167
        _check(lib().chip_ldl_offset_values(self._h, _pu(index), C.c_double(offset), signs.ctypes.data_as(P_I8),
                                            C.c_int64(len(index))), "offset_values")

    def set_values(self, nzval):
        nzval = _f(nzval)
        _check(lib().chip_ldl_set_values(self._h, _pf(nzval)), "set_values")

    # ---- fast path of the strict drop-in (include/clarabel_hip.h: chip_ldl_register_index ...) ----
    def register_index(self, index, signs=None):
        index = _u(index)
        sg = None if signs is None else np.ascontiguousarray(signs, dtype=np.int8)
        out = C.c_int32()
        _check(lib().chip_ldl_register_index(self._h, _pu(index), C.c_int64(len(index)),
                                             None if sg is None else sg.ctypes.data_as(C.POINTER(C.c_int8)), C.byref(out)),
               "ldl_register_index")
        return int(out.value)

    def update_values_id(self, set_id, values):
        values = _f(values)
        _check(lib().chip_ldl_update_values_id(self._h, C.c_int32(set_id), _pf(values)), "ldl_update_values_id")

    def scale_values_id(self, set_id, scale):
        _check(lib().chip_ldl_scale_values_id(self._h, C.c_int32(set_id), C.c_double(scale)), "ldl_scale_values_id")

    def offset_values_id(self, set_id, offset):
        _check(lib().chip_ldl_offset_values_id(self._h, C.c_int32(set_id), C.c_double(offset)), "ldl_offset_values_id")

    def pin_buffer(self, array):
        _check(lib().chip_ldl_pin_buffer(self._h, C.c_void_p(array.ctypes.data), C.c_uint64(array.nbytes)), "ldl_pin_buffer")

    def solve_refined(self, x, b, settings=None):
        """solve + device-resident refinement (directldlkktsolver.rs:266-321); returns (ok, rounds)"""
        its = C.c_int32()
        rc = lib().chip_ldl_solve_refined(self._h, _pf(x), _pf(_f(b)), None if settings is None else C.byref(settings), C.byref(its))
        return bool(_status(rc, "ldl_solve_refined")), int(its.value)

    def refactor(self, kkt=None):
        """-> bool (all Dinv finite), ldlsolvers/qdldl.rs:98-106"""
        return bool(_check(lib().chip_ldl_refactor(self._h), "refactor"))

    def solve(self, kkt, x, b):
        """x <- K^-1 b; b untouched (ldlsolvers/qdldl.rs:91-96)"""
        b = _f(b)
        assert x.dtype == f64 and x.flags.c_contiguous and len(x) == self.n and len(b) == self.n
        _check(lib().chip_ldl_solve(self._h, _pf(x), _pf(b)), "solve")

    def solve_dev(self, x_ptr, b_ptr):
        _check(lib().chip_ldl_solve_dev(self._h, C.c_void_p(x_ptr), C.c_void_p(b_ptr)), "solve_dev")

    def linear_solver_info(self):
        info = Info()
        _check(lib().chip_ldl_info(self._h, C.byref(info)), "info")
        return info

    @property
    def perm(self):
        p = np.zeros(self.n, dtype=u64)
        _check(lib().chip_ldl_get_perm(self._h, _pu(p)), "get_perm")
        return p.astype(np.int64)

    def symbolic(self):
        info = self.linear_solver_info()
        et = np.zeros(self.n, dtype=u64)
        Lp = np.zeros(self.n + 1, dtype=u64)
        Li = np.zeros(max(info.nnzL, 1), dtype=u64)
        lv = np.zeros(max(self.n, 1), dtype=u64)
        _check(lib().chip_ldl_get_symbolic(self._h, _pu(et), _pu(Lp), _pu(Li), _pu(lv)), "get_symbolic")
        et = et.astype(np.int64)  # UINT64_MAX -> -1
        return et, Lp.astype(np.int64), Li[:info.nnzL].astype(np.int64), lv[:self.n].astype(np.int64)

    def supernodes(self):
        return _supernodes(lib().chip_ldl_get_supernodes, self._h)

    def factors(self):
        info = self.linear_solver_info()
        Lp = np.zeros(self.n + 1, dtype=u64)
        Li = np.zeros(max(info.nnzL, 1), dtype=u64)
        Lx = np.zeros(max(info.nnzL, 1))
        D = np.zeros(self.n)
        Dinv = np.zeros(self.n)
        _check(lib().chip_ldl_get_factors(self._h, _pu(Lp), _pu(Li), _pf(Lx), _pf(D), _pf(Dinv)), "get_factors")
        return Lp.astype(np.int64), Li[:info.nnzL].astype(np.int64), Lx[:info.nnzL], D, Dinv


class HipKKTSolver:
    """KKTSolver<f64> (kktsolvers/mod.rs:7-18) == DirectLDLKKTSolver on the device.

    new(P, A, cones, m, n, settings) -- directldlkktsolver.rs:60-118.
    `cones`: list of (tag, dim), (tag, dim, dim2) or (tag, dim, dim2, alpha) SupportedConeT
    descriptors (alpha = PowerConeT exponent)."""

    def __init__(self, P, A, cones, m, n, settings=None, perm=None):
        assert P.n == n and A.n == n and A.m == m
        self.settings = settings or Settings.default()
        self.cones = [(tuple(c) + (0, 0, 0.5)[len(c) - 1:])[:4] if len(c) < 4 else tuple(c) for c in cones]
        tags = np.array([c[0] for c in self.cones], dtype=np.int32)
        dims = np.array([c[1] for c in self.cones], dtype=np.int64)
        dims2 = np.array([c[2] for c in self.cones], dtype=np.int64)
        alphas = np.array([0.5 if c[0] == 5 else c[3] for c in self.cones], dtype=np.float64)
        self._h = C.c_void_p()
        pp = None
        if perm is not None:
            perm = _u(perm)
            pp = _pu(perm)
        _check(lib().chip_kkt_create(C.byref(self._h), C.c_int64(n), C.c_int64(m), _pu(P.colptr), _pu(P.rowval),
                                     _pf(P.nzval), _pu(A.colptr), _pu(A.rowval), _pf(A.nzval),
                                     C.c_int64(len(self.cones)), tags.ctypes.data_as(P_I32),
                                     dims.ctypes.data_as(P_I64), dims2.ctypes.data_as(P_I64), _pf(alphas),
                                     C.byref(self.settings), pp), "chip_kkt_create")
        if self.settings.device != DEVICE_HOST_ONLY:
            for i, c in enumerate(self.cones):  # GenPowerConeT(alpha, dim2) == (5, len(alpha), dim2, alpha)
                if c[0] == 5:
                    a = _f(c[3])
                    assert len(a) == c[1]
                    _check(lib().chip_kkt_set_genpow_alpha(self._h, C.c_int64(i), _pf(a)), "set_genpow_alpha")
        d = (C.c_int64 * 8)()
        lib().chip_kkt_dims(self._h, d)
        self.n, self.m, self.p, self.N, self.nnzK, self.nHs, self.NF, self.nnzU = [int(v) for v in d]
        self.nnzP, self.nnzA = P.nnz, A.nnz

    def __del__(self):
        if getattr(self, "_h", None):
            lib().chip_kkt_destroy(self._h)
            self._h = None

    # -- layout introspection (host) ------------------------------------------
    def kkt_matrix(self):
        cp = np.zeros(self.N + 1, dtype=u64)
        rv = np.zeros(max(self.nnzK, 1), dtype=u64)
        nz = np.zeros(max(self.nnzK, 1))
        _check(lib().chip_kkt_get_matrix(self._h, _pu(cp), _pu(rv), _pf(nz)), "get_matrix")
        return CscMatrix(self.N, self.N, cp, rv[:self.nnzK], nz[:self.nnzK])

    def maps(self):
        mP = np.zeros(max(self.nnzP, 1), dtype=u64)
        mA = np.zeros(max(self.nnzA, 1), dtype=u64)
        mH = np.zeros(max(self.nHs, 1), dtype=u64)
        dP = np.zeros(max(self.n, 1), dtype=u64)
        dF = np.zeros(max(self.N, 1), dtype=u64)
        ds = np.zeros(max(self.N, 1), dtype=np.int8)
        _check(lib().chip_kkt_get_map(self._h, _pu(mP), _pu(mA), _pu(mH), _pu(dP), _pu(dF),
                                      ds.ctypes.data_as(P_I8)), "get_map")
        return {"P": mP[:self.nnzP].astype(np.int64), "A": mA[:self.nnzA].astype(np.int64),
                "Hsblocks": mH[:self.nHs].astype(np.int64), "diagP": dP[:self.n].astype(np.int64),
                "diag_full": dF[:self.N].astype(np.int64), "dsigns": ds[:self.N]}

    @property
    def perm(self):
        p = np.zeros(self.N, dtype=u64)
        _check(lib().chip_kkt_get_perm(self._h, _pu(p)), "get_perm")
        return p.astype(np.int64)

    def symbolic(self):
        info = self.linear_solver_info()
        et = np.zeros(self.N, dtype=u64)
        Lp = np.zeros(self.N + 1, dtype=u64)
        Li = np.zeros(max(info.nnzL, 1), dtype=u64)
        lv = np.zeros(max(self.N, 1), dtype=u64)
        _check(lib().chip_kkt_get_symbolic(self._h, _pu(et), _pu(Lp), _pu(Li), _pu(lv)), "get_symbolic")
        return et.astype(np.int64), Lp.astype(np.int64), Li[:info.nnzL].astype(np.int64), lv[:self.N].astype(np.int64)

    def supernodes(self):
        """[(columns ascending, permuted numbering), ...] of the chain supernodes"""
        return _supernodes(lib().chip_kkt_get_supernodes, self._h)

    def values(self):
        nz = np.zeros(max(self.nnzK, 1))
        _check(lib().chip_kkt_get_values(self._h, _pf(nz)), "get_values")
        return nz[:self.nnzK]

    # -- the KKTSolver trait -----------------------------------------------------
    def update_scaling(self, s, z, mu=1.0, strategy=0):
        """cones.update_scaling(s, z, mu, strategy) for the device-held cones -> bool
        (strategy 0 = PrimalDual, 1 = Dual; mu only matters for Exp/Pow cones under Dual)"""
        s, z = _f(s), _f(z)
        assert len(s) == self.m and len(z) == self.m
        return bool(_check(lib().chip_kkt_update_scaling(self._h, _pf(s), _pf(z), C.c_double(mu),
                                                         C.c_int32(strategy)), "update_scaling"))

    def update_scaling_dev(self, s_ptr, z_ptr, mu=1.0, strategy=0):
        return bool(_check(lib().chip_kkt_update_scaling_dev(self._h, C.c_void_p(s_ptr), C.c_void_p(z_ptr),
                                                             C.c_double(mu), C.c_int32(strategy)),
                           "update_scaling_dev"))

    def update(self, hsblocks=None):
        """KKTSolver::update(cones, settings) -> bool"""
        hp = None
        if hsblocks is not None:
            hsblocks = _f(hsblocks)
            assert len(hsblocks) == self.nHs
            hp = _pf(hsblocks)
        return bool(_check(lib().chip_kkt_update(self._h, hp), "update"))

    def setrhs(self, rhsx, rhsz):
        rhsx, rhsz = _f(rhsx), _f(rhsz)
        assert len(rhsx) == self.n and len(rhsz) == self.m
        _check(lib().chip_kkt_setrhs(self._h, _pf(rhsx), _pf(rhsz)), "setrhs")

    def setrhs_dev(self, x_ptr, z_ptr):
        _check(lib().chip_kkt_setrhs_dev(self._h, C.c_void_p(x_ptr), C.c_void_p(z_ptr)), "setrhs_dev")

    def solve(self, lhsx=None, lhsz=None):
        """KKTSolver::solve(lhsx, lhsz, settings) -> bool"""
        px = _pf(lhsx) if lhsx is not None else None
        pz = _pf(lhsz) if lhsz is not None else None
        return bool(_check(lib().chip_kkt_solve(self._h, px, pz), "solve"))

    def solve_dev(self, x_ptr, z_ptr):
        return bool(_check(lib().chip_kkt_solve_dev(self._h, C.c_void_p(x_ptr) if x_ptr else None,
                                                    C.c_void_p(z_ptr) if z_ptr else None), "solve_dev"))

    def solve_full(self, b):
        b = _f(b)
        assert len(b) == self.N
        x = np.zeros(self.N)
        ok = bool(_check(lib().chip_kkt_solve_full(self._h, _pf(x), _pf(b)), "solve_full"))
        return ok, x

    def update_P(self, Pnzval):
        Pnzval = _f(Pnzval)
        assert len(Pnzval) == self.nnzP
        _check(lib().chip_kkt_update_P(self._h, _pf(Pnzval)), "update_P")

    def update_A(self, Anzval):
        Anzval = _f(Anzval)
        assert len(Anzval) == self.nnzA
        _check(lib().chip_kkt_update_A(self._h, _pf(Anzval)), "update_A")

    def mul_Hs_dev(self, y_ptr, x_ptr):
        _check(lib().chip_kkt_mul_Hs_dev(self._h, C.c_void_p(y_ptr), C.c_void_p(x_ptr)), "mul_Hs_dev")

    # -- CompositeCone operations either side of the solve (device pointers, m doubles) -----
    def affine_ds_dev(self, ds_ptr, s_ptr):
        _check(lib().chip_kkt_affine_ds_dev(self._h, C.c_void_p(ds_ptr), C.c_void_p(s_ptr)), "affine_ds")

    def combined_ds_shift_dev(self, shift_ptr, step_z_ptr, step_s_ptr, sigma_mu):
        _check(lib().chip_kkt_combined_ds_shift_dev(self._h, C.c_void_p(shift_ptr), C.c_void_p(step_z_ptr),
                                                    C.c_void_p(step_s_ptr), C.c_double(sigma_mu)), "combined_ds_shift")

    def ds_from_dz_offset_dev(self, out_ptr, ds_ptr, z_ptr):
        _check(lib().chip_kkt_ds_from_dz_offset_dev(self._h, C.c_void_p(out_ptr), C.c_void_p(ds_ptr),
                                                    C.c_void_p(z_ptr)), "ds_from_dz_offset")

    def step_length_dev(self, dz_ptr, ds_ptr, z_ptr, s_ptr, alpha_max=1.0):
        a = C.c_double(0)
        _check(lib().chip_kkt_step_length_dev(self._h, C.c_void_p(dz_ptr), C.c_void_p(ds_ptr), C.c_void_p(z_ptr),
                                              C.c_void_p(s_ptr), C.c_double(alpha_max), C.byref(a)), "step_length")
        return a.value

    def margins_dev(self, z_ptr):
        a, b = C.c_double(0), C.c_double(0)
        _check(lib().chip_kkt_margins_dev(self._h, C.c_void_p(z_ptr), C.byref(a), C.byref(b)), "margins")
        return a.value, b.value

    def scaled_unit_shift_dev(self, z_ptr, alpha, primal_cone):
        _check(lib().chip_kkt_scaled_unit_shift_dev(self._h, C.c_void_p(z_ptr), C.c_double(alpha),
                                                    C.c_int32(1 if primal_cone else 0)), "scaled_unit_shift")

    def unit_initialization_dev(self, z_ptr, s_ptr):
        _check(lib().chip_kkt_unit_initialization_dev(self._h, C.c_void_p(z_ptr), C.c_void_p(s_ptr)),
               "unit_initialization")

    def compute_barrier_dev(self, z_ptr, s_ptr, dz_ptr, ds_ptr, alpha):
        out = C.c_double(0)
        _check(lib().chip_kkt_compute_barrier_dev(self._h, C.c_void_p(z_ptr), C.c_void_p(s_ptr),
                                                  C.c_void_p(dz_ptr), C.c_void_p(ds_ptr), C.c_double(alpha),
                                                  C.byref(out)), "compute_barrier")
        return out.value

    def degree(self):
        d = C.c_int64()
        _check(lib().chip_kkt_degree(self._h, C.byref(d)), "degree")
        return d.value

    def linear_solver_info(self):
        info = Info()
        _check(lib().chip_kkt_info(self._h, C.byref(info)), "info")
        return info

    def synchronize(self):
        _check(lib().chip_kkt_synchronize(self._h), "synchronize")

    # -- asynchronous variants: enqueue a whole iteration, collect the verdicts once ------------------
    def update_enqueue(self, hsblocks=None):
        hb = None if hsblocks is None else _f(hsblocks)
        _check(lib().chip_kkt_update_enqueue(self._h, None if hb is None else _pf(hb)), "update_enqueue")

    def update_scaled_enqueue(self, s_ptr, z_ptr, mu=1.0, strategy=0, hsblocks=None):
        """cones.update_scaling + the KKT update as ONE enqueue (core/solver.rs:334-352), verdicts with collect()"""
        hb = None if hsblocks is None else _f(hsblocks)
        _check(lib().chip_kkt_update_scaled_enqueue(self._h, C.c_void_p(s_ptr), C.c_void_p(z_ptr), C.c_double(mu),
                                                    C.c_int32(strategy), None if hb is None else _pf(hb)),
               "update_scaled_enqueue")

    def solve_dev_enqueue(self, x_ptr, z_ptr):
        _check(lib().chip_kkt_solve_dev_enqueue(self._h, C.c_void_p(x_ptr), C.c_void_p(z_ptr)), "solve_dev_enqueue")

    def solve2_dev_enqueue(self, rxa, rza, lxa, lza, rxb, rzb, lxb, lzb):
        """two independent solves as one call (chip_kkt_solve2_dev_enqueue): device pointers of the two right-hand sides
        and of the two results"""
        args = [C.c_void_p(int(p)) for p in (rxa, rza, lxa, lza, rxb, rzb, lxb, lzb)]
        _check(lib().chip_kkt_solve2_dev_enqueue(self._h, *args), "solve2_dev_enqueue")

    def collect(self):
        """-> (update_ok, [solve_ok, ...]) of everything enqueued since the last collect; one synchronisation.
        self.repeated_solves: indices (into that list) of solves whose fused launch timed out and that collect repeated
        on the one-kernel-per-phase path -- their lhs held garbage until now: device work enqueued behind them that
        consumed it (an all-gather, a dependent right-hand side) must be re-issued"""
        uok, n = C.c_int32(1), C.c_int32(0)
        sok = (C.c_int32 * 16)()
        _check(lib().chip_kkt_collect(self._h, C.byref(uok), C.byref(n), sok), "collect")
        cnt = min(n.value, 16)
        self.repeated_solves = [i for i in range(cnt) if sok[i] == 2]
        return bool(uok.value), [bool(sok[i]) for i in range(cnt)]

    def set_settings(self, settings):
        """the reference passes `settings` to update() / solve() on every call (kktsolvers/mod.rs:7-18)"""
        _check(lib().chip_kkt_set_settings(self._h, C.byref(settings)), "set_settings")
        self.settings = settings

    def scaling_ok(self):
        return bool(_status(lib().chip_kkt_scaling_ok(self._h), "scaling_ok"))

    def profile(self, family):
        _check(lib().chip_kkt_profile(self._h, C.c_int32(family)), "profile")

    def profile_read(self):
        out = (C.c_double * 8)()
        _check(lib().chip_kkt_profile_read(self._h, out), "profile_read")
        return {"launches": int(out[0]), "ms": float(out[1]), "family": int(out[2])}

    def work_model(self):
        """work of the chain-supernode kernels per refactor / per sweep (chip_kkt_work_model)"""
        out = (C.c_double * 8)()
        _check(lib().chip_kkt_work_model(self._h, out), "work_model")
        return {"sn_update_flops": float(out[0]), "sn_panel_entries": float(out[1]), "sn_extend_flops": float(out[2]),
                "sn_diag_rows_flops": float(out[3]), "n_supernodes": int(out[4]), "fold_groups": int(out[5]),
                "n_bundles": int(out[6]), "fused_threads": int(out[7])}

    def sweep_model(self):
        """how the substitutions run through the chain supernodes (chip_kkt_sweep_model)"""
        out = (C.c_double * 4)()
        _check(lib().chip_kkt_sweep_model(self._h, out), "sweep_model")
        return {"g_doubles": float(out[0]), "g_levels": int(out[1]), "sn_levels": int(out[2]), "g_build_launches": int(out[3])}

    def fused_fallbacks(self):
        return int(lib().chip_kkt_fused_fallbacks(self._h))

    def step_kernels(self):
        """bit 0: the fused solve is k_gstep_solve, bit 1: the bundle factorisation is k_gstep_factor (grouped fold)"""
        return int(lib().chip_kkt_step_kernels(self._h))


class CVars(C.Structure):
    """chip_vars: DefaultVariables (default/variables.rs:12-36) with device pointers"""
    _fields_ = [("x", C.c_void_p), ("z", C.c_void_p), ("s", C.c_void_p), ("tau", C.c_double),
                ("kappa", C.c_double)]


class DeviceVariables:
    """x[n], s[m], z[m] in HBM + tau, kappa on the host (DefaultVariables::new, variables.rs:41-50)"""

    def __init__(self, n, m):
        self.n, self.m = n, m
        self.x, self.s, self.z = DeviceArray(n), DeviceArray(m), DeviceArray(m)
        self.tau, self.kappa = 1.0, 1.0

    def cvars(self):
        return CVars(self.x.ptr, self.z.ptr, self.s.ptr, self.tau, self.kappa)


STEP_AFFINE, STEP_COMBINED = 0, 1


class HipKKTSystem:
    """DefaultKKTSystem (default/kktsystem.rs:16-292) + DefaultResiduals::update
    (default/residuals.rs:69-111), device resident, over an existing HipKKTSolver."""

    def __init__(self, kktsolver, P, A, q, b):
        self.ks = kktsolver
        self.n, self.m = kktsolver.n, kktsolver.m
        self._h = C.c_void_p()
        q, b = _f(q), _f(b)
        _check(lib().chip_kktsystem_create(C.byref(self._h), kktsolver._h, _pu(P.colptr), _pu(P.rowval),
                                           _pf(P.nzval), _pu(A.colptr), _pu(A.rowval), _pf(A.nzval), _pf(q),
                                           _pf(b)), "chip_kktsystem_create")

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().chip_kktsystem_destroy(self._h)
            self._h = C.c_void_p()

    def update(self):
        return _status(lib().chip_kktsystem_update(self._h), "kktsystem_update")

    def solve(self, lhs, rhs, variables, step_direction):
        """lhs, rhs, variables: DeviceVariables; lhs.tau / lhs.kappa are written -> bool"""
        cl, cr, cv = lhs.cvars(), rhs.cvars(), variables.cvars()
        ok = _status(lib().chip_kktsystem_solve(self._h, C.byref(cl), C.byref(cr), C.byref(cv),
                                                C.c_int32(step_direction)), "kktsystem_solve")
        if ok:
            lhs.tau, lhs.kappa = cl.tau, cl.kappa
        return ok

    def solve_initial_point(self, variables):
        cv = variables.cvars()
        return _status(lib().chip_kktsystem_solve_initial_point(self._h, C.byref(cv)), "solve_initial_point")

    def residuals_update(self, variables, rx, rz, rx_inf, rz_inf, Px, norms=False):
        """device outputs (DeviceArray) + dict of the host scalars of residuals.rs:103-110; with
        norms=True also 'norms' = (||x||, ||z||, ||s||, ||rz||, ||rx||) from the same synchronisation"""
        cv = variables.cvars()
        o = (C.c_double * 5)()
        nrm = (C.c_double * 5)() if norms else None
        _check(lib().chip_residuals_update_norms(self._h, C.byref(cv), C.c_void_p(rx.ptr), C.c_void_p(rz.ptr),
                                                 C.c_void_p(rx_inf.ptr), C.c_void_p(rz_inf.ptr), C.c_void_p(Px.ptr),
                                                 o, nrm), "residuals_update")
        out = dict(rtau=o[0], dot_qx=o[1], dot_bz=o[2], dot_sz=o[3], dot_xPx=o[4])
        if norms:
            out["norms"] = tuple(nrm)
        return out

    # ---- DefaultVariables on the device (default/variables.rs:58-261) -------------------------
    @staticmethod
    def _p(a):
        return C.c_void_p(a if isinstance(a, int) else a.ptr)

    def calc_mu(self, variables, dot_sz):
        cv, o = variables.cvars(), C.c_double()
        _check(lib().chip_variables_calc_mu(self._h, C.byref(cv), C.c_double(dot_sz), C.byref(o)), "calc_mu")
        return o.value

    def affine_step_rhs(self, d, rx, rz, rtau, variables):
        cd, cv = d.cvars(), variables.cvars()
        _check(lib().chip_variables_affine_step_rhs(self._h, C.byref(cd), self._p(rx), self._p(rz),
                                                    C.c_double(rtau), C.byref(cv)), "affine_step_rhs")
        d.tau, d.kappa = cd.tau, cd.kappa

    def combined_step_rhs(self, d, rx, rz, rtau, variables, step, sigma, mu, m):
        cd, cv, cs = d.cvars(), variables.cvars(), step.cvars()
        _check(lib().chip_variables_combined_step_rhs(self._h, C.byref(cd), self._p(rx), self._p(rz),
                                                      C.c_double(rtau), C.byref(cv), C.byref(cs),
                                                      C.c_double(sigma), C.c_double(mu), C.c_double(m)),
               "combined_step_rhs")
        d.tau, d.kappa = cd.tau, cd.kappa

    def calc_step_length(self, variables, step, step_direction, max_step_fraction=0.99):
        cv, cs, o = variables.cvars(), step.cvars(), C.c_double()
        _check(lib().chip_variables_calc_step_length(self._h, C.byref(cv), C.byref(cs), C.c_int32(step_direction),
                                                     C.c_double(max_step_fraction), C.byref(o)), "calc_step_length")
        return o.value

    def add_step(self, variables, step, alpha):
        cv, cs = variables.cvars(), step.cvars()
        _check(lib().chip_variables_add_step(self._h, C.byref(cv), C.byref(cs), C.c_double(alpha)), "add_step")
        variables.tau, variables.kappa = cv.tau, cv.kappa

    def symmetric_initialization(self, variables):
        cv = variables.cvars()
        _check(lib().chip_variables_symmetric_initialization(self._h, C.byref(cv)), "symmetric_initialization")
        variables.tau, variables.kappa = cv.tau, cv.kappa

    def unit_initialization(self, variables):
        cv = variables.cvars()
        _check(lib().chip_variables_unit_initialization(self._h, C.byref(cv)), "unit_initialization")
        variables.tau, variables.kappa = cv.tau, cv.kappa

    def barrier(self, variables, step, alpha):
        cv, cs, o = variables.cvars(), step.cvars(), C.c_double()
        _check(lib().chip_variables_barrier(self._h, C.byref(cv), C.byref(cs), C.c_double(alpha), C.byref(o)),
               "barrier")
        return o.value

    def rescale(self, variables):
        cv = variables.cvars()
        _check(lib().chip_variables_rescale(self._h, C.byref(cv)), "rescale")
        variables.tau, variables.kappa = cv.tau, cv.kappa

    def vec_norms(self, *arrays):
        """Euclidean norms of up to 8 DeviceArrays, one host synchronisation"""
        k = len(arrays)
        ptrs = (C.c_void_p * max(k, 1))(*[a.ptr for a in arrays])
        lens = (C.c_int64 * max(k, 1))(*[a.n for a in arrays])
        out = (C.c_double * max(k, 1))()
        _check(lib().chip_vec_norms(self._h, C.c_int32(k), ptrs, lens, out), "vec_norms")
        return [out[i] for i in range(k)]

    def update_data(self, P=None, A=None, q=None, b=None):
        args = [None if v is None else _f(v) for v in (P, A, q, b)]
        _check(lib().chip_kktsystem_update_data(self._h, *[None if v is None else _pf(v) for v in args]),
               "kktsystem_update_data")


# ---------------------------------------------------------------------------
# L4: DefaultSolver::new(P, q, A, b, cones, settings).solve() on the device (csrc/solver.cpp)
# ---------------------------------------------------------------------------
# SolverStatus (core/solver.rs:19-45), in the order of chip_solver_status
SOLVER_STATUS = ("Unsolved", "Solved", "PrimalInfeasible", "DualInfeasible", "AlmostSolved", "AlmostPrimalInfeasible",
                 "AlmostDualInfeasible", "MaxIterations", "MaxTime", "NumericalError", "InsufficientProgress",
                 "CallbackTerminated")


class SolverSettings(C.Structure):
    """chip_solver_settings: the DefaultSettings fields (settings.rs) the loop and the equilibration read, with the
    linear-system settings embedded as `linsys`"""
    _fields_ = [("linsys", Settings), ("max_iter", C.c_int32), ("equilibrate_enable", C.c_int32),
                ("time_limit", C.c_double), ("max_step_fraction", C.c_double), ("tol_gap_abs", C.c_double),
                ("tol_gap_rel", C.c_double), ("tol_feas", C.c_double), ("tol_infeas_abs", C.c_double),
                ("tol_infeas_rel", C.c_double), ("tol_ktratio", C.c_double), ("reduced_tol_gap_abs", C.c_double),
                ("reduced_tol_gap_rel", C.c_double), ("reduced_tol_feas", C.c_double),
                ("reduced_tol_infeas_abs", C.c_double), ("reduced_tol_infeas_rel", C.c_double),
                ("reduced_tol_ktratio", C.c_double), ("equilibrate_max_iter", C.c_int32), ("reserved0", C.c_int32),
                ("equilibrate_min_scaling", C.c_double), ("equilibrate_max_scaling", C.c_double),
                ("linesearch_backtrack_step", C.c_double), ("min_switch_step_length", C.c_double),
                ("min_terminate_step_length", C.c_double), ("presolve_enable", C.c_int32),
                ("chordal_decomposition_enable", C.c_int32), ("chordal_decomposition_merge_method", C.c_int32),
                ("chordal_decomposition_compact", C.c_int32), ("chordal_decomposition_complete_dual", C.c_int32),
                ("reserved1", C.c_int32)]

    @staticmethod
    def default(**kw):
        """DefaultSettings::default(); keyword arguments override fields (`device=` and the other linear-system
        fields go to .linsys).  Unlike the reference, presolve_enable and chordal_decomposition_enable default to 0.
        chordal_decomposition_merge_method takes the reference's strings ("none", "parent_child", "clique_graph") or
        the MERGE_* values; another string raises ValueError (settings.rs validation)."""
        s = SolverSettings()
        lib().chip_solver_settings_default(C.byref(s))
        _apply_settings(s, kw, "SolverSettings.default")
        return s


# chordal_decomposition_merge_method (CHIP_MERGE_*)
MERGE_NONE, MERGE_PARENT_CHILD, MERGE_CLIQUE_GRAPH = 0, 1, 2
MERGE_METHODS = {"none": MERGE_NONE, "parent_child": MERGE_PARENT_CHILD, "clique_graph": MERGE_CLIQUE_GRAPH}


def _apply_settings(s, kw, where):
    own = {f[0] for f in SolverSettings._fields_}
    lin = {f[0] for f in Settings._fields_}
    for k, v in kw.items():
        if k not in own and k not in lin:
            raise TypeError("%s: no setting named %r" % (where, k))
        if k == "chordal_decomposition_merge_method":
            if isinstance(v, str):
                if v not in MERGE_METHODS:
                    raise ValueError("%s: unknown chordal_decomposition_merge_method %r (one of %s)"
                                     % (where, v, ", ".join(sorted(MERGE_METHODS))))
                v = MERGE_METHODS[v]
            elif int(v) not in MERGE_METHODS.values():
                raise ValueError("%s: unknown chordal_decomposition_merge_method %r" % (where, v))
        setattr(s if k in own else s.linsys, k, v)


class TransformInfo(C.Structure):
    """chip_transform_info"""
    _fields_ = [("m_full", C.c_int64), ("m_reduced", C.c_int64), ("n_internal", C.c_int64), ("m_internal", C.c_int64),
                ("nnzA_internal", C.c_int64), ("psd_cones_decomposed", C.c_int64), ("psd_cones_added", C.c_int64),
                ("psd_cones_added_premerge", C.c_int64), ("largest_clique", C.c_int64),
                ("transform_time", C.c_double), ("completion_time", C.c_double)]


class SolutionInfo(C.Structure):
    """chip_solution_info"""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("obj_val", C.c_double),
                ("obj_val_dual", C.c_double), ("r_prim", C.c_double), ("r_dual", C.c_double),
                ("solve_time", C.c_double), ("setup_time", C.c_double), ("equilibration_time", C.c_double),
                ("iteration_time", C.c_double)]


class Solution:
    """DefaultSolution (solution.rs): x, s, z, status (the reference's status name), obj_val, obj_val_dual,
    iterations, r_prim, r_dual, solve_time (+ setup_time, equilibration_time, iteration_time)"""

    def __init__(self, x, s, z, info):
        self.x, self.s, self.z = x, s, z
        self.status = SOLVER_STATUS[info.status]
        for k in ("obj_val", "obj_val_dual", "iterations", "r_prim", "r_dual", "solve_time", "setup_time",
                  "equilibration_time", "iteration_time"):
            setattr(self, k, getattr(info, k))

    def __repr__(self):
        return "Solution(status=%s, iterations=%d, obj_val=%r)" % (self.status, self.iterations, self.obj_val)


class _DataUpdates:
    """the data updates of HipSolver and HipBatchSolver (default/data_updating.rs, python/impl_default_py.rs:699):
    update(), update_P / _A / _q / _b and update_settings over the C entry points <_UPDATE_PREFIX>P .. b, their _dev
    forms and <_UPDATE_PREFIX>settings.  The class has _h, settings, _len and _pattern; it may override _classify (a
    piece -> a form of classify_update) and _check_update_allowed (raises when the handle takes no updates)."""

    _UPDATE_PREFIX = None

    def update(self, P=None, q=None, A=None, b=None, settings=None):
        """solver.update(P=..., q=..., A=..., b=..., settings=...): each piece may be a CscMatrix with the setup's
        pattern (P, A), a full value vector, an (index, values) tuple, an empty vector (no-op) or torch tensors on the
        GPU (float64 values, int64 index); for a HipBatchSolver these address the stack, and a piece may also be a
        LIST with one entry per member (see HipBatchSolver).  Every piece is classified before any is applied; they
        are then applied in the order P, q, A, b, settings, and the first refusal raises ChipError (the pieces before
        it stay applied, as in the reference)."""
        self._check_update_allowed()
        forms = [(k, self._classify(k, v)) for k, v in (("P", P), ("q", q), ("A", A), ("b", b)) if v is not None]
        for k, f in forms:
            self._apply_update(k, f)
        if settings is not None:
            self.update_settings(settings)

    def update_P(self, data):
        self._apply_update("P", self._classify("P", data))

    def update_A(self, data):
        self._apply_update("A", self._classify("A", data))

    def update_q(self, data):
        self._apply_update("q", self._classify("q", data))

    def update_b(self, data):
        self._apply_update("b", self._classify("b", data))

    def _classify(self, key, data):
        return classify_update(key, data, self._len[key], self._pattern.get(key))

    def _check_update_allowed(self):
        pass

    def _apply_update(self, key, form):
        self._check_update_allowed()
        kind = form[0]
        if kind == "none":
            return
        idx, vals = form[1], form[2]
        name = self._UPDATE_PREFIX + key
        if kind in ("full", "partial"):
            _check(getattr(lib(), name)(self._h, None if idx is None else _pu(idx), _pf(vals), C.c_int64(len(vals))),
                   name)
            return
        import torch
        torch.cuda.current_stream(vals.device).synchronize()  # the values are written before the call reads them
        name += "_dev"
        _check(getattr(lib(), name)(self._h, None if idx is None else C.c_void_p(idx.data_ptr()),
                                    C.c_void_p(vals.data_ptr()), C.c_int64(vals.numel())), name)

    _REEQUILIBRATE = None

    def reequilibrate(self, P, q, A, b):
        """New FULL data on the handle's patterns, equilibrated from scratch on the device as a fresh handle would
        equilibrate it, without a new symbolic setup (<_REEQUILIBRATE>[_dev]): afterwards the handle holds what a fresh
        one created on these values would hold, later update()s scale with the new d, e, c, and the next solve()
        restarts from default_start.  Each of the four is a value vector (numpy, or a torch tensor on the host or on
        the GPU), P / A may also be a CscMatrix or a scipy matrix with the handle's pattern, and for a HipBatchSolver
        each may be a LIST with one full entry per member.  Any GPU tensor selects the device entry point, and then all four must be GPU
        tensors.  Everything is classified before the library is called: ChipError(ERR_DIM) for a wrong length or
        another pattern, TypeError for a partial form, a missing piece or a mix of host and GPU data."""
        self._check_update_allowed()
        forms = {}
        for k, v in (("P", P), ("q", q), ("A", A), ("b", b)):
            if v is None:
                raise TypeError("reequilibrate: %s is required (all four, in full)" % k)
            if k in "PA" and hasattr(v, "tocsc"):  # a scipy matrix: held to the handle's pattern like a CscMatrix
                v = CscMatrix.from_scipy(v)
            f = self._classify(k, v)
            if f[0] in ("partial", "dev_partial"):
                # (a batch's list of full members arrives as the positions 0 .. len - 1 in order)
                if f[0] == "dev_partial" or not np.array_equal(f[1], np.arange(self._len[k], dtype=u64)):
                    raise TypeError("reequilibrate: %s must be given in full" % k)
                f = ("full", None, f[2])
            if f[0] == "none" and self._len[k] != 0:
                raise ChipError(ERR_DIM, "reequilibrate: %s: 0 values for %d entries" % (k, self._len[k]))
            forms[k] = f
        on_gpu = [f[0] == "dev_full" for f in forms.values() if f[0] != "none"]
        if any(on_gpu) and not all(on_gpu):
            raise TypeError("reequilibrate: P, q, A, b must all be host arrays or all GPU tensors")
        name = self._REEQUILIBRATE
        if any(on_gpu):
            import torch
            dev = next(f[2].device for f in forms.values() if f[0] == "dev_full")
            torch.cuda.current_stream(dev).synchronize()  # the values are written before the call reads them
            pad = torch.zeros(2, dtype=torch.float64, device=dev)  # (an empty piece is still not NULL)
            keep = [pad if forms[k][0] == "none" else forms[k][2] for k in "PqAb"]
            name += "_dev"
            _check(getattr(lib(), name)(self._h, *[C.c_void_p(t.data_ptr()) for t in keep]), name)
        else:
            keep = [np.zeros(1) if forms[k][0] == "none" else forms[k][2] for k in "PqAb"]
            _check(getattr(lib(), name)(self._h, *[_pf(a) for a in keep]), name)
        self._after_reequilibrate()

    def _after_reequilibrate(self):
        pass

    def update_settings(self, settings=None, **kw):
        """DefaultSolver::update_settings (for a HipBatchSolver: of every member): a SolverSettings, or keyword
        overrides of the current settings (linear-system fields go to .linsys).  An immutable field that differs
        raises ChipError(ERR_ARG) and the settings stay as they were."""
        new = SolverSettings.from_buffer_copy(settings if settings is not None else self.settings)
        _apply_settings(new, kw, "update_settings")
        name = self._UPDATE_PREFIX + "settings"
        _check(getattr(lib(), name)(self._h, C.byref(new)), name)
        self.settings = new


class HipSolver(_DataUpdates):
    """DefaultSolver::new(P, q, A, b, cones, settings) (default/solver.rs) with every layer on the device: Ruiz
    equilibration, the interior-point loop, termination and the status.  P: n x n triu CscMatrix, A: m x n CscMatrix,
    cones as in HipKKTSolver ((tag, dim), (tag, dim, dim2), (tag, dim, dim2, alpha); GenPowerConeT =
    (5, len(alpha), dim2, alpha))."""

    _UPDATE_PREFIX = "chip_problem_update_"
    _REEQUILIBRATE = "chip_reequilibrate_problem"

    def __init__(self, P, q, A, b, cones, settings=None):
        n, m = P.n, A.m
        assert P.m == n and A.n == n
        q, b = _f(q), _f(b)
        assert len(q) == n and len(b) == m
        self.n, self.m = n, m
        self.settings = settings or SolverSettings.default()
        cones = [tuple(c) for c in cones]
        tags = np.array([c[0] for c in cones], dtype=np.int32)
        dims = np.array([c[1] for c in cones], dtype=np.int64)
        dims2 = np.array([c[2] if len(c) > 2 else 0 for c in cones], dtype=np.int64)
        alphas = np.array([c[3] if (len(c) > 3 and c[0] == PowerConeT) else 0.5 for c in cones], dtype=np.float64)
        gp = [np.asarray(c[3], dtype=np.float64) for c in cones if c[0] == GenPowerConeT]
        for c, a in zip([c for c in cones if c[0] == GenPowerConeT], gp):
            assert len(a) == c[1]
        gpa = _f(np.concatenate(gp)) if gp else None
        # the patterns, for update()'s check_equal_sparsity
        self._pattern = {"P": (P.m, P.n, P.colptr.copy(), P.rowval.copy()), "A": (A.m, A.n, A.colptr.copy(),
                                                                                 A.rowval.copy())}
        self._len = {"P": P.nnz, "A": A.nnz, "q": n, "b": m}
        self._h = C.c_void_p()
        _check(lib().chip_solver_create(C.byref(self._h), C.c_int64(n), C.c_int64(m), _pu(P.colptr), _pu(P.rowval),
                                        _pf(P.nzval), _pf(q), _pu(A.colptr), _pu(A.rowval), _pf(A.nzval), _pf(b),
                                        C.c_int64(len(cones)), tags.ctypes.data_as(P_I32), dims.ctypes.data_as(P_I64),
                                        dims2.ctypes.data_as(P_I64), _pf(alphas),
                                        None if gpa is None else _pf(gpa), C.byref(self.settings)),
               "chip_solver_create")

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().chip_solver_destroy(self._h)
            self._h = C.c_void_p()

    def solve(self):
        """IPSolver::solve -> Solution (a second call restarts from default_start).  x, s, z have the sizes of the
        problem passed in, whatever presolve or chordal decomposition did."""
        _check(lib().chip_solver_solve(self._h), "chip_solver_solve")
        x, s, z = np.zeros(self.n), np.zeros(self.m), np.zeros(self.m)
        info = SolutionInfo()
        _check(lib().chip_solver_get_solution(self._h, _pf(x), _pf(s), _pf(z), C.byref(info)),
               "chip_solver_get_solution")
        return Solution(x, s, z, info)

    def solution_dev(self):
        """(x, s, z) of the last solve as non-owning DeviceArray views (valid until the next solve)"""
        px, ps, pz = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().chip_solver_get_solution_dev(self._h, C.byref(px), C.byref(ps), C.byref(pz)),
               "chip_solver_get_solution_dev")
        return (DeviceArray.view(px.value, self.n), DeviceArray.view(ps.value, self.m),
                DeviceArray.view(pz.value, self.m))

    def equilibration(self):
        """DefaultEquilibrationData: (d, e, c) of the internal problem (n_internal, m_internal of transform_info)"""
        t = self.transform_info()
        d, e, c = np.zeros(t["n_internal"]), np.zeros(t["m_internal"]), C.c_double()
        _check(lib().chip_solver_get_equilibration(self._h, _pf(d), _pf(e), C.byref(c)),
               "chip_solver_get_equilibration")
        return d, e, c.value

    def _check_update_allowed(self):
        if not self.is_data_update_allowed():  # data_updating.rs: checked before the data is looked at
            raise UpdateNotAllowedError(ERR_UPDATE_NOT_ALLOWED, "update: presolve or chordal decomposition is active")

    def transform_info(self):
        """what presolve and chordal decomposition did at setup (chip_transform_get_info) as a dict"""
        t = TransformInfo()
        _check(lib().chip_transform_get_info(self._h, C.byref(t)), "chip_transform_get_info")
        return {f[0]: getattr(t, f[0]) for f in TransformInfo._fields_}

    def is_data_update_allowed(self):
        allowed = C.c_int32()
        _check(lib().chip_problem_update_allowed(self._h, C.byref(allowed)), "chip_problem_update_allowed")
        return bool(allowed.value)

    def internal_solution(self):
        """test hook: the internal variables of the last solve, unscaled: (x2, s2, z2) of n_internal / m_internal"""
        t = self.transform_info()
        x, s, z = np.zeros(t["n_internal"]), np.zeros(t["m_internal"]), np.zeros(t["m_internal"])
        _check(lib().chip_debug_solver_internal_solution(self._h, _pf(x), _pf(s), _pf(z)),
               "chip_debug_solver_internal_solution")
        return x, s, z

    def scaled_state(self):
        """test hook: what the last solve left in the handle, SCALED (chip_debug_solver_scaled_state): a dict with the
        iterate x, s, z, tau, kappa, the inverse scalings dinv, einv and the info in its flat 21-double form (cost_primal,
        cost_dual, res_primal, res_dual, res_primal_inf, res_dual_inf, gap_abs, gap_rel, ktratio, six prev_ scalars,
        r_tau, q'x, b'z, s'z, x'Px, status)"""
        t = self.transform_info()
        n, m = t["n_internal"], t["m_internal"]
        x, s, z, tk, dinv, einv, info = (np.zeros(k) for k in (n, m, m, 2, n, m, 21))
        _check(lib().chip_debug_solver_scaled_state(self._h, _pf(x), _pf(s), _pf(z), _pf(tk), _pf(dinv), _pf(einv),
                                                    _pf(info)), "chip_debug_solver_scaled_state")
        return dict(x=x, s=s, z=z, tau=float(tk[0]), kappa=float(tk[1]), dinv=dinv, einv=einv, info=info)

    def scaled_data(self):
        """solver.data as the solver holds it, after the transforms and the equilibration: (P.nzval, A.nzval, q, b)
        of the internal problem (the original sizes unless a transform is active)"""
        t = self.transform_info()
        if t["m_internal"] == self.m and t["n_internal"] == self.n:
            Px, Ax = np.zeros(self._len["P"]), np.zeros(self._len["A"])
        else:  # P keeps its entries (zero-padded columns); A is the internal one
            Px, Ax = np.zeros(self._len["P"]), np.zeros(t["nnzA_internal"])
        q, b = np.zeros(t["n_internal"]), np.zeros(t["m_internal"])
        _check(lib().chip_problem_get_scaled(self._h, _pf(Px), _pf(Ax), _pf(q), _pf(b)), "chip_problem_get_scaled")
        return Px, Ax, q, b


def batch_stack(problems):
    """the block-diagonal stack of a list of (P, q, A, b, cones) with CscMatrix P (n x n triu) and A (m x n): a dict
    with n_part, m_part, n, m, P and A as (colptr, rowval, nzval) uint64 / float64 arrays, q, b and the concatenated
    cones (csc/block_concatenate.rs's layout: member k's columns and rows follow those of members 0 .. k-1)"""
    n_part, m_part, cones = [], [], []
    pc, pr, pv, ac, ar, av, qs, bs = [np.zeros(1, dtype=u64)], [], [], [np.zeros(1, dtype=u64)], [], [], [], []
    noff = moff = 0
    pnz = anz = 0
    for k, pb in enumerate(problems):
        P, q, A, b, cn = pb
        n, m = P.n, A.m
        if P.m != n or A.n != n:
            raise ValueError("batch member %d: P must be n x n and A m x n" % k)
        q, b = _f(q), _f(b)
        if len(q) != n or len(b) != m:
            raise ValueError("batch member %d: q must have n and b m entries" % k)
        pc.append(_u(P.colptr)[1:] + u64(pnz))
        pr.append(_u(P.rowval) + u64(noff))
        pv.append(_f(P.nzval))
        ac.append(_u(A.colptr)[1:] + u64(anz))
        ar.append(_u(A.rowval) + u64(moff))
        av.append(_f(A.nzval))
        qs.append(q)
        bs.append(b)
        cones.extend(tuple(c) for c in cn)
        n_part.append(n)
        m_part.append(m)
        noff, moff, pnz, anz = noff + n, moff + m, pnz + P.nnz, anz + A.nnz
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=dt)  # noqa: E731
    return dict(n_part=np.array(n_part, dtype=np.int64), m_part=np.array(m_part, dtype=np.int64), n=noff, m=moff,
                P=(cat(pc, u64), cat(pr, u64), cat(pv, f64)), A=(cat(ac, u64), cat(ar, u64), cat(av, f64)),
                q=cat(qs, f64), b=cat(bs, f64), cones=cones)


class HipBatchSolver(_DataUpdates):
    """many independent problems in ONE batched interior-point solve on the device (chip_batch_*): every member keeps
    its own tau, kappa, mu, sigma, step length, termination and status.  problems: a list of (P, q, A, b, cones) as
    HipSolver takes them, with Zero / Nonnegative / SecondOrder cones (and PSDTriangle cones with cones="symmetric");
    one settings for every member.

    Data updates (chip_bdata_*; update(), update_P / _A / _q / _b): new values on the stack's fixed patterns, then
    solve() again.  Each piece is a stacked value vector (or a CscMatrix with the stack's pattern), an (index, values)
    tuple of stack positions, an empty vector (no-op), torch tensors on the GPU -- or a LIST with one entry per member,
    each None (member untouched), a value vector of the member's own length (or its CscMatrix) or a member-local
    (index, values); the list is translated with the stack's offsets into one partial update, so updating 3 of 1024
    members moves only their values."""

    _UPDATE_PREFIX = "chip_bdata_update_"
    _REEQUILIBRATE = "chip_reequilibrate_bdata"
    _CREATE = {"basic": "chip_batch_create", "symmetric": "chip_bsym_create"}

    def __init__(self, problems, settings=None, cones="basic"):
        """cones: "basic" (Zero / Nonnegative / SecondOrder members, chip_batch_create) or "symmetric" (PSDTriangle
        members as well, chip_bsym_create: the same solver and the same methods; a member that owns a PSD cone has no
        derivative, valid[k] = 0)"""
        if cones not in self._CREATE:
            raise ValueError('cones must be "basic" or "symmetric", not %r' % (cones,))
        create = self._CREATE[cones]
        problems = list(problems)
        st = batch_stack(problems)
        self.stack = st
        self.settings = settings or SolverSettings.default()
        self.n_part, self.m_part = st["n_part"], st["m_part"]
        # for update(): the stack's lengths and patterns, and the members' offsets, lengths and patterns
        n, m = st["n"], st["m"]
        self._len = {"P": len(st["P"][2]), "A": len(st["A"][2]), "q": n, "b": m}
        self._pattern = {"P": (n, n, st["P"][0], st["P"][1]), "A": (m, n, st["A"][0], st["A"][1])}
        part = {"P": [pb[0].nnz for pb in problems], "A": [pb[2].nnz for pb in problems], "q": self.n_part,
                "b": self.m_part}
        self._offsets = {k: np.concatenate([[0], np.cumsum(np.asarray(v, dtype=np.int64))]).astype(np.int64)
                         for k, v in part.items()}
        self._mpattern = {"P": [(pb[0].m, pb[0].n, pb[0].colptr.copy(), pb[0].rowval.copy()) for pb in problems],
                          "A": [(pb[2].m, pb[2].n, pb[2].colptr.copy(), pb[2].rowval.copy()) for pb in problems]}
        self.generation = 0  # counts the solves (layer.BatchQPFunction checks that its backward meets its own solve)
        tags, dims, dims2, alphas = _cone_arrays(st["cones"])
        self._h = C.c_void_p()
        Pp, Pi, Px = st["P"]
        Ap, Ai, Ax = st["A"]
        _check(getattr(lib(), create)(C.byref(self._h), C.c_int64(len(problems)),
                                      self.n_part.ctypes.data_as(P_I64), self.m_part.ctypes.data_as(P_I64),
                                      C.c_int64(st["n"]), C.c_int64(st["m"]), _pu(Pp), _pu(Pi), _pf(Px), _pf(st["q"]),
                                      _pu(Ap), _pu(Ai), _pf(Ax), _pf(st["b"]), C.c_int64(len(tags)),
                                      tags.ctypes.data_as(P_I32), dims.ctypes.data_as(P_I64),
                                      dims2.ctypes.data_as(P_I64), _pf(alphas), None, C.byref(self.settings)),
               create)

    def __len__(self):
        return len(self.n_part)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().chip_batch_destroy(self._h)
            self._h = C.c_void_p()

    def _solve(self):
        _check(lib().chip_batch_solve(self._h), "chip_batch_solve")
        self.generation += 1

    def solve(self):
        """the batched IPSolver::solve -> one Solution per member, in input order"""
        self._solve()
        out = []
        for k in range(len(self)):
            x, s, z = np.zeros(self.n_part[k]), np.zeros(self.m_part[k]), np.zeros(self.m_part[k])
            info = SolutionInfo()
            _check(lib().chip_batch_get_solution(self._h, C.c_int64(k), _pf(x), _pf(s), _pf(z), C.byref(info)),
                   "chip_batch_get_solution")
            out.append(Solution(x, s, z, info))
        return out

    def infos(self):
        """the members' chip_solution_info of the last solve"""
        arr = (SolutionInfo * max(len(self), 1))()
        _check(lib().chip_batch_get_info(self._h, arr), "chip_batch_get_info")
        return [arr[k] for k in range(len(self))]

    def solutions_dev(self):
        """the stacked (x, s, z) of the last solve as non-owning DeviceArray views (valid until the next solve)"""
        px, ps, pz = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().chip_batch_get_solution_dev(self._h, C.byref(px), C.byref(ps), C.byref(pz)),
               "chip_batch_get_solution_dev")
        return (DeviceArray.view(px.value, self.stack["n"]), DeviceArray.view(ps.value, self.stack["m"]),
                DeviceArray.view(pz.value, self.stack["m"]))

    def equilibration(self, k):
        """member k's (d, e, c)"""
        d, e, c = np.zeros(self.n_part[k]), np.zeros(self.m_part[k]), C.c_double()
        _check(lib().chip_batch_get_equilibration(self._h, C.c_int64(k), _pf(d), _pf(e), C.byref(c)),
               "chip_batch_get_equilibration")
        return d, e, c.value

    def _classify(self, key, data):
        if isinstance(data, list) and len(data) > 0 and not np.isscalar(data[0]):
            return batch_list_update(key, data, self._offsets[key], self._mpattern.get(key))
        return super()._classify(key, data)

    def _after_reequilibrate(self):
        self.generation += 1  # (a backward of a solve before it no longer meets its own data)

    def scaled_data(self):
        """the stack's data as the handle holds it after the equilibration, and the members' norms of the unscaled
        q and b: (P.nzval, A.nzval, q, b, normq, normb)"""
        Px, Ax = np.zeros(self._len["P"]), np.zeros(self._len["A"])
        q, b = np.zeros(self._len["q"]), np.zeros(self._len["b"])
        nq, nb = np.zeros(len(self)), np.zeros(len(self))
        _check(lib().chip_bdata_get_scaled(self._h, _pf(Px), _pf(Ax), _pf(q), _pf(b), _pf(nq), _pf(nb)),
               "chip_bdata_get_scaled")
        return Px, Ax, q, b, nq, nb

    # ---- gradients (chip_bgrad_*): dL/d(x, z, s) of every member -> dL/d(q, b, P, A) of every member --------------
    def solve_torch(self):
        """solve() without the per-member host copies: the stacked (x, s, z) as torch tensors on the GPU (copies of
        the handle's buffers, so they outlive the next solve); statuses with infos()"""
        self._solve()
        px, ps, pz = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().chip_batch_get_solution_dev(self._h, C.byref(px), C.byref(ps), C.byref(pz)),
               "chip_batch_get_solution_dev")
        n, m = self._len["q"], self._len["b"]
        return _torch_copy(px.value, n, "float64"), _torch_copy(ps.value, m, "float64"), \
            _torch_copy(pz.value, m, "float64")

    def _grad_input(self, name, g, key, fn="backward"):
        """one incoming gradient (or, for jvp, one piece of a direction) -> ("none", None), ("host", float64 array) or
        ("dev", contiguous GPU tensor)"""
        name = "%s %s" % (fn, name)
        length = self._len[key]
        if g is None:
            return ("none", None)
        if isinstance(g, list) and len(g) > 0 and not np.isscalar(g[0]):
            off = self._offsets[key]
            if len(g) != len(self):
                raise ChipError(ERR_DIM, "%s: %d list entries for %d members" % (name, len(g), len(self)))
            out = np.zeros(length)
            for k, piece in enumerate(g):
                if piece is None:
                    continue
                if _is_torch(piece) and piece.is_cuda:
                    raise TypeError("%s: member %d: the entries of a list are host arrays" % (name, k))
                v = _host_array(piece, name, False)
                if v.size != off[k + 1] - off[k]:
                    raise ChipError(ERR_DIM, "%s: member %d: %d values for %d entries"
                                    % (name, k, v.size, off[k + 1] - off[k]))
                out[off[k]:off[k + 1]] = v
            return ("host", out)
        if _is_torch(g) and g.is_cuda:
            import torch
            if g.dtype != torch.float64:
                raise TypeError("%s: GPU values must be float64, not %s" % (name, g.dtype))
            if g.dim() != 1 or g.numel() != length:
                raise ChipError(ERR_DIM, "%s: a vector of %d values is needed" % (name, length))
            return ("dev", g.detach().contiguous())
        v = _host_array(g, name, False)
        if v.size != length:
            raise ChipError(ERR_DIM, "%s: %d values for %d entries" % (name, v.size, length))
        return ("host", _f(v))

    def _derivative(self, fn, inputs, values, entry, outputs, result):
        """one derivative pass `fn` ("backward" / "jvp"): inputs = the (name, key) of its arguments, values = what the
        caller gave for them, entry = the C calls "chip_bgrad" / "chip_bjvp" + (pass, pass_dev, "get", "get_dev"),
        outputs = the keys of the results' lengths, result = the class that carries them"""
        run, run_dev, get, get_dev = entry
        forms = [self._grad_input(nm, g, key, fn) for (nm, key), g in zip(inputs, values)]
        kinds = {f[0] for f in forms} - {"none"}
        if len(kinds) > 1:
            names = [nm for nm, _ in inputs]
            raise TypeError("%s: %s and %s must all be host arrays or all GPU tensors"
                            % (fn, ", ".join(names[:-1]), names[-1]))
        lens = [self._len[key] for key in outputs]
        valid = np.zeros(len(self), dtype=np.int32)
        L = lib()
        if kinds == {"dev"}:
            import torch
            dev = [f[1] for f in forms if f[0] == "dev"][0].device
            torch.cuda.current_stream(dev).synchronize()  # the values are written before the call reads them
            ptr = [None if f[0] == "none" else C.c_void_p(f[1].data_ptr()) for f in forms]
            _check(getattr(L, run_dev)(self._h, *ptr), run_dev)
            out = [C.c_void_p() for _ in lens]
            _check(getattr(L, get_dev)(self._h, *[C.byref(o) for o in out], None), get_dev)
            _check(getattr(L, get)(self._h, *[None] * len(lens), valid.ctypes.data_as(P_I32)), get)
            return result(*[_torch_copy(o.value, ln, "float64", dev) for o, ln in zip(out, lens)], valid, self._offsets)
        ptr = [None if f[0] == "none" else _pf(f[1]) for f in forms]
        _check(getattr(L, run)(self._h, *ptr), run)
        res = [np.zeros(ln) for ln in lens]
        _check(getattr(L, get)(self._h, *[_pf(v) for v in res], valid.ctypes.data_as(P_I32)), get)
        return result(*res, valid, self._offsets)

    def backward(self, gx=None, gz=None, gs=None):
        """the gradients of a loss with respect to q, b, P and A of every member from its gradients with respect to
        the members' x, z and s of the last solve() (stacked vectors; None = zeros): numpy arrays, torch tensors on
        the GPU (float64; the result then holds torch tensors on the GPU and nothing crosses to the host), or a list
        with one entry per member (None = zeros for that member; the entries are HOST vectors, as in update()'s list
        form -- gradients that live on the GPU go in as stacked tensors).  Returns a BatchGradient.  Members that did not end
        Solved, or own a SecondOrder or PSDTriangle cone, have valid[k] = 0 and exact zeros.  ChipError(ERR_ARG) before
        a solve and after an update that was not followed by a solve."""
        return self._derivative("backward", (("gx", "q"), ("gz", "b"), ("gs", "b")), (gx, gz, gs),
                                ("chip_bgrad_backward", "chip_bgrad_backward_dev", "chip_bgrad_get",
                                 "chip_bgrad_get_dev"), "qbPA", BatchGradient)

    # ---- tangents (chip_bjvp_*): a direction in (q, b, P, A) of every member -> (dx, dz, ds) of every member ---------
    def jvp(self, dq=None, db=None, dP=None, dA=None):
        """the forward-mode derivative of the last solve(): how x, z and s of every member move when its q, b, P and A
        move along (dq, db, dP, dA) -- stacked vectors, dP / dA in the order of the stack's nzval (the positions
        update_P / update_A index; a stored (i, j), i < j, of P stands for both triangles); None = zeros.  The forms
        are backward()'s: numpy arrays, float64 torch tensors on the GPU (the result then holds torch tensors on the
        GPU and nothing crosses to the host), or a list with one host entry per member (None = zeros for that member).
        Returns a BatchTangent.  Members that did not end Solved, or own a SecondOrder cone, have valid[k] = 0 and
        exact zeros.  The first jvp (or backward) after a solve factors K at the final iterates; every further jvp of
        that solve costs one KKT solve.  ChipError(ERR_ARG) before a solve and after an update that was not followed
        by a solve."""
        return self._derivative("jvp", (("dq", "q"), ("db", "b"), ("dP", "P"), ("dA", "A")), (dq, db, dP, dA),
                                ("chip_bjvp_apply", "chip_bjvp_apply_dev", "chip_bjvp_get", "chip_bjvp_get_dev"),
                                "qbb", BatchTangent)

    # ---- blocks of tangents and the members' Jacobians (chip_bjac_*) ------------------------------------------------
    def _block_input(self, name, g, key, fn="jvp_block"):
        """one piece of a block of directions (or, for backward_block, of cotangents) -> ("none", None), ("host",
        float64 array [K, len]) or ("dev", contiguous GPU tensor [K, len])"""
        name = "%s %s" % (fn, name)
        length = self._len[key]
        if g is None:
            return ("none", None)
        if _is_torch(g) and g.is_cuda:
            import torch
            if g.dtype != torch.float64:
                raise TypeError("%s: GPU values must be float64, not %s" % (name, g.dtype))
            if g.dim() != 2 or g.shape[1] != length:
                raise ChipError(ERR_DIM, "%s: a [K, %d] matrix is needed" % (name, length))
            return ("dev", g.detach().contiguous())
        a = np.asarray(g.detach().numpy() if _is_torch(g) else g)
        if a.dtype != f64:
            raise TypeError("%s: host values must be float64, not %s" % (name, a.dtype))
        if a.ndim != 2 or a.shape[1] != length:
            raise ChipError(ERR_DIM, "%s: a [K, %d] matrix is needed" % (name, length))
        return ("host", _f(a))

    def _block_result(self, ndir, device=None):
        """(dx[ndir, n], dz[ndir, m], ds[ndir, m]) of the last block: numpy arrays, or copies on the GPU `device`"""
        L = lib()
        lens = [self._len[key] for key in "qbb"]
        if device is None:
            res = [np.zeros((ndir, ln)) for ln in lens]
            _check(L.chip_bjac_get(self._h, *[_pf(v) for v in res], None), "chip_bjac_get")
            return res
        out = [C.c_void_p() for _ in lens]
        _check(L.chip_bjac_get_dev(self._h, *[C.byref(o) for o in out], None), "chip_bjac_get_dev")
        return [_torch_copy(o.value, ndir * ln, "float64", device).view(ndir, ln) for o, ln in zip(out, lens)]

    def _block_valid(self):
        valid = np.zeros(len(self), dtype=np.int32)
        _check(lib().chip_bjac_get(self._h, None, None, None, valid.ctypes.data_as(P_I32)), "chip_bjac_get")
        return valid

    def jvp_block(self, dq=None, db=None, dP=None, dA=None):
        """K directions at once: jvp() with every piece a [K, len] matrix (row t = direction t; float64 numpy arrays,
        or contiguous float64 torch tensors on the GPU: the result then holds GPU tensors and nothing crosses to the
        host); None = zeros in every direction; at least one piece is given, all given pieces share K >= 1 and are all
        host or all GPU.  Up to 16 directions are one call with one host synchronisation (chip_bjac_apply); more are
        cut into calls of 16.  Returns a BatchTangentBlock.  Validity, zeros and refusals as for jvp()."""
        names = (("dq", "q"), ("db", "b"), ("dP", "P"), ("dA", "A"))
        forms = [self._block_input(nm, g, key) for (nm, key), g in zip(names, (dq, db, dP, dA))]
        kinds = {f[0] for f in forms} - {"none"}
        if not kinds:
            raise ChipError(ERR_DIM, "jvp_block: at least one piece is needed (it gives the number of directions)")
        if len(kinds) > 1:
            raise TypeError("jvp_block: dq, db, dP and dA must all be host arrays or all GPU tensors")
        counts = {int(f[1].shape[0]) for f in forms if f[0] != "none"}
        if len(counts) != 1 or min(counts) < 1:
            raise ChipError(ERR_DIM, "jvp_block: the pieces must share one number of directions K >= 1, not %s"
                            % sorted(counts))
        K = counts.pop()
        on_dev = kinds == {"dev"}
        device = None
        if on_dev:
            import torch
            device = [f[1] for f in forms if f[0] == "dev"][0].device
            torch.cuda.current_stream(device).synchronize()  # the values are written before the call reads them
        L = lib()
        parts = []
        for t0 in range(0, K, BJAC_MAX_DIR):
            nd = min(BJAC_MAX_DIR, K - t0)
            if on_dev:
                ptr = [None if f[0] == "none" else C.c_void_p(f[1].data_ptr() + 8 * t0 * f[1].shape[1]) for f in forms]
                _check(L.chip_bjac_apply_dev(self._h, C.c_int32(nd), *ptr), "chip_bjac_apply_dev")
            else:
                rows = [None if f[0] == "none" else f[1][t0:t0 + nd] for f in forms]
                _check(L.chip_bjac_apply(self._h, C.c_int32(nd), *[None if r is None else _pf(r) for r in rows]),
                       "chip_bjac_apply")
            parts.append(self._block_result(nd, device))
        if on_dev:
            import torch
            cat = lambda vs: vs[0] if len(vs) == 1 else torch.cat(vs, dim=0)  # noqa: E731
        else:
            cat = lambda vs: vs[0] if len(vs) == 1 else np.concatenate(vs, axis=0)  # noqa: E731
        return BatchTangentBlock(*[cat([p[i] for p in parts]) for i in range(3)], self._block_valid(), self._offsets)

    def member_jacobians(self, wrt="q", torch=False):
        """the Jacobians of every member's solution with respect to its own q (wrt="q") or b (wrt="b"): a list with
        one entry per member, None where the member has no derivative (valid[k] == 0), else (dx_dw [n_k x w_k],
        dz_dw [m_k x w_k], ds_dw [m_k x w_k]) with w_k the member's number of entries of q / b -- numpy arrays, or with
        torch=True tensors on the GPU (nothing crosses to the host).  K is block-diagonal over the members, so one
        direction that holds unit vector j of every member's own q yields column j of every Jacobian: the cost is
        ceil(max_k w_k / 16) calls of chip_bjac_units -- max_k w_k refined solves, not sum_k w_k."""
        if wrt not in ("q", "b"):
            raise ValueError("member_jacobians: wrt is \"q\" or \"b\"")
        piece = 0 if wrt == "q" else 1
        widths = [int(v) for v in (self.n_part if piece == 0 else self.m_part)]
        wmax = max(widths)
        device = None
        if torch:
            import torch as th
            device = th.device("cuda")
            new = lambda r, c: th.zeros((r, c), dtype=th.float64, device=device)  # noqa: E731
        else:
            new = lambda r, c: np.zeros((r, c))  # noqa: E731
        out = [tuple(new(int(r), w) for r in (self.n_part[k], self.m_part[k], self.m_part[k]))
               for k, w in enumerate(widths)]
        off = [self._offsets[key] for key in "qbb"]
        valid = None
        for first in range(0, max(wmax, 1), BJAC_MAX_DIR):  # (no entries at all: one call, for the valid flags)
            nd = max(1, min(BJAC_MAX_DIR, wmax - first))
            _check(lib().chip_bjac_units(self._h, C.c_int32(piece), C.c_int64(first), C.c_int32(nd)),
                   "chip_bjac_units")
            block = self._block_result(nd, device)
            if valid is None:
                valid = self._block_valid()
            for k, w in enumerate(widths):
                cols = min(nd, w - first)
                if cols <= 0 or not valid[k]:
                    continue
                for mat, res, o in zip(out[k], block, off):
                    mat[:, first:first + cols] = res[:cols, int(o[k]):int(o[k + 1])].T
        return [mats if valid[k] else None for k, mats in enumerate(out)]

    # ---- blocks of cotangents and the rows of the members' Jacobians (chip_bvjp_*) ----------------------------------
    @staticmethod
    def _want_bits(want, fn):
        if not isinstance(want, str) or not want or any(ch not in "qbPA" for ch in want):
            raise ValueError("%s: the wanted pieces are a non-empty subset of \"qbPA\"" % fn)
        return sum(1 << "qbPA".index(ch) for ch in set(want))

    def _vjp_result(self, ndir, bits, device=None):
        """[dq[ndir, n], db[ndir, m], dP[ndir, nnz(P)], dA[ndir, nnz(A)]] of the last block, None for a piece that is
        not in `bits`: numpy arrays, or copies on the GPU `device`"""
        L = lib()
        lens = [self._len[key] for key in "qbPA"]
        has = [bool((bits >> i) & 1) for i in range(4)]
        if device is None:
            res = [np.zeros((ndir, ln)) if h else None for ln, h in zip(lens, has)]
            _check(L.chip_bvjp_get(self._h, *[None if v is None else _pf(v) for v in res], None), "chip_bvjp_get")
            return res
        out = [C.c_void_p() for _ in lens]
        _check(L.chip_bvjp_get_dev(self._h, *[C.byref(o) for o in out], None), "chip_bvjp_get_dev")
        return [_torch_copy(o.value, ndir * ln, "float64", device).view(ndir, ln) if h else None
                for o, ln, h in zip(out, lens, has)]

    def _vjp_valid(self):
        valid = np.zeros(len(self), dtype=np.int32)
        _check(lib().chip_bvjp_get(self._h, None, None, None, None, valid.ctypes.data_as(P_I32)), "chip_bvjp_get")
        return valid

    def backward_block(self, gx=None, gz=None, gs=None, want="qbPA"):
        """K cotangents at once: backward() with every piece a [K, len] matrix (row t = cotangent t; float64 numpy
        arrays, or contiguous float64 torch tensors on the GPU: the result then holds GPU tensors and nothing crosses
        to the host); None = zeros in every cotangent; at least one piece is given, all given pieces share K >= 1 and
        are all host or all GPU.  want: the pieces of the result to compute, a non-empty subset of "qbPA"; the others
        are None in the result and cost neither time nor memory.  Up to 16 cotangents are one call with one host
        synchronisation (chip_bvjp_apply); more are cut into calls of 16.  K is factored at the final iterates only by
        the first derivative call after a solve.  Returns a BatchGradientBlock.  Validity, zeros and refusals as for
        backward()."""
        bits = self._want_bits(want, "backward_block")
        names = (("gx", "q"), ("gz", "b"), ("gs", "b"))
        forms = [self._block_input(nm, g, key, "backward_block") for (nm, key), g in zip(names, (gx, gz, gs))]
        kinds = {f[0] for f in forms} - {"none"}
        if not kinds:
            raise ChipError(ERR_DIM, "backward_block: at least one piece is needed (it gives the number of cotangents)")
        if len(kinds) > 1:
            raise TypeError("backward_block: gx, gz and gs must all be host arrays or all GPU tensors")
        counts = {int(f[1].shape[0]) for f in forms if f[0] != "none"}
        if len(counts) != 1 or min(counts) < 1:
            raise ChipError(ERR_DIM, "backward_block: the pieces must share one number of cotangents K >= 1, not %s"
                            % sorted(counts))
        K = counts.pop()
        on_dev = kinds == {"dev"}
        device = None
        if on_dev:
            import torch
            device = [f[1] for f in forms if f[0] == "dev"][0].device
            torch.cuda.current_stream(device).synchronize()  # the values are written before the call reads them
        L = lib()
        parts = []
        for t0 in range(0, K, BVJP_MAX_DIR):
            nd = min(BVJP_MAX_DIR, K - t0)
            if on_dev:
                ptr = [None if f[0] == "none" else C.c_void_p(f[1].data_ptr() + 8 * t0 * f[1].shape[1]) for f in forms]
                _check(L.chip_bvjp_apply_dev(self._h, C.c_int32(nd), C.c_int32(bits), *ptr), "chip_bvjp_apply_dev")
            else:
                rows = [None if f[0] == "none" else f[1][t0:t0 + nd] for f in forms]
                _check(L.chip_bvjp_apply(self._h, C.c_int32(nd), C.c_int32(bits),
                                         *[None if r is None else _pf(r) for r in rows]), "chip_bvjp_apply")
            parts.append(self._vjp_result(nd, bits, device))
        if on_dev:
            import torch
            cat = lambda vs: vs[0] if len(vs) == 1 else torch.cat(vs, dim=0)  # noqa: E731
        else:
            cat = lambda vs: vs[0] if len(vs) == 1 else np.concatenate(vs, axis=0)  # noqa: E731
        res = [None if parts[0][i] is None else cat([p[i] for p in parts]) for i in range(4)]
        return BatchGradientBlock(*res, self._vjp_valid(), self._offsets)

    def member_jacobian_rows(self, of="x", wrt="qb", torch=False):
        """the Jacobians of every member's x (of="x"), z or s with respect to its own q, b and the stored entries of
        its P and A (wrt: a non-empty subset of "qbPA"), built row by row: a list with one entry per member, None
        where the member has no derivative (valid[k] == 0), else a dict that maps each key of wrt to a matrix
        [len(of)_k x w_k], w_k the member's number of entries of q / b, or of stored entries of P / A in the order of
        its own nzval -- numpy arrays, or with torch=True tensors on the GPU (nothing crosses to the host).  A stored
        (i, j), i < j, of P stands for both triangles.  K is block-diagonal over the members, so one cotangent that
        holds unit vector j of every member's own x yields row j of every Jacobian, with respect to all of wrt at
        once: the cost is ceil(max_k len(of)_k / 16) calls of chip_bvjp_units -- max_k len(of)_k refined solves."""
        if of not in ("x", "z", "s"):
            raise ValueError("member_jacobian_rows: of is \"x\", \"z\" or \"s\"")
        bits = self._want_bits(wrt, "member_jacobian_rows")
        keys = [key for key in "qbPA" if key in wrt]
        piece = "xzs".index(of)
        heights = [int(v) for v in (self.n_part if piece == 0 else self.m_part)]
        hmax = max(heights)
        device = None
        if torch:
            import torch as th
            device = th.device("cuda")
            new = lambda r, c: th.zeros((r, c), dtype=th.float64, device=device)  # noqa: E731
        else:
            new = lambda r, c: np.zeros((r, c))  # noqa: E731
        off = {key: self._offsets[key] for key in keys}
        out = [{key: new(hk, int(off[key][k + 1]) - int(off[key][k])) for key in keys} for k, hk in enumerate(heights)]
        valid = None
        for first in range(0, max(hmax, 1), BVJP_MAX_DIR):  # (no entries at all: one call, for the valid flags)
            nd = max(1, min(BVJP_MAX_DIR, hmax - first))
            _check(lib().chip_bvjp_units(self._h, C.c_int32(piece), C.c_int64(first), C.c_int32(nd), C.c_int32(bits)),
                   "chip_bvjp_units")
            block = dict(zip("qbPA", self._vjp_result(nd, bits, device)))
            if valid is None:
                valid = self._vjp_valid()
            for k, hk in enumerate(heights):
                rows = min(nd, hk - first)
                if rows <= 0 or not valid[k]:
                    continue
                for key in keys:
                    o = off[key]
                    out[k][key][first:first + rows, :] = block[key][:rows, int(o[k]):int(o[k + 1])]
        return [mats if valid[k] else None for k, mats in enumerate(out)]

    # ---- test hooks (include/clarabel_hip_testing.h) ----
    def debug_vjp_rhs(self, form, ndir, s, z, valid, gx=None, gz=None, gs=None):
        """the right-hand side pass of a block of cotangents alone (no solve needed): form 1 the block launcher once,
        form 0 the single launcher once per cotangent; pieces [ndir, len] -> the scaled (rx[ndir, n] = d gx,
        ws[ndir, m] = gs / e, rz[ndir, m] = e gz / c)"""
        keep = [None if v is None else _f(v) for v in (s, z, gx, gz, gs)]
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        n, m = self._len["q"], self._len["b"]
        rx, ws, rz = np.zeros((ndir, n)), np.zeros((ndir, m)), np.zeros((ndir, m))
        ptr = [None if v is None else _pf(v) for v in keep]
        _check(lib().chip_debug_batch_vjp_rhs(self._h, C.c_int32(form), C.c_int32(ndir), ptr[0], ptr[1],
                                              valid.ctypes.data_as(P_I32), *ptr[2:], _pf(rx), _pf(ws), _pf(rz)),
               "chip_debug_batch_vjp_rhs")
        return rx, ws, rz

    def debug_vjp_units(self, piece, first, ndir, valid):
        """the unit right-hand sides of a block of cotangents alone (no solve needed) -> the scaled (rx[ndir, n],
        ws[ndir, m], rz[ndir, m])"""
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        n, m = self._len["q"], self._len["b"]
        rx, ws, rz = np.zeros((ndir, n)), np.zeros((ndir, m)), np.zeros((ndir, m))
        _check(lib().chip_debug_batch_vjp_units(self._h, C.c_int32(piece), C.c_int64(first), C.c_int32(ndir),
                                                valid.ctypes.data_as(P_I32), _pf(rx), _pf(ws), _pf(rz)),
               "chip_debug_batch_vjp_units")
        return rx, ws, rz

    def debug_vjp_out(self, form, ndir, want, x, z, valid, vx, vz, gs=None, fill=0.0):
        """the output passes of a block of cotangents alone (no solve needed) on given solve results vx[ndir, n],
        vz[ndir, m]: form 1 the block launchers once, form 0 the single launchers once per cotangent -> (dq, db, dP,
        dA), each [ndir, len] and pre-filled with `fill`: a piece that is not in `want` comes back as it went in"""
        bits = self._want_bits(want, "debug_vjp_out")
        keep = [None if v is None else _f(v) for v in (x, z, vx, vz, gs)]
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        res = [np.full((ndir, self._len[key]), float(fill)) for key in "qbPA"]
        ptr = [None if v is None else _pf(v) for v in keep]
        _check(lib().chip_debug_batch_vjp_out(self._h, C.c_int32(form), C.c_int32(ndir), C.c_int32(bits), ptr[0],
                                              ptr[1], valid.ctypes.data_as(P_I32), *ptr[2:], *[_pf(v) for v in res]),
               "chip_debug_batch_vjp_out")
        return tuple(res)

    def debug_jac_rhs(self, ndir, x, z, valid, dq=None, db=None, dP=None, dA=None):
        """the right-hand side pass of a block alone (no solve needed): pieces [ndir, len] -> the scaled
        (rx[ndir, n], rz[ndir, m])"""
        keep = [None if v is None else _f(v) for v in (x, z, dq, db, dP, dA)]
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        rx, rz = np.zeros((ndir, self._len["q"])), np.zeros((ndir, self._len["b"]))
        ptr = [None if v is None else _pf(v) for v in keep]
        _check(lib().chip_debug_batch_jac_rhs(self._h, C.c_int32(ndir), ptr[0], ptr[1], valid.ctypes.data_as(P_I32),
                                              *ptr[2:], _pf(rx), _pf(rz)), "chip_debug_batch_jac_rhs")
        return rx, rz

    def debug_jac_units(self, piece, first, ndir, valid):
        """the unit right-hand sides of a block alone (no solve needed) -> the scaled (rx[ndir, n], rz[ndir, m])"""
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        rx, rz = np.zeros((ndir, self._len["q"])), np.zeros((ndir, self._len["b"]))
        _check(lib().chip_debug_batch_jac_units(self._h, C.c_int32(piece), C.c_int64(first), C.c_int32(ndir),
                                                valid.ctypes.data_as(P_I32), _pf(rx), _pf(rz)),
               "chip_debug_batch_jac_units")
        return rx, rz

    def debug_jvp_rhs(self, x, z, valid, dq=None, db=None, dP=None, dA=None):
        """the right-hand side pass of jvp alone (no solve needed) -> the scaled (rx[n], rz[m])"""
        keep = [None if v is None else _f(v) for v in (x, z, dq, db, dP, dA)]
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        rx, rz = np.zeros(self._len["q"]), np.zeros(self._len["b"])
        ptr = [None if v is None else _pf(v) for v in keep]
        _check(lib().chip_debug_batch_jvp_rhs(self._h, ptr[0], ptr[1], valid.ctypes.data_as(P_I32), *ptr[2:],
                                              _pf(rx), _pf(rz)), "chip_debug_batch_jvp_rhs")
        return rx, rz

    def debug_inject_nan(self, member, iteration):
        _check(lib().chip_debug_batch_inject_nan(self._h, C.c_int64(member), C.c_int32(iteration)),
               "chip_debug_batch_inject_nan")

    def debug_counter(self, name):
        out = C.c_double()
        _check(lib().chip_debug_batch_counter(self._h, name.encode(), C.byref(out)), "chip_debug_batch_counter")
        return out.value


class _BatchDerivative:
    """stacked result vectors (numpy arrays or torch GPU tensors) named by FIELDS = ((attribute, offset key), ...),
    and valid[nprob] (numpy int32): 1 where the member has a derivative, else its entries are exact zeros"""
    FIELDS = ()

    def __init__(self, *args):
        *vectors, self.valid, self._offsets = args
        if len(vectors) != len(self.FIELDS):
            raise TypeError("%s: %d vectors, valid and offsets are needed" % (type(self).__name__, len(self.FIELDS)))
        for (name, _), v in zip(self.FIELDS, vectors):
            setattr(self, name, v)

    def per_member(self, k):
        """member k's slices of the stacked vectors, in the order of FIELDS"""
        o = self._offsets
        return tuple(getattr(self, name)[int(o[key][k]):int(o[key][k + 1])] for name, key in self.FIELDS)


class BatchGradient(_BatchDerivative):
    """the result of HipBatchSolver.backward: dq[n], db[m], dP[nnz(P)], dA[nnz(A)] of the stack (dP, dA in the order
    of the stack's nzval, the positions update_P / update_A index) as numpy arrays or torch GPU tensors, and
    valid[nprob] (numpy int32): 1 where the member has a gradient, else its entries are exact zeros"""
    FIELDS = (("dq", "q"), ("db", "b"), ("dP", "P"), ("dA", "A"))


class BatchTangent(_BatchDerivative):
    """the result of HipBatchSolver.jvp: dx[n], dz[m], ds[m] of the stack as numpy arrays or torch GPU tensors, and
    valid[nprob] (numpy int32): 1 where the member has a derivative, else its entries are exact zeros"""
    FIELDS = (("dx", "q"), ("dz", "b"), ("ds", "b"))


class BatchTangentBlock:
    """the result of HipBatchSolver.jvp_block: dx[K, n], dz[K, m], ds[K, m] of the stack, row t = direction t, as
    numpy arrays or torch GPU tensors, and valid[nprob] (numpy int32): 1 where the member has a derivative, else its
    entries are exact zeros in every direction"""
    FIELDS = BatchTangent.FIELDS

    def __init__(self, dx, dz, ds, valid, offsets):
        self.dx, self.dz, self.ds, self.valid, self._offsets = dx, dz, ds, valid, offsets

    def per_member(self, k):
        """member k's columns of the three matrices: (dx[:, n_k], dz[:, m_k], ds[:, m_k])"""
        o = self._offsets
        return tuple(getattr(self, name)[:, int(o[key][k]):int(o[key][k + 1])] for name, key in self.FIELDS)


class BatchGradientBlock:
    """the result of HipBatchSolver.backward_block: dq[K, n], db[K, m], dP[K, nnz(P)], dA[K, nnz(A)] of the stack, row
    t = cotangent t, as numpy arrays or torch GPU tensors (None for a piece that was not wanted), and valid[nprob]
    (numpy int32): 1 where the member has a gradient, else its entries are exact zeros in every cotangent"""
    FIELDS = BatchGradient.FIELDS

    def __init__(self, dq, db, dP, dA, valid, offsets):
        self.dq, self.db, self.dP, self.dA, self.valid, self._offsets = dq, db, dP, dA, valid, offsets

    def per_member(self, k):
        """member k's columns of the four matrices: (dq[:, n_k], db[:, m_k], dP[:, nnz(P_k)], dA[:, nnz(A_k)]); None
        for a piece that was not wanted"""
        o = self._offsets
        return tuple(None if getattr(self, name) is None
                     else getattr(self, name)[:, int(o[key][k]):int(o[key][k + 1])] for name, key in self.FIELDS)


def _torch_copy(ptr, n, dtype, device=None):
    """a torch tensor on the GPU holding a copy of n values at device address `ptr`"""
    import torch
    t = torch.empty(int(n), dtype=getattr(torch, dtype), device=device if device is not None else "cuda")
    if n:
        rt = _hiprt()
        rc = rt.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(int(n) * t.element_size()), C.c_int(3))
        if rc == 0:
            rc = rt.hipDeviceSynchronize()
        if rc != 0:
            raise RuntimeError("hipMemcpy D2D failed: %d" % rc)
    return t


def _cone_arrays(cones):
    cones = [tuple(c) for c in cones]
    tags = np.array([c[0] for c in cones], dtype=np.int32)
    dims = np.array([c[1] for c in cones], dtype=np.int64)
    dims2 = np.array([c[2] if len(c) > 2 else 0 for c in cones], dtype=np.int64)
    alphas = np.array([c[3] if (len(c) > 3 and c[0] == PowerConeT) else 0.5 for c in cones], dtype=np.float64)
    return tags, dims, dims2, alphas


class TransformDebug:
    """the presolve / chordal-decomposition transform of chip_solver_create alone, on the host (test hooks of
    include/clarabel_hip_testing.h: a library built with TESTING=1).  Arguments as HipSolver."""

    _INT = {"sizes", "keep", "Pp", "Pi", "Ap", "Ai", "dims", "dims2", "tags", "mode", "ptr", "src", "H_row"}

    def __init__(self, P, q, A, b, cones, settings=None):
        self.n, self.m = P.n, A.m
        self.settings = settings or SolverSettings.default()
        tags, dims, dims2, alphas = _cone_arrays(cones)
        self._h = C.c_void_p()
        _check(lib().chip_debug_transform_create(C.byref(self._h), C.c_int64(P.n), C.c_int64(A.m), _pu(P.colptr),
                                                 _pu(P.rowval), _pf(P.nzval), _pf(_f(q)), _pu(A.colptr),
                                                 _pu(A.rowval), _pf(A.nzval), _pf(_f(b)), C.c_int64(len(tags)),
                                                 tags.ctypes.data_as(P_I32), dims.ctypes.data_as(P_I64),
                                                 dims2.ctypes.data_as(P_I64), _pf(alphas), C.byref(self.settings)),
               "chip_debug_transform_create")
        sz = self.get("sizes")
        (self.active, _, _, self.m_reduced, self.n2, self.m2, self.npatterns, self.premerge_added, self.final_added,
         self.largest_clique) = [int(v) for v in sz]
        self.active = bool(self.active)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().chip_debug_transform_destroy(self._h)
            self._h = C.c_void_p()

    def get(self, name):
        n = C.c_int64()
        L = lib()
        _check(L.chip_debug_transform_get(self._h, name.encode(), C.byref(n), None), "chip_debug_transform_get")
        is_int = name in self._INT or (name.startswith("pattern") and not name.endswith(("Px", "q", "Ax", "b")))
        out = np.zeros(n.value, dtype=np.int64 if is_int else np.float64)
        _check(L.chip_debug_transform_get(self._h, name.encode(), C.byref(n), out.ctypes.data_as(C.c_void_p)),
               "chip_debug_transform_get")
        return out

    def problem(self):
        """the transformed (P, q, A, b, cones) as CscMatrix / arrays / cone tuples"""
        P = CscMatrix(self.n2, self.n2, self.get("Pp"), self.get("Pi"), self.get("Px"))
        A = CscMatrix(self.m2, self.n2, self.get("Ap"), self.get("Ai"), self.get("Ax"))
        cones = [(int(t), int(d), int(d2)) if t == GenPowerConeT or d2 else (int(t), int(d))
                 for t, d, d2 in zip(self.get("tags"), self.get("dims"), self.get("dims2"))]
        al = self.get("alphas")
        cones = [(c[0], c[1], 0, float(al[i])) if c[0] == PowerConeT else c for i, c in enumerate(cones)]
        return P, self.get("q"), A, self.get("b"), cones

    def patterns(self):
        """every decomposed cone: dict(cone, row_orig, row_pre, side, premerge_cliques, ordering, snode_start,
        snode_len, parent, sep = [...], cliques = [sorted original vertices of each clique, in post order])"""
        out = []
        for k in range(self.npatterns):
            info = self.get("pattern%d.info" % k)
            p = dict(zip(("cone", "row_orig", "row_pre", "side", "premerge_cliques"), [int(v) for v in info]))
            for f in ("ordering", "snode_start", "snode_len", "parent"):
                p[f] = self.get("pattern%d.%s" % (k, f))
            p["sep"] = [self.get("pattern%d.sep%d" % (k, j)) for j in range(len(p["snode_start"]))]
            order = p["ordering"]
            p["cliques"] = [sorted([int(order[v]) for v in range(a, a + ln)] + [int(order[v]) for v in sp])
                            for a, ln, sp in zip(p["snode_start"], p["snode_len"], p["sep"])]
            out.append(p)
        return out

    def reverse(self, x2, s2, z2):
        """chip_debug_transform_reverse: (x, s, z) of the original problem from unscaled internal vectors"""
        x, s, z = np.zeros(self.n), np.zeros(self.m), np.zeros(self.m)
        _check(lib().chip_debug_transform_reverse(self._h, _pf(_f(x2)), _pf(_f(s2)), _pf(_f(z2)), _pf(x), _pf(s),
                                                  _pf(z)), "chip_debug_transform_reverse")
        return x, s, z


class BatchPlanDebug:
    """the partition of the batched solver alone (chip_debug_bplan_*; test hooks of include/clarabel_hip_testing.h: a
    library built with TESTING=1), and one launch of each device pass of csrc/batch.hpp on host arrays.  n_part /
    m_part: the members' columns / rows; cones: (tag, dim) tuples in row order.  Creating it and get() need no GPU;
    the first pass uploads the plan.  Every pass returns copies and leaves its arguments alone, except where an
    argument IS the output (blin's w, bunit_shift's z, bunit_reset's x / s / z: updated in place and returned)."""

    NAMES = ("xoff", "zoff", "xmem", "zmem", "ch_beg", "ch_end", "cx_first", "cz_first", "it_beg", "it_end", "it_type",
             "it_first", "rtype")
    SEG_DOT, SEG_WSQ, SEG_SUM, SEG_NONFINITE = range(4)
    CONE_STEP, CONE_MARGINS, CONE_INTERIOR = range(3)
    MASK_ZERO, MASK_Y, MASK_KEEP = range(3)
    ROW_ZERO, ROW_NN, ROW_SOC_HEAD, ROW_SOC_TAIL = range(4)
    ITEM_NN, ITEM_SOC = range(2)
    CHUNK, SEG_MAX = 4096, 16

    PSD_NAMES = ("degree", "psd_sizes", "psd_mem", "psd_start", "psd_dim", "psd_view", "psd_first", "psd_diag")
    ROW_PSD = 4

    def __init__(self, n_part, m_part, cones, symmetric=False):
        """symmetric: the plan of chip_bsym_create (chip_debug_bsymplan_create), which takes PSDTriangle cones too"""
        n_part = np.ascontiguousarray(n_part, dtype=np.int64)
        m_part = np.ascontiguousarray(m_part, dtype=np.int64)
        tags, dims, _, _ = _cone_arrays(cones)
        self._h = C.c_void_p()
        create = "chip_debug_bsymplan_create" if symmetric else "chip_debug_bplan_create"
        _check(getattr(lib(), create)(C.byref(self._h), C.c_int64(len(n_part)), n_part.ctypes.data_as(P_I64),
                                      m_part.ctypes.data_as(P_I64), C.c_int64(len(tags)),
                                      tags.ctypes.data_as(P_I32), dims.ctypes.data_as(P_I64)), create)
        self.nprob, self.n, self.m, self.ncx, self.ncz, self.nitems = [int(v) for v in self.get("sizes")]

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().chip_debug_bplan_destroy(self._h)
            self._h = C.c_void_p()

    def get(self, name):
        n = C.c_int64()
        L = lib()
        _check(L.chip_debug_bplan_get(self._h, name.encode(), C.byref(n), None), "chip_debug_bplan_get")
        out = np.zeros(n.value, dtype=np.int32)
        _check(L.chip_debug_bplan_get(self._h, name.encode(), C.byref(n), out.ctypes.data_as(P_I32)),
               "chip_debug_bplan_get")
        return out

    def _vec(self, a, length, what, null_ok=False, dtype=f64):
        if a is None:
            if not null_ok:
                raise ValueError("%s is required" % what)
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != (length,):
            raise ValueError("%s must have %d entries" % (what, length))
        return a

    @staticmethod
    def _p(a, ptr=P_F64):
        return None if a is None else a.ctypes.data_as(ptr)

    def seg_reduce(self, specs, nslots, fill=0.0):
        """specs: up to SEG_MAX tuples (kind, space, slot, a, b or None) -> out[nslots, nprob], `fill` where no spec
        wrote.  Specs that name the same array object share one device buffer."""
        cnt = len(specs)
        kind = np.array([s[0] for s in specs], dtype=np.int32)
        space = np.array([s[1] for s in specs], dtype=np.int32)
        slot = np.array([s[2] for s in specs], dtype=np.int32)
        keep = {}  # one contiguous copy per distinct array object

        def arr(v, sp_, what):
            if v is None:
                return None
            if id(v) not in keep:
                keep[id(v)] = (v, self._vec(v, self.m if sp_ else self.n, what))
            return keep[id(v)][1]
        av = [arr(s[3], s[1], "a") for s in specs]
        bv = [arr(s[4], s[1], "b") for s in specs]
        pa = (C.c_void_p * max(cnt, 1))(*[None if v is None else v.ctypes.data for v in av])
        pb = (C.c_void_p * max(cnt, 1))(*[None if v is None else v.ctypes.data for v in bv])
        out = np.full((nslots, self.nprob), fill, dtype=f64)
        _check(lib().chip_debug_bplan_seg_reduce(self._h, C.c_int32(cnt), self._p(kind, P_I32), self._p(space, P_I32),
                                                 self._p(slot, P_I32), pa, pb, C.c_int32(nslots), _pf(out)),
               "chip_debug_bplan_seg_reduce")
        return out

    def cone_minima(self, op, z, sv=None, dz=None, ds=None, amax=None, want_sum=True):
        """-> (out_min[nprob], out_sum[nprob] or None)"""
        m, k = self.m, self.nprob
        z, sv = self._vec(z, m, "z"), self._vec(sv, m, "sv", True)
        dz, ds = self._vec(dz, m, "dz", True), self._vec(ds, m, "ds", True)
        amax = self._vec(amax, k, "amax", True)
        omin = np.full(k, np.nan)
        osum = np.full(k, np.nan) if want_sum else None
        _check(lib().chip_debug_bplan_cone_minima(self._h, C.c_int32(op), self._p(dz), self._p(ds), self._p(z),
                                                  self._p(sv), self._p(amax), _pf(omin), self._p(osum)),
               "chip_debug_bplan_cone_minima")
        return omin, osum

    def blin(self, w, x, y=None, sa=None, sb=None, ca=0.0, cb=0.0, space=0, mask=None, mask_mode=0):
        """w (a float64 array, updated in place) = a_k x + b_k y; pass w itself as x or y to alias them"""
        ln, k = (self.m if space else self.n), self.nprob
        if not (isinstance(w, np.ndarray) and w.dtype == f64 and w.flags.c_contiguous and w.shape == (ln,)):
            raise ValueError("w must be a contiguous float64 array of %d entries" % ln)
        xv = w if x is w else self._vec(x, ln, "x")
        yv = w if y is w else self._vec(y, ln, "y", True)
        sa, sb = self._vec(sa, k, "sa", True), self._vec(sb, k, "sb", True)
        mask = self._vec(mask, k, "mask", True, np.int32)
        _check(lib().chip_debug_bplan_blin(self._h, _pf(w), _pf(xv), self._p(yv), self._p(sa), self._p(sb),
                                           C.c_double(ca), C.c_double(cb), C.c_int32(space), self._p(mask, P_I32),
                                           C.c_int32(mask_mode)), "chip_debug_bplan_blin")
        return w

    def bresid(self, rx_inf, Px, q, rz_inf, b, tau):
        """-> (rx, rz)"""
        n, m = self.n, self.m
        rx, rz = np.full(n, np.nan), np.full(m, np.nan)
        _check(lib().chip_debug_bplan_bresid(self._h, _pf(rx), _pf(self._vec(rx_inf, n, "rx_inf")),
                                             _pf(self._vec(Px, n, "Px")), _pf(self._vec(q, n, "q")), _pf(rz),
                                             _pf(self._vec(rz_inf, m, "rz_inf")), _pf(self._vec(b, m, "b")),
                                             _pf(self._vec(tau, self.nprob, "tau"))), "chip_debug_bplan_bresid")
        return rx, rz

    def bunit_shift(self, z, alpha, primal, mask=None):
        """z (copied) += alpha_k e -> the new z"""
        z = self._vec(z, self.m, "z").copy()
        mask = self._vec(mask, self.nprob, "mask", True, np.int32)
        _check(lib().chip_debug_bplan_bunit_shift(self._h, _pf(z), _pf(self._vec(alpha, self.nprob, "alpha")),
                                                  C.c_int32(primal), self._p(mask, P_I32)),
               "chip_debug_bplan_bunit_shift")
        return z

    def bunit_reset(self, x, sv, z, flag):
        """-> the new (x, s, z) (copies)"""
        x, sv, z = self._vec(x, self.n, "x").copy(), self._vec(sv, self.m, "sv").copy(), self._vec(z, self.m, "z").copy()
        flag = self._vec(flag, self.nprob, "flag", False, np.int32)
        _check(lib().chip_debug_bplan_bunit_reset(self._h, _pf(x), _pf(sv), _pf(z), self._p(flag, P_I32)),
               "chip_debug_bplan_bunit_reset")
        return x, sv, z

    def bunscale(self, x, d, z, e, sv, einv, sx, sz):
        """-> (xo, zo, so)"""
        n, m, k = self.n, self.m, self.nprob
        xo, zo, so = np.full(n, np.nan), np.full(m, np.nan), np.full(m, np.nan)
        _check(lib().chip_debug_bplan_bunscale(self._h, _pf(xo), _pf(self._vec(x, n, "x")), _pf(self._vec(d, n, "d")),
                                               _pf(zo), _pf(self._vec(z, m, "z")), _pf(self._vec(e, m, "e")), _pf(so),
                                               _pf(self._vec(sv, m, "sv")), _pf(self._vec(einv, m, "einv")),
                                               _pf(self._vec(sx, k, "sx")), _pf(self._vec(sz, k, "sz"))),
               "chip_debug_bplan_bunscale")
        return xo, zo, so


class PsdConesDebug:
    """the PSD cone kernels of csrc/cones.hip alone (chip_debug_psd_*; test hooks of include/clarabel_hip_testing.h: a
    library built with TESTING=1): a bare device view over a vector that holds only the svec ranges of PSD triangle
    cones of sides `dims`, and one launch of each launcher on host arrays.  Creating it and counter() need no GPU; the
    first pass uploads the view.  Every pass returns new arrays and leaves its arguments alone."""

    def __init__(self, dims):
        dims = np.ascontiguousarray(dims, dtype=np.int64)
        self._h = C.c_void_p()
        _check(lib().chip_debug_psd_create(C.byref(self._h), C.c_int64(len(dims)), dims.ctypes.data_as(P_I64)),
               "chip_debug_psd_create")
        self.dims = [int(d) for d in dims]
        self.ncones = len(self.dims)
        self.start = [0]
        for d in self.dims:
            self.start.append(self.start[-1] + d * (d + 1) // 2)
        self.rows = self.start[-1]
        assert self.rows == int(self.counter("rows"))

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().chip_debug_psd_destroy(self._h)
            self._h = C.c_void_p()

    def counter(self, name):
        """"gs", "jacobi_lds" (of the last update_scaling / step_length / margins), "maxdim", "rows", "scratch_stride",
        "state_doubles" """
        out = C.c_double()
        _check(lib().chip_debug_psd_counter(self._h, name.encode(), C.byref(out)), "chip_debug_psd_counter")
        return out.value

    def rows_of(self, c):
        return slice(self.start[c], self.start[c + 1])

    def _vec(self, a, what):
        a = np.ascontiguousarray(a, dtype=f64)
        if a.shape != (self.rows,):
            raise ValueError("%s must have %d entries" % (what, self.rows))
        return a

    def update_scaling(self, s, z):
        """-> True / False (a cone without a Cholesky factor)"""
        ok = C.c_int32(-1)
        _check(lib().chip_debug_psd_update_scaling(self._h, _pf(self._vec(s, "s")), _pf(self._vec(z, "z")), C.byref(ok)),
               "chip_debug_psd_update_scaling")
        return bool(ok.value)

    def state(self, c):
        """-> B, lambda, lambda^-1/2, R, Rinv of cone c (matrices as numpy (row, column) arrays)"""
        n = self.dims[c]
        buf = np.full(3 * n * n + 2 * n, np.nan)
        _check(lib().chip_debug_psd_state(self._h, C.c_int64(c), _pf(buf)), "chip_debug_psd_state")
        mat = lambda o: buf[o:o + n * n].reshape(n, n).T.copy()  # (column major on the device)
        return mat(0), buf[n * n:n * n + n].copy(), buf[n * n + n:n * n + 2 * n].copy(), mat(n * n + 2 * n), \
            mat(2 * n * n + 2 * n)

    def mul_hs(self, x):
        y = np.full(self.rows, np.nan)
        _check(lib().chip_debug_psd_mul_hs(self._h, _pf(y), _pf(self._vec(x, "x"))), "chip_debug_psd_mul_hs")
        return y

    def affine_ds(self):
        ds = np.full(self.rows, np.nan)
        _check(lib().chip_debug_psd_affine_ds(self._h, _pf(ds)), "chip_debug_psd_affine_ds")
        return ds

    def combined_ds_shift(self, step_z, step_s, sigma_mu):
        """-> (shift, W step_z, W^-T step_s)"""
        shift = np.full(self.rows, np.nan)
        wz, ws = self._vec(step_z, "step_z").copy(), self._vec(step_s, "step_s").copy()
        _check(lib().chip_debug_psd_combined_ds_shift(self._h, _pf(shift), _pf(wz), _pf(ws), C.c_double(sigma_mu)),
               "chip_debug_psd_combined_ds_shift")
        return shift, wz, ws

    def ds_from_dz_offset(self, ds):
        out = np.full(self.rows, np.nan)
        _check(lib().chip_debug_psd_ds_from_dz_offset(self._h, _pf(out), _pf(self._vec(ds, "ds"))),
               "chip_debug_psd_ds_from_dz_offset")
        return out

    def step_length(self, dz, ds, amax):
        """-> the per-cone step lengths"""
        out = np.full(self.ncones, np.nan)
        _check(lib().chip_debug_psd_step_length(self._h, _pf(self._vec(dz, "dz")), _pf(self._vec(ds, "ds")),
                                                C.c_double(amax), _pf(out)), "chip_debug_psd_step_length")
        return out

    def margins(self, z):
        """-> per cone (smallest eigenvalue, sum of the positive eigenvalues)"""
        pmin, psum = np.full(self.ncones, np.nan), np.full(self.ncones, np.nan)
        _check(lib().chip_debug_psd_margins(self._h, _pf(self._vec(z, "z")), _pf(pmin), _pf(psum)),
               "chip_debug_psd_margins")
        return pmin, psum

    def barrier(self, z, s, dz, ds, alpha):
        """-> the per-cone barrier values at (z, s) + alpha (dz, ds)"""
        out = np.full(self.ncones, np.nan)
        _check(lib().chip_debug_psd_barrier(self._h, _pf(self._vec(z, "z")), _pf(self._vec(s, "s")),
                                            _pf(self._vec(dz, "dz")), _pf(self._vec(ds, "ds")), C.c_double(alpha),
                                            _pf(out)), "chip_debug_psd_barrier")
        return out


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _host_array(x, what, integer):
    """a host vector (list, numpy array, CPU torch tensor) -> 1-D numpy array; TypeError for a dtype the form does not
    take (indices: integers; values: real numbers)"""
    if _is_torch(x):
        x = x.detach().numpy()
    a = np.asarray(x)
    if a.ndim != 1:
        raise ChipError(ERR_DIM, "update %s: a 1-D vector is needed" % what)
    if a.size == 0:
        return a
    if integer and a.dtype.kind not in "iu":
        raise TypeError("update %s: indices must be integers, not %s" % (what, a.dtype))
    if not integer and a.dtype.kind not in "iuf":
        raise TypeError("update %s: values must be real numbers, not %s" % (what, a.dtype))
    return a


def classify_update(key, data, length, pattern=None):
    """The form of one piece of update data (no GPU touched): ("none",), ("full", None, values),
    ("partial", index, values) with host numpy arrays (uint64 / float64), or ("dev_full", None, values) /
    ("dev_partial", index, values) with torch tensors on the GPU (int64 / float64, contiguous).  key: "P", "A", "q"
    or "b"; length: nnz(P) / nnz(A) / n / m; pattern: (m, n, colptr, rowval) of P / A for a CscMatrix
    (check_equal_sparsity).  ChipError(ERR_DIM) for a pattern that differs, a full vector of the wrong length or an
    index / value count mismatch; TypeError for a dtype or kind the piece does not take."""
    if data is None:
        return ("none",)
    if isinstance(data, CscMatrix):
        if pattern is None:
            raise TypeError("update %s: a vector, not a matrix" % key)
        m, n, colptr, rowval = pattern
        if (data.m, data.n) != (m, n) or not np.array_equal(data.colptr, colptr) or \
                not np.array_equal(data.rowval, rowval):
            raise ChipError(ERR_DIM, "update %s: the sparsity pattern differs from the setup's" % key)
        data = data.nzval
    if isinstance(data, tuple):
        if len(data) != 2:
            raise TypeError("update %s: an (index, values) tuple has two members" % key)
        idx, vals = data
        on_gpu = [_is_torch(a) and a.is_cuda for a in (idx, vals)]
        if on_gpu[0] != on_gpu[1]:
            raise TypeError("update %s: index and values must both be host arrays or both GPU tensors" % key)
        if on_gpu[1]:
            import torch
            if idx.dtype != torch.int64 or vals.dtype != torch.float64:
                raise TypeError("update %s: GPU index / values must be int64 / float64, not %s / %s"
                                % (key, idx.dtype, vals.dtype))
            if idx.dim() != 1 or vals.dim() != 1 or idx.numel() != vals.numel():
                raise ChipError(ERR_DIM, "update %s: index and values differ in length" % key)
            if vals.numel() == 0:
                return ("none",)
            return ("dev_partial", idx.contiguous(), vals.contiguous())
        idx, vals = _host_array(idx, key, True), _host_array(vals, key, False)
        if idx.size != vals.size:
            raise ChipError(ERR_DIM, "update %s: index and values differ in length" % key)
        if vals.size == 0:
            return ("none",)
        if idx.dtype.kind == "i" and np.any(idx < 0):
            idx = np.where(idx < 0, np.iinfo(np.int64).max, idx)  # (refused by the library as out of range)
        return ("partial", _u(idx), _f(vals))
    if _is_torch(data) and data.is_cuda:
        import torch
        if data.dtype != torch.float64:
            raise TypeError("update %s: GPU values must be float64, not %s" % (key, data.dtype))
        if data.dim() != 1:
            raise ChipError(ERR_DIM, "update %s: a 1-D vector is needed" % key)
        if data.numel() == 0:
            return ("none",)
        if data.numel() != length:
            raise ChipError(ERR_DIM, "update %s: %d values for %d entries" % (key, data.numel(), length))
        return ("dev_full", None, data.contiguous())
    vals = _host_array(data, key, False)
    if vals.size == 0:
        return ("none",)
    if vals.size != length:
        raise ChipError(ERR_DIM, "update %s: %d values for %d entries" % (key, vals.size, length))
    return ("full", None, _f(vals))


def batch_list_update(key, pieces, offsets, patterns=None):
    """The per-member list form of HipBatchSolver.update as ONE partial update of the stack (no GPU touched).  pieces:
    one entry per member -- None (untouched), a value vector of the member's own length (or a CscMatrix with the
    member's pattern) or a member-local (index, values) of host arrays; offsets[k] is where member k's entries start
    in the stacked nzval / vector (nprob + 1 entries); patterns: the members' (m, n, colptr, rowval) for P / A.
    Returns ("none",) or ("partial", index, values) with stack positions in member order (uint64 / float64).
    ChipError(ERR_DIM) for a list of the wrong length, a vector of the wrong length or a member-local index outside
    the member (it must not reach another member's entries)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    if len(pieces) != len(offsets) - 1:
        raise ChipError(ERR_DIM, "update %s: %d list entries for %d members" % (key, len(pieces), len(offsets) - 1))
    idxs, vals = [], []
    for k, piece in enumerate(pieces):
        length = int(offsets[k + 1] - offsets[k])
        form = classify_update(key, piece, length, None if patterns is None else patterns[k])
        if form[0] == "none":
            continue
        if form[0] == "full":
            idxs.append(offsets[k] + np.arange(length, dtype=np.int64))
        elif form[0] == "partial":
            if np.any(form[1] >= np.uint64(length)):
                raise ChipError(ERR_DIM, "update %s: member %d: an index is out of the member's range" % (key, k))
            idxs.append(offsets[k] + form[1].astype(np.int64))
        else:
            raise TypeError("update %s: member %d: the entries of a list are host arrays" % (key, k))
        vals.append(form[2])
    if not idxs:
        return ("none",)
    return ("partial", _u(np.concatenate(idxs)), _f(np.concatenate(vals)))


# ---------------------------------------------------------------------------
# sharded path: RCCL communicator of the C ABI (csrc/comm.cpp)
# ---------------------------------------------------------------------------
COMM_ID_BYTES = 128


def comm_unique_id():
    """rank 0: the rendezvous token to hand to the other ranks out of band (bytes)"""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(lib().chip_comm_get_unique_id(buf), "chip_comm_get_unique_id")
    return bytes(buf)


class Comm:
    """one per process / GPU; collective construction over all ranks"""

    def __init__(self, unique_id, world, rank, device=-1):
        assert len(unique_id) == COMM_ID_BYTES
        self._h = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(lib().chip_comm_create(C.byref(self._h), buf, C.c_int32(world), C.c_int32(rank), C.c_int32(device)),
               "chip_comm_create")
        self.world, self.rank = world, rank

    def __del__(self):
        if getattr(self, "_h", None):
            lib().chip_comm_destroy(self._h)
            self._h = None

    def attach(self, kkt):
        _check(lib().chip_kkt_attach_comm(kkt._h, self._h), "attach_comm")

    def allgather_step(self, kkt, send_ptr, recv_ptr, counts):
        cnt = np.ascontiguousarray(counts, dtype=np.int64)
        assert len(cnt) == self.world
        _check(lib().chip_kkt_allgather_step(kkt._h, self._h, C.c_void_p(send_ptr), C.c_void_p(recv_ptr),
                                             cnt.ctypes.data_as(P_I64)), "allgather_step")

    def wait(self, kkt):
        """kkt's stream waits on the device for the last all-gather"""
        _check(lib().chip_kkt_wait_comm(kkt._h, self._h), "wait_comm")

    def debug_spin(self, blocks, threads=256, usec=60.0):
        """test hook: a spinner on the communicator's stream behind the last collective (chip_comm_debug_spin)"""
        lib().chip_comm_debug_spin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double]
        _check(lib().chip_comm_debug_spin(self._h, blocks, threads, float(usec)), "comm_debug_spin")

    def synchronize(self):
        _check(lib().chip_comm_synchronize(self._h), "comm_synchronize")

    def allreduce(self, vals, op="sum"):
        v = np.ascontiguousarray(np.atleast_1d(vals), dtype=np.float64).copy()
        _check(lib().chip_comm_allreduce(self._h, _pf(v), C.c_int32(len(v)), C.c_int32({"sum": 0, "min": 1, "max": 2}[op])),
               "comm_allreduce")
        return v

    def barrier(self):
        self.allreduce([0.0])


# ---------------------------------------------------------------------------
# raw HBM buffers without torch (tests / single-GPU bench plumbing): thin ctypes
# calls into the SAME libamdhip64 instance the extension is linked against.
# NB when torch is used in the process, import torch BEFORE this package so that
# both share torch's bundled HIP runtime (two runtimes cannot both own the GPU).
# ---------------------------------------------------------------------------
_HIPRT = None


def _hiprt():
    global _HIPRT
    if _HIPRT is None:
        lib()
        _HIPRT = C.CDLL("libamdhip64.so.7")
    return _HIPRT


class DeviceArray:
    """n fp64 values in HBM on the current device"""

    def __init__(self, n_or_array):
        rt = _hiprt()
        host = None
        if not np.isscalar(n_or_array):
            host = _f(n_or_array)
            n = len(host)
        else:
            n = int(n_or_array)
        self.n = n
        self._p = C.c_void_p()
        rc = rt.hipMalloc(C.byref(self._p), C.c_size_t(max(n, 1) * 8))
        if rc != 0:
            raise RuntimeError("hipMalloc failed: %d" % rc)
        if host is not None:
            self.copy_from(host)
        else:
            rt.hipMemset(self._p, 0, C.c_size_t(max(n, 1) * 8))

    @classmethod
    def view(cls, ptr, n):
        """non-owning view of n fp64 values at device address `ptr` (never freed here)"""
        a = cls.__new__(cls)
        a.n = int(n)
        a._p = C.c_void_p(ptr)
        a._borrowed = True
        return a

    @property
    def ptr(self):
        return self._p.value

    def copy_from(self, host):
        host = _f(host)
        assert len(host) == self.n
        rc = _hiprt().hipMemcpy(self._p, host.ctypes.data_as(C.c_void_p), C.c_size_t(self.n * 8), C.c_int(1))
        if rc != 0:
            raise RuntimeError("hipMemcpy H2D failed: %d" % rc)

    def numpy(self):
        out = np.zeros(self.n)
        rc = _hiprt().hipMemcpy(out.ctypes.data_as(C.c_void_p), self._p, C.c_size_t(self.n * 8), C.c_int(2))
        if rc != 0:
            raise RuntimeError("hipMemcpy D2H failed: %d" % rc)
        return out

    def __del__(self):
        if getattr(self, "_borrowed", False):
            return
        if getattr(self, "_p", None) and self._p.value:
            try:
                _hiprt().hipFree(self._p)
            except Exception:
                pass
            self._p = C.c_void_p()


def debug_spin(device, blocks, threads=256, lds_bytes=0, usec=1000.0):
    """test hook (include/clarabel_hip_testing.h; CHIP_TESTING builds): a co-resident kernel that only spins;
    blocks = 0 waits for the spinners"""
    lib().chip_debug_spin.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double]
    _check(lib().chip_debug_spin(device, blocks, threads, lds_bytes, float(usec)), "debug_spin")


def debug_set_switch(name, value=None):
    """test hook: set (value given) or clear one CHIP_* diagnostic switch and re-parse the switch table
    (csrc/switches.hpp) -- for handles that already exist; the environment is read whenever a handle is created"""
    lib().chip_debug_set_switch.argtypes = [C.c_char_p, C.c_char_p]
    _check(lib().chip_debug_set_switch(name.encode(), None if value is None else str(value).encode()), "debug_set_switch")


def debug_counter(kkt, name):
    """test hook: one structural figure of a HipKKTSolver by name (include/clarabel_hip_testing.h: chip_debug_counter)"""
    out = C.c_double(0.0)
    lib().chip_debug_counter.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
    _check(lib().chip_debug_counter(kkt._h, name.encode(), C.byref(out)), "debug_counter")
    return out.value


def debug_create_count(which):
    """test hook: how often this process entered chip_kkt_create (which = 0) / chip_kktsystem_create (1)"""
    out = C.c_double(0.0)
    _check(lib().chip_debug_create_count(C.c_int32(which), C.byref(out)), "chip_debug_create_count")
    return int(out.value)


def debug_reload_pass(src, cap=False, raw=False, misalign=0, fill=-7.0):
    """test hook: the load pass of a re-equilibration alone on the values src (chip_debug_reload_pass).  Returns
    (dst, raw or None, o_dst, o_raw): the whole len + 4 buffers, pre-filled with `fill`, and where the written range
    [o, o + len) starts in each (misalign bits: 1 = dst, 2 = raw, 4 = src start 8 bytes past a 16-byte boundary)"""
    src = _f(src)
    dst = np.full(len(src) + 4, fill)
    rw = np.full(len(src) + 4, fill) if raw else None
    _check(lib().chip_debug_reload_pass(_pf(dst), None if rw is None else _pf(rw), _pf(src if len(src) else np.zeros(1)),
                                        C.c_int64(len(src)), C.c_int32(int(cap)), C.c_int32(misalign)),
           "chip_debug_reload_pass")
    return dst, rw, (1 if misalign & 1 else 2), (1 if misalign & 2 else 2)


def debug_eq_ruiz_step(n, m, P, A, q, b, d, e, c, min_scaling, max_scaling):
    """test hook: ONE Ruiz step (csrc/equilibrate.hip: eq_ruiz_step) from the state (P, A, q, b, d, e, c); P, A are
    (colptr, rowval, nzval) CSC triplets (P the upper triangle).  The caller's arrays are left alone.  Returns a dict:
    Px, Ax, q, b, d, e, c and `factor`, the step's cost factor (1.0: cost scaling skipped)"""
    Pp, Pi, Px = _u(P[0]), _u(P[1]), _f(P[2]).copy()
    Ap, Ai, Ax = _u(A[0]), _u(A[1]), _f(A[2]).copy()
    q, b, d, e = (_f(a).copy() for a in (q, b, d, e))
    assert len(Pp) == n + 1 and len(Ap) == n + 1 and len(q) == n and len(d) == n and len(b) == m and len(e) == m
    assert len(Pi) == len(Px) == Pp[-1] and len(Ai) == len(Ax) == Ap[-1]
    cstate = np.array([c, 1.0])
    _check(lib().chip_debug_eq_ruiz_step(C.c_int64(n), C.c_int64(m), _pu(Pp), _pu(Pi), _pf(Px), _pu(Ap), _pu(Ai),
                                         _pf(Ax), _pf(q), _pf(b), _pf(d), _pf(e), _pf(cstate),
                                         C.c_double(min_scaling), C.c_double(max_scaling)), "chip_debug_eq_ruiz_step")
    return dict(Px=Px, Ax=Ax, q=q, b=b, d=d, e=e, c=float(cstate[0]), factor=float(cstate[1]))


def debug_eq_rectify(n, m, A, b, e, segments):
    """test hook: the rectification (eq_rectify) over the row ranges segments = [(beg, end), ...] -> (Ax, b, e)"""
    Ap, Ai, Ax = _u(A[0]), _u(A[1]), _f(A[2]).copy()
    b, e = _f(b).copy(), _f(e).copy()
    assert len(Ap) == n + 1 and len(Ai) == len(Ax) == Ap[-1] and len(b) == m and len(e) == m
    sb = np.ascontiguousarray([s[0] for s in segments], dtype=np.int32)
    se = np.ascontiguousarray([s[1] for s in segments], dtype=np.int32)
    _check(lib().chip_debug_eq_rectify(C.c_int64(n), C.c_int64(m), _pu(Ap), _pu(Ai), _pf(Ax), _pf(b), _pf(e),
                                       C.c_int32(len(sb)), sb.ctypes.data_as(P_I32), se.ctypes.data_as(P_I32)),
           "chip_debug_eq_rectify")
    return Ax, b, e


def debug_eq_invert(d, e):
    """test hook: eq_invert -> (dinv, einv); the outputs hold NaN before the call"""
    d, e = _f(d), _f(e)
    dinv, einv = np.full(len(d), np.nan), np.full(len(e), np.nan)
    _check(lib().chip_debug_eq_invert(_pf(d), _pf(dinv), C.c_int64(len(d)), _pf(e), _pf(einv), C.c_int64(len(e))),
           "chip_debug_eq_invert")
    return dinv, einv


def debug_wnorm_batch(specs, nslots):
    """test hook: wnorm_batch on specs = [(v, w, slot), ...] (up to 8; v and w of one length per spec, and the SAME
    object where they are to alias) -> out[nslots], sums of (v w)^2; slots no spec names keep the NaN they held"""
    keep = {}

    def arr(a):
        if id(a) not in keep:
            keep[id(a)] = (a, _f(a))
        return keep[id(a)][1]

    count = len(specs)
    vs, ws = [arr(s[0]) for s in specs], [arr(s[1]) for s in specs]
    assert all(len(v) == len(w) for v, w in zip(vs, ws))
    pv, pw = (P_F64 * max(count, 1))(*[_pf(v) for v in vs]), (P_F64 * max(count, 1))(*[_pf(w) for w in ws])
    ns = np.ascontiguousarray([len(v) for v in vs], dtype=np.int32)
    slots = np.ascontiguousarray([s[2] for s in specs], dtype=np.int32)
    out = np.full(nslots, np.nan)
    _check(lib().chip_debug_wnorm_batch(C.c_int32(count), pv, pw, ns.ctypes.data_as(P_I32),
                                        slots.ctypes.data_as(P_I32), C.c_int32(nslots), _pf(out)),
           "chip_debug_wnorm_batch")
    return out


def debug_unscale(x, d, sx, z, e, sz, s, einv, ss):
    """test hook: unscale -> (xo, zo, so) = ((x d) sx, (z e) sz, (s einv) ss); the outputs hold NaN before the call"""
    x, d, z, e, s, einv = (_f(a) for a in (x, d, z, e, s, einv))
    n, m = len(x), len(z)
    assert len(d) == n and len(e) == m and len(s) == m and len(einv) == m
    xo, zo, so = np.full(n, np.nan), np.full(m, np.nan), np.full(m, np.nan)
    _check(lib().chip_debug_unscale(_pf(xo), _pf(x), _pf(d), C.c_double(sx), C.c_int64(n), _pf(zo), _pf(z), _pf(e),
                                    C.c_double(sz), _pf(so), _pf(s), _pf(einv), C.c_double(ss), C.c_int64(m)),
           "chip_debug_unscale")
    return xo, zo, so


def debug_ipm_info_update(info21, sq, tau, kappa, c, normq, normb):
    """test hook: DefaultInfo::update (csrc/ipm_info.hpp) on a flat info (its dots in [15:20]) from the eight squared
    weighted norms -> the updated copy"""
    info, sq = _f(info21).copy(), _f(sq)
    assert len(info) == 21 and len(sq) == 8
    _check(lib().chip_debug_ipm_info_update(_pf(info), _pf(sq), C.c_double(tau), C.c_double(kappa), C.c_double(c),
                                            C.c_double(normq), C.c_double(normb)), "chip_debug_ipm_info_update")
    return info


def debug_kkt_ints(kkt, name):
    """test hook: one int32 array of a HipKKTSolver by name (include/clarabel_hip_testing.h: chip_debug_kkt_ints)"""
    n = C.c_int64(0)
    f = lib().chip_debug_kkt_ints
    f.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64), C.c_void_p]
    _check(f(kkt._h, name.encode(), C.byref(n), None), "debug_kkt_ints")
    out = np.zeros(n.value, dtype=np.int32)
    _check(f(kkt._h, name.encode(), C.byref(n), out.ctypes.data_as(C.c_void_p)), "debug_kkt_ints")
    return out


def debug_factor_updates(kkt, bundle, what):
    """test hook: the update records of the flat bundle factorisation of one bundle of a host-only HipKKTSolver
    (include/clarabel_hip_testing.h: chip_debug_factor_updates): "records" / "leftover" as rows {level, a, b, k, target},
    "runs" as rows {level, first a, b, k, target, strides of a, b, k, target, count}"""
    n = C.c_int64(0)
    f = lib().chip_debug_factor_updates
    f.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.POINTER(C.c_int64), C.c_void_p]
    _check(f(kkt._h, int(bundle), what.encode(), C.byref(n), None), "debug_factor_updates")
    out = np.zeros(n.value, dtype=np.int32)
    _check(f(kkt._h, int(bundle), what.encode(), C.byref(n), out.ctypes.data_as(C.c_void_p)), "debug_factor_updates")
    return out.reshape(-1, 10 if what == "runs" else 5)


def debug_kkt_factors(kkt):
    """test hook: (Lx, D) of a HipKKTSolver as its last refactor left them (permuted numbering, CSC order of symbolic())"""
    nnzL = int(kkt.linear_solver_info().nnzL)
    Lx, D = np.zeros(max(nnzL, 1)), np.zeros(kkt.N)
    f = lib().chip_debug_kkt_factors
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _check(f(kkt._h, Lx.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p)), "debug_kkt_factors")
    return Lx[:nnzL], D


def set_device(ordinal):
    """hipSetDevice for this thread (one process per GPU: the rank's local device)"""
    rc = _hiprt().hipSetDevice(C.c_int(int(ordinal)))
    if rc != 0:
        raise RuntimeError("hipSetDevice(%d) failed: %d" % (ordinal, rc))


def device_synchronize():
    _hiprt().hipDeviceSynchronize()
