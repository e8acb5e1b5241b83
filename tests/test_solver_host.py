"""The L4 solver's host side (no GPU needed): chip_solver_settings_default against the reference's DefaultSettings,
the exported symbols of both builds, the refusal without a device, and the occupancy audit of equilibrate.hip."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clarabel.rs_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# src/solver/implementations/default/settings.rs: the #[builder(default = ...)] line above each field
REFERENCE_DEFAULTS = {
    "max_iter": 200,                        # settings.rs:31
    "time_limit": float("inf"),             # settings.rs:35
    "max_step_fraction": 0.99,              # settings.rs:43
    "tol_gap_abs": 1e-8,                    # settings.rs:47
    "tol_gap_rel": 1e-8,                    # settings.rs:51
    "tol_feas": 1e-8,                       # settings.rs:55
    "tol_infeas_abs": 1e-8,                 # settings.rs:59
    "tol_infeas_rel": 1e-8,                 # settings.rs:63
    "tol_ktratio": 1e-6,                    # settings.rs:67
    "reduced_tol_gap_abs": 5e-5,            # settings.rs:75
    "reduced_tol_gap_rel": 5e-5,            # settings.rs:79
    "reduced_tol_feas": 1e-4,               # settings.rs:83
    "reduced_tol_infeas_abs": 5e-12,        # settings.rs:87
    "reduced_tol_infeas_rel": 5e-5,         # settings.rs:91
    "reduced_tol_ktratio": 1e-4,            # settings.rs:95
    "equilibrate_enable": 1,                # settings.rs:99
    "equilibrate_max_iter": 10,             # settings.rs:103
    "equilibrate_min_scaling": 1e-4,        # settings.rs:107
    "equilibrate_max_scaling": 1e4,         # settings.rs:111
    "linesearch_backtrack_step": 0.8,       # settings.rs:115
    "min_switch_step_length": 1e-1,         # settings.rs:119
    "min_terminate_step_length": 1e-4,      # settings.rs:123
}


def test_solver_settings_default_is_the_reference_default(hip):
    s = hip.SolverSettings.default()
    for k, v in REFERENCE_DEFAULTS.items():
        assert getattr(s, k) == v, (k, getattr(s, k), v)
    lin = hip.Settings.default()
    assert bytes(s.linsys) == bytes(lin)  # the embedded linear-system settings are chip_settings_default's
    # keyword overrides reach the embedded settings
    assert hip.SolverSettings.default(device=hip.DEVICE_HOST_ONLY).linsys.device == hip.DEVICE_HOST_ONLY
    assert hip.SolverSettings.default(max_iter=7).max_iter == 7
    with pytest.raises(TypeError):  # a misspelt keyword is refused, not dropped
        hip.SolverSettings.default(max_iters=5)


def test_solver_settings_layout_matches_header(hip):
    """sizes of the two new structs as the C compiler lays them out"""
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "clarabel_hip.h"\nint main(void){printf("%zu %zu %zu",'
           ' sizeof(chip_solver_settings), sizeof(chip_solution_info), offsetof(chip_solver_settings, max_iter));'
           'return 0;}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(hip.SolverSettings), C.sizeof(hip.SolutionInfo), hip.SolverSettings.max_iter.offset]


SOLVER_SYMBOLS = ["chip_solver_settings_default", "chip_solver_create", "chip_solver_solve", "chip_solver_get_solution",
                  "chip_solver_get_solution_dev", "chip_solver_get_equilibration", "chip_solver_destroy"]


def test_solver_symbols_in_both_builds(hip):
    hdr = open(os.path.join(ROOT, "include", "clarabel_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(chip_solver_[a-z_]+)\s*\(", hdr)))
    assert declared == sorted(SOLVER_SYMBOLS)
    assert os.path.exists(hip.SHIP_LIB_PATH), "run __graft_entry__.build() (make ship)"
    for path in (hip.LIB_PATH, hip.SHIP_LIB_PATH):
        L = C.CDLL(path)
        for sym in SOLVER_SYMBOLS:
            assert hasattr(L, sym), (path, sym)


def test_solver_create_refuses_without_device(hip):
    """no CPU fallback: a host-only setting (or no GPU at all) makes chip_solver_create fail with ERR_NO_DEVICE"""
    P = hip.CscMatrix(2, 2, [0, 1, 3], [0, 0, 1], [4.0, 1.0, 2.0])
    A = hip.CscMatrix(2, 2, [0, 1, 2], [0, 1], [1.0, 1.0])
    with pytest.raises(hip.ChipError) as e:
        hip.HipSolver(P, [1.0, 1.0], A, [1.0, 1.0], [(hip.NonnegativeConeT, 2)],
                      hip.SolverSettings.default(device=hip.DEVICE_HOST_ONLY))
    assert e.value.code == hip.ERR_NO_DEVICE
    if hip.device_count() == 0:
        with pytest.raises(hip.ChipError) as e:
            hip.HipSolver(P, [1.0, 1.0], A, [1.0, 1.0], [(hip.NonnegativeConeT, 2)])
        assert e.value.code == hip.ERR_NO_DEVICE


def test_status_names_follow_solver_status(hip):
    # core/solver.rs:19-45
    assert hip.SOLVER_STATUS[:4] == ("Unsolved", "Solved", "PrimalInfeasible", "DualInfeasible")
    assert hip.SOLVER_STATUS[7] == "MaxIterations" and hip.SOLVER_STATUS[10] == "InsufficientProgress"
    assert len(hip.SOLVER_STATUS) == 12


# ---- occupancy audit of equilibrate.hip (the remark parsing of tests/test_kernel_resources.py) ----------------------
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-munsafe-fp-atomics",
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c"]
# every kernel of the translation unit: no scratch, and eight waves per SIMD (memory-bound passes want every wave)
EQ_KERNELS = ["k_eq_norms", "k_eq_factors", "k_eq_scale", "k_eq_cost_partial", "k_eq_cost_final", "k_eq_cost_apply",
              "k_eq_fill_one", "k_eq_rect_seg", "k_eq_rect_apply", "k_eq_invert", "k_wnorm_partial", "k_wnorm_final",
              "k_unscale"]


def _resources(src):
    out = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, src), "-o", os.devnull], cwd=CSRC, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_equilibrate_kernels_do_not_spill():
    res = _resources("equilibrate.hip")
    for k in EQ_KERNELS:
        names = [n for n in res if re.search(r"\d%s[EI]" % k, n)]
        assert len(names) == 1, (k, names)
        r = res[names[0]]
        assert r["ScratchSize"] == 0, (k, r)
        assert r["Occupancy"] >= 8, (k, r)
    assert len(res) == len(EQ_KERNELS), sorted(res)
