"""The resource figures of the fused KKT solve's two instances and of every other kernel of the three bundle files
(no GPU needed: hipcc cross-compiles gfx950).

k_bundle_irs_fixed is k_bundle_irs with the usual switches folded at compile time (csrc/bundle_ir.hip: irs_body, FIXED).
What it is for is its register figures -- no scratch, no spilled VGPR, four waves per SIMD -- so they are asserted here,
beside the general instance's (which must not pay for sharing its body) and the parent commit's figures of the other
kernels in those files (which must not change at all)."""
import os
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests.test_kernel_resources import HIPCC, _resources

FILES = ("bundle_ir.hip", "bundle_gstep.hip", "bundle_solve.hip")

# (file, mangled name, VGPRs, scratch bytes per lane, waves per SIMD) from a compile of the parent commit 432f0fa with the
# flags of tests/test_kernel_resources.py; k_bundle_irs<256, 4> itself stood at 128 VGPRs, 16 spilled, 68 B, occupancy 4
PARENT = [
    ("bundle_ir.hip", "_ZN4chip3dev12_GLOBAL__N_111k_bundle_irILi256ELb1EEEvNS0_7LdlViewENS0_10BundleViewENS0_8FoldViewENS0_6IrViewENS0_9GFoldViewE", 128, 96, 4),
    ("bundle_ir.hip", "_ZN4chip3dev12_GLOBAL__N_111k_bundle_irILi1024ELb1EEEvNS0_7LdlViewENS0_10BundleViewENS0_8FoldViewENS0_6IrViewENS0_9GFoldViewE", 128, 96, 4),
    ("bundle_ir.hip", "_ZN4chip3dev12_GLOBAL__N_111k_bundle_irILi512ELb1EEEvNS0_7LdlViewENS0_10BundleViewENS0_8FoldViewENS0_6IrViewENS0_9GFoldViewE", 80, 292, 6),
    ("bundle_ir.hip", "_ZN4chip3dev12_GLOBAL__N_111k_bundle_irILi256ELb0EEEvNS0_7LdlViewENS0_10BundleViewENS0_8FoldViewENS0_6IrViewENS0_9GFoldViewE", 128, 80, 4),
    ("bundle_ir.hip", "_ZN4chip3dev12_GLOBAL__N_111k_bundle_irILi1024ELb0EEEvNS0_7LdlViewENS0_10BundleViewENS0_8FoldViewENS0_6IrViewENS0_9GFoldViewE", 128, 80, 4),
    ("bundle_ir.hip", "_ZN4chip3dev12_GLOBAL__N_111k_bundle_irILi512ELb0EEEvNS0_7LdlViewENS0_10BundleViewENS0_8FoldViewENS0_6IrViewENS0_9GFoldViewE", 80, 268, 6),
    ("bundle_gstep.hip", "_ZN4chip3dev12_GLOBAL__N_114k_gstep_factorENS0_7LdlViewENS0_10BundleViewENS0_9GFoldViewENS0_9GStepViewE", 121, 0, 4),
    ("bundle_gstep.hip", "_ZN4chip3dev12_GLOBAL__N_113k_gstep_solveILi6ELi8ELi3EEEvNS0_7LdlViewENS0_10BundleViewENS0_6IrViewENS0_9GFoldViewENS0_9GStepViewE", 128, 20, 4),
    ("bundle_gstep.hip", "_ZN4chip3dev12_GLOBAL__N_113k_gstep_solveILi8ELi10ELi4EEEvNS0_7LdlViewENS0_10BundleViewENS0_6IrViewENS0_9GFoldViewENS0_9GStepViewE", 128, 68, 4),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_112k_bundle_fwdENS0_7LdlViewENS0_10BundleViewEPdNS0_8FoldViewE", 64, 8, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_112k_bundle_bwdENS0_7LdlViewENS0_10BundleViewEPdPKd", 50, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_113k_bundle_symvENS0_10BundleViewEPKiS4_PKdS6_S6_PdPyPiNS0_8FoldViewE", 56, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_116k_fold_top_solveENS0_7LdlViewENS0_8FoldViewEPd", 54, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_119k_fold_top_residualENS0_8FoldViewEPKdS4_S4_PdPyPi", 40, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_114k_topblk_buildENS0_7LdlViewENS0_10TopBlkViewE", 16, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_111k_norm_rowsEPKdPKiiPyPi", 6, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_119k_bundle_sweep_flatILb1EEEvNS0_7LdlViewENS0_10BundleViewEPdPKd", 42, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_119k_bundle_sweep_flatILb0EEEvNS0_7LdlViewENS0_10BundleViewEPdPKd", 47, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_115k_gather_mergedILi0EEEvNS0_10GatherArgsEPKiiS5_iS5_S5_S5_ii", 42, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_115k_gather_mergedILi1EEEvNS0_10GatherArgsEPKiiS5_iS5_S5_S5_ii", 42, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_115k_gather_mergedILi3EEEvNS0_10GatherArgsEPKiiS5_iS5_S5_S5_ii", 42, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_115k_gather_mergedILi2EEEvNS0_10GatherArgsEPKiiS5_iS5_S5_S5_ii", 44, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_113k_topblk_stepILi0EEEvNS0_7LdlViewENS0_10TopBlkViewEPdiS5_Pi", 42, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_113k_topblk_stepILi1EEEvNS0_7LdlViewENS0_10TopBlkViewEPdiS5_Pi", 42, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_17k_chainILi0EEEvNS0_10GatherArgsEPKiS5_S5_S5_ii", 56, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_17k_chainILi1EEEvNS0_10GatherArgsEPKiS5_S5_S5_ii", 56, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_114k_gather_BprepILi0EEEvNS0_10GatherArgsEPKii", 0, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_114k_gather_BprepILi1EEEvNS0_10GatherArgsEPKii", 8, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_114k_gather_BprepILi3EEEvNS0_10GatherArgsEPKii", 4, 0, 8),
    ("bundle_solve.hip", "_ZN4chip3dev12_GLOBAL__N_114k_gather_BprepILi2EEEvNS0_10GatherArgsEPKii", 4, 0, 8),
]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("no hipcc")
    with ThreadPoolExecutor(len(FILES)) as pool:  # (three compiler processes side by side)
        return dict(zip(FILES, pool.map(_resources, FILES)))


def _one(res, *parts):
    names = [n for n in res if all(p in n for p in parts)]
    assert len(names) == 1, (parts, names)
    return res[names[0]]


def test_fixed_instance_has_no_scratch(resources):
    r = _one(resources["bundle_ir.hip"], "k_bundle_irs_fixed", "ILi256ELi4E")
    print("k_bundle_irs_fixed<256, 4>:", r)
    assert r["Occupancy"] >= 4, r
    assert r["ScratchSize"] == 0, r
    assert r["VGPRs Spill"] == 0, r


def test_general_instance_is_no_worse_than_the_parent(resources):
    r = _one(resources["bundle_ir.hip"], "12k_bundle_irsILi256ELi4E")
    print("k_bundle_irs<256, 4>:", r)
    assert r["ScratchSize"] <= 68, r
    assert r["VGPRs Spill"] <= 16, r
    assert r["Occupancy"] >= 4, r


def test_other_bundle_kernels_keep_the_parents_figures(resources):
    seen = {src: set() for src in FILES}
    for src, name, vgprs, scratch, occ in PARENT:
        assert name in resources[src], name
        r = resources[src][name]
        assert (r["VGPRs"], r["ScratchSize"], r["Occupancy"]) == (vgprs, scratch, occ), (name, r)
        seen[src].add(name)
    # (nothing else but the two instances of the fused solve)
    for src in FILES:
        rest = [n for n in resources[src] if n not in seen[src] and "k_bundle_irs" not in n]
        assert not rest, rest
