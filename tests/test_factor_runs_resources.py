"""Occupancy audit of the run-coded bundle factorisation (no GPU needed: hipcc cross-compiles gfx950), beside
tests/test_kernel_resources.py: k_bundle_factor_runs (up to 4096 nodes per bundle, the records outside runs one per
thread) must keep two workgroups of 1024 threads per CU -- 8 waves per SIMD --
without scratch: the kernel it stands in for, k_bundle_factor_flat<4>, spills 44 bytes per lane, and the run loop
compiled into that kernel beside its 8-record batch spilled 68."""
import os
import shutil

import pytest

from tests.test_kernel_resources import HIPCC, _resources

# kernel (substring of the mangled name) -> (fewest waves per SIMD, most scratch bytes per lane)
DESIGNED = {
    "20k_bundle_factor_runsE": (8, 0),
    "20k_bundle_factor_flatILi4E": (8, 44),  # a handle without runs executes what it executed before: the same figures
}


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("make") is None, reason="no hipcc")
def test_run_kernel_reaches_its_designed_occupancy():
    res = _resources("bundle_factor.hip")
    for key, (occ_min, scratch_max) in DESIGNED.items():
        names = [n for n in res if key in n]
        assert len(names) == 1, (key, names)
        r = res[names[0]]
        print(key, r)
        assert r["Occupancy"] >= occ_min, (key, r)
        assert r["ScratchSize"] <= scratch_max, (key, r)
