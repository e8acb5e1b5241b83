"""bench.py's own options: a plain run holds the timed steps only (every other figure needs --full), `--steps` is the
number of timed steps, and `--dump-outputs DIR` writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from tests import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_whole_or_a_fixed_sample(tmp_path):
    arrays = {"small": np.arange(100.0), "big": np.arange(5000.0)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays, budget=1 << 20)
    for name, a in arrays.items():
        got = np.load(tmp_path / "whole" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a)
    # over the budget: the array longer than its share (budget / 8 / 2 = 1000 entries) is sampled, the other kept whole
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=8 * 2000)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"])
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.dtype == np.float64 and big.size == 1000
    assert np.all(np.diff(big) > 0) and np.all(np.isin(big, arrays["big"]))   # distinct entries, in their order
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))            # the same entries run to run


def test_bench_rejects_zero_steps():
    out = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_timed_solutions(tmp_path, hip, oracle):
    """two plain runs of a small config-3 instance: the line carries the timed steps only, and the dumped solutions are
    the oracle's for the same inputs, right-hand sides and permutation (one refinement round, as timed)"""
    cmd = [sys.executable, BENCH, "--nblocks", "20", "--blocksize", "50", "--steps", "3", "--warmup", "1"]
    lines = []
    for d in ("a", "b"):
        out = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads(out.stdout.strip().splitlines()[-1]))
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "iterations/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) <= 1e-2   # (both rounded on the line)
    for key in ("roofline", "roofline_events_pass", "parity", "cpu_baseline", "cpu_baseline_mt", "batched_c4", "c2", "c5",
                "l1_dropin"):
        assert line[key] is None, key
    pr = problems.portfolio_socp(20, 50, seed=3)
    n, m = pr["n"], pr["m"]
    rng = np.random.default_rng(1234)   # (bench.py's right-hand sides of rank 0)
    rhs = [(rng.standard_normal(n), rng.standard_normal(m)) for _ in range(3)]
    ks = hip.HipKKTSolver(hip.CscMatrix(n, n, *pr["P"]), hip.CscMatrix(m, n, *pr["A"]), pr["cones"], m, n)
    ost = oracle.Settings.default()
    ost.ir_max_iter, ost.ir_reltol, ost.ir_abstol = 1, 0.0, 0.0
    cones = oracle.Cones(pr["cones"])
    assert cones.update_scaling(pr["s"], pr["z"])
    ko = oracle.KKTSolver(n, m, pr["P"], pr["A"], cones, settings=ost, perm=ks.perm)
    assert ko.update()
    assert sorted(os.listdir(tmp_path / "a")) == ["solution_0.npy", "solution_1.npy", "solution_2.npy"]
    for k, (rx, rz) in enumerate(rhs):
        got = np.load(tmp_path / "a" / ("solution_%d.npy" % k))
        ko.setrhs(rx, rz)
        ok, x, z = ko.solve()
        assert ok
        ref = np.concatenate([x, z])
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert bench.relerr(got, ref) <= bench.TOL
        assert bench.relerr(np.load(tmp_path / "b" / ("solution_%d.npy" % k)), got) <= 1e-12
