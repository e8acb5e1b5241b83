"""The stamped instance of k_sym_scale_write (CHIP_IR_DEBUG=3, cones.hip: soc_stamp): it is a kernel instance of its own,
launched only when stamps are asked for, so it must (a) leave exactly the K values, regulariser and cone verdict of the
plain instance and (b) write `<CHIP_IR_DEBUG_FILE>.scale` in the format tools/ir_skew.py reads: int32 G, then G x 32
int64 -- word 0 the hardware id, then the time stamps of a cone's ten phase boundaries, ascending."""
import numpy as np
import pytest

from tests import problems

pytestmark = pytest.mark.gpu


def test_stamped_instance_equals_the_plain_one(hip, tmp_path):
    import torch  # noqa: F401  (the extension shares torch's HIP runtime)
    if hip.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    pr = problems.portfolio_socp(4, 200, seed=3)  # four cones of 201 rows: the register form, one element per thread
    P = hip.CscMatrix(pr["n"], pr["n"], *pr["P"])
    A = hip.CscMatrix(pr["m"], pr["n"], *pr["A"])
    ks = hip.HipKKTSolver(P, A, pr["cones"], pr["m"], pr["n"])
    d_s, d_z = hip.DeviceArray(pr["s"]), hip.DeviceArray(pr["z"])

    def run():
        ks.update_scaled_enqueue(d_s.ptr, d_z.ptr)
        uok, sok = ks.collect()
        assert uok and sok == []
        return ks.values().view(np.uint64).copy(), ks.linear_solver_info().last_regularizer

    plain = run()
    base = str(tmp_path / "stamps.bin")
    hip.debug_set_switch("CHIP_IR_DEBUG_FILE", base)
    hip.debug_set_switch("CHIP_IR_DEBUG", "3")
    try:
        stamped = run()
    finally:
        hip.debug_set_switch("CHIP_IR_DEBUG", None)
        hip.debug_set_switch("CHIP_IR_DEBUG_FILE", None)
    assert np.array_equal(plain[0], stamped[0]) and plain[1] == stamped[1]
    raw = open(base + ".scale", "rb").read()
    G = int(np.frombuffer(raw[:4], dtype=np.int32)[0])
    assert G == 4 and len(raw) == 4 + G * 32 * 8
    t = np.frombuffer(raw[4:], dtype=np.int64).reshape(G, 32)
    counts = (t[:, 1:] > 0).sum(axis=1)
    print("  stamps per workgroup %s, a workgroup's span %s us" % (counts.tolist(), ((t[:, 10] - t[:, 1]) * 0.01).tolist()))
    assert (counts == 10).all()
    assert (np.diff(t[:, 1:11], axis=1) >= 0).all()
    assert np.array_equal(run()[0], plain[0])  # (and the plain instance again, after the switch is cleared)
