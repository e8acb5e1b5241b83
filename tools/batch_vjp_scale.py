"""Scale run of the batched solver's blocks of cotangents (chip_bvjp_*, HipBatchSolver.backward_block /
member_jacobian_rows) on the batches of tools/batch_jac_scale.py: synthetic.portfolio_qp(n_assets, n_factors,
seed=200+i).  For every batch size, on ONE handle in ONE process with host clocks around synchronised calls, medians of
--repeats after a warm-up:
  a 16-cotangent block with device inputs (chip_bvjp_apply_dev) that reuses the factorisation, at want = q|b and at
  want = q|b|P|A, as ms per cotangent;
  the first block after a solve (it pays the scaling update and the refactor), each measured behind a solve of its own;
  a single backward, device inputs (chip_bgrad_backward_dev), which refactors on every call: the yardstick;
  the device work of member_jacobian_rows("x", "qbA"): the ceil(max n_k / 16) calls of chip_bvjp_units, against max n_k
  single backwards;
the bytes of the block's buffers as a function of want, its launch and synchronisation counts, and the worst relative
difference of a block's cotangents against the dense numpy restatement tests/adjoint_ref.py on up to --check sampled
members at the device's own solution.  Prints one JSON object per batch size and, with --out FILE, rewrites FILE after
every size."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--assets", type=int, default=2000)
    ap.add_argument("--factors", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", type=int, default=4, help="members compared with the dense restatement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    hip = g.load_package()
    from clarabel_rs_amd import synthetic
    from tests import adjoint_ref as R

    def clock(fn, before=None, warm=True):
        if warm:
            if before:
                before()
            fn()
        ts = []
        for _ in range(a.repeats):
            if before:
                before()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return {"min_ms": 1e3 * min(ts), "median_ms": 1e3 * float(np.median(ts))}

    K = hip.BVJP_MAX_DIR
    QB, ALL, QBA = 3, 15, 11
    res = {"problem": "portfolio_qp(%d, %d, seed=200+i)" % (a.assets, a.factors), "cotangents_per_block": K, "runs": []}
    for nprob in a.nprob:
        prs = [synthetic.portfolio_qp(a.assets, a.factors, seed=200 + i) for i in range(nprob)]
        mem = [(hip.CscMatrix(p["n"], p["n"], *p["P"]), p["q"], hip.CscMatrix(p["m"], p["n"], *p["A"]), p["b"],
                p["cones"]) for p in prs]
        bs = hip.HipBatchSolver(mem)
        sols = bs.solve()
        iters = max(s.iterations for s in sols)
        n, m, nP, nA = bs.stack["n"], bs.stack["m"], len(bs.stack["P"][2]), len(bs.stack["A"][2])
        even = lambda v: (v + 1) // 2 * 2  # noqa: E731
        work = 8 * 3 * (even(n) + even(m))  # per cotangent: D gx, gs / e, the right-hand side, the solution
        run = {"nprob": nprob, "n": n, "m": m, "nnzP": nP, "nnzA": nA, "iterations_max": iters,
               "solved": sum(s.status == "Solved" for s in sols),
               "ms_per_iteration": 1e3 * sols[0].iteration_time / max(iters, 1),
               "bytes_per_cotangent_want_qb": work + 8 * (n + m),
               "bytes_per_cotangent_want_qbA": work + 8 * (n + m + nA),
               "bytes_per_cotangent_want_qbPA": work + 8 * (n + m + nP + nA)}
        gen = torch.Generator(device="cuda").manual_seed(1)  # (16 cotangents of the stack: drawn where they are used)
        gg = [torch.randn((K, k), dtype=torch.float64, device="cuda", generator=gen) for k in (n, m, m)]
        torch.cuda.synchronize()
        blk = bs.backward_block(*gg)  # allocates the block's buffers, factors K at the final iterates; the result checked
        run["valid"] = int(np.sum(blk.valid))
        L = hip.lib()
        bptr = [C.c_void_p(t.data_ptr()) for t in gg]
        sptr = [C.c_void_p(t[0].data_ptr()) for t in gg]
        block = lambda want: hip._check(L.chip_bvjp_apply_dev(bs._h, K, want, *bptr), "block")  # noqa: E731
        single = lambda: hip._check(L.chip_bgrad_backward_dev(bs._h, *sptr), "backward")  # noqa: E731
        single()  # (allocates the single backward's buffers)
        run["block16_qb_reusing"] = clock(lambda: block(QB))
        run["block16_qbPA_reusing"] = clock(lambda: block(ALL))
        run["backward_single"] = clock(single)
        # (alternating once more: the three are compared, so none should own the quieter moment)
        run["block16_qb_reusing_again"] = clock(lambda: block(QB))
        run["block16_qbPA_reusing_again"] = clock(lambda: block(ALL))
        run["backward_single_again"] = clock(single)
        run["block16_qb_first_after_solve"] = clock(lambda: block(QB), before=bs.solve, warm=False)
        run["block16_qbPA_first_after_solve"] = clock(lambda: block(ALL), before=bs.solve, warm=False)
        one = run["backward_single"]["median_ms"]
        for key in ("qb", "qbPA"):
            per = run["block16_%s_reusing" % key]["median_ms"] / K
            run["ms_per_cotangent_%s_reusing" % key] = per
            run["backward_over_cotangent_%s_reusing" % key] = one / per
            per = run["block16_%s_first_after_solve" % key]["median_ms"] / K
            run["ms_per_cotangent_%s_first" % key] = per
            run["backward_over_cotangent_%s_first" % key] = one / per
        height = int(max(bs.n_part))

        def units_calls():
            for first in range(0, height, K):
                hip._check(L.chip_bvjp_units(bs._h, 0, C.c_int64(first), min(K, height - first), QBA), "units")
        block(ALL)  # (K is factored at the final iterates again after the solves above)
        run["jacobian_x_rows"] = height
        run["jacobian_x_rows_qbA_units_calls"] = clock(units_calls, warm=False)
        run["jacobian_x_rows_as_single_backwards_ms"] = height * one
        run["single_backwards_over_units_calls"] = (run["jacobian_x_rows_as_single_backwards_ms"]
                                                    / run["jacobian_x_rows_qbA_units_calls"]["median_ms"])
        try:
            for key, want, first in (("qb", QB, False), ("qbPA", ALL, False), ("qbPA_first", ALL, True)):
                if first:
                    bs.solve()
                block(want)
                run["vjp_launches_" + key] = bs.debug_counter("vjp_launches")
                run["vjp_host_syncs_" + key] = bs.debug_counter("vjp_host_syncs")
            run["vjp_repeats"] = bs.debug_counter("vjp_repeats")
            run["vjp_refactors"] = bs.debug_counter("vjp_refactors")
            single()
            run["backward_launches"] = bs.debug_counter("backward_launches")
            run["backward_host_syncs"] = bs.debug_counter("backward_host_syncs")
        except Exception:  # (a library without the test hooks)
            pass
        keys = ("q", "b", "b")
        off = {k: np.asarray(bs._offsets[k]).astype(int) for k in set(keys)}
        picks = sorted(set(np.linspace(0, nprob - 1, min(a.check, nprob)).astype(int).tolist()))
        worst = 0.0
        for k in picks:
            if sols[k].status != "Solved":
                continue
            for t in ((0, K - 1) if k == picks[0] else (K - 1,)):  # (a dense solve of n_k + m_k unknowns each)
                want = R.adjoint(prs[k], sols[k].x, sols[k].s, sols[k].z,
                                 *[v[t, off[key][k]:off[key][k + 1]].cpu().numpy() for v, key in zip(gg, keys)])
                for w, got in zip(want, blk.per_member(k)):
                    worst = max(worst, R.rel(got[t].cpu().numpy(), w))
        run["checked_members"] = picks
        run["worst_gradient_difference"] = worst
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
        del bs, blk, gg


if __name__ == "__main__":
    main()
