"""A batch of QPs / LPs as a differentiable torch layer: q, b and the values of P and A come from a model, the
members' solutions feed a loss.  Forward is HipBatchSolver.update + one batched solve, backward is
HipBatchSolver.backward (chip_bgrad_*: one KKT update and one KKT solve at the final iterates); with
tensors on the GPU nothing crosses to the host in either direction.

    solver = HipBatchSolver(problems)                    # the patterns and the initial values
    x, z, s = BatchQPFunction.apply(q, b, Px, Ax, solver)
    loss(x, z, s).backward()                             # fills q.grad, b.grad, Px.grad, Ax.grad

q[n], b[m], Px[nnz(P)], Ax[nnz(A)] are stacked float64 vectors in the stack's order (the positions update_P /
update_A index); any of them may be None: that piece keeps the solver's current values and gets no gradient.  Members
that did not end Solved, or own a SecondOrder cone, get zero gradients (solver.last_gradient.valid tells which).

Forward mode works through the same Function: under torch.autograd.forward_ad.dual_level() (or torch.func.jvp) the
tangents of (x, z, s) come from HipBatchSolver.jvp (chip_bjvp_*: one KKT solve at the final iterates per direction,
DESIGN.md 4.16); solver.last_tangent.valid tells which members have one.

Full sensitivities: batch_jacobians(solver, "q" | "b") gives every member's Jacobian of (x, z, s) with respect to its
own q or b as GPU tensors, in max_k w_k solves for the whole batch (chip_bjac_units).
batch_jacobian_rows(solver, "x" | "z" | "s", wrt) builds the same Jacobians row by row, which also reaches the stored
entries of P and A (wrt any subset of "qbPA"), and batch_vjp_block(solver, GX, GZ, GS, want) runs K backwards at once
with one host synchronisation per 16 (chip_bvjp_*).  BatchQPFunction itself is unchanged."""
import torch


def batch_jacobians(solver, wrt="q"):
    """the Jacobians of the members' solutions of the solver's last solve with respect to their own q or b, on the
    GPU: a list with one entry per member, None where the member has no derivative, else (dx_dw [n_k x w_k],
    dz_dw [m_k x w_k], ds_dw [m_k x w_k]) -- HipBatchSolver.member_jacobians(wrt, torch=True)"""
    return solver.member_jacobians(wrt, torch=True)


def batch_vjp_block(solver, GX=None, GZ=None, GS=None, want="qbPA"):
    """K cotangents of the solver's last solve at once: GX [K, n], GZ [K, m], GS [K, m] (float64 GPU tensors; None =
    zeros) -> a BatchGradientBlock of GPU tensors holding the pieces named in `want`, with one host synchronisation
    per 16 cotangents -- HipBatchSolver.backward_block (chip_bvjp_*)"""
    return solver.backward_block(gx=GX, gz=GZ, gs=GS, want=want)


def batch_jacobian_rows(solver, of="x", wrt="qb"):
    """the Jacobians of the members' x, z or s of the solver's last solve with respect to their own q, b and the
    stored entries of their P and A, on the GPU: a list with one entry per member, None where the member has no
    derivative, else {key: [len(of)_k x w_k]} -- HipBatchSolver.member_jacobian_rows(of, wrt, torch=True)"""
    return solver.member_jacobian_rows(of, wrt, torch=True)


class BatchQPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, b, Px, Ax, solver):
        pieces = {"P": Px, "q": q, "A": Ax, "b": b}
        solver.update(**{k: (None if v is None else v.detach()) for k, v in pieces.items()})
        x, s, z = solver.solve_torch()
        ctx.solver = solver
        ctx.generation = solver.generation  # backward differentiates the LAST solve of the handle: which one this was
        ctx.device = x.device
        ctx.like = [None if v is None else (v.device, v.dtype) for v in (q, b, Px, Ax)]
        return x, z, s

    @staticmethod
    def backward(ctx, gx, gz, gs):
        solver = ctx.solver
        if solver.generation != ctx.generation:
            raise RuntimeError("BatchQPFunction.backward: the solver has been solved again since this forward")
        dev = ctx.device
        prep = lambda g: None if g is None else g.detach().to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
        if gx is None and gz is None and gs is None:
            gx = torch.zeros(solver.stack["n"], dtype=torch.float64, device=dev)
        g = solver.backward(gx=prep(gx), gz=prep(gz), gs=prep(gs))
        solver.last_gradient = g
        outs = (g.dq, g.db, g.dP, g.dA)
        grads = [None if like is None or not need else o.to(device=like[0], dtype=like[1])
                 for o, like, need in zip(outs, ctx.like, ctx.needs_input_grad[:4])]
        return grads[0], grads[1], grads[2], grads[3], None

    @staticmethod
    def jvp(ctx, tq, tb, tPx, tAx, _):
        solver = ctx.solver
        if solver.generation != ctx.generation:
            raise RuntimeError("BatchQPFunction.jvp: the solver has been solved again since this forward")
        dev = ctx.device
        prep = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float64).contiguous()  # noqa: E731
        t = solver.jvp(dq=prep(tq), db=prep(tb), dP=prep(tPx), dA=prep(tAx))
        solver.last_tangent = t
        return t.dx, t.dz, t.ds
