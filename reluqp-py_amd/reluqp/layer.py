"""Differentiable QP layer: ``x, y = ReLUQPLayer()(H, g, A, l, u)`` solves

    min 1/2 x'Hx + g'x   s.t.   l <= A x <= u

for a batch on the GPU and back-propagates through the solution with the library's adjoint (C-ABI rqp_adjoint, DESIGN.md
section 5 "Adjoint (autograd)").  The backward pass solves the reduced KKT system of each instance's active set; it is
exact where the active set is strictly complementary and non-degenerate, the one-sided derivative on rows sitting exactly on
a bound with a zero multiplier, and the delta-regularised solution on degenerate active sets (``Gradients.residual``).
With ``ReLUQPLayer(sensitivity=True)`` forward-mode AD (``torch.autograd.forward_ad``) works too: ``QPFunction.jvp`` pushes the
input tangents through the same reduced KKT system (C-ABI rqp_sensitivity, DESIGN.md section 5 "Forward sensitivities").

Host code is plumbing: handle bookkeeping, reshapes and casts.  The batch sums of broadcast inputs are the only reductions.
"""
import torch

from reluqp import _cabi, mpc
from reluqp.reluqpth import ReLU_QP

_NAMES = ("dH", "dg", "dA", "dl", "du")


class QPFunction(torch.autograd.Function):
    """``QPFunction.apply(layer, return_z, H, g, A, l, u)`` -> ``(x, y)`` or ``(x, y, z)`` (z without a gradient)."""

    @staticmethod
    def forward(ctx, layer, return_z, H, g, A, l, u):
        solver, shapes = layer._solve(H, g, A, l, u)
        res = solver.results
        qp = solver.QP
        x, y, z = res.x.clone(), res.y.clone(), res.z.clone()
        status = torch.as_tensor(res.info.status_code).to(device=x.device, dtype=torch.int32).reshape(-1).clone()
        ctx.solver, ctx.shapes, ctx.return_z = solver, shapes, return_z
        ctx.save_for_backward(qp.H, qp.A, qp.l, qp.u, x, z, y, status)
        ctx.save_for_forward(qp.H, qp.A, qp.l, qp.u, x, z, y, status)
        ctx.mark_non_differentiable(z)
        return (x, y, z) if return_z else (x, y)

    @staticmethod
    def backward(ctx, gx, gy, gz=None):
        H, A, l, u, x, z, y, status = ctx.saved_tensors
        shapes = ctx.shapes
        want = tuple(k for k, need in zip(_NAMES, ctx.needs_input_grad[2:]) if need)
        if not want:
            return (None,) * 7
        solver = ctx.solver
        gx = gx.reshape(x.shape)
        gy = None if gy is None else gy.reshape(y.shape)
        gr = solver.adjoint_at(H, A, l, u, x, z, y, gx, gy, status=status, want=want)
        grads = [None, None]
        for k, (shape, dtype, batched_in) in zip(_NAMES, shapes["inputs"]):
            d = getattr(gr, k)
            if d is None or k not in want:
                grads.append(None)
                continue
            if shapes["broadcast"] and not batched_in and k in ("dg", "dl", "du"):
                d = d.sum(0)                                   # an un-batched input broadcast over the batch
            grads.append(d.reshape(shape).to(dtype))
        return tuple(grads)


    @staticmethod
    def jvp(ctx, _layer, _return_z, dH, dg, dA, dl, du):
        """Tangents of (x, y) along the input tangents (None for z): one direction, through ReLU_QP.jvp_at.  A tangent of an
        input without the batch axis (shared H / A, or g / l / u broadcast over the batch) is passed as a shared one."""
        H, A, l, u, x, z, y, status = ctx.saved_tensors
        solver = ctx.solver
        if not solver._sens_reserved:
            raise RuntimeError("forward-mode AD through ReLUQPLayer needs ReLUQPLayer(sensitivity=True)")
        prec = x.dtype
        tan = {k: None if t is None else t.to(prec) for k, t in zip(_NAMES, (dH, dg, dA, dl, du))}
        s = solver.jvp_at(H, A, l, u, x, z, y, status=status, **tan)
        dx, dy = s.dx.reshape(x.shape), s.dy.reshape(y.shape)
        return (dx, dy, None) if ctx.return_z else (dx, dy)


class ReLUQPLayer(torch.nn.Module):
    """A batched QP as a differentiable module.  ``forward(H, g, A, l, u)`` returns ``(x, y)`` (``(x, y, z)`` with
    ``return_z=True``).  H [n, n] / A [m, n] are shared by the batch, [B, n, n] / [B, m, n] per instance; g, l, u are [B, .]
    or un-batched (then broadcast over the batch of the other inputs, and their gradients summed over it).

    One solver handle is kept per (shapes, dtype, device); ``setup`` runs on first use, ``update(Hx=, Ax=)`` when H or A is
    not the previous call's tensor (another object, or modified in place), then ``update(g, l, u)`` and ``solve()``.  The
    keyword arguments are those of ``ReLU_QP.setup`` (defaults here: ``differentiable=True``, ``polish=True``,
    ``precision`` = the dtype of g).  ``sensitivity=True`` also reserves the forward sensitivities: forward-mode AD
    (``torch.autograd.forward_ad``, ``gradcheck(..., check_forward_ad=True)``) then works through the layer."""

    def __init__(self, return_z=False, **setup_kwargs):
        super().__init__()
        self.return_z = bool(return_z)
        kw = dict(differentiable=True, polish=True)
        kw.update(setup_kwargs)
        if not kw["differentiable"]:
            raise ValueError("ReLUQPLayer needs differentiable=True")
        self.setup_kwargs = kw
        self._handles = {}

    def forward(self, H, g, A, l, u):
        return QPFunction.apply(self, self.return_z, H, g, A, l, u)

    def _solve(self, H, g, A, l, u):
        dev = g.device
        if dev.type != "cuda":
            raise _cabi.RqpUnavailable("ReLUQPLayer needs a HIP device; the MI355X build has no CPU path")
        prec = self.setup_kwargs.get("precision", g.dtype if g.dtype in (torch.float32, torch.float64) else torch.float64)
        n, m = H.shape[-1], A.shape[-2]
        bs = [t.shape[0] for t, d in ((H, 3), (g, 2), (A, 3), (l, 2), (u, 2)) if t.dim() == d]
        B = max(bs) if bs else None
        batched = B is not None
        broadcast = batched and any(t.dim() == 1 for t in (g, l, u))
        shared = batched and H.dim() == 2
        if batched and (H.dim() == 2) != (A.dim() == 2):
            raise ValueError("H and A must both be shared ([n, n], [m, n]) or both per instance")
        # (shape, dtype, batched) of every input as the caller passed it: the gradients go back to these
        inputs = [(tuple(t.shape), t.dtype, t.dim() == d) for t, d in ((H, 3), (g, 2), (A, 3), (l, 2), (u, 2))]
        if batched:
            g, l, u = (t.expand(B, t.shape[-1]) if t.dim() == 1 else t for t in (g, l, u))
        shapes = dict(broadcast=broadcast, inputs=inputs)
        key = (n, m, B, shared, prec, dev)
        ent = self._handles.get(key)
        if ent is None:
            kw = dict(self.setup_kwargs)
            kw.update(device=dev, precision=prec)
            solver = ReLU_QP()
            solver.setup(H, g, A, l, u, **kw)
            ent = self._handles[key] = dict(solver=solver, H=(H, H._version), A=(A, A._version))
        else:
            solver = ent["solver"]
            newH = not (ent["H"][0] is H and ent["H"][1] == H._version)
            newA = not (ent["A"][0] is A and ent["A"][1] == A._version)
            if newH or newA:
                solver.update(Hx=H if newH else None, Ax=A if newA else None)
                ent["H"], ent["A"] = (H, H._version), (A, A._version)
            solver.update(g=g, l=l, u=u)
        solver.solve()
        return solver, shapes


def _ltv_layer_weights(cd, slot, B, device, Q, R, Qf):
    """The weights of one forward as the C-ABI reads them: (``mpc._LtvWeights``, (Qd, Rd, Qfd)), symmetric float64 device
    tensors.  Q, R both matrices: the shared weights.  Q or R with a stage axis ([N, ., .] or [B, N, ., .]): stage weights, both
    expanded to [B, N, ., .] on the device (a shared Q as Q, ..., Q, Qf) and Qfd = None."""
    if Q.dim() == 2 and R.dim() == 2:
        f64 = lambda W: (0.5 * (W.detach() + W.detach().transpose(0, 1))).to(device=device, dtype=torch.float64).contiguous()
        Qd, Rd, Qfd = f64(Q), f64(R), f64(Qf)
        return mpc._LtvTensorWeights(Qd, Rd, Qfd, slot["K"]), (Qd, Rd, Qfd)
    Qd, Rd, _, _ = mpc._LtvStageWeights(cd.nx, cd.nu, cd.horizon, Q.detach(), R.detach(), None if Qf is None else Qf.detach(),
                                        None).on(device, B)
    return mpc._LtvStageTensorWeights(Qd, Rd, slot["K"]), (Qd, Rd, None)


def _ltv_saved_weights(slot, Qd, Rd, Qfd):
    return mpc._LtvStageTensorWeights(Qd, Rd, slot["K"]) if Qfd is None else mpc._LtvTensorWeights(Qd, Rd, Qfd, slot["K"])


class LTVCondenseFunction(torch.autograd.Function):
    """``LTVCondenseFunction.apply(condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, l_add, u_add)`` -> ``(H, A, g, l, u)``: the
    condensed QPs of a batch of LTV plants (C-ABI rqp_ltv_condense + rqp_ltv_vectors) with their reverse mode (C-ABI
    rqp_ltv_condense_adjoint, DESIGN.md section 5 "LTV condensing, adjoint").  ``condenser`` is an ``mpc.LTVCondenser``; Ad
    [B, N, nx, nx], Bd [B, N, nx, nu], x0 [B, nx] are device tensors of one precision, c [B, N, nx], xref [B, N, nx], uref
    [B, N, nu] may be None, Q, R, Qf are symmetric tensors (their symmetric part is used, their gradients are symmetric),
    l_add / u_add [m] or [B, m].  Only the gradients that ``needs_input_grad`` names are computed.
    Stage weights: Q and / or R may be [N, ., .] or [B, N, ., .] (Q_k weighs x_{k+1}; a staged Q comes with ``Qf=None``, a shared
    Q beside a staged R is repeated as Q, ..., Q, Qf); their gradients come back in the input's shape and dtype, summed over
    the batch only where the input has no batch axis."""

    @staticmethod
    def forward(ctx, condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, l_add, u_add):
        cd = condenser
        dtype, device, B = Ad.dtype, Ad.device, Ad.shape[0]
        slot = cd.slot(B, device, dtype)
        w, (Qd, Rd, Qfd) = _ltv_layer_weights(cd, slot, B, device, Q, R, Qf)
        det = lambda t: None if t is None else t.detach().contiguous()
        Ad, Bd, c, x0, xref, uref = (det(t) for t in (Ad, Bd, c, x0, xref, uref))
        slot["stamp"] = ctx.stamp = cd.next_stamp()
        H, A = mpc.condense_ltv_device(Ad, Bd, w, slot["ws"], c=c)
        g, l, u = mpc.ltv_vectors_device((cd.nx, cd.nu, cd.horizon, cd.K is not None, c is not None), x0, l_add.detach(),
                                         u_add.detach(), w, slot["ws"], xref=xref, uref=uref)
        ctx.condenser, ctx.slot = cd, slot
        ctx.meta = (Q.dtype, R.dtype, None if Qf is None else Qf.dtype, l_add.dim(), u_add.dim(), l_add.dtype, u_add.dtype)
        ctx.wdims = (Q.dim(), R.dim())
        ctx.save_for_backward(Ad, Bd, c, x0, xref, uref, Qd, Rd, Qfd)
        ctx.set_materialize_grads(False)
        return H, A, g, l, u

    @staticmethod
    def restore(ctx):
        """The forward workspace of this ctx's linearisation: condensed again from the saved inputs when a later forward has
        overwritten it.  Returns (slot, weights)."""
        Ad, Bd, c, x0, xref, uref, Qd, Rd, Qfd = ctx.saved_tensors[:9]
        slot = ctx.slot
        w = _ltv_saved_weights(slot, Qd, Rd, Qfd)
        if slot["stamp"] != ctx.stamp:
            Hs, As = ctx.condenser.recondense_outputs(slot, Ad.shape[0], Ad.device, Ad.dtype)
            mpc.condense_ltv_device(Ad, Bd, w, slot["ws"], c=c, H=Hs, A=As)
            slot["stamp"] = ctx.stamp
        return slot, w

    @staticmethod
    def reverse(ctx, gH, gA, gg, gl, gu, ninputs, rate=None):
        """The gradients of (Ad, Bd, c, x0, xref, uref, Q, R, Qf) -- inputs 1 .. 9 of ``forward`` -- that ``needs_input_grad``
        names, in a list of ``ninputs`` entries (the others None).  ``rate`` (``LTVRateFunction``): the keyword arguments of
        ``mpc.condense_ltv_adjoint_rate_device`` beside the cotangents above, and ``want``, which of "S", "uprev" to compute
        as well; those two come back in ``rate["out"]``."""
        Ad, Bd, c, x0, xref, uref, Qd, Rd, Qfd = ctx.saved_tensors[:9]
        names = ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R", "Qf")
        want = tuple(k for k, nd in zip(names, ctx.needs_input_grad[1:10]) if nd)
        staged = Qfd is None
        if staged and "Qf" in want:                                      # (a shared Q beside a staged R: Qf is stage N-1 of Q)
            want = tuple(k for k in want if k not in ("Q", "Qf")) + ("Q",)
        grads = [None] * ninputs
        extra = () if rate is None else tuple(rate["want"])
        if want or extra:
            slot, w = LTVCondenseFunction.restore(ctx)
            if rate is None:
                out = mpc.condense_ltv_adjoint_device(Ad, Bd, x0, w, slot["ws"], slot["adj"], xref=xref, uref=uref, dH=gH, dA=gA,
                                                      dg=gg, dl=gl, du=gu, want=want)
            else:
                out = mpc.condense_ltv_adjoint_rate_device(Ad, Bd, x0, w, slot["ws"], ctx.condenser.rate_adjoint_workspace(slot),
                                                           xref=xref, uref=uref, dH=gH, dA=gA, dg=gg, dl=gl, du=gu,
                                                           want=want + extra, **{k: v for k, v in rate.items() if k != "want"})
                rate["out"] = {k: out.pop(k) for k in extra}
            if staged:                                                   # [B, N, ., .] back to the shape the weight was given in
                N = Ad.shape[1]
                if "Q" in out and ctx.wdims[0] == 2:
                    out["Qf"] = out["Q"][:, N - 1].sum(0)
                    out["Q"] = out["Q"][:, :N - 1].sum((0, 1))
                for k, dim in zip(("Q", "R"), ctx.wdims):
                    if k in out and dim == 3:
                        out[k] = out[k].sum(0)
                    elif k in out and dim == 2 and k == "R":
                        out[k] = out[k].sum((0, 1))
                out = {k: t for k, t in out.items() if ctx.needs_input_grad[1 + names.index(k)]}
            qdt = dict(Q=ctx.meta[0], R=ctx.meta[1], Qf=ctx.meta[2])
            for i, k in enumerate(names):
                if k in out:
                    grads[1 + i] = out[k].to(qdt[k]) if k in qdt else out[k]
        return grads

    @staticmethod
    def backward(ctx, gH, gA, gg, gl, gu):
        need = ctx.needs_input_grad
        grads = LTVCondenseFunction.reverse(ctx, gH, gA, gg, gl, gu, 12)
        for i, gb, dim, dt in ((10, gl, ctx.meta[3], ctx.meta[5]), (11, gu, ctx.meta[4], ctx.meta[6])):
            if need[i] and gb is not None:
                grads[i] = (gb if dim == 2 else gb.sum(0)).to(dt)
        return tuple(grads)


class StageConstraintFunction(torch.autograd.Function):
    """``StageConstraintFunction.apply(condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, E, lo, hi)`` -> ``(H, A_c, g, l_c, u_c)``:
    the condensed QPs of a batch of LTV plants under stage constraints lo_k <= E_k [u_k ; x_{k+1}] <= hi_k (E [B, N, nc, nu + nx]
    or shared [N, nc, nu + nx]; lo, hi [B, N nc] or [N nc]).  Forward: ``LTVCondenseFunction``'s condensing (H, g), then C-ABI
    rqp_ltv_stage_rows + rqp_ltv_stage_vectors on its workspace.  Backward: rqp_ltv_stage_adjoint turns the cotangents of (A_c,
    l_c, u_c) into dE and into the (dA, dl) that ``LTVCondenseFunction``'s reverse maps on to the plant; it shares that class's
    workspace stamp, so a backward whose workspace a later forward has overwritten condenses its stages again first.  The
    gradients of a shared E and of shared bounds are summed over the batch."""

    @staticmethod
    def forward(ctx, condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, E, lo, hi):
        cd = condenser
        dtype, device, B = Ad.dtype, Ad.device, Ad.shape[0]
        slot = cd.slot(B, device, dtype)
        w, (Qd, Rd, Qfd) = _ltv_layer_weights(cd, slot, B, device, Q, R, Qf)
        det = lambda t: None if t is None else t.detach().contiguous()
        Ad, Bd, c, x0, xref, uref = (det(t) for t in (Ad, Bd, c, x0, xref, uref))
        Ed = E.detach().to(device=device, dtype=dtype).contiguous()
        slot["stamp"] = ctx.stamp = cd.next_stamp()
        _, As = cd.recondense_outputs(slot, B, device, dtype)            # (A = F of the box is not an output here)
        H, _ = mpc.condense_ltv_device(Ad, Bd, w, slot["ws"], c=c, A=As)
        if "box0" not in slot:
            slot["box0"] = torch.zeros(cd.m, dtype=dtype, device=device)
        g, _, _ = mpc.ltv_vectors_device((cd.nx, cd.nu, cd.horizon, cd.K is not None, c is not None), x0, slot["box0"],
                                         slot["box0"], w, slot["ws"], xref=xref, uref=uref)
        dims4 = (B, cd.nx, cd.nu, cd.horizon)
        A_c = mpc.stage_rows_device(dims4, Ed, slot["ws"])
        l_c, u_c = mpc.stage_vectors_device(dims4, Ed, x0, lo.detach(), hi.detach(), slot["ws"])
        ctx.condenser, ctx.slot, ctx.dims4 = cd, slot, dims4
        ctx.meta = (Q.dtype, R.dtype, None if Qf is None else Qf.dtype, E.dim(), lo.dim(), hi.dim(), E.dtype, lo.dtype, hi.dtype)
        ctx.wdims = (Q.dim(), R.dim())
        ctx.save_for_backward(Ad, Bd, c, x0, xref, uref, Qd, Rd, Qfd, Ed)
        ctx.set_materialize_grads(False)
        return H, A_c, g, l_c, u_c

    @staticmethod
    def backward(ctx, gH, gA, gg, gl, gu):
        need = ctx.needs_input_grad
        x0, Ed = ctx.saved_tensors[3], ctx.saved_tensors[9]
        plant = any(need[1:10])
        dA_full = dl_full = dE = None
        if (gA is not None or gl is not None or gu is not None) and (plant or need[10]):
            slot, _ = LTVCondenseFunction.restore(ctx)
            want = (("dA_full", "dl_full") if plant else ()) + (("dE",) if need[10] else ())
            out = mpc.stage_adjoint_device(ctx.dims4, Ed, x0, slot["ws"], dA_c=gA, dl_c=gl, du_c=gu, want=want)
            dA_full, dl_full, dE = out.get("dA_full"), out.get("dl_full"), out.get("dE")
        grads = LTVCondenseFunction.reverse(ctx, gH, dA_full, gg, dl_full, None, 13)
        if dE is not None:
            grads[10] = (dE if ctx.meta[3] == 4 else dE.sum(0)).to(ctx.meta[6])
        for i, gb, dim, dt in ((11, gl, ctx.meta[4], ctx.meta[7]), (12, gu, ctx.meta[5], ctx.meta[8])):
            if need[i] and gb is not None:
                grads[i] = (gb if dim == 2 else gb.sum(0)).to(dt)
        return tuple(grads)


class LTVRateFunction(torch.autograd.Function):
    """``LTVRateFunction.apply(condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, b0, b1, b2, S, u_prev, du_lo, du_hi)`` ->
    ``(H, A, g, l, u)``: the condensed QPs with input rates (DESIGN.md section 5 "LTV condensing, input rates").  The base rows
    are the box (b0 = None, b1, b2 = l_add, u_add) or stage rows (b0, b1, b2 = E, lo, hi).  S [nu, nu], [N, nu, nu] or
    [B, N, nu, nu] is the rate weight (None: no rate cost, S = 0 on the same kernels), u_prev [B, nu] the input applied before
    stage 0; du_lo, du_hi [N nu] or [B, N nu] (both or neither) append the N nu slew-rate rows after the base rows, as
    ``mpc.BatchedLTVMPC`` places them.  Forward: C-ABI rqp_ltv_condense_rate + rqp_ltv_vectors_rate (+ rqp_ltv_stage_rows /
    rqp_ltv_stage_vectors, rqp_ltv_rate_rows / rqp_ltv_rate_bounds).  Backward: rqp_ltv_condense_adjoint_rate (after
    rqp_ltv_stage_adjoint for stage rows), which reads the tails of the cotangents of (A, l, u) in place; it shares
    ``LTVCondenseFunction``'s workspace stamp (only F and [G | f] of the workspace are read, so a re-condense needs no S).
    Gradients of S, du_lo, du_hi come back in the input's shape, summed where the input is shared."""

    @staticmethod
    def forward(ctx, condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, b0, b1, b2, S, u_prev, du_lo, du_hi):
        cd = condenser
        dtype, device, B = Ad.dtype, Ad.device, Ad.shape[0]
        nx, nu, N, n = cd.nx, cd.nu, cd.horizon, cd.n
        slot = cd.slot(B, device, dtype)
        w, (Qd, Rd, Qfd) = _ltv_layer_weights(cd, slot, B, device, Q, R, Qf)
        det = lambda t: None if t is None else t.detach().contiguous()
        Ad, Bd, c, x0, xref, uref = (det(t) for t in (Ad, Bd, c, x0, xref, uref))
        stage, rows = b0 is not None, du_lo is not None
        Ed = b0.detach().to(device=device, dtype=dtype).contiguous() if stage else None
        Sd = mpc.rate_weight_device(torch.zeros(nu, nu, dtype=torch.float64, device=device) if S is None else S, nu, N, B, device)
        up = u_prev.detach().to(device=device, dtype=dtype).contiguous()
        slot["stamp"] = ctx.stamp = cd.next_stamp()
        dims4, dims5 = (B, nx, nu, N), (nx, nu, N, cd.K is not None, c is not None)
        m0 = N * Ed.shape[-2] if stage else cd.m
        if stage:
            _, As = cd.recondense_outputs(slot, B, device, dtype)        # (A = F of the box is not an output here)
            H, _ = mpc.condense_ltv_device(Ad, Bd, w, slot["ws"], c=c, A=As, S=Sd)
            if "box0" not in slot:
                slot["box0"] = torch.zeros(cd.m, dtype=dtype, device=device)
            g, _, _ = mpc.ltv_vectors_device(dims5, x0, slot["box0"], slot["box0"], w, slot["ws"], xref=xref, uref=uref, S=Sd, uprev=up)
            A0 = mpc.stage_rows_device(dims4, Ed, slot["ws"])
            l0, u0 = mpc.stage_vectors_device(dims4, Ed, x0, b1.detach(), b2.detach(), slot["ws"])
        else:
            H, A0 = mpc.condense_ltv_device(Ad, Bd, w, slot["ws"], c=c, S=Sd)
            g, l0, u0 = mpc.ltv_vectors_device(dims5, x0, b1.detach(), b2.detach(), w, slot["ws"], xref=xref, uref=uref, S=Sd, uprev=up)
        if rows:
            A = torch.empty((B, m0 + n, n), dtype=dtype, device=device)
            l, u = torch.empty((B, m0 + n), dtype=dtype, device=device), torch.empty((B, m0 + n), dtype=dtype, device=device)
            A[:, :m0].copy_(A0)
            l[:, :m0].copy_(l0)
            u[:, :m0].copy_(u0)
            mpc.rate_rows_device(dims4, slot["ws"], dtype, A_r=A, row0=m0)
            mpc.rate_bounds_device(dims4, x0, up, du_lo.detach(), du_hi.detach(), slot["ws"], l_r=l, u_r=u, row0=m0)
        else:
            A, l, u = A0, l0, u0
        ctx.condenser, ctx.slot, ctx.dims4, ctx.m0, ctx.stage, ctx.rows = cd, slot, dims4, m0, stage, rows
        ctx.meta = (Q.dtype, R.dtype, None if Qf is None else Qf.dtype)
        ctx.wdims = (Q.dim(), R.dim())
        ctx.like = [None if t is None else (t.dim(), t.dtype) for t in (b0, b1, b2, S, u_prev, du_lo, du_hi)]
        ctx.save_for_backward(Ad, Bd, c, x0, xref, uref, Qd, Rd, Qfd, Ed, Sd, up)
        ctx.set_materialize_grads(False)
        return H, A, g, l, u

    @staticmethod
    def backward(ctx, gH, gA, gg, gl, gu):
        need, m0, like = ctx.needs_input_grad, ctx.m0, ctx.like
        x0, Ed, Sd, up = ctx.saved_tensors[3], ctx.saved_tensors[9], ctx.saved_tensors[10], ctx.saved_tensors[11]
        con = lambda t: None if t is None else t.contiguous()
        gA, gl, gu = con(gA), con(gl), con(gu)
        head = lambda t: t if (t is None or not ctx.rows) else t[:, :m0].contiguous()
        dA, dl, du = head(gA), head(gl), head(gu)
        plant = any(need[1:10])
        dE = None
        if ctx.stage:
            dA_c, dl_c, du_c = dA, dl, du
            dA = dl = du = None
            if (dA_c is not None or dl_c is not None or du_c is not None) and (plant or need[10]):
                slot, _ = LTVCondenseFunction.restore(ctx)
                want = (("dA_full", "dl_full") if plant else ()) + (("dE",) if need[10] else ())
                out = mpc.stage_adjoint_device(ctx.dims4, Ed, x0, slot["ws"], dA_c=dA_c, dl_c=dl_c, du_c=du_c, want=want)
                dA, dl, dE = out.get("dA_full"), out.get("dl_full"), out.get("dE")
        else:
            dl_c, du_c = dl, du
        rows = ctx.rows
        rate = dict(S=Sd, uprev=up, row0=m0 if rows else 0, dA_r=gA if rows else None, dl_r=gl if rows else None,
                    du_r=gu if rows else None, want=(("S",) if need[13] else ()) + (("uprev",) if need[14] else ()))
        grads = LTVCondenseFunction.reverse(ctx, gH, dA, gg, dl, du, 17, rate=rate)
        out = rate.get("out", {})
        if dE is not None:
            grads[10] = (dE if like[0][0] == 4 else dE.sum(0)).to(like[0][1])
        for i, gb in ((11, dl_c), (12, du_c)):                           # the base bounds: l_add, u_add or lo, hi
            if need[i] and gb is not None:
                grads[i] = (gb if like[i - 10][0] == 2 else gb.sum(0)).to(like[i - 10][1])
        if "S" in out:                                                   # [B, N, nu, nu] back to the shape S was given in
            dS = out["S"]
            dS = dS if like[3][0] == 4 else (dS.sum(0) if like[3][0] == 3 else dS.sum((0, 1)))
            grads[13] = dS.to(like[3][1])
        if "uprev" in out:
            grads[14] = out["uprev"].to(like[4][1])
        for i, gb in ((15, gl), (16, gu)):
            if rows and need[i] and gb is not None:
                tail = gb[:, m0:]
                grads[i] = (tail if like[i - 10][0] == 2 else tail.sum(0)).to(like[i - 10][1])
        return tuple(grads)


class LTVMPCLayer(torch.nn.Module):
    """Differentiable MPC on a batch of LTV plants: ``u0, v = LTVMPCLayer(nx, nu, horizon, u_max, x_max, K=None)(Ad, Bd, x0, Q, R,
    Qf, c=None, xref=None, uref=None)``.  The stages are condensed on the device (``LTVCondenseFunction``), the QPs solved by a
    ``ReLUQPLayer`` on per-instance matrices (``setup_kwargs`` are its keyword arguments; its defaults ``differentiable=True,
    polish=True``), and the first input is u0 = v[:, :nu] - x0 K' [B, nu]; v [B, n] is the whole QP solution.  Gradients flow to
    Ad, Bd, c, x0, xref, uref and to the weights Q, R, Qf (shared by the batch: summed over it).  The box |u| <= u_max,
    |x| <= x_max and the gain K are constants of the layer.

    Stage weights: Q may be [N, nx, nx] or [B, N, nx, nx] (Q_k weighs x_{k+1}, Q[..., N-1, :, :] is the terminal weight; pass
    ``Qf=None``) and R [N, nu, nu] or [B, N, nu, nu]; one of them may stay a shared matrix.  Their gradients have the input's
    shape: per instance and stage for [B, N, ., .], summed over the batch for [N, ., .].

    ``LTVMPCLayer(nx, nu, horizon, K=None, stage_rows=nc)`` (no u_max, x_max) replaces the box by nc rows per stage, lo_k <=
    E_k [u_k ; x_{k+1}] <= hi_k, given with every call: ``layer(Ad, Bd, x0, Q, R, Qf, ..., E=, lo=, hi=)`` with E [B, N, nc,
    nu + nx] or shared [N, nc, nu + nx] and lo, hi [B, N nc] or [N nc] (``StageConstraintFunction``).  Gradients then also flow
    to E, lo and hi (summed over the batch where the input is shared).

    Input rates (``LTVRateFunction``; both act on the plant's input u_k = -K x_k + v_k): ``layer(..., S=, u_prev=)`` adds the
    move-suppression cost 1/2 sum_k (u_k - u_{k-1})' S_k (u_k - u_{k-1}), u_{-1} = u_prev [B, nu], with S [nu, nu], [N, nu, nu]
    or [B, N, nu, nu] (symmetric blocks); ``LTVMPCLayer(..., rate_rows=True)`` appends the N nu rows du_lo_k <= u_k - u_{k-1} <=
    du_hi_k after the box or the stage rows, their bounds given with every call: ``layer(..., u_prev=, du_lo=, du_hi=)``, [N nu]
    or [B, N nu].  The cost alone, the rows alone, or both.  Gradients then also flow to S, u_prev, du_lo and du_hi, in the
    input's shape (summed over the batch, and for S [nu, nu] over the stages, where the input is shared).  Without any rate
    argument the layer makes the calls it made before."""

    def __init__(self, nx, nu, horizon, u_max=None, x_max=None, K=None, stage_rows=None, rate_rows=False, **setup_kwargs):
        super().__init__()
        self.condenser = mpc.LTVCondenser(nx, nu, horizon, K=K)
        self.nx, self.nu, self.horizon = self.condenser.nx, self.condenser.nu, self.condenser.horizon
        self.stage_rows = None if stage_rows is None else int(stage_rows)
        if self.stage_rows is not None:
            if u_max is not None or x_max is not None:
                raise ValueError("stage_rows replaces the box: u_max and x_max must be None (write the box as rows of E)")
            mpc._stage_check_sizes(self.horizon, self.stage_rows)
            self.l_add = self.u_add = None
        else:
            if u_max is None or x_max is None:
                raise ValueError("u_max and x_max are required without stage_rows")
            _, self.l_add, self.u_add = mpc.box_constraints(self.nx, self.nu, self.horizon, u_max, x_max)
        self.rate_rows = bool(rate_rows)
        m0 = self.horizon * (self.stage_rows if self.stage_rows is not None else self.nx + self.nu)
        if self.rate_rows and m0 + self.horizon * self.nu > mpc.LTV_LIMITS["m"]:
            raise ValueError("unsupported size: %d base rows + %d rate rows, the QPs hold m <= %d"
                             % (m0, self.horizon * self.nu, mpc.LTV_LIMITS["m"]))
        self.qp = ReLUQPLayer(**setup_kwargs)
        self._const = {}

    def _check_stage(self, B, dtype, device, E, lo, hi):
        nc, N, blk = self.stage_rows, self.horizon, self.nx + self.nu
        if nc is None:
            if E is not None or lo is not None or hi is not None:
                raise ValueError("E, lo, hi need LTVMPCLayer(stage_rows=nc)")
            return
        for name, t in (("E", E), ("lo", lo), ("hi", hi)):
            if not torch.is_tensor(t):
                raise ValueError("stage_rows: %s must be given as a torch tensor" % name)
        if tuple(E.shape) not in ((B, N, nc, blk), (N, nc, blk)):
            raise ValueError("E has shape %s, expected %s or %s" % (tuple(E.shape), (B, N, nc, blk), (N, nc, blk)))
        for name, t in (("lo", lo), ("hi", hi)):
            if tuple(t.shape) not in ((B, N * nc), (N * nc,)):
                raise ValueError("%s has shape %s, expected %s or %s" % (name, tuple(t.shape), (B, N * nc), (N * nc,)))
        if lo.dim() != hi.dim():
            raise ValueError("lo and hi must both be [B, N nc] or both [N nc]")
        if any(t.dtype != dtype for t in (E, lo, hi)):
            raise ValueError("E, lo, hi must have the precision of Ad")
        if any(t.device != device for t in (E, lo, hi)):
            raise ValueError("E, lo, hi must be on the device of Ad (%s)" % device)

    def _check_rate(self, B, dtype, device, S, u_prev, du_lo, du_hi):
        """True when the call has rate terms.  (The symmetry of S is tested in ``_check``, in the read-back it makes for Q, R, Qf.)"""
        nu, N = self.nu, self.horizon
        if not self.rate_rows and (du_lo is not None or du_hi is not None):
            raise ValueError("du_lo, du_hi need LTVMPCLayer(rate_rows=True)")
        if self.rate_rows and (du_lo is None or du_hi is None):
            raise ValueError("rate_rows: du_lo and du_hi must be given")
        if S is None and not self.rate_rows:
            if u_prev is not None:
                raise ValueError("u_prev needs S or LTVMPCLayer(rate_rows=True)")
            return False
        if u_prev is None:
            raise ValueError("input rates need u_prev [B, nu], the input applied before stage 0")
        for name, t in (("S", S), ("u_prev", u_prev), ("du_lo", du_lo), ("du_hi", du_hi)):
            if t is not None and not torch.is_tensor(t):
                raise ValueError("%s must be given as a torch tensor" % name)
        if S is not None:
            mpc._rate_weight_shapes(nu, N, S, B=B)
        if tuple(u_prev.shape) != (B, nu):
            raise ValueError("u_prev has shape %s, expected %s" % (tuple(u_prev.shape), (B, nu)))
        if self.rate_rows:
            for name, t in (("du_lo", du_lo), ("du_hi", du_hi)):
                if tuple(t.shape) not in ((B, N * nu), (N * nu,)):
                    raise ValueError("%s has shape %s, expected %s or %s" % (name, tuple(t.shape), (B, N * nu), (N * nu,)))
            if du_lo.dim() != du_hi.dim():
                raise ValueError("du_lo and du_hi must both be [B, N nu] or both [N nu]")
        if any(t is not None and t.dtype != dtype for t in (u_prev, du_lo, du_hi)):
            raise ValueError("u_prev, du_lo, du_hi must have the precision of Ad")
        if any(t is not None and t.device != device for t in (S, u_prev, du_lo, du_hi)):
            raise ValueError("S, u_prev, du_lo, du_hi must be on the device of Ad (%s)" % device)
        return True

    def _check(self, Ad, Bd, x0, Q, R, Qf, c, xref, uref, stage=(None, None, None), rate=(None, None, None, None)):
        nx, nu, N = self.nx, self.nu, self.horizon
        staged = torch.is_tensor(Q) and torch.is_tensor(R) and (Q.dim() > 2 or R.dim() > 2)
        for name, t in (("Ad", Ad), ("Bd", Bd), ("x0", x0), ("Q", Q), ("R", R)) + (() if staged and Qf is None else (("Qf", Qf),)):
            if not torch.is_tensor(t):
                raise ValueError("%s must be a torch tensor" % name)
        B, Ns, nxs, nus = mpc._ltv_shapes(Ad, Bd)
        if (Ns, nxs, nus) != (N, nx, nu):
            raise ValueError("stages of shape (N=%d, nx=%d, nu=%d), expected (%d, %d, %d)" % (Ns, nxs, nus, N, nx, nu))
        for name, t, shape in (("x0", x0, (B, nx)), ("c", c, (B, N, nx)), ("xref", xref, (B, N, nx)), ("uref", uref, (B, N, nu))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), shape))
        if staged:                                                       # [N, ., .] or [B, N, ., .]; a staged Q has no Qf
            mpc._ltv_stage_shapes(nx, nu, N, Q, R, Qf, B=B)
        elif tuple(Q.shape) != (nx, nx) or tuple(Qf.shape) != (nx, nx) or tuple(R.shape) != (nu, nu):
            raise ValueError("Q, Qf must be [%d, %d] and R [%d, %d]" % (nx, nx, nu, nu))
        # symmetric up to rounding, as BatchedLTVMPC asks (the symmetric part is what is used); the three tests share one read-back
        # (a rate weight S on the device of Q joins them: no read-back of its own)
        sym = [(name, W) for name, W in (("Q", Q), ("R", R), ("Qf", Qf)) if W is not None]
        if torch.is_tensor(rate[0]) and rate[0].dim() >= 2 and rate[0].device == Q.device:
            sym.append(("S", rate[0]))
        asym = torch.stack([((W.detach() - W.detach().transpose(-1, -2)).abs().max() - 1e-9 * W.detach().abs().max()).double()
                            for _, W in sym]).tolist()
        for (name, _), a in zip(sym, asym):
            if a > 0:
                raise ValueError("%s must be symmetric" % name)
        if Ad.dtype not in (torch.float32, torch.float64) or any(t is not None and t.dtype != Ad.dtype for t in (Bd, x0, c, xref, uref)):
            raise ValueError("Ad, Bd, x0 (c, xref, uref) must share one precision, float32 or float64")
        self._check_stage(B, Ad.dtype, Ad.device, *stage)
        has_rate = self._check_rate(B, Ad.dtype, Ad.device, *rate)
        if Ad.device.type != "cuda":
            raise _cabi.RqpUnavailable("LTVMPCLayer needs a HIP device; the MI355X build has no CPU path")
        return B, has_rate

    def forward(self, Ad, Bd, x0, Q, R, Qf, c=None, xref=None, uref=None, E=None, lo=None, hi=None, S=None, u_prev=None, du_lo=None,
                du_hi=None):
        B, has_rate = self._check(Ad, Bd, x0, Q, R, Qf, c, xref, uref, stage=(E, lo, hi), rate=(S, u_prev, du_lo, du_hi))
        key = (str(Ad.device), Ad.dtype)
        if key not in self._const:
            t = lambda a: None if a is None else torch.as_tensor(a, dtype=Ad.dtype, device=Ad.device)
            self._const[key] = (t(self.l_add), t(self.u_add), t(self.condenser.K))
        l_add, u_add, K = self._const[key]
        if has_rate:
            base = (None, l_add, u_add) if self.stage_rows is None else (E, lo, hi)
            H, A, g, l, u = LTVRateFunction.apply(self.condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, *base, S, u_prev, du_lo, du_hi)
        elif self.stage_rows is None:
            H, A, g, l, u = LTVCondenseFunction.apply(self.condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, l_add, u_add)
        else:
            H, A, g, l, u = StageConstraintFunction.apply(self.condenser, Ad, Bd, c, x0, xref, uref, Q, R, Qf, E, lo, hi)
        out = self.qp(H, g, A, l, u)
        v = out[0]
        u0 = v[:, :self.nu] if K is None else v[:, :self.nu] - x0 @ K.transpose(0, 1)
        return u0, v
