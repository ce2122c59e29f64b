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

from reluqp import _cabi
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
