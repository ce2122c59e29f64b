"""numpy restatement of the forward sensitivities of a QP solution (include/rqp_abi.h rqp_sensitivity, DESIGN.md section 5
"Forward sensitivities"), on top of tests/adjoint_ref.py.

    min 1/2 x'Hx + g'x  s.t.  l <= A x <= u;   at the solution sym(H) x + g + A'y = 0, active rows a (adjoint's convention).
    [[sym(H), A_a'], [A_a, 0]] [dx; dy_a] = [-(sym(dH) x + dg + dA' ybar);  db_a - dA_a x],   dy = 0 off a,
    dz = A dx + dA x,   db = dl on lower-active rows, du on upper-active rows.
"""
import numpy as np

import adjoint_ref as R


def jvp(H, A, x, y, act, dH=None, dg=None, dA=None, dl=None, du=None):
    """Tangents (dx, dy, dz) of one instance along one direction (float64; None tangents are zero)."""
    H, A, x, y = (np.asarray(t, dtype=np.float64) for t in (H, A, x, y))
    act = np.asarray(act)
    n, m = x.shape[0], y.shape[0]
    z = lambda t, shape: np.zeros(shape) if t is None else np.asarray(t, dtype=np.float64)
    dH, dg, dA, dl, du = z(dH, (n, n)), z(dg, n), z(dA, (m, n)), z(dl, m), z(du, m)
    ybar = np.where(act != 0, y, 0.0)
    r1 = -(0.5 * (dH + dH.T) @ x + dg + dA.T @ ybar)
    db = np.where(act < 0, dl, np.where(act > 0, du, 0.0))
    dx, dy = R.kkt_solve(H, A, act != 0, r1, db - dA @ x)
    return dx, dy, A @ dx + dA @ x


def jvp_batch(H, A, x, y, act, ndir, **tangents):
    """dx [B, n, ndir], dy / dz [B, m, ndir].  H, A [B, ...] or shared; each tangent has the direction axis last, with a batch
    axis ([B, ..., ndir]) or without one (shared)."""
    B = x.shape[0]
    shared = H.ndim == 2
    full = dict(dH=3, dg=2, dA=3, dl=2, du=2)
    out = [np.zeros((B, x.shape[1], ndir)), np.zeros((B, y.shape[1], ndir)), np.zeros((B, y.shape[1], ndir))]
    for b in range(B):
        for j in range(ndir):
            tj = {}
            for k, t in tangents.items():
                if t is None:
                    continue
                t = np.asarray(t)
                tj[k] = (t[b] if t.ndim == full[k] + 1 else t)[..., j]
            res = jvp(H if shared else H[b], A if shared else A[b], x[b], y[b], act[b], **tj)
            for o, r in zip(out, res):
                o[b, :, j] = r
    return tuple(out)
