"""numpy restatement of the solution polishing of include/rqp_abi.h (rqp_set_polish), used by tests/test_polish_*.py.

    active set   lower: z - l < -lam;  upper (not lower): u - z < lam;  inactive otherwise
    reduced KKT  [[H + delta I, A_a'], [A_a, -delta I]] [x; y_a] = [-g; b_a],  b_a = l (lower) / u (upper),
                 then `refine` steps of iterative refinement against [[H, A_a'], [A_a, 0]]
    point        z = clip(A x, l, u);  y = y_a on the active rows, 0 elsewhere, projected onto the sign cone
                 (<= 0 lower, >= 0 upper, free where l == u)
    acceptance   both residuals below the ADMM ones, or one below and the other ADMM residual < 1e-10 (OSQP)
"""
import numpy as np


def classify(z, lam, l, u):
    """-1 lower-active, +1 upper-active, 0 inactive (per row; any leading batch dimensions)."""
    lower = (z - l) < -lam
    upper = ~lower & ((u - z) < lam)
    return np.where(lower, -1, np.where(upper, 1, 0)).astype(np.int8)


def _rhs_b(l, u, act):
    return np.where(act < 0, l, np.where(act > 0, u, 0.0))


def point(H, g, A, l, u, act, x, y):
    """(x, z, y) of the polished point from a solution (x, y) of the reduced system (y over all rows, 0 where inactive)."""
    z = np.clip(A @ x, l, u)
    y = np.where(act != 0, y, 0.0)
    free = l == u
    y = np.where((act < 0) & ~free, np.minimum(y, 0.0), y)
    y = np.where((act > 0) & ~free, np.maximum(y, 0.0), y)
    return x, z, y


def kkt_exact(H, g, A, l, u, act):
    """Exact solution of [[H, A_a'], [A_a, 0]] [x; y_a] = [-g; b_a] (float64, dense), as the polished point."""
    n = H.shape[0]
    idx = np.nonzero(act)[0]
    Aa = A[idx]
    K = np.zeros((n + len(idx), n + len(idx)))
    K[:n, :n] = 0.5 * (H + H.T)
    K[:n, n:] = Aa.T
    K[n:, :n] = Aa
    rhs = np.concatenate([-g, _rhs_b(l, u, act)[idx]])
    sol = np.linalg.solve(K, rhs)
    y = np.zeros(A.shape[0])
    y[idx] = sol[n:]
    return point(H, g, A, l, u, act, sol[:n], y)


def polish(H, g, A, l, u, act, delta=1e-6, refine=3):
    """The library's algorithm: regularised solve through the reduced n x n system, then `refine` refinement steps."""
    n = H.shape[0]
    Hs = 0.5 * (H + H.T)
    w = (act != 0).astype(float)
    b = _rhs_b(l, u, act)
    M = Hs + delta * np.eye(n) + (A.T * w) @ A / delta
    Minv = np.linalg.inv(M)
    x = Minv @ (-g + A.T @ (w * b) / delta)
    y = w * (A @ x - b) / delta
    for _ in range(refine):
        r1 = -g - Hs @ x - A.T @ y
        r2 = w * (b - A @ x)
        dx = Minv @ (r1 + A.T @ r2 / delta)
        y = y + w * (A @ dx - r2) / delta
        x = x + dx
    return point(H, g, A, l, u, act, x, y)


def residuals(H, g, A, x, z, y):
    """(pri, dua, obj) of a point, inf-norms (no scaling)."""
    Hs = 0.5 * (H + H.T)
    return (np.abs(A @ x - z).max(), np.abs(Hs @ x + A.T @ y + g).max(), 0.5 * x @ Hs @ x + g @ x)


def accept(pri, dua, pri_admm, dua_admm):
    return (pri < pri_admm and dua < dua_admm) or (pri < pri_admm and dua_admm < 1e-10) or (dua < dua_admm and pri_admm < 1e-10)
