"""End-to-end fixture of the differentiable LTV MPC tests (tests/test_ltv_adjoint_*.py): a batch of LTV MPC problems whose
solutions have active sets with clear margins, and the numpy chain  condense_ltv_vjp o adjoint_ref.adjoint  the device
gradients are compared with.  Everything is a pure function of (nx, nu, N): the CPU test checks the margins, the GPU test
uses the same problems and excludes no instance."""
import numpy as np

from reluqp import mpc

import adjoint_ref as R

B = 16
SHAPES = ((6, 2, 8), (12, 4, 20))
U_MAX, X_MAX = 0.4, 8.0
# scale of each instance's (standard normal) initial state, fixed so that on every instance the solution's active set is small
# (<= n / 2 rows, empty on every fourth instance) and has margins >= 3e-3; tests/test_ltv_adjoint_cpu.py checks MARGIN for all
X0_SCALE = {(6, 2, 8): (0.1, 0.1, 0.1, 0.04, 0.1, 0.16, 0.1, 0.04, 0.26, 0.1, 0.12, 0.04, 0.1, 0.1, 0.14, 0.04),
            (12, 4, 20): (0.16, 0.12, 0.1, 0.04, 0.1, 0.12, 0.14, 0.04, 0.14, 0.1, 0.1, 0.04, 0.1, 0.1, 0.1, 0.04)}
SEED = {(6, 2, 8): 3, (12, 4, 20): 5}
MARGIN = 1e-3


def problem(nx, nu, N, step=0):
    """Inputs of the layer (numpy float64): Ad, Bd, c, x0, xref, uref [B, ...], Q, R, Qf, K.  ``step`` > 0 draws another
    linearisation and state of the same plant (the unrolled-loop test)."""
    seed = SEED[(nx, nu, N)]
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)
    rs = np.random.RandomState(100 * seed + step)
    Ad = Ad0[None, None] + 0.02 * rs.randn(B, N, nx, nx) / np.sqrt(nx)
    Bd = Bd0[None, None] + 0.02 * rs.randn(B, N, nx, nu)
    c = 0.01 * rs.randn(B, N, nx)
    x0 = np.asarray(X0_SCALE[(nx, nu, N)], dtype=np.float64).reshape(-1, 1) * rs.randn(B, nx)
    xref, uref = 0.05 * rs.randn(B, N, nx), 0.02 * rs.randn(B, N, nu)

    def spd(k, w):
        M = rs.randn(k, k)
        return w * (np.eye(k) + 0.1 * (M @ M.T) / k)

    Q, R_ = spd(nx, 1.0), spd(nu, 0.1)
    K, P = mpc.ihlqr(Ad0, Bd0, Q, R_, Q)
    Qf = 0.5 * (P + P.T)
    return dict(Ad=Ad, Bd=Bd, c=c, x0=x0, xref=xref, uref=uref, Q=Q, R=R_, Qf=Qf, K=K)


def condensed(p):
    """(H, A, g, l, u) of the batch on the host."""
    N, nx, nu = p["Ad"].shape[1], p["Ad"].shape[2], p["Bd"].shape[3]
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, U_MAX, X_MAX)
    cond = mpc.condense_ltv(p["Ad"], p["Bd"], p["Q"], p["R"], p["Qf"], K=p["K"], c=p["c"])
    g, l, u = mpc.ltv_vectors(cond, p["x0"], l_add, u_add, xref=p["xref"], uref=p["uref"])
    return cond["H"], cond["A"], g, l, u


def classify(z, lam, l, u):
    """polish's rule (include/rqp_abi.h rqp_set_polish): lower-active z - l < -lam, upper-active u - z < lam."""
    act = np.zeros(z.shape, dtype=np.int8)
    lower = z - l < -lam
    act[lower] = -1
    act[~lower & (u - z < lam)] = 1
    return act


def margins(H, A, g, l, u, act):
    """Exact solution on the active set `act` and its margins: (x, y, distance of the inactive rows to their bounds,
    |multiplier| of the active rows with the sign the side asks for, else negative)."""
    x, y = R.exact_solve(H, g, A, l, u, act)
    ax = A @ x
    off = act == 0
    dist = np.minimum(ax - l, u - ax)[off].min() if off.any() else np.inf
    mult = (y * act)[~off].min() if (~off).any() else np.inf
    return x, y, dist, mult


def reference_gradients(p, x, y, act, w):
    """d(sum w . u0) / d(inputs) by the numpy chain at the solution (x, y) [B, ...] and active sets act: per-instance arrays for
    Ad, Bd, c, x0, xref, uref, batch sums for Q, R, Qf."""
    N, nx, nu = p["Ad"].shape[1], p["Ad"].shape[2], p["Bd"].shape[3]
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, U_MAX, X_MAX)
    H, A, _, _, _ = condensed(p)
    n = N * nu
    adj = []
    for b in range(B):
        dx = np.zeros(n)
        dx[:nu] = w[b]                                          # u0 = v[:nu] - K x0
        adj.append(R.adjoint(H[b], A[b], x[b], y[b], act[b], dx))
    st = lambda k: np.stack([a[k] for a in adj])
    out = mpc.condense_ltv_vjp(p["Ad"], p["Bd"], p["Q"], p["R"], p["Qf"], p["x0"], l_add, u_add, K=p["K"], c=p["c"],
                               xref=p["xref"], uref=p["uref"], dH=st("dH"), dA=st("dA"), dg=st("dg"), dl=st("dl"), du=st("du"))
    out["x0"] = out["x0"] - w @ p["K"]                          # the direct term of u0 = v0 - K x0
    return out
