"""numpy restatement of the adjoint of a QP solution (include/rqp_abi.h rqp_adjoint), and a generator of
QPs with a planted solution whose active set has clear margins (tests/test_adjoint_*.py).

    min 1/2 x'Hx + g'x  s.t.  l <= A x <= u;   at the solution sym(H) x + g + A'y = 0, active rows a on their bound b_a.
    [[sym(H), A_a'], [A_a, 0]] [rx; ry_a] = -[dx; dy_a]
    dg = rx;  dl = -ry (lower-active), du = -ry (upper-active);  dH = (rx x' + x rx') / 2;  dA = ybar rx' + ry x'
"""
import numpy as np


def kkt_solve(H, A, act, rhs_x, rhs_y):
    """Solve [[sym(H), A_a'], [A_a, 0]] [v; w_a] = [rhs_x; rhs_y_a] in float64 (w = 0 off the active set)."""
    n = H.shape[0]
    Hs = 0.5 * (H + H.T)
    idx = np.flatnonzero(act)
    Aa = A[idx]
    K = np.block([[Hs, Aa.T], [Aa, np.zeros((len(idx), len(idx)))]])
    sol = np.linalg.solve(K, np.concatenate([rhs_x, rhs_y[idx]]))
    w = np.zeros(A.shape[0])
    w[idx] = sol[n:]
    return sol[:n], w


def adjoint(H, A, x, y, act, dx, dy=None):
    """Gradients of one instance: dict dH, dg, dA, dl, du (float64)."""
    H, A, x, y = (np.asarray(t, dtype=np.float64) for t in (H, A, x, y))
    act = np.asarray(act)
    dy = np.zeros(A.shape[0]) if dy is None else np.asarray(dy, dtype=np.float64)
    rx, ry = kkt_solve(H, A, act != 0, -np.asarray(dx, dtype=np.float64), -dy)
    ybar = np.where(act != 0, y, 0.0)
    return dict(dg=rx, dl=np.where(act < 0, -ry, 0.0), du=np.where(act > 0, -ry, 0.0),
                dH=0.5 * (np.outer(rx, x) + np.outer(x, rx)), dA=np.outer(ybar, rx) + np.outer(ry, x))


def adjoint_batch(H, A, x, y, act, dx, dy=None):
    """Per-instance gradients of a batch; H, A [B, ...] or shared [n, n] / [m, n] (then dH, dA summed over the batch)."""
    B = x.shape[0]
    shared = H.ndim == 2
    outs = [adjoint(H if shared else H[b], A if shared else A[b], x[b], y[b], act[b], dx[b], None if dy is None else dy[b])
            for b in range(B)]
    res = {k: np.stack([o[k] for o in outs]) for k in outs[0]}
    if shared:
        res["dH"], res["dA"] = res["dH"].sum(0), res["dA"].sum(0)
    return res


def exact_solve(H, g, A, l, u, act):
    """Solution (x, y) of the QP whose active set is `act` (-1 lower, +1 upper, 0 inactive), from its KKT system."""
    b = np.where(act < 0, l, np.where(act > 0, u, 0.0))
    x, y = kkt_solve(H, A, act != 0, -np.asarray(g, dtype=np.float64), b)
    return x, y


def _matrices(rs, n, n_eq, n_ineq):
    # the draw pattern of reluqp.utils._draw: H = M'M + I symmetrised, then equality rows, then inequality rows
    M = rs.randn(n, n)
    H = M.T @ M + np.eye(n)
    H = H + H.T
    return H, np.vstack((rs.randn(n_eq, n), rs.randn(n_ineq, n)))


def margin_qp_batch(B, n, n_eq, n_ineq, seed, shared=False, n_active=None):
    """B QPs with a planted solution x, multipliers y and active set with margins: every active multiplier |y| in
    [0.5, 1.5], every inactive slack (on both sides) in [0.5, 1.5], at most n / 2 active rows: fewer than n, so the
    multipliers are unique, and far enough from n that the active rows are well conditioned (an active set of n - 1 random
    rows can be nearly dependent; the regularised solve with its few refinement steps then does not converge).
    Equality rows (l == u) are active with a random sign of y.  `n_active` (length B, default None: the random sets above,
    drawn exactly as without the keyword) gives the exact number of active inequality rows of each instance, 0 allowed and
    at most min(n // 2 - n_eq, n_ineq); with n_eq = 0 and n_active[b] = 0 instance b has an empty active set (y = 0 and
    l < A x < u).  Returns dict H, g, A, l, u, x, y, z, active (numpy;
    H [n, n] / A [m, n] when shared, else with a leading batch dimension)."""
    rs = np.random.RandomState(seed)
    m = n_eq + n_ineq
    assert n_eq <= n // 2
    Hs, As = _matrices(rs, n, n_eq, n_ineq) if shared else (None, None)
    out = {k: [] for k in ("H", "g", "A", "l", "u", "x", "y", "z", "active")}
    cap = n // 2 - n_eq                                            # active inequality rows allowed
    assert n_active is None or len(n_active) == B
    for b in range(B):
        H, A = (Hs, As) if shared else _matrices(rs, n, n_eq, n_ineq)
        if n_active is None:
            side = rs.choice([-1, 0, 1], size=n_ineq, p=[0.25, 0.5, 0.25])
            on = np.flatnonzero(side)
            if len(on) > cap:
                side[rs.permutation(on)[:len(on) - cap]] = 0
        else:
            k = int(n_active[b])
            assert 0 <= k <= min(cap, n_ineq), (k, cap, n_ineq)
            side = np.zeros(n_ineq, dtype=np.int64)
            side[rs.permutation(n_ineq)[:k]] = rs.choice([-1, 1], size=k)
        x = rs.randn(n)
        ax = A @ x
        mag = rs.uniform(0.5, 1.5, size=m)
        s_lo = rs.uniform(0.5, 1.5, size=m)
        s_up = rs.uniform(0.5, 1.5, size=m)
        act = np.concatenate([np.where(rs.randn(n_eq) > 0, 1, -1), side]).astype(np.int8)
        y = act * mag
        l = ax - s_lo
        u = ax + s_up
        l[act < 0] = ax[act < 0]
        u[act > 0] = ax[act > 0]
        l[:n_eq] = u[:n_eq] = ax[:n_eq]
        g = -H @ x - A.T @ y
        for k, v in (("H", H), ("g", g), ("A", A), ("l", l), ("u", u), ("x", x), ("y", y), ("z", ax), ("active", act)):
            out[k].append(v)
    res = {k: np.stack(v) for k, v in out.items()}
    if shared:
        res["H"], res["A"] = Hs, As
    return res
