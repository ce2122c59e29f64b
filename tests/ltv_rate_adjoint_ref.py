"""Helpers of the rate-adjoint tests (tests/test_ltv_rate_adjoint_*.py), beside tests/ltv_rate_fixture.py.

Kernel tests: ``abs_scale``, the formulas of ``mpc.condense_ltv_vjp`` with its rate keywords evaluated on the absolute values of
every term (one instance): the size of what each output sums, the `scale` of the rule of tests/test_ltv_gpu.py.

Layer tests: the problem of ``ltv_rate_fixture.driver_problem`` on the box (|u| <= U_MAX, |x| <= X_MAX) or on its stage rows, the
numpy QP of either, and the numpy chain  adjoint_ref.adjoint -> (stage_constraints_vjp ->) condense_ltv_vjp(S=, uprev=, dA_r=,
dl_r=, du_r=)  the layer's gradients are compared with.  The slew limit DU_MAX = 0.5 of the fixture is kept: the step from u_prev
(about 0.2) to the unconstrained u_0 (about U_MAX = 2) runs into it, with or without the half-planes, so every instance has an
active rate row at the optimum (tests/test_ltv_rate_adjoint_cpu.py computes the number with the oracle and checks it)."""
import numpy as np

from reluqp import mpc

import adjoint_ref as R
import ltv_rate_fixture as RF
import ltv_stage_fixture as SF

X_MAX = 50.0                                                   # the box variant: never active
GRAD_NAMES = ("Ad", "Bd", "x0", "S", "uprev", "dlo", "dhi")


def abs_scale(Ad, Bd, Q, R_, Qf, K, c, x0, xref, uref, S, uprev, bars):
    """{output: max|entry|} of the rate vjp's formulas on absolute values.  bars = (dH, dA, dg, dl, du, dA_r, dl_r, du_r); Q, R
    shared ([., .], with Qf) or per stage ([N, ., .], Qf None); S [N, nu, nu]."""
    N, nx, nu = Ad.shape[0], Ad.shape[1], Bd.shape[2]
    blk, n = nx + nu, N * nu
    cond = mpc.condense_ltv(Ad, Bd, Q, R_, Qf, K=K, c=c)
    F, G, f, H_sp = (np.abs(cond[k]) for k in ("F", "G", "f", "H_sp"))
    Hb, Ab, gb, lb, ub, Arb, lrb, urb = (np.abs(b) for b in bars)
    Kz = np.zeros((nu, nx)) if K is None else np.abs(K)
    yref = np.abs(np.hstack([np.zeros((N, nu)) if uref is None else uref, np.zeros((N, nx)) if xref is None else xref]).reshape(-1))
    x0 = np.abs(x0)
    s = G @ x0 + f
    e = s + yref
    Hs = (Hb + Hb.T) / 2
    T = F @ Hs
    D = np.abs(mpc._rate_difference(N, nx, nu, np.float64))
    Sig = mpc._blkdiag_dense(np.abs(S))
    a0 = np.zeros(n)
    a0[:nu] = np.abs(uprev)
    dF, r, q, t = D @ F, D @ s + a0, D @ (F @ gb), lrb + urb
    left = np.arange(n)[None, :] < ((np.repeat(np.arange(N), nu) + 1) * nu)[:, None]
    dF = np.where(left, dF, 0)                                  # (|F[u_k]| + |F[u_{k-1}]| is zero right of the staircase anyway)
    M = dF @ Hs
    Fb = Ab + D.T @ (np.where(left, Arb, 0) + Sig @ (2 * M + np.outer(r, gb))) + 2 * (H_sp @ T) + np.outer(H_sp @ e, gb)
    eb = H_sp @ (F @ gb)
    sb = eb + lb + ub + D.T @ (t + Sig @ q)
    Yb = np.hstack([Fb, np.outer(sb, x0), sb[:, None]])
    Fg = F @ gb
    Rst, Qst = np.zeros((N, nu, nu)), np.zeros((N, nx, nx))
    for k in range(N):
        rk = slice(k * blk, (k + 1) * blk)
        Sk = F[rk] @ T[rk].T + np.outer(Fg[rk], e[rk])
        Rst[k], Qst[k] = Sk[:nu, :nu], Sk[nu:, nu:]
    Y = np.hstack([F, G, f[:, None]])
    X0 = np.zeros((nx, n + nx + 1))
    X0[:, n:n + nx] = np.eye(nx)
    X = [X0] + [Y[k * blk + nu:(k + 1) * blk] for k in range(N)]
    Adb, Bdb, cb = np.zeros(Ad.shape), np.zeros(Bd.shape), np.zeros((N, nx))
    Lam = Yb[(N - 1) * blk + nu:N * blk].copy()
    for k in range(N - 1, -1, -1):
        Aclb = Lam @ X[k].T
        Adb[k], Bdb[k], cb[k] = Aclb, Lam[:, k * nu:(k + 1) * nu] + Aclb @ Kz.T, Lam[:, -1]
        if k >= 1:
            Lam = (np.abs(Ad[k]) + np.abs(Bd[k]) @ Kz).T @ Lam + Kz.T @ Yb[k * blk:k * blk + nu] + Yb[(k - 1) * blk + nu:k * blk]
    yr = eb.reshape(N, blk)
    ks = lambda k: slice(k * nu, (k + 1) * nu)
    Sb = np.stack([M[ks(k)] @ dF[ks(k)].T + np.outer(q[ks(k)], r[ks(k)]) for k in range(N)])
    out = dict(Ad=Adb, Bd=Bdb, c=cb, x0=G.T @ sb, xref=yr[:, nu:], uref=yr[:, :nu], S=Sb, uprev=t[:nu] + np.abs(S[0]) @ q[:nu])
    if np.ndim(Q) == 3:
        out.update(Q=Qst, R=Rst)
    else:
        out.update(Q=Qst[:N - 1].sum(0), R=Rst.sum(0), Qf=Qst[N - 1])
    return {k: float(np.abs(v).max()) for k, v in out.items()}


def layer_problem(stage, step=0):
    """``ltv_rate_fixture.driver_problem`` (numpy float64); ``stage`` False: its box instead of E, lo, hi."""
    p = RF.driver_problem(step)
    p["dlo"], p["dhi"] = np.tile(p["dlo"], (SF.B, 1)), np.tile(p["dhi"], (SF.B, 1))
    if not stage:
        _, p["l_add"], p["u_add"] = mpc.box_constraints(SF.NX, SF.NU, SF.N, SF.U_MAX, X_MAX)
    p["stage"] = stage
    return p


def layer_qp(p):
    """(cond, H, g, A, l, u, m0) of the batch by the numpy statements: the base rows, then the rate rows."""
    if p["stage"]:
        cond, H, g, A, l, u = RF.driver_qp(p)
        return cond, H, g, A, l, u, SF.N * SF.NC
    cond = mpc.condense_ltv(p["Ad"], p["Bd"], p["Q"], p["R"], p["Qf"], K=p["K"], S=p["S"])
    g, l0, u0 = mpc.ltv_vectors(cond, p["x0"], p["l_add"], p["u_add"], uprev=p["uprev"])
    A_r, l_r, u_r = mpc.rate_constraints(cond, p["x0"], p["uprev"], p["dlo"], p["dhi"])
    return (cond, cond["H"], g, np.concatenate([cond["A"], A_r], 1), np.concatenate([l0, l_r], 1), np.concatenate([u0, u_r], 1),
            SF.N * (SF.NX + SF.NU))


def rate_active(z, lam, l, u, m0, tol=1e-6):
    """Per instance: some rate row sits on a bound with a multiplier of the matching sign."""
    r = slice(m0, None)
    up = (np.abs(z[:, r] - u[:, r]) <= tol) & (lam[:, r] > tol)
    dn = (np.abs(z[:, r] - l[:, r]) <= tol) & (lam[:, r] < -tol)
    return (up | dn).any(1)


def reference_gradients(p, x, y, act, w):
    """d(sum w . u0) / d(Ad, Bd, x0, S, uprev, dlo, dhi, and E, lo, hi on stage rows) by the numpy chain at the solution (x, y)
    [B, ...] and active sets act; S per instance and stage, dlo / dhi per instance."""
    cond, H, _, A, _, _, m0 = layer_qp(p)
    B, n = SF.B, SF.N * SF.NU
    adj = []
    for b in range(B):
        dx = np.zeros(n)
        dx[:SF.NU] = w[b]                                       # u0 = v[:nu] - K x0
        adj.append(R.adjoint(H[b], A[b], x[b], y[b], act[b], dx))
    st = lambda k: np.stack([a[k] for a in adj])
    dA, dl, du = st("dA"), st("dl"), st("du")
    kw = dict(K=p["K"], dH=st("dH"), dg=st("dg"), S=p["S"], uprev=p["uprev"], dA_r=dA[:, m0:], dl_r=dl[:, m0:], du_r=du[:, m0:])
    extra = {}
    if p["stage"]:
        dA_full, dl_full, dE, dlo, dhi = mpc.stage_constraints_vjp(cond, p["E"], p["x0"], dA[:, :m0], dl[:, :m0], du[:, :m0])
        box = np.zeros(SF.N * (SF.NX + SF.NU))
        out = mpc.condense_ltv_vjp(p["Ad"], p["Bd"], p["Q"], p["R"], p["Qf"], p["x0"], box, box, dA=dA_full, dl=dl_full, du=None, **kw)
        extra = dict(E=dE, lo=dlo, hi=dhi)
    else:
        out = mpc.condense_ltv_vjp(p["Ad"], p["Bd"], p["Q"], p["R"], p["Qf"], p["x0"], p["l_add"], p["u_add"], dA=dA[:, :m0],
                                   dl=dl[:, :m0], du=du[:, :m0], **kw)
    out["x0"] = out["x0"] - w @ p["K"]                          # the direct term of u0 = v0 - K x0
    out.update(extra)
    return out
