"""Fixtures of the stage-weight tests (tests/test_ltv_stage_cost_*.py): weights that differ for every (instance, stage), and
the end-to-end problems of the layer test with their numpy reference chain.

Weights: random symmetric positive definite blocks, not diagonal, (1 + 0.3 k)(1 + 0.1 b) w (D + 0.05 M M') with D a random
positive diagonal and M standard normal: the scale grows with the stage k and with the instance b, so a block read from the
wrong stage or the wrong instance, or a misplaced terminal block, moves the result far outside any tolerance.

Layer problems: the plants, states and references of tests/ltv_adjoint_fixture.py with such weights in place of its shared
(Q, R, Qf); the scale of every instance's initial state is chosen (on the CPU, tests/test_ltv_stage_cost_cpu.py checks it for
every instance) so that the solution has active rows (two to six of them) with margins >= ltv_adjoint_fixture.MARGIN."""
import numpy as np

from reluqp import mpc

import adjoint_ref as R
import ltv_adjoint_fixture as FX

B = FX.B
SHAPES = FX.SHAPES
U_MAX, X_MAX = FX.U_MAX, FX.X_MAX
WEIGHT_SEED = {(6, 2, 8): 21, (12, 4, 20): 22}
# scale of each instance's initial state (times the unit-normal draw of ltv_adjoint_fixture.problem)
X0_SCALE = {(6, 2, 8): (0.1, 0.1, 0.1, 0.14, 0.2, 0.26, 0.14, 0.1, 0.32, 0.1, 0.26, 0.2, 0.12, 0.26, 0.14, 0.06),
            (12, 4, 20): (0.1, 0.06, 0.06, 0.2, 0.08, 0.12, 0.12, 0.1, 0.1, 0.1, 0.08, 0.1, 0.1, 0.14, 0.06, 0.14)}


def spd_blocks(rs, lead, d, w=1.0):
    """Blocks [*lead, d, d] = growth(k, b) w (D + 0.05 M M'); lead = (N,) or (B, N)."""
    M = rs.randn(*lead, d, d)
    D = 1.0 + rs.rand(*lead, d)
    W = 0.05 * M @ np.swapaxes(M, -1, -2)
    W[..., np.arange(d), np.arange(d)] += D
    k = np.arange(lead[-1], dtype=np.float64)
    grow = 1.0 + 0.3 * k
    if len(lead) == 2:
        grow = (1.0 + 0.1 * np.arange(lead[0], dtype=np.float64))[:, None] * grow[None, :]
    W = w * grow[..., None, None] * W
    return 0.5 * (W + np.swapaxes(W, -1, -2))


def stage_weights(rs, B, N, nx, nu):
    """(Q [B, N, nx, nx], R [B, N, nu, nu])."""
    return spd_blocks(rs, (B, N), nx, 1.0), spd_blocks(rs, (B, N), nu, 0.1)


def repeated(Q, R, Qf, B, N):
    """The shared (Q, R, Qf) written as stage weights [B, N, ., .]."""
    Qs = np.stack([Q] * (N - 1) + [Qf])
    Rs = np.stack([R] * N)
    return np.ascontiguousarray(np.broadcast_to(Qs, (B,) + Qs.shape)), np.ascontiguousarray(np.broadcast_to(Rs, (B,) + Rs.shape))


def dense_H_sp(Q, R):
    """blkdiag(R_0, Q_0, ..., R_{N-1}, Q_{N-1}) of one instance, written out (Q [N, nx, nx], R [N, nu, nu])."""
    N, nx, nu = Q.shape[0], Q.shape[1], R.shape[1]
    blk = nx + nu
    S = np.zeros((N * blk, N * blk), dtype=np.result_type(Q.dtype, R.dtype))
    for k in range(N):
        S[k * blk:k * blk + nu, k * blk:k * blk + nu] = R[k]
        S[k * blk + nu:(k + 1) * blk, k * blk + nu:(k + 1) * blk] = Q[k]
    return S


DRIVER = dict(nx=12, nu=4, N=20, B=16, seed=0, x0_seed=7)


def driver_case():
    """The closed-loop driver's case (numpy float64): perturbed stages of one plant, the shared (Q, R, P) with their LQR gain
    K, stage weights [B, N, ., .] and initial states; the oracle's float32 and float64 runs on the host-condensed QPs agree on
    the iteration counts (tests/test_ltv_stage_cost_cpu.py)."""
    d = DRIVER
    nx, nu, N, B = d["nx"], d["nu"], d["N"], d["B"]
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=d["seed"])
    rs = np.random.RandomState(d["seed"] + 1)
    Ad = Ad0[None, None] + 0.02 * rs.randn(B, N, nx, nx) / np.sqrt(nx)
    Bd = Bd0[None, None] + 0.02 * rs.randn(B, N, nx, nu)
    Q, R_ = np.eye(nx), 0.1 * np.eye(nu)
    K, P = mpc.ihlqr(Ad0, Bd0, Q, R_, Q)
    Qs, Rs = stage_weights(rs, B, N, nx, nu)
    x0 = 1.5 * np.random.RandomState(d["x0_seed"]).randn(B, nx)
    return dict(Ad=Ad, Bd=Bd, Ad0=Ad0, Bd0=Bd0, Q=Q, R=R_, P=0.5 * (P + P.T), K=K, Qs=Qs, Rs=Rs, x0=x0)


def driver_qp(c, Qs=None, Rs=None):
    """(H, g, A, l, u) of the driver's batch condensed on the host, box |u| <= U_MAX, |x| <= X_MAX."""
    d = DRIVER
    _, l_add, u_add = mpc.box_constraints(d["nx"], d["nu"], d["N"], U_MAX, X_MAX)
    cond = mpc.condense_ltv(c["Ad"], c["Bd"], c["Qs"] if Qs is None else Qs, c["Rs"] if Rs is None else Rs, None, K=c["K"])
    g, l, u = mpc.ltv_vectors(cond, c["x0"], l_add, u_add)
    return cond["H"], g, cond["A"], l, u


FACTORS = (1.0, 1.3, 1.2)                                      # the three forwards of the stale-workspace test: Q f, R / f


def problem(nx, nu, N, x0_scale=None, factor=1.0):
    """Inputs of the layer (numpy float64): Ad, Bd, c, x0, xref, uref [B, ...], Q [B, N, nx, nx], R [B, N, nu, nu], Qf = None, K.
    ``factor`` f: the weights Q f and R / f."""
    p = FX.problem(nx, nu, N)
    unit = p["x0"] / np.asarray(FX.X0_SCALE[(nx, nu, N)], dtype=np.float64).reshape(-1, 1)
    scale = X0_SCALE[(nx, nu, N)] if x0_scale is None else x0_scale
    p["x0"] = np.asarray(scale, dtype=np.float64).reshape(-1, 1) * unit
    Q, R_ = stage_weights(np.random.RandomState(WEIGHT_SEED[(nx, nu, N)]), B, N, nx, nu)
    p["Q"], p["R"], p["Qf"] = factor * Q, R_ / factor, None
    return p


def condensed(p):
    """(H, A, g, l, u) of the batch on the host."""
    N, nx, nu = p["Ad"].shape[1], p["Ad"].shape[2], p["Bd"].shape[3]
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, U_MAX, X_MAX)
    cond = mpc.condense_ltv(p["Ad"], p["Bd"], p["Q"], p["R"], None, K=p["K"], c=p["c"])
    g, l, u = mpc.ltv_vectors(cond, p["x0"], l_add, u_add, xref=p["xref"], uref=p["uref"])
    return cond["H"], cond["A"], g, l, u


def reference_gradients(p, x, y, act, w):
    """d(sum w . u0) / d(inputs) by the numpy chain condense_ltv_vjp o adjoint_ref.adjoint at the solution (x, y) [B, ...] and
    active sets act: per-instance arrays, Q [B, N, nx, nx] and R [B, N, nu, nu] among them."""
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
    out = mpc.condense_ltv_vjp(p["Ad"], p["Bd"], p["Q"], p["R"], None, p["x0"], l_add, u_add, K=p["K"], c=p["c"],
                               xref=p["xref"], uref=p["uref"], dH=st("dH"), dA=st("dA"), dg=st("dg"), dl=st("dl"), du=st("du"))
    out["x0"] = out["x0"] - w @ p["K"]                          # the direct term of u0 = v0 - K x0
    return out
