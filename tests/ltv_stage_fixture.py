"""End-to-end fixture of the stage-constraint tests (tests/test_ltv_stage_gpu.py): a batch of 2-D double integrators (state
[p_x, p_y, v_x, v_y], input = acceleration) steered to the origin, each stage constrained by nc = 3 rows of E: the input box
written as two rows, and one half-plane a_k' p_{k+1} <= b of the instance's own (per stage slightly turned) normal that cuts the
origin off, so it is active at the optimum; every fourth instance has its half-plane far away (never active).  The numpy chain
the layer's gradients are compared with is  stage_constraints_vjp o condense_ltv_vjp o adjoint_ref.adjoint.
Everything is a pure function of the constants below."""
import numpy as np

from reluqp import mpc

import adjoint_ref as R

B, NX, NU, N, NC = 16, 4, 2, 8, 3
U_MAX, DT, FAR = 2.0, 0.25, -50.0                              # FAR: the half-plane's (never active) lower bound
SEED = 4


def problem(step=0):
    """numpy float64: Ad, Bd [B, N, ...], x0 [B, nx], E [B, N, nc, nu + nx], lo, hi [B, N nc], Q, R, Qf, K."""
    rs = np.random.RandomState(100 * SEED + step)
    I2, Z2 = np.eye(2), np.zeros((2, 2))
    A0 = np.block([[I2, DT * I2], [Z2, I2]])
    B0 = np.vstack([0.5 * DT * DT * I2, DT * I2])
    Ad = A0[None, None] + 0.01 * rs.randn(B, N, NX, NX)
    Bd = B0[None, None] + 0.01 * rs.randn(B, N, NX, NU)
    ang = rs.uniform(0, 2 * np.pi, B)
    p0 = (1.0 + 0.3 * rs.rand(B))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    x0 = np.hstack([p0, 0.1 * rs.randn(B, 2)])
    E = np.zeros((B, N, NC, NU + NX))
    E[:, :, 0, 0] = E[:, :, 1, 1] = 1.0                         # rows 0, 1: u_k
    th = ang[:, None] + np.pi + 0.2 * rs.randn(B, N)            # the normal points from p0 to the origin, turned a little
    E[:, :, 2, NU] = np.cos(th)                                 # row 2: a_k' p_{k+1}
    E[:, :, 2, NU + 1] = np.sin(th)
    b = np.where(np.arange(B) % 4 == 3, 5.0, -0.3)              # a' 0 = 0 > -0.3: the origin is cut off
    lo = np.tile(np.array([-U_MAX, -U_MAX, FAR]), (B, N))
    hi = np.tile(np.array([U_MAX, U_MAX, 0.0]), (B, N))
    hi[:, 2::NC] = b[:, None]
    Q, R_ = np.diag([1.0, 1.0, 0.1, 0.1]), 0.05 * np.eye(NU)
    K = 0.05 * rs.randn(NU, NX)
    return dict(Ad=Ad, Bd=Bd, x0=x0, E=E, lo=lo, hi=hi, Q=Q, R=R_, Qf=2.0 * Q, K=K)


def condensed(p):
    """(cond, H, g, A_c, l_c, u_c) of the batch by the numpy statements."""
    cond = mpc.condense_ltv(p["Ad"], p["Bd"], p["Q"], p["R"], p["Qf"], K=p["K"])
    box = np.zeros(N * (NX + NU))
    g, _, _ = mpc.ltv_vectors(cond, p["x0"], box, box)
    A_c, l_c, u_c = mpc.stage_constraints(cond, p["E"], p["x0"], p["lo"], p["hi"])
    return cond, cond["H"], g, A_c, l_c, u_c


def halfplane_active(z, lam, u_c, tol=1e-6):
    """Per instance: some half-plane row sits on its upper bound with a positive multiplier."""
    hp = slice(2, None, NC)
    return ((np.abs(z[:, hp] - u_c[:, hp]) <= tol) & (lam[:, hp] > tol)).any(1)


def reference_gradients(p, x, y, act, w):
    """d(sum w . u0) / d(Ad, Bd, x0, E, lo, hi) by the numpy chain at the solution (x, y) [B, ...] and active sets act."""
    cond, H, _, A_c, _, _ = condensed(p)
    n = N * NU
    adj = []
    for b in range(B):
        dx = np.zeros(n)
        dx[:NU] = w[b]                                          # u0 = v[:nu] - K x0
        adj.append(R.adjoint(H[b], A_c[b], x[b], y[b], act[b], dx))
    st = lambda k: np.stack([a[k] for a in adj])
    dA_full, dl_full, dE, dlo, dhi = mpc.stage_constraints_vjp(cond, p["E"], p["x0"], st("dA"), st("dl"), st("du"))
    box = np.zeros(N * (NX + NU))
    out = mpc.condense_ltv_vjp(p["Ad"], p["Bd"], p["Q"], p["R"], p["Qf"], p["x0"], box, box, K=p["K"], dH=st("dH"), dA=dA_full,
                               dg=st("dg"), dl=dl_full, du=None)
    out["x0"] = out["x0"] - w @ p["K"]                          # the direct term of u0 = v0 - K x0
    out.update(E=dE, lo=dlo, hi=dhi)
    return out
