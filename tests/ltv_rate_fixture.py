"""Fixtures of the input-rate tests (tests/test_ltv_rate_*.py): rate weights that differ for every (instance, stage), a
step-by-step rollout of the plant with its cost written out, and the end-to-end problem of the driver test.

Weights: the recipe of tests/ltv_stage_cost_fixture.py, S_{b,k} = (1 + 0.3 k)(1 + 0.1 b)(D + 0.05 M M'), symmetric positive definite
and not diagonal: a block read from the wrong stage or instance moves the result far outside any tolerance.

Driver problem: the 2-D double integrators of tests/ltv_stage_fixture.py (nx = 4, nu = 2, N = 8, B = 16, stage_rows = 3: the input
box as two rows and a half-plane) with a move-suppression weight and the slew limit |u_k - u_{k-1}| <= DU_MAX.  The optimum of the
problem without the limit starts with an input of about U_MAX towards the origin; u_prev is a small random input, so the step
from u_prev to u_0 runs into the limit: at the oracle's optimum 16 of the 16 instances have an active rate row
(tests/test_ltv_rate_cpu.py computes the number from the numpy QP and checks it).  Everything is a pure function of the
constants below."""
import numpy as np

from reluqp import mpc

import ltv_stage_cost_fixture as SC
import ltv_stage_fixture as SF

DU_MAX = 0.5
DRIVER_SEED = 31


def rate_weights(rs, B, N, nu):
    """S [B, N, nu, nu]."""
    return SC.spd_blocks(rs, (B, N), nu, 1.0)


def rollout(Ad, Bd, K, c, x0, v):
    """The plant, one step at a time: (u [N, nu], x [N, nx]) with u_k = -K x_k + v_k, x = x_1 .. x_N."""
    N, nx, nu = Ad.shape[0], Ad.shape[1], Bd.shape[2]
    Kz = np.zeros((nu, nx), dtype=Ad.dtype) if K is None else K
    cz = np.zeros((N, nx), dtype=Ad.dtype) if c is None else c
    x, us, xs = np.asarray(x0).copy(), [], []
    for k in range(N):
        u = -Kz @ x + v[k * nu:(k + 1) * nu]
        x = Ad[k] @ x + Bd[k] @ u + cz[k]
        us.append(u)
        xs.append(x)
    return np.stack(us), np.stack(xs)


def rollout_cost(us, xs, Q, R, S, uprev, xref=None, uref=None):
    """(J, sum of the absolute values of its terms) of a rolled-out trajectory: Q, R [N, ., .] (Q_k weighs x_{k+1}), S [N, nu, nu],
    J = sum_k 1/2 (u_k - uref_k)' R_k (.) + 1/2 (x_{k+1} - xref_k)' Q_k (.) + 1/2 (u_k - u_{k-1})' S_k (.),  u_{-1} = uprev."""
    N = us.shape[0]
    J = Jabs = 0.0
    quad = lambda W, e: (0.5 * e @ W @ e, 0.5 * np.abs(e) @ np.abs(W) @ np.abs(e))
    for k in range(N):
        eu = us[k] - (0.0 if uref is None else uref[k])
        ex = xs[k] - (0.0 if xref is None else xref[k])
        du = us[k] - (uprev if k == 0 else us[k - 1])
        for val, mag in (quad(R[k], eu), quad(Q[k], ex), quad(S[k], du)):
            J, Jabs = J + val, Jabs + mag
    return J, Jabs


def driver_problem(step=0):
    """ltv_stage_fixture.problem plus S [B, N, nu, nu], uprev [B, nu], dlo, dhi [N nu] (numpy float64)."""
    p = SF.problem(step)
    rs = np.random.RandomState(DRIVER_SEED)
    p["S"] = 0.02 * rate_weights(rs, SF.B, SF.N, SF.NU)
    p["uprev"] = 0.2 * rs.randn(SF.B, SF.NU)
    p["dlo"], p["dhi"] = np.full(SF.N * SF.NU, -DU_MAX), np.full(SF.N * SF.NU, DU_MAX)
    return p


def driver_qp(p, uprev=None):
    """(cond, H, g, A, l, u) of the batch by the numpy statements: the stage rows, then the rate rows."""
    uprev = p["uprev"] if uprev is None else uprev
    cond = mpc.condense_ltv(p["Ad"], p["Bd"], p["Q"], p["R"], p["Qf"], K=p["K"], S=p["S"])
    box = np.zeros(SF.N * (SF.NX + SF.NU))
    g, _, _ = mpc.ltv_vectors(cond, p["x0"], box, box, uprev=uprev)
    A_c, l_c, u_c = mpc.stage_constraints(cond, p["E"], p["x0"], p["lo"], p["hi"])
    A_r, l_r, u_r = mpc.rate_constraints(cond, p["x0"], uprev, p["dlo"], p["dhi"])
    return (cond, cond["H"], g, np.concatenate([A_c, A_r], 1), np.concatenate([l_c, l_r], 1), np.concatenate([u_c, u_r], 1))


def rate_active(z, lam, l, u, tol=1e-6):
    """Per instance: some rate row sits on a bound with a multiplier of the matching sign."""
    r = slice(SF.N * SF.NC, None)
    up = (np.abs(z[:, r] - u[:, r]) <= tol) & (lam[:, r] > tol)
    dn = (np.abs(z[:, r] - l[:, r]) <= tol) & (lam[:, r] < -tol)
    return (up | dn).any(1)
