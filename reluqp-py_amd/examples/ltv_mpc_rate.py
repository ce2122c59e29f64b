"""Input-rate (delta u) cost and bounds of batched LTV MPC: move suppression and a slew limit.

A batch of 2-D double integrators (state [p, v], input = acceleration) is steered to the origin.  Without rate terms the first
input jumps to the box |u| <= u_max and the optimal sequence switches sign abruptly.  With BatchedLTVMPC(rate_weight=S, du_max=d)
the cost gains 1/2 sum_k (u_k - u_{k-1})' S (u_k - u_{k-1}) and every step obeys |u_k - u_{k-1}| <= d, both counted from the
input applied at the previous control step: `u_prev` is given once, every later step starts from the input the one before
returned, so `simulate` runs the closed loop unchanged.

    python reluqp-py_amd/examples/ltv_mpc_rate.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from reluqp import mpc                      # noqa: E402

nx, nu, N, B, dt = 4, 2, 10, 64, 0.25
dev, f64 = torch.device("cuda:0"), torch.float64
t = lambda a: torch.as_tensor(a, dtype=f64, device=dev)
I2, Z2 = np.eye(2), np.zeros((2, 2))
A0 = np.block([[I2, dt * I2], [Z2, I2]])
B0 = np.vstack([0.5 * dt * dt * I2, dt * I2])
rs = np.random.RandomState(0)
Ad = t(A0[None, None] + 0.01 * rs.randn(B, N, nx, nx))           # one linearisation per instance and stage
Bd = t(B0[None, None] + 0.01 * rs.randn(B, N, nx, nu))
ang = rs.uniform(0, 2 * np.pi, B)
x0 = t(np.hstack([1.5 * np.stack([np.cos(ang), np.sin(ang)], 1), 0.1 * rs.randn(B, 2)]))
Q, R = np.diag([1.0, 1.0, 0.1, 0.1]), 0.05 * np.eye(nu)
u_max, du_max, steps = 2.0, 0.4, 24
u_start = t(np.zeros((B, nu)))                                   # the actuators are at rest


def plant(x, u):                                                 # the stage-0 model of every instance; the linearisation is kept
    return torch.einsum("bij,bj->bi", Ad[:, 0], x) + torch.einsum("bij,bj->bi", Bd[:, 0], u), Ad, Bd, None


def run(**rate):
    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, 2.0 * Q, u_max=u_max, x_max=10.0, device=dev, precision=f64, eps_abs=1e-5, **rate)
    ctl.linearize(Ad, Bd)
    xs, us, its = ctl.simulate(x0, steps, plant, relinearize_every=steps, u_prev=u_start if rate else None)
    moves = torch.diff(torch.cat([u_start[None], us]), dim=0).abs()
    return ctl, xs, us, its, moves


for name, rate in (("no rate terms", {}), ("move suppression", dict(rate_weight=0.5 * np.eye(nu))),
                   ("slew limit", dict(du_max=du_max)), ("both", dict(rate_weight=0.5 * np.eye(nu), du_max=du_max))):
    ctl, xs, us, its, moves = run(**rate)
    print("%-17s m = %3d  max|u_k - u_{k-1}| %.3f  mean %.3f  |p| after %d steps %.3f  mean iterations %.0f"
          % (name, ctl.m, moves.max().item(), moves.mean().item(), steps, xs[-1, :, :2].norm(dim=1).mean().item(),
             its.double().mean().item()))

# per-instance, per-stage weights and asymmetric limits: linearize(S=) and step(du_lo=, du_hi=), kept until replaced
ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, 2.0 * Q, u_max=u_max, x_max=10.0, du_max=np.inf, device=dev, precision=f64, eps_abs=1e-5)
k = torch.arange(N, dtype=f64, device=dev)
scale = torch.linspace(0.1, 2.0, B, dtype=f64, device=dev)
S = (scale[:, None] / (1.0 + k[None, :]))[:, :, None, None] * torch.eye(nu, dtype=f64, device=dev)        # [B, N, nu, nu]
ctl.linearize(Ad, Bd, S=S)
lo = t(np.tile([-du_max, -np.inf], N))                           # the first input may only rise slowly, the second is free
hi = t(np.tile([0.5 * du_max, np.inf], N))
u0, res = ctl.step(x0, u_prev=u_start, du_lo=lo, du_hi=hi)
print("stage weights + asymmetric limits: u0[:, 0] - u_prev in [%.3f, %.3f] (limits [%.3f, %.3f]); %d / %d solved"
      % ((u0 - u_start)[:, 0].min().item(), (u0 - u_start)[:, 0].max().item(), -du_max, 0.5 * du_max,
         sum(s == "solved" for s in res.info.status), B))
