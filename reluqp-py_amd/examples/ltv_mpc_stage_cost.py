"""Stage-varying, per-instance cost weights of batched LTV MPC.

Part 1: one BatchedLTVMPC handle drives a batch in which every instance ramps its state weight towards the end of the horizon
at its own rate (Q_k = (1 + a_b k / N) Q, a different a_b per instance): stage weights [B, N, nx, nx] given to linearize().
Part 2: the per-stage ramp of an expert controller is recovered by gradient descent on ||u0 - u0_expert||^2 through
reluqp.layer.LTVMPCLayer, whose gradient of a [N, nx, nx] weight is per stage (summed over the batch).

    python reluqp-py_amd/examples/ltv_mpc_stage_cost.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from reluqp import mpc                      # noqa: E402
from reluqp.layer import LTVMPCLayer        # noqa: E402

nx, nu, N, B = 6, 2, 8, 32
dev, f64 = torch.device("cuda:0"), torch.float64
Ad0, Bd0 = mpc.random_plant(nx, nu, seed=3)
rs = np.random.RandomState(0)
t = lambda a: torch.as_tensor(a, dtype=f64, device=dev)
Ad = t(Ad0[None, None] + 0.02 * rs.randn(B, N, nx, nx))          # one linearisation per instance and stage
Bd = t(Bd0[None, None] + 0.02 * rs.randn(B, N, nx, nu))
x0 = t(0.3 * rs.randn(B, nx))
Q, R = np.eye(nx), 0.1 * np.eye(nu)
k = torch.arange(N, dtype=f64, device=dev)

# ---- 1. a batch of different tasks on one handle
ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, u_max=0.4, x_max=8.0, device=dev, precision=f64, eps_abs=1e-4)
ctl.linearize(Ad, Bd)                                            # the constructor's shared (Q, R, Qf)
u_shared, _ = ctl.step(x0)
slope = torch.linspace(0.0, 8.0, B, dtype=f64, device=dev)       # instance b ramps to (1 + slope_b) Q at the end of the horizon
Qs = (1.0 + slope[:, None] * (k[None, :] + 1) / N)[:, :, None, None] * t(Q)      # [B, N, nx, nx]; R stays the shared one
ctl.linearize(Ad, Bd, Q=Qs)                                      # kept until replaced
u_ramp, res = ctl.step(x0)
moved = (u_ramp - u_shared).norm(dim=1)
print("shared weights -> per-instance ramps: |u0 change| %.2e (slope 0: the terminal weight alone) ... %.2e (slope 8); %d / %d solved"
      % (moved[0].item(), moved[-1].item(), sum(s == "solved" for s in res.info.status), B))

# ---- 2. recover a per-stage weight profile through the layer
layer = LTVMPCLayer(nx, nu, N, u_max=0.4, x_max=8.0, eps_abs=1e-6)
Rt = t(R)
profile_true = 1.0 + 3.0 * (k / (N - 1)) ** 2                    # the expert's Q_k = profile_k Q
stage_Q = lambda profile: profile[:, None, None] * t(Q)          # [N, nx, nx]: shared by the batch, one block per stage
with torch.no_grad():
    u_expert, _ = layer(Ad, Bd, x0, stage_Q(profile_true), Rt, None)

w = torch.zeros(N, dtype=f64, device=dev, requires_grad=True)    # profile = exp(w), started flat
opt = torch.optim.Adam([w], lr=0.1)
for it in range(150):
    opt.zero_grad()
    u0, _ = layer(Ad, Bd, x0, stage_Q(torch.exp(w)), Rt, None)
    loss = ((u0 - u_expert) ** 2).sum()
    loss.backward()
    opt.step()
    if it % 30 == 0 or it == 149:
        print("iter %3d  loss %.3e  profile %s" % (it, loss.item(), np.round(torch.exp(w).tolist(), 2)))
print("expert profile        %s" % np.round(profile_true.tolist(), 2))
