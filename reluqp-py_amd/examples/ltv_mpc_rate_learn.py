"""Learning how hard a controller is penalised for moving the actuator: recover the move-suppression weight S of an expert
controller by gradient descent on ||u0 - u0_expert||^2 through reluqp.layer.LTVMPCLayer(rate_rows=True) (device condensing with
the input-rate cost and slew-rate rows, batched QP solve, adjoint of both).

    python reluqp-py_amd/examples/ltv_mpc_rate_learn.py
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
u_prev = t(0.05 * rs.randn(B, nu))                               # the input applied before stage 0
Q, R = t(np.eye(nx)), t(0.05 * np.eye(nu))
du = t(np.full(N * nu, 0.3))                                     # |u_k - u_{k-1}| <= 0.3, shared by the batch
S_true = t(np.diag([0.4, 0.05]))

layer = LTVMPCLayer(nx, nu, N, u_max=0.4, x_max=8.0, rate_rows=True, eps_abs=1e-6)
with torch.no_grad():
    u_expert, _ = layer(Ad, Bd, x0, Q, R, Q, S=S_true, u_prev=u_prev, du_lo=-du, du_hi=du)

s = torch.full((nu,), np.log(0.15), dtype=f64, device=dev, requires_grad=True)    # S = diag(exp(s)), started at 0.15 I
opt = torch.optim.Adam([s], lr=0.1)
for it in range(80):
    opt.zero_grad()
    u0, _ = layer(Ad, Bd, x0, Q, R, Q, S=torch.diag(torch.exp(s)), u_prev=u_prev, du_lo=-du, du_hi=du)
    loss = ((u0 - u_expert) ** 2).sum()
    loss.backward()
    opt.step()
    if it % 10 == 0 or it == 79:
        print("iter %2d  loss %.3e  S = diag(%s)" % (it, loss.item(), np.round(torch.exp(s).tolist(), 4)))
print("expert S = diag(%s)" % S_true.diagonal().tolist())
