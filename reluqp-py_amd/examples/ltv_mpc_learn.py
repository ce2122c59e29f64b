"""Learning through a batched MPC controller: recover the input weight R of an expert controller by gradient descent on
||u0 - u0_expert||^2 through reluqp.layer.LTVMPCLayer (device condensing, batched QP solve, adjoint of both).

    python reluqp-py_amd/examples/ltv_mpc_learn.py
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
Q = t(np.eye(nx))
R_true = t(np.diag([0.3, 0.05]))

layer = LTVMPCLayer(nx, nu, N, u_max=0.4, x_max=8.0, eps_abs=1e-6)
with torch.no_grad():
    u_expert, _ = layer(Ad, Bd, x0, Q, R_true, Q)

r = torch.full((nu,), np.log(0.1), dtype=f64, device=dev, requires_grad=True)     # R = diag(exp(r)), started at 0.1 I
opt = torch.optim.Adam([r], lr=0.1)
for it in range(60):
    opt.zero_grad()
    u0, _ = layer(Ad, Bd, x0, Q, torch.diag(torch.exp(r)), Q)
    loss = ((u0 - u_expert) ** 2).sum()
    loss.backward()
    opt.step()
    if it % 10 == 0 or it == 59:
        print("iter %2d  loss %.3e  R = diag(%s)" % (it, loss.item(), np.round(torch.exp(r).tolist(), 4)))
print("expert R = diag(%s)" % R_true.diagonal().tolist())
