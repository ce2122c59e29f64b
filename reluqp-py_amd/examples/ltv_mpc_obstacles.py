"""Obstacle avoidance by linearised half-planes on a batch of 2-D double integrators (BatchedLTVMPC(stage_rows=nc)).

Every instance drives its own point mass (state [p_x, p_y, v_x, v_y], input = acceleration) to the origin past its own disc
obstacle.  At every control step the disc is replaced, per instance and per stage of the horizon, by the half-plane tangent to
it at the point nearest the predicted position, a_k' p_{k+1} >= a_k' o + r  with  a_k = (p_k - o) / |p_k - o|: one row of
E_k on the state.  Two more rows of E_k are the input box, so a stage has nc = 3 constraint rows and the QPs m = 3 N rows
instead of the box's 6 N.  A_c = E F, l_c, u_c are built on the device (rqp_ltv_stage_rows / rqp_ltv_stage_vectors) on the
workspace of the condensing; E changes at every step, so every step is a linearize().

    python reluqp-py_amd/examples/ltv_mpc_obstacles.py [--batch 256] [--steps 60]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from reluqp import mpc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args()
    dev, prec = torch.device("cuda:0"), torch.float32
    B, N, nx, nu, nc, dt, u_max, big = args.batch, 12, 4, 2, 3, 0.2, 1.5, 1e3
    gen = torch.Generator().manual_seed(0)
    I2, Z2 = torch.eye(2), torch.zeros(2, 2)
    A0 = torch.cat([torch.cat([I2, dt * I2], 1), torch.cat([Z2, I2], 1)], 0).to(dev, prec)
    B0 = torch.cat([0.5 * dt * dt * I2, dt * I2], 0).to(dev, prec)
    Ad, Bd = A0.expand(B, N, nx, nx).contiguous(), B0.expand(B, N, nx, nu).contiguous()
    ang = 2 * np.pi * torch.rand(B, generator=gen)
    p0 = 4.0 * torch.stack([torch.cos(ang), torch.sin(ang)], 1)
    side = 0.5 * (2 * torch.rand(B, 1, generator=gen) - 1)      # the disc sits a little off the straight line to the origin
    obst = (0.5 * p0 + side * torch.stack([-p0[:, 1], p0[:, 0]], 1) / 4.0).to(dev, prec)
    radius = (0.6 + 0.3 * torch.rand(B, generator=gen)).to(dev, prec)
    x = torch.cat([p0, torch.zeros(B, 2)], 1).to(dev, prec)

    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q=np.diag([1.0, 1.0, 0.1, 0.1]), R=0.1 * np.eye(nu), Qf=np.diag([10.0, 10.0, 1.0, 1.0]),
                            stage_rows=nc, device=dev, precision=prec, eps_abs=1e-3)
    E = torch.zeros(B, N, nc, nu + nx, device=dev, dtype=prec)
    E[:, :, 0, 0] = E[:, :, 1, 1] = 1.0
    lo = torch.empty(B, N, nc, device=dev, dtype=prec)
    hi = torch.empty(B, N, nc, device=dev, dtype=prec)
    lo[:, :, :2], hi[:, :, :2], hi[:, :, 2] = -u_max, u_max, big
    pred = x[:, None, :2].expand(B, N, 2).clone()               # predicted positions p_1 .. p_N (first step: the start)
    clearance, its = [], []
    for _ in range(args.steps):
        a = pred - obst[:, None]
        a = a / a.norm(dim=2, keepdim=True).clamp_min(1e-6)
        E[:, :, 2, nu:nu + 2] = a
        lo[:, :, 2] = (a * obst[:, None]).sum(2) + radius[:, None]
        ctl.linearize(Ad, Bd, E=E)
        u0, res = ctl.step(x, lo=lo.reshape(B, N * nc), hi=hi.reshape(B, N * nc))
        v = res.x.reshape(B, N, nu)
        xk, traj = x, []
        for k in range(N):                                      # the predicted trajectory, for the next step's half-planes
            xk = xk @ A0.T + v[:, k] @ B0.T
            traj.append(xk[:, :2])
        pred = torch.stack(traj, 1)
        x = x @ A0.T + u0 @ B0.T
        clearance.append(((x[:, :2] - obst).norm(dim=1) - radius).min().item())
        its.append(res.info.iter.float().mean().item())
    print("kernel: %s, QP rows m = %d (the box would have %d)" % (ctl.solver.kernel, ctl.m, N * (nx + nu)))
    print("distance to the origin: start %.2f -> end %.3f (max over the batch)" % (4.0, x[:, :2].norm(dim=1).max().item()))
    print("smallest clearance to an obstacle over the run: %.3f; mean ADMM iterations: first step %.1f, last ten %.1f"
          % (min(clearance), its[0], float(np.mean(its[-10:]))))


if __name__ == "__main__":
    main()
