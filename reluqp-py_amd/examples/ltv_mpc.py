"""Nonlinear MPC by successive linearisation on a batch of damped pendulums (reluqp.mpc.BatchedLTVMPC).

Every instance is its own plant (length and damping differ) and is re-linearised at its current state at every
control step; the condensed QPs (H, A, g, l, u) are built on the device (rqp_ltv_condense / rqp_ltv_vectors) and solved by
the per-instance kernels with the previous step's ADMM state as warm start.  State x = [angle from upright, angular
velocity], input u = torque; the task is to bring the pendulum upright (x = 0) from an initial deflection of up to 0.4 rad (within what the torque limit
can hold for every length in the batch).

    python reluqp-py_amd/examples/ltv_mpc.py [--batch 256] [--steps 80]
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
    ap.add_argument("--steps", type=int, default=80)
    args = ap.parse_args()
    dev, prec = torch.device("cuda:0"), torch.float32
    B, N, nx, nu, dt = args.batch, 20, 2, 1, 0.05
    gen = torch.Generator().manual_seed(0)
    grav_l = (9.81 / (0.8 + 0.4 * torch.rand(B, generator=gen))).to(dev, prec)       # g / length
    damp = (0.05 + 0.1 * torch.rand(B, generator=gen)).to(dev, prec)

    def f(x, u):                                                # explicit Euler step of th'' = (g / l) sin th - d th' + u
        th, om = x[..., 0], x[..., 1]
        return torch.stack([th + dt * om, om + dt * (grav_l * torch.sin(th) - damp * om + u[..., 0])], dim=-1)

    def linearise(x):
        """Stages of the model linearised at the current state (held over the horizon, input 0):
        A = df/dx(x, 0), B = df/du, c = f(x, 0) - A x, per instance."""
        A = torch.zeros(B, nx, nx, device=dev, dtype=prec)
        A[:, 0, 0], A[:, 0, 1] = 1.0, dt
        A[:, 1, 0], A[:, 1, 1] = dt * grav_l * torch.cos(x[:, 0]), 1.0 - dt * damp
        Bm = torch.zeros(B, nx, nu, device=dev, dtype=prec)
        Bm[:, 1, 0] = dt
        c = f(x, torch.zeros(B, nu, device=dev, dtype=prec)) - (A @ x[..., None])[..., 0]
        rep = lambda t: t[:, None].expand(B, N, *t.shape[1:]).contiguous()
        return rep(A), rep(Bm), rep(c)

    def plant(x, u):
        xn = f(x, u)
        return (xn,) + linearise(xn)

    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q=np.diag([10.0, 1.0]), R=0.1 * np.eye(1), Qf=np.diag([50.0, 5.0]), u_max=6.0, x_max=4.0,
                            device=dev, precision=prec, eps_abs=1e-3)
    x0 = torch.stack([0.4 * (2 * torch.rand(B, generator=gen) - 1), torch.zeros(B)], dim=-1).to(dev, prec)
    ctl.linearize(*linearise(x0))
    xs, us, its = ctl.simulate(x0, args.steps, plant, relinearize_every=1)
    print("kernel:", ctl.solver.kernel, " last step solved: %d / %d" % (sum(s == "solved" for s in ctl.solver.results.info.status), B))
    print("max |angle|: start %.3f -> end %.4f" % (xs[0, :, 0].abs().max().item(), xs[-1, :, 0].abs().max().item()))
    print("max |torque| %.3f, mean ADMM iterations: first step %.1f, last ten steps %.1f"
          % (us.abs().max().item(), its[0].float().mean().item(), its[-10:].float().mean().item()))


if __name__ == "__main__":
    main()
