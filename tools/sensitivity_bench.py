"""Cost of the forward sensitivities (ReLU_QP.jvp, include/rqp_abi.h rqp_sensitivity) next to one adjoint call on the same solve.

For each workload, one handle set up with polish=True, differentiable=True and sensitivity=True (cold solve,
warm_starting=False).  After one solve: the adjoint call adjoint(dx, dy) with and without the matrix gradients, and the
sensitivity call jvp() with ndir = 1, 12 and 16 shared directions of g, l and u (MPC's feedback-gain tangents: dg, dl = du),
each timed with HIP events -- the first call (cold) and the median of --reps further calls (warm).  On the MPC workloads also
LinearMPC.feedback_gain (ndir = nx = 12).  Per-kernel times: run the same command under `rocprofv3 --kernel-trace --stats`.

    python tools/sensitivity_bench.py [--reps 10] [--out profiles/r7_sensitivity/sensitivity_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "reluqp-py_amd")]

from reluqp import mpc, utils  # noqa: E402
import reluqp.reluqpth as reluqpth  # noqa: E402

DEV = torch.device("cuda:0")


def _ctl(form):
    Ad, Bd = mpc.random_plant(12, 4, seed=0)
    return mpc.LinearMPC(Ad, Bd, np.eye(12), 0.1 * np.eye(4), 20, 0.5, 10.0, form=form)


def _timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(reps + 1):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return out[0], float(np.median(out[1:]))


def _run(name, H, g, A, l, u, prec, reps, ctl=None, x0=None):
    out = dict(name=name, batch=int(g.shape[0]), n=int(g.shape[1]), m=int(l.shape[1]), shared=H.ndim == 2,
               dtype=str(prec).replace("torch.", ""))
    m = reluqpth.ReLU_QP()
    m.setup(H, g, A, l, u, device=DEV, precision=prec, warm_starting=False, polish=True, differentiable=True,
            sensitivity=True)
    out["kernel"] = m.kernel
    m.solve()
    r = m.results
    out["solved"] = int((r.info.status_code == 0).sum())
    rs = np.random.RandomState(0)
    dx = torch.as_tensor(rs.randn(*r.x.shape), dtype=prec, device=DEV)
    dy = torch.as_tensor(rs.randn(*r.y.shape), dtype=prec, device=DEV)
    m.synchronous = False
    out["adjoint_cold_ms"], out["adjoint_ms"] = _timed(lambda: m.adjoint(dx, dy), reps)
    _, out["adjoint_vec_only_ms"] = _timed(lambda: m.adjoint(dx, dy, mats=False), reps)
    n, mm = out["n"], out["m"]
    for nd in (1, 12, 16):
        dg = torch.as_tensor(rs.randn(n, nd), dtype=prec, device=DEV)
        dlu = torch.as_tensor(rs.randn(mm, nd), dtype=prec, device=DEV)
        cold, warm = _timed(lambda: m.jvp(dg=dg, dl=dlu, du=dlu), reps)
        out["jvp%d_cold_ms" % nd], out["jvp%d_ms" % nd] = cold, warm
        out["jvp%d_over_adjoint" % nd] = warm / out["adjoint_ms"]
        out["jvp%d_over_adjoint_vec_only" % nd] = warm / out["adjoint_vec_only_ms"]
    s = m.jvp(dg=dg, dl=dlu, du=dlu)
    torch.cuda.synchronize()
    st = s.status.cpu().numpy()
    res = s.residual.cpu().numpy()[st == 1]
    out["sens_status_1"] = int((st == 1).sum())
    out["sens_res_median"] = float(np.median(res)) if res.size else None
    if ctl is not None:
        ctl.solver, ctl._ready = m, True
        xt = torch.as_tensor(x0, dtype=prec, device=DEV)
        _, out["feedback_gain_ms"] = _timed(lambda: ctl.feedback_gain(xt), reps)
        out["feedback_gain_over_adjoint"] = out["feedback_gain_ms"] / out["adjoint_ms"]
    print(json.dumps(out), flush=True)
    del m
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r7_sensitivity", "sensitivity_bench.json"))
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    args = ap.parse_args()
    only = None if args.only is None else set(args.only.split(","))
    res = []
    if only is None or "headline_randqp" in only:
        # (the generator forks its workers: the batch is drawn before the process touches the GPU)
        p300 = utils.rand_qp_batch(4096, 100, 25, 275, seed0=0, feasible=True, workers=16)
        res.append(_run("headline_randqp", *p300[:5], torch.float32, args.reps))
        del p300
    for form, B in (("condensed", 4096), ("sparse", 1024)):
        name = "mpc_c3_" + form
        if only is None or name in only:
            ctl = _ctl(form)
            x0 = np.random.RandomState(1).randn(B, 12)
            g, l, u = ctl.qp_vectors(x0)
            res.append(_run(name, ctl.H, g, ctl.A, l, u, torch.float32, args.reps, ctl=ctl, x0=x0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, results=res), f, indent=1)


if __name__ == "__main__":
    main()
