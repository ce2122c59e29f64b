"""Cost and effect of solution polishing (ReLU_QP.setup(polish=True), include/rqp_abi.h rqp_set_polish).

For each workload: the device time of solve() with and without polish (cold solves, warm_starting=False, so every
repetition runs the same iterations; median of --reps), the polish chain's share (the difference), the status_polish
counts, the max residuals before / after, and on the planted random QPs max |x - x_sol| with and without polish.

    python tools/polish_bench.py [--reps 10] [--out profiles/r5_polish/polish_bench.json]
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


def _mpc(B, form):
    Ad, Bd = mpc.random_plant(12, 4, seed=0)
    ctl = mpc.LinearMPC(Ad, Bd, np.eye(12), 0.1 * np.eye(4), 20, 0.5, 10.0, form=form)
    g, l, u = ctl.qp_vectors(np.random.RandomState(1).randn(B, 12))
    return ctl.H, g, ctl.A, l, u, None


def _run(name, H, g, A, l, u, xs, prec, reps, **kw):
    out = dict(name=name, batch=int(g.shape[0]), n=int(g.shape[1]), m=int(l.shape[1]), shared=H.ndim == 2,
               dtype=str(prec).replace("torch.", ""))
    for pol in (False, True):
        m = reluqpth.ReLU_QP()
        m.setup(H, g, A, l, u, device=DEV, precision=prec, warm_starting=False, polish=pol, **kw)
        times = []
        for _ in range(reps + 1):
            r = m.solve()
            times.append(m.last_kernel_time)
        key = "polish" if pol else "plain"
        out["kernel"] = m.kernel
        out[key + "_ms"] = 1e3 * float(np.median(times[1:]))
        out[key + "_iter_max"] = int(r.info.iter.max())
        out[key + "_pri_max"] = float(r.info.pri_res[r.info.status_code == 0].max())
        out[key + "_dua_max"] = float(r.info.dua_res[r.info.status_code == 0].max())
        if xs is not None:
            out[key + "_max_err_x"] = float(np.abs(r.x.double().cpu().numpy() - xs).max())
        if pol:
            sp = r.info.status_polish.cpu().numpy()
            out["status_polish"] = {str(k): int((sp == k).sum()) for k in (1, 0, -1)}
            acc = sp == 1
            if xs is not None and acc.any():
                out["polish_max_err_x_accepted"] = float(np.abs(r.x.double().cpu().numpy()[acc] - xs[acc]).max())
            nact = (r.active.cpu().numpy() != 0).sum(1)
            out["active_rows_gt_n"] = int((nact > out["n"]).sum())
        del m
        torch.cuda.empty_cache()
    out["polish_chain_ms"] = out["polish_ms"] - out["plain_ms"]
    out["polish_over_solve"] = out["polish_chain_ms"] / out["plain_ms"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r5_polish", "polish_bench.json"))
    args = ap.parse_args()
    res = []
    # (the generator forks its workers: both batches are drawn before the process touches the GPU)
    p300 = utils.rand_qp_batch(4096, 100, 25, 275, seed0=0, feasible=True, workers=16)
    p200 = utils.rand_qp_batch(4096, 100, 25, 175, seed0=0, feasible=True, workers=16)
    res.append(_run("headline_randqp", *p300, torch.float32, args.reps))
    res.append(_run("headline_randqp_f64", *p300, torch.float64, args.reps))
    res.append(_run("randqp_m200", *p200, torch.float32, args.reps))
    del p300, p200
    res.append(_run("mpc_c3_condensed", *_mpc(4096, "condensed"), torch.float32, args.reps))
    res.append(_run("mpc_c3_sparse", *_mpc(4096, "sparse"), torch.float32, args.reps))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, results=res), f, indent=1)


if __name__ == "__main__":
    main()
