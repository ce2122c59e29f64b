"""Cost of condensing a batch of LTV plants on the device (reluqp.mpc.condense_ltv_device / ltv_vectors_device,
include/rqp_abi.h rqp_ltv_condense / rqp_ltv_vectors) next to the solver calls it feeds.

At B = 4096, (nx, nu, N) = (12, 4, 20) -> (n, m) = (80, 320), float32 and float64 outputs: device time (HIP events, median of
--reps calls after warm-up) of `condense` (transition + Hessian kernels) and `vectors`, and of update(Hx, Ax) and a
warm-started solve() of the handle set up on that data, in the same run; then the backward column: the condensing's reverse
mode (condense_ltv_adjoint_device, rqp_ltv_condense_adjoint: every cotangent given, every gradient wanted) next to the forward
`condense` and to adjoint() of a differentiable handle set up on the same data.  The host path it replaces -- numpy condense_ltv
over the batch on --workers processes plus the host-to-device copy of (H, A) -- is timed on --host-batch instances and
scaled to B.  Stage columns (--stage-rows nc, default 6 -> m_c = 120): rqp_ltv_stage_rows, rqp_ltv_stage_vectors and
rqp_ltv_stage_adjoint next to `condense`, and update(Hx, Ax) + warm solve() of a BatchedLTVMPC(stage_rows=nc) handle (the input
box as nu rows of E plus nc - nu random half-planes per stage) next to the same two of the box handle at m = 320.
Stage-weight columns (--stage-weights): `condense`, `vectors` (with xref: the call that reads the weights) and the adjoint with
Q [B, N, nx, nx], R [B, N, nu, nu] (RQP_LTV_STAGE_WEIGHTS) next to the shared-weight calls of the same run, the two alternating
call by call (medians of --reps each), on a workspace of their own.
Input-rate columns (--rate): `condense` with a rate weight S [B, N, nu, nu] (rqp_ltv_condense_rate) and `vectors` with it
(rqp_ltv_vectors_rate) next to the plain calls of the same run, alternating call by call, on a workspace of their own;
rqp_ltv_rate_rows and rqp_ltv_rate_bounds written into the tail of [B, m + N nu, ...] tensors; the driver's strided copy of the m
base rows into that tensor; and update(Hx, Ax) + warm solve() of a BatchedLTVMPC(stage_rows=nc, du_max=) handle (m_c + N nu rows)
next to the same two of the stage handle (m_c rows).
Rate-adjoint columns (--rate-adjoint): the reverse mode with the rate terms (condense_ltv_adjoint_rate_device,
rqp_ltv_condense_adjoint_rate: every cotangent given, the three of the rate rows among them, every gradient wanted, dS and duprev
among them) next to the plain adjoint of the same build, alternating call by call, on workspaces of its own (rate_adj_* in --out).
Per-kernel times (k_ltv_transition among them): run the same command under `rocprofv3 --kernel-trace --stats`.

    python tools/ltv_bench.py [--reps 20] [--stage-rows 6] [--stage-weights] [--rate] [--rate-adjoint]
        [--out profiles/r8_ltv/ltv_bench.json] [--rate-out profiles/r12_ltv_rate/ltv_rate_bench.json]
        [--stage-out profiles/r10_ltv_stage/ltv_stage_bench.json] [--stage-weights-out profiles/r11_ltv_stage_cost/ltv_stage_cost_bench.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "reluqp-py_amd")]

from reluqp import mpc  # noqa: E402

NX, NU, N = 12, 4, 20


def _host_one(args):
    Ad, Bd, Q, R, P, K = args
    c = mpc.condense_ltv(Ad, Bd, Q, R, P, K=K)
    return c["H"], c["A"]


def _host_baseline(Ad, Bd, Q, R, P, K, workers):
    """Seconds per instance of the numpy path on `workers` processes (run before this process touches the GPU)."""
    jobs = [(Ad[b], Bd[b], Q, R, P, K) for b in range(Ad.shape[0])]
    with ProcessPoolExecutor(max_workers=workers) as pool:
        list(pool.map(_host_one, jobs[:workers]))                 # start the workers
        t0 = time.perf_counter()
        out = list(pool.map(_host_one, jobs, chunksize=max(1, len(jobs) // (4 * workers))))
        dt = time.perf_counter() - t0
    return dt / len(jobs), out


def _timed(torch, fn, reps, warm=3):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(warm + reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out[warm:])), float(np.min(out[warm:])), float(np.max(out[warm:]))


def _timed_ab(torch, fa, fb, reps, warm=3):
    """fa and fb alternating call by call: ((median, min, max) of fa, the same of fb), ms."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = ([], [])
    for _ in range(warm + reps):
        for fn, o in zip((fa, fb), out):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            o.append(ev[0].elapsed_time(ev[1]))
    return tuple((float(np.median(o[warm:])), float(np.min(o[warm:])), float(np.max(o[warm:]))) for o in out)


def _stage_weights(rs, B):
    """Q [B, N, nx, nx], R [B, N, nu, nu]: symmetric positive definite, different for every (instance, stage)."""
    def blocks(d, w):
        M = rs.randn(B, N, d, d)
        W = 0.05 * M @ np.swapaxes(M, -1, -2)
        W[..., np.arange(d), np.arange(d)] += 1.0 + rs.rand(B, N, d)
        return w * (1.0 + 0.3 * np.arange(N))[None, :, None, None] * (1.0 + 0.1 * (np.arange(B) % 16))[:, None, None, None] * W
    return blocks(NX, 1.0), blocks(NU, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--host-batch", type=int, default=256)
    ap.add_argument("--stage-rows", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r8_ltv", "ltv_bench.json"))
    ap.add_argument("--stage-out", default=os.path.join(REPO, "profiles", "r10_ltv_stage", "ltv_stage_bench.json"),
                    help="where the stage columns go, next to the condense / update / solve columns of the same run")
    ap.add_argument("--stage-weights", action="store_true",
                    help="add the stage-weight columns: condense, vectors and the adjoint with per-(instance, stage) Q, R")
    ap.add_argument("--stage-weights-out", default=os.path.join(REPO, "profiles", "r11_ltv_stage_cost", "ltv_stage_cost_bench.json"))
    ap.add_argument("--rate", action="store_true",
                    help="add the input-rate columns: condense / vectors with a rate weight, the rate rows and bounds, the base-row copy")
    ap.add_argument("--rate-out", default=os.path.join(REPO, "profiles", "r12_ltv_rate", "ltv_rate_bench.json"))
    ap.add_argument("--rate-adjoint", action="store_true",
                    help="add the rate-adjoint columns: rqp_ltv_condense_adjoint_rate alternating with rqp_ltv_condense_adjoint")
    args = ap.parse_args()
    if not NU <= args.stage_rows <= 32:
        ap.error("--stage-rows must be in [%d, 32]: the input box takes %d rows of E, the kernels hold 32" % (NU, NU))
    B = args.batch
    Ad0, Bd0 = mpc.random_plant(NX, NU, seed=0)
    Q, R = np.eye(NX), 0.1 * np.eye(NU)
    K, P = mpc.ihlqr(Ad0, Bd0, Q, R, Q)
    rs = np.random.RandomState(1)
    Ad = Ad0[None, None] + 0.02 * rs.randn(B, N, NX, NX) / np.sqrt(NX)
    Bd = Bd0[None, None] + 0.02 * rs.randn(B, N, NX, NU)
    x0 = 1.5 * rs.randn(B, NX)
    hb = min(B, args.host_batch)
    host_s, host_out = _host_baseline(Ad[:hb], Bd[:hb], Q, R, P, K, args.workers)

    import torch
    import reluqp.reluqpth as reluqpth
    dev = torch.device("cuda:0")
    res = []
    for prec in (torch.float32, torch.float64):
        t = lambda a: torch.as_tensor(a, device=dev, dtype=prec)
        ctl = mpc.BatchedLTVMPC(NX, NU, N, Q, R, P, u_max=0.4, x_max=8.0, K=K, device=dev, precision=prec, eps_abs=1e-3)
        Adt, Bdt, xt = t(Ad), t(Bd), t(x0)
        ctl.linearize(Adt, Bdt)
        ctl.step(xt)
        buf, s = ctl._buf, ctl.solver
        out = dict(batch=B, nx=NX, nu=NU, horizon=N, n=ctl.n, m=ctl.m, dtype=str(prec).replace("torch.", ""), kernel=s.kernel,
                   reps=args.reps)
        cond = lambda: mpc.condense_ltv_device(Adt, Bdt, ctl.weights, buf["ws"], H=buf["H"], A=buf["A"])
        out["condense_ms"], out["condense_min_ms"], out["condense_max_ms"] = _timed(torch, cond, args.reps)
        out["vectors_ms"], _, _ = _timed(torch, lambda: ctl.qp_vectors(xt), args.reps)
        xr = t(0.1 * rs.randn(B, N, NX))
        out["vectors_with_xref_ms"], _, _ = _timed(torch, lambda: ctl.qp_vectors(xt, xref=xr), args.reps)
        ctl.qp_vectors(xt)
        s.synchronous = False
        out["update_mats_ms"], out["update_mats_min_ms"], out["update_mats_max_ms"] = _timed(
            torch, lambda: s.update(Hx=buf["H"], Ax=buf["A"]), args.reps)

        def warm_solve():
            s.update(g=buf["g"], l=buf["l"], u=buf["u"])
            s.solve()
        out["warm_solve_ms"], _, _ = _timed(torch, warm_solve, args.reps)
        # backward: the condensing's adjoint (the workspace holds this linearisation) and the QP adjoint of the same handle
        adj_ws = mpc.ltv_adjoint_workspace(B, NX, NU, N, dev)
        cot = dict(dH=t(rs.randn(B, ctl.n, ctl.n)), dA=t(rs.randn(B, ctl.m, ctl.n)), dg=t(rs.randn(B, ctl.n)),
                   dl=t(rs.randn(B, ctl.m)), du=t(rs.randn(B, ctl.m)))
        back = lambda: mpc.condense_ltv_adjoint_device(Adt, Bdt, xt, ctl.weights, buf["ws"], adj_ws, xref=xr, **cot)
        out["condense_adjoint_ms"], out["condense_adjoint_min_ms"], out["condense_adjoint_max_ms"] = _timed(torch, back, args.reps)
        only_x0 = lambda: mpc.condense_ltv_adjoint_device(Adt, Bdt, xt, ctl.weights, buf["ws"], adj_ws, xref=xr, want=("x0",), **cot)
        out["condense_adjoint_x0_only_ms"], _, _ = _timed(torch, only_x0, args.reps)
        if args.rate_adjoint:                  # the adjoint with the rate terms, alternating with the plain one
            Sr = _stage_weights(np.random.RandomState(3), B)[1]
            Sd = mpc.rate_weight_device(Sr, NU, N, B, dev)
            del Sr
            ws2, adj2 = mpc.ltv_workspace(B, NX, NU, N, dev), mpc.ltv_adjoint_rate_workspace(B, NX, NU, N, dev)
            H2, A2 = torch.empty_like(buf["H"]), torch.empty_like(buf["A"])
            mpc.condense_ltv_device(Adt, Bdt, ctl.weights, ws2, H=H2, A=A2, S=Sd)
            del H2, A2
            up = t(0.1 * rs.randn(B, NU))
            rcot = dict(dA_r=t(rs.randn(B, ctl.n, ctl.n)), dl_r=t(rs.randn(B, ctl.n)), du_r=t(rs.randn(B, ctl.n)))
            back_r = lambda: mpc.condense_ltv_adjoint_rate_device(Adt, Bdt, xt, ctl.weights, ws2, adj2, Sd, up, xref=xr, **cot, **rcot)
            a, b = _timed_ab(torch, back, back_r, args.reps)
            out["rate_adj_ab_plain_ms"], out["rate_adj_ab_plain_min_ms"], out["rate_adj_ab_plain_max_ms"] = a
            out["rate_adj_ab_rate_ms"], out["rate_adj_ab_rate_min_ms"], out["rate_adj_ab_rate_max_ms"] = b
            out["rate_adj_rate_minus_plain_ms"] = b[0] - a[0]
            del Sd, ws2, adj2, up, rcot
        if args.stage_weights:                 # the same three calls with per-(instance, stage) weights, alternating with the shared ones
            Qs, Rs = _stage_weights(np.random.RandomState(2), B)
            sw = mpc._LtvStageWeights(NX, NU, N, Qs, Rs, None, K)
            sw.on(dev, B)
            del Qs, Rs
            ws2 = mpc.ltv_workspace(B, NX, NU, N, dev)
            H2, A2 = torch.empty_like(buf["H"]), torch.empty_like(buf["A"])
            g2, l2, u2 = torch.empty_like(buf["g"]), torch.empty_like(buf["l"]), torch.empty_like(buf["u"])
            d5 = (NX, NU, N, True, False)
            cond_s = lambda: mpc.condense_ltv_device(Adt, Bdt, sw, ws2, H=H2, A=A2)
            vec = lambda w, ws, g, l, u: (lambda: mpc.ltv_vectors_device(d5, xt, buf["l_add"], buf["u_add"], w, ws, xref=xr, g=g, l=l, u=u))
            back_s = lambda: mpc.condense_ltv_adjoint_device(Adt, Bdt, xt, sw, ws2, adj_ws, xref=xr, **cot)
            cond_s()
            for name, fa, fb in (("condense", cond, cond_s),
                                 ("vectors_with_xref", vec(ctl.weights, buf["ws"], buf["g"], buf["l"], buf["u"]), vec(sw, ws2, g2, l2, u2)),
                                 ("condense_adjoint", back, back_s)):
                a, b = _timed_ab(torch, fa, fb, args.reps)
                out["ab_%s_shared_ms" % name], out["ab_%s_shared_min_ms" % name], out["ab_%s_shared_max_ms" % name] = a
                out["ab_%s_stage_weights_ms" % name], out["ab_%s_stage_weights_min_ms" % name], out["ab_%s_stage_weights_max_ms" % name] = b
                out["ab_%s_stage_over_shared" % name] = b[0] / a[0]
            ctl.qp_vectors(xt)                 # (the driver's g, l, u as the columns below expect them)
            del sw, ws2, H2, A2, g2, l2, u2
        if args.rate:                          # condense / vectors with a rate weight, alternating with the plain calls
            Sr = _stage_weights(np.random.RandomState(3), B)[1]
            Sd = mpc.rate_weight_device(Sr, NU, N, B, dev)
            del Sr
            ws2 = mpc.ltv_workspace(B, NX, NU, N, dev)
            H2, A2 = torch.empty_like(buf["H"]), torch.empty_like(buf["A"])
            g2, l2, u2 = torch.empty_like(buf["g"]), torch.empty_like(buf["l"]), torch.empty_like(buf["u"])
            up = t(0.1 * rs.randn(B, NU))
            d5, d4r = (NX, NU, N, True, False), (B, NX, NU, N)
            cond_r = lambda: mpc.condense_ltv_device(Adt, Bdt, ctl.weights, ws2, H=H2, A=A2, S=Sd)
            vec_p = lambda: mpc.ltv_vectors_device(d5, xt, buf["l_add"], buf["u_add"], ctl.weights, buf["ws"], g=buf["g"], l=buf["l"],
                                                   u=buf["u"])
            vec_r = lambda: mpc.ltv_vectors_device(d5, xt, buf["l_add"], buf["u_add"], ctl.weights, ws2, g=g2, l=l2, u=u2, S=Sd, uprev=up)
            cond_r()
            for name, fa, fb in (("condense", cond, cond_r), ("vectors", vec_p, vec_r)):
                a, b = _timed_ab(torch, fa, fb, args.reps)
                out["rate_ab_%s_plain_ms" % name], out["rate_ab_%s_plain_min_ms" % name], out["rate_ab_%s_plain_max_ms" % name] = a
                out["rate_ab_%s_rate_ms" % name], out["rate_ab_%s_rate_min_ms" % name], out["rate_ab_%s_rate_max_ms" % name] = b
                out["rate_ab_%s_rate_minus_plain_ms" % name] = b[0] - a[0]
            # k_rate_w moves the u rows of W (read, write) and of F (read): 3 x 8 N nu n bytes per instance
            out["rate_w_bytes_estimate"] = 3 * 8 * N * NU * ctl.n * B
            mt, nr = ctl.m + ctl.n, ctl.n
            At = torch.empty(B, mt, ctl.n, dtype=prec, device=dev)
            lt, ut = torch.empty(B, mt, dtype=prec, device=dev), torch.empty(B, mt, dtype=prec, device=dev)
            dl = t(np.full(nr, 0.2))
            out["rate_rows_ms"], out["rate_rows_min_ms"], out["rate_rows_max_ms"] = _timed(
                torch, lambda: mpc.rate_rows_device(d4r, buf["ws"], prec, A_r=At, row0=ctl.m), args.reps)
            out["rate_bounds_ms"], out["rate_bounds_min_ms"], out["rate_bounds_max_ms"] = _timed(
                torch, lambda: mpc.rate_bounds_device(d4r, xt, up, -dl, dl, buf["ws"], l_r=lt, u_r=ut, row0=ctl.m), args.reps)
            out["rate_base_row_copy_ms"], out["rate_base_row_copy_min_ms"], out["rate_base_row_copy_max_ms"] = _timed(
                torch, lambda: At[:, :ctl.m].copy_(buf["A"]), args.reps)
            out["rate_base_row_copy_bytes"] = 2 * B * ctl.m * ctl.n * At.element_size()
            ctl.qp_vectors(xt)
            del Sd, ws2, H2, A2, g2, l2, u2, At, lt, ut
        # (a second handle on the same data: the columns above stay those of a handle without the adjoint's workspace)
        sd = reluqpth.ReLU_QP()
        sd.setup(buf["H"], buf["g"], buf["A"], buf["l"], buf["u"], device=dev, precision=prec, eps_abs=1e-3, differentiable=True)
        sd.solve()
        sd.synchronous = False
        dx = t(rs.randn(B, ctl.n))
        out["qp_adjoint_ms"], _, _ = _timed(torch, lambda: sd.adjoint(dx), args.reps)
        del sd
        out["condense_adjoint_over_condense"] = out["condense_adjoint_ms"] / out["condense_ms"]
        # stage constraints on the same workspace: nc rows per stage, the input box as rows of E plus half-planes on the state
        nc, blk = args.stage_rows, NX + NU
        Eh = np.zeros((B, N, nc, blk))
        Eh[:, :, :NU, :NU] = np.eye(NU)
        Eh[:, :, NU:, NU:] = rs.randn(B, N, nc - NU, NX) / np.sqrt(NX)
        lo_h = np.tile(np.hstack([np.full(NU, -0.4), np.full(nc - NU, -8.0)]), N)
        Et, lot, hit = t(Eh), t(lo_h), t(-lo_h)
        d4 = (B, NX, NU, N)
        sb = dict(A_c=torch.empty(B, N * nc, ctl.n, dtype=prec, device=dev), l_c=torch.empty(B, N * nc, dtype=prec, device=dev),
                  u_c=torch.empty(B, N * nc, dtype=prec, device=dev))
        out["stage_rows"], out["m_c"] = nc, N * nc
        out["stage_rows_ms"], out["stage_rows_min_ms"], out["stage_rows_max_ms"] = _timed(
            torch, lambda: mpc.stage_rows_device(d4, Et, buf["ws"], A_c=sb["A_c"]), args.reps)
        out["stage_vectors_ms"], _, _ = _timed(
            torch, lambda: mpc.stage_vectors_device(d4, Et, xt, lot, hit, buf["ws"], l_c=sb["l_c"], u_c=sb["u_c"]), args.reps)
        scot = [t(rs.randn(B, N * nc, ctl.n)), t(rs.randn(B, N * nc)), t(rs.randn(B, N * nc))]
        sout = {k: torch.empty(sh, dtype=prec, device=dev) for k, sh in
                (("dA_full", (B, ctl.m, ctl.n)), ("dl_full", (B, ctl.m)), ("dE", (B, N, nc, blk)))}
        out["stage_adjoint_ms"], out["stage_adjoint_min_ms"], out["stage_adjoint_max_ms"] = _timed(
            torch, lambda: mpc.stage_adjoint_device(d4, Et, xt, buf["ws"], *scot, out=sout), args.reps)
        out["stage_rows_over_condense"] = out["stage_rows_ms"] / out["condense_ms"]
        del scot, sout, sb
        sctl = mpc.BatchedLTVMPC(NX, NU, N, Q, R, P, K=K, stage_rows=nc, device=dev, precision=prec, eps_abs=1e-3)
        sctl.linearize(Adt, Bdt, E=Et)
        sctl.step(xt, lo=lot, hi=hit)
        ss, sbuf = sctl.solver, sctl._buf
        out["stage_kernel"] = ss.kernel
        ss.synchronous = False
        out["stage_update_mats_ms"], _, _ = _timed(torch, lambda: ss.update(Hx=sbuf["H"], Ax=sbuf["A"]), args.reps)
        sctl.qp_vectors(xt)

        def stage_warm_solve():
            ss.update(g=sbuf["g"], l=sbuf["l"], u=sbuf["u"])
            ss.solve()
        out["stage_warm_solve_ms"], _, _ = _timed(torch, stage_warm_solve, args.reps)
        if args.rate:                          # the same handle with N nu rate rows behind the stage rows
            rctl = mpc.BatchedLTVMPC(NX, NU, N, Q, R, P, K=K, stage_rows=nc, du_max=0.2, rate_weight=0.05 * np.eye(NU), device=dev,
                                     precision=prec, eps_abs=1e-3)
            rctl.linearize(Adt, Bdt, E=Et)
            rctl.step(xt, lo=lot, hi=hit, u_prev=t(np.zeros((B, NU))))
            rs_, rbuf = rctl.solver, rctl._buf
            out["rate_m"], out["rate_kernel"] = rctl.m, rs_.kernel
            rs_.synchronous = False
            out["rate_update_mats_ms"], _, _ = _timed(torch, lambda: rs_.update(Hx=rbuf["H"], Ax=rbuf["A"]), args.reps)
            rctl.qp_vectors(xt)

            def rate_warm_solve():
                rs_.update(g=rbuf["g"], l=rbuf["l"], u=rbuf["u"])
                rs_.solve()
            out["rate_warm_solve_ms"], _, _ = _timed(torch, rate_warm_solve, args.reps)
            del rctl, rs_, rbuf
        del sctl, ss, sbuf, Et
        del adj_ws, cot
        torch.cuda.synchronize()
        out["condense_over_update_mats"] = out["condense_ms"] / out["update_mats_ms"]
        # the host path: numpy over the batch (scaled from --host-batch instances) + the copy of its (H, A) to the device
        Hh = torch.as_tensor(np.stack([o[0] for o in host_out])).to(prec).pin_memory()
        Ah = torch.as_tensor(np.stack([o[1] for o in host_out])).to(prec).pin_memory()
        h2d, _, _ = _timed(torch, lambda: (Hh.to(dev, non_blocking=True), Ah.to(dev, non_blocking=True)), 5)
        out["host_numpy_ms"] = host_s * B * 1e3
        out["host_h2d_ms"] = h2d * B / hb
        out["host_workers"], out["host_batch_timed"] = args.workers, hb
        out["host_over_condense"] = (out["host_numpy_ms"] + out["host_h2d_ms"]) / out["condense_ms"]
        print(json.dumps(out), flush=True)
        res.append(out)
        del ctl, s, buf
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=res), f, indent=1)
    # the stage figures with what they are read against, in a file of their own
    keep = ("batch", "nx", "nu", "horizon", "n", "m", "dtype", "kernel", "reps", "condense_ms", "condense_min_ms", "condense_max_ms",
            "vectors_ms", "update_mats_ms", "warm_solve_ms", "condense_adjoint_ms")
    stage = [{k: v for k, v in r.items() if k in keep or k.startswith("stage_") or k == "m_c"} for r in res]
    os.makedirs(os.path.dirname(args.stage_out), exist_ok=True)
    with open(args.stage_out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=stage), f, indent=1)
    if args.rate:
        rt = [{k: v for k, v in r.items() if k in keep or k.startswith("rate_") or k in ("stage_update_mats_ms", "stage_warm_solve_ms",
                                                                                        "m_c", "stage_rows_ms")} for r in res]
        os.makedirs(os.path.dirname(args.rate_out), exist_ok=True)
        with open(args.rate_out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=rt), f, indent=1)
    if args.stage_weights:
        sw = [{k: v for k, v in r.items() if k in keep or k.startswith("ab_")} for r in res]
        os.makedirs(os.path.dirname(args.stage_weights_out), exist_ok=True)
        with open(args.stage_weights_out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=sw), f, indent=1)


if __name__ == "__main__":
    main()
