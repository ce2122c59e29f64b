#!/usr/bin/env python3
"""bench.py -- QP solves/sec of the MI355X ReLU-QP hot path (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 4
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one batched cold-start solve() of the per-GPU batch (default: 4096 random
dense QPs, n=100, m=300, float32, feasible rand_qp generator of SURVEY.md 8(d), eps_abs
1e-3, all reference defaults), inputs and the K(rho) table already resident in HBM.
The timed steps rotate through --fresh-batches DISTINCT batches (one handle each) with the
dispatch history switched off, so `value` is the rate of a batch the solver has never seen
(grid-order launch, like the first solve() of a fresh handle).  The rate of re-solving ONE
batch with the longest-first order learnt from its previous solve is reported separately as
`value_with_history` (a second timed leg after the contract's K steps).
Instances are independent: each rank owns its own shard, there is NO data-path collective;
torch.distributed is used only for the barrier around the timed region and for the
max-over-ranks / sum reductions of the reported numbers.

  --scaling weak    (default) every rank solves --batch instances: the job grows with N
  --scaling strong  --batch is the GLOBAL batch, split contiguously over the ranks (D.shard_range)
  --workload random_qp | mpc (BASELINE config 3) | c4 (BASELINE config 4: n=32, m=64, 8192 per GPU = 65536 on 8 GPUs)

Rank 0 prints ONE JSON line.  `value` = all QPs solved by all ranks / max-over-ranks time.
`roofline` prices the ADMM kernel against the roof that BINDS it:
  resident2 / wave : "valu" -- matrices live in registers, HBM is out of the picture; algorithmic flops
                     (2n^2 + 4mn per instance-iteration) / kernel time / 157.3 TF fp32 vector peak
  mfma             : "mfma" -- the same flops against the 157.3 TF fp32 matrix peak (mfma16: against the 2.5 PF dense bf16 peak)
  generic          : "hbm"  -- algorithmic bytes 4(n^2 + mn) per instance-iteration / kernel time / 8 TB/s
`hbm_algorithmic_x` keeps the streaming-model GB/s figure (may exceed the HBM peak for the resident kernels: the
matrices are not re-read).  `cpu_baseline` times the oracle on the host cores in child processes started BEFORE this
process touches the GPU.

A plain run only sets up, warms up, times the --steps steps and prints the line (`value`, `ms_per_step`, ...).
`--full` adds the legs the headline does not need: `cpu_baseline`, `value_with_history` and `roofline`.
`--dump-outputs DIR` writes the Results of the last timed step as DIR/<name>.npy; the inputs are seeded, so two
builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (REPO, os.path.join(REPO, "reluqp-py_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s spec
FP32_VALU_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: vector fp32 peak
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_*_f32 (f32 in / f32 acc) dense peak
FP64_VALU_PEAK_TFLOPS = 78.6   # MI355X_MICROARCH.md: vector fp64 peak
FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X spec: fp64 matrix (v_mfma_f64_16x16x4_f64) = the vector fp64 rate on this part
BF16_MFMA_PEAK_TFLOPS = 2500.0 # MI355X_MICROARCH.md: dense bf16 / fp16 MFMA peak (the sparsity figure is twice that: never priced against)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)     # (one per fresh batch: every handle has solved once before the timed steps)
    ap.add_argument("--batch", type=int, default=None, help="instances per GPU (weak) / in total (strong); default 4096 "
                                                             "(c4: 8192 weak, 65536 strong)")
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--n-eq", type=int, default=25)
    ap.add_argument("--n-ineq", type=int, default=275)
    ap.add_argument("--eps-abs", type=float, default=1e-3)
    ap.add_argument("--precision", choices=["f32", "f64"], default="f32")
    ap.add_argument("--cpu-seconds", type=float, default=24.0, help="--full: budget of the cpu_baseline leg, split over its modes (0 = skip)")
    ap.add_argument("--seed0", type=int, default=0)
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--kernel", default="auto", help="C-ABI kernel request (auto | generic | resident | wave | mfma)")
    ap.add_argument("--tile", choices=["same", "f16", "bf16"], default="same", help="f16: fp16 K(rho) tile of the resident kernel; "
                    "bf16: shared-matrix batches on the 16-bit matrix pipe (two bf16 planes per operand; BASELINE config 5)")
    ap.add_argument("--low-memory", action="store_true", help="setup(low_memory=True): no packed copy of K(rho) (less workspace "
                    "and setup time, ~1 %% more solve time; not the default)")
    ap.add_argument("--workload", choices=["random_qp", "mpc", "c4"], default="random_qp",
                    help="random_qp: the headline metric's workload (default); mpc: BASELINE config 3, batch of condensed "
                         "linear-MPC QPs (horizon 20, nx=12, nu=4 -> n=80, m=320) sharing H and A; c4: BASELINE config 4, "
                         "random dense QPs n=32, m=64")
    ap.add_argument("--mpc-form", choices=["condensed", "sparse"], default="condensed",
                    help="workload mpc: condensed (n=80, m=320; BASELINE config 3 as quoted) or the reference's own sparse form "
                         "(loose_code/RandomLinMPC.py:54-66: n=320, m=560, 2.4 %% of A non-zero; streamed-operand MFMA kernel)")
    ap.add_argument("--full-ladder", action="store_true", help="setup(full_ladder=True): K(rho) for all 18 ladder entries of every "
                    "matrix as the reference builds them (default: a window of 5 with exact continuation)")
    ap.add_argument("--fresh-batches", type=int, default=4, help="distinct synthetic batches (one handle each) the timed steps "
                    "rotate through; every solve runs without dispatch history")
    ap.add_argument("--history-steps", type=int, default=5, help="--full: steps of the separately reported with-history leg (0 = skip)")
    ap.add_argument("--full", action="store_true", help="also run what the headline does not need: the cpu_baseline leg, the "
                    "with-history leg and the roofline figures (default: set up, warm up, time --steps, print the result line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the Results of the last "
                    "timed solve() as DIR/<name>.npy (float32/float64; a fixed sample of instances beyond 64 MB)")
    ap.add_argument("--cpu-worker", default=None, help=argparse.SUPPRESS)     # internal: child process of the cpu_baseline leg
    a = ap.parse_args()
    if a.workload == "c4":
        a.n, a.n_eq, a.n_ineq = 32, 8, 56
        if a.batch is None:
            a.batch = 65536 if a.scaling == "strong" else 8192
    if a.batch is None:
        a.batch = 4096
    return a


# ------------------------------------------------------------------------------------------------ cpu_baseline leg
def _mpc_controller(form="condensed"):
    from reluqp import mpc
    Adyn, Bdyn = mpc.random_plant(12, 4, seed=0)                      # one plant, the batch is the initial states
    return mpc.LinearMPC(Adyn, Bdyn, np.eye(12), 0.1 * np.eye(4), 20, 0.5, 10.0, form=form)


def _nz_blocks(M, bs=16):
    """Number of non-zero bs x bs blocks of a matrix (zero padded to multiples of bs)."""
    r, c = M.shape
    P = np.zeros(((r + bs - 1) // bs * bs, (c + bs - 1) // bs * bs))
    P[:r, :c] = M != 0
    return int((P.reshape(P.shape[0] // bs, bs, P.shape[1] // bs, bs).sum(axis=(1, 3)) != 0).sum())


def cpu_worker(args):
    """Child process of the cpu_baseline leg: never imports torch / touches the GPU.  Spec "form:dtype:rank:P:budget".
    Solves instances rank, rank+P, ... of the bench batch with the oracle until the budget is spent; prints one JSON."""
    form, dtype, rank, P, budget = args.cpu_worker.split(":")
    rank, P, budget = int(rank), int(P), float(budget)
    from oracle import reluqp_oracle as O
    from reluqp import utils
    dt = np.float32 if dtype == "f32" else np.float64
    ctl = x0 = None
    if args.workload == "mpc":
        ctl = _mpc_controller(args.mpc_form)
        x0 = np.random.RandomState(args.seed0 + 1).randn(args.batch, 12)
    t_setup = t_solve = 0.0
    iters = done = 0
    idx = rank
    t0 = time.perf_counter()
    while idx < args.batch and (time.perf_counter() - t0) < budget:
        if ctl is not None:
            g, l, u = ctl.qp_vectors(x0[idx:idx + 1])
            H, A, g, l, u = ctl.H, ctl.A, g[0], l[0], u[0]
        else:
            H, g, A, l, u, _ = utils.rand_qp(args.n, args.n_eq, args.n_ineq, seed=args.seed0 + idx, compute_sol=False,
                                             feasible=True)
        qp = O.OracleQP(form=form, quirks=False)
        qp.setup(H, g, A, l, u, eps_abs=args.eps_abs, dtype=dt)
        r = qp.solve()
        t_setup += qp.info.setup_time
        t_solve += r.info.run_time
        iters += r.info.iter
        done += 1
        idx += P
    print(json.dumps({"done": done, "t_solve": t_solve, "t_setup": t_setup, "iters": iters}))


def _run_cpu_mode(args, form, dtype, procs, threads, budget):
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(threads)
    base = [sys.executable, os.path.abspath(__file__), "--workload", args.workload, "--batch", str(args.batch), "--n", str(args.n),
            "--n-eq", str(args.n_eq), "--n-ineq", str(args.n_ineq), "--eps-abs", str(args.eps_abs), "--seed0", str(args.seed0),
            "--mpc-form", args.mpc_form]
    ps = [subprocess.Popen(base + ["--cpu-worker", "%s:%s:%d:%d:%g" % (form, dtype, r, procs, budget)], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(procs)]
    outs = []
    for p in ps:
        so, se = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("cpu_baseline worker failed: " + se[-400:])
        outs.append(json.loads(so.strip().splitlines()[-1]))
    done = sum(o["done"] for o in outs)
    # all workers are busy for the whole budget, so the job's rate is the sum of the per-worker rates
    qps = sum(o["done"] / o["t_solve"] for o in outs if o["t_solve"] > 0)
    qps_setup = sum(o["done"] / (o["t_solve"] + o["t_setup"]) for o in outs if o["t_solve"] > 0)
    its = sum(o["iters"] / o["t_solve"] for o in outs if o["t_solve"] > 0)
    return {"form": form, "dtype": dtype, "processes": procs, "threads_per_process": threads, "cores": procs * threads,
            "instances": done, "value": qps, "setup_plus_solve_value": qps_setup, "admm_iters_per_sec": its}


def cpu_baseline(args):
    """SURVEY.md 8(d) / BASELINE.md section 3: the oracle (kind "port"; the reference's Python cannot travel) on the host
    cores, on the first instances of the same workload, three modes of budget/3 seconds each:
      (i)   W form float64, 1 process x 8 BLAS threads  -- how the reference would run (the 700^2 matvec does not scale
            past ~8 threads: tools/cpu_baseline_threads.py)
      (ii)  W form float64, P processes x 1 thread, instances sharded -- best-case throughput of the reference formulation
      (iii) factored float32 ("refine" statement, what the GPU kernels execute), P x 1 thread -- the stronger baseline, so
            that the GPU/CPU ratio is not inflated by the W form's 7x extra flops
    `value` = the best reference-faithful (W form) mode; P = min(available cores, 16) (the GPU box's CPU share)."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    P = max(1, min(avail, 16))
    per = args.cpu_seconds / 3.0
    modes = [_run_cpu_mode(args, "W", "f64", 1, min(8, avail), per),
             _run_cpu_mode(args, "W", "f64", P, 1, per),
             _run_cpu_mode(args, "refine", "f32", P, 1, per)]
    best = max(modes[:2], key=lambda mo: mo["value"])
    return {
        "value": best["value"], "unit": "QP/s", "cores": best["cores"], "kind": "port",
        "sample": "oracle W form (reference-faithful dense (n+2m)^2 matvec per iteration) float64 on the first %d instances "
                  "of the same workload, %d process(es) x %d thread(s), %.0f s; solve-only (setup amortised like `value`); "
                  "host has %d cores available" % (best["instances"], best["processes"], best["threads_per_process"], per, avail),
        "setup_plus_solve_value": best["setup_plus_solve_value"], "admm_iters_per_sec": best["admm_iters_per_sec"],
        "modes": modes,
        "factored_f32_value": modes[2]["value"],
    }


# ------------------------------------------------------------------------------------------------ PMC traffic
def pmc_traffic(kernel, args, kern_s):
    """HBM traffic of the dominant kernel in GB/s from the PMC passes committed under profiles/ for THIS round's build
    (counters cannot be read from inside this process; the passes are separate `rocprofv3 --pmc FETCH_SIZE` /
    `--pmc WRITE_SIZE` runs of this same command, tools/pmc_collect.sh).  KB units, FETCH_SIZE doubled on gfx950
    (MI355X_MICROARCH.md).  None when no profile of this kernel on this workload is committed."""
    sig = (args.workload if args.mpc_form == "condensed" else "mpc_sparse", args.batch, args.n, args.n_eq, args.n_ineq, args.precision, args.tile)
    table = {
        ("resident2", ("random_qp", 4096, 100, 25, 275, "f32", "same")): "r3_resident2/pmc.json",
        ("mfma", ("mpc", 4096, 100, 25, 275, "f32", "same")): "r3_mfma/pmc.json",
        ("mfma16", ("mpc", 4096, 100, 25, 275, "f32", "bf16")): "r3_mfma16/pmc.json",
        ("mfmal", ("mpc_sparse", 4096, 100, 25, 275, "f32", "same")): "r3_mfmal/pmc.json",
        ("wave", ("c4", 8192, 32, 8, 56, "f32", "same")): "r3_wave/pmc.json",
    }
    name = table.get((kernel, sig))
    if name is None:
        return None, None
    path = os.path.join(REPO, "profiles", name)
    try:
        with open(path) as f:
            pm = json.load(f)
        nbytes = (2.0 * float(pm["FETCH_SIZE"]) + float(pm["WRITE_SIZE"])) * 1024.0
        if kernel == "mfmal":          # a cold solve of this kernel is two launches (regrouped at the first check): pmc.json is per launch
            nbytes *= 2.0
    except (OSError, KeyError, ValueError):
        return None, None
    return nbytes / kern_s / 1e9, "profiles/" + name + " (bytes per launch / this run's kernel time)"


def roofline(kernel, args, n, m, esz, blocks, rank_iters_max, kern_avg_s, cold_ms):
    """--full: the ADMM kernel priced against the roof that binds it (module docstring)."""
    # algorithmic work per launch (one rank's launch: the slowest rank's time against the largest rank's work): SURVEY.md 8(d)
    b_iter = esz * (n * n + m * n)
    f_iter = 2 * n * n + 4 * m * n
    alg_bytes = rank_iters_max * b_iter
    alg_flops = rank_iters_max * f_iter
    hbm_gbs = alg_bytes / kern_avg_s / 1e9
    tf = alg_flops / kern_avg_s / 1e12
    traffic, traffic_src = pmc_traffic(kernel, args, kern_avg_s)
    kname = "k_admm_%s" % {"resident2": "res2", "resident64": "res64"}.get(kernel, kernel)
    if kernel == "mfma":
        roof = {"bound": "mfma", "achieved": tf, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / FP32_MFMA_PEAK_TFLOPS,
                "note": "dense algorithmic flops 2n^2+4mn per instance-iteration; the kernel skips all-zero operand groups of the "
                        "block-triangular MPC matrices, so it executes fewer"}
    elif kernel in ("mfmal", "mfmad"):
        # streamed-operand MFMA kernel: the work is the NON-ZERO 16 x 16 blocks of A (twice: A' nu and A dx) and H plus the
        # dense K -- 512 flops per block and instance-iteration (every block is 4 v_mfma_f32_16x16x4_f32 over 16 instances)
        bl = 2 * blocks[0] + blocks[1] + blocks[2]
        tfb = rank_iters_max * bl * 512.0 / kern_avg_s / 1e12
        mpeak = FP32_MFMA_PEAK_TFLOPS if kernel == "mfmal" else FP64_MFMA_PEAK_TFLOPS
        roof = {"bound": "mfma", "achieved": tfb, "peak": mpeak, "unit": "TFLOP/s", "frac": tfb / mpeak,
                "note": "block-sparse algorithmic flops: 512 per non-zero 16x16 block of A (x2), H and the dense K = %d blocks per "
                        "instance-iteration (the dense count 2n^2+4mn would be %.1fx that); operands stream from L2, "
                        "%d KB per block and 16 instances" % (bl, f_iter / (bl * 512.0), esz // 4),
                "blocks_per_iteration": bl, "l2_operand_gbs": rank_iters_max / 16.0 * bl * 256.0 * esz / kern_avg_s / 1e9}
    elif kernel == "mfma16":
        # three bf16 MFMAs per product term pair: the executed matrix flops are 3x the algorithmic ones; priced in ALGORITHMIC
        # flops against the dense bf16 matrix peak (the kernel is bound by its VALU / LDS phases, not by this roof)
        roof = {"bound": "mfma", "achieved": tf, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / BF16_MFMA_PEAK_TFLOPS,
                "note": "algorithmic flops 2n^2+4mn per instance-iteration against the dense bf16 MFMA peak; operands are two bf16 "
                        "planes and a product is three v_mfma_f32_16x16x32_bf16 (executed matrix flops = 3x + padding); the "
                        "kernel's time is VALU / LDS latency of its row and column phases (DESIGN.md section 4)",
                "frac_of_fp32_mfma_peak": tf / FP32_MFMA_PEAK_TFLOPS}
    elif kernel == "generic":
        roof = {"bound": "hbm", "achieved": hbm_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hbm_gbs / HBM_PEAK_GBS}
    else:
        peak = FP32_VALU_PEAK_TFLOPS if args.precision == "f32" else FP64_VALU_PEAK_TFLOPS
        roof = {"bound": "valu", "achieved": tf, "peak": peak, "unit": "TFLOP/s", "frac": tf / peak,
                "note": "A and K live in registers for the whole solve; the binding roof is %s vector FMA issue.  `traffic` "
                        "(HBM, PMC) is ~2.5x the compulsory bytes of a launch (the padded lane-linear A / K / H images are "
                        "larger than the matrices, and K is re-read at every rho move) and still < 10 %% of the HBM peak: "
                        "irrelevant to the bound" % args.precision}
    roof.update({"traffic": traffic, "traffic_unit": "GB/s (HBM, PMC)", "traffic_source": traffic_src,
                 "kernel": kname, "kernel_ms": kern_avg_s * 1e3,
                 "algorithmic_flops_per_launch": alg_flops, "algorithmic_bytes_per_launch": alg_bytes,
                 "hbm_algorithmic_gbs": hbm_gbs, "hbm_algorithmic_x": hbm_gbs / HBM_PEAK_GBS})
    if cold_ms is not None:
        roof["kernel_ms_cold_process"] = cold_ms      # the very first launch of the process (code-object load included)
    return roof


# ------------------------------------------------------------------------------------------------ --dump-outputs
DUMP_CAP_BYTES = 64 << 20


def dump_outputs(res, outdir, suffix="", cap=DUMP_CAP_BYTES):
    """Write what a caller of the timed solve() receives -- the batched Results: x, z, y and the per-instance info
    tensors -- as outdir/<name><suffix>.npy.  Floating arrays keep their dtype (float32 / float64), integer ones
    (iter, status_code, rho_ind) become float64 (exact).  Every array has one row per instance; when all of them
    together exceed `cap` bytes, the same seeded sample of rows is kept in each and `instance_index` lists it."""
    info = res.info
    named = {"x": res.x, "z": res.z, "y": res.y, "iter": info.iter, "status_code": info.status_code,
             "rho_ind": info.rho_ind, "obj_val": info.obj_val, "pri_res": info.pri_res, "dua_res": info.dua_res,
             "rho_estimate": info.rho_estimate}
    host = {}
    for k, t in named.items():
        a = t.detach().cpu().numpy()
        host[k] = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
    rows = host["x"].shape[0]
    row_bytes = sum(a.nbytes for a in host.values()) // rows
    if rows * row_bytes > cap:
        keep = cap // (row_bytes + 8)
        idx = np.sort(np.random.RandomState(0).choice(rows, keep, replace=False))
        host = {k: a[idx] for k, a in host.items()}
        host["instance_index"] = idx.astype(np.float64)
    os.makedirs(outdir, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(outdir, k + suffix + ".npy"), np.ascontiguousarray(a))
    return sorted(host)


def main():
    args = parse()
    if args.cpu_worker:
        cpu_worker(args)
        return
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    rank_env = int(os.environ.get("RANK", "0"))
    cpu = None
    if args.full and world_env == 1 and args.cpu_seconds > 0:
        cpu = cpu_baseline(args)          # child processes, finished before this process initialises the GPU

    # ---- synthetic inputs: `nb` DISTINCT batches per rank, drawn before the GPU is touched (the generator forks workers).
    # Step i solves batch i % nb on a handle whose dispatch history is off: every timed solve is the first sight of its
    # batch for the scheduler -- grid order, exactly like the first solve() of a fresh handle -- and consecutive steps
    # solve different problems.  (Round-2 VERDICT: a rate that needs the iteration counts of a previous solve of the same
    # problems is not the metric "solves/sec of a batch of random QPs"; that rate is reported as `value_with_history`.)
    n, m = args.n, args.n_eq + args.n_ineq
    nb = max(1, min(args.fresh_batches, args.steps + args.warmup))
    if args.scaling == "weak":      # the job is world*batch instances per step; rank r owns the contiguous shard [r*B, (r+1)*B)
        total = world_env * args.batch
    else:                           # the job is `batch` instances in total, split contiguously
        total = args.batch
    base_, rem_ = divmod(total, world_env)            # = reluqp.distributed.shard_range (that module imports torch: the
    start, B = rank_env * base_ + min(rank_env, rem_), base_ + (1 if rank_env < rem_ else 0)     # generator forks first)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    gen_workers = max(1, min(16, avail // max(1, min(world_env, 8))))
    from reluqp import utils
    np_dt = np.float32 if args.precision == "f32" else np.float64
    batches = []
    t_gen = time.perf_counter()
    blocks = None
    if args.workload == "mpc":
        ctl = _mpc_controller(args.mpc_form)
        n, m = ctl.H.shape[0], ctl.A.shape[0]
        blocks = (_nz_blocks(ctl.A), _nz_blocks(ctl.H), ((n + 15) // 16) ** 2)      # (A, H, K) 16 x 16 blocks
        for i in range(nb):           # one plant; a batch is a set of initial states (H, A shared and un-batched)
            x0 = np.random.RandomState(args.seed0 + 1 + i).randn(start + B, 12)[start:]
            g, l, u = ctl.qp_vectors(x0)
            batches.append((ctl.H, g, ctl.A, l, u))
    else:
        for i in range(nb):
            H, g, A, l, u, _ = utils.rand_qp_batch(B, n, args.n_eq, args.n_ineq, seed0=args.seed0 + i * total + start,
                                                   feasible=True, dtype=np_dt, workers=gen_workers)
            batches.append((H, g, A, l, u))
    t_gen = time.perf_counter() - t_gen

    import torch
    from reluqp import distributed as D
    rank, world, local_rank, dist = D.init()          # nccl (= RCCL) when WORLD_SIZE > 1; barrier/reductions only
    assert torch.cuda.is_available(), "bench.py needs an MI355X; there is no CPU path"
    dev = D.local_device(local_rank)
    torch.cuda.set_device(dev)

    import reluqp.reluqpth as reluqpth

    prec = torch.float32 if args.precision == "f32" else torch.float64
    esz = 4 if args.precision == "f32" else 8
    # inputs resident in HBM in the working dtype before anything is timed (host->device of 655 MB per batch is data loading)
    models, setup_times = [], []
    for (H, g, A, l, u) in batches:
        Hd, gd, Ad, ld, ud = (torch.from_numpy(np.ascontiguousarray(t)).to(device=dev, dtype=prec) for t in (H, g, A, l, u))
        torch.cuda.synchronize(dev)
        model = reluqpth.ReLU_QP()
        t0 = time.perf_counter()
        model.setup(Hd, gd, Ad, ld, ud, device=dev, precision=prec, eps_abs=args.eps_abs, warm_starting=False, kernel=args.kernel,
                    iterate_dtype={"f16": torch.float16, "bf16": torch.bfloat16}.get(args.tile), low_memory=args.low_memory,
                    full_ladder=args.full_ladder)
        torch.cuda.synchronize(dev)
        setup_times.append(time.perf_counter() - t0)
        model.dispatch_history(False)
        models.append(model)
        del Hd, Ad                                     # the handle keeps its own packed copies
    batches = None
    setup_s = min(setup_times[1:]) if len(setup_times) > 1 else setup_times[0]     # (the first setup of a process also loads the code objects)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    cold_ms = None
    for w in range(args.warmup):
        models[w % nb].solve()
        if w == 0:
            cold_ms = models[0].last_kernel_time * 1e3   # first launch of the PROCESS: code-object load on top of the solve
    # host-side pools the timed steps draw from, for the handles the warm-up did not reach (W < number of fresh batches): the
    # caching allocator gets one block set per handle (each handle keeps its last results alive) and every handle its event
    # pair -- a first hipMalloc / event creation inside the timed region is not part of a solve.  No solver work is done here.
    pool = []
    for mdl in models:
        mdl._events()
        pool.append((torch.empty(B * (n + 2 * m), device=dev, dtype=prec), torch.empty(3, B, device=dev, dtype=torch.int32),
                     torch.empty(4, B, device=dev, dtype=torch.float64)))
    del pool
    barrier()
    t0 = time.perf_counter()
    kern_s = 0.0
    outs = []
    for i in range(args.steps):
        mdl = models[(args.warmup + i) % nb]
        res = mdl.solve()             # cold start every step (warm_starting=False clears the state), no dispatch history
        kern_s += mdl.last_kernel_time
        outs.append((res.info.iter, res.info.status_code))
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:             # before the with-history leg, whose solves may overwrite the Results object `res`
        dump_outputs(res, args.dump_outputs, "" if world_env == 1 else "_rank%d" % rank_env)

    sum_iters = float(sum(float(it.to(torch.float64).sum()) for it, _ in outs)) / max(1, args.steps)     # per step
    solved = float(sum(float((sc == 0).sum()) for _, sc in outs)) / max(1, args.steps)

    # ---- second, separately reported leg: the SAME batch solved again and again with the longest-first dispatch order
    # learnt from the previous solve (closed loops, parameter sweeps); not `value`
    hist = None
    if args.full and args.history_steps > 0:
        mdl = models[0]
        mdl.dispatch_history(True)
        for _ in range(2):
            mdl.solve()
        barrier()
        th = time.perf_counter()
        kh = 0.0
        for _ in range(args.history_steps):
            rh = mdl.solve()
            kh += mdl.last_kernel_time
        barrier()
        th = time.perf_counter() - th
        hist = (th / args.history_steps, kh / args.history_steps, float(rh.info.iter.to(torch.float64).sum()))
        mdl.dispatch_history(False)

    # (the minima over the ranks ride along as maxima of the negated values: SURVEY.md 8(e) asks for the min / max per-GPU time)
    elapsed_rank = elapsed
    elapsed, (kern_avg_s, setup_max, rank_iters_max, hist_step, hist_kern, hist_iters, neg_kern_min, neg_el_min, neg_it_min), \
        tot_iters, tot_solved, tot_qps = D.reduce_report(
            dist, dev, elapsed, sum_iters, solved, B,
            extra_max=[kern_s / max(1, args.steps), setup_s, sum_iters] + (list(hist) if hist else [0.0, 0.0, 0.0]) +
                      [-kern_s / max(1, args.steps), -elapsed_rank, -sum_iters])

    if rank == 0:
        step_s = elapsed / args.steps
        value = tot_qps / step_s
        kernel = models[0].kernel
        per = "/GPU" if args.scaling == "weak" else " total"
        fresh = ("%d distinct batches in rotation, every solve without dispatch history (= first solve of a fresh handle)" % nb)
        if args.workload == "mpc":
            wl = ("batch=%d%s %s linear-MPC QPs (horizon 20, nx=12, nu=4: n=%d, m=%d), H and A shared by the "
                  "batch, random initial states seeds %d.., eps_abs=%g, cold start, reference defaults; %s"
                  % (args.batch, per, args.mpc_form, n, m, args.seed0 + 1, args.eps_abs, fresh))
            metric = "QP solves/sec (batch=%d linear-MPC QPs n=%d m=%d)" % (args.batch, n, m)
        else:
            wl = ("batch=%d%s random dense QPs n=%d m=%d (n_eq=%d), feasible rand_qp seeds %d.., eps_abs=%g, cold "
                  "start, reference defaults; %s" % (args.batch, per, n, m, args.n_eq, args.seed0, args.eps_abs, fresh))
            metric = "QP solves/sec (batch=%d random dense QPs n=%d m=%d)" % (args.batch, n, m)
        out = {
            "metric": metric,
            "value": value,
            "unit": "QP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": step_s * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": args.precision,
            "data": "synthetic",
            "config": {"workload": wl,
                       "global_batch": int(tot_qps), "parallelism": "batch-split x%d, no collectives" % world,
                       "kernel": kernel, "tile": args.tile, "low_memory": bool(args.low_memory),
                       "fresh_batches": nb, "dispatch_history": False,
                       "rho_window": models[0].get_window()[0]},
            "admm_iters_per_sec": tot_iters / step_s,
            "mean_iters": tot_iters / tot_qps,
            "solved_frac": tot_solved / tot_qps,
            "setup_s": setup_max,
            "setup_plus_solve_qps": tot_qps / (setup_max + step_s),
            "input_generation_s": t_gen,
        }
        if args.full:
            roof = out["roofline"] = roofline(kernel, args, n, m, esz, blocks, rank_iters_max, kern_avg_s, cold_ms)
        if hist_step > 0:
            out["value_with_history"] = tot_qps / hist_step
            out["with_history"] = {"ms_per_step": hist_step * 1e3, "kernel_ms": hist_kern * 1e3,
                                   "steps": args.history_steps,
                                   "roofline_frac": (hist_iters * (2 * n * n + 4 * m * n) / hist_kern / 1e12) /
                                                    (roof["peak"] if roof["unit"] == "TFLOP/s" else float("nan")),
                                   "note": "one batch solved repeatedly, workgroups issued longest-first by the previous solve's "
                                           "iteration counts; NOT the headline"}
        if world > 1:     # per-GPU spread (instances are independent: a rank's time is its own shard's work, nothing is exchanged)
            out["per_gpu"] = {"kernel_ms_min": -neg_kern_min * 1e3, "kernel_ms_max": kern_avg_s * 1e3,
                              "ms_per_step_min": -neg_el_min / args.steps * 1e3, "ms_per_step_max": step_s * 1e3,
                              "iterations_per_step_min": -neg_it_min, "iterations_per_step_max": rank_iters_max}
        if cpu is not None:
            out["cpu_baseline"] = cpu
            out["gpu_over_cpu"] = value / cpu["value"]
            out["gpu_over_cpu_factored_f32"] = value / cpu["factored_f32_value"]
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
