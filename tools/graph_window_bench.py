"""A/B of the fixed-pass window protocol (rqp_set_window_passes, setup(graph_passes=P)) on one GPU, one process.

Per shape (headline batch: 4096 x n=100, m=300 float32; config 4: 8192 x n=32, m=64 float32) and variant
  a  default windowed handle (host loop), eager        b  graph_passes=4, eager
  c  graph_passes=4, replayed from a HIP graph          d  full_ladder=True, replayed
it runs the same warm-started closed loop -- update(g, l, u) + solve() on a rotation of 4 perturbed vector sets -- and
reports ms per step (device events around `steps` steps), setup time and the workspace the handle allocated
(torch.cuda.mem_get_info before / after setup).  The cost of one idle pass is (replay time at P = 4 + 8 minus replay time
at P = 4) / 8 on the same inputs (reported only when no instance needed more than 4 passes).  Final outputs of a, b, c, d
are compared bit for bit.  Prints one JSON line.

    python tools/graph_window_bench.py [--steps 20] [--warmup 3] [--shapes headline,config4] [--only c]
(--only runs one variant of each shape, e.g. under rocprofv3.)
"""
import argparse
import json
import os
import sys

R0 = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R0, "reluqp-py_amd"))

import numpy as np  # noqa: E402

SHAPES = {"headline": (4096, 100, 25, 275), "config4": (8192, 32, 8, 56)}


def run_variant(H, vecs, variant, passes, steps, warmup, dev):
    import torch
    import reluqp.reluqpth as reluqpth
    graph_passes = None if variant == "a" else (None if variant == "d" else passes)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    m = reluqpth.ReLU_QP()
    g0, l0, u0 = vecs[0]
    m.setup(H[0], g0, H[1], l0, u0, device=dev, precision=torch.float32, full_ladder=(variant == "d"),
            graph_passes=graph_passes)
    setup_ms = m.results.info.setup_time * 1e3
    torch.cuda.synchronize()
    ws = free0 - torch.cuda.mem_get_info(dev)[0]
    m.synchronous = False
    gs, ls, us = (v.clone() for v in vecs[0])

    def step():
        m.update(g=gs, l=ls, u=us)
        return m.solve()

    def load(k):
        for dst, src in zip((gs, ls, us), vecs[k % len(vecs)]):
            dst.copy_(src)

    replay = variant in ("c", "d")
    res = None
    if replay:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            res = step()
        run = graph.replay
    else:
        step()
        run = None
    for k in range(warmup):
        load(k + 1)
        if replay:
            run()
        else:
            res = step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(steps):
        load(warmup + 1 + k)
        if replay:
            run()
        else:
            res = step()
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / steps
    sc = res.info.status_code
    out = dict(ms_per_step=round(ms, 4), setup_ms=round(setup_ms, 3), workspace_gb=round(ws / 1e9, 3),
               kernel=m.kernel, window=m.get_window()[0], exhausted=int((sc == 5).sum()),
               mean_iter=float(res.info.iter.float().mean()), solved_frac=float((sc == 0).float().mean()))
    final = (res.x.clone(), res.info.iter.clone(), res.info.rho_ind.clone(), res.info.pri_res.clone())
    del m, res
    torch.cuda.synchronize()
    return out, final


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--shapes", default="headline,config4")
    ap.add_argument("--only", default=None, help="one variant (a, b, c, d) per shape")
    args = ap.parse_args()
    from reluqp import utils
    data = {}
    for name in args.shapes.split(","):      # inputs first: the generator forks workers before the GPU is initialised
        B, n, ne, ni = SHAPES[name]
        data[name] = utils.rand_qp_batch(B, n, ne, ni, seed0=0, feasible=True, dtype=np.float32, workers=16)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("graph_window_bench needs a GPU")
    dev = torch.device("cuda:0")
    result = {"tool": "graph_window_bench", "steps": args.steps, "warmup": args.warmup, "passes": args.passes, "shapes": {}}
    for name in args.shapes.split(","):
        H, g, A, l, u, _ = data[name]
        Hd = (torch.as_tensor(H, device=dev), torch.as_tensor(A, device=dev))
        vecs = [tuple(torch.as_tensor(v, device=dev) for v in (g * (1.0 + 0.02 * k), l, u)) for k in range(4)]
        variants = [args.only] if args.only else ["a", "b", "c", "d"]
        rows, finals = {}, {}
        for v in variants:
            rows[v], finals[v] = run_variant(Hd, vecs, v, args.passes, args.steps, args.warmup, dev)
        if not args.only:
            rows["c_idle"], _ = run_variant(Hd, vecs, "c", args.passes + 8, args.steps, args.warmup, dev)
            if rows["c"]["exhausted"] == 0:
                rows["idle_pass_us"] = round((rows["c_idle"]["ms_per_step"] - rows["c"]["ms_per_step"]) * 1e3 / 8, 2)
            same = lambda p, q: all(torch.equal(torch.nan_to_num(x, nan=1.0), torch.nan_to_num(y, nan=1.0))
                                    for x, y in zip(finals[p], finals[q]))
            rows["bit_identical"] = {"a=b": same("a", "b"), "a=c": same("a", "c"), "a=d": same("a", "d")}
        result["shapes"][name] = dict(batch=H.shape[0], n=H.shape[1], m=A.shape[1], **rows)
        del Hd, vecs
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
