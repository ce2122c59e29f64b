"""Reverse mode of the LTV condensing on the device (rqp_ltv_condense_adjoint, reluqp.layer.LTVCondenseFunction / LTVMPCLayer).

Kernel vs host, the rule of tests/test_ltv_gpu.py: the formulas are evaluated once in np.longdouble (the yardstick,
reluqp.mpc.condense_ltv_vjp on longdouble inputs); e_host is the error of the float64 numpy evaluation against it, per output,
relative to `scale` = max|entry| of the same formulas evaluated on the absolute values of every term (what a backward-stable
evaluation of these sums is accurate to).  float64 device outputs: e_dev <= 10 max(e_host, 2^-52); float32 outputs within 1
ulp(float32) of the rounded yardstick wherever |entry| >= 2^-24 scale.  Ratios are printed before they are asserted.

End to end: gradients of sum(w . u0) through LTVMPCLayer against the numpy chain condense_ltv_vjp o adjoint_ref.adjoint at the
device's own solution (tests/ltv_adjoint_fixture.py), |err| <= 1e-9 (1 + max|ref|)."""
import numpy as np
import pytest
import torch

from reluqp import _cabi, mpc
from reluqp.layer import LTVCondenseFunction, LTVMPCLayer

import adjoint_ref as R
import ltv_adjoint_fixture as FX

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
OUT = ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R", "Qf")


def _close(got, ref, rel):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.abs(got - ref).max() <= rel * (1 + np.abs(ref).max()), (np.abs(got - ref).max(), np.abs(ref).max())


def _abs_scale(Ad, Bd, Q, R_, Qf, K, c, x0, xref, uref, bars):
    """The vjp's formulas with every term replaced by its absolute value (one instance): the size of what is summed."""
    N, nx, nu = Ad.shape[0], Ad.shape[1], Bd.shape[2]
    blk, n = nx + nu, N * nu
    cond = mpc.condense_ltv(Ad, Bd, Q, R_, Qf, K=K, c=c)
    F, G, f, S = (np.abs(cond[k]) for k in ("F", "G", "f", "H_sp"))
    Hb, Ab, gb, lb, ub = (np.abs(b) for b in bars)
    Kz = np.zeros((nu, nx)) if K is None else np.abs(K)
    yref = np.abs(np.hstack([np.zeros((N, nu)) if uref is None else uref, np.zeros((N, nx)) if xref is None else xref]).reshape(-1))
    x0 = np.abs(x0)
    e = G @ x0 + f + yref
    Hs = (Hb + Hb.T) / 2
    T = F @ Hs
    Fb = Ab + 2 * (S @ T) + np.outer(S @ e, gb)
    eb = S @ (F @ gb)
    sb = eb + lb + ub
    Yb = np.hstack([Fb, np.outer(sb, x0), sb[:, None]])
    Fg = F @ gb
    Rb, Qb, Qfb = np.zeros((nu, nu)), np.zeros((nx, nx)), np.zeros((nx, nx))
    for k in range(N):
        rk = slice(k * blk, (k + 1) * blk)
        Sk = F[rk] @ T[rk].T + np.outer(Fg[rk], e[rk])
        Rb += Sk[:nu, :nu]
        if k == N - 1:
            Qfb += Sk[nu:, nu:]
        else:
            Qb += Sk[nu:, nu:]
    Y = np.hstack([F, G, f[:, None]])
    X0 = np.zeros((nx, n + nx + 1))
    X0[:, n:n + nx] = np.eye(nx)
    X = [X0] + [Y[k * blk + nu:(k + 1) * blk] for k in range(N)]
    Adb, Bdb, cb = np.zeros(Ad.shape), np.zeros(Bd.shape), np.zeros((N, nx))
    Lam = Yb[(N - 1) * blk + nu:N * blk].copy()
    for k in range(N - 1, -1, -1):
        Aclb = Lam @ X[k].T
        Adb[k], Bdb[k], cb[k] = Aclb, Lam[:, k * nu:(k + 1) * nu] + Aclb @ Kz.T, Lam[:, -1]
        if k >= 1:
            Lam = (np.abs(Ad[k]) + np.abs(Bd[k]) @ Kz).T @ Lam + Kz.T @ Yb[k * blk:k * blk + nu] + Yb[(k - 1) * blk + nu:k * blk]
    yr = eb.reshape(N, blk)
    out = dict(Ad=Adb, Bd=Bdb, c=cb, x0=G.T @ sb, xref=yr[:, nu:], uref=yr[:, :nu], Q=Qb, R=Rb, Qf=Qfb)
    return {k: float(np.abs(v).max()) for k, v in out.items()}


def _kernel_case(shape, prec, opts, seed=11):
    nx, nu, N, B = shape
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)
    rs = np.random.RandomState(seed + 1)
    Ad = Ad0[None, None] + 0.05 * rs.randn(B, N, nx, nx) / np.sqrt(nx)
    Bd = Bd0[None, None] + 0.05 * rs.randn(B, N, nx, nu)
    full = opts == "K_c_refs"
    c = 0.1 * rs.randn(B, N, nx) if full else None
    Q, R_ = np.diag(1.0 + rs.rand(nx)), 0.1 * np.eye(nu) + 0.01 * np.ones((nu, nu))
    Qf = 2.0 * Q + 0.1 * np.ones((nx, nx))
    K = 0.1 * rs.randn(nu, nx) if opts != "plain" else None
    n, m = N * nu, N * (nx + nu)
    x0 = rs.randn(B, nx)
    xref, uref = (0.3 * rs.randn(B, N, nx), 0.1 * rs.randn(B, N, nu)) if full else (None, None)
    bars = [rs.randn(B, n, n), rs.randn(B, m, n), rs.randn(B, n), rs.randn(B, m), rs.randn(B, m)]
    npt = np.float32 if prec == torch.float32 else np.float64
    rnd = lambda a: None if a is None else np.asarray(a).astype(npt)     # the values the device sees
    Ad, Bd, c, x0, xref, uref = (rnd(a) for a in (Ad, Bd, c, x0, xref, uref))
    bars = [rnd(b) for b in bars]
    return dict(Ad=Ad, Bd=Bd, c=c, x0=x0, xref=xref, uref=uref, Q=Q, R=R_, Qf=Qf, K=K, bars=bars, dims=(nx, nu, N, B))


def _device(d, sl=slice(None), bars=(0, 1, 2, 3, 4), want=OUT, ws=None):
    """Forward condensing + adjoint of the instances `sl` on the device; returns (dict of tensors, workspaces)."""
    nx, nu, N, _ = d["dims"]
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a[sl]), device=DEV)
    Ad, Bd, c, x0, xref, uref = (t(d[k]) for k in ("Ad", "Bd", "c", "x0", "xref", "uref"))
    B = Ad.shape[0]
    w = (d["Q"], d["R"], d["Qf"], d["K"])
    if ws is None:
        ws = (mpc.ltv_workspace(B, nx, nu, N, DEV), mpc.ltv_adjoint_workspace(B, nx, nu, N, DEV))
        mpc.condense_ltv_device(Ad, Bd, w, ws[0], c=c)
    cot = {k: (t(b) if i in bars else None) for i, (k, b) in enumerate(zip(("dH", "dA", "dg", "dl", "du"), d["bars"]))}
    out = mpc.condense_ltv_adjoint_device(Ad, Bd, x0, w, ws[0], ws[1], xref=xref, uref=uref, want=want, **cot)
    return out, ws


@pytest.mark.parametrize("opts", ["plain", "K", "K_c_refs"])
@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", [(12, 4, 20, 64), (7, 3, 9, 5), (16, 4, 32, 4), (12, 8, 20, 3), (3, 1, 7, 3)])
def test_kernels_match_host_vjp(shape, prec, opts):
    nx, nu, N, B = shape
    d = _kernel_case(shape, prec, opts)
    out, _ = _device(d)
    # instances compared with the yardstick: a spread over the batch (first, second, middle, last); every instance of the
    # B = 64 batch in its float64 case with K, c and references, where the batch sums of all 64 are held to the same rule
    everyone = B > 4 and prec == torch.float64 and opts == "K_c_refs"
    idx = list(range(B)) if (everyone or B <= 4) else sorted({0, 1, B // 2, B - 1})
    sub, _ = _device(d, idx, want=("Q", "R", "Qf"))             # the batch sums of a call with these instances alone
    torch.cuda.synchronize()
    dev = {k: v.cpu().numpy() for k, v in out.items()}
    dev_sub = {k: v.cpu().numpy() for k, v in sub.items()}
    npt = np.float32 if prec == torch.float32 else np.float64
    assert dev["Ad"].dtype == npt and dev["Q"].dtype == np.float64
    for k in ("Q", "R", "Qf"):
        assert np.array_equal(dev[k], dev[k].T), "%s gradient must be bitwise symmetric" % k
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    res = {dt: {} for dt in (LD, np.float64)}
    scales = {}
    for b in idx:
        at = lambda a, dt: None if a is None else a[b].astype(dt)
        for dt in (LD, np.float64):
            res[dt][b] = mpc.condense_ltv_vjp(
                at(d["Ad"], dt), at(d["Bd"], dt), d["Q"].astype(dt), d["R"].astype(dt), d["Qf"].astype(dt), at(d["x0"], dt),
                l_add, u_add, K=None if d["K"] is None else d["K"].astype(dt), c=at(d["c"], dt), xref=at(d["xref"], dt),
                uref=at(d["uref"], dt), **{k: at(v, dt) for k, v in zip(("dH", "dA", "dg", "dl", "du"), d["bars"])})
        at64 = lambda a: None if a is None else a[b].astype(np.float64)
        scales[b] = _abs_scale(at64(d["Ad"]), at64(d["Bd"]), d["Q"], d["R"], d["Qf"], d["K"], at64(d["c"]), at64(d["x0"]),
                               at64(d["xref"]), at64(d["uref"]), [v[b].astype(np.float64) for v in d["bars"]])
    assert res[LD][idx[0]]["Ad"].dtype == LD
    worst = {}

    def compare(k, got, ref, host, scale):
        e_host = float(np.abs(host.astype(LD) - ref).max()) / scale
        if got.dtype == np.float64:
            e_dev = float(np.abs(got.astype(LD) - ref).max()) / scale
            ratio = e_dev / max(e_host, 2.0 ** -52)
            if ratio >= worst.get(k, [-1.0])[0]:
                worst[k] = [ratio, e_dev, e_host]
        else:
            r32 = ref.astype(np.float32)
            ulps = np.abs(got.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
            big = np.abs(ref) >= 2.0 ** -24 * scale
            worst[k] = [max(worst.get(k, [0.0])[0], float(ulps[big].max()) if big.any() else 0.0)]

    for b in idx:
        for k in ("Ad", "Bd", "c", "x0", "xref", "uref"):
            compare(k, dev[k][b], res[LD][b][k], res[np.float64][b][k], scales[b][k])
    tot = {k: sum(scales[b][k] for b in idx) for k in ("Q", "R", "Qf")}
    for k in ("Q", "R", "Qf"):
        if N == 1 and k == "Q":
            continue
        # (float32 inputs still give float64 sums: held to the float64 rule)
        compare(k, dev_sub[k], sum(res[LD][b][k] for b in idx), sum(res[np.float64][b][k] for b in idx), tot[k])
        if everyone:                                            # the sum over the whole batch of 64 against its yardstick
            compare(k + " (B = %d)" % B, dev[k], sum(res[LD][b][k] for b in idx), sum(res[np.float64][b][k] for b in idx), tot[k])
    for k, w in worst.items():
        if len(w) == 3:
            print("LTV adjoint f64 %s %s %s: e_dev / max(e_host, 2^-52) = %.3f (e_dev %.3e, e_host %.3e)" % (shape, opts, k, *w))
        else:
            print("LTV adjoint f32 %s %s %s: max ulp distance from the rounded yardstick = %.3f" % (shape, opts, k, w[0]))
    # the whole batch's sums against the sums of its chunks of 4 instances (two summation orders of the same terms; a
    # device-against-device check of the batch indexing of the reduction, not an accuracy statement)
    if B > 4 and B % 4 == 0:
        for k in ("Q", "R", "Qf"):
            acc = sum(_device(d, slice(i, i + 4), want=(k,))[0][k].cpu().numpy() for i in range(0, B, 4))
            err = np.abs(acc - dev[k]).max() / (B / len(idx) * tot[k])
            print("LTV adjoint %s %s %s: batch of %d vs its chunks, relative to the summed terms: %.3e" % (shape, opts, k, B, err))
            assert err <= 64 * 2.0 ** -52
    for k, w in worst.items():
        assert w[0] <= (10.0 if len(w) == 3 else 1.0), (k, w)


def test_subsets_of_cotangents_and_outputs_are_bitwise_those_of_the_full_call():
    d = _kernel_case((7, 3, 9, 5), torch.float64, "K_c_refs")
    full, ws = _device(d)
    for keep in ((2,), (0, 1)):                                 # only dg; only dH, dA: absent == zero
        some, _ = _device(d, bars=keep, ws=ws)
        dz = dict(d, bars=[b if i in keep else np.zeros_like(b) for i, b in enumerate(d["bars"])])
        zero, _ = _device(dz, ws=ws)
        for k in OUT:
            assert torch.equal(some[k], zero[k]), (keep, k)
    for want in (("x0",), ("xref", "uref"), ("Ad",), ("Bd", "c"), ("R",), ("Q", "Qf", "x0")):
        part, _ = _device(d, want=want, ws=ws)
        assert tuple(part) == want
        for k in want:
            assert torch.equal(part[k], full[k]), (want, k)
    # garbage at the structural zeros of dA changes nothing
    nx, nu, N, B = d["dims"]
    junk = [b.copy() for b in d["bars"]]
    for j in range(1, N):
        junk[1][:, :j * (nx + nu), j * nu:(j + 1) * nu] = 1e6
    got, _ = _device(dict(d, bars=junk), ws=ws)
    for k in OUT:
        assert torch.equal(got[k], full[k]), k


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
def test_two_calls_and_a_graph_replay_are_bitwise_equal(prec):
    d = _kernel_case((12, 4, 20, 64), prec, "K_c_refs")
    nx, nu, N, B = d["dims"]
    t = lambda a: torch.as_tensor(a, device=DEV)
    Ad, Bd, c, x0, xref, uref = (t(d[k]) for k in ("Ad", "Bd", "c", "x0", "xref", "uref"))
    cot = {k: t(b) for k, b in zip(("dH", "dA", "dg", "dl", "du"), d["bars"])}
    w = mpc._LtvWeights(nx, nu, d["Q"], d["R"], d["Qf"], d["K"])
    ws, adj = mpc.ltv_workspace(B, nx, nu, N, DEV), mpc.ltv_adjoint_workspace(B, nx, nu, N, DEV)
    mpc.condense_ltv_device(Ad, Bd, w, ws, c=c)
    run = lambda: mpc.condense_ltv_adjoint_device(Ad, Bd, x0, w, ws, adj, xref=xref, uref=uref, **cot)
    a = run()
    b = run()
    torch.cuda.synchronize()
    for k in OUT:
        assert torch.equal(a[k], b[k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                   # (warm-up on the side stream: LDS attributes set outside capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run()
    graph.replay()
    torch.cuda.synchronize()
    for k in OUT:
        assert torch.equal(cap[k], a[k]), k


def _layer_inputs(p, grad=("Ad", "Bd", "c", "x0", "xref", "Q", "R", "Qf")):
    t = {k: torch.as_tensor(p[k], dtype=torch.float64, device=DEV) for k in ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R", "Qf")}
    for k in grad:
        t[k].requires_grad_()
    return t


def _solution(layer):
    solver = next(iter(layer.qp._handles.values()))["solver"]
    r = solver.results
    return (r.x.detach().cpu().numpy().copy(), r.y.detach().cpu().numpy().copy(), r.active.cpu().numpy().copy(),
            solver.info.status_polish.cpu().numpy().copy())


@pytest.mark.parametrize("shape", FX.SHAPES)
def test_layer_gradients_match_the_numpy_chain(shape):
    nx, nu, N = shape
    p = FX.problem(*shape)
    layer = LTVMPCLayer(nx, nu, N, FX.U_MAX, FX.X_MAX, K=p["K"], eps_abs=1e-6)
    t = _layer_inputs(p)
    u0, v = layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], t["Qf"], c=t["c"], xref=t["xref"], uref=t["uref"])
    x, y, act, pol = _solution(layer)
    # (i) the active set the device reports is the exact one of the fixture, on every instance
    H, A, g, l, u = FX.condensed(p)
    for b in range(FX.B):
        xe, ye, dist, mult = FX.margins(H[b], A[b], g[b], l[b], u[b], act[b])
        assert dist >= FX.MARGIN and mult >= FX.MARGIN, (b, dist, mult)      # only the true active set solves the QP with margins
        assert np.abs(xe - x[b]).max() <= 1e-5 * max(1.0, np.abs(xe).max()), b
    w = np.random.RandomState(9).randn(FX.B, nu)
    (u0 * torch.as_tensor(w, device=DEV)).sum().backward()
    ref = FX.reference_gradients(p, x, y, act, w)
    for k in ("Ad", "Bd", "c", "x0", "xref", "Q", "R", "Qf"):
        got = t[k].grad.cpu().numpy()
        err = np.abs(got - ref[k]).max()
        print("%s d/d%-4s max|err| %.3e, max|ref| %.3e" % (shape, k, err, np.abs(ref[k]).max()))
    for k in ("Ad", "Bd", "c", "x0", "xref", "Q", "R", "Qf"):
        _close(t[k].grad.cpu().numpy(), ref[k], 1e-9)
    assert t["uref"].grad is None


def test_three_forwards_before_one_backward():
    """An unrolled closed loop with a new linearisation at every step: each backward step finds the shared forward workspace
    overwritten by the later forwards and has to rebuild its own."""
    shape = FX.SHAPES[0]
    nx, nu, N = shape
    steps = [FX.problem(*shape, step=s) for s in range(3)]
    p0 = steps[0]
    layer = LTVMPCLayer(nx, nu, N, FX.U_MAX, FX.X_MAX, K=p0["K"], eps_abs=1e-6)
    f64 = torch.float64
    tt = lambda a: torch.as_tensor(a, dtype=f64, device=DEV)
    Q, R_, Qf = (tt(p0[k]).requires_grad_() for k in ("Q", "R", "Qf"))
    x0 = tt(p0["x0"]).requires_grad_()
    stage = [dict(Ad=tt(s["Ad"]).requires_grad_(), Bd=tt(s["Bd"]).requires_grad_(), c=tt(s["c"])) for s in steps]
    x, sols, states = x0, [], []
    for s in stage:
        states.append(x.detach().cpu().numpy().copy())
        u0, _ = layer(s["Ad"], s["Bd"], x, Q, R_, Qf, c=s["c"])
        sols.append(_solution(layer))
        x = (s["Ad"][:, 0] @ x.unsqueeze(2)).squeeze(2) + (s["Bd"][:, 0] @ u0.unsqueeze(2)).squeeze(2) + s["c"][:, 0]
    w = np.random.RandomState(4).randn(FX.B, nx)
    (x * tt(w)).sum().backward()
    # the numpy chain, backwards through the same loop at the device's solutions and active sets
    xb = w.copy()
    ref = dict(Q=0.0, R=0.0, Qf=0.0, Ad=[None] * 3, Bd=[None] * 3)
    for i in (2, 1, 0):
        s, (v, y, act, _) = steps[i], sols[i]
        xs = states[i]
        u0 = v[:, :nu] - xs @ p0["K"].T
        A0, B0 = s["Ad"][:, 0], s["Bd"][:, 0]
        dA0 = np.einsum("bi,bj->bij", xb, xs)                   # x+ = A_0 x + B_0 u0 + c_0
        dB0 = np.einsum("bi,bj->bij", xb, u0)
        ub = np.einsum("bij,bi->bj", B0, xb)
        pi = dict(s, x0=xs, xref=None, uref=None, Q=p0["Q"], R=p0["R"], Qf=p0["Qf"], K=p0["K"])
        gr = _loop_reference(pi, v, y, act, ub)
        gr["Ad"][:, 0] += dA0
        gr["Bd"][:, 0] += dB0
        ref["Ad"][i], ref["Bd"][i] = gr["Ad"], gr["Bd"]
        for k in ("Q", "R", "Qf"):
            ref[k] = ref[k] + gr[k]
        xb = np.einsum("bij,bi->bj", A0, xb) + gr["x0"]
    for i in range(3):
        _close(stage[i]["Ad"].grad.cpu().numpy(), ref["Ad"][i], 1e-9)
        _close(stage[i]["Bd"].grad.cpu().numpy(), ref["Bd"][i], 1e-9)
    _close(x0.grad.cpu().numpy(), xb, 1e-9)
    for k, tns in (("Q", Q), ("R", R_), ("Qf", Qf)):
        _close(tns.grad.cpu().numpy(), ref[k], 1e-9)


def _loop_reference(p, x, y, act, w):
    q = dict(p)
    N, nx = p["Ad"].shape[1], p["Ad"].shape[2]
    nu = p["Bd"].shape[3]
    q["xref"], q["uref"] = np.zeros((FX.B, N, nx)), np.zeros((FX.B, N, nu))
    return FX.reference_gradients(q, x, y, act, w)


def test_gradcheck_of_the_condensing_alone():
    rs = np.random.RandomState(2)
    B, nx, nu, N = 2, 3, 1, 4
    m = N * (nx + nu)
    f64 = torch.float64
    tt = lambda a: torch.as_tensor(a, dtype=f64, device=DEV).requires_grad_()
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=1)
    Ad, Bd = tt(Ad0[None, None] + 0.1 * rs.randn(B, N, nx, nx)), tt(Bd0[None, None] + 0.1 * rs.randn(B, N, nx, nu))
    c, x0, xref, uref = tt(0.1 * rs.randn(B, N, nx)), tt(rs.randn(B, nx)), tt(0.3 * rs.randn(B, N, nx)), tt(0.1 * rs.randn(B, N, nu))

    def spd(k):
        W = rs.randn(k, k)
        return W @ W.T / k + np.eye(k)

    Q, R_, Qf = tt(spd(nx)), tt(spd(nu)), tt(spd(nx))
    l_add, u_add = tt(-np.ones(m) + 0.1 * rs.randn(m)), tt(np.ones(m) + 0.1 * rs.randn(m))      # shared: gradients summed over the batch
    cd = mpc.LTVCondenser(nx, nu, N, K=0.2 * rs.randn(nu, nx))
    fn = lambda *a: LTVCondenseFunction.apply(cd, *a)
    assert torch.autograd.gradcheck(fn, (Ad, Bd, c, x0, xref, uref, Q, R_, Qf, l_add, u_add))
    lb, ub = tt(l_add.detach().expand(B, m).clone()), tt(u_add.detach().expand(B, m).clone())      # per-instance bounds
    norefs = lambda Ad, Bd, c, x0, Q, R_, Qf, lb, ub: LTVCondenseFunction.apply(cd, Ad, Bd, c, x0, None, None, Q, R_, Qf, lb, ub)
    assert torch.autograd.gradcheck(norefs, (Ad, Bd, c, x0, Q, R_, Qf, lb, ub))


def test_a_gain_that_requires_grad_is_refused():
    with pytest.raises(ValueError, match="K cannot require a gradient"):
        mpc.LTVCondenser(3, 1, 4, K=torch.zeros(1, 3, device=DEV, requires_grad=True))
