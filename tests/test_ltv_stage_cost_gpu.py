"""Stage-varying, per-instance cost weights of the LTV condensing on the device (RQP_LTV_STAGE_WEIGHTS: rqp_ltv_condense,
rqp_ltv_vectors, rqp_ltv_condense_adjoint), the BatchedLTVMPC driver and LTVMPCLayer on top of them.

Kernel vs host, the rules of tests/test_ltv_gpu.py and tests/test_ltv_adjoint_gpu.py unchanged: the formulas are evaluated once
in np.longdouble (the yardstick: reluqp.mpc.condense_ltv / condense_ltv_vjp on longdouble inputs, the stage weights in them);
e_host is the error of the float64 numpy evaluation against it, per output, relative to max|entry| of the output (forward) or
of the same formulas on the absolute values of every term (adjoint).  float64 device outputs: e_dev <= 10 max(e_host, 2^-52);
float32 outputs within 1 ulp(float32) of the rounded yardstick wherever |entry| >= 2^-24 of that scale.  The ratios are
printed before they are asserted.  The weights (tests/ltv_stage_cost_fixture.py) differ for every (instance, stage) and grow
with both, so a block taken from the wrong place is far outside these bounds."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reluqp_oracle as O
from reluqp import _cabi, mpc
from reluqp.layer import LTVCondenseFunction, LTVMPCLayer

import ltv_adjoint_fixture as FX
import ltv_stage_cost_fixture as SF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
# (nx, nu, N, B): a plain one; the LDS limit with two [G | f] tiles; n = 160; below one tile; more instances than a slice of anything
SHAPES = [(7, 3, 9, 5), (16, 4, 32, 4), (12, 8, 20, 3), (3, 1, 7, 3), (12, 4, 20, 9)]
BARS = ("dH", "dA", "dg", "dl", "du")
OUT = ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R")


def _close(got, ref, rel):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.abs(got - ref).max() <= rel * (1 + np.abs(ref).max()), (np.abs(got - ref).max(), np.abs(ref).max())


_CASES = {}


def _case(shape, prec, opts, seed=11):
    """Inputs of one kernel case as the device sees them (rounded to `prec`), computed once and left unchanged."""
    key = (shape, prec, opts)
    if key in _CASES:
        return _CASES[key]
    nx, nu, N, B = shape
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)
    rs = np.random.RandomState(seed + 1)
    Ad = Ad0[None, None] + 0.05 * rs.randn(B, N, nx, nx) / np.sqrt(nx)
    Bd = Bd0[None, None] + 0.05 * rs.randn(B, N, nx, nu)
    full = opts == "K_c_refs"
    c = 0.1 * rs.randn(B, N, nx) if full else None
    K = 0.1 * rs.randn(nu, nx) if full else None
    n, m = N * nu, N * (nx + nu)
    x0 = rs.randn(B, nx)
    xref, uref = (0.3 * rs.randn(B, N, nx), 0.1 * rs.randn(B, N, nu)) if full else (None, None)
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    if full:                                                    # per-instance bounds
        l_add, u_add = l_add[None] - rs.rand(B, m), u_add[None] + rs.rand(B, m)
    bars = [rs.randn(B, n, n), rs.randn(B, m, n), rs.randn(B, n), rs.randn(B, m), rs.randn(B, m)]
    Q, R = SF.stage_weights(rs, B, N, nx, nu)                   # float64 whatever the precision of the stages
    npt = np.float32 if prec == torch.float32 else np.float64
    rnd = lambda a: None if a is None else np.asarray(a).astype(npt)
    d = dict(Ad=rnd(Ad), Bd=rnd(Bd), c=rnd(c), x0=rnd(x0), xref=rnd(xref), uref=rnd(uref), l_add=rnd(l_add), u_add=rnd(u_add),
             bars=[rnd(b) for b in bars], Q=Q, R=R, K=K, dims=shape, npt=npt)
    _CASES[key] = d
    return d


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _forward(d, weights, ws=None):
    """condense + vectors on the device: (dict of H, A, g, l, u tensors, workspace)."""
    nx, nu, N, B = d["dims"]
    ws = mpc.ltv_workspace(B, nx, nu, N, DEV) if ws is None else ws
    H, A = mpc.condense_ltv_device(_t(d["Ad"]), _t(d["Bd"]), weights, ws, c=_t(d["c"]))
    g, l, u = mpc.ltv_vectors_device((nx, nu, N, d["K"] is not None, d["c"] is not None), _t(d["x0"]), _t(d["l_add"]), _t(d["u_add"]),
                                     weights, ws, xref=_t(d["xref"]), uref=_t(d["uref"]))
    return dict(H=H, A=A, g=g, l=l, u=u), ws


def _adjoint(d, weights, ws, bars=None, want=OUT):
    nx, nu, N, B = d["dims"]
    adj = mpc.ltv_adjoint_workspace(B, nx, nu, N, DEV)
    cot = {k: _t(b) for k, b in zip(BARS, d["bars"] if bars is None else bars)}
    return mpc.condense_ltv_adjoint_device(_t(d["Ad"]), _t(d["Bd"]), _t(d["x0"]), weights, ws, adj, xref=_t(d["xref"]),
                                           uref=_t(d["uref"]), want=want, **cot)


class _Worst(object):
    """The rule of test_kernels_match_host_formulas / test_kernels_match_host_vjp, per output name."""

    def __init__(self, tag):
        self.tag, self.w = tag, {}

    def add(self, k, got, ref, host, scale):
        e_host = float(np.abs(host.astype(LD) - ref).max()) / scale
        if got.dtype == np.float64:
            e_dev = float(np.abs(got.astype(LD) - ref).max()) / scale
            ratio = e_dev / max(e_host, 2.0 ** -52)
            if ratio >= self.w.get(k, [-1.0])[0]:
                self.w[k] = [ratio, e_dev, e_host]
        else:
            r32 = ref.astype(np.float32)
            ulps = np.abs(got.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
            big = np.abs(ref) >= 2.0 ** -24 * scale
            self.w[k] = [max(self.w.get(k, [0.0])[0], float(ulps[big].max()) if big.any() else 0.0)]

    def check(self):
        for k, w in self.w.items():
            if len(w) == 3:
                print("%s f64 %s: e_dev / max(e_host, 2^-52) = %.3f (e_dev %.3e, e_host %.3e)" % (self.tag, k, *w))
            else:
                print("%s f32 %s: max ulp distance from the rounded yardstick = %.3f" % (self.tag, k, w[0]))
        for k, w in self.w.items():
            assert w[0] <= (10.0 if len(w) == 3 else 1.0), (k, w)


@pytest.mark.parametrize("opts", ["plain", "K_c_refs"])
@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_match_host_formulas(shape, prec, opts):
    nx, nu, N, B = shape
    d = _case(shape, prec, opts)
    n, m, blk = N * nu, N * (nx + nu), nx + nu
    out, _ = _forward(d, (d["Q"], d["R"], None, d["K"]))
    torch.cuda.synchronize()
    dev = {k: v.cpu().numpy() for k, v in out.items()}
    assert dev["H"].dtype == d["npt"] and dev["H"].shape == (B, n, n) and dev["A"].shape == (B, m, n)
    for b in range(B):
        assert np.array_equal(dev["H"][b], dev["H"][b].T), "H must be bitwise symmetric"
    for j in range(1, N):                                       # block column j of F is zero above stage j
        assert not dev["A"][:, :j * blk, j * nu:(j + 1) * nu].any(), "structural zeros of A must be exact"
    worst = _Worst("LTV stage weights %s %s" % (shape, opts))
    for b in range(B):
        res = {}
        for dt in (LD, np.float64):
            at = lambda a: None if a is None else a[b].astype(dt)
            cond = mpc.condense_ltv(at(d["Ad"]), at(d["Bd"]), at(d["Q"]), at(d["R"]), None,
                                    K=None if d["K"] is None else d["K"].astype(dt), c=at(d["c"]))
            la, ua = (d["l_add"][b], d["u_add"][b]) if d["l_add"].ndim == 2 else (d["l_add"], d["u_add"])
            g, l, u = mpc.ltv_vectors(cond, at(d["x0"]), la.astype(dt), ua.astype(dt), xref=at(d["xref"]), uref=at(d["uref"]))
            res[dt] = dict(H=cond["H"], A=cond["A"], g=g, l=l, u=u)
        assert res[LD]["H"].dtype == LD
        for k in ("H", "A", "g", "l", "u"):
            worst.add(k, dev[k][b], res[LD][k], res[np.float64][k], float(np.abs(res[LD][k]).max()))
    worst.check()


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", [(12, 4, 20, 6), (16, 4, 32, 2)])
def test_repeated_shared_weights_give_the_bits_of_the_shared_call(shape, prec):
    """Forward and adjoint: the inner products are the same, in the same order."""
    nx, nu, N, B = shape
    d = _case(shape, prec, "K_c_refs")
    rs = np.random.RandomState(5)
    Q, R, Qf = SF.spd_blocks(rs, (1,), nx)[0], SF.spd_blocks(rs, (1,), nu, 0.1)[0], 2.5 * SF.spd_blocks(rs, (1,), nx)[0]
    Qs, Rs = SF.repeated(Q, R, Qf, B, N)
    shared, ws0 = _forward(d, (Q, R, Qf, d["K"]))
    for w in ((Qs, Rs, None, d["K"]), (Qs[0], Rs[0], None, d["K"]), (Q, Rs, Qf, d["K"]), (Qs, R, None, d["K"])):
        staged, ws1 = _forward(d, w)
        for k in ("H", "A", "g", "l", "u"):
            assert torch.equal(staged[k], shared[k]), k
    a0 = _adjoint(d, (Q, R, Qf, d["K"]), ws0, want=OUT + ("Qf",))
    a1 = _adjoint(d, (Qs, Rs, None, d["K"]), ws1)
    torch.cuda.synchronize()
    for k in ("Ad", "Bd", "c", "x0", "xref", "uref"):
        assert torch.equal(a0[k], a1[k]), k
    dQ, dR = a1["Q"].cpu().numpy(), a1["R"].cpu().numpy()
    assert dQ.shape == (B, N, nx, nx) and dR.shape == (B, N, nu, nu) and dQ.dtype == np.float64
    # (the sums are ordered differently: not bitwise)
    _close(dQ[:, :N - 1].sum((0, 1)), a0["Q"].cpu().numpy(), 1e-12)
    _close(dQ[:, N - 1].sum(0), a0["Qf"].cpu().numpy(), 1e-12)
    _close(dR.sum((0, 1)), a0["R"].cpu().numpy(), 1e-12)


def _abs_scale(Ad, Bd, Q, R_, K, c, x0, xref, uref, bars):
    """The vjp's formulas with every term replaced by its absolute value (one instance, stage weights Q [N, nx, nx], R [N, nu,
    nu]): the size of what is summed, per output; for Q and R over the blocks of all stages."""
    N, nx, nu = Ad.shape[0], Ad.shape[1], Bd.shape[2]
    blk, n = nx + nu, N * nu
    cond = mpc.condense_ltv(Ad, Bd, Q, R_, None, K=K, c=c)
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
    Rb, Qb = np.zeros((N, nu, nu)), np.zeros((N, nx, nx))
    for k in range(N):
        rk = slice(k * blk, (k + 1) * blk)
        Sk = F[rk] @ T[rk].T + np.outer(Fg[rk], e[rk])
        Rb[k], Qb[k] = Sk[:nu, :nu], Sk[nu:, nu:]
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
    out = dict(Ad=Adb, Bd=Bdb, c=cb, x0=G.T @ sb, xref=yr[:, nu:], uref=yr[:, :nu], Q=Qb, R=Rb)
    return {k: float(np.abs(v).max()) for k, v in out.items()}


@pytest.mark.parametrize("opts", ["plain", "K_c_refs"])
@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint_kernels_match_host_vjp(shape, prec, opts):
    """Every cotangent given, every output wanted; dQ, dR per block, not summed."""
    nx, nu, N, B = shape
    d = _case(shape, prec, opts)
    w = (d["Q"], d["R"], None, d["K"])
    _, ws = _forward(d, w)
    out = _adjoint(d, w, ws)
    zb = 1                                                      # the cotangents of this instance zeroed: exactly its blocks are zero
    bars0 = [b.copy() for b in d["bars"]]
    for b in bars0:
        b[zb] = 0
    out0 = _adjoint(d, w, ws, bars=bars0, want=("Q", "R"))
    torch.cuda.synchronize()
    dev = {k: v.cpu().numpy() for k, v in out.items()}
    assert dev["Ad"].dtype == d["npt"] and dev["Q"].dtype == np.float64 and dev["R"].dtype == np.float64
    assert dev["Q"].shape == (B, N, nx, nx) and dev["R"].shape == (B, N, nu, nu)
    for k in ("Q", "R"):
        assert np.array_equal(dev[k], np.swapaxes(dev[k], -1, -2)), "every block of d%s must be bitwise symmetric" % k
        z = out0[k].cpu().numpy()
        assert not z[zb].any(), "instance %d has zero cotangents: its d%s blocks must be zero" % (zb, k)
        others = [b for b in range(B) if b != zb]
        assert np.array_equal(z[others], dev[k][others]), "the blocks of the other instances must not move"
        assert all(z[b, j].any() for b in others for j in range(N))
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    worst = _Worst("LTV stage weights adjoint %s %s" % (shape, opts))
    for b in range(B):
        res = {}
        for dt in (LD, np.float64):
            at = lambda a: None if a is None else a[b].astype(dt)
            res[dt] = mpc.condense_ltv_vjp(at(d["Ad"]), at(d["Bd"]), at(d["Q"]), at(d["R"]), None, at(d["x0"]), l_add, u_add,
                                           K=None if d["K"] is None else d["K"].astype(dt), c=at(d["c"]), xref=at(d["xref"]),
                                           uref=at(d["uref"]), **{k: at(v) for k, v in zip(BARS, d["bars"])})
        assert res[LD]["Ad"].dtype == LD and "Qf" not in res[LD]
        at64 = lambda a: None if a is None else a[b].astype(np.float64)
        scale = _abs_scale(at64(d["Ad"]), at64(d["Bd"]), d["Q"][b], d["R"][b], d["K"], at64(d["c"]), at64(d["x0"]), at64(d["xref"]),
                           at64(d["uref"]), [v[b].astype(np.float64) for v in d["bars"]])
        for k in OUT:
            worst.add(k, dev[k][b], res[LD][k], res[np.float64][k], scale[k])
    worst.check()


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
def test_two_calls_and_a_graph_replay_are_bitwise_equal(prec):
    d = _case((12, 4, 20, 9), prec, "K_c_refs")
    nx, nu, N, B = d["dims"]
    Ad, Bd, c, x0, xref, uref, l_add, u_add = (_t(d[k]) for k in ("Ad", "Bd", "c", "x0", "xref", "uref", "l_add", "u_add"))
    cot = {k: _t(b) for k, b in zip(BARS, d["bars"])}
    w = mpc._LtvStageWeights(nx, nu, N, d["Q"], d["R"], None, d["K"])
    w.on(DEV, B)                                                # (the expansion to device tensors happens outside the capture)
    ws, adj = mpc.ltv_workspace(B, nx, nu, N, DEV), mpc.ltv_adjoint_workspace(B, nx, nu, N, DEV)

    def run():
        H, A = mpc.condense_ltv_device(Ad, Bd, w, ws, c=c)
        g, l, u = mpc.ltv_vectors_device((nx, nu, N, True, True), x0, l_add, u_add, w, ws, xref=xref, uref=uref)
        out = mpc.condense_ltv_adjoint_device(Ad, Bd, x0, w, ws, adj, xref=xref, uref=uref, **cot)
        out.update(H=H, A=A, g=g, l=l, u=u)
        return out

    a = run()
    b = run()
    torch.cuda.synchronize()
    for k in a:
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
    for k in a:
        assert torch.equal(cap[k], a[k]), k


# ------------------------------------------------------------------------------------------------------------------ driver
def _driver(c, prec, **kw):
    d = SF.DRIVER
    kw.setdefault("u_max", SF.U_MAX)
    kw.setdefault("x_max", SF.X_MAX)
    ctl = mpc.BatchedLTVMPC(d["nx"], d["nu"], d["N"], c["Q"], c["R"], c["P"], K=c["K"], device=DEV, precision=prec, eps_abs=1e-3, **kw)
    return ctl, (lambda a: torch.as_tensor(a, device=DEV, dtype=prec))


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
def test_driver_with_stage_weights_matches_the_oracle(prec):
    c = SF.driver_case()
    ctl, t = _driver(c, prec)
    ctl.linearize(t(c["Ad"]), t(c["Bd"]), Q=c["Qs"], R=c["Rs"])
    u0, res = ctl.step(t(c["x0"]))
    H, g, A, l, u = SF.driver_qp(c)                             # the staged QPs condensed on the host
    ref = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-3)
    f32 = lambda a: a.astype(np.float32)
    ref32 = O.solve_batch(f32(H), f32(g), f32(A), f32(l), f32(u), form="factored", eps_abs=1e-3, dtype=np.float32)
    print("oracle f32 vs f64: same-iteration share %.3f" % np.mean(ref32["iter"] == ref["iter"]))
    assert np.mean(ref32["iter"] == ref["iter"]) >= 0.9
    it = res.info.iter.cpu().numpy()
    same = it == ref["iter"]
    print("device %s vs oracle: same-iteration share %.3f, kernel %s, iterations %s" % (prec, same.mean(), ctl.solver.kernel, it))
    assert res.info.status == ref["status"]
    assert same.mean() >= 0.75
    scale = max(1.0, np.abs(ref["x"]).max())
    np.testing.assert_allclose(res.x.cpu().double().numpy()[same], ref["x"][same], rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(res.z.cpu().double().numpy()[same], ref["z"][same], rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(res.y.cpu().double().numpy()[same], ref["lam"][same], rtol=0,
                               atol=2e-3 * max(1.0, np.abs(ref["lam"]).max()))
    # the device-built matrices are those of the host statement
    _close(ctl._buf["H"].cpu().double().numpy(), H, 1e-5 if prec == torch.float32 else 1e-12)


def test_driver_keeps_stage_weights_until_replaced():
    prec = torch.float64
    c = SF.driver_case()
    ctl, t = _driver(c, prec)
    Ad, Bd, x0 = t(c["Ad"]), t(c["Bd"]), t(c["x0"])
    ctl.linearize(Ad, Bd, Q=c["Qs"], R=t(c["Rs"]))              # numpy and tensors alike
    H1 = ctl._buf["H"].clone()
    u1, _ = ctl.step(x0)
    ctl.linearize(Ad, Bd)                                       # kept
    assert torch.equal(ctl._buf["H"], H1)
    fresh, _ = _driver(c, prec)
    fresh.linearize(Ad, Bd, Q=c["Qs"][3], R=c["Rs"])            # [N, ., .]: one instance's blocks for the whole batch
    H3 = fresh._buf["H"].clone()
    u3, _ = fresh.step(x0)
    ctl.linearize(Ad, Bd, Q=t(c["Qs"][3]))                      # a new Q replaces the kept one, R stays
    assert torch.equal(ctl._buf["H"], H3) and not torch.equal(H3, H1)
    assert (u3 - u1).abs().max().item() > 1e-3                  # and moves u0
    with pytest.raises(ValueError, match="batch of 16"):
        fresh2, _ = _driver(c, prec)
        fresh2.linearize(Ad, Bd, Q=c["Qs"], R=c["Rs"])
        fresh2.linearize(Ad[:8], Bd[:8])
    # only R given: Q repeats the constructor's Q, ..., Q, Qf
    onlyR, _ = _driver(c, prec)
    onlyR.linearize(Ad, Bd, R=c["Rs"])
    Qrep, _ = SF.repeated(c["Q"], c["R"], c["P"], 16, SF.DRIVER["N"])
    both, _ = _driver(c, prec)
    both.linearize(Ad, Bd, Q=Qrep, R=c["Rs"])
    assert torch.equal(onlyR._buf["H"], both._buf["H"])


def test_repeated_stage_weights_give_the_shared_drivers_input():
    prec = torch.float64
    c = SF.driver_case()
    Ad, Bd, x0 = (torch.as_tensor(c[k], device=DEV, dtype=prec) for k in ("Ad", "Bd", "x0"))
    shared, _ = _driver(c, prec)
    shared.linearize(Ad, Bd)
    u_sh, r_sh = shared.step(x0)
    Qs, Rs = SF.repeated(c["Q"], c["R"], c["P"], 16, SF.DRIVER["N"])
    staged, _ = _driver(c, prec)
    staged.linearize(Ad, Bd, Q=Qs, R=Rs[0])
    u_st, r_st = staged.step(x0)
    for k in ("H", "A", "g", "l", "u"):
        assert torch.equal(shared._buf[k], staged._buf[k]), k
    assert torch.equal(r_sh.info.iter.cpu(), r_st.info.iter.cpu())
    assert torch.equal(u_sh, u_st)


def test_stage_rows_handle_takes_stage_weights():
    prec, nc = torch.float64, 3
    c = SF.driver_case()
    d = SF.DRIVER
    nx, nu, N, B = d["nx"], d["nu"], d["N"], d["B"]
    Ad, Bd, x0 = (torch.as_tensor(c[k], device=DEV, dtype=prec) for k in ("Ad", "Bd", "x0"))
    box, _ = _driver(c, prec)
    box.linearize(Ad, Bd, Q=c["Qs"], R=c["Rs"])
    g_box, _, _ = box.qp_vectors(x0)
    rs = np.random.RandomState(3)
    E = np.zeros((N, nc, nu + nx))                              # shared E: the first input, a random row, the first state
    E[:, 0, 0], E[:, 2, nu] = 1.0, 1.0
    E[:, 1] = 0.3 * rs.randn(N, nu + nx)
    rows, _ = _driver(c, prec, u_max=None, x_max=None, stage_rows=nc)
    rows.linearize(Ad, Bd, E=torch.as_tensor(E, device=DEV, dtype=prec), Q=c["Qs"], R=c["Rs"])
    lo = torch.full((N * nc,), -5.0, device=DEV, dtype=prec)
    g_rows, l, u = rows.qp_vectors(x0, lo=lo, hi=-lo)
    assert rows._buf["A"].shape == (B, N * nc, N * nu)
    assert torch.equal(rows._buf["H"], box._buf["H"]) and torch.equal(g_rows, g_box)
    u0, res = rows.step(x0, lo=lo, hi=-lo)
    assert np.mean([s == "solved" for s in res.info.status]) >= 0.75


# ------------------------------------------------------------------------------------------------------------------- layer
def _layer_inputs(p, grad=("Ad", "Bd", "x0", "Q", "R")):
    t = {k: torch.as_tensor(p[k], dtype=torch.float64, device=DEV) for k in ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R")}
    for k in grad:
        t[k].requires_grad_()
    return t


def _solution(layer):
    solver = next(iter(layer.qp._handles.values()))["solver"]
    r = solver.results
    return (r.x.detach().cpu().numpy().copy(), r.y.detach().cpu().numpy().copy(), r.active.cpu().numpy().copy())


_LAYER_RUNS = {}


def _layer_run(shape):
    """One forward + backward of the layer on the fixture with 4-D weights: (gradients, solution, w), computed once."""
    if shape not in _LAYER_RUNS:
        nx, nu, N = shape
        p = SF.problem(*shape)
        layer = LTVMPCLayer(nx, nu, N, SF.U_MAX, SF.X_MAX, K=p["K"], eps_abs=1e-6)
        t = _layer_inputs(p)
        u0, v = layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], None, c=t["c"], xref=t["xref"], uref=t["uref"])
        sol = _solution(layer)
        w = np.random.RandomState(9).randn(SF.B, nu)
        (u0 * torch.as_tensor(w, device=DEV)).sum().backward()
        _LAYER_RUNS[shape] = ({k: t[k].grad.cpu().numpy() for k in ("Ad", "Bd", "x0", "Q", "R")}, sol, w, p)
    return _LAYER_RUNS[shape]


@pytest.mark.parametrize("shape", SF.SHAPES)
def test_layer_gradients_match_the_numpy_chain(shape):
    nx, nu, N = shape
    grads, (x, y, act), w, p = _layer_run(shape)
    H, A, g, l, u = SF.condensed(p)
    for b in range(SF.B):                                       # the active set the device reports is the exact one, on every instance
        xe, ye, dist, mult = FX.margins(H[b], A[b], g[b], l[b], u[b], act[b])
        assert dist >= FX.MARGIN and mult >= FX.MARGIN, (b, dist, mult)
        assert (act[b] != 0).any(), b
        assert np.abs(xe - x[b]).max() <= 1e-5 * max(1.0, np.abs(xe).max()), b
    ref = SF.reference_gradients(p, x, y, act, w)
    assert grads["Q"].shape == (SF.B, N, nx, nx) and grads["R"].shape == (SF.B, N, nu, nu)
    for k in ("Q", "R"):
        assert np.array_equal(grads[k], np.swapaxes(grads[k], -1, -2)), k
    for k in ("Ad", "Bd", "x0", "Q", "R"):
        print("%s d/d%-4s max|err| %.3e, max|ref| %.3e" % (shape, k, np.abs(grads[k] - ref[k]).max(), np.abs(ref[k]).max()))
    for k in ("Ad", "Bd", "x0", "Q", "R"):
        _close(grads[k], ref[k], 1e-9)


def test_layer_weights_shared_over_the_batch_get_the_batch_sum():
    """[N, ., .] weights (float32 leaves beside float64 stages): the gradient has the input's shape and dtype and is the sum over
    the batch of the per-instance gradients of the same weights given as [B, N, ., .]."""
    shape = SF.SHAPES[0]
    nx, nu, N = shape
    p = SF.problem(*shape)
    Q3, R3 = p["Q"][2].astype(np.float32), p["R"][2].astype(np.float32)      # (float32 values: both runs see the same numbers)
    grads = {}
    for kind in ("N", "BN", "mixed"):
        layer = LTVMPCLayer(nx, nu, N, SF.U_MAX, SF.X_MAX, K=p["K"], eps_abs=1e-6)
        t = _layer_inputs(p, grad=())
        if kind == "BN":
            Q = torch.as_tensor(Q3, device=DEV, dtype=torch.float64).expand(SF.B, N, nx, nx).contiguous().requires_grad_()
            R_ = torch.as_tensor(R3, device=DEV, dtype=torch.float64).expand(SF.B, N, nu, nu).contiguous().requires_grad_()
        else:
            Q = torch.as_tensor(Q3, device=DEV).requires_grad_()
            R_ = torch.as_tensor(R3 if kind == "N" else np.broadcast_to(R3, (SF.B, N, nu, nu)).copy(), device=DEV).requires_grad_()
        u0, _ = layer(t["Ad"], t["Bd"], t["x0"], Q, R_, None, c=t["c"], xref=t["xref"], uref=t["uref"])
        w = torch.as_tensor(np.random.RandomState(9).randn(SF.B, nu), device=DEV)
        (u0 * w).sum().backward()
        grads[kind] = (Q.grad, R_.grad)
    gQ, gR = grads["N"]
    assert gQ.shape == (N, nx, nx) and gR.shape == (N, nu, nu) and gQ.dtype == torch.float32 and gR.dtype == torch.float32
    bQ, bR = grads["BN"]
    assert bQ.shape == (SF.B, N, nx, nx) and bQ.dtype == torch.float64
    assert bQ.abs().sum((1, 2, 3)).min().item() > 0             # every instance contributes
    _close(gQ.double().cpu().numpy(), bQ.sum(0).cpu().numpy(), 1e-6)         # (float32 rounding of the returned gradient)
    _close(gR.double().cpu().numpy(), bR.sum(0).cpu().numpy(), 1e-6)
    mQ, mR = grads["mixed"]
    assert mQ.shape == (N, nx, nx) and mR.shape == (SF.B, N, nu, nu)
    _close(mQ.double().cpu().numpy(), bQ.sum(0).cpu().numpy(), 1e-6)
    _close(mR.double().cpu().numpy(), bR.cpu().numpy(), 1e-6)


def test_gradcheck_of_the_condensing_alone():
    rs = np.random.RandomState(2)
    B, nx, nu, N = 2, 3, 1, 4
    m = N * (nx + nu)
    f64 = torch.float64
    tt = lambda a: torch.as_tensor(a, dtype=f64, device=DEV).requires_grad_()
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=1)
    Ad, Bd = tt(Ad0[None, None] + 0.1 * rs.randn(B, N, nx, nx)), tt(Bd0[None, None] + 0.1 * rs.randn(B, N, nx, nu))
    c, x0, xref, uref = tt(0.1 * rs.randn(B, N, nx)), tt(rs.randn(B, nx)), tt(0.3 * rs.randn(B, N, nx)), tt(0.1 * rs.randn(B, N, nu))
    Qs, Rs = SF.stage_weights(rs, B, N, nx, nu)
    l_add, u_add = tt(-np.ones(m) + 0.1 * rs.randn(m)), tt(np.ones(m) + 0.1 * rs.randn(m))
    cd = mpc.LTVCondenser(nx, nu, N, K=0.2 * rs.randn(nu, nx))
    fn = lambda Ad, Bd, c, x0, xref, uref, Q, R_, l_add, u_add: LTVCondenseFunction.apply(cd, Ad, Bd, c, x0, xref, uref, Q, R_, None,
                                                                                         l_add, u_add)
    assert torch.autograd.gradcheck(fn, (Ad, Bd, c, x0, xref, uref, tt(Qs), tt(Rs), l_add, u_add))
    assert torch.autograd.gradcheck(fn, (Ad, Bd, c, x0, xref, uref, tt(Qs[1]), tt(Rs), l_add, u_add))     # [N, ., .] beside [B, N, ., .]
    Qsh, Qf = tt(SF.spd_blocks(rs, (1,), nx)[0]), tt(2.0 * SF.spd_blocks(rs, (1,), nx)[0])
    mixed = lambda Ad, Bd, x0, Q, R_, Qf: LTVCondenseFunction.apply(cd, Ad, Bd, None, x0, None, None, Q, R_, Qf, l_add.detach(),
                                                                    u_add.detach())
    assert torch.autograd.gradcheck(mixed, (Ad, Bd, x0, Qsh, tt(Rs[0]), Qf))                              # a shared Q beside a staged R


def test_three_forwards_before_one_backward():
    """Three forwards with different stage weights share one forward workspace; each backward finds it overwritten by the later
    forwards and condenses its own saved stages and weights again: the gradients are those of single runs."""
    shape = SF.SHAPES[0]
    nx, nu, N = shape
    p = SF.problem(*shape)
    w = torch.as_tensor(np.random.RandomState(4).randn(SF.B, nu), device=DEV)
    factors = SF.FACTORS

    def inputs(f):
        t = _layer_inputs(SF.problem(*shape, factor=f), grad=("Ad", "x0"))
        return t, t["Q"].requires_grad_(), t["R"].requires_grad_()

    layer = LTVMPCLayer(nx, nu, N, SF.U_MAX, SF.X_MAX, K=p["K"], eps_abs=1e-6)
    runs, loss = [], 0.0
    for f in factors:
        t, Q, R_ = inputs(f)
        u0, _ = layer(t["Ad"], t["Bd"], t["x0"], Q, R_, None, c=t["c"], xref=t["xref"], uref=t["uref"])
        loss = loss + (u0 * w).sum()
        runs.append((t, Q, R_))
    loss.backward()
    for f, (t, Q, R_) in zip(factors, runs):
        single = LTVMPCLayer(nx, nu, N, SF.U_MAX, SF.X_MAX, K=p["K"], eps_abs=1e-6)
        t1, Q1, R1 = inputs(f)
        u0, _ = single(t1["Ad"], t1["Bd"], t1["x0"], Q1, R1, None, c=t1["c"], xref=t1["xref"], uref=t1["uref"])
        (u0 * w).sum().backward()
        for name, a, b in (("Q", Q, Q1), ("R", R_, R1), ("Ad", t["Ad"], t1["Ad"]), ("x0", t["x0"], t1["x0"])):
            print("factor %.1f d/d%-2s max|diff| %.3e, max|ref| %.3e" % (f, name, (a.grad - b.grad).abs().max().item(),
                                                                       b.grad.abs().max().item()))
            _close(a.grad.cpu().numpy(), b.grad.cpu().numpy(), 1e-9)
    assert not torch.equal(runs[0][1].grad, runs[1][1].grad)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_refusals():
    lib = _cabi.load()
    ref = ctypes.byref
    nx, nu, N, B = 4, 2, 5, 2
    flag = _cabi.LTV_STAGE_WEIGHTS
    d = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64, flags=flag)
    n, m = N * nu, N * (nx + nu)
    z = lambda *s: torch.zeros(s, device=DEV, dtype=torch.float64)
    Ad, Bd, x0, Q, R = z(B, N, nx, nx), z(B, N, nx, nu), z(B, nx), z(B, N, nx, nx), z(B, N, nu, nu)
    H, A, g, l, u, box = torch.ones(B, n, n, device=DEV, dtype=torch.float64), z(B, m, n), z(B, n), z(B, m), z(B, m), z(m)
    ws, adj = mpc.ltv_workspace(B, nx, nu, N, DEV), mpc.ltv_adjoint_workspace(B, nx, nu, N, DEV)
    dQ, dR, dQf = torch.ones(B, N, nx, nx, device=DEV, dtype=torch.float64), z(B, N, nu, nu), z(nx, nx)
    p = _cabi.ptr
    # Q or R NULL with the flag
    for q, r in ((None, p(R)), (p(Q), None)):
        assert lib.rqp_ltv_condense(ref(d), 0, p(Ad), p(Bd), None, q, r, None, None, p(H), p(A), p(ws), None) == _cabi.RQP_ERR_ARG
        assert lib.rqp_ltv_vectors(ref(d), 0, p(x0), None, None, p(box), p(box), q, r, None, p(ws), p(g), p(l), p(u), None) == _cabi.RQP_ERR_ARG
        assert len(lib.rqp_last_error(None)) > 0

    def io(**kw):
        s = _cabi.LtvAdjointIO()
        for name, t in dict(dict(Ad=Ad, Bd=Bd, x0=x0, Q=Q, R=R, workspace=ws, adjoint_workspace=adj, dQ=dQ, dR=dR), **kw).items():
            setattr(s, name, None if t is None else t.data_ptr())
        return s

    for missing in ("Q", "R"):
        assert lib.rqp_ltv_condense_adjoint(ref(d), 0, ref(io(**{missing: None})), None) == _cabi.RQP_ERR_ARG
    # dQf given with the flag
    assert lib.rqp_ltv_condense_adjoint(ref(d), 0, ref(io(dQf=dQf)), None) == _cabi.RQP_ERR_ARG
    assert b"dQf" in lib.rqp_last_error(None)
    # sizes beyond the limits, as before
    big = _cabi.LtvDims(batch=B, nx=17, nu=nu, horizon=N, dtype=_cabi.RQP_F64, flags=flag)
    assert lib.rqp_ltv_condense(ref(big), 0, p(Ad), p(Bd), None, p(Q), p(R), None, None, p(H), p(A), p(ws), None) == _cabi.RQP_ERR_UNSUPPORTED
    assert lib.rqp_ltv_condense_adjoint(ref(big), 0, ref(io()), None) == _cabi.RQP_ERR_UNSUPPORTED
    assert b"nx <= 16" in lib.rqp_last_error(None)
    torch.cuda.synchronize()
    assert torch.equal(H, torch.ones_like(H)) and torch.equal(dQ, torch.ones_like(dQ))      # nothing was launched
    # the same calls with Qf NULL and dQf NULL go through; the workspace sizes do not depend on the flag
    assert lib.rqp_ltv_condense(ref(d), 0, p(Ad), p(Bd), None, p(Q), p(R), None, None, p(H), p(A), p(ws), None) == 0
    assert lib.rqp_ltv_condense_adjoint(ref(d), 0, ref(io()), None) == 0
    assert lib.rqp_last_error(None) == b""
    d0 = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64, flags=0)
    for fn in (lib.rqp_ltv_workspace_bytes, lib.rqp_ltv_adjoint_workspace_bytes):
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        assert fn(ref(d), ref(a)) == 0 and fn(ref(d0), ref(b)) == 0 and a.value == b.value
    # the stage-constraint calls accept the flag and ignore it
    nc = 2
    E, A_c = z(B, N, nc, nu + nx), z(B, N * nc, n)
    assert lib.rqp_ltv_stage_rows(ref(d), 0, nc, p(E), p(ws), p(A_c), None) == 0
    torch.cuda.synchronize()
    assert not H.any()                                          # (zero stages and weights: H = 0 was written)
