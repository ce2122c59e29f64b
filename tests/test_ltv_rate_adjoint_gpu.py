"""Reverse mode of the input-rate terms on the device (rqp_ltv_condense_adjoint_rate, reluqp.layer.LTVRateFunction /
LTVMPCLayer(rate_rows=), layer(S=, u_prev=, du_lo=, du_hi=)).

Kernel vs host, the rule of tests/test_ltv_gpu.py: the formulas are evaluated once in np.longdouble (the yardstick,
reluqp.mpc.condense_ltv_vjp with its rate keywords on longdouble inputs); e_host is the error of the float64 numpy evaluation
against it, per output, relative to `scale` = max|entry| of the same formulas evaluated on the absolute values of every term
(tests/ltv_rate_adjoint_ref.abs_scale).  float64 device outputs: e_dev <= 10 max(e_host, 2^-52); float32 outputs within 1
ulp(float32) of the rounded yardstick wherever |entry| >= 2^-24 scale.  Ratios are printed before they are asserted.

End to end (tests/ltv_rate_adjoint_ref.py): the layer's gradients of sum(w . u0) against the numpy chain at the device's own
solution, |err| <= 1e-9 (1 + max|ref|), on the box and on stage rows, with an active rate row on at least a quarter of the
instances."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from reluqp import _cabi, mpc
from reluqp.layer import LTVMPCLayer

import ltv_rate_adjoint_ref as RR
import ltv_rate_fixture as RF
import ltv_stage_fixture as SF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
BARS = ("dH", "dA", "dg", "dl", "du", "dA_r", "dl_r", "du_r")
# (nx, nu, N, B): nu = 1; odd sizes, nu not dividing 16; the workload's dims; nu = 8 (the padding limit) with n = 160 (the size
# limit, three waves); nx and N at their limits
SHAPES = [(3, 1, 7, 5), (7, 3, 9, 5), (12, 4, 20, 8), (12, 8, 20, 4), (16, 4, 32, 4)]
# opts -> (K, c and references; stage weights)
OPTS = dict(plain=(False, False), K_c_refs=(True, False), K_c_refs_staged=(True, True))


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV)


@functools.lru_cache(maxsize=None)
def _case(shape, f32, opts, seed=11):
    """The inputs as the device sees them (numpy); every cotangent random."""
    nx, nu, N, B = shape
    full, staged = OPTS[opts]
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)
    rs = np.random.RandomState(seed + 1)
    npt = np.float32 if f32 else np.float64
    rnd = lambda a: None if a is None else np.asarray(a).astype(npt)
    n, m = N * nu, N * (nx + nu)
    d = dict(Ad=rnd(Ad0[None, None] + 0.05 * rs.randn(B, N, nx, nx) / np.sqrt(nx)), Bd=rnd(Bd0[None, None] + 0.05 * rs.randn(B, N, nx, nu)),
             c=rnd(0.1 * rs.randn(B, N, nx)) if full else None, K=0.1 * rs.randn(nu, nx) if full else None, x0=rnd(rs.randn(B, nx)),
             xref=rnd(0.3 * rs.randn(B, N, nx)) if full else None, uref=rnd(0.1 * rs.randn(B, N, nu)) if full else None,
             uprev=rnd(0.5 * rs.randn(B, nu)), S=0.3 * RF.rate_weights(rs, B, N, nu),
             bars=[rnd(rs.randn(B, n, n)), rnd(rs.randn(B, m, n)), rnd(rs.randn(B, n)), rnd(rs.randn(B, m)), rnd(rs.randn(B, m)),
                   rnd(rs.randn(B, n, n)), rnd(rs.randn(B, n)), rnd(rs.randn(B, n))])
    if staged:
        d["Q"], d["R"], d["Qf"] = RF.SC.spd_blocks(rs, (B, N), nx, 1.0), RF.SC.spd_blocks(rs, (B, N), nu, 0.1), None
    else:
        d["Q"], d["R"] = np.diag(1.0 + rs.rand(nx)), 0.1 * np.eye(nu) + 0.01 * np.ones((nu, nu))
        d["Qf"] = 2.0 * d["Q"] + 0.1 * np.ones((nx, nx))
    d["dims"], d["staged"] = shape, staged
    return d


def _device(d, sl=slice(None), bars=range(8), want=None, ws=None, rate_ws=True, tails=False, over=None):
    """Condensing + rate adjoint of the instances `sl`; returns (dict of tensors, (forward workspace, adjoint workspace))."""
    nx, nu, N, _ = d["dims"]
    n, m = N * nu, N * (nx + nu)
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a[sl]), device=DEV)
    Ad, Bd, c, x0, xref, uref, uprev = (t(d[k]) for k in ("Ad", "Bd", "c", "x0", "xref", "uref", "uprev"))
    B = Ad.shape[0]
    w = (d["Q"][sl] if d["staged"] else d["Q"], d["R"][sl] if d["staged"] else d["R"], d["Qf"], d["K"])
    S = mpc.rate_weight_device(d["S"][sl], nu, N, B, DEV)
    if ws is None:
        ws = (mpc.ltv_workspace(B, nx, nu, N, DEV), mpc.ltv_adjoint_rate_workspace(B, nx, nu, N, DEV))
        mpc.condense_ltv_device(Ad, Bd, w, ws[0], c=c, S=S if rate_ws else None)
    cot = {k: (t(b) if i in bars else None) for i, (k, b) in enumerate(zip(BARS, d["bars"]))}
    cot.update(over or {})
    row0 = 0
    if tails:                                                   # the rate cotangents as the tails of [B, m + n, .] tensors
        row0 = m
        for k, shp in (("dA_r", (B, m + n, n)), ("dl_r", (B, m + n)), ("du_r", (B, m + n))):
            if cot[k] is not None:
                whole = torch.full(shp, 7.0, dtype=cot[k].dtype, device=DEV)
                whole[:, m:] = cot[k]
                cot[k] = whole
    out = mpc.condense_ltv_adjoint_rate_device(Ad, Bd, x0, w, ws[0], ws[1], S, uprev, xref=xref, uref=uref, row0=row0, want=want, **cot)
    return out, ws


def _host(d, b, dt, bars=None):
    at = lambda a: None if a is None else a[b].astype(dt)
    bars = d["bars"] if bars is None else bars
    nx, nu, N, _ = d["dims"]
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    st = d["staged"]
    return mpc.condense_ltv_vjp(at(d["Ad"]), at(d["Bd"]), at(d["Q"]) if st else d["Q"].astype(dt), at(d["R"]) if st else d["R"].astype(dt),
                                None if st else d["Qf"].astype(dt), at(d["x0"]), l_add, u_add,
                                K=None if d["K"] is None else d["K"].astype(dt), c=at(d["c"]), xref=at(d["xref"]), uref=at(d["uref"]),
                                S=at(d["S"]), uprev=at(d["uprev"]), **{k: at(v) for k, v in zip(BARS, bars)})


def _compare(worst, k, got, ref, host, scale):
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


@pytest.mark.parametrize("opts", list(OPTS))
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_match_host_vjp(shape, f32, opts):
    nx, nu, N, B = shape
    d = _case(shape, f32, opts)
    staged = d["staged"]
    out, _ = _device(d)
    idx = list(range(B)) if B <= 5 else sorted({0, 1, B // 2, B - 1})
    wnames = ("Q", "R") if staged else ("Q", "R", "Qf")
    sub = out if (staged or len(idx) == B) else _device(d, idx, want=wnames)[0]     # the batch sums of these instances alone
    torch.cuda.synchronize()
    dev = {k: v.cpu().numpy() for k, v in out.items()}
    dev_sub = {k: v.cpu().numpy() for k, v in sub.items()}
    npt = np.float32 if f32 else np.float64
    assert set(dev) == set(("Ad", "Bd", "c", "x0", "xref", "uref", "S", "uprev") + wnames)
    assert dev["Ad"].dtype == dev["uprev"].dtype == npt and dev["Q"].dtype == dev["S"].dtype == np.float64
    assert dev["S"].shape == (B, N, nu, nu) and dev["uprev"].shape == (B, nu)
    assert np.array_equal(dev["S"], np.swapaxes(dev["S"], -1, -2)), "every dS block must be bitwise symmetric"
    res, scales = {LD: {}, np.float64: {}}, {}
    for b in idx:
        for dt in (LD, np.float64):
            res[dt][b] = _host(d, b, dt)
        at64 = lambda a: None if a is None else a[b].astype(np.float64)
        scales[b] = RR.abs_scale(at64(d["Ad"]), at64(d["Bd"]), d["Q"][b] if staged else d["Q"], d["R"][b] if staged else d["R"], d["Qf"],
                                 d["K"], at64(d["c"]), at64(d["x0"]), at64(d["xref"]), at64(d["uref"]), d["S"][b], at64(d["uprev"]),
                                 [v[b].astype(np.float64) for v in d["bars"]])
    assert res[LD][idx[0]]["Ad"].dtype == LD and res[LD][idx[0]]["S"].dtype == LD
    worst = {}
    per = ("Ad", "Bd", "c", "x0", "xref", "uref", "S", "uprev") + (("Q", "R") if staged else ())
    for b in idx:
        for k in per:
            _compare(worst, k, dev[k][b], res[LD][b][k], res[np.float64][b][k], scales[b][k])
    if not staged:                                              # the batch sums (float64 whatever the precision of the inputs)
        for k in wnames:
            _compare(worst, k, dev_sub[k], sum(res[LD][b][k] for b in idx), sum(res[np.float64][b][k] for b in idx),
                     sum(scales[b][k] for b in idx))
    for k, w in worst.items():
        if len(w) == 3:
            print("rate adjoint f64 %s %s %s: e_dev / max(e_host, 2^-52) = %.3f (e_dev %.3e, e_host %.3e)" % (shape, opts, k, *w))
        else:
            print("rate adjoint f32 %s %s %s: max ulp distance from the rounded yardstick = %.3f" % (shape, opts, k, w[0]))
    for k, w in worst.items():
        assert w[0] <= (10.0 if len(w) == 3 else 1.0), (k, w)


@pytest.mark.parametrize("f32", [False, True])
def test_null_cotangents_staircase_garbage_strides_and_either_workspace(f32):
    d = _case((7, 3, 9, 5), f32, "K_c_refs")
    nx, nu, N, B = d["dims"]
    n = N * nu
    full, ws = _device(d)
    names = tuple(full)
    for keep in ((), (5,), (6,), (7,), (5, 7), (6, 7)):          # a NULL rate cotangent is a zero one, bitwise
        some, _ = _device(d, bars=(0, 1, 2, 3, 4) + keep, ws=ws)
        zero, _ = _device(dict(d, bars=[b if (i < 5 or i in keep) else np.zeros_like(b) for i, b in enumerate(d["bars"])]), ws=ws)
        for k in names:
            assert torch.equal(some[k], zero[k]), (keep, k)
    junk = [b.copy() for b in d["bars"]]                        # finite garbage in dA_r right of the staircase changes nothing
    right = np.arange(n)[None, :] >= ((np.repeat(np.arange(N), nu) + 1) * nu)[:, None]
    junk[5][:, right] = 1e6
    got, _ = _device(dict(d, bars=junk), ws=ws)
    for k in names:
        assert torch.equal(got[k], full[k]), k
    tail, _ = _device(d, ws=ws, tails=True)                     # the inst_stride form: the tails of [B, m + n, .] cotangents
    for k in names:
        assert torch.equal(tail[k], full[k]), k
    plain_ws, _ = _device(d, rate_ws=False)                     # the workspace of rqp_ltv_condense serves as well: the same bits
    for k in names:
        assert torch.equal(plain_ws[k], full[k]), k
    for want in (("S",), ("uprev",), ("x0", "uprev"), ("Ad", "S"), ("R", "S"), ("xref", "uref")):
        part, _ = _device(d, want=want, ws=ws)                  # a subset of the outputs is bitwise that of the full call
        assert tuple(part) == want
        for k in want:
            assert torch.equal(part[k], full[k]), (want, k)


@pytest.mark.parametrize("opts", ["K_c_refs", "K_c_refs_staged"])
@pytest.mark.parametrize("f32", [False, True])
def test_weight_gradients_are_bitwise_those_of_the_plain_adjoint(f32, opts):
    d = _case((7, 3, 9, 5), f32, opts)
    nx, nu, N, B = d["dims"]
    names = ("Q", "R") if d["staged"] else ("Q", "R", "Qf")
    rate, ws = _device(d, want=names, rate_ws=False)
    t = lambda a: None if a is None else torch.as_tensor(a, device=DEV)
    plain = mpc.condense_ltv_adjoint_device(t(d["Ad"]), t(d["Bd"]), t(d["x0"]), (d["Q"], d["R"], d["Qf"], d["K"]), ws[0], ws[1],
                                            xref=t(d["xref"]), uref=t(d["uref"]), want=names,
                                            **{k: t(b) for k, b in zip(BARS[:5], d["bars"])})
    for k in names:
        assert torch.equal(rate[k], plain[k]), k


@pytest.mark.parametrize("f32", [False, True])
def test_two_calls_and_a_graph_replay_are_bitwise_equal(f32):
    d = _case((12, 4, 20, 8), f32, "K_c_refs")
    nx, nu, N, B = d["dims"]
    Ad, Bd, c, x0, xref, uref, uprev = (_t(d[k]) for k in ("Ad", "Bd", "c", "x0", "xref", "uref", "uprev"))
    cot = {k: _t(b) for k, b in zip(BARS, d["bars"])}
    w = mpc._LtvWeights(nx, nu, d["Q"], d["R"], d["Qf"], d["K"])
    S = mpc.rate_weight_device(d["S"], nu, N, B, DEV)
    ws, adj = mpc.ltv_workspace(B, nx, nu, N, DEV), mpc.ltv_adjoint_rate_workspace(B, nx, nu, N, DEV)
    mpc.condense_ltv_device(Ad, Bd, w, ws, c=c, S=S)
    run = lambda: mpc.condense_ltv_adjoint_rate_device(Ad, Bd, x0, w, ws, adj, S, uprev, xref=xref, uref=uref, **cot)
    a, b = run(), run()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                   # (warm-up on the side stream, as torch's capture rules ask)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run()
    graph.replay()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(cap[k], a[k]), k


def test_abi_validation_on_the_device():
    lib = _cabi.load()
    nx, nu, N, B = 7, 3, 9, 5
    n, m = N * nu, N * (nx + nu)
    ref = ctypes.byref
    d = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64, flags=0)
    z = lambda *s: torch.zeros(s, device=DEV, dtype=torch.float64)
    ws, adj = mpc.ltv_workspace(B, nx, nu, N, DEV).zero_(), mpc.ltv_adjoint_rate_workspace(B, nx, nu, N, DEV)
    keep = dict(Ad=z(B, N, nx, nx), Bd=z(B, N, nx, nu), x0=z(B, nx), Q=z(nx, nx), R=z(nu, nu), Qf=z(nx, nx), workspace=ws,
                adjoint_workspace=adj, dg=z(B, n), dAd=z(B, N, nx, nx), dx0=z(B, nx) + 1, dQ=z(nx, nx), dR=z(nu, nu))
    rkeep = dict(S=z(B, N, nu, nu), uprev=z(B, nu), dl_r=z(B, n), dS=z(B, N, nu, nu) + 1, duprev=z(B, nu) + 1)

    def call(dims=d, skip=None, rskip=None, **rset):
        io, rio = _cabi.LtvAdjointIO(), _cabi.LtvRateAdjointIO()
        for k, t in keep.items():
            setattr(io, k, None if k == skip else t.data_ptr())
        for k, t in rkeep.items():
            setattr(rio, k, None if k == rskip else t.data_ptr())
        rio.dA_stride, rio.dl_stride = n * n, n
        for k, v in rset.items():
            setattr(rio, k, v)
        return lib.rqp_ltv_condense_adjoint_rate(ref(dims), 0, ref(io), ref(rio), None)

    before = torch.cuda.current_device()
    assert call() == 0
    assert lib.rqp_last_error(None) == b""
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == before                # the caller's device is what it was
    assert not keep["dx0"].any() and not rkeep["dS"].any() and not rkeep["duprev"].any()   # zero data: zero gradients, written
    for name in ("Ad", "Bd", "x0", "Q", "R", "Qf", "workspace", "adjoint_workspace"):
        assert call(skip=name) == _cabi.RQP_ERR_ARG, name
        assert b"are required" in lib.rqp_last_error(None)
    for name in ("S", "uprev"):
        assert call(rskip=name) == _cabi.RQP_ERR_ARG, name
        assert b"rate_io, S and uprev are required" in lib.rqp_last_error(None)
    for name in ("dl_r", "dS", "duprev"):                       # optional: NULL means zero / not wanted
        assert call(rskip=name) == 0, name
    for name in ("dg", "dAd", "dx0", "dQ", "dR"):
        assert call(skip=name) == 0, name
    flagged = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64, flags=_cabi.LTV_HAS_XREF)
    assert call(dims=flagged) == _cabi.RQP_ERR_ARG
    assert b"a flag names an input" in lib.rqp_last_error(None)
    assert call(dl_stride=n - 1) == _cabi.RQP_ERR_ARG
    assert call(dl_stride=641) == _cabi.RQP_ERR_UNSUPPORTED
    assert call(dl_stride=n - 1, rskip="dl_r") == 0             # a stride is checked only when one of its pointers is given
    io, rio = _cabi.LtvAdjointIO(), _cabi.LtvRateAdjointIO()
    assert lib.rqp_ltv_condense_adjoint_rate(ref(d), 7, ref(io), ref(rio), None) == _cabi.RQP_ERR_ARG   # (arguments first)
    for k, t in keep.items():
        setattr(io, k, t.data_ptr())
    rio.S, rio.uprev = rkeep["S"].data_ptr(), rkeep["uprev"].data_ptr()
    assert lib.rqp_ltv_condense_adjoint_rate(ref(d), 7, ref(io), ref(rio), None) < 0      # no such device
    assert b"no such HIP device" in lib.rqp_last_error(None)
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == before


# ------------------------------------------------------------------------------------------------------------------ layer
def _solution(layer):
    solver = next(iter(layer.qp._handles.values()))["solver"]
    r = solver.results
    return r.x.detach().cpu().numpy().copy(), r.y.detach().cpu().numpy().copy(), r.active.cpu().numpy().copy()


def _layer(p):
    if p["stage"]:
        return LTVMPCLayer(SF.NX, SF.NU, SF.N, K=p["K"], stage_rows=SF.NC, rate_rows=True, eps_abs=1e-6)
    return LTVMPCLayer(SF.NX, SF.NU, SF.N, SF.U_MAX, RR.X_MAX, K=p["K"], rate_rows=True, eps_abs=1e-6)


def _layer_inputs(p, shared=False):
    names = ("Ad", "Bd", "x0", "Q", "R", "Qf", "S", "uprev", "dlo", "dhi") + (("E", "lo", "hi") if p["stage"] else ())
    t = {k: torch.as_tensor(p[k], dtype=torch.float64, device=DEV) for k in names}
    if shared:
        t["S"], t["dlo"], t["dhi"] = t["S"][0, 0].clone(), t["dlo"][0].clone(), t["dhi"][0].clone()
    for k in names:
        if k not in ("Q", "R", "Qf"):
            t[k].requires_grad_()
    return t


def _run(layer, t, p):
    kw = dict(E=t["E"], lo=t["lo"], hi=t["hi"]) if p["stage"] else {}
    return layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], t["Qf"], S=t["S"], u_prev=t["uprev"], du_lo=t["dlo"], du_hi=t["dhi"], **kw)


def _close(got, ref, rel, what):
    got, ref = np.asarray(got), np.asarray(ref)
    err = np.abs(got - ref).max()
    print("%-5s max|err| %.3e, max|ref| %.3e" % (what, err, np.abs(ref).max()))
    return got.shape == ref.shape and err <= rel * (1 + np.abs(ref).max())


@pytest.mark.parametrize("stage", [False, True])
def test_layer_gradients_match_the_numpy_chain(stage):
    p = RR.layer_problem(stage)
    m0 = SF.N * SF.NC if stage else SF.N * (SF.NX + SF.NU)
    layer, t = _layer(p), _layer_inputs(p)
    u0, v = _run(layer, t, p)
    x, y, act = _solution(layer)
    assert act.shape == (SF.B, m0 + SF.N * SF.NU)
    n_act = int((act[:, m0:] != 0).any(1).sum())
    print("stage rows %s: instances with an active rate row at the device's optimum: %d of %d" % (stage, n_act, SF.B))
    assert n_act >= SF.B // 4                                   # the rate rows shape the gradients
    w = np.random.RandomState(9).randn(SF.B, SF.NU)
    (u0 * torch.as_tensor(w, device=DEV)).sum().backward()
    ref = RR.reference_gradients(p, x, y, act, w)
    names = RR.GRAD_NAMES + (("E", "lo", "hi") if stage else ())
    ok = [_close(t[k].grad.cpu().numpy(), ref[k], 1e-9, k) for k in names]
    assert all(ok), ok
    assert np.abs(ref["S"]).max() > 1e-4 and np.abs(ref["uprev"]).max() > 1e-3 and np.abs(ref["dhi"] + ref["dlo"]).max() > 1e-3
    # a shared S [nu, nu] and shared rate bounds [N nu]: the batch-and-stage sum, the batch sums
    ps = dict(p, S=np.tile(p["S"][:1, :1], (SF.B, SF.N, 1, 1)))
    layer2, ts = _layer(ps), _layer_inputs(ps, shared=True)
    u0, _ = _run(layer2, ts, ps)
    x, y, act = _solution(layer2)
    (u0 * torch.as_tensor(w, device=DEV)).sum().backward()
    refs = RR.reference_gradients(ps, x, y, act, w)
    ok = [_close(ts["S"].grad.cpu().numpy(), refs["S"].sum((0, 1)), 1e-9, "S"),
          _close(ts["dlo"].grad.cpu().numpy(), refs["dlo"].sum(0), 1e-9, "dlo"),
          _close(ts["dhi"].grad.cpu().numpy(), refs["dhi"].sum(0), 1e-9, "dhi")]
    ok += [_close(ts[k].grad.cpu().numpy(), refs[k], 1e-9, k) for k in ("Ad", "Bd", "x0", "uprev")]
    assert all(ok), ok


def test_cost_alone_and_rows_alone():
    p = RR.layer_problem(False)
    w = np.random.RandomState(9).randn(SF.B, SF.NU)
    # the rows alone: no S; the reference is the chain with S = 0
    layer, t = _layer(p), _layer_inputs(p)
    u0, _ = layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], t["Qf"], u_prev=t["uprev"], du_lo=t["dlo"], du_hi=t["dhi"])
    x, y, act = _solution(layer)
    (u0 * torch.as_tensor(w, device=DEV)).sum().backward()
    ref = RR.reference_gradients(dict(p, S=np.zeros_like(p["S"])), x, y, act, w)
    ok = [_close(t[k].grad.cpu().numpy(), ref[k], 1e-9, k) for k in ("Ad", "Bd", "x0", "uprev", "dlo", "dhi")]
    assert all(ok) and t["S"].grad is None, ok
    # the cost alone: no rate rows; the numpy QP without them
    layer = LTVMPCLayer(SF.NX, SF.NU, SF.N, SF.U_MAX, RR.X_MAX, K=p["K"], eps_abs=1e-6)
    t = _layer_inputs(p)
    u0, _ = layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], t["Qf"], S=t["S"], u_prev=t["uprev"])
    x, y, act = _solution(layer)
    m0 = SF.N * (SF.NX + SF.NU)
    assert act.shape == (SF.B, m0)
    (u0 * torch.as_tensor(w, device=DEV)).sum().backward()
    far = dict(p, dlo=np.full_like(p["dlo"], -1e3), dhi=np.full_like(p["dhi"], 1e3))       # rate rows that are never active
    pad = lambda a: np.concatenate([a, np.zeros((SF.B, SF.N * SF.NU), dtype=a.dtype)], 1)
    ref = RR.reference_gradients(far, x, pad(y), pad(act), w)
    ok = [_close(t[k].grad.cpu().numpy(), ref[k], 1e-9, k) for k in ("Ad", "Bd", "x0", "S", "uprev")]
    assert all(ok), ok
    with pytest.raises(ValueError, match="rate_rows=True"):
        layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], t["Qf"], S=t["S"], u_prev=t["uprev"], du_lo=t["dlo"], du_hi=t["dhi"])
    with pytest.raises(ValueError, match="need u_prev"):
        layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], t["Qf"], S=t["S"])


def test_three_forwards_before_one_backward_give_the_first_forwards_gradients():
    steps = [RR.layer_problem(True, step=s) for s in range(3)]
    layer = _layer(steps[0])
    w = torch.as_tensor(np.random.RandomState(9).randn(SF.B, SF.NU), device=DEV)
    ins = [_layer_inputs(p) for p in steps]
    outs, sols = [], []
    for t, p in zip(ins, steps):
        outs.append(_run(layer, t, p)[0])
        sols.append(_solution(layer))
    (outs[0] * w).sum().backward()                              # the workspace holds the third forward's linearisation
    ref = RR.reference_gradients(steps[0], *sols[0], w.cpu().numpy())
    ok = [_close(ins[0][k].grad.cpu().numpy(), ref[k], 1e-9, k) for k in RR.GRAD_NAMES + ("E", "lo", "hi")]
    assert all(ok), ok
    assert ins[1]["Ad"].grad is None and ins[2]["S"].grad is None
