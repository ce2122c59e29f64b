"""Input-rate cost and bounds of the LTV condensing on the device (rqp_ltv_condense_rate, rqp_ltv_vectors_rate,
rqp_ltv_rate_rows, rqp_ltv_rate_bounds) and the BatchedLTVMPC driver on top of them.

Kernel vs host, the rule of tests/test_ltv_gpu.py, tests/test_ltv_stage_gpu.py and tests/test_ltv_stage_cost_gpu.py unchanged:
the numpy statements (reluqp.mpc.condense_ltv(S=), ltv_vectors(uprev=), rate_constraints) are evaluated once in np.longdouble
(the yardstick); e_host is the error of their float64 evaluation against it, per output, relative to max|entry| of the output.
float64 device outputs: e_dev <= 10 max(e_host, 2^-52); float32 outputs within 1 ulp(float32) of the rounded yardstick wherever
|entry| >= 2^-24 of that scale.  The ratios are printed before they are asserted.  The inputs of a case are float32 numbers, so
that the float64 and the float32 run of it share one yardstick (computed once per case, never changed).  The rate weights
(tests/ltv_rate_fixture.py) differ for every (instance, stage) and grow with both.  The K != 0, x0 != 0 cases matter most: with
K = 0 the u rows of [G | f] are zero and a wrong first row of the [G | f] tiles of k_ltv_hess would not show."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reluqp_oracle as O
from reluqp import _cabi, mpc

import ltv_rate_fixture as RF
import ltv_stage_cost_fixture as SC
import ltv_stage_fixture as SF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
# (nx, nu, N, B): below one tile; stage boundaries off the 16-column tiles; many instances; nu = 8, n = 160; the size limit with
# two [G | f] tiles (cost only: its box already has m = 640 rows)
SHAPES = [(3, 1, 7, 5), (7, 3, 9, 5), (12, 4, 20, 64), (12, 8, 20, 4), (16, 4, 32, 4)]
COST_ONLY = (16, 4, 32, 4)
KEYS = ("H", "g", "A_r", "l_r", "u_r")

_CASES, _REFS = {}, {}


def _case(shape, opts, staged, seed=11):
    """Inputs of one kernel case (float32 numbers held in float64 arrays; the weights are float64 whatever the precision)."""
    key = (shape, opts, staged)
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
    x0, uprev = rs.randn(B, nx), 0.5 * rs.randn(B, nu)
    xref, uref = (0.3 * rs.randn(B, N, nx), 0.1 * rs.randn(B, N, nu)) if full else (None, None)
    dlo, dhi = -0.5 - rs.rand(n), 0.5 + rs.rand(n)
    if full:                                                    # per-instance bounds
        dlo, dhi = dlo[None] - rs.rand(B, n), dhi[None] + rs.rand(B, n)
    if staged:
        Q, R = SC.stage_weights(rs, B, N, nx, nu)
        Qf = None
    else:
        Q, R, Qf = SC.spd_blocks(rs, (1,), nx)[0], SC.spd_blocks(rs, (1,), nu, 0.1)[0], 2.5 * SC.spd_blocks(rs, (1,), nx)[0]
    S = RF.rate_weights(rs, B, N, nu)
    rnd = lambda a: None if a is None else np.asarray(a).astype(np.float32).astype(np.float64)
    d = dict(Ad=rnd(Ad), Bd=rnd(Bd), c=rnd(c), x0=rnd(x0), uprev=rnd(uprev), xref=rnd(xref), uref=rnd(uref), dlo=rnd(dlo),
             dhi=rnd(dhi), box=np.zeros(m), Q=Q, R=R, Qf=Qf, S=S, K=K, dims=shape)
    _CASES[key] = d
    return d


def _host(d, b, dt):
    """The numpy statements of instance b in dtype dt: dict of H, g, A_r, l_r, u_r."""
    at = lambda a: None if a is None else a[b].astype(dt)
    wt = lambda W: None if W is None else (W[b] if W.ndim == 4 else W).astype(dt)
    cond = mpc.condense_ltv(at(d["Ad"]), at(d["Bd"]), wt(d["Q"]), wt(d["R"]), wt(d["Qf"]),
                            K=None if d["K"] is None else d["K"].astype(dt), c=at(d["c"]), S=d["S"][b].astype(dt))
    g, _, _ = mpc.ltv_vectors(cond, at(d["x0"]), d["box"], d["box"], xref=at(d["xref"]), uref=at(d["uref"]), uprev=at(d["uprev"]))
    lo, hi = ((d["dlo"][b], d["dhi"][b]) if d["dlo"].ndim == 2 else (d["dlo"], d["dhi"]))
    A_r, l_r, u_r = mpc.rate_constraints(cond, at(d["x0"]), at(d["uprev"]), lo.astype(dt), hi.astype(dt))
    return dict(H=cond["H"], g=g, A_r=A_r, l_r=l_r, u_r=u_r)


def _reference(shape, opts, staged):
    """Per instance the yardstick (longdouble) and the float64 evaluation, computed once and shared."""
    key = (shape, opts, staged)
    if key not in _REFS:
        d = _case(shape, opts, staged)
        _REFS[key] = [(_host(d, b, LD), _host(d, b, np.float64)) for b in range(shape[3])]
        assert _REFS[key][0][0]["H"].dtype == LD and _REFS[key][0][0]["l_r"].dtype == LD
    return _REFS[key]


def _t(a, prec=None):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if prec is None else t.to(prec)


def _weights(d):
    return (d["Q"], d["R"], d["Qf"], d["K"])


def _device(d, prec, S=None, rows=True, ws=None):
    """The four device calls: dict of H, A, g, l, u (and A_r, l_r, u_r), and the workspace."""
    nx, nu, N, B = d["dims"]
    ws = mpc.ltv_workspace(B, nx, nu, N, DEV) if ws is None else ws
    S = mpc.rate_weight_device(d["S"], nu, N, B, DEV) if S is None else S
    H, A = mpc.condense_ltv_device(_t(d["Ad"], prec), _t(d["Bd"], prec), _weights(d), ws, c=_t(d["c"], prec), S=S)
    g, l, u = mpc.ltv_vectors_device((nx, nu, N, d["K"] is not None, d["c"] is not None), _t(d["x0"], prec), _t(d["box"], prec),
                                     _t(d["box"], prec), _weights(d), ws, xref=_t(d["xref"], prec), uref=_t(d["uref"], prec), S=S,
                                     uprev=_t(d["uprev"], prec))
    out = dict(H=H, A=A, g=g, l=l, u=u)
    if rows:
        out["A_r"] = mpc.rate_rows_device((B, nx, nu, N), ws, prec)
        out["l_r"], out["u_r"] = mpc.rate_bounds_device((B, nx, nu, N), _t(d["x0"], prec), _t(d["uprev"], prec), _t(d["dlo"], prec),
                                                        _t(d["dhi"], prec), ws)
    return out, ws


class _Worst(object):
    """The rule of the module docstring, per output name."""

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


@pytest.mark.parametrize("staged", [False, True], ids=["shared_weights", "stage_weights"])
@pytest.mark.parametrize("opts", ["plain", "K_c_refs"])
@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_match_host_formulas(shape, prec, opts, staged):
    nx, nu, N, B = shape
    d = _case(shape, opts, staged)
    n = N * nu
    rows = shape != COST_ONLY
    out, _ = _device(d, prec, rows=rows)
    torch.cuda.synchronize()
    dev = {k: v.cpu().numpy() for k, v in out.items()}
    npt = np.float32 if prec == torch.float32 else np.float64
    assert dev["H"].dtype == npt and dev["H"].shape == (B, n, n) and dev["g"].shape == (B, n)
    for b in range(B):
        assert np.array_equal(dev["H"][b], dev["H"][b].T), "H must be bitwise symmetric"
    keys = KEYS if rows else ("H", "g")
    if rows:
        assert dev["A_r"].shape == (B, n, n) and dev["l_r"].shape == dev["u_r"].shape == (B, n) and dev["A_r"].dtype == npt
        for k in range(N - 1):
            assert not dev["A_r"][:, k * nu:(k + 1) * nu, (k + 1) * nu:].any(), "A_r must be exactly zero right of the staircase"
        if d["K"] is None:                                      # u_k = v_k: the rows are [-I I]
            assert np.array_equal(dev["A_r"], np.broadcast_to(np.eye(n) - np.eye(n, k=-nu), (B, n, n)))
    worst = _Worst("LTV input rates %s %s %s" % (shape, opts, "staged" if staged else "shared"))
    for b, (ref, host) in enumerate(_reference(shape, opts, staged)):
        for k in keys:
            worst.add(k, dev[k][b], ref[k], host[k], float(np.abs(ref[k]).max()))
    worst.check()


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
def test_infinite_bounds_and_the_instance_stride(prec):
    """inf bounds come back inf; rows written into the tail of a larger tensor leave every other entry as it was."""
    shape = (7, 3, 9, 5)
    nx, nu, N, B = shape
    d = _case(shape, "K_c_refs", True)
    n = N * nu
    out, ws = _device(d, prec)
    dlo, dhi = d["dlo"].copy(), d["dhi"].copy()
    dlo[:, ::2], dhi[:, 1::3] = -np.inf, np.inf
    dlo[1, 3] = np.inf
    x0, up = _t(d["x0"], prec), _t(d["uprev"], prec)
    l_r, u_r = mpc.rate_bounds_device((B, nx, nu, N), x0, up, _t(dlo, prec), _t(dhi, prec), ws)
    fin_lo, fin_hi = torch.as_tensor(np.isfinite(dlo), device=DEV), torch.as_tensor(np.isfinite(dhi), device=DEV)
    assert torch.equal(l_r[fin_lo], out["l_r"][fin_lo]) and torch.equal(u_r[fin_hi], out["u_r"][fin_hi])
    assert torch.equal(l_r[~fin_lo], _t(dlo, prec)[~fin_lo]) and torch.equal(u_r[~fin_hi], _t(dhi, prec)[~fin_hi])
    # rows 4 .. 4 + n of [B, n + 9, ...] tensors: the gaps keep their bytes
    row0, mt = 4, n + 9
    A = torch.full((B, mt, n), 7.25, dtype=prec, device=DEV)
    l, u = torch.full((B, mt), -3.5, dtype=prec, device=DEV), torch.full((B, mt), 3.5, dtype=prec, device=DEV)
    assert mpc.rate_rows_device((B, nx, nu, N), ws, prec, A_r=A, row0=row0) is A
    mpc.rate_bounds_device((B, nx, nu, N), x0, up, _t(d["dlo"], prec), _t(d["dhi"], prec), ws, l_r=l, u_r=u, row0=row0)
    torch.cuda.synchronize()
    assert torch.equal(A[:, row0:row0 + n], out["A_r"]) and torch.equal(l[:, row0:row0 + n], out["l_r"])
    assert torch.equal(u[:, row0:row0 + n], out["u_r"])
    for t, v in ((A, 7.25), (l, -3.5), (u, 3.5)):
        assert (t[:, :row0] == v).all() and (t[:, row0 + n:] == v).all()
    with pytest.raises(ValueError, match="room for"):
        mpc.rate_rows_device((B, nx, nu, N), ws, prec, A_r=A, row0=10)


@pytest.mark.parametrize("staged", [False, True], ids=["shared_weights", "stage_weights"])
@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", [(7, 3, 9, 5), (12, 4, 20, 64), (16, 4, 32, 4)])
def test_zero_weight_gives_the_plain_calls_numbers(shape, prec, staged):
    nx, nu, N, B = shape
    d = _case(shape, "K_c_refs", staged)
    zero, _ = _device(d, prec, S=torch.zeros((B, N, nu, nu), dtype=torch.float64, device=DEV), rows=False)
    ws = mpc.ltv_workspace(B, nx, nu, N, DEV)
    H, A = mpc.condense_ltv_device(_t(d["Ad"], prec), _t(d["Bd"], prec), _weights(d), ws, c=_t(d["c"], prec))
    g, l, u = mpc.ltv_vectors_device((nx, nu, N, True, True), _t(d["x0"], prec), _t(d["box"], prec), _t(d["box"], prec), _weights(d),
                                     ws, xref=_t(d["xref"], prec), uref=_t(d["uref"], prec))
    torch.cuda.synchronize()
    for k, t in (("H", H), ("A", A), ("g", g), ("l", l), ("u", u)):
        assert torch.equal(zero[k], t), k
    nonzero, _ = _device(d, prec, rows=False)
    assert not torch.equal(nonzero["H"], H) and not torch.equal(nonzero["g"], g) and torch.equal(nonzero["A"], A)


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
def test_two_calls_and_a_graph_replay_are_bitwise_equal(prec):
    d = _case((12, 4, 20, 64), "K_c_refs", True)
    nx, nu, N, B = d["dims"]
    S = mpc.rate_weight_device(d["S"], nu, N, B, DEV)
    w = mpc._LtvStageWeights(nx, nu, N, d["Q"], d["R"], None, d["K"])
    w.on(DEV, B)                                                # (the expansion to device tensors happens outside the capture)
    ws = mpc.ltv_workspace(B, nx, nu, N, DEV)
    Ad, Bd, c, x0, xref, uref, up, box, dlo, dhi = (_t(d[k], prec) for k in ("Ad", "Bd", "c", "x0", "xref", "uref", "uprev", "box",
                                                                            "dlo", "dhi"))

    def run():
        H, A = mpc.condense_ltv_device(Ad, Bd, w, ws, c=c, S=S)
        g, l, u = mpc.ltv_vectors_device((nx, nu, N, True, True), x0, box, box, w, ws, xref=xref, uref=uref, S=S, uprev=up)
        A_r = mpc.rate_rows_device((B, nx, nu, N), ws, prec)
        l_r, u_r = mpc.rate_bounds_device((B, nx, nu, N), x0, up, dlo, dhi, ws)
        return dict(H=H, A=A, g=g, l=l, u=u, A_r=A_r, l_r=l_r, u_r=u_r)

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


def test_abi_rejects_each_missing_pointer_in_its_position():
    nx, nu, N, B = 7, 3, 9, 5
    n, m = N * nu, N * (nx + nu)
    lib = _cabi.load()
    before = torch.cuda.current_device()
    ref = ctypes.byref
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = mpc.ltv_workspace(B, nx, nu, N, DEV)
    Ad, Bd, Q, R, S, H, A = z(B, N, nx, nx), z(B, N, nx, nu), z(nx, nx), z(nu, nu), z(B, N, nu, nu), z(B, n, n), z(B, m, n)
    x0, up, lo, g, l = z(B, nx), z(B, nu), z(n), z(B, n), z(B, m)
    d = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64, flags=0)
    # rqp_ltv_condense_rate(dims, device, Ad, Bd, c, Q, R, Qf, K, S, H, A, workspace, stream): S is the 8th pointer
    good = [p(Ad), p(Bd), None, p(Q), p(R), p(Q), None, p(S), p(H), p(A), p(ws)]
    assert lib.rqp_ltv_condense_rate(ref(d), 0, *good, None) == 0
    for i in (0, 1, 3, 4, 5, 7, 8, 9, 10):
        args = list(good)
        args[i] = None
        assert lib.rqp_ltv_condense_rate(ref(d), 0, *args, None) == _cabi.RQP_ERR_ARG, i
        assert b"S, H, A and workspace are required" in lib.rqp_last_error(None)
    # rqp_ltv_vectors_rate(dims, device, x0, xref, uref, l_add, u_add, Q, R, Qf, S, uprev, workspace, g, l, u, stream)
    box, u = z(m), z(B, m)
    good = [p(x0), None, None, p(box), p(box), p(Q), p(R), p(Q), p(S), p(up), p(ws), p(g), p(l), p(u)]
    assert lib.rqp_ltv_vectors_rate(ref(d), 0, *good, None) == 0
    for i in (0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13):
        args = list(good)
        args[i] = None
        assert lib.rqp_ltv_vectors_rate(ref(d), 0, *args, None) == _cabi.RQP_ERR_ARG, i
        assert b"S, uprev, workspace" in lib.rqp_last_error(None)
    A_r, l_r, u_r = z(B, n, n), z(B, n), z(B, n)
    assert lib.rqp_ltv_rate_rows(ref(d), 0, p(ws), p(A_r), n * n, None) == 0
    for args in ((None, p(A_r)), (p(ws), None)):
        assert lib.rqp_ltv_rate_rows(ref(d), 0, *args, n * n, None) == _cabi.RQP_ERR_ARG
    # rqp_ltv_rate_bounds(dims, device, x0, uprev, dlo, dhi, workspace, l_r, u_r, inst_stride, stream)
    good = [p(x0), p(up), p(lo), p(lo), p(ws), p(l_r), p(u_r)]
    assert lib.rqp_ltv_rate_bounds(ref(d), 0, *good, n, None) == 0
    for i in range(7):
        args = list(good)
        args[i] = None
        assert lib.rqp_ltv_rate_bounds(ref(d), 0, *args, n, None) == _cabi.RQP_ERR_ARG, i
        assert b"uprev, dlo, dhi" in lib.rqp_last_error(None)
    assert lib.rqp_ltv_rate_rows(ref(d), 0, p(ws), p(A_r), n * n - 1, None) == _cabi.RQP_ERR_ARG
    assert lib.rqp_ltv_rate_rows(ref(d), 7, p(ws), p(A_r), n * n, None) < 0                  # no such device
    assert b"no such HIP device" in lib.rqp_last_error(None)
    # (16, 4, 32): the box has m = 640 rows, the rate rows do not fit behind it
    big = _cabi.LtvDims(batch=1, nx=16, nu=4, horizon=32, dtype=_cabi.RQP_F64, flags=0)
    wsb = mpc.ltv_workspace(1, 16, 4, 32, DEV)
    tail = z(1, 640 + 128, 128)
    assert lib.rqp_ltv_rate_rows(ref(big), 0, p(wsb), ctypes.c_void_p(tail.data_ptr() + 640 * 128 * 8), (640 + 128) * 128,
                                 None) == _cabi.RQP_ERR_UNSUPPORTED
    assert lib.rqp_ltv_rate_bounds(ref(big), 0, p(x0), p(up), p(lo), p(lo), p(wsb), p(tail), p(tail), 640 + 128,
                                   None) == _cabi.RQP_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="640 base rows"):
        mpc.BatchedLTVMPC(16, 4, 32, np.eye(16), np.eye(4), np.eye(16), u_max=1.0, x_max=5.0, du_max=0.5, device=DEV)
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == before


# ------------------------------------------------------------------------------------------------------------------ driver
def _driver(p, prec, **kw):
    ctl = mpc.BatchedLTVMPC(SF.NX, SF.NU, SF.N, p["Q"], p["R"], p["Qf"], K=p["K"], stage_rows=SF.NC, du_max=RF.DU_MAX, device=DEV,
                            precision=prec, **kw)
    return ctl, (lambda a: torch.as_tensor(a, device=DEV, dtype=prec))


def test_driver_end_to_end_with_stage_rows_rate_rows_and_rate_cost():
    """float64.  At the oracle's optimum of the numpy QP 16 of the 16 instances have an active rate row (computed below)."""
    import reluqp.reluqpth as reluqpth
    p = RF.driver_problem()
    cond, H, g, A, l, u = RF.driver_qp(p)
    ref = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-9, max_iter=20000)
    active = RF.rate_active(ref["z"], ref["lam"], l, u)
    print("instances with an active rate row at the oracle's optimum: %d of %d" % (active.sum(), SF.B))
    assert active.sum() >= SF.B // 2
    ctl, t = _driver(p, torch.float64, eps_abs=1e-6, polish=True)
    m0, n = SF.N * SF.NC, SF.N * SF.NU
    assert ctl.m == m0 + n
    ctl.linearize(t(p["Ad"]), t(p["Bd"]), E=t(p["E"]), S=p["S"])
    with pytest.raises(ValueError, match="needs u_prev"):
        ctl.step(t(p["x0"]), lo=t(p["lo"]), hi=t(p["hi"]))
    with pytest.raises(ValueError, match="u_prev has shape"):
        ctl.step(t(p["x0"]), lo=t(p["lo"]), hi=t(p["hi"]), u_prev=t(p["uprev"])[:, :1])
    u0, res = ctl.step(t(p["x0"]), lo=t(p["lo"]), hi=t(p["hi"]), u_prev=t(p["uprev"]))
    assert ctl.solver.QP.A.shape[-2] == m0 + n
    assert all(s == "solved" for s in res.info.status)
    direct = reluqpth.ReLU_QP()
    direct.setup(H, g, A, l, u, device=DEV, precision=torch.float64, eps_abs=1e-6, polish=True)
    xd = direct.solve().x.cpu().numpy()
    x = res.x.cpu().numpy()
    err = np.abs(x - xd).max()
    print("driver vs the numpy-assembled QP: max|x - x_direct| = %.3e, max|x| = %.3e, vs oracle %.3e; kernel %s"
          % (err, np.abs(xd).max(), np.abs(x - ref["x"]).max(), ctl.solver.kernel))
    assert err <= 1e-9 * (1 + np.abs(xd).max())
    u0n = u0.cpu().numpy()
    assert np.abs(u0n - (x[:, :SF.NU] - p["x0"] @ p["K"].T)).max() <= 1e-12
    assert np.all(np.abs(u0n - p["uprev"]) <= RF.DU_MAX + 1e-5)                    # the slew limit holds on the plant's input
    assert (np.abs(np.abs(u0n - p["uprev"]) - RF.DU_MAX) <= 1e-5).any(1).sum() >= SF.B // 2
    # a second step without u_prev starts from the first step's u0
    _, res1 = ctl.step(t(p["x0"]))
    _, _, g1, _, l1, u1 = RF.driver_qp(p, uprev=u0n)
    buf = ctl._buf
    for got, want in ((buf["l"], l1), (buf["u"], u1), (buf["g"], g1)):
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-12 * (1 + np.abs(want).max())
    assert np.abs(buf["l"][:, m0:m0 + SF.NU].cpu().numpy() - l1[:, m0:m0 + SF.NU]).max() <= 1e-12     # l_r of stage 0
    assert np.abs(l1[:, m0:m0 + SF.NU] - l[:, m0:m0 + SF.NU]).min() > 1e-3          # (and u0 is not the first u_prev)
    assert all(s == "solved" for s in res1.info.status)
    # replaced rate bounds and a new linearisation re-use the handle
    p2 = RF.driver_problem(step=1)
    ctl.linearize(t(p2["Ad"]), t(p2["Bd"]))
    _, res2 = ctl.step(t(p["x0"]), u_prev=t(p["uprev"]), du_lo=t(np.tile(2 * p["dlo"], (SF.B, 1))),
                       du_hi=t(np.tile(2 * p["dhi"], (SF.B, 1))))  # (per-instance bounds [B, N nu])
    q = dict(p, Ad=p2["Ad"], Bd=p2["Bd"], dlo=2 * p["dlo"], dhi=2 * p["dhi"])
    _, H2, g2, A2, l2, u2 = RF.driver_qp(q)
    direct.update(Hx=H2, Ax=A2)
    direct.update(g=g2, l=l2, u=u2)
    xd2 = direct.solve().x.cpu().numpy()
    assert np.abs(res2.x.cpu().numpy() - xd2).max() <= 1e-9 * (1 + np.abs(xd2).max())


def test_driver_float32_iterations_equal_the_oracles():
    p = RF.driver_problem()
    _, H, g, A, l, u = RF.driver_qp(p)
    f32 = lambda a: a.astype(np.float32)
    ref32 = O.solve_batch(f32(H), f32(g), f32(A), f32(l), f32(u), form="factored", eps_abs=1e-3, dtype=np.float32)
    ctl, t = _driver(p, torch.float32, eps_abs=1e-3)
    ctl.linearize(t(p["Ad"]), t(p["Bd"]), E=t(p["E"]), S=p["S"])
    u0, res = ctl.step(t(p["x0"]), lo=t(p["lo"]), hi=t(p["hi"]), u_prev=t(p["uprev"]))
    it = res.info.iter.cpu().numpy()
    print("device float32 iterations %s, oracle float32 %s, kernel %s" % (it, ref32["iter"], ctl.solver.kernel))
    assert res.info.status == ref32["status"]
    assert np.array_equal(it, ref32["iter"])
    scale = max(1.0, np.abs(ref32["x"]).max())
    np.testing.assert_allclose(res.x.cpu().double().numpy(), ref32["x"], rtol=0, atol=1e-4 * scale)


@pytest.mark.parametrize("rows,cost", [(True, True), (False, True), (True, False)])
def test_driver_on_the_box_builds_the_numpy_qp(rows, cost):
    """No stage_rows: the rate rows follow the box; the cost alone leaves m as it was.  (H, A, g, l, u) as the solver gets them."""
    nx, nu, N, B = 7, 3, 9, 5
    d = _case((nx, nu, N, B), "K_c_refs", False)
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    S = d["S"][0, 0]
    kw = dict(rate_weight=S) if cost else {}
    if rows:
        kw["du_max"] = [0.3, np.inf, 0.5]
    ctl = mpc.BatchedLTVMPC(nx, nu, N, d["Q"], d["R"], d["Qf"], u_max=0.4, x_max=8.0, K=d["K"], device=DEV, precision=torch.float64,
                            **kw)
    t = lambda a: torch.as_tensor(a, device=DEV, dtype=torch.float64)
    ctl.linearize(t(d["Ad"]), t(d["Bd"]), c=t(d["c"]))
    g, l, u = ctl.qp_vectors(t(d["x0"]), xref=t(d["xref"]), uref=t(d["uref"]), u_prev=t(d["uprev"]))
    cond = mpc.condense_ltv(d["Ad"], d["Bd"], d["Q"], d["R"], d["Qf"], K=d["K"], c=d["c"], S=S if cost else None)
    gn, ln, un = mpc.ltv_vectors(cond, d["x0"], l_add, u_add, xref=d["xref"], uref=d["uref"], uprev=d["uprev"] if cost else None)
    An = cond["A"]
    if rows:
        du = np.tile([0.3, np.inf, 0.5], N)
        A_r, l_r, u_r = mpc.rate_constraints(cond, d["x0"], d["uprev"], -du, du)
        An, ln, un = np.concatenate([An, A_r], 1), np.concatenate([ln, l_r], 1), np.concatenate([un, u_r], 1)
    assert tuple(ctl._buf["A"].shape) == An.shape and ctl.m == An.shape[1]
    for got, want in ((ctl._buf["H"], cond["H"]), (ctl._buf["A"], An), (g, gn), (l, ln), (u, un)):
        got = got.cpu().numpy()
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin], want[~fin])
        assert np.abs(got[fin] - want[fin]).max() <= 1e-12 * (1 + np.abs(want[fin]).max())
