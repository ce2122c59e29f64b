"""Stage constraints of batched LTV MPC on the device (rqp_ltv_stage_rows / rqp_ltv_stage_vectors / rqp_ltv_stage_adjoint,
BatchedLTVMPC(stage_rows=), reluqp.layer.StageConstraintFunction / LTVMPCLayer(stage_rows=)).

Kernel vs host, the rule of tests/test_ltv_gpu.py: the formulas are evaluated once in np.longdouble (the yardstick,
reluqp.mpc.stage_constraints / stage_constraints_vjp on longdouble inputs); e_host is the error of the float64 numpy evaluation
against it, per output, relative to `scale` = max|entry| of the same formulas evaluated on the absolute values of every term.
float64 device outputs: e_dev <= 10 max(e_host, 2^-52); float32 outputs within 1 ulp(float32) of the rounded yardstick wherever
|entry| >= 2^-24 scale.  Ratios are printed before they are asserted.

End to end (tests/ltv_stage_fixture.py): the driver's solution against ReLU_QP.setup on the QP the numpy statement assembles,
and the layer's gradients of sum(w . u0) against the numpy chain at the device's own solution, |err| <= 1e-9 (1 + max|ref|)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import reluqp_oracle as O
from reluqp import _cabi, mpc
from reluqp.layer import LTVMPCLayer

import ltv_stage_fixture as SF

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
# (nx, nu, N, nc, B): one row and the nu = 1 staircase; nothing a multiple of anything; the LTV shape of the benchmarks; both
# limits at once (nc = 32, m_c = 640, n = 160: three waves of columns, three outputs of dE per thread, three LDS chunks)
SHAPES = [(3, 1, 7, 1, 3), (7, 3, 9, 5, 5), (12, 4, 20, 6, 64), (16, 8, 20, 32, 4)]
# opts -> (K, c, per-instance E, batched bounds)
OPTS = dict(plain=(False, False, True, False), K=(True, False, False, True), K_c=(True, True, True, True))


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV)


@functools.lru_cache(maxsize=None)
def _case(shape, f32, opts, seed=11):
    """Inputs (the values the device sees), the device's outputs of the three entry points, and the instances to compare."""
    nx, nu, N, nc, B = shape
    has_K, has_c, e_batched, lu_batched = OPTS[opts]
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)
    rs = np.random.RandomState(seed + 1)
    npt = np.float32 if f32 else np.float64
    rnd = lambda a: None if a is None else np.asarray(a).astype(npt)
    n, m, mc, blk = N * nu, N * (nx + nu), N * nc, nx + nu
    d = dict(Ad=rnd(Ad0[None, None] + 0.05 * rs.randn(B, N, nx, nx) / np.sqrt(nx)), Bd=rnd(Bd0[None, None] + 0.05 * rs.randn(B, N, nx, nu)),
             c=rnd(0.1 * rs.randn(B, N, nx)) if has_c else None, K=0.1 * rs.randn(nu, nx) if has_K else None, x0=rnd(rs.randn(B, nx)),
             E=rnd(rs.randn(B, N, nc, blk) if e_batched else rs.randn(N, nc, blk)),
             lo=rnd(-1.0 - rs.rand(B, mc) if lu_batched else -1.0 - rs.rand(mc)),
             hi=rnd(1.0 + rs.rand(B, mc) if lu_batched else 1.0 + rs.rand(mc)),
             bars=[rnd(rs.randn(B, mc, n)), rnd(rs.randn(B, mc)), rnd(rs.randn(B, mc))])
    d["Q"], d["R"] = np.diag(1.0 + rs.rand(nx)), 0.1 * np.eye(nu) + 0.01 * np.ones((nu, nu))
    d["Qf"] = 2.0 * d["Q"]
    ws = mpc.ltv_workspace(B, nx, nu, N, DEV)
    _, A = mpc.condense_ltv_device(_t(d["Ad"]), _t(d["Bd"]), (d["Q"], d["R"], d["Qf"], d["K"]), ws, c=_t(d["c"]))
    dims4 = (B, nx, nu, N)
    A_c = mpc.stage_rows_device(dims4, _t(d["E"]), ws)
    l_c, u_c = mpc.stage_vectors_device(dims4, _t(d["E"]), _t(d["x0"]), _t(d["lo"]), _t(d["hi"]), ws)
    adj = mpc.stage_adjoint_device(dims4, _t(d["E"]), _t(d["x0"]), ws, *(_t(b) for b in d["bars"]))
    torch.cuda.synchronize()
    d["dev"] = {k: v.cpu().numpy() for k, v in dict(A_c=A_c, l_c=l_c, u_c=u_c, **adj).items()}
    d["idx"] = list(range(B)) if B <= 5 else sorted({0, 1, B // 2, B - 1})
    d["ws"], d["A_box"] = ws, A
    return d


def _host(d, b, dt):
    """The statements for instance b in dtype dt, and (dt = float64 only used) nothing else."""
    at = lambda a: None if a is None else a[b].astype(dt)
    per = lambda a, nd: (a[b] if a.ndim == nd else a).astype(dt)
    cond = mpc.condense_ltv(at(d["Ad"]), at(d["Bd"]), d["Q"].astype(dt), d["R"].astype(dt), d["Qf"].astype(dt),
                            K=None if d["K"] is None else d["K"].astype(dt), c=at(d["c"]))
    E, x0, lo, hi = per(d["E"], 4), at(d["x0"]), per(d["lo"], 2), per(d["hi"], 2)
    return cond, E, x0, lo, hi


def _staircase(N, rows_per_stage, nu, n):
    """Boolean [N rows_per_stage, n]: True left of the staircase (where block row k can be non-zero)."""
    k = np.repeat(np.arange(N), rows_per_stage)
    return np.arange(n)[None, :] < ((k + 1) * nu)[:, None]


def _yardsticks(d, b, shape):
    """{name: (longdouble, float64 host, scale)} of the six device outputs for instance b."""
    nx, nu, N, nc, _ = shape
    n, blk = N * nu, nx + nu
    res = {}
    for dt in (LD, np.float64):
        cond, E, x0, lo, hi = _host(d, b, dt)
        A_c, l_c, u_c = mpc.stage_constraints(cond, E, x0, lo, hi)
        dA_full, dl_full, dE, _, _ = mpc.stage_constraints_vjp(cond, E, x0, *(v[b].astype(dt) for v in d["bars"]))
        dA_full = np.where(_staircase(N, blk, nu, n), dA_full, 0)        # (right of it the kernel writes zeros: nothing reads them)
        res[dt] = dict(A_c=A_c, l_c=l_c, u_c=u_c, dA_full=dA_full, dl_full=dl_full, dE=dE)
    assert res[LD]["A_c"].dtype == LD and res[LD]["dE"].dtype == LD
    # the same formulas on absolute values
    cond, E, x0, lo, hi = _host(d, b, np.float64)
    aF, aE = np.abs(cond["F"]), np.abs(E)
    s_abs = np.abs(cond["G"]) @ np.abs(x0) + np.abs(cond["f"])
    bA, bl, bu = (np.abs(v[b].astype(np.float64)) for v in d["bars"])
    bA = np.where(_staircase(N, nc, nu, n), bA, 0)
    t = bl + bu
    Es = np.concatenate([aE[k] @ s_abs[k * blk:(k + 1) * blk] for k in range(N)])
    sc = dict(A_c=np.concatenate([aE[k] @ aF[k * blk:(k + 1) * blk] for k in range(N)]), l_c=np.abs(lo) + Es, u_c=np.abs(hi) + Es,
              dA_full=np.concatenate([aE[k].T @ bA[k * nc:(k + 1) * nc] for k in range(N)]),
              dl_full=np.concatenate([aE[k].T @ t[k * nc:(k + 1) * nc] for k in range(N)]),
              dE=np.stack([bA[k * nc:(k + 1) * nc] @ aF[k * blk:(k + 1) * blk].T
                           + np.outer(t[k * nc:(k + 1) * nc], s_abs[k * blk:(k + 1) * blk]) for k in range(N)]))
    return {k: (res[LD][k], res[np.float64][k], float(sc[k].max())) for k in sc}


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


def _check(d, shape, opts, names, what):
    worst = {}
    for b in d["idx"]:
        y = _yardsticks(d, b, shape)
        for k in names:
            _compare(worst, k, d["dev"][k][b], *y[k])
    for k, w in worst.items():
        if len(w) == 3:
            print("%s f64 %s %s %s: e_dev / max(e_host, 2^-52) = %.3f (e_dev %.3e, e_host %.3e)" % (what, shape, opts, k, *w))
        else:
            print("%s f32 %s %s %s: max ulp distance from the rounded yardstick = %.3f" % (what, shape, opts, k, w[0]))
    for k, w in worst.items():
        assert w[0] <= (10.0 if len(w) == 3 else 1.0), (k, w)


@pytest.mark.parametrize("opts", list(OPTS))
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_kernels_match_host_statement(shape, f32, opts):
    nx, nu, N, nc, B = shape
    d = _case(shape, f32, opts)
    dev = d["dev"]
    assert dev["A_c"].dtype == (np.float32 if f32 else np.float64) and dev["A_c"].shape == (B, N * nc, N * nu)
    assert dev["l_c"].shape == dev["u_c"].shape == (B, N * nc)
    right = ~_staircase(N, nc, nu, N * nu)
    assert not dev["A_c"][:, right].any(), "block row k of A_c must be exactly zero at the columns >= (k + 1) nu"
    _check(d, shape, opts, ("A_c", "l_c", "u_c"), "stage")


@pytest.mark.parametrize("opts", list(OPTS))
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint_kernel_matches_host_vjp(shape, f32, opts):
    nx, nu, N, nc, B = shape
    d = _case(shape, f32, opts)
    dev = d["dev"]
    assert dev["dA_full"].shape == (B, N * (nx + nu), N * nu) and dev["dl_full"].shape == (B, N * (nx + nu))
    assert dev["dE"].shape == (B, N, nc, nx + nu)               # per instance also for a shared E
    assert not dev["dA_full"][:, ~_staircase(N, nx + nu, nu, N * nu)].any()
    _check(d, shape, opts, ("dA_full", "dl_full", "dE"), "stage adjoint")


@pytest.mark.parametrize("f32", [False, True])
def test_structure_survives_any_E_and_infinite_bounds_stay_infinite(f32):
    shape = (7, 3, 9, 5, 5)
    nx, nu, N, nc, B = shape
    d = _case(shape, f32, "K_c")
    dims4 = (B, nx, nu, N)
    E = d["E"].copy()
    E[0, 0, 0, :] = np.inf                                      # an E that would turn 0 * E into NaN right of the staircase
    E[1, 2, 1, 0] = np.nan
    A_c = mpc.stage_rows_device(dims4, _t(E), d["ws"]).cpu().numpy()
    assert not A_c[:, ~_staircase(N, nc, nu, N * nu)].any()
    lo, hi = d["lo"].copy(), d["hi"].copy()
    lo[:, ::2], hi[:, 1::3], hi[0, 0] = -np.inf, np.inf, -np.inf
    l_c, u_c = (v.cpu().numpy() for v in mpc.stage_vectors_device(dims4, _t(d["E"]), _t(d["x0"]), _t(lo), _t(hi), d["ws"]))
    assert np.array_equal(np.isinf(l_c), np.isinf(lo)) and np.array_equal(np.isinf(u_c), np.isinf(hi))
    assert np.all(l_c[np.isinf(lo)] == -np.inf) and np.array_equal(u_c[np.isinf(hi)], hi[np.isinf(hi)])
    fin = np.isfinite(lo)
    assert np.array_equal(l_c[fin], d["dev"]["l_c"][fin])       # the finite ones are what they were


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", [(7, 3, 9, 5), (12, 4, 20, 64)])
def test_identity_block_reproduces_the_box_on_the_device(shape, f32):
    nx, nu, N, B = shape
    blk = nx + nu
    d = _case((nx, nu, N, 5 if N == 9 else 6, B), f32, "K_c")  # (its condensing: the workspace and the A = F it wrote)
    npt = np.float32 if f32 else np.float64
    w = (d["Q"], d["R"], d["Qf"], d["K"])
    E = np.tile(np.eye(blk, dtype=npt), (N, 1, 1))              # shared
    _, lo, hi = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    dims4 = (B, nx, nu, N)
    A_c = mpc.stage_rows_device(dims4, _t(E), d["ws"])
    assert A_c.dtype == d["A_box"].dtype
    assert torch.equal(A_c.view(torch.int32 if f32 else torch.int64), d["A_box"].view(torch.int32 if f32 else torch.int64))
    l_c, u_c = mpc.stage_vectors_device(dims4, _t(E), _t(d["x0"]), _t(lo.astype(npt)), _t(hi.astype(npt)), d["ws"])
    _, l, u = mpc.ltv_vectors_device((nx, nu, N, True, True), _t(d["x0"]), _t(lo.astype(npt)), _t(hi.astype(npt)), w, d["ws"])
    worst = {}
    for b in (list(range(B)) if B <= 5 else sorted({0, 1, B // 2, B - 1})):
        out = {}
        for dt in (LD, np.float64):
            cond, _, x0, _, _ = _host(d, b, dt)
            _, ll, uu = mpc.ltv_vectors(cond, x0, lo.astype(npt).astype(dt), hi.astype(npt).astype(dt))
            out[dt] = dict(l=ll, u=uu)
        s_abs = np.abs(cond["G"]) @ np.abs(x0) + np.abs(cond["f"])
        for k, got, box in (("l", l_c, l), ("u", u_c, u)):
            scale = float((np.abs(lo if k == "l" else hi) + s_abs).max())
            _compare(worst, k + "_c", got[b].cpu().numpy(), out[LD][k], out[np.float64][k], scale)
            _compare(worst, k, box[b].cpu().numpy(), out[LD][k], out[np.float64][k], scale)
    print("identity block %s f32=%s: %s" % (shape, f32, worst))
    for k, wv in worst.items():
        assert wv[0] <= (10.0 if len(wv) == 3 else 1.0), (k, wv)


def test_a_null_cotangent_is_a_zero_one_bitwise():
    shape = (7, 3, 9, 5, 5)
    nx, nu, N, nc, B = shape
    d = _case(shape, False, "K_c")
    dims4 = (B, nx, nu, N)
    run = lambda bars: mpc.stage_adjoint_device(dims4, _t(d["E"]), _t(d["x0"]), d["ws"], *(_t(b) for b in bars))
    for keep in ((0,), (1,), (2,), (1, 2), ()):
        some = run([b if i in keep else None for i, b in enumerate(d["bars"])])
        zero = run([b if i in keep else np.zeros_like(b) for i, b in enumerate(d["bars"])])
        for k in mpc.STAGE_ADJOINT_OUTPUTS:
            assert torch.equal(some[k], zero[k]), (keep, k)
    full = run(d["bars"])
    for want in (("dE",), ("dA_full",), ("dl_full", "dE")):      # a subset of the outputs is bitwise that of the full call
        part = mpc.stage_adjoint_device(dims4, _t(d["E"]), _t(d["x0"]), d["ws"], *(_t(b) for b in d["bars"]), want=want)
        assert tuple(part) == want
        for k in want:
            assert torch.equal(part[k], full[k]), (want, k)
    junk = [b.copy() for b in d["bars"]]                        # garbage right of the staircase of dA_c changes nothing
    junk[0][:, ~_staircase(N, nc, nu, N * nu)] = 1e6
    got = run(junk)
    for k in mpc.STAGE_ADJOINT_OUTPUTS:
        assert torch.equal(got[k], full[k]), k


@pytest.mark.parametrize("f32", [False, True])
def test_two_calls_and_a_graph_replay_are_bitwise_equal(f32):
    shape = (12, 4, 20, 6, 64)
    nx, nu, N, nc, B = shape
    d = _case(shape, f32, "K_c")
    dims4 = (B, nx, nu, N)
    E, x0, lo, hi = (_t(d[k]) for k in ("E", "x0", "lo", "hi"))
    bars = [_t(b) for b in d["bars"]]

    def run():
        A_c = mpc.stage_rows_device(dims4, E, d["ws"])
        l_c, u_c = mpc.stage_vectors_device(dims4, E, x0, lo, hi, d["ws"])
        return dict(A_c=A_c, l_c=l_c, u_c=u_c, **mpc.stage_adjoint_device(dims4, E, x0, d["ws"], *bars))

    a, b = run(), run()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert np.array_equal(a[k].cpu().numpy(), d["dev"][k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                   # (warm-up on the side stream, as torch's capture rules ask)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run()                                             # one stream, a linear chain of five kernels
    graph.replay()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(cap[k], a[k]), k


def test_abi_validation_on_the_device():
    lib = _cabi.load()
    nx, nu, N, nc, B = 7, 3, 9, 5, 5
    ref = ctypes.byref
    d = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64, flags=0)
    ws = mpc.ltv_workspace(B, nx, nu, N, DEV).zero_()
    E = torch.zeros(B, N, nc, nx + nu, device=DEV, dtype=torch.float64)
    x0 = torch.zeros(B, nx, device=DEV, dtype=torch.float64)
    lo = torch.zeros(N * nc, device=DEV, dtype=torch.float64)
    A_c = torch.empty(B, N * nc, N * nu, device=DEV, dtype=torch.float64)
    l_c, u_c = torch.empty(B, N * nc, device=DEV, dtype=torch.float64), torch.empty(B, N * nc, device=DEV, dtype=torch.float64)
    p = _cabi.ptr
    before = torch.cuda.current_device()
    assert lib.rqp_ltv_stage_rows(ref(d), 0, nc, p(E), p(ws), p(A_c), None) == 0
    assert lib.rqp_ltv_stage_vectors(ref(d), 0, nc, p(E), p(x0), p(lo), p(lo), p(ws), p(l_c), p(u_c), None) == 0
    assert lib.rqp_last_error(None) == b""
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == before                # the caller's device is what it was
    assert not A_c.any() and not l_c.any()
    for args in ((None, p(ws), p(A_c)), (p(E), None, p(A_c)), (p(E), p(ws), None)):
        assert lib.rqp_ltv_stage_rows(ref(d), 0, nc, *args, None) == _cabi.RQP_ERR_ARG
    good = [p(E), p(x0), p(lo), p(lo), p(ws), p(l_c), p(u_c)]
    for i in range(7):
        args = list(good)
        args[i] = None
        assert lib.rqp_ltv_stage_vectors(ref(d), 0, nc, *args, None) == _cabi.RQP_ERR_ARG
    for missing in ("E", "x0", "workspace"):
        io = _cabi.LtvStageAdjointIO()
        for name, t in (("E", E), ("x0", x0), ("workspace", ws), ("dl_full", torch.empty(B, N * (nx + nu), device=DEV, dtype=torch.float64))):
            setattr(io, name, None if name == missing else t.data_ptr())
        assert lib.rqp_ltv_stage_adjoint(ref(d), 0, nc, ref(io), None) == _cabi.RQP_ERR_ARG
        assert b"are required" in lib.rqp_last_error(None)
    assert lib.rqp_ltv_stage_rows(ref(d), 7, nc, p(E), p(ws), p(A_c), None) < 0          # no such device
    assert b"no such HIP device" in lib.rqp_last_error(None)
    for dims, k in ((d, 33), (_cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=32, dtype=_cabi.RQP_F64, flags=0), 21)):
        assert lib.rqp_ltv_stage_rows(ref(dims), 0, k, p(E), p(ws), p(A_c), None) == _cabi.RQP_ERR_UNSUPPORTED
        assert len(lib.rqp_last_error(None)) > 0 and b"nc <= 32" in lib.rqp_last_error(None)
    shared = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64, flags=_cabi.LTV_STAGE_SHARED_E)
    assert lib.rqp_ltv_stage_rows(ref(shared), 0, nc, p(E), p(ws), p(A_c), None) == 0
    nbytes = ctypes.c_size_t()
    assert lib.rqp_ltv_workspace_bytes(ref(shared), ref(nbytes)) == _cabi.RQP_ERR_ARG       # the old entry points refuse the flag
    assert lib.rqp_ltv_vectors(ref(shared), 0, *([p(ws)] * 13)) == _cabi.RQP_ERR_ARG
    assert b"unknown flag" in lib.rqp_last_error(None)
    torch.cuda.synchronize()
    assert torch.cuda.current_device() == before


def _driver(p, **kw):
    ctl = mpc.BatchedLTVMPC(SF.NX, SF.NU, SF.N, p["Q"], p["R"], p["Qf"], K=p["K"], stage_rows=SF.NC, device=DEV,
                            precision=torch.float64, eps_abs=1e-6, polish=True, **kw)
    t = lambda a: torch.as_tensor(a, device=DEV, dtype=torch.float64)
    return ctl, t


def test_driver_end_to_end_on_double_integrators_with_half_planes():
    import reluqp.reluqpth as reluqpth
    p = SF.problem()
    cond, H, g, A_c, l_c, u_c = SF.condensed(p)
    ref = O.solve_batch(H, g, A_c, l_c, u_c, form="factored", eps_abs=1e-9, max_iter=20000)
    assert all(s == "solved" for s in ref["status"])
    active = SF.halfplane_active(ref["z"], ref["lam"], u_c)
    print("instances with an active half-plane at the oracle's optimum: %d of %d" % (active.sum(), SF.B))
    assert active.sum() >= SF.B // 4
    ctl, t = _driver(p)
    with pytest.raises(ValueError, match="needs E"):
        ctl.linearize(t(p["Ad"]), t(p["Bd"]))
    ctl.linearize(t(p["Ad"]), t(p["Bd"]), E=t(p["E"]))
    with pytest.raises(ValueError, match="needs lo and hi"):
        ctl.step(t(p["x0"]))
    with pytest.raises(ValueError, match="lo has shape"):
        ctl.step(t(p["x0"]), lo=t(p["lo"])[:, :5], hi=t(p["hi"]))
    u0, res = ctl.step(t(p["x0"]), lo=t(p["lo"]), hi=t(p["hi"]))
    assert ctl.m == 24 and ctl.solver.QP.A.shape[-2] == 24
    assert ctl.solver.kernel != "generic", ctl.solver.kernel    # not the streaming kernel
    assert all(s == "solved" for s in res.info.status)
    direct = reluqpth.ReLU_QP()
    direct.setup(H, g, A_c, l_c, u_c, device=DEV, precision=torch.float64, eps_abs=1e-6, polish=True)
    rd = direct.solve()
    x, xd = res.x.cpu().numpy(), rd.x.cpu().numpy()
    err = np.abs(x - xd).max()
    print("driver vs the numpy-assembled QP: max|x - x_direct| = %.3e, max|x| = %.3e, vs oracle %.3e; kernel %s"
          % (err, np.abs(xd).max(), np.abs(x - ref["x"]).max(), ctl.solver.kernel))
    assert err <= 1e-9 * (1 + np.abs(xd).max())
    y = np.einsum("bij,bj->bi", cond["F"], x) + np.einsum("bij,bj->bi", cond["G"], p["x0"]) + cond["f"]
    Ey = np.einsum("bkci,bki->bkc", p["E"], y.reshape(SF.B, SF.N, -1)).reshape(SF.B, -1)
    assert np.all(Ey >= p["lo"] - 1e-5) and np.all(Ey <= p["hi"] + 1e-5)
    assert np.abs(u0.cpu().numpy() - (x[:, :SF.NU] - p["x0"] @ p["K"].T)).max() <= 1e-12
    assert np.all(np.abs(u0.cpu().numpy()) <= SF.U_MAX + 1e-5)  # E constrains the plant's input, K or not
    # the kept E and bounds serve the next step; a new linearisation re-factors the same handle
    u1, res1 = ctl.step(t(p["x0"]))
    assert np.abs(res1.x.cpu().numpy() - x).max() <= 1e-9 * (1 + np.abs(x).max())
    p2 = SF.problem(step=1)                                     # another linearisation of the same plants, the same states
    ctl.linearize(t(p2["Ad"]), t(p2["Bd"]))
    _, res2 = ctl.step(t(p["x0"]))
    assert all(s == "solved" for s in res2.info.status)
    q = dict(p, Ad=p2["Ad"], Bd=p2["Bd"])
    _, H2, g2, A2, l2, u2 = SF.condensed(q)
    direct.update(Hx=H2, Ax=A2)
    direct.update(g=g2, l=l2, u=u2)
    xd2 = direct.solve().x.cpu().numpy()
    assert np.abs(res2.x.cpu().numpy() - xd2).max() <= 1e-9 * (1 + np.abs(xd2).max())


def _solution(layer):
    solver = next(iter(layer.qp._handles.values()))["solver"]
    r = solver.results
    return r.x.detach().cpu().numpy().copy(), r.y.detach().cpu().numpy().copy(), r.active.cpu().numpy().copy()


def _layer_inputs(p, shared=False):
    t = {k: torch.as_tensor(p[k], dtype=torch.float64, device=DEV) for k in ("Ad", "Bd", "x0", "E", "lo", "hi", "Q", "R", "Qf")}
    if shared:
        t["E"], t["lo"], t["hi"] = t["E"][0].clone(), t["lo"][0].clone(), t["hi"][0].clone()
    for k in ("Ad", "Bd", "x0", "E", "lo", "hi"):
        t[k].requires_grad_()
    return t


def _close(got, ref, rel, what):
    got, ref = np.asarray(got), np.asarray(ref)
    err = np.abs(got - ref).max()
    print("%-3s max|err| %.3e, max|ref| %.3e" % (what, err, np.abs(ref).max()))
    return err <= rel * (1 + np.abs(ref).max())


def test_layer_gradients_match_the_numpy_chain():
    p = SF.problem()
    layer = LTVMPCLayer(SF.NX, SF.NU, SF.N, K=p["K"], stage_rows=SF.NC, eps_abs=1e-6)
    t = _layer_inputs(p)
    u0, v = layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], t["Qf"], E=t["E"], lo=t["lo"], hi=t["hi"])
    x, y, act = _solution(layer)
    w = np.random.RandomState(9).randn(SF.B, SF.NU)
    (u0 * torch.as_tensor(w, device=DEV)).sum().backward()
    ref = SF.reference_gradients(p, x, y, act, w)
    assert (act[:, 2::SF.NC] != 0).any(1).sum() >= SF.B // 4    # the half-planes shape the gradients
    ok = [_close(t[k].grad.cpu().numpy(), ref[k], 1e-9, k) for k in ("E", "lo", "hi", "Ad", "Bd", "x0")]
    assert all(ok), ok
    assert np.abs(ref["E"]).max() > 1e-3 and np.abs(ref["hi"]).max() > 1e-3
    # a shared E and shared bounds: their gradients are the batch sums
    ps = dict(p, E=np.tile(p["E"][:1], (SF.B, 1, 1, 1)), lo=np.tile(p["lo"][:1], (SF.B, 1)), hi=np.tile(np.full_like(p["hi"][:1], 5.0), (SF.B, 1)))
    ps["hi"][:, 0::SF.NC] = ps["hi"][:, 1::SF.NC] = SF.U_MAX
    ts = _layer_inputs(ps, shared=True)
    layer2 = LTVMPCLayer(SF.NX, SF.NU, SF.N, K=p["K"], stage_rows=SF.NC, eps_abs=1e-6)
    u0, _ = layer2(ts["Ad"], ts["Bd"], ts["x0"], ts["Q"], ts["R"], ts["Qf"], E=ts["E"], lo=ts["lo"], hi=ts["hi"])
    x, y, act = _solution(layer2)
    (u0 * torch.as_tensor(w, device=DEV)).sum().backward()
    refs = SF.reference_gradients(ps, x, y, act, w)
    assert ts["E"].grad.shape == ts["E"].shape and ts["lo"].grad.shape == ts["lo"].shape
    ok = [_close(ts[k].grad.cpu().numpy(), refs[k].sum(0), 1e-9, k) for k in ("E", "lo", "hi")]
    ok += [_close(ts[k].grad.cpu().numpy(), refs[k], 1e-9, k) for k in ("Ad", "Bd", "x0")]
    assert all(ok), ok


def test_three_forwards_before_one_backward_give_the_first_forwards_gradients():
    steps = [SF.problem(step=s) for s in range(3)]
    K = steps[0]["K"]
    layer = LTVMPCLayer(SF.NX, SF.NU, SF.N, K=K, stage_rows=SF.NC, eps_abs=1e-6)
    w = torch.as_tensor(np.random.RandomState(9).randn(SF.B, SF.NU), device=DEV)
    ins = [_layer_inputs(p) for p in steps]
    outs, sols = [], []
    for t in ins:
        u0, _ = layer(t["Ad"], t["Bd"], t["x0"], t["Q"], t["R"], t["Qf"], E=t["E"], lo=t["lo"], hi=t["hi"])
        outs.append(u0)
        sols.append(_solution(layer))
    (outs[0] * w).sum().backward()                              # the workspace holds the third forward's linearisation
    ref = SF.reference_gradients(steps[0], *sols[0], w.cpu().numpy())
    ok = [_close(ins[0][k].grad.cpu().numpy(), ref[k], 1e-9, k) for k in ("E", "lo", "hi", "Ad", "Bd", "x0")]
    assert all(ok), ok
    assert ins[1]["Ad"].grad is None and ins[2]["E"].grad is None
