"""Input-rate cost and bounds of batched LTV MPC, host side: reluqp.mpc.condense_ltv(S=) / ltv_vectors(uprev=) /
rate_constraints against a step-by-step rollout of the plant with its cost written out, the zero weight, the batch axis and
np.longdouble, the driver's fixture, and the argument errors of the driver and of the four C-ABI entry points (host-side
validation: no device is touched).  Runs without a GPU.

Tolerance of the identities: 1e-12 of the summed absolute values of the terms, the rule of tests/test_ltv_stage_cpu.py."""
import ctypes

import numpy as np
import pytest

from oracle import reluqp_oracle as O
from reluqp import _cabi, mpc

import ltv_rate_fixture as RF
import ltv_stage_cost_fixture as SC
import ltv_stage_fixture as SF


def _case(nx, nu, N, seed, full, s_form):
    rs = np.random.RandomState(seed)
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)
    P = dict(Ad=Ad0[None] + 0.05 * rs.randn(N, nx, nx), Bd=Bd0[None] + 0.05 * rs.randn(N, nx, nu),
             c=0.1 * rs.randn(N, nx) if full else None, x0=rs.randn(nx), K=0.2 * rs.randn(nu, nx) if full else None,
             xref=0.3 * rs.randn(N, nx) if full else None, uref=0.1 * rs.randn(N, nu) if full else None,
             uprev=rs.randn(nu), dlo=-0.5 - rs.rand(N * nu), dhi=0.5 + rs.rand(N * nu))
    Q, R = SC.stage_weights(rs, 1, N, nx, nu)
    P["Q"], P["R"] = Q[0], R[0]
    S = RF.rate_weights(rs, 1, N, nu)[0]
    P["S"] = S if s_form == "staged" else S[2]
    return P, rs


SHAPES = [(3, 1, 7), (7, 3, 9), (12, 4, 20)]


@pytest.mark.parametrize("s_form", ["staged", "shared"])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_cost_differences_equal_those_of_the_rolled_out_cost(shape, full, s_form):
    nx, nu, N = shape
    P, rs = _case(nx, nu, N, 3, full, s_form)
    cond = mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], None, K=P["K"], c=P["c"], S=P["S"])
    g, _, _ = mpc.ltv_vectors(cond, P["x0"], np.zeros(N * (nx + nu)), np.zeros(N * (nx + nu)), xref=P["xref"], uref=P["uref"],
                              uprev=P["uprev"])
    H = cond["H"]
    assert np.array_equal(H, H.T) and np.array_equal(cond["H_sp"], SC.dense_H_sp(P["Q"], P["R"]))
    Sk = P["S"] if P["S"].ndim == 3 else np.stack([P["S"]] * N)

    def J(v):
        us, xs = RF.rollout(P["Ad"], P["Bd"], P["K"], P["c"], P["x0"], v)
        return RF.rollout_cost(us, xs, P["Q"], P["R"], Sk, P["uprev"], xref=P["xref"], uref=P["uref"])

    for _ in range(3):
        va, vb = rs.randn(N * nu), rs.randn(N * nu)
        q = lambda v: 0.5 * v @ H @ v + g @ v
        qabs = lambda v: 0.5 * np.abs(v) @ np.abs(H) @ np.abs(v) + np.abs(g) @ np.abs(v)
        (Ja, Jaa), (Jb, Jba) = J(va), J(vb)
        scale = Jaa + Jba + qabs(va) + qabs(vb)
        rel = abs((q(va) - q(vb)) - (Ja - Jb)) / scale
        assert rel <= 1e-12, rel


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_rate_rows_are_the_rolled_out_input_differences(shape, full):
    nx, nu, N = shape
    P, rs = _case(nx, nu, N, 4, full, "staged")
    cond = mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], None, K=P["K"], c=P["c"])       # (the rows need no rate weight)
    A_r, l_r, u_r = mpc.rate_constraints(cond, P["x0"], P["uprev"], P["dlo"], P["dhi"])
    assert A_r.shape == (N * nu, N * nu) and l_r.shape == u_r.shape == (N * nu,)
    for _ in range(3):
        v = rs.randn(N * nu)
        us, _ = RF.rollout(P["Ad"], P["Bd"], P["K"], P["c"], P["x0"], v)
        prev = np.vstack([P["uprev"][None], us[:-1]])
        du = (us - prev).reshape(-1)
        scale = np.abs(A_r) @ np.abs(v) + np.abs(l_r - P["dlo"]) + (np.abs(us) + np.abs(prev)).reshape(-1)
        for lhs in (A_r @ v - (l_r - P["dlo"]), A_r @ v - (u_r - P["dhi"])):
            rel = np.abs(lhs - du) / scale
            assert rel.max() <= 1e-12, rel.max()
    for k in range(N - 1):                                      # right of the staircase: exact zeros
        assert not A_r[k * nu:(k + 1) * nu, (k + 1) * nu:].any()
    if not full:                                                # K = 0: u_k = v_k
        D = np.eye(N * nu) - np.eye(N * nu, k=-nu)
        assert np.array_equal(A_r, D)
    inf = mpc.rate_constraints(cond, P["x0"], P["uprev"], np.full(N * nu, -np.inf), np.full(N * nu, np.inf))
    assert np.all(inf[1] == -np.inf) and np.all(inf[2] == np.inf)


def test_zero_weight_leaves_the_condensing_unchanged():
    nx, nu, N = 7, 3, 9
    P, _ = _case(nx, nu, N, 5, True, "staged")
    box = np.zeros(N * (nx + nu))
    plain = mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], None, K=P["K"], c=P["c"])
    gl = mpc.ltv_vectors(plain, P["x0"], box, box, xref=P["xref"], uref=P["uref"])
    for S0 in (np.zeros((nu, nu)), np.zeros((N, nu, nu))):
        zero = mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], None, K=P["K"], c=P["c"], S=S0)
        for k in plain:
            assert np.array_equal(plain[k], zero[k]), k
        assert not zero["H_rate"].any()
        gz = mpc.ltv_vectors(zero, P["x0"], box, box, xref=P["xref"], uref=P["uref"], uprev=P["uprev"])
        for a, b in zip(gl, gz):
            assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="uprev"):
        mpc.ltv_vectors(zero, P["x0"], box, box)
    with pytest.raises(ValueError, match="uprev"):
        mpc.ltv_vectors(plain, P["x0"], box, box, uprev=P["uprev"])
    with pytest.raises(ValueError, match="S has shape"):
        mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], None, S=np.zeros((N + 1, nu, nu)))
    with pytest.raises(ValueError, match="batch axis"):
        mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], None, S=np.zeros((2, N, nu, nu)))


def test_batch_axis_and_longdouble():
    rs = np.random.RandomState(2)
    B, nx, nu, N = 3, 3, 2, 4
    Ad, Bd = rs.randn(B, N, nx, nx), rs.randn(B, N, nx, nu)
    Q, R = SC.stage_weights(rs, B, N, nx, nu)
    S = RF.rate_weights(rs, B, N, nu)
    x0, uprev = rs.randn(B, nx), rs.randn(B, nu)
    dlo, dhi = -rs.rand(B, N * nu), rs.rand(B, N * nu)
    box = np.zeros(N * (nx + nu))
    LD = np.longdouble
    for Sb in (S, S[0], S[0, 1]):                               # [B, N, ., .], [N, ., .], [., .]
        cond = mpc.condense_ltv(Ad, Bd, Q, R, None, S=Sb)
        g, _, _ = mpc.ltv_vectors(cond, x0, box, box, uprev=uprev)
        A_r, l_r, u_r = mpc.rate_constraints(cond, x0, uprev, dlo, dhi)
        assert cond["H"].shape == (B, N * nu, N * nu) and A_r.shape == (B, N * nu, N * nu) and l_r.shape == (B, N * nu)
        for b in range(B):
            one = mpc.condense_ltv(Ad[b], Bd[b], Q[b], R[b], None, S=Sb[b] if Sb.ndim == 4 else Sb)
            assert np.array_equal(one["H"], cond["H"][b])
            assert np.array_equal(mpc.ltv_vectors(one, x0[b], box, box, uprev=uprev[b])[0], g[b])
            for a, c in zip(mpc.rate_constraints(one, x0[b], uprev[b], dlo[b], dhi[b]), (A_r[b], l_r[b], u_r[b])):
                assert np.array_equal(a, c)
        wide = mpc.condense_ltv(Ad.astype(LD), Bd.astype(LD), Q.astype(LD), R.astype(LD), None, S=Sb.astype(LD))
        gw, _, _ = mpc.ltv_vectors(wide, x0.astype(LD), box, box, uprev=uprev.astype(LD))
        rw = mpc.rate_constraints(wide, x0.astype(LD), uprev.astype(LD), dlo.astype(LD), dhi.astype(LD))
        assert wide["H"].dtype == LD and gw.dtype == LD and all(a.dtype == LD for a in rw)
        assert np.abs(wide["H"].astype(np.float64) - cond["H"]).max() <= 1e-12 * np.abs(cond["H"]).max()
        assert np.abs(rw[1].astype(np.float64) - l_r).max() <= 1e-12 * (1 + np.abs(l_r).max())
    shared_lo = mpc.rate_constraints(cond, x0, uprev, dlo[0], dhi[0])
    assert np.array_equal(shared_lo[1][0], l_r[0])


def test_driver_fixture_has_active_rate_rows():
    p = RF.driver_problem()
    _, H, g, A, l, u = RF.driver_qp(p)
    assert A.shape == (SF.B, SF.N * (SF.NC + SF.NU), SF.N * SF.NU)
    ref = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-9, max_iter=20000)
    assert all(s == "solved" for s in ref["status"])
    active = RF.rate_active(ref["z"], ref["lam"], l, u)
    print("instances with an active rate row at the oracle's optimum: %d of %d" % (active.sum(), SF.B))
    assert active.sum() == 16                                   # (the number the fixture's docstring states)
    f32 = lambda a: a.astype(np.float32)
    r64 = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-3)
    r32 = O.solve_batch(f32(H), f32(g), f32(A), f32(l), f32(u), form="factored", eps_abs=1e-3, dtype=np.float32)
    assert np.array_equal(r32["iter"], r64["iter"])             # the float32 run of the driver test has a stable yardstick


def test_driver_argument_errors():
    nx, nu, N = 4, 2, 8
    Q, R = np.eye(nx), np.eye(nu)
    box = dict(u_max=1.0, x_max=5.0)
    with pytest.raises(ValueError, match="rate_weight has shape"):
        mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, rate_weight=np.eye(nu + 1), **box)
    with pytest.raises(ValueError, match="symmetric"):
        mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, rate_weight=np.array([[1.0, 0.5], [0.0, 1.0]]), **box)
    with pytest.raises(ValueError, match="du_max"):
        mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, du_max=-1.0, **box)
    with pytest.raises(ValueError, match="du_max"):
        mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, du_max=np.ones(nu + 1), **box)
    # (16, 4, 32): the box alone has m = 640 rows
    with pytest.raises(ValueError, match="640 base rows \\+ 128 rate rows"):
        mpc.BatchedLTVMPC(16, 4, 32, np.eye(16), np.eye(4), np.eye(16), du_max=1.0, **box)
    mpc.BatchedLTVMPC(16, 4, 32, np.eye(16), np.eye(4), np.eye(16), rate_weight=np.eye(4), **box)       # the cost alone fits
    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, du_max=[0.5, np.inf], rate_weight=np.eye(nu), **box)
    assert ctl.m == N * (nx + nu) + N * nu and ctl.m_base == N * (nx + nu) and ctl.rate_rows
    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, stage_rows=3, du_max=0.5)
    assert ctl.m == N * 3 + N * nu and ctl.m_base == N * 3
    plain = mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, **box)
    assert plain.m == plain.m_base == N * (nx + nu) and not plain.rate_rows
    for kw in (dict(u_prev=np.zeros((1, nu))), dict(du_lo=np.zeros(N * nu))):
        with pytest.raises(ValueError, match="need BatchedLTVMPC"):
            plain.qp_vectors(np.zeros((1, nx)), **kw)


def test_abi_names_and_host_side_validation():
    names = ("rqp_ltv_condense_rate", "rqp_ltv_vectors_rate", "rqp_ltv_rate_rows", "rqp_ltv_rate_bounds")
    for name in names:
        assert name in _cabi.ABI_SYMBOLS
    lib = _cabi.load()
    ref = ctypes.byref
    d = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)

    def calls(dims, stride_A=80 * 80, stride_l=80, only=(0, 1, 2, 3)):
        """(return code, rqp_last_error text) of the four calls with every pointer NULL."""
        p = None if dims is None else ref(dims)
        fns = (lambda: lib.rqp_ltv_condense_rate(p, 0, *([None] * 12)), lambda: lib.rqp_ltv_vectors_rate(p, 0, *([None] * 15)),
               lambda: lib.rqp_ltv_rate_rows(p, 0, None, None, stride_A, None),
               lambda: lib.rqp_ltv_rate_bounds(p, 0, None, None, None, None, None, None, None, stride_l, None))
        return [(fns[i](), lib.rqp_last_error(None)) for i in only]

    for (rc, err), name in zip(calls(d), names):
        assert rc == _cabi.RQP_ERR_ARG
        assert b"required" in err and name.encode() in err
    for rc, _ in calls(None):
        assert rc == _cabi.RQP_ERR_ARG
    big = _cabi.LtvDims(batch=4, nx=17, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)
    for rc, err in calls(big):
        assert rc == _cabi.RQP_ERR_UNSUPPORTED
        assert b"nx <= 16" in err
    for flags in (64, _cabi.LTV_STAGE_SHARED_E):
        bad = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=flags)
        for rc, err in calls(bad):
            assert rc == _cabi.RQP_ERR_ARG
            assert b"unknown flag" in err
    # the instance stride: at least the rate rows of one instance, at most m = 640 rows
    for rc, err in calls(d, stride_A=80 * 80 - 1, stride_l=79, only=(2, 3)):
        assert rc == _cabi.RQP_ERR_ARG
        assert b"inst_stride" in err
    for rc, err in calls(d, stride_A=641 * 80, stride_l=641, only=(2, 3)):
        assert rc == _cabi.RQP_ERR_UNSUPPORTED
        assert b"640" in err
    lim = _cabi.LtvDims(batch=4, nx=16, nu=4, horizon=32, dtype=_cabi.RQP_F64, flags=0)       # its box has m = 640 already
    for rc, _ in calls(lim, stride_A=(640 + 128) * 128, stride_l=640 + 128, only=(2, 3)):
        assert rc == _cabi.RQP_ERR_UNSUPPORTED
    nbytes = ctypes.c_size_t()
    assert lib.rqp_ltv_workspace_bytes(ref(d), ref(nbytes)) == 0
    assert nbytes.value == 8 * 4 * (2 * 320 * 80 + 320 * 13 + 80 * 13)             # the forward workspace is what it was
    assert lib.rqp_last_error(None) == b""
