"""Stage constraints of batched LTV MPC, host side: reluqp.mpc.stage_constraints against a step-by-step rollout of the plant,
the identity block against the box statement, stage_constraints_vjp composed with condense_ltv_vjp against central differences,
and the argument errors of the driver, the layer and the three C-ABI entry points (host-side validation: no device is touched).
Runs without a GPU."""
import ctypes

import numpy as np
import pytest

from reluqp import _cabi, mpc


def _case(nx, nu, N, nc, seed, full):
    rs = np.random.RandomState(seed)
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)

    def spd(k):
        W = rs.randn(k, k)
        return W @ W.T / k + np.eye(k)

    P = dict(Ad=Ad0[None] + 0.05 * rs.randn(N, nx, nx), Bd=Bd0[None] + 0.05 * rs.randn(N, nx, nu),
             c=0.1 * rs.randn(N, nx) if full else None, x0=rs.randn(nx), E=rs.randn(N, nc, nu + nx),
             lo=-np.ones(N * nc) + 0.1 * rs.randn(N * nc), hi=np.ones(N * nc) + 0.1 * rs.randn(N * nc),
             Q=spd(nx), R=spd(nu), Qf=spd(nx))
    K = 0.2 * rs.randn(nu, nx) if full else None
    return P, K, rs


def _forward(P, K):
    cond = mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], P["Qf"], K=K, c=P["c"])
    return cond, mpc.stage_constraints(cond, P["E"], P["x0"], P["lo"], P["hi"])


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("shape", [(3, 1, 7, 1), (7, 3, 9, 5), (12, 4, 20, 6)])
def test_stage_constraints_are_E_times_the_rolled_out_trajectory(shape, full):
    nx, nu, N, nc = shape
    P, K, rs = _case(nx, nu, N, nc, 3, full)
    cond, (A_c, l_c, u_c) = _forward(P, K)
    assert A_c.shape == (N * nc, N * nu) and l_c.shape == u_c.shape == (N * nc,)
    Kz = np.zeros((nu, nx)) if K is None else K
    cz = np.zeros((N, nx)) if P["c"] is None else P["c"]
    s = cond["G"] @ P["x0"] + cond["f"]
    for _ in range(3):
        v = rs.randn(N * nu)
        x, y = P["x0"].copy(), []
        for k in range(N):                                      # the plant, one step at a time
            u = -Kz @ x + v[k * nu:(k + 1) * nu]
            x = P["Ad"][k] @ x + P["Bd"][k] @ u + cz[k]
            y.append(np.hstack([u, x]))
        Ey = np.hstack([P["E"][k] @ y[k] for k in range(N)])
        absE = np.abs(P["E"]).reshape(N * nc, nu + nx)
        scale = (np.abs(A_c) @ np.abs(v) + (absE * np.repeat(np.abs(s).reshape(N, -1), nc, 0)).sum(1)
                 + (absE * np.repeat(np.abs(np.stack(y)), nc, 0)).sum(1))
        for lhs in (A_c @ v - (l_c - P["lo"]), A_c @ v - (u_c - P["hi"])):
            rel = np.abs(lhs - Ey) / scale
            assert rel.max() <= 1e-12, rel.max()
    for k in range(N - 1):                                      # right of the staircase: exact zeros
        assert not A_c[k * nc:(k + 1) * nc, (k + 1) * nu:].any()


@pytest.mark.parametrize("full", [False, True])
def test_identity_block_is_the_box(full):
    nx, nu, N = 7, 3, 9
    P, K, _ = _case(nx, nu, N, nx + nu, 5, full)
    P["E"] = np.tile(np.eye(nx + nu), (N, 1, 1))
    _, P["lo"], P["hi"] = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    cond, (A_c, l_c, u_c) = _forward(P, K)
    _, l, u = mpc.ltv_vectors(cond, P["x0"], P["lo"], P["hi"])
    assert np.array_equal(A_c, cond["F"]) and np.array_equal(l_c, l) and np.array_equal(u_c, u)


def test_batch_axis_and_longdouble():
    rs = np.random.RandomState(2)
    B, nx, nu, N, nc = 3, 3, 2, 4, 2
    Ad, Bd, c, x0 = 0.5 * rs.randn(B, N, nx, nx), rs.randn(B, N, nx, nu), rs.randn(B, N, nx), rs.randn(B, nx)
    W = (np.eye(nx), np.eye(nu), 2 * np.eye(nx))
    E, lo, hi = rs.randn(B, N, nc, nx + nu), -rs.rand(B, N * nc), rs.rand(N * nc)
    cond = mpc.condense_ltv(Ad, Bd, *W, c=c)
    A_c, l_c, u_c = mpc.stage_constraints(cond, E, x0, lo, hi)
    assert A_c.shape == (B, N * nc, N * nu) and l_c.shape == (B, N * nc)
    one = mpc.stage_constraints(mpc.condense_ltv(Ad[1], Bd[1], *W, c=c[1]), E[1], x0[1], lo[1], hi)
    assert all(np.array_equal(a[1], b) for a, b in zip((A_c, l_c, u_c), one))
    sh = mpc.stage_constraints(cond, E[0], x0, lo, hi)          # shared E
    assert np.array_equal(sh[0][0], A_c[0]) and not np.array_equal(sh[0][1], A_c[1])
    bars = (rs.randn(B, N * nc, N * nu), rs.randn(B, N * nc), rs.randn(B, N * nc))
    per = mpc.stage_constraints_vjp(cond, E, x0, *bars)
    assert per[2].shape == E.shape and np.array_equal(per[3], bars[1]) and np.array_equal(per[4], bars[2])
    shv = mpc.stage_constraints_vjp(cond, E[0], x0, *bars)
    assert shv[2].shape == E[0].shape                           # summed over the batch
    LD = np.longdouble
    condl = mpc.condense_ltv(Ad.astype(LD), Bd.astype(LD), *W, c=c.astype(LD))
    outl = mpc.stage_constraints(condl, E.astype(LD), x0.astype(LD), lo, hi) + mpc.stage_constraints_vjp(condl, E.astype(LD), x0, *bars)
    assert all(o.dtype == LD for o in outl)
    # an absent cotangent is a zero one
    some = mpc.stage_constraints_vjp(cond, E, x0, None, bars[1], None)
    zero = mpc.stage_constraints_vjp(cond, E, x0, np.zeros_like(bars[0]), bars[1], np.zeros_like(bars[2]))
    assert all(np.array_equal(a, b) for a, b in zip(some, zero))


@pytest.mark.parametrize("shape,full", [((3, 1, 7, 1), True), ((7, 3, 9, 5), False), ((12, 4, 20, 6), True), ((3, 2, 4, 3), False)])
def test_vjp_composed_with_the_condensing_vjp_matches_central_differences(shape, full):
    nx, nu, N, nc = shape
    P, K, rs = _case(nx, nu, N, nc, 7, full)
    cond, outs = _forward(P, K)
    bars = [rs.randn(*o.shape) for o in outs]
    bH, bg = rs.randn(N * nu, N * nu), rs.randn(N * nu)
    box = np.zeros(N * (nx + nu))

    def loss(P):
        cond, (A_c, l_c, u_c) = _forward(P, K)
        g, _, _ = mpc.ltv_vectors(cond, P["x0"], box, box)
        return (bars[0] * A_c).sum() + (bars[1] * l_c).sum() + (bars[2] * u_c).sum() + (bH * cond["H"]).sum() + (bg * g).sum()

    dA_full, dl_full, dE, dlo, dhi = mpc.stage_constraints_vjp(cond, P["E"], P["x0"], *bars)
    gr = mpc.condense_ltv_vjp(P["Ad"], P["Bd"], P["Q"], P["R"], P["Qf"], P["x0"], box, box, K=K, c=P["c"], dH=bH, dA=dA_full,
                              dg=bg, dl=dl_full, du=None)
    gr.update(E=dE, lo=dlo, hi=dhi)
    h = 1e-5
    for name in ("Ad", "Bd", "c", "x0", "E", "lo", "hi", "Q", "R", "Qf"):
        d = rs.randn(*gr[name].shape)
        if name in ("Q", "R", "Qf"):
            d = d + d.T
        base = P[name] if P[name] is not None else np.zeros(gr[name].shape)      # an absent c is zero
        Pp, Pm = dict(P), dict(P)
        Pp[name], Pm[name] = base + h * d, base - h * d
        fd = (loss(Pp) - loss(Pm)) / (2 * h)
        an = (gr[name] * d).sum()
        rel = abs(fd - an) / max(abs(fd), abs(an), 1e-300)
        print("%s %s %-3s fd % .9e  vjp % .9e  rel %.2e" % (shape, full, name, fd, an, rel))
        assert rel <= 1e-6, name


def test_driver_and_layer_argument_errors():
    import torch
    from reluqp.layer import LTVMPCLayer
    nx, nu, N = 4, 2, 8
    Q, R = np.eye(nx), np.eye(nu)
    with pytest.raises(ValueError, match="u_max and x_max must be None"):
        mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, u_max=0.4, stage_rows=3)
    with pytest.raises(ValueError, match="u_max and x_max must be None"):
        LTVMPCLayer(nx, nu, N, 0.4, 8.0, stage_rows=3)
    with pytest.raises(ValueError, match="u_max and x_max are required"):
        mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q)
    for nc in (0, 33):
        with pytest.raises(ValueError, match="1 <= nc <= 32"):
            mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, stage_rows=nc)
        with pytest.raises(ValueError, match="1 <= nc <= 32"):
            LTVMPCLayer(nx, nu, N, stage_rows=nc)
    with pytest.raises(ValueError, match="horizon nc <= 640"):
        mpc.BatchedLTVMPC(nx, nu, 32, Q, R, Q, stage_rows=21)     # 32 * 21 = 672
    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, stage_rows=3)
    assert ctl.m == 24 and ctl.n == 16
    Ad, Bd = np.zeros((5, N, nx, nx)), np.zeros((5, N, nx, nu))
    with pytest.raises(ValueError, match="first linearize\\(\\) needs E"):
        ctl.linearize(Ad, Bd)
    with pytest.raises(ValueError, match="E has shape"):
        ctl.linearize(Ad, Bd, E=np.zeros((5, N, 2, nx + nu)))
    with pytest.raises(ValueError, match="E has shape"):
        ctl.linearize(Ad, Bd, E=np.zeros((4, N, 3, nx + nu)))
    with pytest.raises(ValueError, match="first step\\(\\) needs lo and hi"):
        ctl.step(np.zeros((5, nx)))
    with pytest.raises(ValueError, match="first step\\(\\) needs lo and hi"):
        ctl.step(np.zeros((5, nx)), lo=np.zeros(24))
    box = mpc.BatchedLTVMPC(nx, nu, N, Q, R, Q, 0.4, 8.0)
    with pytest.raises(ValueError, match="stage_rows"):
        box.linearize(Ad, Bd, E=np.zeros((5, N, 3, nx + nu)))
    # the host statements and the device wrappers
    cond = mpc.condense_ltv(np.zeros((N, nx, nx)), np.zeros((N, nx, nu)), Q, R, Q)
    with pytest.raises(ValueError, match="E has shape"):
        mpc.stage_constraints(cond, np.zeros((N, 3, nx)), np.zeros(nx), np.zeros(24), np.zeros(24))
    with pytest.raises(ValueError, match="lo, hi have shapes"):
        mpc.stage_constraints(cond, np.zeros((N, 3, nx + nu)), np.zeros(nx), np.zeros(23), np.zeros(24))
    ws = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError, match="E has shape"):
        mpc.stage_rows_device((5, nx, nu, N), torch.zeros(5, N, 3, nx), ws)
    for nc in (0, 33):
        with pytest.raises(ValueError, match="1 <= nc <= 32"):
            mpc.stage_rows_device((5, nx, nu, N), torch.zeros(5, N, nc, nx + nu), ws)
    with pytest.raises(_cabi.RqpUnavailable):                    # host tensors: refused, never a CPU path
        mpc.stage_rows_device((5, nx, nu, N), torch.zeros(5, N, 3, nx + nu), ws)
    # the layer
    layer = LTVMPCLayer(nx, nu, N, stage_rows=3)
    f64 = torch.float64
    tA, tB, tx = torch.zeros(5, N, nx, nx, dtype=f64), torch.zeros(5, N, nx, nu, dtype=f64), torch.zeros(5, nx, dtype=f64)
    tQ, tR = torch.eye(nx, dtype=f64), torch.eye(nu, dtype=f64)
    E, lo, hi = torch.zeros(5, N, 3, nx + nu, dtype=f64), torch.zeros(24, dtype=f64), torch.zeros(24, dtype=f64)
    with pytest.raises(ValueError, match="E must be given"):
        layer(tA, tB, tx, tQ, tR, tQ)
    with pytest.raises(ValueError, match="hi must be given"):
        layer(tA, tB, tx, tQ, tR, tQ, E=E, lo=lo)
    with pytest.raises(ValueError, match="E has shape"):
        layer(tA, tB, tx, tQ, tR, tQ, E=E[:, :, :2], lo=lo, hi=hi)
    with pytest.raises(ValueError, match="lo has shape"):
        layer(tA, tB, tx, tQ, tR, tQ, E=E, lo=lo[:23], hi=hi)
    with pytest.raises(ValueError, match="both"):
        layer(tA, tB, tx, tQ, tR, tQ, E=E, lo=lo, hi=hi.expand(5, 24))
    with pytest.raises(ValueError, match="precision of Ad"):
        layer(tA, tB, tx, tQ, tR, tQ, E=E.float(), lo=lo, hi=hi)
    with pytest.raises(_cabi.RqpUnavailable):
        layer(tA, tB, tx, tQ, tR, tQ, E=E, lo=lo, hi=hi)
    with pytest.raises(ValueError, match="stage_rows"):
        LTVMPCLayer(nx, nu, N, 0.4, 8.0)(tA, tB, tx, tQ, tR, tQ, E=E, lo=lo, hi=hi)


def test_abi_names_and_host_side_validation():
    for name in ("rqp_ltv_stage_rows", "rqp_ltv_stage_vectors", "rqp_ltv_stage_adjoint"):
        assert name in _cabi.ABI_SYMBOLS
    assert _cabi.LTV_STAGE_SHARED_E == 32
    lib = _cabi.load()
    io = _cabi.LtvStageAdjointIO()
    d = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=_cabi.LTV_STAGE_SHARED_E)
    ref = ctypes.byref

    def calls(dims, nc):
        p = None if dims is None else ref(dims)
        return (lib.rqp_ltv_stage_rows(p, 0, nc, None, None, None, None),
                lib.rqp_ltv_stage_vectors(p, 0, nc, None, None, None, None, None, None, None, None),
                lib.rqp_ltv_stage_adjoint(p, 0, nc, ref(io), None))

    for rc in calls(d, 6):                                      # every pointer NULL
        assert rc == _cabi.RQP_ERR_ARG
        assert b"are required" in lib.rqp_last_error(None)
    assert lib.rqp_ltv_stage_adjoint(ref(d), 0, 6, None, None) == _cabi.RQP_ERR_ARG
    for rc in calls(None, 6):
        assert rc == _cabi.RQP_ERR_ARG
    for dims, nc in ((d, 0), (d, 33), (_cabi.LtvDims(batch=4, nx=12, nu=4, horizon=32, dtype=_cabi.RQP_F32, flags=0), 21)):
        for rc in calls(dims, nc):
            assert rc == _cabi.RQP_ERR_UNSUPPORTED
            assert b"nc <= 32" in lib.rqp_last_error(None) and b"<= 640" in lib.rqp_last_error(None)
    big = _cabi.LtvDims(batch=4, nx=17, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)
    for rc in calls(big, 6):                                    # the condensing's own limits hold too
        assert rc == _cabi.RQP_ERR_UNSUPPORTED
        assert b"nx <= 16" in lib.rqp_last_error(None)
    bad = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=64)
    for rc in calls(bad, 6):
        assert rc == _cabi.RQP_ERR_ARG
        assert b"unknown flag" in lib.rqp_last_error(None)
    # the new flag belongs to the new entry points alone
    nbytes = ctypes.c_size_t()
    aio = _cabi.LtvAdjointIO()
    for rc in (lib.rqp_ltv_workspace_bytes(ref(d), ref(nbytes)), lib.rqp_ltv_adjoint_workspace_bytes(ref(d), ref(nbytes)),
               lib.rqp_ltv_condense(ref(d), 0, *([None] * 11)), lib.rqp_ltv_vectors(ref(d), 0, *([None] * 13)),
               lib.rqp_ltv_condense_adjoint(ref(d), 0, ref(aio), None)):
        assert rc == _cabi.RQP_ERR_ARG
        assert b"unknown flag" in lib.rqp_last_error(None)
    d.flags = 0
    assert lib.rqp_ltv_workspace_bytes(ref(d), ref(nbytes)) == 0
    assert nbytes.value == 8 * 4 * (2 * 320 * 80 + 320 * 13 + 80 * 13)             # the forward workspace is what it was
    assert lib.rqp_last_error(None) == b""
