"""Reverse mode of the LTV condensing, host side: reluqp.mpc.condense_ltv_vjp against central differences of condense_ltv +
ltv_vectors, its batch axis and its treatment of absent cotangents and of A's structural zeros, the C-ABI names and the
host-side validation of the two new entry points, LTVMPCLayer's argument errors, and the margins of the end-to-end fixture
(tests/ltv_adjoint_fixture.py) the GPU tests differentiate.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest

from oracle import reluqp_oracle as O
from reluqp import _cabi, mpc

import ltv_adjoint_fixture as FX

INPUTS = ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R", "Qf", "l_add", "u_add")


def _case(nx, nu, N, seed, full):
    rs = np.random.RandomState(seed)
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)

    def spd(k):
        W = rs.randn(k, k)
        return W @ W.T / k + np.eye(k)

    m = N * (nx + nu)
    P = dict(Ad=Ad0[None] + 0.05 * rs.randn(N, nx, nx), Bd=Bd0[None] + 0.05 * rs.randn(N, nx, nu), c=0.1 * rs.randn(N, nx),
             x0=rs.randn(nx), xref=0.3 * rs.randn(N, nx), uref=0.1 * rs.randn(N, nu), Q=spd(nx), R=spd(nu), Qf=spd(nx),
             l_add=-np.ones(m) + 0.1 * rs.randn(m), u_add=np.ones(m) + 0.1 * rs.randn(m))
    K = 0.2 * rs.randn(nu, nx) if full else None
    if not full:
        P["c"] = P["xref"] = P["uref"] = None
    return P, K, rs


def _forward(P, K):
    cond = mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], P["Qf"], K=K, c=P["c"])
    g, l, u = mpc.ltv_vectors(cond, P["x0"], P["l_add"], P["u_add"], xref=P["xref"], uref=P["uref"])
    return cond["H"], cond["A"], g, l, u


def _vjp(P, K, bars):
    return mpc.condense_ltv_vjp(P["Ad"], P["Bd"], P["Q"], P["R"], P["Qf"], P["x0"], P["l_add"], P["u_add"], K=K, c=P["c"],
                                xref=P["xref"], uref=P["uref"], **dict(zip(("dH", "dA", "dg", "dl", "du"), bars)))


@pytest.mark.parametrize("shape,full", [((3, 2, 4), True), ((5, 2, 6), False), ((12, 4, 20), True), ((3, 2, 4), False)])
def test_vjp_matches_central_differences(shape, full):
    nx, nu, N = shape
    P, K, rs = _case(nx, nu, N, 7, full)
    bars = [rs.randn(*o.shape) for o in _forward(P, K)]
    loss = lambda P: sum((b * o).sum() for b, o in zip(bars, _forward(P, K)))
    gr = _vjp(P, K, bars)
    h = 1e-5
    for name in INPUTS:
        d = rs.randn(*gr[name].shape)
        if name in ("Q", "R", "Qf"):
            d = d + d.T
        base = P[name] if P[name] is not None else np.zeros(gr[name].shape)      # an absent c / reference is zero
        Pp, Pm = dict(P), dict(P)
        Pp[name], Pm[name] = base + h * d, base - h * d
        fd = (loss(Pp) - loss(Pm)) / (2 * h)
        an = (gr[name] * d).sum()
        rel = abs(fd - an) / max(abs(fd), abs(an), 1e-300)
        print("%s %s %-6s fd % .9e  vjp % .9e  rel %.2e" % (shape, full, name, fd, an, rel))
        assert rel <= 1e-6, name


def test_batch_axis_stacks_instances_and_sums_shared_inputs():
    rs = np.random.RandomState(5)
    B, N, nx, nu = 3, 4, 3, 2
    n, m = N * nu, N * (nx + nu)
    Ad, Bd, c = rs.randn(B, N, nx, nx), rs.randn(B, N, nx, nu), rs.randn(B, N, nx)
    K = 0.1 * rs.randn(nu, nx)
    x0, xref = rs.randn(B, nx), rs.randn(B, N, nx)
    W = (np.eye(nx), np.eye(nu), 2 * np.eye(nx))
    bars = dict(dH=rs.randn(B, n, n), dA=rs.randn(B, m, n), dg=rs.randn(B, n), dl=rs.randn(B, m), du=rs.randn(B, m))
    la, ua = -np.ones(m), np.ones(m)
    full = mpc.condense_ltv_vjp(Ad, Bd, *W, x0, la, ua, K=K, c=c, xref=xref, **bars)
    ones = [mpc.condense_ltv_vjp(Ad[b], Bd[b], *W, x0[b], la, ua, K=K, c=c[b], xref=xref[b], **{k: v[b] for k, v in bars.items()})
            for b in range(B)]
    assert full["Ad"].shape == (B, N, nx, nx) and full["Q"].shape == (nx, nx) and full["l_add"].shape == (m,)
    for k in ("Ad", "Bd", "c", "x0", "xref", "uref"):
        assert np.array_equal(full[k][1], ones[1][k]), k
    for k in ("Q", "R", "Qf", "K", "l_add", "u_add"):
        assert np.allclose(full[k], sum(o[k] for o in ones), rtol=0, atol=1e-12 * np.abs(full[k]).max()), k
    assert np.array_equal(full["Q"], full["Q"].T) and np.array_equal(full["R"], full["R"].T)
    per = mpc.condense_ltv_vjp(Ad, Bd, *W, x0, np.tile(la, (B, 1)), np.tile(ua, (B, 1)), K=K, c=c, xref=xref, **bars)
    assert per["l_add"].shape == (B, m) and np.array_equal(per["l_add"], bars["dl"])


def test_absent_cotangents_are_zero_and_structural_zeros_of_dA_are_ignored():
    P, K, rs = _case(5, 2, 6, 3, True)
    nx, nu, N = 5, 2, 6
    outs = _forward(P, K)
    bars = [rs.randn(*o.shape) for o in outs]
    for keep in ((2,), (0, 1), (3, 4)):
        some = [b if i in keep else None for i, b in enumerate(bars)]
        zero = [b if i in keep else np.zeros_like(b) for i, b in enumerate(bars)]
        a, z = _vjp(P, K, some), _vjp(P, K, zero)
        for k in a:
            assert np.array_equal(a[k], z[k]), (keep, k)
    ref = _vjp(P, K, bars)
    junk = [b.copy() for b in bars]
    blk = nx + nu
    for j in range(1, N):                                       # block column j of F is zero above stage j
        junk[1][:j * blk, j * nu:(j + 1) * nu] = 1e3 * rs.randn(j * blk, nu)
    got = _vjp(P, K, junk)
    for k in ref:
        assert np.abs(got[k] - ref[k]).max() <= 1e-9 * max(1.0, np.abs(ref[k]).max()), k


def test_longdouble_inputs_keep_their_precision():
    P, K, rs = _case(3, 2, 4, 1, True)
    bars = [rs.randn(*o.shape) for o in _forward(P, K)]
    LD = np.longdouble
    Pl = {k: v.astype(LD) for k, v in P.items()}
    out = _vjp(Pl, K.astype(LD), [b.astype(LD) for b in bars])
    assert all(v.dtype == LD for v in out.values())
    ref = _vjp(P, K, bars)
    for k in ref:
        assert np.abs(out[k].astype(np.float64) - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), k


def test_abi_names_and_host_side_validation():
    for name in ("rqp_ltv_adjoint_workspace_bytes", "rqp_ltv_condense_adjoint"):
        assert name in _cabi.ABI_SYMBOLS
    lib = _cabi.load()
    nbytes, fwd = ctypes.c_size_t(), ctypes.c_size_t()
    d = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)
    assert lib.rqp_ltv_adjoint_workspace_bytes(ctypes.byref(d), ctypes.byref(nbytes)) == 0
    assert nbytes.value >= 8 * 4 * 320 * 80                      # at least one [m, n] float64 matrix per instance
    assert lib.rqp_ltv_workspace_bytes(ctypes.byref(d), ctypes.byref(fwd)) == 0
    assert fwd.value == 8 * 4 * (2 * 320 * 80 + 320 * 13 + 80 * 13)             # the forward workspace is what it was
    io = _cabi.LtvAdjointIO()
    # host-side validation: no device is touched
    assert lib.rqp_ltv_adjoint_workspace_bytes(None, ctypes.byref(nbytes)) == _cabi.RQP_ERR_ARG
    assert lib.rqp_ltv_condense_adjoint(None, 0, ctypes.byref(io), None) == _cabi.RQP_ERR_ARG
    big = _cabi.LtvDims(batch=4, nx=17, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)
    for rc in (lib.rqp_ltv_adjoint_workspace_bytes(ctypes.byref(big), ctypes.byref(nbytes)),
               lib.rqp_ltv_condense_adjoint(ctypes.byref(big), 0, ctypes.byref(io), None)):
        assert rc == _cabi.RQP_ERR_UNSUPPORTED
        assert b"nx <= 16" in lib.rqp_last_error(None)
    bad = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=64)
    assert lib.rqp_ltv_adjoint_workspace_bytes(ctypes.byref(bad), ctypes.byref(nbytes)) == _cabi.RQP_ERR_ARG
    assert lib.rqp_ltv_condense_adjoint(ctypes.byref(bad), 0, ctypes.byref(io), None) == _cabi.RQP_ERR_ARG
    assert b"unknown flag" in lib.rqp_last_error(None)
    assert lib.rqp_ltv_condense_adjoint(ctypes.byref(d), 0, ctypes.byref(io), None) == _cabi.RQP_ERR_ARG      # every pointer NULL
    assert lib.rqp_ltv_condense_adjoint(ctypes.byref(d), 0, None, None) == _cabi.RQP_ERR_ARG
    assert lib.rqp_ltv_adjoint_workspace_bytes(ctypes.byref(d), ctypes.byref(nbytes)) == 0
    assert lib.rqp_last_error(None) == b""


def test_layer_validates_arguments_before_any_gpu_call():
    import torch
    from reluqp.layer import LTVMPCLayer
    with pytest.raises(ValueError, match="unsupported LTV size"):
        LTVMPCLayer(17, 4, 20, 0.4, 8.0)
    with pytest.raises(ValueError, match="K has shape"):
        LTVMPCLayer(12, 4, 20, 0.4, 8.0, K=np.zeros((12, 4)))
    with pytest.raises(ValueError, match="K cannot require a gradient"):
        LTVMPCLayer(12, 4, 20, 0.4, 8.0, K=torch.zeros(4, 12, requires_grad=True))
    layer = LTVMPCLayer(3, 1, 4, 0.4, 8.0, K=np.zeros((1, 3)))
    f64 = torch.float64
    Ad, Bd, x0 = torch.zeros(2, 4, 3, 3, dtype=f64), torch.zeros(2, 4, 3, 1, dtype=f64), torch.zeros(2, 3, dtype=f64)
    Q, R = torch.eye(3, dtype=f64), torch.eye(1, dtype=f64)
    with pytest.raises(ValueError, match=r"\[B, N, nx, nx\]"):
        layer(Ad[0], Bd[0], x0, Q, R, Q)
    with pytest.raises(ValueError, match="stages of shape"):
        layer(Ad[:, :3], Bd[:, :3], x0, Q, R, Q)
    with pytest.raises(ValueError, match="x0 has shape"):
        layer(Ad, Bd, x0[:1], Q, R, Q)
    with pytest.raises(ValueError, match="c has shape"):
        layer(Ad, Bd, x0, Q, R, Q, c=torch.zeros(2, 4, 2, dtype=f64))
    with pytest.raises(ValueError, match="Q, Qf must be"):
        layer(Ad, Bd, x0, torch.eye(2, dtype=f64), R, Q)
    with pytest.raises(ValueError, match="symmetric"):
        layer(Ad, Bd, x0, torch.triu(torch.ones(3, 3, dtype=f64)), R, Q)
    with pytest.raises(ValueError, match="one precision"):
        layer(Ad, Bd.float(), x0, Q, R, Q)
    with pytest.raises(_cabi.RqpUnavailable):                    # host tensors: refused, never a CPU path
        layer(Ad, Bd, x0, Q, R, Q)


@pytest.mark.parametrize("shape", FX.SHAPES)
def test_fixture_has_active_sets_with_margins_on_every_instance(shape):
    nx, nu, N = shape
    n = N * nu
    p = FX.problem(*shape)
    H, A, g, l, u = FX.condensed(p)
    ref = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-6)
    assert all(s == "solved" for s in ref["status"])
    act = FX.classify(ref["z"], ref["lam"], l, u)
    nonempty = 0
    for b in range(FX.B):
        x, y, dist, mult = FX.margins(H[b], A[b], g[b], l[b], u[b], act[b])
        na = int((act[b] != 0).sum())
        err = np.abs(x - ref["x"][b]).max()
        print("%s instance %2d: %2d active rows, inactive distance %.2e, active |y| %.2e, |x_exact - x_oracle| %.1e"
              % (shape, b, na, dist, mult, err))
        assert err <= 1e-4 * max(1.0, np.abs(x).max())          # two orders above the oracle's eps_abs = 1e-6 exit
        assert dist >= FX.MARGIN and mult >= FX.MARGIN
        assert na <= n // 2
        nonempty += na > 0
    assert nonempty >= FX.B // 2
