"""CPU checks of the forward sensitivities (include/rqp_abi.h: rqp_set_sensitivity / rqp_sensitivity; ReLU_QP.jvp;
QPFunction.jvp; LinearMPC.feedback_gain): the boundary declares and exports both entry points with the struct's fields, the
host-only argument checks hold, the Python surface exists, and the numpy restatement (tests/sensitivity_ref.py) -- the
specification the GPU kernels are tested against (tests/test_sensitivity_gpu.py) -- agrees with finite differences of exact
solves, with the adjoint through the duality identity, and with the LQR gain on an unconstrained MPC problem."""
import ctypes
import inspect
import os
import re

import numpy as np
import torch

from reluqp import _cabi, mpc

import adjoint_ref as R
import sensitivity_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("H", "A", "l", "u", "x", "z", "y", "status", "active", "ndir", "shared_tangents", "dH", "dg", "dA", "dl", "du",
          "dx", "dy", "dz", "active_out", "sens_status", "sens_res")


def test_sensitivity_symbols_declared_exported_listed():
    src = open(os.path.join(REPO, "include", "rqp_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+rqp_set_sensitivity\s*\(\s*rqp_handle\s*\*\s*h\s*,\s*int32_t\s+enable\s*\)", src)
    assert re.search(r"int\s+rqp_sensitivity\s*\(\s*rqp_handle\s*\*\s*h\s*,\s*const\s+rqp_sensitivity_io\s*\*\s*io\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", src)
    body = re.search(r"typedef\s+struct\s+rqp_sensitivity_io\s*\{(.*?)\}\s*rqp_sensitivity_io\s*;", src, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert tuple(names) == FIELDS
    assert tuple(f for f, _ in _cabi.SensitivityIO._fields_) == FIELDS
    for k, bit in _cabi.SENS_SHARED.items():
        assert re.search(r"#define\s+RQP_SENS_SHARED_D%s\s+%d\b" % (k[1:].upper(), bit), src), k
    lib = _cabi.load()
    for name in ("rqp_set_sensitivity", "rqp_sensitivity"):
        assert name in _cabi.ABI_SYMBOLS
        assert hasattr(lib, name)


def test_null_handle_and_null_io():
    lib = _cabi.load()
    io = _cabi.SensitivityIO()
    assert lib.rqp_sensitivity(None, ctypes.byref(io), None) == _cabi.RQP_ERR_ARG
    assert lib.rqp_sensitivity(None, None, None) == _cabi.RQP_ERR_ARG
    assert lib.rqp_set_sensitivity(None, 1) == _cabi.RQP_ERR_ARG


def test_python_surface():
    from reluqp.reluqpth import ReLU_QP, Sensitivities
    from reluqp.layer import QPFunction, ReLUQPLayer
    assert inspect.signature(ReLU_QP.setup).parameters["sensitivity"].default is False
    assert Sensitivities._fields == ("dx", "dy", "dz", "status", "residual", "active")
    assert callable(ReLU_QP.jvp) and callable(ReLU_QP.jvp_at)
    assert "jvp" in QPFunction.__dict__
    assert callable(mpc.LinearMPC.feedback_gain)
    assert ReLUQPLayer().setup_kwargs.get("sensitivity", False) is False     # the layer's defaults do not change
    m = ReLU_QP()
    try:
        m.jvp(dg=np.zeros(3))
    except RuntimeError:
        pass
    else:
        raise AssertionError("jvp before setup must raise")


def _dirs(rs, d, b):
    return {k: rs.randn(*np.shape(d[k][b])) for k in ("H", "g", "A", "l", "u")}


def test_reference_matches_finite_differences_of_exact_solves():
    d = R.margin_qp_batch(4, 12, 3, 21, seed=7)
    rs = np.random.RandomState(3)
    eps = 1e-6
    for b in range(4):
        H, g, A, l, u, x, y, act = (d[k][b] for k in ("H", "g", "A", "l", "u", "x", "y", "active"))
        v = _dirs(rs, d, b)
        v["u"][:3] = v["l"][:3]                               # (equality rows stay equalities)
        dx, dy, dz = S.jvp(H, A, x, y, act, dH=v["H"], dg=v["g"], dA=v["A"], dl=v["l"], du=v["u"])
        sols = []
        for t in (eps, -eps):
            xe, ye = R.exact_solve(H + t * v["H"], g + t * v["g"], A + t * v["A"], l + t * v["l"], u + t * v["u"], act)
            sols.append((xe, ye, (A + t * v["A"]) @ xe))
        for got, k in zip((dx, dy, dz), range(3)):
            fd = (sols[0][k] - sols[1][k]) / (2 * eps)
            assert np.abs(fd - got).max() <= 1e-6 * max(1.0, np.abs(got).max()), (b, k)
        db = np.where(act < 0, v["l"], v["u"])
        assert np.abs((dz - db)[act != 0]).max() < 1e-9                   # dz = db on active rows


def test_duality_with_the_adjoint():
    for shared in (False, True):
        B, n, n_eq, n_ineq, ndir = 3, 10, 2, 16, 4
        d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=11, shared=shared)
        m = n_eq + n_ineq
        rs = np.random.RandomState(5)
        mat = () if shared else (B,)
        v = dict(dH=rs.randn(*(mat + (n, n, ndir))), dg=rs.randn(B, n, ndir), dA=rs.randn(*(mat + (m, n, ndir))),
                 dl=rs.randn(B, m, ndir), du=rs.randn(B, m, ndir))
        gx, gy = rs.randn(B, n), rs.randn(B, m)
        dx, dy, _ = S.jvp_batch(d["H"], d["A"], d["x"], d["y"], d["active"], ndir, **v)
        gr = R.adjoint_batch(d["H"], d["A"], d["x"], d["y"], d["active"], gx, gy)
        for j in range(ndir):
            lhs = np.sum(gx * dx[..., j]) + np.sum(gy * dy[..., j])
            rhs = sum(np.sum(gr[k] * v[k][..., j]) for k in ("dH", "dg", "dA", "dl", "du"))
            assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs)), (shared, j, lhs, rhs)


def test_sparse_mpc_unconstrained_gain_is_minus_lqr_gain():
    Ad, Bd = mpc.random_plant(12, 4, seed=0)
    ctl = mpc.LinearMPC(Ad, Bd, np.eye(12), 0.1 * np.eye(4), 10, 0.5, 10.0, form="sparse")
    nx, nu = 12, 4
    x0 = 1e-3 * np.random.RandomState(0).randn(nx)
    g, l, u = ctl.qp_vectors(x0[None])
    m = ctl.A.shape[0]
    act = np.zeros(m, np.int8)
    act[:10 * nx] = -1                                         # the dynamics rows; no box row is active
    x, y = R.exact_solve(ctl.H, g[0], ctl.A, l[0], u[0], act)
    assert (ctl.A @ x - l[0])[10 * nx:].min() > 0 and (u[0] - ctl.A @ x)[10 * nx:].min() > 0
    lumap = np.zeros((m, nx))
    lumap[:nx] = -Ad
    dx, _, _ = S.jvp_batch(ctl.H, ctl.A, x[None], y[None], act[None], nx, dg=np.zeros((ctl.H.shape[0], nx)), dl=lumap,
                           du=lumap)
    assert np.abs(dx[0, :nu, :] + ctl.K).max() < 1e-6
    # and the solution itself is linear in x0: u0 = -K x0
    assert np.abs(x[:nu] + ctl.K @ x0).max() < 1e-9
