"""GPU checks of the forward sensitivities (rqp_sensitivity; ReLU_QP.jvp / jvp_at; QPFunction.jvp; LinearMPC.feedback_gain):
the kernels against the numpy restatement (tests/sensitivity_ref.py), duality with the GPU adjoint, finite differences of GPU
re-solves, MPC facts that do not depend on this solver, forward-mode autograd through the layer, determinism across
direction blocks, instances that were not solved, graph capture, and unchanged solves on a handle that reserves it."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from reluqp import mpc
from reluqp.layer import ReLUQPLayer
from reluqp.reluqpth import ReLU_QP

import adjoint_ref as R
import sensitivity_ref as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64


def _t(a, prec):
    return torch.as_tensor(np.asarray(a), dtype=prec, device=DEV)


def _np(t):
    return t.detach().cpu().double().numpy()


def _solver(H, g, A, l, u, prec, **kw):
    m = ReLU_QP()
    m.setup(_t(H, prec), _t(g, prec), _t(A, prec), _t(l, prec), _t(u, prec), precision=prec, device=DEV, **kw)
    return m


def _close(got, ref, rel):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.abs(got - ref).max() <= rel * (1 + np.abs(ref).max()), (np.abs(got - ref).max(), np.abs(ref).max())


def _round32(d):
    return {k: (v if k == "active" else v.astype(np.float32).astype(np.float64)) for k, v in d.items()}


# ------------------------------------------------------------------------------------------ 1. kernel against the reference
@pytest.mark.parametrize("prec", [F64, torch.float32])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("ndir", [1, 12, 40])
def test_kernel_matches_reference(prec, shared, ndir):
    B, n, n_eq, n_ineq = 24, 32, 6, 50
    m = n_eq + n_ineq
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=3 + ndir, shared=shared)
    rs = np.random.RandomState(ndir)
    mat = () if shared else (B,)
    # matrix tangents follow the matrices (shared on a shared handle), dl shared, the others per instance
    v = dict(dH=rs.randn(*(mat + (n, n, ndir))), dg=rs.randn(B, n, ndir), dA=rs.randn(*(mat + (m, n, ndir))),
             dl=rs.randn(m, ndir), du=rs.randn(B, m, ndir))
    if prec == torch.float32:
        d = _round32(d)
        v = {k: t.astype(np.float32).astype(np.float64) for k, t in v.items()}
    sv = _solver(d["H"], d["g"], d["A"], d["l"], d["u"], prec, sensitivity=True)
    s = sv.jvp_at(*(_t(d[k], prec) for k in ("H", "A", "l", "u", "x", "z", "y")),
                  active=torch.as_tensor(d["active"], device=DEV), **{k: _t(t, prec) for k, t in v.items()})
    dx, dy, dz = S.jvp_batch(d["H"], d["A"], d["x"], d["y"], d["active"], ndir, **v)
    assert tuple(s.dx.shape) == (B, n, ndir)                   # (the tangents carry an ndir axis: not squeezed)
    tol = 1e-9 if prec == F64 else 1e-5
    _close(_np(s.dx).reshape(dx.shape), dx, tol)
    _close(_np(s.dy).reshape(dy.shape), dy, tol)
    _close(_np(s.dz).reshape(dz.shape), dz, tol)
    assert (_np(s.status) == 1).all()
    assert (s.active.cpu().numpy() == d["active"]).all()
    if prec == F64:
        assert _np(s.residual).max() < 1e-10


def test_tangent_shapes_and_squeeze():
    B, n, n_eq, n_ineq = 8, 12, 2, 20
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=21)
    sv = _solver(d["H"], d["g"], d["A"], d["l"], d["u"], F64, sensitivity=True)
    args = [_t(d[k], F64) for k in ("H", "A", "l", "u", "x", "z", "y")]
    act = torch.as_tensor(d["active"], device=DEV)
    rs = np.random.RandomState(0)
    dg = rs.randn(n)
    one = sv.jvp_at(*args, dg=_t(dg, F64), active=act)                         # shared, one direction: squeezed
    per = sv.jvp_at(*args, dg=_t(np.tile(dg, (B, 1)), F64), active=act)        # per instance, one direction
    multi = sv.jvp_at(*args, dg=_t(dg[:, None], F64), active=act)              # shared, ndir = 1 axis kept
    assert tuple(one.dx.shape) == (B, n) and tuple(multi.dx.shape) == (B, n, 1)
    assert torch.equal(one.dx, per.dx) and torch.equal(one.dx, multi.dx[..., 0])
    with pytest.raises(ValueError):
        sv.jvp_at(*args, dg=_t(rs.randn(n, 3), F64), dl=_t(rs.randn(n_eq + n_ineq, 2), F64), active=act)


# ----------------------------------------------------------------------------------------- 2. duality with the GPU adjoint
@pytest.mark.parametrize("shared", [False, True])
def test_duality_with_gpu_adjoint(shared):
    B, n, n_eq, n_ineq, ndir = 64, 40, 8, 72, 5
    m = n_eq + n_ineq
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=31, shared=shared)
    sv = _solver(d["H"], d["g"], d["A"], d["l"], d["u"], F64, sensitivity=True, differentiable=True)
    args = [_t(d[k], F64) for k in ("H", "A", "l", "u", "x", "z", "y")]
    act = torch.as_tensor(d["active"], device=DEV)
    rs = np.random.RandomState(1)
    mat = () if shared else (B,)
    v = dict(dH=rs.randn(*(mat + (n, n, ndir))), dg=rs.randn(B, n, ndir), dA=rs.randn(*(mat + (m, n, ndir))),
             dl=rs.randn(B, m, ndir), du=rs.randn(B, m, ndir))
    s = sv.jvp_at(*args, active=act, **{k: _t(t, F64) for k, t in v.items()})
    gx, gy = rs.randn(B, n), rs.randn(B, m)
    gr = sv.adjoint_at(*args, _t(gx, F64), _t(gy, F64), active=act)
    dx, dy = _np(s.dx), _np(s.dy)
    for j in range(ndir):
        lhs = np.sum(gx * dx[..., j]) + np.sum(gy * dy[..., j])
        rhs = sum(np.sum(_np(getattr(gr, k)) * v[k][..., j]) for k in ("dH", "dg", "dA", "dl", "du"))
        assert abs(lhs - rhs) <= 1e-9 * max(1.0, abs(lhs)), (j, lhs, rhs)


# ------------------------------------------------------------------------------ 3. finite differences of GPU re-solves
def test_matches_finite_differences_of_polished_resolves():
    B, n, n_eq, n_ineq = 64, 12, 3, 21
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=9)
    layer = ReLUQPLayer(eps_abs=1e-10, max_iter=20000, sensitivity=True)
    ins = {k: _t(d[k], F64) for k in ("H", "g", "A", "l", "u")}
    layer(*(ins[k] for k in ("H", "g", "A", "l", "u")))
    solver = next(iter(layer._handles.values()))["solver"]
    rs = np.random.RandomState(3)
    dirs = {k: _t(rs.randn(*d[k].shape), F64) for k in ("H", "g", "A", "l", "u")}
    dirs["u"][:, :n_eq] = dirs["l"][:, :n_eq]                  # (equality rows stay equalities)
    s = solver.jvp(**{"d" + k: t for k, t in dirs.items()})
    step = 1e-6
    outs, good = [], solver.info.status_polish.cpu().numpy() == 1
    for sgn in (1, -1):
        xs, ys = layer(*(ins[k] + sgn * step * dirs[k] for k in ("H", "g", "A", "l", "u")))
        good &= solver.info.status_polish.cpu().numpy() == 1
        good &= (solver.results.active.cpu().numpy() == d["active"]).all(1)
        outs.append((_np(xs), _np(ys)))
    assert good.mean() >= 0.8, good.mean()
    for k, an in ((0, _np(s.dx)), (1, _np(s.dy))):
        fd = (outs[0][k] - outs[1][k]) / (2 * step)
        err = np.abs(fd - an).max(1) / np.maximum(1.0, np.abs(an).max(1))
        assert err[good].max() <= 1e-5, err[good].max()


# ------------------------------------------------------------------------------------- 4. MPC facts independent of the solver
def _ctl(form, **kw):
    Ad, Bd = mpc.random_plant(12, 4, seed=0)
    return mpc.LinearMPC(Ad, Bd, np.eye(12), 0.1 * np.eye(4), 20, 0.5, 10.0, form=form, sensitivity=True, **kw)


@pytest.mark.parametrize("form", ["sparse", "condensed"])
def test_feedback_gain_is_minus_lqr_gain_when_nothing_is_active(form):
    ctl = _ctl(form, precision=F64, eps_abs=1e-6)
    x0 = 1e-3 * np.random.RandomState(0).randn(64, 12)
    ctl.simulate_device(x0, 1, DEV, F64)                       # (update_affine path: QP.l / QP.u are not those of the solve)
    gain, st = ctl.feedback_gain(_t(x0, F64))
    assert tuple(gain.shape) == (64, 4, 12)
    assert (_np(st) == 1).all()
    assert np.abs(_np(gain) + ctl.K[None]).max() < 1e-6       # (condensed: d v0 / d x0 = 0 with no row active)


def test_feedback_gain_rows_of_saturated_inputs_are_zero():
    ctl = _ctl("condensed", precision=F64, eps_abs=1e-6, polish=True)
    x0 = 3.0 * np.random.RandomState(1).randn(128, 12)
    g, l, u = ctl.qp_vectors(x0)
    ctl.solver = ReLU_QP()
    ctl.solver.setup(ctl.H, g, ctl.A, l, u, device=DEV, **ctl.solver_kw)
    ctl._ready = True
    res = ctl.solver.solve()
    gain, st = ctl.feedback_gain(x0)
    z, y, lt, ut = _np(res.z), _np(res.y), l, u
    lo, hi = z - lt < -y, ut - z < y
    sat = (lo | hi)[:, :4] & (_np(st) == 1)[:, None]
    assert sat.sum() >= 10, sat.sum()
    assert np.abs(_np(gain)[sat]).max() < 1e-9
    assert np.abs(_np(gain)[~sat & (_np(st) == 1)[:, None]]).max() > 1e-3


# ---------------------------------------------------------------------------------------------------- 5. forward-mode AD
def test_forward_ad_through_layer_equals_jvp():
    B, n, n_eq, n_ineq = 16, 12, 3, 21
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=5, shared=True)
    layer = ReLUQPLayer(eps_abs=1e-10, max_iter=20000, sensitivity=True)
    H, A = _t(d["H"], F64), _t(d["A"], F64)
    g, l, u = (_t(d[k], F64) for k in ("g", "l", "u"))
    rs = np.random.RandomState(2)
    tg, tl, tH = _t(rs.randn(B, n), F64), _t(rs.randn(B, n_eq + n_ineq), F64), _t(rs.randn(n, n), F64)   # (tH: shared)
    with fwAD.dual_level():
        x, y = layer(fwAD.make_dual(H, tH), fwAD.make_dual(g, tg), A, fwAD.make_dual(l, tl), u)
        tx, ty = fwAD.unpack_dual(x).tangent, fwAD.unpack_dual(y).tangent
    solver = next(iter(layer._handles.values()))["solver"]
    s = solver.jvp(dH=tH, dg=tg, dl=tl)
    assert torch.equal(tx, s.dx) and torch.equal(ty, s.dy)


def test_forward_ad_requires_the_reservation():
    d = R.margin_qp_batch(4, 8, 1, 12, seed=5)
    layer = ReLUQPLayer(eps_abs=1e-8)
    g = _t(d["g"], F64)
    with fwAD.dual_level():
        with pytest.raises(RuntimeError, match="sensitivity=True"):
            layer(_t(d["H"], F64), fwAD.make_dual(g, torch.ones_like(g)), _t(d["A"], F64), _t(d["l"], F64), _t(d["u"], F64))


def test_layer_gradcheck_forward_ad():
    B, n, n_eq, n_ineq = 3, 8, 0, 16
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=9)
    layer = ReLUQPLayer(eps_abs=1e-10, max_iter=20000, sensitivity=True)
    H, A = _t(d["H"], F64), _t(d["A"], F64)
    g, l, u = (_t(d[k], F64).requires_grad_() for k in ("g", "l", "u"))
    assert torch.autograd.gradcheck(lambda g, l, u: layer(H, g, A, l, u), (g, l, u), eps=1e-6, atol=1e-5, rtol=1e-4,
                                    check_forward_ad=True)


# ------------------------------------------------------------------------------------------------------ 6. determinism
def test_direction_blocks_are_bitwise_independent():
    B, n, n_eq, n_ineq, ndir = 32, 30, 5, 55, 40
    m = n_eq + n_ineq
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=41)
    sv = _solver(d["H"], d["g"], d["A"], d["l"], d["u"], F64, sensitivity=True)
    args = [_t(d[k], F64) for k in ("H", "A", "l", "u", "x", "z", "y")]
    act = torch.as_tensor(d["active"], device=DEV)
    rs = np.random.RandomState(4)
    v = dict(dH=_t(rs.randn(B, n, n, ndir), F64), dg=_t(rs.randn(n, ndir), F64), dA=_t(rs.randn(B, m, n, ndir), F64),
             dl=_t(rs.randn(B, m, ndir), F64), du=_t(rs.randn(m, ndir), F64))
    full = sv.jvp_at(*args, active=act, **v)
    again = sv.jvp_at(*args, active=act, **v)
    for k in ("dx", "dy", "dz", "residual"):
        assert torch.equal(getattr(full, k), getattr(again, k)), k
    for j in range(ndir):
        one = sv.jvp_at(*args, active=act, **{k: t[..., j:j + 1].contiguous() for k, t in v.items()})
        for k in ("dx", "dy", "dz"):
            assert torch.equal(getattr(one, k)[..., 0], getattr(full, k)[..., j]), (k, j)


# ------------------------------------------------------------------------------------------ 7. instances that were not solved
def test_unsolved_instances_get_zero_tangents():
    B, n, n_eq, n_ineq = 64, 30, 5, 55
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=13)
    it = _solver(d["H"], d["g"], d["A"], d["l"], d["u"], F64, eps_abs=1e-6).solve().info.iter.cpu().numpy()
    budget = int(np.median(it))
    sv = _solver(d["H"], d["g"], d["A"], d["l"], d["u"], F64, sensitivity=True, max_iter=budget, eps_abs=1e-6)
    res = sv.solve()
    st = res.info.status_code.cpu().numpy()
    assert (st != 0).any() and (st == 0).any()
    rs = np.random.RandomState(1)
    v = dict(dg=_t(rs.randn(B, n, 3), F64), du=_t(rs.randn(B, n_eq + n_ineq, 3), F64))
    s = sv.jvp(**v)
    every = sv.jvp_at(sv.QP.H, sv.QP.A, sv.QP.l, sv.QP.u, res.x, res.z, res.y, **v)
    bad = torch.as_tensor(st != 0, device=DEV)
    assert (_np(s.status) == (st == 0)).all()
    assert np.isnan(_np(s.residual)[st != 0]).all() and not np.isnan(_np(s.residual)[st == 0]).any()
    for k in ("dx", "dy", "dz"):
        assert (getattr(s, k)[bad] == 0).all(), k
        assert torch.equal(getattr(s, k)[~bad], getattr(every, k)[~bad]), k
    assert (s.active[bad] == 0).all()


# ------------------------------------------------------------------------------------------------------ 8. graph capture
def test_jvp_is_graph_capturable():
    B, n, n_eq, n_ineq = 64, 20, 4, 36
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=19)
    sv = _solver(d["H"], d["g"], d["A"], d["l"], d["u"], F64, sensitivity=True)
    sv.synchronous = False
    args = [_t(d[k], F64) for k in ("H", "A", "l", "u", "x", "z", "y")]
    dg = _t(np.random.RandomState(0).randn(B, n, 20), F64)
    eager = sv.jvp_at(*args, dg=dg)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sv.jvp_at(*args, dg=dg)                       # (warm-up on the side stream: LDS attributes set outside capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = sv.jvp_at(*args, dg=dg)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("dx", "dy", "dz", "residual"):
        assert torch.equal(getattr(cap, k), getattr(eager, k)), k


# -------------------------------------------------------------------------------------------------- 9. nothing else changes
@pytest.mark.parametrize("prec,kw", [(torch.float32, dict()), (F64, dict(full_ladder=True)), (F64, dict(polish=True))])
def test_sensitivity_handle_solves_bit_identically(prec, kw):
    B, n, n_eq, n_ineq = 64, 40, 10, 60
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=17)
    outs = []
    for sens in (False, True):
        m = _solver(d["H"], d["g"], d["A"], d["l"], d["u"], prec, sensitivity=sens, **kw)
        r = m.solve()
        m.update(g=_t(d["g"] * 1.01, prec))
        r2 = m.solve()
        outs.append([t.clone() for t in (r.x, r.z, r.y, r.info.iter, r.info.status_code, r.info.pri_res)] +
                    [r2.x.clone(), r2.info.iter.clone()])
        if not sens:
            with pytest.raises(RuntimeError):
                m.jvp(dg=torch.zeros(B, n, dtype=prec, device=DEV))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_jvp_refused_after_update_affine_and_on_shards():
    Ad, Bd = mpc.random_plant(12, 4, seed=0)
    ctl = mpc.LinearMPC(Ad, Bd, np.eye(12), 0.1 * np.eye(4), 20, 0.5, 10.0, form="condensed")
    g, l, u = ctl.qp_vectors(np.random.RandomState(1).randn(32, 12))
    m = _solver(ctl.H, g, ctl.A, l, u, F64, sensitivity=True)
    m.solve()
    m.update_affine(_t(np.zeros((32, 12)), F64), _t(ctl.g_x0, F64), _t(ctl.lu_x0, F64), _t(ctl.l_add, F64),
                    _t(ctl.u_add, F64))
    m.solve()
    with pytest.raises(RuntimeError):
        m.jvp(dg=torch.zeros(32, ctl.H.shape[0], dtype=F64, device=DEV))
    m.update(l=m.QP.l, u=m.QP.u)
    m.solve()
    m.jvp(dg=torch.zeros(32, ctl.H.shape[0], dtype=F64, device=DEV))
    multi = ReLU_QP()
    multi.setup(_t(ctl.H, F64), _t(g, F64), _t(ctl.A, F64), _t(l, F64), _t(u, F64), precision=F64, devices=[0, 0],
                sensitivity=True)
    multi.solve()
    with pytest.raises(RuntimeError):
        multi.jvp(dg=torch.zeros(32, ctl.H.shape[0], dtype=F64, device=DEV))
