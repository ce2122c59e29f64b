"""GPU checks of the float64 reduced-KKT chain behind rqp_adjoint and rqp_sensitivity (pack -> rqp_launch_gram_masked ->
rqp_launch_factor with a float64 output -> k_adjoint / k_adj_outer / k_adj_gemm, k_sens_classify / k_sens_rhs / k_sens_solve)
against the numpy restatements (tests/adjoint_ref.py, tests/sensitivity_ref.py) at every shape at which the chain takes
another code path: each gram and factor class, each column width of pcolmv, n > 256, m > 256, n and m that are no multiples
of 4 or 16, an empty active set, batch tails of k_adj_gemm's four waves, and a batch of per-instance matrices larger than one
chunk of the workspace.  Planted solutions (tests/kkt_edges_fixture.py) through adjoint_at / jvp_at: no ADMM solve is involved.
Each test prints its measured maximum relative error (the table of DESIGN.md section 5)."""
import time

import numpy as np
import pytest
import torch

from reluqp.reluqpth import ReLU_QP

import adjoint_ref as R
import kkt_edges_fixture as F
import sensitivity_ref as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
GRADS = ("dH", "dg", "dA", "dl", "du")
TOL = {F64: 1e-9, F32: 1e-5}               # the bounds of test_adjoint_gpu.py / test_sensitivity_gpu.py for these comparisons


def _t(a, prec):
    if torch.is_tensor(a):
        return a.to(device=DEV, dtype=prec)
    return torch.as_tensor(np.asarray(a), dtype=prec, device=DEV)


def _np(t):
    return t.detach().cpu().double().numpy()


def _err(got, ref):
    """Maximum error relative to 1 + max|ref| (what _close of the adjoint's and the sensitivities' tests bounds)."""
    got, ref = np.asarray(got), np.asarray(ref)
    return np.abs(got - ref).max() / (1 + np.abs(ref).max())


def _close(got, ref, rel, what):
    e = _err(got, ref)
    assert e <= rel, (what, e, np.abs(np.asarray(ref)).max())
    return e


def _r32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _solver(d, prec, **kw):
    m = ReLU_QP()
    m.setup(*(_t(d[k], prec) for k in ("H", "g", "A", "l", "u")), precision=prec, device=DEV, **kw)
    return m


def _args(d, prec):
    return [_t(d[k], prec) for k in ("H", "A", "l", "u", "x", "z", "y")]


# --------------------------------------------------------------- 1. per-instance matrices: every dispatch class of the chain
@pytest.fixture(scope="module", params=[(s, a, p) for s, a in F.SHAPES for p in (F64, F32)],
                ids=["%s-%s" % (F.shape_id(s), "f64" if p == F64 else "f32") for s, _ in F.SHAPES for p in (F64, F32)])
def case(request):
    """One handle per shape and precision (both kernels reserved), the planted batch as that handle sees it."""
    shape, n_active, prec = request.param
    d = F.per_instance(shape, n_active)
    if prec == F32:
        d = F.round32(d)
    m = _solver(d, prec, differentiable=True, sensitivity=True)
    yield shape, prec, d, m
    m._destroy()


def test_adjoint_per_instance(case):
    shape, prec, d, m = case
    n, n_eq, n_ineq, B = shape
    dx, dy = F.cotangents(shape)
    if prec == F32:
        dx, dy = _r32(dx), _r32(dy)
    act = torch.as_tensor(d["active"], device=DEV)
    worst = 0.0
    for cot in (dy, None):
        gr = m.adjoint_at(*_args(d, prec), _t(dx, prec), None if cot is None else _t(cot, prec), active=act)
        ref = R.adjoint_batch(d["H"], d["A"], d["x"], d["y"], d["active"], dx, cot)
        res = _np(gr.residual)
        print("adjoint %s %s dy=%s residual %.2e" % (F.shape_id(shape), prec, cot is not None, res.max()))
        for k in GRADS:
            worst = max(worst, _err(_np(getattr(gr, k)), ref[k]))
        print("adjoint %s %s dy=%s max rel err %.2e" % (F.shape_id(shape), prec, cot is not None, worst))
        for k in GRADS:
            _close(_np(getattr(gr, k)), ref[k], TOL[prec], k)
        assert (_np(gr.status) == 1).all()
        assert (gr.active.cpu().numpy() == d["active"]).all()
        if prec == F64:
            assert res.max() < 1e-10, res
        if cot is not None:
            full = gr
    part = m.adjoint_at(*_args(d, prec), _t(dx, prec), _t(dy, prec), active=act, want=("dg", "dA"))
    assert torch.equal(part.dg, full.dg) and torch.equal(part.dA, full.dA)
    assert part.dH is None and part.dl is None and part.du is None


def test_sensitivity_per_instance(case):
    shape, prec, d, m = case
    n, n_eq, n_ineq, B = shape
    mm = n_eq + n_ineq
    v = F.tangents(B, n, mm, F.NDIR, seed=2)
    if prec == F32:
        v = {k: _r32(t) for k, t in v.items()}
    s = m.jvp_at(*_args(d, prec), active=torch.as_tensor(d["active"], device=DEV), **{k: _t(t, prec) for k, t in v.items()})
    ref = S.jvp_batch(d["H"], d["A"], d["x"], d["y"], d["active"], F.NDIR, **v)
    assert tuple(s.dx.shape) == (B, n, F.NDIR) and tuple(s.dy.shape) == tuple(s.dz.shape) == (B, mm, F.NDIR)
    res = _np(s.residual)
    errs = [_err(_np(got), r) for got, r in zip((s.dx, s.dy, s.dz), ref)]
    print("sensitivity %s %s residual %.2e max rel err %.2e" % (F.shape_id(shape), prec, res.max(), max(errs)))
    for k, got, r in zip(("dx", "dy", "dz"), (s.dx, s.dy, s.dz), ref):
        _close(_np(got), r, TOL[prec], k)
    assert (_np(s.status) == 1).all()
    assert (s.active.cpu().numpy() == d["active"]).all()
    if prec == F64:
        assert res.max() < 1e-10, res


# ------------------------------------------------------------------- 2. shared matrices: k_adj_gemm's clamps and wave tails
@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("B", F.SHARED_B)
def test_shared_matrices_ragged_batch(B, prec):
    n, n_eq, n_ineq = F.SHARED
    mm = n_eq + n_ineq
    shape = F.SHARED + (B,)
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=F.seed_of(shape) + B, shared=True)
    dx, dy = F.cotangents(shape, seed=B)
    v = F.tangents(B, n, mm, F.NDIR, seed=3 + B, shared_mats=True)
    if prec == F32:
        d, dx, dy, v = F.round32(d), _r32(dx), _r32(dy), {k: _r32(t) for k, t in v.items()}
    m = _solver(d, prec, differentiable=True, sensitivity=True)
    act = torch.as_tensor(d["active"], device=DEV)
    gr = m.adjoint_at(*_args(d, prec), _t(dx, prec), _t(dy, prec), active=act)
    again = m.adjoint_at(*_args(d, prec), _t(dx, prec), _t(dy, prec), active=act)
    assert tuple(gr.dH.shape) == (n, n) and tuple(gr.dA.shape) == (mm, n)
    assert torch.equal(gr.dH, again.dH) and torch.equal(gr.dA, again.dA)            # a fixed summation order
    ref = R.adjoint_batch(d["H"], d["A"], d["x"], d["y"], d["active"], dx, dy)     # (dH, dA summed over the batch)
    errs = [_err(_np(getattr(gr, k)), ref[k]) for k in GRADS]
    s = m.jvp_at(*_args(d, prec), active=act, **{k: _t(t, prec) for k, t in v.items()})
    sref = S.jvp_batch(d["H"], d["A"], d["x"], d["y"], d["active"], F.NDIR, **v)
    serrs = [_err(_np(got), r) for got, r in zip((s.dx, s.dy, s.dz), sref)]
    print("shared B=%d %s adjoint max rel err %.2e (residual %.2e) sensitivity %.2e (residual %.2e)"
          % (B, prec, max(errs), _np(gr.residual).max(), max(serrs), _np(s.residual).max()))
    for k in GRADS:
        _close(_np(getattr(gr, k)), ref[k], TOL[prec], k)
    for k, got, r in zip(("dx", "dy", "dz"), (s.dx, s.dy, s.dz), sref):
        _close(_np(got), r, TOL[prec], k)
    for out in (gr, s):
        assert (_np(out.status) == 1).all()
        assert (out.active.cpu().numpy() == d["active"]).all()
        if prec == F64:
            assert _np(out.residual).max() < 1e-10


# ------------------------------------------------------------------ 3. more per-instance matrices than one chunk holds
def _planted_on_device(B, n, n_eq, n_ineq, seed):
    """margin_qp_batch's construction in float32 on the device (660 matrices of n = 320 take seconds on the host): H = M'M + I
    symmetrised, a planted x, multipliers and slacks with margins in [0.5, 1.5] on about half of the inequality rows (far
    below n / 2).  adjoint_at / jvp_at differentiate at (H, A, l, u, x, z, y) as given; g only feeds setup()."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rs = np.random.RandomState(seed)
    m = n_eq + n_ineq
    M = torch.randn(B, n, n, device=DEV, dtype=F32, generator=gen)
    H = torch.baddbmm(torch.eye(n, device=DEV, dtype=F32).expand(B, n, n), M.transpose(1, 2), M)
    H = H + H.transpose(1, 2)
    del M
    A = torch.randn(B, m, n, device=DEV, dtype=F32, generator=gen)
    x = torch.randn(B, n, device=DEV, dtype=F32, generator=gen)
    act = np.concatenate([np.where(rs.randn(B, n_eq) > 0, 1, -1), rs.choice([-1, 0, 1], size=(B, n_ineq), p=[0.25, 0.5, 0.25])],
                         1).astype(np.int8)
    mag, s_lo, s_up = (rs.uniform(0.5, 1.5, size=(B, m)) for _ in range(3))
    s_lo[act < 0] = 0.0
    s_up[act > 0] = 0.0
    s_lo[:, :n_eq] = s_up[:, :n_eq] = 0.0
    z = torch.bmm(A, x[:, :, None])[:, :, 0]
    y = _t(act * mag, F32)
    g = -(torch.bmm(H, x[:, :, None]) + torch.bmm(A.transpose(1, 2), y[:, :, None]))[:, :, 0]
    return dict(H=H, g=g, A=A, l=z - _t(s_lo, F32), u=z + _t(s_up, F32), x=x, y=y, z=z), act


def test_second_chunk_of_per_instance_matrices():
    """B = 660 float32 instances of n = 320: rqp_polish_chunk() = 2^30 / (16 n^2) = 655, so instances 655..659 run in a second
    pass of the chain with b0 = 655 (f.only = flag + b0, pw_act + b0 m, mat = blockIdx.x, Minv of blockIdx.x).  They must equal
    bit for bit what a five-instance handle (b0 = 0) gives for the same data, and the numpy references to the float32 bound.
    Measured on an MI355X: 0.7 s for the whole test, 0.4 s of it data, setup() and both calls of the 660-instance handle."""
    t0 = time.time()
    n, n_eq, n_ineq, B = F.CHUNK
    mm, ndir = n_eq + n_ineq, 3
    dev, active = _planted_on_device(B, n, n_eq, n_ineq, seed=F.seed_of(F.CHUNK))
    rs = np.random.RandomState(7)
    dx, dy = rs.randn(B, n).astype(np.float32), rs.randn(B, mm).astype(np.float32)
    # (the matrix tangents shared: per instance dH alone would be 800 MB)
    v = dict(dH=rs.randn(n, n, ndir), dg=rs.randn(B, n, ndir), dA=rs.randn(mm, n, ndir), dl=rs.randn(B, mm, ndir),
             du=rs.randn(B, mm, ndir))
    v = {k: t.astype(np.float32) for k, t in v.items()}
    status = np.zeros(B, np.int32)
    status[list(F.CHUNK_UNSOLVED)] = 1                         # max_iters_reached (any exit code but 0 = solved)
    # one rho: a ladder of one K(rho) per instance keeps setup() and the handle's own workspace small
    kw = dict(differentiable=True, sensitivity=True, adaptive_rho=False)
    big = _solver(dev, F32, **kw)
    act = torch.as_tensor(active, device=DEV)
    tan = {k: _t(t, F32) for k, t in v.items()}
    mats = [dev[k] for k in ("H", "A", "l", "u", "x", "z", "y")]
    st = torch.as_tensor(status, device=DEV)
    gr = big.adjoint_at(*mats, _t(dx, F32), _t(dy, F32), status=st, active=act)
    sn = big.jvp_at(*mats, status=st, active=act, **tan)
    t_big = time.time() - t0

    # the second chunk alone, on a handle where it is the first
    tail = slice(655, 660)
    small = _solver({k: t[tail] for k, t in dev.items()}, F32, **kw)
    gr5 = small.adjoint_at(*(t[tail] for t in mats), _t(dx[tail], F32), _t(dy[tail], F32), status=st[tail], active=act[tail])
    sn5 = small.jvp_at(*(t[tail] for t in mats), status=st[tail], active=act[tail],
                       **{k: (t if k in ("dH", "dA") else t[tail]) for k, t in tan.items()})
    for k in GRADS:
        assert torch.equal(getattr(gr, k)[tail], getattr(gr5, k)), k
    for k in ("dx", "dy", "dz"):
        assert torch.equal(getattr(sn, k)[tail], getattr(sn5, k)), k
    for a, b in ((gr, gr5), (sn, sn5)):
        assert torch.equal(a.status[tail], b.status) and torch.equal(a.active[tail], b.active)
        ra, rb = a.residual[tail], b.residual
        assert bool(((ra == rb) | (torch.isnan(ra) & torch.isnan(rb))).all())

    # instances that were not solved, and everything else reported as computed
    bad = np.zeros(B, bool)
    bad[list(F.CHUNK_UNSOLVED)] = True
    badt = torch.as_tensor(bad, device=DEV)
    for out, names in ((gr, GRADS), (sn, ("dx", "dy", "dz"))):
        assert (_np(out.status) == ~bad).all()
        res = _np(out.residual)
        assert np.isnan(res[bad]).all() and not np.isnan(res[~bad]).any()
        assert (out.active[badt] == 0).all() and torch.equal(out.active[~badt], act[~badt])
        for k in names:
            assert (getattr(out, k)[badt] == 0).all(), k

    # both chunks against the numpy references on the float32 data
    idx = np.array(F.CHUNK_REF)
    it = torch.as_tensor(idx, device=DEV)
    r = {k: _np(dev[k][it]) for k in ("H", "A", "x", "y")}
    r["active"] = active[idx]
    ref = R.adjoint_batch(r["H"], r["A"], r["x"], r["y"], r["active"], dx[idx].astype(np.float64), dy[idx].astype(np.float64))
    v64 = {k: (t if k in ("dH", "dA") else t[idx]).astype(np.float64) for k, t in v.items()}
    sref = S.jvp_batch(r["H"], r["A"], r["x"], r["y"], r["active"], ndir, **v64)
    errs = [_err(_np(getattr(gr, k)[it]), ref[k]) for k in GRADS]
    serrs = [_err(_np(getattr(sn, k)[it]), q) for k, q in zip(("dx", "dy", "dz"), sref)]
    print("chunked adjoint max rel err %.2e sensitivity %.2e; big handle %.2f s, whole test %.2f s"
          % (max(errs), max(serrs), t_big, time.time() - t0))
    for k in GRADS:
        _close(_np(getattr(gr, k)[it]), ref[k], TOL[F32], k)
    for k, q in zip(("dx", "dy", "dz"), sref):
        _close(_np(getattr(sn, k)[it]), q, TOL[F32], k)
