"""Condensed QPs of LTV plants built on the device (rqp_ltv_condense / rqp_ltv_vectors) and the BatchedLTVMPC driver.

Kernel vs host: the formulas are evaluated once in np.longdouble (the yardstick, reluqp.mpc.condense_ltv on longdouble
inputs); e_host is the error of the float64 numpy evaluation against it, per output, relative to that output's
max|entry|.  The float64 device outputs must be within 10 x max(e_host, 2^-52) of the yardstick; float32 outputs within
1 ulp(float32) of the rounded yardstick wherever |entry| >= 2^-24 max|entry|.  The ratios are printed before they are
asserted."""
import numpy as np
import pytest
import torch

from oracle import reluqp_oracle as O
from reluqp import mpc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble


def _stages(B, nx, nu, N, seed, rel=0.05, c_scale=0.1):
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)
    rs = np.random.RandomState(seed + 1)
    Ad = Ad0[None, None] + rel * rs.randn(B, N, nx, nx) / np.sqrt(nx)
    Bd = Bd0[None, None] + rel * rs.randn(B, N, nx, nu)
    c = c_scale * rs.randn(B, N, nx)
    return Ad0, Bd0, Ad, Bd, c, rs


@pytest.mark.parametrize("opts", ["plain", "K", "K_c_refs"])
@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
# the issue's two shapes, then the limits of what the ABI accepts: nx = 16 ([G | f] needs two tiles), horizon = 32 with m = 640
# (the largest LDS image), nu = 8 with n = 160, and a tiny one (nx padded to 4, n below one tile)
@pytest.mark.parametrize("shape", [(12, 4, 20, 64), (7, 3, 9, 5), (16, 4, 32, 4), (12, 8, 20, 3), (3, 1, 7, 3)])
def test_kernels_match_host_formulas(shape, prec, opts):
    nx, nu, N, B = shape
    _, _, Ad, Bd, c, rs = _stages(B, nx, nu, N, seed=11)
    Q, R = np.diag(1.0 + rs.rand(nx)), 0.1 * np.eye(nu) + 0.01 * np.ones((nu, nu))
    Qf = 2.0 * Q + 0.1 * np.ones((nx, nx))
    K = 0.1 * rs.randn(nu, nx) if opts != "plain" else None
    full = opts == "K_c_refs"
    n, m = N * nu, N * (nx + nu)
    x0 = rs.randn(B, nx)
    xref, uref = (0.3 * rs.randn(B, N, nx), 0.1 * rs.randn(B, N, nu)) if full else (None, None)
    _, l_add, u_add = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    if full:                                                    # per-instance bounds
        l_add, u_add = l_add[None] - rs.rand(B, m), u_add[None] + rs.rand(B, m)
    npt = np.float32 if prec == torch.float32 else np.float64
    rnd = lambda a: None if a is None else np.asarray(a).astype(npt)     # the values the device sees
    Ad, Bd, c, x0, xref, uref, l_add, u_add = (rnd(a) for a in (Ad, Bd, c if full else None, x0, xref, uref, l_add, u_add))
    t = lambda a: None if a is None else torch.as_tensor(a, device=DEV)
    ws = mpc.ltv_workspace(B, nx, nu, N, DEV)
    H, A = mpc.condense_ltv_device(t(Ad), t(Bd), (Q, R, Qf, K), ws, c=t(c))
    g, l, u = mpc.ltv_vectors_device((nx, nu, N, K is not None, c is not None), t(x0), t(l_add), t(u_add), (Q, R, Qf, K), ws,
                                     xref=t(xref), uref=t(uref))
    torch.cuda.synchronize()
    dev = {k: v.cpu().numpy() for k, v in dict(H=H, A=A, g=g, l=l, u=u).items()}
    assert dev["H"].dtype == npt and dev["H"].shape == (B, n, n) and dev["A"].shape == (B, m, n)
    for b in range(B):
        assert np.array_equal(dev["H"][b], dev["H"][b].T), "H must be bitwise symmetric"
    blk = nx + nu
    for j in range(1, N):                                       # block column j of F is zero above stage j
        assert not dev["A"][:, :j * blk, j * nu:(j + 1) * nu].any(), "structural zeros of A must be exact"
    sub = list(range(min(B, 8)))
    worst = {}
    for b in sub:
        out = {}
        for dt in (LD, np.float64):
            kw = dict(K=None if K is None else K.astype(dt), c=None if c is None else c[b].astype(dt))
            cond = mpc.condense_ltv(Ad[b].astype(dt), Bd[b].astype(dt), Q.astype(dt), R.astype(dt), Qf.astype(dt), **kw)
            la, ua = (l_add[b], u_add[b]) if l_add.ndim == 2 else (l_add, u_add)
            gg, ll, uu = mpc.ltv_vectors(cond, x0[b].astype(dt), la.astype(dt), ua.astype(dt),
                                         xref=None if xref is None else xref[b].astype(dt),
                                         uref=None if uref is None else uref[b].astype(dt))
            out[dt] = dict(H=cond["H"], A=cond["A"], g=gg, l=ll, u=uu)
        assert out[LD]["H"].dtype == LD
        for k in ("H", "A", "g", "l", "u"):
            ref = out[LD][k]
            scale = float(np.abs(ref).max())
            e_host = float(np.abs(out[np.float64][k].astype(LD) - ref).max()) / scale
            if prec == torch.float64:
                e_dev = float(np.abs(dev[k][b].astype(LD) - ref).max()) / scale
                w = worst.setdefault(k, [0.0, 0.0, 0.0])
                ratio = e_dev / max(e_host, 2.0 ** -52)
                if ratio > w[0]:
                    worst[k] = [ratio, e_dev, e_host]
            else:
                r32 = ref.astype(np.float32)
                ulps = np.abs(dev[k][b].astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
                big = np.abs(ref) >= 2.0 ** -24 * scale
                w = worst.setdefault(k, [0.0])
                w[0] = max(w[0], float(ulps[big].max()))
    for k, w in worst.items():
        if prec == torch.float64:
            print("LTV f64 %s %s %s: e_dev / max(e_host, 2^-52) = %.3f (e_dev %.3e, e_host %.3e)" % (shape, opts, k, *w))
        else:
            print("LTV f32 %s %s %s: max ulp distance from the rounded yardstick = %.3f" % (shape, opts, k, w[0]))
    for k, w in worst.items():
        if prec == torch.float64:
            assert w[0] <= 10.0, (k, w)
        else:
            assert w[0] <= 1.0, (k, w)


def _c3_driver(prec, B=64, seed=7, rel=0.02, **kw):
    nx, nu, N = 12, 4, 20
    Ad0, Bd0, Ad, Bd, c, rs = _stages(B, nx, nu, N, seed=0, rel=rel, c_scale=0.0)
    Q, R = np.eye(nx), 0.1 * np.eye(nu)
    K, P = mpc.ihlqr(Ad0, Bd0, Q, R, Q)
    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, P, u_max=0.4, x_max=8.0, K=K, device=DEV, precision=prec, eps_abs=1e-3, **kw)
    x0 = 1.5 * np.random.RandomState(seed).randn(B, nx)
    t = lambda a: torch.as_tensor(a, device=DEV, dtype=prec)
    return ctl, t(Ad), t(Bd), t(x0), (Ad0, Bd0, Q, R, P, K)


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
def test_solver_on_device_built_data_matches_oracle(prec):
    ctl, Ad, Bd, x0, _ = _c3_driver(prec)
    ctl.linearize(Ad, Bd)
    u0, res = ctl.step(x0)
    model = ctl.solver
    if prec == torch.float32:
        assert model.kernel in ("resident", "resident2", "wave"), model.kernel     # a per-instance kernel, not generic
    assert not model.QP.shared_mats
    buf = ctl._buf
    H, g, A, l, u = (buf[k].cpu().double().numpy() for k in ("H", "g", "A", "l", "u"))
    ref = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-3)
    # the oracle alone, float32 against float64 on these inputs, stays inside the same-iteration condition
    f32 = lambda a: a.astype(np.float32)
    ref32 = O.solve_batch(f32(H), f32(g), f32(A), f32(l), f32(u), form="factored", eps_abs=1e-3, dtype=np.float32)
    print("oracle f32 vs f64: same-iteration share %.3f" % np.mean(ref32["iter"] == ref["iter"]))
    assert np.mean(ref32["iter"] == ref["iter"]) >= 0.9
    assert res.info.status == ref["status"]
    assert np.mean([s == "solved" for s in res.info.status]) >= 0.9
    it = res.info.iter.cpu().numpy()
    same = it == ref["iter"]
    print("device %s vs oracle: same-iteration share %.3f, kernel %s, mean iter %.1f" % (prec, same.mean(), model.kernel, it.mean()))
    assert same.mean() >= 0.9
    scale = max(1.0, np.abs(ref["x"]).max())
    np.testing.assert_allclose(res.x.cpu().double().numpy()[same], ref["x"][same], rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(res.z.cpu().double().numpy()[same], ref["z"][same], rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(res.y.cpu().double().numpy()[same], ref["lam"][same], rtol=0,
                               atol=2e-3 * max(1.0, np.abs(ref["lam"]).max()))
    assert np.all(np.abs(u0.cpu().numpy()) <= 0.4 + 2e-2)


def test_relinearisation_keeps_the_warm_start():
    prec = torch.float64
    ctl, Ad, Bd, x0, _ = _c3_driver(prec)
    gen = torch.Generator(device="cpu").manual_seed(3)
    Ad2 = Ad * (1 + 1e-3 * torch.randn(Ad.shape, generator=gen, dtype=prec).to(DEV))
    Bd2 = Bd * (1 + 1e-3 * torch.randn(Bd.shape, generator=gen, dtype=prec).to(DEV))
    ctl.linearize(Ad, Bd)
    ctl.step(x0)
    ctl.linearize(Ad2, Bd2)
    u_warm, r_warm = ctl.step(x0)
    cold, _, _, _, _ = _c3_driver(prec)
    cold.linearize(Ad2, Bd2)
    u_cold, r_cold = cold.step(x0)
    it_w, it_c = r_warm.info.iter.double().mean().item(), r_cold.info.iter.double().mean().item()
    print("mean iterations: warm %.1f, cold %.1f" % (it_w, it_c))
    assert it_w < it_c
    ok = [a == "solved" and b == "solved" for a, b in zip(r_warm.info.status, r_cold.info.status)]
    assert np.mean(ok) >= 0.9
    ok = torch.as_tensor(ok, device=DEV)
    scale = max(1.0, r_cold.x.abs().max().item())
    assert (r_warm.x - r_cold.x)[ok].abs().max().item() <= 2e-2 * scale      # two eps_abs = 1e-3 exits of the same QP
    assert (u_warm - u_cold)[ok].abs().max().item() <= 2e-2


def test_lti_closed_loop_agrees_with_linear_mpc():
    prec, B, nx, nu, N, steps = torch.float64, 32, 12, 4, 20, 30
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=0)
    Q, R = np.eye(nx), 0.1 * np.eye(nu)
    lti = mpc.LinearMPC(Ad0, Bd0, Q, R, N, u_max=0.4, x_max=8.0, form="condensed", device=DEV, precision=prec, eps_abs=1e-3)
    x0 = 1.5 * np.random.RandomState(5).randn(B, nx)
    x_lti, _ = lti.simulate_device(x0, steps, DEV, prec)
    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, lti.P, u_max=0.4, x_max=8.0, K=lti.K, device=DEV, precision=prec, eps_abs=1e-3)
    t = lambda a: torch.as_tensor(a, device=DEV, dtype=prec)
    Ad = t(Ad0).expand(B, N, nx, nx).contiguous()
    Bd = t(Bd0).expand(B, N, nx, nu).contiguous()
    Adt, Bdt = t(Ad0.T), t(Bd0.T)
    plant = lambda x, u: (x @ Adt + u @ Bdt, Ad, Bd, None)
    ctl.linearize(Ad, Bd)
    xs, us, its = ctl.simulate(t(x0), steps, plant)
    err = (xs[-1] - x_lti).abs().max().item()
    print("closed loop: max|x_ltv - x_lti| = %.3e, max|x| = %.3e" % (err, xs.abs().max().item()))
    assert err <= 2e-3 * max(1.0, xs.abs().max().item())
    assert us.abs().max().item() <= 0.4 + 2e-2
    # every intermediate state and input, against the host loop of the same controller (a fresh handle)
    host = mpc.LinearMPC(Ad0, Bd0, Q, R, N, u_max=0.4, x_max=8.0, form="condensed", device=DEV, precision=prec, eps_abs=1e-3)
    xs_h, us_h, _ = host.simulate(x0, steps)
    err_x = np.abs(xs.cpu().numpy() - xs_h).max()
    err_u = np.abs(us.cpu().numpy() - us_h).max()
    print("closed loop, whole trajectory: max|x_ltv - x_host| = %.3e, max|u_ltv - u_host| = %.3e" % (err_x, err_u))
    assert err_x <= 2e-3 * max(1.0, np.abs(xs_h).max())
    assert err_u <= 2e-3 * max(1.0, np.abs(us_h).max())


def test_tracking_a_constant_reference():
    prec, B, nx, nu, N, steps = torch.float32, 16, 6, 2, 10, 60
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=7)
    Q, R = np.eye(nx), 0.1 * np.eye(nu)
    K, P = mpc.ihlqr(Ad0, Bd0, Q, R, Q)
    t = lambda a: torch.as_tensor(a, device=DEV, dtype=prec)
    # an equilibrium inside the box: x* = Ad x* + Bd u*  with a small constant input
    rs = np.random.RandomState(2)
    ustar = 0.05 * rs.randn(B, nu)
    xstar = np.linalg.solve(np.eye(nx) - Ad0, Bd0 @ ustar.T).T
    assert np.abs(xstar).max() < 8.0
    ctl = mpc.BatchedLTVMPC(nx, nu, N, Q, R, P, u_max=0.4, x_max=8.0, K=K, device=DEV, precision=prec, eps_abs=1e-3)
    Ad, Bd = t(Ad0).expand(B, N, nx, nx).contiguous(), t(Bd0).expand(B, N, nx, nu).contiguous()
    Adt, Bdt = t(Ad0.T), t(Bd0.T)
    plant = lambda x, u: (x @ Adt + u @ Bdt, Ad, Bd, None)
    xref = t(xstar)[:, None, :].expand(B, N, nx).contiguous()
    uref = t(ustar)[:, None, :].expand(B, N, nu).contiguous()
    x0 = t(xstar + 1.0 * rs.randn(B, nx))
    ctl.linearize(Ad, Bd)
    xs, us, _ = ctl.simulate(x0, steps, plant, relinearize_every=5, xref=xref, uref=uref)
    e = (xs - t(xstar)[None]).norm(dim=2)
    print("tracking error: initial %s -> final %s" % (e[0].max().item(), e[-1].max().item()))
    assert torch.all(e[-1] < 0.5 * e[0])
    assert us.abs().max().item() <= 0.4 + 2e-2


def test_two_shards_on_one_gpu_give_the_same_input():
    prec = torch.float64
    one, Ad, Bd, x0, _ = _c3_driver(prec, B=32)
    one.linearize(Ad, Bd)
    u_one, r_one = one.step(x0)
    two, _, _, _, _ = _c3_driver(prec, B=32, devices=[0, 0])
    two.linearize(Ad, Bd)
    u_two, r_two = two.step(x0)
    assert r_one.info.status == r_two.info.status
    assert torch.equal(r_one.info.iter.cpu(), r_two.info.iter.cpu())
    assert (u_one - u_two.to(DEV)).abs().max().item() <= 1e-9
    # a second linearisation goes through update(Hx=, Ax=) on every shard: the same calls on the same data as the one handle
    one.linearize(Ad * 1.001, Bd)
    two.linearize(Ad * 1.001, Bd)
    u_one2, r_one2 = one.step(x0)
    u_two2, r_two2 = two.step(x0)
    assert torch.equal(r_one2.info.iter.cpu(), r_two2.info.iter.cpu())
    assert (u_one2 - u_two2.to(DEV)).abs().max().item() <= 1e-9


def test_unsupported_shape_is_refused_by_the_abi():
    import ctypes
    from reluqp import _cabi
    lib = _cabi.load()
    d = _cabi.LtvDims(batch=2, nx=12, nu=8, horizon=32, dtype=_cabi.RQP_F64, flags=0)
    buf = torch.zeros(16, device=DEV, dtype=torch.float64)
    p = _cabi.ptr(buf)
    assert lib.rqp_ltv_condense(ctypes.byref(d), 0, p, p, None, p, p, p, None, p, p, p, None) == _cabi.RQP_ERR_UNSUPPORTED
    assert b"n = horizon nu <= 160" in lib.rqp_last_error(None)
