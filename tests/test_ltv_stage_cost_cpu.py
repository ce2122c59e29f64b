"""Stage-varying, per-instance cost weights of the LTV condensing, host side: reluqp.mpc.condense_ltv / ltv_vectors /
condense_ltv_vjp with Q [N, nx, nx] or [B, N, nx, nx] and R likewise against a dense construction written out here and
against central differences, the argument checks of the wrappers, the driver and the layer, and the margins of the layer
fixture the GPU test differentiates (tests/ltv_stage_cost_fixture.py).  Runs without a GPU."""
import numpy as np
import pytest

from oracle import reluqp_oracle as O
from reluqp import _cabi, mpc

import ltv_adjoint_fixture as FX
import ltv_stage_cost_fixture as SF


def _plant(B, nx, nu, N, seed):
    rs = np.random.RandomState(seed)
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)
    Ad = Ad0[None, None] + 0.05 * rs.randn(B, N, nx, nx)
    Bd = Bd0[None, None] + 0.05 * rs.randn(B, N, nx, nu)
    P = dict(Ad=Ad, Bd=Bd, c=0.1 * rs.randn(B, N, nx), x0=rs.randn(B, nx), xref=0.3 * rs.randn(B, N, nx), uref=0.1 * rs.randn(B, N, nu),
             K=0.2 * rs.randn(nu, nx))
    m = N * (nx + nu)
    P["l_add"], P["u_add"] = -np.ones(m) + 0.1 * rs.randn(m), np.ones(m) + 0.1 * rs.randn(m)
    return P, rs


def _dense(P, b, Qb, Rb):
    """(H, g_x0, g_f, g) of instance b from the maps F, G, f (which do not depend on the weights) and an explicit H_sp."""
    N, nx, nu = Qb.shape[0], Qb.shape[1], Rb.shape[1]
    maps = mpc.condense_ltv(P["Ad"][b], P["Bd"][b], np.eye(nx), np.eye(nu), np.eye(nx), K=P["K"], c=P["c"][b])
    F, G, f = maps["F"], maps["G"], maps["f"]
    S = SF.dense_H_sp(Qb, Rb)
    H = F.T @ S @ F
    yref = np.hstack([P["uref"][b], P["xref"][b]]).reshape(-1)
    g = F.T @ S @ (G @ P["x0"][b] + f - yref)
    return 0.5 * (H + H.T), F.T @ S @ G, F.T @ S @ f, g, S


def _near(got, ref):
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (np.abs(got - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize("kind", ["BN_BN", "N_N", "BN_N", "BN_shared", "shared_BN", "N_shared", "shared_N"])
def test_staged_condensing_matches_the_dense_construction(kind):
    B, nx, nu, N = 3, 4, 2, 5
    P, rs = _plant(B, nx, nu, N, 3)
    Q4, R4 = SF.stage_weights(rs, B, N, nx, nu)
    Qsh, Rsh, Qf = SF.spd_blocks(rs, (1,), nx)[0], SF.spd_blocks(rs, (1,), nu, 0.1)[0], 3.0 * SF.spd_blocks(rs, (1,), nx)[0]
    qk, rk = kind.split("_")
    Q = dict(BN=Q4, N=Q4[1], shared=Qsh)[qk]
    R = dict(BN=R4, N=R4[2], shared=Rsh)[rk]
    qf = Qf if qk == "shared" else None
    # the blocks of instance b, written out
    Qb = lambda b: dict(BN=Q4[b], N=Q4[1], shared=np.stack([Qsh] * (N - 1) + [Qf]))[qk]
    Rb = lambda b: dict(BN=R4[b], N=R4[2], shared=np.stack([Rsh] * N))[rk]
    cond = mpc.condense_ltv(P["Ad"], P["Bd"], Q, R, qf, K=P["K"], c=P["c"])
    g, l, u = mpc.ltv_vectors(cond, P["x0"], P["l_add"], P["u_add"], xref=P["xref"], uref=P["uref"])
    assert cond["H_sp"].ndim == (3 if "BN" in kind else 2)
    for b in range(B):
        H, gx, gf, gg, S = _dense(P, b, Qb(b), Rb(b))
        _near(cond["H"][b], H)
        _near(cond["g_x0"][b], gx)
        _near(cond["g_f"][b], gf)
        _near(g[b], gg)
        assert np.array_equal(cond["H_sp"][b] if cond["H_sp"].ndim == 3 else cond["H_sp"], S)
        # one instance, no batch axis anywhere
        one = mpc.condense_ltv(P["Ad"][b], P["Bd"][b], Qb(b) if qk != "shared" else Qsh, Rb(b) if rk != "shared" else Rsh, qf,
                               K=P["K"], c=P["c"][b])
        g1, l1, u1 = mpc.ltv_vectors(one, P["x0"][b], P["l_add"], P["u_add"], xref=P["xref"][b], uref=P["uref"][b])
        assert np.array_equal(one["H"], cond["H"][b]) and np.array_equal(g1, g[b])
        assert np.array_equal(l1, l[b]) and np.array_equal(u1, u[b])
    # a block from the wrong stage or instance is far outside the bound (the weights grow with k and b)
    H1 = _dense(P, 1, Qb(1), Rb(1))[0]
    wrong = _dense(P, 1, np.roll(Qb(1), 1, axis=0), Rb(1))[0]
    assert np.abs(wrong - H1).max() > 1e-3 * np.abs(H1).max()


def test_repeated_shared_weights_are_bitwise_the_shared_call():
    B, nx, nu, N = 2, 5, 2, 6
    P, rs = _plant(B, nx, nu, N, 4)
    Q, R, Qf = SF.spd_blocks(rs, (1,), nx)[0], SF.spd_blocks(rs, (1,), nu, 0.1)[0], 2.0 * SF.spd_blocks(rs, (1,), nx)[0]
    Qs, Rs = SF.repeated(Q, R, Qf, B, N)
    shared = mpc.condense_ltv(P["Ad"], P["Bd"], Q, R, Qf, K=P["K"], c=P["c"])
    for Qv, Rv, qf in ((Qs, Rs, None), (Qs[0], Rs[0], None), (Qs, R, None), (Q, Rs[0], Qf)):
        staged = mpc.condense_ltv(P["Ad"], P["Bd"], Qv, Rv, qf, K=P["K"], c=P["c"])
        for k in ("H", "g_x0", "g_f", "F", "G", "f"):
            assert np.array_equal(staged[k], shared[k]), k
        gs = mpc.ltv_vectors(staged, P["x0"], P["l_add"], P["u_add"], xref=P["xref"], uref=P["uref"])
        g0 = mpc.ltv_vectors(shared, P["x0"], P["l_add"], P["u_add"], xref=P["xref"], uref=P["uref"])
        for a, b in zip(gs, g0):
            assert np.array_equal(a, b)


def _one(P, b=0):
    return {k: (v[b] if k not in ("K", "l_add", "u_add") else v) for k, v in P.items()}


def _forward(P, Q, R, Qf):
    cond = mpc.condense_ltv(P["Ad"], P["Bd"], Q, R, Qf, K=P["K"], c=P["c"])
    g, l, u = mpc.ltv_vectors(cond, P["x0"], P["l_add"], P["u_add"], xref=P["xref"], uref=P["uref"])
    return cond["H"], cond["A"], g, l, u


def _vjp(P, Q, R, Qf, bars):
    return mpc.condense_ltv_vjp(P["Ad"], P["Bd"], Q, R, Qf, P["x0"], P["l_add"], P["u_add"], K=P["K"], c=P["c"], xref=P["xref"],
                                uref=P["uref"], **dict(zip(("dH", "dA", "dg", "dl", "du"), bars)))


@pytest.mark.parametrize("shape", [(3, 2, 4), (5, 2, 6), (12, 4, 20)])
def test_staged_vjp_matches_central_differences(shape):
    """The method and bounds of tests/test_ltv_adjoint_cpu.py::test_vjp_matches_central_differences (h = 1e-5, relative 1e-6);
    Q_k and R_k are perturbed one entry at a time, symmetrically, the other inputs along a random direction."""
    nx, nu, N = shape
    Pb, rs = _plant(1, nx, nu, N, 7)
    P = _one(Pb)
    Q4, R4 = SF.stage_weights(rs, 1, N, nx, nu)
    W = dict(Q=Q4[0], R=R4[0])
    bars = [rs.randn(*o.shape) for o in _forward(P, W["Q"], W["R"], None)]
    loss = lambda P, W: sum((b * o).sum() for b, o in zip(bars, _forward(P, W["Q"], W["R"], None)))
    gr = _vjp(P, W["Q"], W["R"], None, bars)
    assert "Qf" not in gr and gr["Q"].shape == (N, nx, nx) and gr["R"].shape == (N, nu, nu)
    assert np.array_equal(gr["Q"], np.swapaxes(gr["Q"], 1, 2)) and np.array_equal(gr["R"], np.swapaxes(gr["R"], 1, 2))
    h = 1e-5

    def check(tag, fd, an):
        rel = abs(fd - an) / max(abs(fd), abs(an), 1e-300)
        print("%s %-12s fd % .9e  vjp % .9e  rel %.2e" % (shape, tag, fd, an, rel))
        assert rel <= 1e-6, tag

    for name in ("Ad", "Bd", "c", "x0", "xref", "uref", "l_add", "u_add"):
        d = rs.randn(*gr[name].shape)
        Pp, Pm = dict(P), dict(P)
        Pp[name], Pm[name] = P[name] + h * d, P[name] - h * d
        check(name, (loss(Pp, W) - loss(Pm, W)) / (2 * h), (gr[name] * d).sum())
    for name, dim in (("Q", nx), ("R", nu)):
        entries = [(0, 0, 0), (N - 1, dim - 1, 0), (N - 1, dim - 1, dim - 1), (N // 2, 0, dim - 1), (1, dim // 2, dim // 2)]
        for k, i, j in entries:
            d = np.zeros_like(W[name])
            d[k, i, j] = d[k, j, i] = 1.0
            Wp, Wm = dict(W), dict(W)
            Wp[name], Wm[name] = W[name] + h * d, W[name] - h * d
            check("%s[%d][%d,%d]" % (name, k, i, j), (loss(P, Wp) - loss(P, Wm)) / (2 * h), (gr[name] * d).sum())


def test_staged_vjp_stacks_a_batched_weight_and_sums_a_shared_one():
    B, nx, nu, N = 3, 3, 2, 4
    P, rs = _plant(B, nx, nu, N, 5)
    Q4, R4 = SF.stage_weights(rs, B, N, nx, nu)
    n, m = N * nu, N * (nx + nu)
    bars = [rs.randn(B, n, n), rs.randn(B, m, n), rs.randn(B, n), rs.randn(B, m), rs.randn(B, m)]
    full = _vjp(P, Q4, R4, None, bars)
    assert full["Q"].shape == (B, N, nx, nx) and full["R"].shape == (B, N, nu, nu) and "Qf" not in full
    ones = [_vjp(_one(P, b), Q4[b], R4[b], None, [v[b] for v in bars]) for b in range(B)]
    for b in range(B):
        for k in ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R"):
            assert np.array_equal(full[k][b], ones[b][k]), (k, b)
    # [N, ., .] shared by the batch: the sum over the instances
    sh = _vjp(P, Q4[1], R4, None, bars)
    assert sh["Q"].shape == (N, nx, nx) and sh["R"].shape == (B, N, nu, nu)
    ones = [_vjp(_one(P, b), Q4[1], R4[b], None, [v[b] for v in bars]) for b in range(B)]
    ref = sum(o["Q"] for o in ones)
    assert np.abs(sh["Q"] - ref).max() <= 1e-12 * np.abs(ref).max()
    # a shared Q beside a staged R: Q summed over the stages below the last, Qf the last, R per stage
    Qsh, Qf = SF.spd_blocks(rs, (1,), nx)[0], 2.0 * SF.spd_blocks(rs, (1,), nx)[0]
    mix = _vjp(P, Qsh, R4[0], Qf, bars)
    rep = _vjp(P, np.stack([Qsh] * (N - 1) + [Qf]), R4[0], None, bars)
    assert mix["Q"].shape == (nx, nx) and mix["Qf"].shape == (nx, nx) and mix["R"].shape == (N, nu, nu)
    assert np.abs(mix["Q"] - rep["Q"][:N - 1].sum(0)).max() <= 1e-12 * np.abs(mix["Q"]).max()
    assert np.abs(mix["Qf"] - rep["Q"][N - 1]).max() <= 1e-12 * np.abs(mix["Qf"]).max()
    assert np.array_equal(mix["R"], rep["R"])


def test_longdouble_stage_weights_keep_their_precision():
    nx, nu, N = 3, 2, 4
    Pb, rs = _plant(1, nx, nu, N, 1)
    P = _one(Pb)
    Q4, R4 = SF.stage_weights(rs, 1, N, nx, nu)
    LD = np.longdouble
    Pl = {k: v.astype(LD) for k, v in P.items()}
    outs = _forward(Pl, Q4[0].astype(LD), R4[0].astype(LD), None)
    assert all(o.dtype == LD for o in outs)
    bars = [rs.randn(*o.shape) for o in outs]
    out = _vjp(Pl, Q4[0].astype(LD), R4[0].astype(LD), None, [b.astype(LD) for b in bars])
    assert all(v.dtype == LD for v in out.values())
    ref = _vjp(P, Q4[0], R4[0], None, bars)
    for k in ref:
        assert np.abs(out[k].astype(np.float64) - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), k


def test_the_flag_is_a_bit_of_its_own():
    flag = _cabi.LTV_STAGE_WEIGHTS
    others = [getattr(_cabi, k) for k in dir(_cabi) if k.startswith("LTV_") and k != "LTV_STAGE_WEIGHTS"]
    assert len(others) >= 6
    assert flag > 0 and flag & (flag - 1) == 0                  # one bit
    for o in others:
        assert flag & o == 0
    # 64 stays what the earlier tests use it for, a bit no rqp_ltv_* call knows; the stage weights are the next one
    assert flag == 128


def test_numpy_statements_refuse_bad_stage_weights():
    B, nx, nu, N = 2, 3, 2, 4
    P, rs = _plant(B, nx, nu, N, 2)
    Q4, R4 = SF.stage_weights(rs, B, N, nx, nu)
    for fn in (lambda Q, R, Qf: mpc.condense_ltv(P["Ad"], P["Bd"], Q, R, Qf),
               lambda Q, R, Qf: mpc.condense_ltv_vjp(P["Ad"], P["Bd"], Q, R, Qf, P["x0"], P["l_add"], P["u_add"])):
        with pytest.raises(ValueError, match="Qf must be None"):
            fn(Q4, R4, np.eye(nx))
        with pytest.raises(ValueError, match="Q has shape"):
            fn(Q4[:, :3], R4, None)
        with pytest.raises(ValueError, match="R has shape"):
            fn(Q4, R4[:, :, :1], None)
        with pytest.raises(ValueError, match="batch of 1"):
            fn(Q4[:1], R4, None)
        with pytest.raises(ValueError, match="needs Qf"):
            fn(np.eye(nx), R4, None)
    with pytest.raises(ValueError, match="batch axis"):          # one instance cannot take [B, N, ., .]
        mpc.condense_ltv(P["Ad"][0], P["Bd"][0], Q4, R4[0], None)


def test_driver_and_wrappers_validate_stage_weights_before_any_gpu_call():
    nx, nu, N, B = 12, 4, 20, 2
    rs = np.random.RandomState(0)
    Q4, R4 = SF.stage_weights(rs, B, N, nx, nu)
    Qa = Q4.copy()
    Qa[1, 3, 0, 1] += 1e-3
    with pytest.raises(ValueError, match="symmetric"):
        mpc._LtvStageWeights(nx, nu, N, Qa, R4, None, None)
    with pytest.raises(ValueError, match="Qf must be None"):
        mpc._LtvStageWeights(nx, nu, N, Q4, R4, np.eye(nx), None)
    with pytest.raises(ValueError, match="R has shape"):
        mpc._LtvStageWeights(nx, nu, N, Q4, R4[:, :, :3, :3], None, None)
    with pytest.raises(ValueError, match="K has shape"):
        mpc._LtvStageWeights(nx, nu, N, Q4, R4, None, np.zeros((nx, nu)))
    w = mpc._LtvStageWeights(nx, nu, N, Q4[0], R4, None, None)
    assert w.staged and w.batch == B and mpc._LtvStageWeights(nx, nu, N, Q4[0], R4[0], None, None).batch is None
    ctl = mpc.BatchedLTVMPC(nx, nu, N, np.eye(nx), 0.1 * np.eye(nu), np.eye(nx), u_max=0.4, x_max=8.0)
    Ad, Bd = np.zeros((B, N, nx, nx)), np.zeros((B, N, nx, nu))
    with pytest.raises(ValueError, match="Q has shape"):
        ctl.linearize(Ad, Bd, Q=Q4[:, :N - 1])
    with pytest.raises(ValueError, match="Q has shape"):
        ctl.linearize(Ad, Bd, Q=np.eye(nx))                      # a shared matrix belongs to the constructor
    with pytest.raises(ValueError, match="R has shape"):
        ctl.linearize(Ad, Bd, Q=Q4, R=R4[:1])
    with pytest.raises(ValueError, match="symmetric"):
        ctl.linearize(Ad, Bd, Q=Qa)
    assert ctl._stage_weights is None                            # nothing was kept from the refused calls


def test_layer_validates_stage_weights_before_any_gpu_call():
    import torch
    from reluqp.layer import LTVMPCLayer
    nx, nu, N, B = 3, 1, 4, 2
    layer = LTVMPCLayer(nx, nu, N, 0.4, 8.0, K=np.zeros((nu, nx)))
    f64 = torch.float64
    Ad, Bd, x0 = torch.zeros(B, N, nx, nx, dtype=f64), torch.zeros(B, N, nx, nu, dtype=f64), torch.zeros(B, nx, dtype=f64)
    Q4 = torch.eye(nx, dtype=f64).expand(B, N, nx, nx).contiguous()
    R4 = torch.eye(nu, dtype=f64).expand(B, N, nu, nu).contiguous()
    with pytest.raises(ValueError, match="Qf must be None"):
        layer(Ad, Bd, x0, Q4, R4, torch.eye(nx, dtype=f64))
    with pytest.raises(ValueError, match="Q has shape"):
        layer(Ad, Bd, x0, Q4[:, :3], R4, None)
    with pytest.raises(ValueError, match="R has shape"):
        layer(Ad, Bd, x0, Q4, R4[0, :2], None)
    with pytest.raises(ValueError, match="batch of 3"):          # mixed batch sizes
        layer(Ad, Bd, x0, Q4, torch.eye(nu, dtype=f64).expand(3, N, nu, nu).contiguous(), None)
    with pytest.raises(ValueError, match="batch of 1"):
        layer(Ad, Bd, x0, Q4[:1], R4, None)
    with pytest.raises(ValueError, match="needs Qf"):
        layer(Ad, Bd, x0, torch.eye(nx, dtype=f64), R4, None)
    with pytest.raises(ValueError, match="Qf must be a torch tensor"):
        layer(Ad, Bd, x0, torch.eye(nx, dtype=f64), torch.eye(nu, dtype=f64), None)
    Qa = Q4.clone()
    Qa[1, 2, 0, 1] = 0.5
    with pytest.raises(ValueError, match="Q must be symmetric"):
        layer(Ad, Bd, x0, Qa, R4, None)
    for Q, R in ((Q4, R4), (Q4[0], R4), (Q4, R4[0])):
        with pytest.raises(_cabi.RqpUnavailable):                # host tensors: refused, never a CPU path
            layer(Ad, Bd, x0, Q, R, None)


def test_driver_case_keeps_the_oracles_two_precisions_on_the_same_iterations():
    """The seed of the driver test (GPU): on the host-condensed staged QPs the oracle's float32 run takes the iterations of its
    float64 run, so a device that differs from the oracle differs for a reason of its own."""
    H, g, A, l, u = SF.driver_qp(SF.driver_case())
    ref = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-3)
    f32 = lambda a: a.astype(np.float32)
    ref32 = O.solve_batch(f32(H), f32(g), f32(A), f32(l), f32(u), form="factored", eps_abs=1e-3, dtype=np.float32)
    print("iterations f64 %s\niterations f32 %s" % (ref["iter"], ref32["iter"]))
    assert all(s == "solved" for s in ref["status"]) and ref32["status"] == ref["status"]
    assert np.mean(ref32["iter"] == ref["iter"]) >= 0.9


@pytest.mark.parametrize("shape,factor", [(s, 1.0) for s in SF.SHAPES] + [(SF.SHAPES[0], f) for f in SF.FACTORS[1:]])
def test_layer_fixture_has_active_sets_with_margins_on_every_instance(shape, factor):
    """The check of tests/test_ltv_adjoint_cpu.py::test_fixture_has_active_sets_with_margins_on_every_instance on the
    stage-weight problems (and on the rescaled weights of the stale-workspace test)."""
    nx, nu, N = shape
    n = N * nu
    p = SF.problem(*shape, factor=factor)
    assert p["Q"].shape == (SF.B, N, nx, nx) and p["R"].shape == (SF.B, N, nu, nu) and p["Qf"] is None
    H, A, g, l, u = SF.condensed(p)
    ref = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-6)
    assert all(s == "solved" for s in ref["status"])
    act = FX.classify(ref["z"], ref["lam"], l, u)
    nonempty = 0
    for b in range(SF.B):
        x, y, dist, mult = FX.margins(H[b], A[b], g[b], l[b], u[b], act[b])
        na = int((act[b] != 0).sum())
        err = np.abs(x - ref["x"][b]).max()
        print("%s instance %2d: %2d active rows, inactive distance %.2e, active |y| %.2e, |x_exact - x_oracle| %.1e"
              % (shape, b, na, dist, mult, err))
        assert err <= 1e-4 * max(1.0, np.abs(x).max())          # two orders above the oracle's eps_abs = 1e-6 exit
        assert dist >= FX.MARGIN and mult >= FX.MARGIN
        assert na <= n // 2
        nonempty += na > 0
    assert nonempty >= SF.B // 2
