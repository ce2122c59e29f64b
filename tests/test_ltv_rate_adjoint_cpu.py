"""Reverse mode of the input-rate terms, host side: reluqp.mpc.condense_ltv_vjp(S=, uprev=, dA_r=, dl_r=, du_r=) against central
differences of condense_ltv(S=) + ltv_vectors(uprev=) + rate_constraints, its reduction to the plain vjp, its batch axis and
longdouble path, and the host-side validation of rqp_ltv_condense_adjoint_rate.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest

from reluqp import _cabi, mpc

BARS = ("dH", "dA", "dg", "dl", "du", "dA_r", "dl_r", "du_r")


def _case(nx, nu, N, seed, Sdim, staged):
    """One instance with K, c, references and uprev != 0; S [nu, nu] (Sdim 2) or stage-varying (3); shared or stage weights."""
    rs = np.random.RandomState(seed)
    Ad0, Bd0 = mpc.random_plant(nx, nu, seed=seed)

    def spd(k, *lead):
        W = rs.randn(*lead, k, k)
        return W @ np.swapaxes(W, -1, -2) / k + np.eye(k)

    m, n = N * (nx + nu), N * nu
    P = dict(Ad=Ad0[None] + 0.05 * rs.randn(N, nx, nx), Bd=Bd0[None] + 0.05 * rs.randn(N, nx, nu), c=0.1 * rs.randn(N, nx),
             x0=rs.randn(nx), xref=0.3 * rs.randn(N, nx), uref=0.1 * rs.randn(N, nu),
             Q=spd(nx, N) if staged else spd(nx), R=spd(nu, N) if staged else spd(nu), Qf=None if staged else spd(nx),
             l_add=-np.ones(m) + 0.1 * rs.randn(m), u_add=np.ones(m) + 0.1 * rs.randn(m),
             S=spd(nu, N) if Sdim == 3 else spd(nu), uprev=0.5 * rs.randn(nu), dlo=-0.3 + 0.1 * rs.randn(n), dhi=0.3 + 0.1 * rs.randn(n))
    return P, 0.2 * rs.randn(nu, nx), rs


def _forward(P, K):
    cond = mpc.condense_ltv(P["Ad"], P["Bd"], P["Q"], P["R"], P["Qf"], K=K, c=P["c"], S=P["S"])
    g, l, u = mpc.ltv_vectors(cond, P["x0"], P["l_add"], P["u_add"], xref=P["xref"], uref=P["uref"], uprev=P["uprev"])
    A_r, l_r, u_r = mpc.rate_constraints(cond, P["x0"], P["uprev"], P["dlo"], P["dhi"])
    return cond["H"], cond["A"], g, l, u, A_r, l_r, u_r


def _vjp(P, K, bars, **over):
    kw = dict(zip(BARS, bars))
    kw.update(S=P["S"], uprev=P["uprev"])
    kw.update(over)
    return mpc.condense_ltv_vjp(P["Ad"], P["Bd"], P["Q"], P["R"], P["Qf"], P["x0"], P["l_add"], P["u_add"], K=K, c=P["c"],
                                xref=P["xref"], uref=P["uref"], **kw)


@pytest.mark.parametrize("Sdim,staged", [(3, False), (2, False), (3, True)])
def test_rate_vjp_matches_central_differences(Sdim, staged):
    P, K, rs = _case(3, 2, 4, 11, Sdim, staged)
    bars = [rs.randn(*o.shape) for o in _forward(P, K)]
    loss = lambda P: sum((b * o).sum() for b, o in zip(bars, _forward(P, K)))
    gr = _vjp(P, K, bars)
    h = 1e-6
    names = [k for k in P if P[k] is not None]
    assert {"S", "uprev", "dlo", "dhi"} <= set(names) <= set(gr)
    for name in names:
        d = rs.randn(*gr[name].shape)
        if name in ("Q", "R", "Qf", "S"):
            d = d + np.swapaxes(d, -1, -2)
        Pp, Pm = dict(P), dict(P)
        Pp[name], Pm[name] = P[name] + h * d, P[name] - h * d
        fd = (loss(Pp) - loss(Pm)) / (2 * h)
        an = (gr[name] * d).sum()
        rel = abs(fd - an) / max(abs(fd), abs(an), 1e-300)
        print("S%dd staged=%s %-6s fd % .9e  vjp % .9e  rel %.2e" % (Sdim, staged, name, fd, an, rel))
        assert rel <= 1e-6, name


def test_zero_rate_weight_without_rate_cotangents_is_the_plain_vjp():
    P, K, rs = _case(3, 2, 4, 2, 3, False)
    bars = [rs.randn(*o.shape) for o in _forward(P, K)][:5]
    plain = mpc.condense_ltv_vjp(P["Ad"], P["Bd"], P["Q"], P["R"], P["Qf"], P["x0"], P["l_add"], P["u_add"], K=K, c=P["c"],
                                 xref=P["xref"], uref=P["uref"], **dict(zip(BARS, bars)))
    assert not {"S", "uprev", "dlo", "dhi"} & set(plain)          # without the new keywords: what it returned
    rate = _vjp(P, K, bars, S=np.zeros_like(P["S"]))
    for k in plain:
        assert np.array_equal(plain[k], rate[k]), k
    assert not rate["dlo"].any() and not rate["dhi"].any() and not rate["uprev"].any()
    rows = _vjp(P, K, bars + [None, rs.randn(8), None], S=None)   # the rows alone: S absent is S = 0
    assert rows["S"].shape == (2, 2) and not rows["dhi"].any()
    assert np.array_equal(rows["uprev"], rows["dlo"][:2])        # duprev = t_0 when S = 0


def test_batch_axis_and_per_instance_rate_weight():
    rs = np.random.RandomState(4)
    B, N, nx, nu = 3, 4, 3, 2
    n, m = N * nu, N * (nx + nu)
    cases = [_case(nx, nu, N, 20 + b, 3, False)[0] for b in range(B)]
    K = 0.1 * rs.randn(nu, nx)
    st = lambda k: np.stack([p[k] for p in cases])
    W = (cases[0]["Q"], cases[0]["R"], cases[0]["Qf"])
    bars = dict(dH=rs.randn(B, n, n), dA=rs.randn(B, m, n), dg=rs.randn(B, n), dl=rs.randn(B, m), du=rs.randn(B, m),
                dA_r=rs.randn(B, n, n), dl_r=rs.randn(B, n), du_r=rs.randn(B, n))
    la, ua = -np.ones(m), np.ones(m)
    kw = dict(K=K, c=st("c"), xref=st("xref"), uref=st("uref"))
    full = mpc.condense_ltv_vjp(st("Ad"), st("Bd"), *W, st("x0"), la, ua, S=st("S"), uprev=st("uprev"), **kw, **bars)
    ones = [mpc.condense_ltv_vjp(p["Ad"], p["Bd"], *W, p["x0"], la, ua, K=K, c=p["c"], xref=p["xref"], uref=p["uref"], S=p["S"],
                                 uprev=p["uprev"], **{k: v[b] for k, v in bars.items()}) for b, p in enumerate(cases)]
    assert full["S"].shape == (B, N, nu, nu) and full["uprev"].shape == (B, nu) and full["dlo"].shape == (B, n)
    for k in ("Ad", "Bd", "x0", "S", "uprev", "dlo", "dhi"):
        assert np.array_equal(full[k][1], ones[1][k]), k
    assert np.array_equal(full["S"], np.swapaxes(full["S"], -1, -2))
    assert np.array_equal(full["dlo"], bars["dl_r"]) and np.array_equal(full["dhi"], bars["du_r"])
    shared = mpc.condense_ltv_vjp(st("Ad"), st("Bd"), *W, st("x0"), la, ua, S=cases[0]["S"], uprev=st("uprev"), **kw, **bars)
    one = mpc.condense_ltv_vjp(st("Ad"), st("Bd"), *W, st("x0"), la, ua, S=cases[0]["S"][0], uprev=st("uprev"), **kw, **bars)
    assert shared["S"].shape == (N, nu, nu) and one["S"].shape == (nu, nu)
    per = mpc.condense_ltv_vjp(st("Ad"), st("Bd"), *W, st("x0"), la, ua, S=np.stack([cases[0]["S"]] * B), uprev=st("uprev"), **kw,
                               **bars)
    assert np.allclose(shared["S"], per["S"].sum(0), rtol=0, atol=1e-12 * np.abs(per["S"]).max())
    with pytest.raises(ValueError, match="S has shape"):
        mpc.condense_ltv_vjp(st("Ad"), st("Bd"), *W, st("x0"), la, ua, S=np.zeros((N + 1, nu, nu)), uprev=st("uprev"), **kw, **bars)


def test_longdouble_inputs_keep_their_precision():
    P, K, rs = _case(3, 2, 4, 1, 3, True)
    bars = [rs.randn(*o.shape) for o in _forward(P, K)]
    LD = np.longdouble
    Pl = {k: None if v is None else v.astype(LD) for k, v in P.items()}
    out = _vjp(Pl, K.astype(LD), [b.astype(LD) for b in bars])
    assert all(v.dtype == LD for v in out.values())
    ref = _vjp(P, K, bars)
    for k in ref:
        assert np.abs(out[k].astype(np.float64) - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), k


def test_abi_names_and_host_side_validation():
    for name in ("rqp_ltv_adjoint_rate_workspace_bytes", "rqp_ltv_condense_adjoint_rate"):
        assert name in _cabi.ABI_SYMBOLS
    lib = _cabi.load()
    nbytes, plain = ctypes.c_size_t(), ctypes.c_size_t()
    d = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)
    assert lib.rqp_ltv_adjoint_workspace_bytes(ctypes.byref(d), ctypes.byref(plain)) == 0
    assert lib.rqp_ltv_adjoint_rate_workspace_bytes(ctypes.byref(d), ctypes.byref(nbytes)) == 0
    assert plain.value == 8 * (4 * (320 * 80 + 4 * 320 + 20 * 160) + 256 * 2 * 160)      # the plain size is what it was
    assert nbytes.value == plain.value + 8 * 4 * 2 * 80                                  # and q, r per instance
    io, rio = _cabi.LtvAdjointIO(), _cabi.LtvRateAdjointIO()
    call = lambda dims, io_, rio_: lib.rqp_ltv_condense_adjoint_rate(dims, 0, io_, rio_, None)
    # host-side validation: no device is touched
    assert lib.rqp_ltv_adjoint_rate_workspace_bytes(None, ctypes.byref(nbytes)) == _cabi.RQP_ERR_ARG
    assert lib.rqp_ltv_adjoint_rate_workspace_bytes(ctypes.byref(d), None) == _cabi.RQP_ERR_ARG
    assert call(None, ctypes.byref(io), ctypes.byref(rio)) == _cabi.RQP_ERR_ARG
    big = _cabi.LtvDims(batch=4, nx=17, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)
    for rc in (lib.rqp_ltv_adjoint_rate_workspace_bytes(ctypes.byref(big), ctypes.byref(nbytes)),
               call(ctypes.byref(big), ctypes.byref(io), ctypes.byref(rio))):
        assert rc == _cabi.RQP_ERR_UNSUPPORTED
        assert b"nx <= 16" in lib.rqp_last_error(None)
    bad = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=64)
    assert call(ctypes.byref(bad), ctypes.byref(io), ctypes.byref(rio)) == _cabi.RQP_ERR_ARG
    assert b"unknown flag" in lib.rqp_last_error(None)
    assert call(ctypes.byref(d), ctypes.byref(io), ctypes.byref(rio)) == _cabi.RQP_ERR_ARG        # every pointer NULL
    assert call(ctypes.byref(d), None, ctypes.byref(rio)) == _cabi.RQP_ERR_ARG
    for f in ("Ad", "Bd", "x0", "Q", "R", "Qf", "workspace", "adjoint_workspace"):                # (fake addresses: never read)
        setattr(io, f, 64)
    assert call(ctypes.byref(d), ctypes.byref(io), None) == _cabi.RQP_ERR_ARG
    assert b"rate_io, S and uprev" in lib.rqp_last_error(None)
    rio.S = 64
    assert call(ctypes.byref(d), ctypes.byref(io), ctypes.byref(rio)) == _cabi.RQP_ERR_ARG        # uprev NULL
    rio.uprev, rio.dA_r, rio.dA_stride = 64, 64, 80 * 80 - 1
    assert call(ctypes.byref(d), ctypes.byref(io), ctypes.byref(rio)) == _cabi.RQP_ERR_ARG
    assert b"inst_stride is smaller" in lib.rqp_last_error(None)
    rio.dA_stride = 641 * 80
    assert call(ctypes.byref(d), ctypes.byref(io), ctypes.byref(rio)) == _cabi.RQP_ERR_UNSUPPORTED
    rio.dA_stride, rio.du_r, rio.dl_stride = 80 * 80, 64, 79
    assert call(ctypes.byref(d), ctypes.byref(io), ctypes.byref(rio)) == _cabi.RQP_ERR_ARG
    assert b"inst_stride is smaller" in lib.rqp_last_error(None)
    staged = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=_cabi.LTV_STAGE_WEIGHTS)
    rio.dl_stride, io.dQf = 80, 64
    assert call(ctypes.byref(staged), ctypes.byref(io), ctypes.byref(rio)) == _cabi.RQP_ERR_ARG
    assert b"dQf must be NULL" in lib.rqp_last_error(None)
    assert lib.rqp_ltv_adjoint_rate_workspace_bytes(ctypes.byref(d), ctypes.byref(nbytes)) == 0
    assert lib.rqp_last_error(None) == b""


@pytest.mark.parametrize("stage", [False, True])
def test_layer_fixture_has_active_rate_rows(stage):
    from oracle import reluqp_oracle as O
    import ltv_rate_adjoint_ref as RR
    import ltv_stage_fixture as SF
    p = RR.layer_problem(stage)
    _, H, g, A, l, u, m0 = RR.layer_qp(p)
    assert A.shape == (SF.B, m0 + SF.N * SF.NU, SF.N * SF.NU)
    ref = O.solve_batch(H, g, A, l, u, form="factored", eps_abs=1e-9, max_iter=20000)
    assert all(s == "solved" for s in ref["status"])
    active = RR.rate_active(ref["z"], ref["lam"], l, u, m0)
    print("stage rows %s: instances with an active rate row at the oracle's optimum: %d of %d" % (stage, active.sum(), SF.B))
    assert active.sum() >= SF.B // 4


def test_layer_validates_rate_arguments_before_any_gpu_call():
    import torch
    from reluqp.layer import LTVMPCLayer
    f64 = torch.float64
    Ad, Bd, x0 = torch.zeros(2, 4, 3, 3, dtype=f64), torch.zeros(2, 4, 3, 2, dtype=f64), torch.zeros(2, 3, dtype=f64)
    Q, R = torch.eye(3, dtype=f64), torch.eye(2, dtype=f64)
    up, du, S = torch.zeros(2, 2, dtype=f64), torch.ones(8, dtype=f64), torch.eye(2, dtype=f64)
    with pytest.raises(ValueError, match="m <= 640"):
        LTVMPCLayer(16, 4, 32, 0.4, 8.0, rate_rows=True)       # 640 box rows + 128 rate rows
    rows, plain = LTVMPCLayer(3, 2, 4, 0.4, 8.0, rate_rows=True), LTVMPCLayer(3, 2, 4, 0.4, 8.0)
    with pytest.raises(ValueError, match="du_lo and du_hi must be given"):
        rows(Ad, Bd, x0, Q, R, Q, u_prev=up)
    with pytest.raises(ValueError, match="need u_prev"):
        rows(Ad, Bd, x0, Q, R, Q, du_lo=-du, du_hi=du)
    with pytest.raises(ValueError, match="du_lo has shape"):
        rows(Ad, Bd, x0, Q, R, Q, u_prev=up, du_lo=-du[:7], du_hi=du)
    with pytest.raises(ValueError, match="both"):
        rows(Ad, Bd, x0, Q, R, Q, u_prev=up, du_lo=-du, du_hi=du.expand(2, 8))
    with pytest.raises(ValueError, match="rate_rows=True"):
        plain(Ad, Bd, x0, Q, R, Q, S=S, u_prev=up, du_lo=-du, du_hi=du)
    with pytest.raises(ValueError, match="u_prev needs S"):
        plain(Ad, Bd, x0, Q, R, Q, u_prev=up)
    with pytest.raises(ValueError, match="need u_prev"):
        plain(Ad, Bd, x0, Q, R, Q, S=S)
    with pytest.raises(ValueError, match="u_prev has shape"):
        plain(Ad, Bd, x0, Q, R, Q, S=S, u_prev=up[:1])
    with pytest.raises(ValueError, match="S must be symmetric"):
        plain(Ad, Bd, x0, Q, R, Q, S=torch.triu(torch.ones(2, 2, dtype=f64)), u_prev=up)
    with pytest.raises(ValueError, match="S has shape"):
        plain(Ad, Bd, x0, Q, R, Q, S=torch.ones(3, 2, 2, dtype=f64), u_prev=up)
    with pytest.raises(ValueError, match="precision of Ad"):
        plain(Ad, Bd, x0, Q, R, Q, S=S, u_prev=up.float())
    with pytest.raises(_cabi.RqpUnavailable):                    # host tensors: refused, never a CPU path
        rows(Ad, Bd, x0, Q, R, Q, S=S, u_prev=up, du_lo=-du, du_hi=du)
