"""Condensed QPs of linear time-varying plants, host side (reluqp.mpc.condense_ltv): the LTI identity with
gen_condensed_mpc_qp, correctness against the un-condensed KKT system and the true recursion, the C-ABI names, and
BatchedLTVMPC's argument validation (before any GPU call).  Runs without a GPU."""
import numpy as np
import pytest

from reluqp import _cabi, mpc


def _c3():
    nx, nu, N = 12, 4, 20
    Ad, Bd = mpc.random_plant(nx, nu, seed=0)
    Q, R = np.eye(nx), 0.1 * np.eye(nu)
    K, P = mpc.ihlqr(Ad, Bd, Q, R, Q)
    return nx, nu, N, Ad, Bd, Q, R, P, K


@pytest.mark.parametrize("lqr", [True, False])
def test_lti_identity_with_gen_condensed_mpc_qp(lqr):
    """Constant stages: condense_ltv == gen_condensed_mpc_qp + condensed_x0_update to 1e-12 max|entry| per output.
    With K from ihlqr and Qf = P (lqr=True) the unconstrained optimum is v = 0, so g = F'H_sp G x0 is zero in exact
    arithmetic: its computed entries (~1e-9 here) are what the cancellation of terms of size ~1 leaves, and two summation
    orders differ by ~1e-17 there.  max|entry| of g is therefore taken over the terms that are summed,
    |F|'|H_sp||G||x0| (the scale a backward-stable evaluation of these sums is accurate to); lqr=False (K = 0, Qf = Q)
    has no such cancellation and uses max|g| itself."""
    nx, nu, N, Ad, Bd, Q, R, P, K = _c3()
    if not lqr:
        P, K = Q, None
    A_add, l_add, u_add = mpc.box_constraints(nx, nu, N, 0.4, 8.0)
    H, _, A, _, _, g_x0, lu_x0 = mpc.gen_condensed_mpc_qp(Ad, Bd, Q, R, P, N, A_add, l_add, u_add, K=K)
    cond = mpc.condense_ltv(np.repeat(Ad[None], N, 0), np.repeat(Bd[None], N, 0), Q, R, P, K=K)
    x0 = 1.5 * np.random.RandomState(1).randn(5, nx)
    g_ref, l_ref, u_ref = mpc.condensed_x0_update(g_x0, lu_x0, l_add, u_add, x0)
    for b in range(5):
        g, l, u = mpc.ltv_vectors(cond, x0[b], l_add, u_add)
        gs = (np.abs(cond["F"]).T @ np.abs(cond["H_sp"]) @ np.abs(cond["G"]) @ np.abs(x0[b])).max() if lqr else np.abs(g_ref[b]).max()
        for name, got, want, scale in (("H", cond["H"], H, np.abs(H).max()), ("A", cond["A"], A, np.abs(A).max()),
                                       ("g", g, g_ref[b], gs), ("l", l, l_ref[b], np.abs(l_ref[b]).max()),
                                       ("u", u, u_ref[b], np.abs(u_ref[b]).max())):
            err = np.abs(got - want).max()
            print("%s: max err %.3e (scale %.3e)" % (name, err, scale))
            assert err <= 1e-12 * scale, name


def test_ltv_matches_uncondensed_kkt_and_true_recursion():
    nx, nu, N, Ad0, Bd0, Q, R, P, K = _c3()
    rs = np.random.RandomState(3)
    Ad = Ad0[None] + 0.05 * rs.randn(N, nx, nx)
    Bd = Bd0[None] + 0.05 * rs.randn(N, nx, nu)
    c = 0.1 * rs.randn(N, nx)
    xref, uref = 0.3 * rs.randn(N, nx), 0.1 * rs.randn(N, nu)
    x0 = rs.randn(nx)
    blk, m, n = nx + nu, N * (nx + nu), N * nu
    cond = mpc.condense_ltv(Ad, Bd, Q, R, P, K=K, c=c)
    g, l, u = mpc.ltv_vectors(cond, x0, np.full(m, -1e6), np.full(m, 1e6), xref=xref, uref=uref)    # loose box: nothing active
    v = -np.linalg.solve(cond["H"], g)
    y = cond["F"] @ v + cond["G"] @ x0 + cond["f"]
    assert np.all(l < cond["A"] @ v) and np.all(cond["A"] @ v < u)
    # (a) the true recursion with u_k = -K x_k + v_k reproduces y
    x, roll = x0.copy(), []
    for k in range(N):
        uk = -K @ x + v[k * nu:(k + 1) * nu]
        x = Ad[k] @ x + Bd[k] @ uk + c[k]
        roll += [uk, x]
    roll = np.concatenate(roll)
    scale = np.abs(y).max()
    print("rollout err %.3e, scale %.3e" % (np.abs(roll - y).max(), scale))
    assert np.abs(roll - y).max() <= 1e-9 * scale
    # (b) the un-condensed problem: min 0.5 (y - yref)' H_sp (y - yref)  s.t.  B_k u_k - x_{k+1} + A_k x_k = -c_k
    H_sp = cond["H_sp"]
    yref = np.hstack([np.hstack([uref[k], xref[k]]) for k in range(N)])
    E, rhs = np.zeros((N * nx, m)), np.zeros(N * nx)
    for k in range(N):
        E[k * nx:(k + 1) * nx, k * blk:k * blk + nu] = Bd[k]
        E[k * nx:(k + 1) * nx, k * blk + nu:(k + 1) * blk] = -np.eye(nx)
        if k > 0:
            E[k * nx:(k + 1) * nx, (k - 1) * blk + nu:k * blk] = Ad[k]
        rhs[k * nx:(k + 1) * nx] = -c[k] - (Ad[0] @ x0 if k == 0 else 0)
    KKT = np.block([[H_sp, E.T], [E, np.zeros((N * nx, N * nx))]])
    sol = np.linalg.solve(KKT, np.hstack([H_sp @ yref, rhs]))
    print("kkt err %.3e" % np.abs(sol[:m] - y).max())
    assert np.abs(sol[:m] - y).max() <= 1e-9 * scale


def test_batched_condense_ltv_stacks_instances():
    rs = np.random.RandomState(5)
    Ad, Bd, c = rs.randn(3, 4, 3, 3), rs.randn(3, 4, 3, 2), rs.randn(3, 4, 3)
    K = 0.1 * rs.randn(2, 3)
    cond = mpc.condense_ltv(Ad, Bd, np.eye(3), np.eye(2), 2 * np.eye(3), K=K, c=c)
    one = mpc.condense_ltv(Ad[1], Bd[1], np.eye(3), np.eye(2), 2 * np.eye(3), K=K, c=c[1])
    assert cond["H"].shape == (3, 8, 8) and cond["A"].shape == (3, 20, 8) and cond["f"].shape == (3, 20)
    for k in ("H", "A", "G", "f", "g_x0", "g_f"):
        assert np.array_equal(cond[k][1], one[k]), k
    x0 = rs.randn(3, 3)
    g, l, u = mpc.ltv_vectors(cond, x0, -np.ones(20), np.ones(20), xref=rs.randn(3, 4, 3))
    assert g.shape == (3, 8) and l.shape == (3, 20) and np.all(u - l == pytest.approx(2.0))


def test_abi_names_and_bindings():
    for name in ("rqp_ltv_workspace_bytes", "rqp_ltv_condense", "rqp_ltv_vectors"):
        assert name in _cabi.ABI_SYMBOLS
    import ctypes
    lib = _cabi.load()
    nbytes = ctypes.c_size_t()
    d = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)
    assert lib.rqp_ltv_workspace_bytes(ctypes.byref(d), ctypes.byref(nbytes)) == 0
    n, m = 80, 320
    assert nbytes.value == 8 * 4 * (2 * m * n + m * 13 + n * 13)
    # host-side validation: no device is touched
    assert lib.rqp_ltv_workspace_bytes(None, ctypes.byref(nbytes)) == _cabi.RQP_ERR_ARG
    big = _cabi.LtvDims(batch=4, nx=17, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=0)
    assert lib.rqp_ltv_workspace_bytes(ctypes.byref(big), ctypes.byref(nbytes)) == _cabi.RQP_ERR_UNSUPPORTED
    assert b"nx <= 16" in lib.rqp_last_error(None)
    assert lib.rqp_ltv_workspace_bytes(ctypes.byref(d), ctypes.byref(nbytes)) == 0
    assert lib.rqp_last_error(None) == b""                       # cleared at entry: no stale text after a success
    big = _cabi.LtvDims(batch=4, nx=12, nu=8, horizon=32, dtype=_cabi.RQP_F32, flags=0)      # n = 256 > 160
    assert lib.rqp_ltv_condense(ctypes.byref(big), 0, *([None] * 11)) == _cabi.RQP_ERR_UNSUPPORTED
    assert lib.rqp_ltv_condense(ctypes.byref(d), 0, *([None] * 11)) == _cabi.RQP_ERR_ARG
    assert lib.rqp_ltv_vectors(ctypes.byref(d), 0, *([None] * 13)) == _cabi.RQP_ERR_ARG
    bad = _cabi.LtvDims(batch=4, nx=12, nu=4, horizon=20, dtype=_cabi.RQP_F32, flags=64)
    assert lib.rqp_ltv_workspace_bytes(ctypes.byref(bad), ctypes.byref(nbytes)) == _cabi.RQP_ERR_ARG


def test_batched_ltv_mpc_validates_arguments_before_any_gpu_call():
    Q, R = np.eye(12), 0.1 * np.eye(4)
    ok = dict(nx=12, nu=4, horizon=20, Q=Q, R=R, Qf=Q, u_max=0.4, x_max=8.0)
    ctl = mpc.BatchedLTVMPC(**ok)
    assert (ctl.n, ctl.m) == (80, 320) and ctl.l_add.shape == (320,)
    with pytest.raises(ValueError, match="K has shape"):
        mpc.BatchedLTVMPC(**dict(ok, K=np.zeros((12, 4))))
    with pytest.raises(ValueError, match="Q, Qf must be"):
        mpc.BatchedLTVMPC(**dict(ok, Q=np.eye(11)))
    with pytest.raises(ValueError, match="symmetric"):
        mpc.BatchedLTVMPC(**dict(ok, R=np.triu(np.ones((4, 4)))))
    for bad in (dict(nx=17, Q=np.eye(17), Qf=np.eye(17)), dict(nu=9, R=np.eye(9)), dict(horizon=33), dict(nu=8, R=np.eye(8), horizon=21),
                dict(nx=16, Q=np.eye(16), Qf=np.eye(16), nu=8, R=np.eye(8), horizon=27)):
        with pytest.raises(ValueError, match="unsupported LTV size"):
            mpc.BatchedLTVMPC(**dict(ok, **bad))
    with pytest.raises(ValueError, match=r"\[B, N, nx, nx\]"):
        ctl.linearize(np.zeros((20, 12, 12)), np.zeros((20, 12, 4)))
    with pytest.raises(ValueError, match="stages of shape"):
        ctl.linearize(np.zeros((2, 10, 12, 12)), np.zeros((2, 10, 12, 4)))
    with pytest.raises(ValueError, match="c has shape"):
        ctl.linearize(np.zeros((2, 20, 12, 12)), np.zeros((2, 20, 12, 4)), c=np.zeros((2, 20, 11)))
    with pytest.raises(RuntimeError, match="linearize"):
        ctl.step(np.zeros((2, 12)))
