"""CPU checks behind tests/test_kkt_edges_gpu.py: the generator's new `n_active` keyword leaves the default draws as they were,
its planted points are stationary with the docstring's margins at every shape of tests/kkt_edges_fixture.py (the empty,
equality-only and cap-sized active sets among them), and the two numpy references the kernels are held to
(adjoint_ref.adjoint_batch, sensitivity_ref.jvp_batch) agree with each other there through the duality identity."""
import numpy as np
import pytest

import adjoint_ref as R
import kkt_edges_fixture as F


def _margin_qp_batch_before(B, n, n_eq, n_ineq, seed, shared=False):
    """The draw order of margin_qp_batch before it took `n_active` (kept here: the default draws must not move)."""
    rs = np.random.RandomState(seed)
    m = n_eq + n_ineq
    Hs, As = R._matrices(rs, n, n_eq, n_ineq) if shared else (None, None)
    out = {k: [] for k in ("H", "g", "A", "l", "u", "x", "y", "z", "active")}
    cap = n // 2 - n_eq
    for _ in range(B):
        H, A = (Hs, As) if shared else R._matrices(rs, n, n_eq, n_ineq)
        side = rs.choice([-1, 0, 1], size=n_ineq, p=[0.25, 0.5, 0.25])
        on = np.flatnonzero(side)
        if len(on) > cap:
            side[rs.permutation(on)[:len(on) - cap]] = 0
        x = rs.randn(n)
        ax = A @ x
        mag = rs.uniform(0.5, 1.5, size=m)
        s_lo = rs.uniform(0.5, 1.5, size=m)
        s_up = rs.uniform(0.5, 1.5, size=m)
        act = np.concatenate([np.where(rs.randn(n_eq) > 0, 1, -1), side]).astype(np.int8)
        y = act * mag
        l = ax - s_lo
        u = ax + s_up
        l[act < 0] = ax[act < 0]
        u[act > 0] = ax[act > 0]
        l[:n_eq] = u[:n_eq] = ax[:n_eq]
        g = -H @ x - A.T @ y
        for k, v in (("H", H), ("g", g), ("A", A), ("l", l), ("u", u), ("x", x), ("y", y), ("z", ax), ("active", act)):
            out[k].append(v)
    res = {k: np.stack(v) for k, v in out.items()}
    if shared:
        res["H"], res["A"] = Hs, As
    return res


@pytest.mark.parametrize("seed,shape,shared", [(3, (5, 12, 3, 21), False), (31, (4, 10, 2, 30), True)])
def test_default_draws_are_unchanged(seed, shape, shared):
    """(the second shape draws more than n / 2 - n_eq nonzero sides: the trimming branch runs too)"""
    new = R.margin_qp_batch(*shape, seed=seed, shared=shared)
    old = _margin_qp_batch_before(*shape, seed=seed, shared=shared)
    assert set(new) == set(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k
    nact = (new["active"][:, shape[2]:] != 0).sum(1)
    assert nact.max() <= shape[1] // 2 - shape[2]
    if shared:
        assert (nact == shape[1] // 2 - shape[2]).any()


def _check_planted(d, n_eq):
    """sym(H) x + g + A'y = 0; multipliers and slacks with the docstring's margins; equality rows l == u == Ax."""
    B = d["x"].shape[0]
    shared = d["H"].ndim == 2
    for b in range(B):
        H, A = (d["H"], d["A"]) if shared else (d["H"][b], d["A"][b])
        g, l, u, x, y, z, act = (d[k][b] for k in ("g", "l", "u", "x", "y", "z", "active"))
        Hs = 0.5 * (H + H.T)
        scale = 1 + np.abs(Hs @ x).max() + np.abs(g).max()
        assert np.abs(Hs @ x + g + A.T @ y).max() <= 1e-12 * scale, b
        assert np.array_equal(z, A @ x)
        on, lo, up = act != 0, act < 0, act > 0
        assert (np.abs(y[on]) >= 0.5).all() and (np.abs(y[on]) <= 1.5).all() and (y[~on] == 0).all()
        assert (np.sign(y) == act).all()
        assert (z[lo] == l[lo]).all() and (z[up] == u[up]).all()
        free_lo, free_up = ~lo, ~up
        free_lo[:n_eq] = free_up[:n_eq] = False
        for slack in ((z - l)[free_lo], (u - z)[free_up]):
            assert (slack >= 0.5 - 1e-12).all() and (slack <= 1.5 + 1e-12).all()
        assert (l[:n_eq] == u[:n_eq]).all() and on[:n_eq].all()


@pytest.mark.parametrize("shape,n_active", F.SHAPES, ids=[F.shape_id(s) for s, _ in F.SHAPES])
def test_planted_points_and_reference_duality(shape, n_active):
    n, n_eq, n_ineq, B = shape
    m = n_eq + n_ineq
    cap = min(n // 2 - n_eq, n_ineq)
    assert n_active[0] == 0 and n_active[1] == cap and len(n_active) == B
    assert all((n_eq + k) % 4 for k in n_active[2:])
    d = F.per_instance(shape, n_active)
    assert ((d["active"][:, n_eq:] != 0).sum(1) == np.asarray(n_active)).all()
    if n_eq == 0:                                              # an empty active set: y = 0 and l < A x < u
        assert (d["active"][0] == 0).all() and (d["y"][0] == 0).all()
        assert (d["l"][0] < d["z"][0]).all() and (d["z"][0] < d["u"][0]).all()
    _check_planted(d, n_eq)
    gx, gy = F.cotangents(shape)
    ndir = 2                                                   # (the identity holds per direction: two are enough here)
    v = F.tangents(B, n, m, ndir, seed=1)
    assert F.duality_gap(d, gx, gy, v, ndir) <= 1e-9


def test_shared_batch_is_planted():
    n, n_eq, n_ineq = F.SHARED
    d = R.margin_qp_batch(5, n, n_eq, n_ineq, seed=F.seed_of(F.SHARED + (5,)), shared=True)
    assert d["H"].shape == (n, n) and d["A"].shape == (n_eq + n_ineq, n)
    _check_planted(d, n_eq)
    gx, gy = F.cotangents(F.SHARED + (5,))
    v = F.tangents(5, n, n_eq + n_ineq, 2, seed=1, shared_mats=True)
    assert F.duality_gap(d, gx, gy, v, 2) <= 1e-9


def test_n_active_is_checked():
    with pytest.raises(AssertionError):
        R.margin_qp_batch(2, 12, 2, 20, seed=0, n_active=[0, 5])       # above the cap of 12 // 2 - 2 = 4
    with pytest.raises(AssertionError):
        R.margin_qp_batch(2, 12, 2, 20, seed=0, n_active=[0])          # one count per instance
