"""GPU tests of solution polishing (include/rqp_abi.h: rqp_set_polish / rqp_get_polish; ReLU_QP.setup(polish=True)).

The bar:
  * accuracy on the headline generator: polished answers reach the planted optimum to float64 accuracy (float64 handles) or
    equal the float64 reduced-KKT solution of the float32-rounded data (float32 handles), >= 100x below the ADMM error;
  * on every solve path, the polished point is the numpy restatement's (tests/polish_ref.py) for the reported active set,
    and that set is the classification rule applied to the plain handle's final iterate;
  * nothing else moves: iteration counts, exits, rho indices and estimates, the handle's ADMM state, and every output of
    an instance polish did not accept are bit-identical to a handle without polish;
  * both outcomes of the acceptance rule happen, polish stays capturable, shards gather its results.
"""
import numpy as np
import pytest
import torch

from reluqp import mpc, utils
import reluqp.reluqpth as reluqpth

import polish_ref as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _solver(H, g, A, l, u, prec, **kw):
    m = reluqpth.ReLU_QP()
    m.prefill_outputs = True
    m.setup(H, g, A, l, u, device=DEV, precision=prec, **kw)
    return m


def _np(t):
    return t.detach().cpu().double().numpy()


def _snap(res, model):
    i = res.info
    d = dict(x=res.x.clone(), z=res.z.clone(), y=res.y.clone(), iter=i.iter.clone(), status=i.status_code.clone(),
             rho_ind=i.rho_ind.clone(), pri=i.pri_res.clone(), dua=i.dua_res.clone(), rho=i.rho_estimate.clone(),
             obj=i.obj_val.clone())
    if i.status_polish is not None:
        d["spol"], d["act"] = i.status_polish.clone(), res.active.clone()
    st, ri = model.get_state()
    d["state"], d["state_ri"] = st.clone(), ri.clone()
    return d


def _eq(a, b):
    return torch.equal(a, b) or bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _check_outcomes(sp, s0):
    """The invariants every polished solve keeps against the plain handle's solve `s0`."""
    for k in ("iter", "status", "rho_ind", "rho", "state", "state_ri"):
        assert _eq(sp[k], s0[k]), k
    spol = sp["spol"]
    solved = s0["status"] == 0
    assert bool((spol[~solved] == 0).all())                                  # not solved: not attempted
    assert bool((spol[solved] != 0).all())
    keep = spol != 1
    for k in ("x", "z", "y", "pri", "dua", "obj"):                           # rejected / not attempted: the ADMM outputs
        assert _eq(sp[k][keep], s0[k][keep]), k
    acc = spol == 1
    assert bool((sp["pri"][acc] <= s0["pri"][acc]).all()) and bool((sp["dua"][acc] <= s0["dua"][acc]).all())
    assert bool((sp["act"][~solved] == 0).all())


def _check_kkt(sp, H, g, A, l, u, shared, rtol, idx=None):
    """Accepted instances: x, z, y equal the numpy restatement for the reported active set."""
    acc = np.nonzero(_np(sp["spol"]) == 1)[0]
    if idx is not None:
        acc = np.intersect1d(acc, idx)
    assert len(acc)
    act = sp["act"].cpu().numpy()
    x, z, y = _np(sp["x"]), _np(sp["z"]), _np(sp["y"])
    for b in acc:
        Hb, Ab = (H, A) if shared else (H[b], A[b])
        xr, zr, yr = P.polish(Hb, g[b], Ab, l[b], u[b], act[b])
        sx, sy = 1 + np.abs(xr).max(), 1 + np.abs(yr).max()
        assert np.abs(x[b] - xr).max() <= rtol * sx, (b, np.abs(x[b] - xr).max())
        assert np.abs(z[b] - zr).max() <= rtol * (1 + np.abs(zr[np.isfinite(zr)]).max()), b
        assert np.abs(y[b] - yr).max() <= rtol * sy * 1e2, (b, np.abs(y[b] - yr).max())


def _f32(*arrs):
    return [a.astype(np.float32).astype(np.float64) for a in arrs]


# ------------------------------------------------------------------------------------------------------------- 1. accuracy
def _accuracy(prec, n_ineq):
    n = 100
    H, g, A, l, u, xs = utils.rand_qp_batch(256, n, 25, n_ineq, seed0=0, feasible=True)
    m0 = _solver(H, g, A, l, u, prec)
    s0 = _snap(m0.solve(), m0)
    mp = _solver(H, g, A, l, u, prec, polish=True)
    sp = _snap(mp.solve(), mp)
    _check_outcomes(sp, s0)
    spol = _np(sp["spol"])
    nact = (sp["act"].cpu().numpy() != 0).sum(1)
    acc = spol == 1
    x, x0 = _np(sp["x"]), _np(s0["x"])
    err = np.abs(x - xs).max(1)
    err0 = np.abs(x0 - xs).max(1)
    if prec == torch.float64:
        # a polished point with vanishing residuals IS the optimum (H is positive definite): the planted x_sol
        exact = acc & (_np(sp["pri"]) < 1e-9) & (_np(sp["dua"]) < 1e-9)
        assert exact.sum() >= 0.5 * acc.sum(), (exact.sum(), acc.sum())
        assert bool((err[exact] <= 1e-8 * (1 + np.abs(xs[exact]).max(1))).all()), err[exact].max()
    else:
        Hf, gf, Af, lf, uf = _f32(H, g, A, l, u)
        _check_kkt(sp, Hf, gf, Af, lf, uf, False, 2e-6)
        exact = acc & (_np(sp["pri"]) < 1e-5) & (_np(sp["dua"]) < 1e-5)
        assert exact.sum() >= 0.5 * acc.sum(), (exact.sum(), acc.sum())
    assert err[exact].max() * 100 <= np.median(err0), (err[exact].max(), np.median(err0))
    return spol, nact <= n


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
def test_accuracy_headline_generator(prec):
    """The headline shape (n = 100, m = 300).  Its planted active sets hold ~110 rows, more than n, on most instances:
    x is then unique but the multipliers are not, the regularised solve picks small ones, and their projection onto the
    sign cone breaks the dual residual -- OSQP's rule rejects (measured: ~10 % accepted)."""
    spol, licq = _accuracy(prec, 275)
    assert (spol == 1).sum() >= 10
    assert (spol == 1)[licq].mean() >= 0.5, ((spol == 1)[licq].mean(), licq.sum())


@pytest.mark.parametrize("prec", [torch.float64, torch.float32])
def test_accuracy_fewer_active_rows_than_variables(prec):
    """The same generator with 175 inequalities: ~80 active rows, unique multipliers (measured: ~90 % accepted)."""
    spol, licq = _accuracy(prec, 175)
    assert licq.mean() >= 0.9
    assert (spol == 1).mean() >= 0.8, (spol == 1).mean()


# -------------------------------------------------------------------------------------------------------- 2. solve paths
def _shared_dense(n, n_eq, n_ineq, B, seed=5):
    H, g0, A, l0, u0, _ = utils.rand_qp(n, n_eq, n_ineq, seed=seed, compute_sol=False, feasible=True)
    qs = [utils.update_qp(H, A, n_eq, n_ineq, seed=50 + b, compute_sol=False, feasible=True) for b in range(B)]
    g, l, u = (np.stack([q[i] for q in qs]) for i in (1, 3, 4))
    return H, g, A, l, u


def _sparse_mpc(B, seed=1):
    Ad, Bd = mpc.random_plant(12, 4, seed=0)
    ctl = mpc.LinearMPC(Ad, Bd, np.eye(12), 0.1 * np.eye(4), 20, 0.5, 10.0, form="sparse")
    x0 = np.random.RandomState(seed).randn(B, 12)
    g, l, u = ctl.qp_vectors(x0)
    return ctl.H, g, ctl.A, l, u


PATHS = {
    # name: (problem, precision, setup keywords, expected kernel)
    "generic": ("dense", torch.float64, dict(kernel="generic"), "generic"),
    "resident_windowed": ("dense", torch.float32, dict(kernel="resident"), "resident2"),
    "resident_full_ladder": ("dense", torch.float32, dict(kernel="resident", full_ladder=True), "resident2"),
    "resident_fp16_tile": ("dense", torch.float32, dict(kernel="resident", iterate_dtype=torch.float16), "resident2"),
    "res64": ("dense", torch.float64, dict(kernel="resident"), "resident64"),
    "wave": ("small", torch.float32, dict(kernel="wave"), "wave"),
    "mfma_f32": ("shared", torch.float32, dict(kernel="mfma"), "mfma"),
    "mfma_bf16": ("shared", torch.float32, dict(kernel="mfma", iterate_dtype=torch.bfloat16), "mfma16"),
    "mfmal_chunked": ("sparse_mpc", torch.float32, dict(kernel="mfma"), "mfmal"),
    "mfmad": ("shared", torch.float64, dict(kernel="mfma"), "mfmad"),
    "scaling": ("dense", torch.float64, dict(kernel="generic", scaling=10), "generic"),
    # warm_starting = 0 keeps the state through the polish chain: on k_admm_mfmal that replaces the regrouped two-launch cold
    # solve by one launch -- same results (_check_outcomes: bit-identical iterations, exits, state, rejected outputs)
    "mfmal_cold": ("sparse_mpc_small", torch.float32, dict(kernel="mfma", warm_starting=False), "mfmal"),
    # 128 < n <= 192: the column-oriented products of k_polish leave a quarter of the workgroup idle
    "generic_n150_f64": ("n150", torch.float64, dict(kernel="generic"), "generic"),
    "generic_n150_f32": ("n150", torch.float32, dict(kernel="generic"), "generic"),
    # the factor classes with a float64 output that polish had not run: k_factor_fast (113 <= n <= 128), the LDS-mode k_factor
    # (129 <= n <= 141) and the global-slab k_factor (n > 320, its scratch aliased onto G_a).  Measured: every instance solved
    # and accepted (8 / 8, 8 / 8, 4 / 4 in both precisions, as 16 / 16 at n = 150), so the floor of 0.8 below holds for them too
    "generic_n120_f64": ("n120", torch.float64, dict(kernel="generic"), "generic"),
    "generic_n120_f32": ("n120", torch.float32, dict(kernel="generic"), "generic"),
    "generic_n136_f64": ("n136", torch.float64, dict(kernel="generic"), "generic"),
    "generic_n136_f32": ("n136", torch.float32, dict(kernel="generic"), "generic"),
    "generic_n324_f64": ("n324", torch.float64, dict(kernel="generic"), "generic"),
    "generic_n324_f32": ("n324", torch.float32, dict(kernel="generic"), "generic"),
}


def _problem(kind):
    if kind == "dense":
        return utils.rand_qp_batch(64, 40, 10, 60, seed0=7, feasible=True) + (False,)
    if kind == "sparse_mpc_small":
        return _sparse_mpc(64) + (None, True)
    if kind == "n150":
        return utils.rand_qp_batch(16, 150, 10, 100, seed0=13, feasible=True) + (False,)
    if kind == "n120":
        return utils.rand_qp_batch(8, 120, 10, 80, seed0=17, feasible=True) + (False,)
    if kind == "n136":
        return utils.rand_qp_batch(8, 136, 10, 90, seed0=19, feasible=True) + (False,)
    if kind == "n324":
        return utils.rand_qp_batch(4, 324, 10, 100, seed0=23, feasible=True) + (False,)
    if kind == "small":
        return utils.rand_qp_batch(64, 20, 5, 30, seed0=9, feasible=True) + (False,)
    if kind == "shared":
        return _shared_dense(60, 10, 100, 64) + (None, True)
    return _sparse_mpc(704) + (None, True)        # 704 > the 655 instances of one 1 GiB chunk at n = 320


@pytest.mark.parametrize("name", list(PATHS))
def test_every_solve_path(name):
    kind, prec, kw, kernel = PATHS[name]
    H, g, A, l, u, xs, shared = _problem(kind)
    m0 = _solver(H, g, A, l, u, prec, **kw)
    assert m0.kernel == kernel
    s0 = _snap(m0.solve(), m0)
    mp = _solver(H, g, A, l, u, prec, polish=True, **kw)
    sp = _snap(mp.solve(), mp)
    _check_outcomes(sp, s0)
    spol = _np(sp["spol"])
    act = sp["act"].cpu().numpy()
    licq = (act != 0).sum(1) <= H.shape[-1]
    print("polish %s: accepted %d of %d LICQ instances (%d solved of %d)"
          % (name, (spol == 1)[licq].sum(), licq.sum(), int((s0["status"] == 0).sum()), len(spol)))
    assert (spol == 1)[licq].mean() >= 0.8, ((spol == 1)[licq].mean(), licq.sum())
    solved = _np(s0["status"]) == 0
    if prec == torch.float64 and "scaling" not in kw:                        # the rule on the plain handle's final iterate
        ref = P.classify(_np(s0["z"]), _np(s0["y"]), l, u)
        assert np.array_equal(act[solved], ref[solved])
    data = (H, g, A, l, u) if prec == torch.float64 else _f32(H, g, A, l, u)
    if "scaling" in kw:
        # the rule applies in the scaled space; the polished x is the planted optimum in the caller's space
        acc = spol == 1
        close = np.abs(_np(sp["x"])[acc] - xs[acc]).max(1) <= 1e-7 * (1 + np.abs(xs).max())
        assert close.mean() >= 0.95, close.mean()
        return
    idx = None
    if kind == "sparse_mpc":                                                  # a sample from both chunks
        idx = np.r_[0:8, 650:670, 696:704]
    rtol = 1e-8 if prec == torch.float64 else 2e-6
    _check_kkt(sp, *data, shared, rtol, idx)


# ------------------------------------------------------------------------------------------------ 2b. condensed linear MPC
@pytest.mark.parametrize("prec,kernel,warm", [(torch.float32, "mfma", False), (torch.float32, "mfma", True),
                                              (torch.float32, "resident", False), (torch.float64, "mfma", False)])
def test_condensed_mpc_is_polished(prec, kernel, warm):
    """The condensed MPC form (n = 80, m = 320, shared H and A; 5-40 active rows, well-conditioned H): nearly every solved
    instance is polished.  A batch of <= 16 tiles per CU on the MFMA kernel hands its stragglers to the resident kernel; with
    warm_starting = 0 that continuation pass must keep the state of the other instances for polish (measured: 489 / 512)."""
    Ad, Bd = mpc.random_plant(12, 4, seed=0)
    ctl = mpc.LinearMPC(Ad, Bd, np.eye(12), 0.1 * np.eye(4), 20, 0.5, 10.0, form="condensed")
    g, l, u = ctl.qp_vectors(np.random.RandomState(1).randn(512, 12))
    m0 = _solver(ctl.H, g, ctl.A, l, u, prec, kernel=kernel, warm_starting=warm)
    s0 = _snap(m0.solve(), m0)
    mp = _solver(ctl.H, g, ctl.A, l, u, prec, kernel=kernel, warm_starting=warm, polish=True)
    assert mp.kernel == m0.kernel
    sp = _snap(mp.solve(), mp)
    _check_outcomes(sp, s0)
    spol = _np(sp["spol"])
    assert (spol == 1).mean() >= 0.9, (spol == 1).mean()
    data = (ctl.H, g, ctl.A, l, u) if prec == torch.float64 else _f32(ctl.H, g, ctl.A, l, u)
    _check_kkt(sp, *data, True, 1e-8 if prec == torch.float64 else 2e-6, idx=np.arange(0, 512, 16))


# -------------------------------------------------------------------------------------------------- 3. nothing else moves
@pytest.mark.parametrize("warm", [True, False])
def test_state_and_sequence_unchanged(warm):
    H, g, A, l, u, _ = utils.rand_qp_batch(64, 30, 8, 50, seed0=21, feasible=True)
    models = [_solver(H, g, A, l, u, torch.float32, warm_starting=warm, polish=p) for p in (False, True)]
    rng = np.random.RandomState(0)
    for k in range(3):
        if k:
            g2 = g + 0.05 * rng.randn(*g.shape)
            for mdl in models:
                mdl.update(g=g2)
        s0 = _snap(models[0].solve(), models[0])
        sp = _snap(models[1].solve(), models[1])
        _check_outcomes(sp, s0)
        assert int((sp["spol"] == 1).sum()) > 0


# ------------------------------------------------------------------------------------------------------- 4. rejection path
def test_not_solved_instances_are_not_attempted():
    H, g, A, l, u, _ = utils.rand_qp_batch(32, 30, 8, 50, seed0=31, feasible=True)
    m0 = _solver(H, g, A, l, u, torch.float64, max_iter=50, full_ladder=True)
    s0 = _snap(m0.solve(), m0)
    mp = _solver(H, g, A, l, u, torch.float64, max_iter=50, full_ladder=True, polish=True)
    sp = _snap(mp.solve(), mp)
    unsolved = s0["status"] != 0
    assert int(unsolved.sum()) > 0
    _check_outcomes(sp, s0)
    assert bool((sp["spol"][unsolved] == 0).all())


def test_poor_polish_is_rejected():
    H, g, A, l, u, _ = utils.rand_qp_batch(32, 30, 8, 50, seed0=41, feasible=True)
    kw = dict(eps_abs=1e-7, full_ladder=True)
    m0 = _solver(H, g, A, l, u, torch.float64, **kw)
    s0 = _snap(m0.solve(), m0)
    mp = _solver(H, g, A, l, u, torch.float64, polish=True, delta=1e-1, polish_refine_iter=0, **kw)
    sp = _snap(mp.solve(), mp)
    _check_outcomes(sp, s0)
    solved = s0["status"] == 0
    assert int(solved.sum()) > 0
    assert bool((sp["spol"][solved] == -1).all()), sp["spol"]
    # switching polish off / on after setup
    mp.update_settings(polish=False)
    so = _snap(mp.solve(), mp)
    assert mp.results.info.status_polish is None and "spol" not in so
    m1 = _solver(H, g, A, l, u, torch.float64, **kw)                      # a plain handle at the same point of its sequence
    m1.solve()
    s1 = _snap(m1.solve(), m1)
    for k in ("x", "z", "y", "iter", "status", "rho_ind", "pri", "dua", "obj", "state", "state_ri"):
        assert _eq(so[k], s1[k]), k
    with pytest.raises(ValueError):
        m0.update_settings(polish=True)


# ---------------------------------------------------------------------------------------------------------------- 5. capture
@pytest.mark.parametrize("mode", ["full_ladder", "graph_passes"])
def test_capture_replays_bit_identically(mode):
    H, g, A, l, u, _ = utils.rand_qp_batch(64, 30, 8, 50, seed0=51, feasible=True)
    kw = dict(full_ladder=True) if mode == "full_ladder" else dict(graph_passes=reluqpth.window_pass_bound(4000, 25))
    rng = np.random.RandomState(1)
    vecs = [(g + 0.05 * rng.randn(*g.shape), l, u) for _ in range(3)]
    me = _solver(H, g, A, l, u, torch.float32, polish=True, **kw)
    mg = _solver(H, g, A, l, u, torch.float32, polish=True, **kw)
    gs, ls, us = (torch.as_tensor(v, device=DEV, dtype=torch.float32).clone() for v in vecs[0])
    mg.synchronous = False
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                    # warm-up outside the capture (allocator, LDS attributes)
        mg.update(g=gs, l=ls, u=us)
        mg.solve()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    me.update(g=vecs[0][0], l=vecs[0][1], u=vecs[0][2])
    me.solve()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        mg.update(g=gs, l=ls, u=us)
        res = mg.solve()
    for k in range(1, len(vecs)):
        for dst, src in zip((gs, ls, us), vecs[k]):
            dst.copy_(torch.as_tensor(src, device=DEV, dtype=torch.float32))
        graph.replay()
        torch.cuda.synchronize()
        me.update(g=vecs[k][0], l=vecs[k][1], u=vecs[k][2])
        se = _snap(me.solve(), me)
        sg = _snap(res, mg)
        for key in se:
            assert _eq(sg[key], se[key]), (k, key)
        assert int((sg["spol"] == 1).sum()) > 0


# ---------------------------------------------------------------------------------------------- 6. shards, single QP form
def test_shards_and_single_qp():
    H, g, A, l, u, _ = utils.rand_qp_batch(48, 30, 8, 50, seed0=61, feasible=True)
    m1 = _solver(H, g, A, l, u, torch.float64, polish=True)
    r1 = m1.solve()
    ms = reluqpth.ReLU_QP()
    ms.setup(H, g, A, l, u, device=DEV, precision=torch.float64, polish=True, devices=[0, 0, 0])
    rs = ms.solve()
    for a, b in ((r1.x, rs.x), (r1.z, rs.z), (r1.y, rs.y), (r1.info.status_polish, rs.info.status_polish),
                 (r1.active, rs.active), (r1.info.pri_res, rs.info.pri_res), (r1.info.obj_val, rs.info.obj_val)):
        assert _eq(a, b)
    assert int((rs.info.status_polish == 1).sum()) > 0
    mq = reluqpth.ReLU_QP()
    mq.setup(H[0], g[0], A[0], l[0], u[0], device=DEV, precision=torch.float64, polish=True)
    rq = mq.solve()
    assert isinstance(rq.info.status_polish, int) and rq.info.status_polish in (-1, 0, 1)
    assert tuple(rq.active.shape) == (A.shape[1],)
    m0 = reluqpth.ReLU_QP()
    m0.setup(H[0], g[0], A[0], l[0], u[0], device=DEV, precision=torch.float64)
    r0 = m0.solve()
    assert r0.info.status_polish is None and r0.active is None
    if rq.info.status_polish == 1:
        assert float(rq.info.pri_res) <= float(r0.info.pri_res)


# ------------------------------------------------------------------------------------------------------ 7. update(Hx, Ax)
@pytest.mark.parametrize("shared", [False, True])
def test_matrix_update_is_polished_with_the_new_matrices(shared):
    if shared:
        H, g, A, l, u = _shared_dense(30, 8, 50, 32, seed=71)
        H2, g2, A2, l2, u2 = _shared_dense(30, 8, 50, 32, seed=72)
    else:
        H, g, A, l, u, _ = utils.rand_qp_batch(32, 30, 8, 50, seed0=71, feasible=True)
        H2, g2, A2, l2, u2, xs2 = utils.rand_qp_batch(32, 30, 8, 50, seed0=171, feasible=True)
    mp = _solver(H, g, A, l, u, torch.float64, polish=True, warm_starting=False)
    mp.solve()
    mp.update(g=g2, l=l2, u=u2, Hx=H2, Ax=A2)
    sp = _snap(mp.solve(), mp)
    assert int((sp["spol"] == 1).sum()) > 0
    _check_kkt(sp, H2, g2, A2, l2, u2, shared, 1e-8)
    if not shared:
        acc = _np(sp["spol"]) == 1
        assert np.abs(_np(sp["x"])[acc] - xs2[acc]).max() <= 1e-7
