"""GPU tests of the fixed-pass window protocol (include/rqp_abi.h: rqp_set_window_passes; ReLU_QP.setup(graph_passes=P)).

A windowed handle (RQP_WINDOW K(rho) entries per matrix) normally reads the count of instances that left their window
after every pass and synchronises the stream, so it cannot be captured into a HIP graph.  With P >= 1 fixed passes it
enqueues the first launch, P gated continuation passes and a finalize kernel, with no host read-back.  The bar:
  * bit-identity with the host loop (and with the full ladder) whenever P covers the passes the solve needs;
  * a captured update(g, l, u) + solve() replays bit-identically to eager solves, with windows moving during replays;
  * an instance the budget does not cover reports "window_passes_exhausted" with its exact state at the stop;
  * handles without the option behave as before.
"""
import numpy as np
import pytest
import torch

from reluqp import utils, _cabi
from reluqp.reluqpth import window_pass_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STATUS_WINDOW_PASSES = 5


def _solver(H, g, A, l, u, prec, full=False, **kw):
    import reluqp.reluqpth as reluqpth
    m = reluqpth.ReLU_QP()
    m.collect_trace = True
    m.prefill_outputs = True
    m.setup(H, g, A, l, u, device=DEV, precision=prec, full_ladder=full, **kw)
    return m


def _snap(res, model):
    i = res.info
    d = dict(x=res.x.clone(), z=res.z.clone(), y=res.y.clone(), iter=i.iter.clone(), status=i.status_code.clone(),
             rho_ind=i.rho_ind.clone(), pri=i.pri_res.clone(), dua=i.dua_res.clone(), rho=i.rho_estimate.clone(),
             obj=i.obj_val.clone(), trace=model.last_trace.clone())
    st, ri = model.get_state()
    d["state"], d["state_ri"] = st.clone(), ri.clone()
    return d


def _eq(x, y):
    if x.is_floating_point():
        return torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0))
    return torch.equal(x, y)


def _same(a, b, what):
    for k in a:
        assert _eq(a[k], b[k]), "%s: %s differs" % (what, k)


CASES = [  # (precision, kernel, n, n_eq, n_ineq, feasible, settings) -- the case list of test_window_gpu.py
    (torch.float32, "resident", 10, 5, 15, False, dict(max_iter=600)),
    (torch.float64, "generic", 10, 5, 15, False, dict(max_iter=600)),
    (torch.float32, "generic", 12, 4, 20, False, dict(max_iter=500, check_interval=10)),
    (torch.float32, "resident", 40, 10, 70, False, dict(max_iter=400)),
    (torch.float64, "generic", 30, 8, 50, True, dict(eps_abs=1e-7, max_iter=2000)),
    (torch.float32, "resident", 100, 25, 275, True, dict(eps_abs=1e-4)),
    (torch.float32, "resident", 72, 18, 150, True, dict(eps_abs=1e-4)),
    (torch.float32, "resident", 33, 8, 60, False, dict(max_iter=400)),
    (torch.float64, "resident", 10, 5, 15, False, dict(max_iter=600)),               # k_admm_res64
    (torch.float64, "resident", 40, 10, 70, False, dict(max_iter=400, check_interval=10)),
    (torch.float64, "resident", 100, 25, 275, True, dict(eps_abs=1e-6)),
    (torch.float32, "wave", 10, 5, 15, False, dict(max_iter=600)),                   # k_admm_wave
    (torch.float64, "wave", 12, 4, 20, False, dict(max_iter=500, check_interval=10)),
    (torch.float32, "wave", 30, 8, 100, False, dict(max_iter=400)),
    (torch.float32, "wave", 60, 10, 90, True, dict(eps_abs=1e-5)),
    (torch.float32, "wave", 32, 8, 56, True, dict(eps_abs=1e-5)),
]


def _bound(st):
    return window_pass_bound(st.get("max_iter", 4000), st.get("check_interval", 25))


def _problem(prec, n, n_eq, n_ineq, feasible, B=48, seed0=11):
    dt = np.float32 if prec == torch.float32 else np.float64
    return utils.rand_qp_batch(B, n, n_eq, n_ineq, seed0=seed0, feasible=feasible, dtype=dt)


@pytest.mark.parametrize("prec,kernel,n,n_eq,n_ineq,feasible,st", CASES)
def test_fixed_passes_bit_identical_to_host_loop(prec, kernel, n, n_eq, n_ineq, feasible, st):
    H, g, A, l, u, _ = _problem(prec, n, n_eq, n_ineq, feasible)
    mh = _solver(H, g, A, l, u, prec, kernel=kernel, **st)                           # host loop (default)
    mp = _solver(H, g, A, l, u, prec, kernel=kernel, graph_passes=_bound(st), **st)  # fixed passes
    mf = _solver(H, g, A, l, u, prec, full=True, kernel=kernel, **st)                # whole ladder
    assert mh.kernel == mp.kernel == mf.kernel
    assert mp.get_window()[0] == 5
    wb0 = mp.get_window()[1].clone()

    def step(what):
        sh, sp, sf = (_snap(m_.solve(), m_) for m_ in (mh, mp, mf))
        assert not bool((sp["status"] == STATUS_WINDOW_PASSES).any()), what
        _same(sp, sh, what + " (fixed passes vs host loop)")
        _same(sp, sf, what + " (fixed passes vs full ladder)")
        assert torch.equal(mp.get_window()[1], mh.get_window()[1])

    step("cold solve")
    if not feasible:
        assert not torch.equal(mp.get_window()[1], wb0), "this case is meant to move windows"
    step("warm re-solve")
    for m_ in (mh, mp, mf):
        m_.update(g=g * 1.25)
    step("after update(g)")
    for m_ in (mh, mp, mf):
        m_.clear_primal_dual()
    step("after clear_primal_dual")


GRAPH_CASES = [  # (precision, kernel, n, n_eq, n_ineq, settings): steps alternate ratchet (infeasible) and feasible vectors
    (torch.float32, "resident", 10, 5, 15, dict(max_iter=600)),
    (torch.float32, "wave", 10, 5, 15, dict(max_iter=600)),
    (torch.float64, "generic", 12, 4, 20, dict(max_iter=500, check_interval=10)),
    (torch.float64, "resident", 40, 10, 70, dict(max_iter=400, check_interval=10)),
]


@pytest.mark.parametrize("prec,kernel,n,n_eq,n_ineq,st", GRAPH_CASES)
def test_captured_update_solve_replays_bit_identical(prec, kernel, n, n_eq, n_ineq, st):
    B = 48
    Hi, gi, Ai, li, ui, _ = _problem(prec, n, n_eq, n_ineq, False, B=B)
    Hf, gf, Af, lf, uf, _ = _problem(prec, n, n_eq, n_ineq, True, B=B)
    assert np.array_equal(Hi, Hf) and np.array_equal(Ai, Af)                # same matrices: only g, l, u change
    tdt = prec
    vecs = []
    for k in range(6):
        g, l, u = (gi, li, ui) if k % 2 == 0 else (gf, lf, uf)
        s = 1.0 + 0.05 * k
        vecs.append(tuple(torch.as_tensor(v, device=DEV, dtype=tdt) for v in (g * s, l, u)))
    mg = _solver(Hi, gi, Ai, li, ui, prec, kernel=kernel, graph_passes=_bound(st), **st)
    me = _solver(Hi, gi, Ai, li, ui, prec, kernel=kernel, **st)
    assert mg.kernel == me.kernel and mg.get_window()[0] == 5
    gs, ls, us = (v.clone() for v in vecs[0])                               # static inputs of the graph

    mg.synchronous = False
    side = torch.cuda.Stream(device=DEV)                                    # warm-up = step 0, on a side stream
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        mg.update(g=gs, l=ls, u=us)
        mg.solve()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    me.update(g=vecs[0][0], l=vecs[0][1], u=vecs[0][2])
    _same(_snap(mg.results, mg), _snap(me.solve(), me), "warm-up step")

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        mg.update(g=gs, l=ls, u=us)
        res = mg.solve()
    moved = 0
    for k in range(1, len(vecs)):
        wb_before = mg.get_window()[1].clone()
        for dst, src in zip((gs, ls, us), vecs[k]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        me.update(g=vecs[k][0], l=vecs[k][1], u=vecs[k][2])
        se = _snap(me.solve(), me)
        sg = _snap(res, mg)
        assert not bool((sg["status"] == STATUS_WINDOW_PASSES).any())
        _same(sg, se, "replay %d" % k)
        assert torch.equal(mg.get_window()[1], me.get_window()[1])
        moved += int((mg.get_window()[1] != wb_before).sum())
    assert moved > 0, "windows were meant to move during the replays"


RATCHET = [(torch.float32, "resident"), (torch.float64, "generic"), (torch.float32, "wave"), (torch.float64, "resident")]


def _passes_needed(snap, ci, max_iter, nrho, wb0=6, kwin=5):
    """Continuation passes each instance of a fresh handle's cold solve needed, replayed from the host loop's trace: an
    instance leaves when its incoming index lies outside the window, or when a check moves the index out of it (not at the
    last iteration, not at the converging check); its new window is centred on the index, clipped to the ladder."""
    tr, ri_end, st = snap["trace"].cpu().numpy(), snap["rho_ind"].cpu().numpy(), snap["status"].cpu().numpy()
    centre = lambda ri: min(max(ri - kwin // 2, 0), nrho - kwin)
    out = []
    for b in range(tr.shape[0]):
        rows = tr[b][~np.isnan(tr[b, :, 3])]
        ris = [int(r) for r in rows[:, 3]] + [int(ri_end[b])]
        wb, p = wb0, 0
        if not wb <= ris[0] < wb + kwin:
            wb, p = centre(ris[0]), p + 1
        for c in range(len(rows)):
            last = c == len(rows) - 1
            if ris[c + 1] != ris[c] and (c + 1) * ci < max_iter and not (last and st[b] == 0) and not wb <= ris[c + 1] < wb + kwin:
                wb, p = centre(ris[c + 1]), p + 1
        out.append(p)
    return np.array(out)


@pytest.mark.parametrize("prec,kernel", RATCHET)
def test_pass_budget_exhausted(prec, kernel):
    st = dict(max_iter=600)
    H, g, A, l, u, _ = _problem(prec, 10, 5, 15, False)
    mh = _solver(H, g, A, l, u, prec, kernel=kernel, **st)
    sh = _snap(mh.solve(), mh)
    nrho = len(mh._rhos)
    need = _passes_needed(sh, 25, 600, nrho)
    assert need.max() >= 3 and int(sh["rho_ind"].max()) >= 14             # the ratchet: 7 -> 11 -> 14 -> 17 and beyond
    mP = _solver(H, g, A, l, u, prec, kernel=kernel, graph_passes=int(need.max()), **st)
    _same(_snap(mP.solve(), mP), sh, "graph_passes = the passes the solve needs")
    m1 = _solver(H, g, A, l, u, prec, kernel=kernel, graph_passes=1, **st)
    s1 = _snap(m1.solve(), m1)

    ex = s1["status"] == STATUS_WINDOW_PASSES
    assert int(ex.sum()) > 0, "the ratchet is meant to exhaust one pass"
    assert np.array_equal(ex.cpu().numpy(), need > 1)                      # exactly the instances that needed more passes
    ok = ~ex
    for k in sh:                                                             # instances that needed <= 1 pass: as the host loop
        assert _eq(s1[k][ok], sh[k][ok]), k
    assert not bool((s1["status"] == 0)[ex].any())                         # never "solved" wrongly

    ci, n = 25, H.shape[1]
    for b in torch.nonzero(ex).flatten().tolist():
        it = int(s1["iter"][b])
        assert 0 < it < int(sh["iter"][b]) and it % ci == 0
        c = it // ci                                                          # checks run before the stop
        assert bool(torch.isnan(s1["pri"][b])) and bool(torch.isnan(s1["dua"][b])) and bool(torch.isnan(s1["obj"][b]))
        ri = int(s1["rho_ind"][b])
        assert 0 <= ri < nrho and ri == int(sh["trace"][b, c, 3])             # the index after that check (host trajectory)
        assert float(s1["rho"][b]) == float(sh["trace"][b, c - 1, 2])         # the carried estimate of that check
        assert _eq(s1["trace"][b, :c], sh["trace"][b, :c])
        assert bool(torch.isnan(s1["trace"][b, c:]).all())
        assert torch.equal(s1["x"][b], s1["state"][b, :n]) and int(s1["state_ri"][b]) == ri   # the exact state at the stop
    # the next eager solve on that handle continues every instance like any other
    r = m1.solve()
    sc = r.info.status_code
    assert bool(((sc == 0) | (sc == 1) | (sc == STATUS_WINDOW_PASSES)).all())
    assert not bool(torch.isnan(r.x).any()) and bool((r.info.iter >= 0).all())


def test_exhausted_cold_start_clears_state():
    """warm_starting = False: an exhausted instance leaves the cleared state a finished one leaves."""
    prec, st = torch.float32, dict(max_iter=600, warm_starting=False)
    H, g, A, l, u, _ = _problem(prec, 10, 5, 15, False)
    m1 = _solver(H, g, A, l, u, prec, kernel="resident", graph_passes=1, **st)
    s1 = _snap(m1.solve(), m1)
    ex = s1["status"] == STATUS_WINDOW_PASSES
    assert int(ex.sum()) > 0
    assert bool((s1["state"][ex] == 0).all()) and bool((s1["state_ri"][ex] == 7).all())
    assert not bool((s1["x"][ex] == 0).all())                              # the outputs carry the state at the stop


def test_handles_without_the_option():
    B, n, n_eq, n_ineq = 40, 10, 3, 12
    H, g, A, l, u, _ = utils.rand_qp_batch(B, n, n_eq, n_ineq, seed0=5, feasible=True, dtype=np.float32)
    # a windowed handle without the option still refuses capture
    mw = _solver(H, g, A, l, u, torch.float32, kernel="resident")
    assert mw.get_window()[0] == 5
    mw.synchronous = False
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        mw.solve()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    dummy = torch.zeros(8, device=DEV)
    err = None
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        dummy.add_(1.0)
        try:
            mw.solve()
        except _cabi.RqpError as e:
            err = e
    torch.cuda.synchronize()
    assert err is not None and err.code == _cabi.RQP_ERR_UNSUPPORTED and "FULL_LADDER" in str(err)
    # handles that are not windowed: graph_passes changes nothing
    for args, kw in (((H, g, A, l, u), dict(full=True, kernel="resident")),
                     ((H[:8], g[:8], A[:8], l[:8], u[:8]), dict(kernel="resident")),
                     ((H[0], g, A[0], l, u), dict())):
        m0 = _solver(*args, torch.float32, **kw)
        m4 = _solver(*args, torch.float32, graph_passes=4, **kw)
        assert m0.get_window()[1] is None and m4.get_window()[1] is None
        _same(_snap(m4.solve(), m4), _snap(m0.solve(), m0), "not windowed: %s" % kw)
        _same(_snap(m4.solve(), m4), _snap(m0.solve(), m0), "not windowed, warm: %s" % kw)
    with pytest.raises(_cabi.RqpError):
        _solver(H, g, A, l, u, torch.float32, graph_passes=-1)
