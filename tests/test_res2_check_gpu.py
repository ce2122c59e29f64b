"""The check of the resident float32 kernel (k_admm_res2) against the streaming kernel on a batch whose rho index moves often.

A check of k_admm_res2 takes its row norms inside the row pass, forms A' lam and H x in one transposed pass, reduces its
eight quantities as a reduce-scatter and, at a rho move, leaves the K reload in flight until K is next read.  None of that
may change a decision: on every instance the resident and the streaming kernel must run the same number of iterations, end
at the same rho index and walk the same per-check rho-index path; the per-check residuals and the carried rho estimate
agree within the float32 trace tolerance of test_hip_parity.py (5e-2 relative / 1e-3 absolute; the carried estimate
max(2e-2, 2 * 5e-2) relative where both residuals exceed 1e-6).

The instances are seeds of the feasible random-QP generator (n = 100, m = 300: the big tile) picked on the CPU with the
oracle (form "refine", float32): solved, and every decision of every check -- both residuals against their thresholds, the
estimate against both move thresholds of the current rung -- at least 12 % away from its threshold, i.e. more than twice
the trace tolerance, so that float32 rounding differences between the two kernels cannot flip one.  Among them the oracle
moves rho at least twice on more than half; the test asserts that on the device, too (otherwise the in-flight K reload
is not exercised).
"""
import numpy as np
import pytest
import torch

from reluqp import utils

pytestmark = pytest.mark.gpu

N, N_EQ, N_INEQ = 100, 25, 275
SEEDS = (9010, 9011, 9012, 9013, 9015, 9017, 9024, 9028, 9029, 9030, 9040, 9041, 9051, 9055, 9057, 9064,
         9066, 9072, 9078, 9089, 9092, 9099, 9100, 9102, 9109, 9112, 9113, 9123, 9132, 9139, 9147, 9148)
RES_RTOL, RES_ATOL = 5e-2, 1e-3                  # test_hip_parity.py: PREC (float32 residual traces)
RHO_RTOL = max(2e-2, 2 * RES_RTOL)               # test_hip_parity.py: _check_vs_gold (the carried estimate compounds)


def _batch():
    qps = [utils.rand_qp(N, N_EQ, N_INEQ, seed=s, compute_sol=False, feasible=True) for s in SEEDS]
    return [np.stack([q[k] for q in qps]) for k in range(5)]


def _run(kernel, full_ladder):
    import reluqp.reluqpth as reluqpth
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    H, g, A, l, u = _batch()
    m = reluqpth.ReLU_QP()
    m.collect_trace = True
    m.setup(H=H, g=g, A=A, l=l, u=u, device=torch.device("cuda:0"), precision=torch.float32, warm_starting=False,
            kernel=kernel, full_ladder=full_ladder)
    r = m.solve()
    return m, r, m.last_trace.detach().cpu().double().numpy()


@pytest.mark.parametrize("full_ladder", [True, False], ids=["full_ladder", "window"])
def test_check_path_resident_equals_generic(full_ladder):
    mr, rr, tr = _run("resident", full_ladder)
    mg, rg, tg = _run("generic", full_ladder)
    assert mr.kernel == "resident2" and mg.kernel == "generic"
    itr, itg = rr.info.iter.cpu().numpy(), rg.info.iter.cpu().numpy()
    rir, rig = rr.info.rho_ind.cpu().numpy(), rg.info.rho_ind.cpu().numpy()
    print("iterations resident %s\niterations generic  %s" % (itr.tolist(), itg.tolist()))
    assert all(s == "solved" for s in rg.info.status) and all(s == "solved" for s in rr.info.status)
    nchk = min(tr.shape[1], tg.shape[1])
    moved = []
    worst = [0.0, 0.0, 0.0]
    for b in range(len(SEEDS)):
        c = int(itg[b]) // 25                                  # checks this instance ran (check_interval = 25)
        assert c <= nchk
        pr, pg = tr[b, :c], tg[b, :c]
        path = np.append(pg[:, 3], rig[b])
        moved.append(int((np.diff(path) != 0).sum()))
        for e in range(2):
            worst[e] = max(worst[e], float(np.max(np.abs(pr[:, e] - pg[:, e]) / (RES_ATOL + RES_RTOL * np.abs(pg[:, e])))))
        ok = (pg[:, 0] > 1e-6) & (pg[:, 1] > 1e-6)
        if ok.any():
            worst[2] = max(worst[2], float(np.max(np.abs(pr[ok, 2] / pg[ok, 2] - 1.0))) / RHO_RTOL)
    print("rho moves per instance %s" % moved)
    print("worst trace deviation / tolerance: pri %.3g dua %.3g rho_est %.3g" % tuple(worst))
    assert np.array_equal(itr, itg)
    assert np.array_equal(rir, rig)
    for b in range(len(SEEDS)):
        c = int(itg[b]) // 25
        pr, pg = tr[b, :c], tg[b, :c]
        assert np.array_equal(pr[:, 3], pg[:, 3]), "rho-index path of instance %d" % b
        np.testing.assert_allclose(pr[:, :2], pg[:, :2], rtol=RES_RTOL, atol=RES_ATOL)
        ok = (pg[:, 0] > 1e-6) & (pg[:, 1] > 1e-6)
        np.testing.assert_allclose(pr[ok, 2], pg[ok, 2], rtol=RHO_RTOL)
    # the batch must exercise the in-flight K reload: at least half of the instances move rho at least twice
    assert np.mean(np.array(moved) >= 2) >= 0.5, moved
