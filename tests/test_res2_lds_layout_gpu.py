"""The LDS image of the resident float32 kernel (k_admm_res2) on all four tiles, at the edges of each.

k_admm_res2 lays d, dx and g out interleaved by wave block on the two big tiles and back to back on the two small ones, keeps
H x of a check in d's array, and carries float(x) in slot order only for the incoming state; the x update writes x64 / xnat / dx
through their own lane addresses.  A wrong offset, pitch or alias there shows as a wrong iterate on one tile and not on another,
so every tile solves a batch at its largest shape(s) and at the smallest shape that still selects it -- (n, m) one past the
next smaller tile -- and must agree with the streaming kernel (k_admm_generic, which has no such image): the same number of
iterations, the same final rho index, and x, z, y within the float32 kernel-against-streaming tolerances of
test_hip_parity.py (test_wave_equals_generic_small_problems: 5e-5 of max(1, largest entry, largest |x|) for x and z, 40 times
that for the duals, which carry rho-amplified float32 noise; the objective -- the kernel's epilogue reads x64 and H x from d's
array -- within rtol 5e-4, atol 5e-4 as there).  Both handle kinds run: full_ladder (K for every rung) and the rho window.
One case solves twice with warm_starting: the second solve starts from the x, z, lam the first one wrote back, i.e. the state
makes the round trip through the kernel's x64 / xin / xnat.

The instances are seeds of the feasible random-QP generator, n_eq = m // 12, the first six of seeds 0..199 per shape that the
oracle (form "refine", float32) solves with every decision of every check -- both residuals against their thresholds, the rho
estimate against both move thresholds of the current rung -- at least 12 % away from its threshold, so that float32 rounding
differences between the two kernels cannot flip one.  Every shape yielded six.  The warm-start seeds satisfy that in both
solves.  `python tools/res2_pick_seeds.py` (CPU only) prints these lists.
"""
import functools

import numpy as np
import pytest
import torch

from reluqp import utils

pytestmark = pytest.mark.gpu

# (n, m) -> seeds; grouped by the tile the shape selects
SHAPES = {
    # Res2Cfg<2, 4, 2, 4>: n <= 32, m <= 64
    (32, 64): (3, 12, 15, 18, 19, 20),
    (9, 17): (4, 9, 13, 14, 15, 16),
    # Res2Cfg<4, 7, 2, 7>: n <= 56, m <= 128
    (56, 128): (1, 10, 12, 26, 27, 29),
    (33, 65): (0, 1, 8, 11, 17, 18),
    # Res2Cfg<10, 10, 4, 10>: n <= 80, m <= 320
    (80, 320): (0, 5, 6, 9, 10, 15),
    (57, 129): (10, 12, 15, 16, 18, 19),
    # Res2Cfg<10, 13, 4, 13>: n <= 104, m <= 320
    (104, 320): (6, 19, 23, 28, 42, 43),
    (100, 300): (5, 10, 12, 15, 26, 30),
    (81, 129): (3, 7, 11, 12, 16, 17),
}
WARM_SHAPE, WARM_SEEDS = (100, 300), (5, 10, 12, 15, 30, 37)
TOL = 5e-5                                       # test_hip_parity.py: test_wave_equals_generic_small_problems (float32)
WEIGHT = dict(x=1.0, z=1.0, y=40.0)              # ... duals carry rho-amplified float32 noise


@functools.lru_cache(maxsize=None)
def _batch(n, m, seeds):
    n_eq = m // 12
    qps = [utils.rand_qp(n, n_eq, m - n_eq, seed=s, compute_sol=False, feasible=True) for s in seeds]
    return tuple(np.stack([q[k] for q in qps]) for k in range(5))


def _model(n, m, seeds, kernel, full_ladder, warm_starting):
    import reluqp.reluqpth as reluqpth
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    H, g, A, l, u = _batch(n, m, seeds)
    mdl = reluqpth.ReLU_QP()
    mdl.setup(H=H, g=g, A=A, l=l, u=u, device=torch.device("cuda:0"), precision=torch.float32, warm_starting=warm_starting,
              kernel=kernel, full_ladder=full_ladder)
    return mdl


def _take(r):
    return dict(it=r.info.iter.cpu().numpy().copy(), ri=r.info.rho_ind.cpu().numpy().copy(), status=list(r.info.status),
                x=r.x.detach().cpu().double().numpy().copy(), z=r.z.detach().cpu().double().numpy().copy(),
                y=r.y.detach().cpu().double().numpy().copy(), obj=r.info.obj_val.detach().cpu().double().numpy().copy())


def _agree(rr, rg, what):
    print("%s: iterations resident %s generic %s, rho index %s / %s" % (what, rr["it"].tolist(), rg["it"].tolist(),
                                                                          rr["ri"].tolist(), rg["ri"].tolist()))
    scale = float(np.abs(rg["x"]).max())
    atol = {k: WEIGHT[k] * TOL * max(1.0, float(np.abs(rg[k]).max()), scale) for k in "xzy"}
    for k in "xzy":
        print("%s: max|%s resident - generic| = %.3g (tolerance %.3g)" % (what, k, float(np.abs(rr[k] - rg[k]).max()), atol[k]))
    assert all(s == "solved" for s in rg["status"]) and all(s == "solved" for s in rr["status"])
    assert np.array_equal(rr["it"], rg["it"])
    assert np.array_equal(rr["ri"], rg["ri"])
    for k in "xzy":
        np.testing.assert_allclose(rr[k], rg[k], rtol=0, atol=atol[k], err_msg=k)
    print("%s: max|obj resident - generic| = %.3g" % (what, float(np.abs(rr["obj"] - rg["obj"]).max())))
    np.testing.assert_allclose(rr["obj"], rg["obj"], rtol=TOL * 10, atol=TOL * 10, err_msg="obj_val")


@pytest.mark.parametrize("full_ladder", [True, False], ids=["full_ladder", "window"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=["n%d_m%d" % s for s in SHAPES])
def test_tile_edges_resident_equals_generic(shape, full_ladder):
    n, m = shape
    seeds = SHAPES[shape]
    assert len(seeds) == 6
    mr = _model(n, m, seeds, "resident", full_ladder, False)
    mg = _model(n, m, seeds, "generic", full_ladder, False)
    rr, rg = _take(mr.solve()), _take(mg.solve())
    assert mr.kernel == "resident2" and mg.kernel == "generic"
    _agree(rr, rg, "n=%d m=%d" % shape)


@pytest.mark.parametrize("full_ladder", [True, False], ids=["full_ladder", "window"])
def test_warm_start_round_trip(full_ladder):
    n, m = WARM_SHAPE
    mr = _model(n, m, WARM_SEEDS, "resident", full_ladder, True)
    mg = _model(n, m, WARM_SEEDS, "generic", full_ladder, True)
    r1, g1 = _take(mr.solve()), _take(mg.solve())
    r2, g2 = _take(mr.solve()), _take(mg.solve())
    assert mr.kernel == "resident2" and mg.kernel == "generic"
    _agree(r1, g1, "cold solve")
    _agree(r2, g2, "warm solve")
    assert (g2["it"] <= g1["it"]).all() and (g2["it"] < g1["it"]).any()      # the second solve did start from the first one's state
