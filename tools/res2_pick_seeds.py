#!/usr/bin/env python3
"""Seeds for tests/test_res2_lds_layout_gpu.py, picked on the CPU with the oracle (no GPU needed):

    python tools/res2_pick_seeds.py [--count 6] [--first 200] [--margin 0.12]

For every (n, m) of the test, n_eq = m // 12, the first `count` seeds of 0 .. first-1 of the feasible random-QP generator that
the oracle (form "refine", float32) solves with every decision of every check at least `margin` away from its threshold:
both residuals against eps_abs sqrt(m) / eps_abs sqrt(n), the rho estimate against both move thresholds of the current rung.
The warm-start list is picked the same way for two solves in a row with warm_starting=True, both of which must qualify.
"""
import argparse
import os
import sys

import numpy as np

R0 = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R0, os.path.join(R0, "reluqp-py_amd")):
    sys.path.insert(0, p)
from oracle import reluqp_oracle as O          # noqa: E402
from reluqp import utils                       # noqa: E402

SHAPES = [(32, 64), (9, 17), (56, 128), (33, 65), (80, 320), (57, 129), (104, 320), (100, 300), (81, 129)]
WARM_SHAPE = (100, 300)


def margins_ok(q, n, m, margin):
    st = q.settings
    thr_p, thr_d = st.eps_abs * np.sqrt(m), st.eps_abs * np.sqrt(n)
    tol, nrho = st.adaptive_rho_tolerance, len(q.rhos)
    for pri, dua, rho, ri in q.trace:
        if abs(pri / thr_p - 1.0) < margin or abs(dua / thr_d - 1.0) < margin:
            return False
        if ri < nrho - 1 and abs(rho / (q.rhos[ri] * tol) - 1.0) < margin:
            return False
        if ri > 0 and abs(rho / (q.rhos[ri] / tol) - 1.0) < margin:
            return False
    return True


def pick(n, m, solves, a):
    good = []
    for seed in range(a.first):
        n_eq = m // 12
        H, g, A, l, u, _ = utils.rand_qp(n, n_eq, m - n_eq, seed=seed, compute_sol=False, feasible=True)
        q = O.OracleQP(form="refine")
        q.setup(H, g, A, l, u, dtype=np.float32, warm_starting=solves > 1)
        ok, its = True, []
        for _ in range(solves):
            r = q.solve()
            ok = ok and str(r.info.status) == "solved" and margins_ok(q, n, m, a.margin)
            its.append(int(r.info.iter))
        if ok:
            good.append((seed, its))
        if len(good) == a.count:
            break
    return good


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--count", type=int, default=6)
    ap.add_argument("--first", type=int, default=200)
    ap.add_argument("--margin", type=float, default=0.12)
    a = ap.parse_args()
    for n, m in SHAPES:
        good = pick(n, m, 1, a)
        print("(%d, %d): %s   # iterations %s" % (n, m, tuple(s for s, _ in good), [i[0] for _, i in good]), flush=True)
    good = pick(*WARM_SHAPE, 2, a)
    print("warm %s: %s   # iterations (cold, warm) %s" % (WARM_SHAPE, tuple(s for s, _ in good), [tuple(i) for _, i in good]))


if __name__ == "__main__":
    main()
