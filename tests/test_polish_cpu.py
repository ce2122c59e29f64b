"""CPU checks of solution polishing (include/rqp_abi.h: rqp_set_polish / rqp_get_polish; ReLU_QP.setup(polish=True)):
the boundary declares and exports both entry points, the host-only argument checks hold, the Python surface has OSQP's
names and defaults, and the numpy restatement of the rule (tests/polish_ref.py) recovers the planted optimum from the
oracle's ADMM iterate -- the specification the GPU kernels are tested against (tests/test_polish_gpu.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle import reluqp_oracle as O
from reluqp import _cabi, utils
from reluqp.classes import Settings

import polish_ref as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_polish_symbols_declared_exported_listed():
    src = open(os.path.join(REPO, "include", "rqp_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+rqp_set_polish\s*\(\s*rqp_handle\s*\*\s*h\s*,\s*int32_t\s+enable\s*,\s*double\s+delta\s*,"
                     r"\s*int32_t\s+refine_iter\s*\)", src)
    assert re.search(r"int\s+rqp_get_polish\s*\(\s*rqp_handle\s*\*\s*h\s*,\s*int32_t\s*\*\s*status_polish\s*,"
                     r"\s*int8_t\s*\*\s*active\s*,\s*void\s*\*\s*stream\s*\)", src)
    lib = _cabi.load()
    for name in ("rqp_set_polish", "rqp_get_polish"):
        assert name in _cabi.ABI_SYMBOLS
        assert hasattr(lib, name)


def test_null_handle_and_bad_arguments():
    lib = _cabi.load()
    assert lib.rqp_set_polish(None, 1, 1e-6, 3) == _cabi.RQP_ERR_ARG
    assert lib.rqp_set_polish(None, 0, 1e-6, 3) == _cabi.RQP_ERR_ARG
    assert lib.rqp_get_polish(None, None, None, None) == _cabi.RQP_ERR_ARG


def test_setup_signature_and_settings_defaults():
    from reluqp.reluqpth import ReLU_QP
    sig = inspect.signature(ReLU_QP.setup).parameters
    assert sig["polish"].default is False
    assert sig["delta"].default == 1e-6
    assert sig["polish_refine_iter"].default == 3
    s = Settings(device="cpu")
    assert (s.polish, s.delta, s.polish_refine_iter) == (False, 1e-6, 3)


def test_numpy_rule_recovers_planted_optimum_from_the_oracle_iterate():
    """Planted problems (feasible=True: x_sol is the optimum) solved by the oracle at eps_abs 1e-3; polishing its final
    iterate lands on x_sol to 1e-9, and the polished point is accepted by OSQP's rule."""
    B, n, n_eq, n_ineq = 6, 10, 5, 15
    H, g, A, l, u, xs = utils.rand_qp_batch(B, n, n_eq, n_ineq, seed0=3, feasible=True)
    ref = O.solve_batch(H, g, A, l, u, form="factored")
    assert all(s == "solved" for s in ref["status"])
    for b in range(B):
        act = P.classify(ref["z"][b], ref["lam"][b], l[b], u[b])
        assert (act[:n_eq] != 0).all()                                   # equality rows are always active
        x, z, y = P.polish(H[b], g[b], A[b], l[b], u[b], act)
        assert np.abs(x - xs[b]).max() <= 1e-9 * (1 + np.abs(xs[b]).max())
        xe, _, _ = P.kkt_exact(H[b], g[b], A[b], l[b], u[b], act)
        assert np.abs(x - xe).max() <= 1e-9 * (1 + np.abs(xe).max())
        pri, dua, _ = P.residuals(H[b], g[b], A[b], x, z, y)
        assert pri < 1e-9
        if int((act != 0).sum()) <= n:       # (more active rows than variables: x is unique, the multipliers are not -- the
            assert dua < 1e-9                #  regularised solve picks small ones whose signs the projection may clip)
            assert P.accept(pri, dua, ref["pri_res"][b], ref["dua_res"][b])


def test_numpy_rule_rejects_a_wrong_active_set():
    """A wrong guess shows up in the residuals: with the projection onto the sign cone, a row wrongly marked active gets a
    multiplier of the wrong sign clipped to 0, and the dual residual grows."""
    n, n_eq, n_ineq = 10, 5, 15
    H, g, A, l, u, xs = utils.rand_qp_batch(1, n, n_eq, n_ineq, seed0=11, feasible=True)
    H, g, A, l, u = H[0], g[0], A[0], l[0], u[0]
    ref = O.solve_batch(H[None], g[None], A[None], l[None], u[None], form="factored")
    act = P.classify(ref["z"][0], ref["lam"][0], l, u)
    inactive = np.nonzero(act == 0)[0]
    assert len(inactive)
    bad = act.copy()
    bad[inactive[0]] = -1                                                 # force an inactive row onto its lower bound
    x, z, y = P.polish(H, g, A, l, u, bad)
    pri, dua, _ = P.residuals(H, g, A, x, z, y)
    assert not P.accept(pri, dua, 1e-6, 1e-6)
