"""Shapes and planted problems of the reduced-KKT edge tests (tests/test_kkt_edges_cpu.py, tests/test_kkt_edges_gpu.py): one
batch of per-instance matrices for every dispatch class of the float64 chain behind rqp_adjoint and rqp_sensitivity (pack ->
rqp_launch_gram_masked -> rqp_launch_factor with k_f64 = 1 -> k_adjoint / k_sens_solve), a shared-matrix batch whose n and m
are no multiples of 16, and the planted batch of the chunked test.  Everything is a pure function of the constants below."""
import numpy as np

import adjoint_ref as R

NDIR = 17                                  # one full block of 16 directions and a tail of one

# (n, n_eq, n_ineq, B), n_active per instance: what the shape reaches.  ldn = n rounded up to 4; m = n_eq + n_ineq; m_a = n_eq +
# n_active[b] is the active count (the k += 4 and 16-row tails of mul_rows / mul_cols).  In every batch instance 0 has only
# its equality rows active, instance 1 sits at the cap min(n // 2 - n_eq, n_ineq), the others have an m_a that is no
# multiple of 4.
SHAPES = [
    # gram n <= 32; k_factor_reg2 n <= 32; pcolmv 64 wide (S = 4); one 16-tile with n % 4 = 3, ldn = 8, m < 16; m_a = 2, 3
    ((7, 2, 9, 5), (0, 1, 1, 0, 1)),
    # gram n <= 32; k_factor_reg2 n <= 32; pcolmv 64 wide; instance 0 has an EMPTY active set (m_a = 0: mul_cols / mul_rows
    # run no tile); m_a = 10, 3, 7
    ((20, 0, 30, 4), (0, 10, 3, 7)),
    # gram n <= 64; k_factor_reg2 n <= 64 (first size past the 32 class); pcolmv 64 wide; ldn = 36; m_a = 5, 16, 6, 7, 10, 13
    ((33, 5, 60, 6), (0, 11, 1, 2, 5, 8)),
    # gram n <= 112; k_factor_reg2 n <= 112 (first size past the 64 class); pcolmv 128 wide (S = 2); ldn = 68; m_a = 8, 33, 13, 21
    ((66, 8, 70, 4), (0, 25, 5, 13)),
    # gram n <= 112 && ldn <= 112 (last: ldn = 112); k_factor_reg2 n <= 112 (last); pcolmv 128 wide; m_a = 12, 55, 19, 34
    ((111, 12, 130, 4), (0, 43, 7, 22)),
    # generic k_gram (ldn = 116 > 112); k_factor_fast 113..128; pcolmv 128 wide; m_a = 10, 57, 23
    ((114, 10, 120, 3), (0, 47, 13)),
    # generic k_gram; k_factor_fast with ldn = 128; pcolmv 128 wide; m_a = 10, 63, 27
    ((126, 10, 100, 3), (0, 53, 17)),
    # generic k_gram; LDS-mode k_factor 129..141; pcolmv 192 wide (S = 1, a quarter of the workgroup idle); m = 280 > 256:
    # second trip of k_sens_classify's prefix sum with active rows past row 256; m_a = 10, 65, 33
    ((130, 10, 270, 3), (0, 55, 23)),
    # generic k_gram; LDS-mode k_factor, its last size ((n^2 + 2 n) * 8 <= 160 KB - 512 holds up to n = 141, not 142);
    # pcolmv 192 wide; every inequality row active on instance 1; m_a = 10, 70
    ((141, 10, 60, 2), (0, 60)),
    # generic k_gram; k_factor_blk 142..320, its first size (20448 doubles of LDS would be 32 over the limit); pcolmv 192 wide;
    # m_a = 10, 70
    ((142, 10, 60, 2), (0, 60)),
    # generic k_gram; k_factor_blk with n % 16 = 2 (a ragged last pivot block); pcolmv 192 wide; m_a = 10, 70
    ((146, 10, 60, 2), (0, 60)),
    # generic k_gram; k_factor_blk; pcolmv 256 wide; m = 320 > 256 with active rows past row 256; m_a = 20, 100, 57
    ((200, 20, 300, 3), (0, 80, 37)),
    # generic k_gram; k_factor_blk; pcolmv 256 wide with a second cb trip (n > 256); k_adj_outer's walk with dr = 0; m_a = 10, 50
    ((260, 10, 40, 2), (0, 40)),
    # generic k_gram; global-slab k_factor (n > 320) with fscratch aliased onto G_a; pcolmv second cb trip; k_adj_outer dr = 0;
    # n16 = 336 rows of X, V, T in k_sens_solve's LDS; m_a = 8, 38
    ((324, 8, 30, 2), (0, 30)),
]
PAST_256 = {(130, 10, 270, 3), (200, 20, 300, 3)}      # batches that must hold an active row of index >= 256

SHARED = (37, 4, 97)                       # (n, n_eq, n_ineq) of the shared-matrix batch: m = 101, neither a multiple of 16
SHARED_B = (1, 5, 17, 67)                  # k_adj_gemm: one wave holds everything; waves 2, 3 empty; a wave of one row; ragged 16-group

CHUNK = (320, 4, 20, 660)                  # one 1 GiB chunk of float64 n x n matrices holds 655 at n = 320: a second chunk of five
CHUNK_UNSOLVED = (3, 657)
CHUNK_REF = (0, 1, 2, 4, 654, 655, 656, 658, 659)   # compared with the numpy references ({0, 1, 654, 655, 656, 659} and the
                                                    # neighbours 2, 4, 656, 658 of the instances that were not solved)


def shape_id(shape):
    return "n%d_eq%d_in%d_B%d" % shape


def seed_of(shape):
    return 1000 + shape[0]


def per_instance(shape, n_active):
    """The planted batch of one row of SHAPES (adjoint_ref.margin_qp_batch's dict)."""
    n, n_eq, n_ineq, B = shape
    d = R.margin_qp_batch(B, n, n_eq, n_ineq, seed=seed_of(shape), n_active=n_active)
    nact = (d["active"] != 0).sum(1)
    assert (nact == n_eq + np.asarray(n_active)).all()
    if shape in PAST_256:
        assert (d["active"][:, 256:] != 0).any()
    return d


def round32(d):
    """The data as a float32 handle sees it (the references are evaluated on it)."""
    return {k: (v if k == "active" else v.astype(np.float32).astype(np.float64)) for k, v in d.items()}


def cotangents(shape, seed=0):
    """dx [B, n], dy [B, m] of the adjoint."""
    n, n_eq, n_ineq, B = shape
    rs = np.random.RandomState(seed)
    return rs.randn(B, n), rs.randn(B, n_eq + n_ineq)


def tangents(B, n, m, ndir, seed, shared_mats=False):
    """All five tangents, per instance (dH, dA shared when the matrices are), direction axis last."""
    rs = np.random.RandomState(seed)
    mat = () if shared_mats else (B,)
    return dict(dH=rs.randn(*(mat + (n, n, ndir))), dg=rs.randn(B, n, ndir), dA=rs.randn(*(mat + (m, n, ndir))),
                dl=rs.randn(B, m, ndir), du=rs.randn(B, m, ndir))


def duality_gap(d, gx, gy, v, ndir):
    """max over the directions of |<gx, dx_jvp> + <gy, dy_jvp> - sum_k <grad_k, tangent_k>| / max(1, |lhs|) between
    adjoint_ref.adjoint_batch and sensitivity_ref.jvp_batch (matrix tangents per instance or shared, as the matrices)."""
    import sensitivity_ref as S
    dx, dy, _ = S.jvp_batch(d["H"], d["A"], d["x"], d["y"], d["active"], ndir, **v)
    gr = R.adjoint_batch(d["H"], d["A"], d["x"], d["y"], d["active"], gx, gy)
    worst = 0.0
    for j in range(ndir):
        lhs = np.sum(gx * dx[..., j]) + np.sum(gy * dy[..., j])
        rhs = sum(np.sum(gr[k] * v[k][..., j]) for k in ("dH", "dg", "dA", "dl", "du"))
        worst = max(worst, abs(lhs - rhs) / max(1.0, abs(lhs)))
    return worst
