"""Linear-MPC problem generators and a closed-loop driver.

The reference ships these as ``loose_code/RandomLinMPC.py``: ``ihlqr`` works (``:6-15``) but
``gen_sparse_mpc_qp`` (``:54-66``) and ``gen_condensed_mpc_qp`` (``:76-90``) raise ``ValueError``
as written (mistranslated block-diagonal at ``:56``, ``-eye(nu)`` for ``-I_nx`` at ``:58``, 3 of 5
return values unpacked at ``:80``) and there is no driver.  This module implements their documented
INTENT with the same function names, argument order and return tuples; since the reference code does
not run, parity is pinned by construction properties instead (tests/test_mpc_cpu.py): the Riccati
fixed point, dynamics feasibility of the sparse form, and sparse == condensed optima.

Variable order of the sparse form (``:54`` intent): y = [u_0, x_1, u_1, x_2, ..., u_{N-1}, x_N].
Condensed form: y = F v + G x0 with pre-stabilising feedback u_k = -K x_k + v_k, so that
H = F'H_sp F, g = (F'H_sp G) x0, A = A_add F, l/u = l_add/u_add - (A_add G) x0 -- per step only
(g, l, u) change: exactly the ``update(g, l, u)`` + warm-started ``solve()`` path of the solver
(reluqpth.py:159-183), with H and A shared by every instance of a batch.
"""
from copy import deepcopy

import numpy as np


def ihlqr(A, B, Q, R, Qf, max_iters=1000, tol=1e-8):
    """Infinite-horizon LQR by Riccati fixed-point iteration; returns (K, P).
    Same recursion and stopping rule as RandomLinMPC.py:6-15."""
    P = Qf
    K = np.zeros((B.shape[1], A.shape[0]))
    for _ in range(max_iters):
        P_prev = deepcopy(P)
        K = np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)
        P = Q + A.T @ P @ (A - B @ K)
        if np.linalg.norm(P - P_prev, 2) < tol:
            return K, P
    raise Exception("ihlqr didn't converge")


def _blkdiag(blocks):
    n = sum(b.shape[0] for b in blocks)
    out = np.zeros((n, n))
    i = 0
    for b in blocks:
        k = b.shape[0]
        out[i:i + k, i:i + k] = b
        i += k
    return out


def gen_sparse_mpc_qp(Ad, Bd, Q, R, Qf, horizon, A_add=None, l_add=None, u_add=None):
    """Sparse-form MPC QP (intent of RandomLinMPC.py:54-66).  Returns (H, g, A, l, u) for x0 = 0;
    the x0-dependence is l[:nx] = u[:nx] = -Ad x0 (first dynamics block)."""
    nx, nu = Ad.shape[0], Bd.shape[1]
    N = horizon
    H = _blkdiag([R, Q] * (N - 1) + [R, Qf])
    g = np.zeros(H.shape[0])
    # dynamics rows k: B u_k - x_{k+1} + A x_k = 0
    A = np.kron(np.eye(N), np.hstack([Bd, -np.eye(nx)]))
    if N > 1:
        A[nx:, nu:nu + (N - 1) * (nx + nu)] += np.kron(np.eye(N - 1), np.hstack([Ad, np.zeros((nx, nu))]))
    l = np.zeros(A.shape[0])
    u = np.zeros(A.shape[0])
    if A_add is not None:
        A = np.vstack([A, A_add])
        l = np.hstack([l, l_add])
        u = np.hstack([u, u_add])
    return H, g, A, l, u


def sparse_x0_update(Ad, nx, l, u, x0):
    """(l, u) of the sparse form for an initial state x0 (batched x0 [B, nx] -> [B, m])."""
    x0 = np.atleast_2d(x0)
    lb = np.repeat(l[None], x0.shape[0], 0)
    ub = np.repeat(u[None], x0.shape[0], 0)
    lb[:, :nx] = ub[:, :nx] = -(x0 @ Ad.T)
    return lb, ub


def gen_condensed_mpc_qp(Ad, Bd, Q, R, Qf, horizon, A_add, l_add, u_add, K=None):
    """Condensed MPC QP (intent of RandomLinMPC.py:76-90): states eliminated through
    y = F v + G x0 with u_k = -K x_k + v_k.  Returns (H, g, A, l, u, g_x0, lu_x0) with
    g = g_x0 @ x0, l = l_add + lu_x0 @ x0, u = u_add + lu_x0 @ x0 (returned for x0 = 0)."""
    nx, nu = Ad.shape[0], Bd.shape[1]
    N = horizon
    if K is None:
        K = np.zeros((nu, nx))
    H_sp, g_sp, _, _, _ = gen_sparse_mpc_qp(Ad, Bd, Q, R, Qf, N)
    Acl = Ad - Bd @ K
    pw = [np.eye(nx)]
    for _ in range(N):
        pw.append(Acl @ pw[-1])
    blk = nu + nx
    F = np.zeros((N * blk, N * nu))
    G = np.zeros((N * blk, nx))
    for k in range(N):
        G[k * blk:k * blk + nu] = -K @ pw[k]
        G[k * blk + nu:(k + 1) * blk] = pw[k + 1]
        F[k * blk:k * blk + nu, k * nu:(k + 1) * nu] = np.eye(nu)
        F[k * blk + nu:(k + 1) * blk, k * nu:(k + 1) * nu] = Bd
        for j in range(k):
            F[k * blk:k * blk + nu, j * nu:(j + 1) * nu] = -K @ pw[k - 1 - j] @ Bd
            F[k * blk + nu:(k + 1) * blk, j * nu:(j + 1) * nu] = pw[k - j] @ Bd
    H = F.T @ H_sp @ F
    H = 0.5 * (H + H.T)
    g_x0 = F.T @ H_sp @ G
    g = g_x0 @ np.zeros(nx) + F.T @ g_sp
    A = A_add @ F
    lu_x0 = -A_add @ G
    return H, g, A, l_add, u_add, g_x0, lu_x0


def condensed_x0_update(g_x0, lu_x0, l_add, u_add, x0):
    """(g, l, u) of the condensed form for (a batch of) initial states x0 [B, nx]."""
    x0 = np.atleast_2d(x0)
    shift = x0 @ lu_x0.T
    return x0 @ g_x0.T, l_add[None] + shift, u_add[None] + shift


def random_plant(nx=12, nu=4, seed=0, dt=0.1):
    """Random controllable, marginally stable discrete plant:
    Ad = I + dt*S with S = (W - W')/2 - 0.05 W W'/nx (lightly damped rotation), rescaled to spectral
    radius <= 0.999 so that box-constrained MPC problems stay feasible; Bd = dt*randn."""
    rs = np.random.RandomState(seed)
    W = rs.randn(nx, nx)
    S = 0.5 * (W - W.T) - 0.05 * (W @ W.T) / nx
    Ad = np.eye(nx) + dt * S
    rad = np.max(np.abs(np.linalg.eigvals(Ad)))
    Ad = Ad / max(1.0, rad / 0.999)
    Bd = dt * rs.randn(nx, nu)
    return Ad, Bd


def box_constraints(nx, nu, horizon, u_max, x_max):
    """A_add = I on y = [u_0, x_1, ...]: |u| <= u_max, |x| <= x_max."""
    blk = nu + nx
    A_add = np.eye(horizon * blk)
    hi = np.tile(np.hstack([np.full(nu, u_max), np.full(nx, x_max)]), horizon)
    return A_add, -hi, hi


class LinearMPC(object):
    """Closed-loop linear MPC on a batch of independent plants/initial states sharing (H, A).

    setup: one ``ReLU_QP.setup`` with un-batched (shared) H, A and batched (g, l, u);
    step(x): ``update(g, l, u)`` from the current states, warm-started ``solve()``, returns the
    first input of every instance (the path of reluqpth.py:159-183 + :201-249 per control step)."""

    def __init__(self, Ad, Bd, Q, R, horizon, u_max, x_max, form="condensed", solver=None, **solver_kw):
        self.Ad, self.Bd, self.horizon, self.form = Ad, Bd, horizon, form
        self.nx, self.nu = Ad.shape[0], Bd.shape[1]
        self.K, self.P = ihlqr(Ad, Bd, Q, R, Q)
        A_add, l_add, u_add = box_constraints(self.nx, self.nu, horizon, u_max, x_max)
        self.l_add, self.u_add = l_add, u_add
        if form == "condensed":
            (self.H, _, self.A, _, _, self.g_x0, self.lu_x0) = gen_condensed_mpc_qp(
                Ad, Bd, Q, R, self.P, horizon, A_add, l_add, u_add, K=self.K)
        else:
            self.H, _, self.A, self.l0, self.u0 = gen_sparse_mpc_qp(Ad, Bd, Q, R, self.P, horizon, A_add, l_add, u_add)
        self.solver = solver
        self.solver_kw = solver_kw
        self._ready = False

    def qp_vectors(self, x):
        """(g, l, u) [B, .] of the QPs for the current states x [B, nx]."""
        x = np.atleast_2d(x)
        if self.form == "condensed":
            return condensed_x0_update(self.g_x0, self.lu_x0, self.l_add, self.u_add, x)
        lb, ub = sparse_x0_update(self.Ad, self.nx, self.l0, self.u0, x)
        return np.zeros((x.shape[0], self.H.shape[0])), lb, ub

    def first_input(self, sol, x):
        """u_0 of every instance from the QP solution (condensed: u_0 = -K x_0 + v_0)."""
        x = np.atleast_2d(x)
        if self.form == "condensed":
            return sol[:, :self.nu] - x @ self.K.T
        return sol[:, :self.nu]

    def step(self, x):
        g, l, u = self.qp_vectors(x)
        if not self._ready:
            import reluqp.reluqpth as reluqpth
            self.solver = self.solver or reluqpth.ReLU_QP()
            self.solver.setup(self.H, g, self.A, l, u, **self.solver_kw)
            self._ready = True
        else:
            self.solver.update(g=g, l=l, u=u)
        res = self.solver.solve()
        sol = res.x
        if hasattr(sol, "detach"):
            sol = sol.detach().cpu().double().numpy()
        sol = np.asarray(sol, dtype=np.float64)
        if sol.ndim == 1:
            sol = sol[None]
        return self.first_input(sol, x), res

    def _device_maps(self, device, dtype):
        """Constant maps of the closed loop on the device.  With u0 = v0 - K x the plant step is
        x+ = Ad x + Bd u0 = (Ad - Bd K) x + Bd v0: two GEMMs per step (Acl' and Bd' are what they multiply from the right)."""
        import torch
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device, dtype=dtype)
        if self.form == "sparse":
            # the reference's own form (RandomLinMPC.py:54-66): g does not depend on x0; l = u = -Ad x0 on the first dynamics
            # block; the first input is the first nu variables, the plant step x+ = Ad x + Bd u0
            n, m = self.H.shape[0], self.A.shape[0]
            lumap = np.zeros((m, self.nx))
            lumap[:self.nx] = -self.Ad
            return dict(gmap=t(np.zeros((n, self.nx))), lumap=t(lumap), ladd=t(self.l0), uadd=t(self.u0),
                        Aclt=t(self.Ad.T), Bdt=t(self.Bd.T))
        return dict(gmap=t(self.g_x0), lumap=t(self.lu_x0), ladd=t(self.l_add), uadd=t(self.u_add),
                    Aclt=t((self.Ad - self.Bd @ self.K).T), Bdt=t(self.Bd.T))

    def feedback_gain(self, x):
        """Local feedback gain d u0* / d x0 of the handle's last solve: a device tensor [B, nu, nx], and the per-instance
        status of the sensitivities (1 computed, 0: that solve did not succeed, its gain is then the condensed form's -K or 0).
        ``x`` [B, nx] are the states that solve was for.  The solver must be set up with ``sensitivity=True`` (solver_kw).
        One rqp_sensitivity call with ndir = nx: the device maps of the closed loop are the shared tangents (dg = gmap,
        dl = du = lumap); l and u are rebuilt from x, so this also follows simulate_device / update_affine.  Every equality
        row (l == u: the sparse form's dynamics) is active, also where its multiplier rounds to zero.  The condensed form's
        input is u0 = v0 - K x0: its gain is d v0 / d x0 - K."""
        import torch
        s = self.solver
        if s is None or not self._ready:
            raise RuntimeError("feedback_gain: solve first (step / simulate_device)")
        st, res = s.settings, s.results
        mp = self._device_maps(st.device, st.precision)
        x = torch.as_tensor(np.atleast_2d(x) if not torch.is_tensor(x) else x, device=st.device, dtype=st.precision)
        shift = x @ mp["lumap"].T
        l, u = mp["ladd"] + shift, mp["uadd"] + shift
        # the adjoint's classification in the caller's units, equality rows forced active (side: the sign of y)
        z, y = res.z, res.y
        act = torch.where(z - l < -y, -1, torch.where(u - z < y, 1, 0))
        act = torch.where(l == u, torch.where(y > 0, 1, -1), act).to(torch.int8)
        dx, _, _, status, _, _ = s._sens_call(s.QP.H, s.QP.A, l, u, res.x, z, y,
                                              dict(dg=(mp["gmap"], True), dl=(mp["lumap"], True), du=(mp["lumap"], True)),
                                              self.nx, status=res.info.status_code, active=act, want_dz=False)
        gain = dx[:, :self.nu, :]
        if self.form == "condensed":
            gain = gain - torch.as_tensor(self.K, device=st.device, dtype=st.precision)
        return gain, status

    def simulate_device(self, x0, steps, device, dtype):
        """Closed loop with every per-step map on the device (no host round trip per control step):
        g = G x, l/u = l_add/u_add + LU x (rqp_update_affine), warm solve, x+ = (Ad - Bd K) x + Bd v0 with v0 the first
        input block of the solution.  torch is used here for the caller-side plant step only; the QP path is the HIP library.
        Returns (final states [B, nx] tensor, mean ADMM iterations per solve)."""
        import torch
        mp = self._device_maps(device, dtype)
        x = torch.as_tensor(np.atleast_2d(x0), device=device, dtype=dtype)
        it_acc = None
        for k in range(steps):
            fresh = False
            if not self._ready:
                shift = x @ mp["lumap"].T
                g, l, u = x @ mp["gmap"].T, mp["ladd"] + shift, mp["uadd"] + shift
                import reluqp.reluqpth as reluqpth
                self.solver = self.solver or reluqpth.ReLU_QP()
                self.solver.setup(self.H, g, self.A, l, u, **self.solver_kw)
                self._ready = True
                fresh = True                         # setup() already holds this step's vectors
            sync = self.solver.synchronous
            self.solver.synchronous = False          # enqueue only: the steps chain on the stream, no host wait per step
            try:
                if not fresh:                        # g = G x, l/u = l_add/u_add + LU x in one device pass
                    self.solver.update_affine(x, mp["gmap"], mp["lumap"], mp["ladd"], mp["uadd"])
                res = self.solver.solve()
            finally:
                self.solver.synchronous = sync
            x = torch.addmm(x @ mp["Aclt"], res.x[:, :self.nu], mp["Bdt"])
            it_acc = res.info.iter.clone() if it_acc is None else it_acc.add_(res.info.iter)
        return x, float(it_acc.sum()) / (steps * x.shape[0])

    def simulate_graph(self, x0, steps, device, dtype):
        """simulate_device with the control step (x0 update, warm-started solve, plant step) captured ONCE in a HIP graph
        and replayed ``steps`` times: no host work per step at all (launch-bound small batches gain the most).
        The solver must be set up (run simulate_device for one step first).  Returns as simulate_device."""
        import torch
        assert self._ready
        mp = self._device_maps(device, dtype)
        x = torch.as_tensor(np.atleast_2d(x0), device=device, dtype=dtype).clone()   # static buffer: rewritten in place
        it_acc = torch.zeros(x.shape[0], device=device, dtype=torch.int32)
        sync = self.solver.synchronous
        self.solver.synchronous = False
        try:
            def step():
                self.solver.update_affine(x, mp["gmap"], mp["lumap"], mp["ladd"], mp["uadd"])
                res = self.solver.solve()
                x.copy_(torch.addmm(x @ mp["Aclt"], res.x[:, :self.nu], mp["Bdt"]))
                it_acc.add_(res.info.iter)
            side = torch.cuda.Stream(device=device)           # warm-up on a side stream, as torch's capture rules ask
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream(device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            # thread-local capture error mode: frees / allocations on OTHER threads cannot invalidate the capture; on this
            # thread rqp_destroy (a finaliser, an explicit del) frees its workspace under the relaxed capture mode
            # (csrc/rqp_abi.hip: free_ws), so destroying a solver mid-capture is safe too (tests/test_mpc_gpu.py)
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                step()
            done = 1                                          # the warm-up ran one step (capturing only records)
            for _ in range(max(0, steps - done)):
                graph.replay()
        finally:
            self.solver.synchronous = sync
        torch.cuda.synchronize(device)
        return x, float(it_acc.sum()) / (max(steps, done) * x.shape[0])

    def simulate(self, x0, steps, noise=0.0, seed=0):
        """Closed loop x+ = Ad x + Bd u (+ noise); returns (states [steps+1, B, nx], inputs, iteration counts)."""
        rs = np.random.RandomState(seed)
        x = np.atleast_2d(np.array(x0, dtype=np.float64))
        xs, us, its = [x.copy()], [], []
        for _ in range(steps):
            u0, res = self.step(x)
            x = x @ self.Ad.T + u0 @ self.Bd.T + noise * rs.randn(*x.shape)
            xs.append(x.copy())
            us.append(u0)
            it = res.info.iter
            its.append(it.cpu().numpy() if hasattr(it, "cpu") else np.atleast_1d(np.asarray(it)))
        return np.stack(xs), np.stack(us), np.stack(its)


# ----------------------------------------------------------------------------------------------------------------------
# Linear time-varying (LTV) plants, one linearisation per instance: x_{k+1} = A_k x_k + B_k u_k + c_k, u_k = -K x_k + v_k.
# y = [u_0, x_1, ..., u_{N-1}, x_N] = F v + G x0 + f;  H = sym(F'H_sp F), A = F (box constraints: A_add = I),
# g = F'H_sp (G x0 + f - yref), l / u = l_add / u_add - (G x0 + f), first input u_0 = v_0 - K x0.
# condense_ltv is the host statement of these formulas (dense F, G, then F.T @ H_sp @ F); condense_ltv_device /
# ltv_vectors_device run them on the device (C-ABI rqp_ltv_condense / rqp_ltv_vectors) straight into the tensors
# setup() / update() read, and BatchedLTVMPC is the closed-loop driver on top.

LTV_LIMITS = dict(nx=16, nu=8, horizon=32, n=160, m=640)     # what the device kernels hold (rqp_abi.h)


def _ltv_shapes(Ad, Bd):
    if Ad.ndim != 4 or Bd.ndim != 4:
        raise ValueError("Ad must be [B, N, nx, nx] and Bd [B, N, nx, nu], got %s and %s" % (tuple(Ad.shape), tuple(Bd.shape)))
    B, N, nx, nu = Ad.shape[0], Ad.shape[1], Ad.shape[2], Bd.shape[3]
    if tuple(Ad.shape) != (B, N, nx, nx) or tuple(Bd.shape) != (B, N, nx, nu):
        raise ValueError("Ad must be [B, N, nx, nx] and Bd [B, N, nx, nu], got %s and %s" % (tuple(Ad.shape), tuple(Bd.shape)))
    return B, N, nx, nu


def _ltv_check_sizes(nx, nu, N):
    L = LTV_LIMITS
    if nx < 1 or nu < 1 or N < 1:
        raise ValueError("nx, nu and horizon must be >= 1")
    if nx > L["nx"] or nu > L["nu"] or N > L["horizon"] or N * nu > L["n"] or N * (nx + nu) > L["m"]:
        raise ValueError("unsupported LTV size (nx=%d, nu=%d, horizon=%d): the device condensing holds nx <= %d, nu <= %d, "
                         "horizon <= %d, n = horizon nu <= %d, m = horizon (nx + nu) <= %d"
                         % (nx, nu, N, L["nx"], L["nu"], L["horizon"], L["n"], L["m"]))


def _ltv_weights(nx, nu, Q, R, Qf, K):
    Q, R, Qf = (np.asarray(a, dtype=np.float64) for a in (Q, R, Qf))
    if Q.shape != (nx, nx) or Qf.shape != (nx, nx) or R.shape != (nu, nu):
        raise ValueError("Q, Qf must be [%d, %d] and R [%d, %d]" % (nx, nx, nu, nu))
    for name, W in (("Q", Q), ("R", R), ("Qf", Qf)):                # symmetric up to rounding (a Riccati P is): the symmetric part is used
        if np.abs(W - W.T).max() > 1e-9 * max(np.abs(W).max(), 1e-300):
            raise ValueError("%s must be symmetric" % name)
    Q, R, Qf = (0.5 * (W + W.T) for W in (Q, R, Qf))
    if K is not None:
        K = np.asarray(K, dtype=np.float64)
        if K.shape != (nu, nx):
            raise ValueError("K has shape %s, expected (%d, %d)" % (K.shape, nu, nx))
    return Q, R, Qf, K


# Stage weights: instead of one (Q, R, Qf), R_k weighs u_k and Q_k weighs x_{k+1} (so Q_{N-1} is the terminal weight),
# H_sp = blkdiag(R_0, Q_0, ..., R_{N-1}, Q_{N-1}), per stage ([N, ., .]) or per instance and stage ([B, N, ., .]).  One of Q, R
# may stay shared ([., .]): it is repeated, a shared Q as Q, ..., Q, Qf.  A staged Q has no Qf.

def _ltv_staged(Q, R):
    """True when Q or R carries a stage axis (3-D or 4-D); both plain matrices: the shared-weight path."""
    return np.ndim(Q) > 2 or np.ndim(R) > 2


def _ltv_stage_shapes(nx, nu, N, Q, R, Qf, B=None):
    """Shape rules of staged weights (numpy arrays or tensors; nothing is read).  ``B``: the batch of the stages, None for one
    instance (no batch axis allowed).  Returns the batch size the weights themselves name (None: none of them has a batch axis)."""
    batch = None
    for name, W, d in (("Q", Q, nx), ("R", R, nu)):
        shape = tuple(W.shape)
        ok = (shape == (d, d) or shape == (N, d, d) or (len(shape) == 4 and shape[1:] == (N, d, d)))
        if not ok:
            raise ValueError("%s has shape %s, expected %s, %s or %s" % (name, shape, ("B", N, d, d), (N, d, d), (d, d)))
        if len(shape) == 4:
            if B is None:
                raise ValueError("%s has a batch axis %s but the stages have none" % (name, shape))
            if shape[0] != B or (batch is not None and batch != shape[0]):
                raise ValueError("%s is for a batch of %d, the stages for %d" % (name, shape[0], B))
            batch = shape[0]
    if len(Q.shape) > 2:
        if Qf is not None:
            raise ValueError("staged Q has no Qf (Q[..., N-1, :, :] is the terminal weight): Qf must be None")
    elif Qf is None or tuple(Qf.shape) != (nx, nx):
        raise ValueError("a shared Q needs Qf [%d, %d] (it is repeated as Q, ..., Q, Qf)" % (nx, nx))
    return batch


def _ltv_stage_expand(N, Q, R, Qf):
    """numpy: Q, R with a stage axis each ([N, ., .] or [B, N, ., .]); a shared one is repeated (Q as Q, ..., Q, Qf)."""
    if Q.ndim == 2:
        Q = np.stack([Q] * (N - 1) + [np.asarray(Qf).astype(Q.dtype)])
    if R.ndim == 2:
        R = np.stack([R] * N)
    return Q, R


def _rate_difference(N, nx, nu, dt):
    """D [N nu, m]: (D y)_k = u_k - u_{k-1} on y = [u_0, x_1, ..., u_{N-1}, x_N] (block row 0 picks u_0: u_{-1} is not in y)."""
    blk = nu + nx
    D = np.zeros((N * nu, N * blk), dtype=dt)
    for k in range(N):
        D[k * nu:(k + 1) * nu, k * blk:k * blk + nu] = np.eye(nu, dtype=dt)
        if k >= 1:
            D[k * nu:(k + 1) * nu, (k - 1) * blk:(k - 1) * blk + nu] = -np.eye(nu, dtype=dt)
    return D


def _rate_weight_shapes(nu, N, S, B=None):
    shape = tuple(S.shape)
    if not (shape == (nu, nu) or shape == (N, nu, nu) or (len(shape) == 4 and shape[1:] == (N, nu, nu))):
        raise ValueError("S has shape %s, expected %s, %s or %s" % (shape, ("B", N, nu, nu), (N, nu, nu), (nu, nu)))
    if len(shape) == 4 and shape[0] != B:
        raise ValueError("S has a batch axis %s, the stages %s" % (shape, "none" if B is None else "a batch of %d" % B))


def condense_ltv(Ad, Bd, Q, R, Qf=None, K=None, c=None, S=None):
    """Condensed QP maps of LTV plants on the host (numpy, the formulas as written above).

    Ad [N, nx, nx], Bd [N, nx, nu], c [N, nx] (optional) for one instance, or with a leading batch axis.  Returns a dict of
    F [m, n], G [m, nx], f [m], H = sym(F'H_sp F) [n, n], A = F, g_x0 = F'H_sp G [n, nx], g_f = F'H_sp f [n], H_sp [m, m]
    (each with the batch axis when the input has one; H_sp is shared).  Then for an initial state x0 and references:
    g = g_x0 x0 + g_f - F'H_sp yref, l / u = l_add / u_add - (G x0 + f)  (``ltv_vectors``).

    Stage weights: Q [N, nx, nx] and / or R [N, nu, nu], or [B, N, ., .] when the stages have a batch axis; Q_k weighs x_{k+1}, a
    staged Q has no Qf (``Qf=None``, else ValueError); one of Q, R may stay a shared matrix and is repeated (Q as Q, ..., Q,
    Qf).  H_sp then is per instance when a weight is.

    Input rates (section "LTV condensing, input rates"): S [nu, nu], [N, nu, nu] or [B, N, nu, nu] (symmetric blocks) adds
    1/2 sum_k (u_k - u_{k-1})' S_k (u_k - u_{k-1}), u_{-1} = uprev, to the cost.  With D y the stacked differences and
    H_rate = D' blkdiag(S_k) D (both formed densely, both returned): H = sym(F'(H_sp + H_rate) F), g_x0 = F'(H_sp + H_rate) G,
    g_f = F'(H_sp + H_rate) f; H_sp stays the stage cost alone (yref does not enter the rate term), and ``ltv_vectors`` then
    needs ``uprev``."""
    Ad, Bd = np.asarray(Ad), np.asarray(Bd)
    Q, R = np.asarray(Q), np.asarray(R)
    Qf = None if Qf is None else np.asarray(Qf)
    S = None if S is None else np.asarray(S)
    if S is not None:
        _rate_weight_shapes(Bd.shape[-1], Ad.shape[-3], S, B=Ad.shape[0] if Ad.ndim == 4 else None)
    if _ltv_staged(Q, R):
        B, N, nx, nu = (Ad.shape[0] if Ad.ndim == 4 else None,) + tuple(Ad.shape[-3:-1]) + (Bd.shape[-1],)
        _ltv_stage_shapes(nx, nu, N, Q, R, Qf, B=B)
    elif Qf is None:
        raise ValueError("shared weights need Qf")
    if Ad.ndim == 4:
        at = lambda W, b: W[b] if W.ndim == 4 else W
        outs = [condense_ltv(Ad[b], Bd[b], at(Q, b), at(R, b), Qf, K=K, c=None if c is None else np.asarray(c)[b],
                             S=None if S is None else at(S, b)) for b in range(Ad.shape[0])]
        res = {k: np.stack([o[k] for o in outs]) for k in outs[0] if k != "H_sp"}
        res["H_sp"] = np.stack([o["H_sp"] for o in outs]) if Q.ndim == 4 or R.ndim == 4 else outs[0]["H_sp"]
        return res
    dt = np.result_type(Ad.dtype, np.float64)                  # float64, or wider when the caller passes longdouble
    Ad, Bd = Ad.astype(dt), Bd.astype(dt)
    N, nx, nu = Ad.shape[0], Ad.shape[1], Bd.shape[2]
    Q, R = Q.astype(dt), R.astype(dt)
    Qf = None if Qf is None else Qf.astype(dt)
    K = np.zeros((nu, nx), dtype=dt) if K is None else np.asarray(K).astype(dt)
    c = np.zeros((N, nx), dtype=dt) if c is None else np.asarray(c).astype(dt)
    Acl = [Ad[k] - Bd[k] @ K for k in range(N)]

    memo = {}

    def phi(k, j):                                             # Acl_{k-1} ... Acl_j, phi(j, j) = I (each product formed once)
        if k == j:
            return np.eye(nx, dtype=dt)
        if (k, j) not in memo:
            memo[(k, j)] = Acl[k - 1] @ phi(k - 1, j)
        return memo[(k, j)]

    blk = nu + nx
    m, n = N * blk, N * nu
    F, G, f = np.zeros((m, n), dtype=dt), np.zeros((m, nx), dtype=dt), np.zeros(m, dtype=dt)
    xF, xG, xf = np.zeros((N + 1, nx, n), dtype=dt), np.zeros((N + 1, nx, nx), dtype=dt), np.zeros((N + 1, nx), dtype=dt)
    for k in range(N + 1):                                     # x_k = phi(k, 0) x0 + sum_{j<k} phi(k, j+1) (B_j v_j + c_j)
        xG[k] = phi(k, 0)
        for j in range(k):
            P = phi(k, j + 1)
            xF[k][:, j * nu:(j + 1) * nu] = P @ Bd[j]
            xf[k] += P @ c[j]
    for k in range(N):                                         # u_k = -K x_k + v_k
        ru, rx = slice(k * blk, k * blk + nu), slice(k * blk + nu, (k + 1) * blk)
        F[ru] = -K @ xF[k]
        F[ru, k * nu:(k + 1) * nu] += np.eye(nu, dtype=dt)
        G[ru], f[ru] = -K @ xG[k], -K @ xf[k]
        F[rx], G[rx], f[rx] = xF[k + 1], xG[k + 1], xf[k + 1]
    H_sp = np.zeros((m, m), dtype=dt)
    for k in range(N):
        H_sp[k * blk:k * blk + nu, k * blk:k * blk + nu] = R[k] if R.ndim == 3 else R
        H_sp[k * blk + nu:(k + 1) * blk, k * blk + nu:(k + 1) * blk] = Q[k] if Q.ndim == 3 else (Qf if k == N - 1 else Q)
    if S is None:
        H = F.T @ H_sp @ F
        H = (H + H.T) / 2
        return dict(F=F, G=G, f=f, H=H, A=F, g_x0=F.T @ H_sp @ G, g_f=F.T @ H_sp @ f, H_sp=H_sp)
    S = S.astype(dt)
    S = np.stack([S] * N) if S.ndim == 2 else S
    D = _rate_difference(N, nx, nu, dt)
    H_rate = D.T @ _blkdiag_dense(S) @ D
    FtH = F.T @ (H_sp + H_rate)                                # (formed once: the products associate as in the lines above)
    H = FtH @ F
    H = (H + H.T) / 2
    return dict(F=F, G=G, f=f, H=H, A=F, g_x0=FtH @ G, g_f=FtH @ f, H_sp=H_sp, H_rate=H_rate, S=S)


def _blkdiag_dense(blocks):
    """blkdiag of [N, d, d] blocks, written out in the blocks' dtype."""
    N, d = blocks.shape[0], blocks.shape[1]
    M = np.zeros((N * d, N * d), dtype=blocks.dtype)
    for k in range(N):
        M[k * d:(k + 1) * d, k * d:(k + 1) * d] = blocks[k]
    return M


def ltv_vectors(cond, x0, l_add, u_add, xref=None, uref=None, uprev=None):
    """(g, l, u) of the condensed LTV QP from ``condense_ltv``'s maps (one instance: x0 [nx]; batch: x0 [B, nx]).
    Maps condensed with a rate weight S need ``uprev`` [nu] ([B, nu]), the input applied before stage 0:
    g -= F' D' blkdiag(S_k) [uprev; 0; ...] (= S_0 uprev in the first nu entries, F[u_0] = [I 0])."""
    F, G, f = cond["F"], cond["G"], cond["f"]
    x0 = np.asarray(x0, dtype=F.dtype)
    if ("S" in cond) != (uprev is not None):
        raise ValueError("uprev is needed exactly when the maps were condensed with a rate weight S")
    if F.ndim == 3:
        outs = [ltv_vectors({k: (v if k == "H_sp" and v.ndim == 2 else v[b]) for k, v in cond.items()}, x0[b],
                            np.asarray(l_add)[b] if np.ndim(l_add) == 2 else l_add,
                            np.asarray(u_add)[b] if np.ndim(u_add) == 2 else u_add,
                            None if xref is None else xref[b], None if uref is None else uref[b],
                            None if uprev is None else np.asarray(uprev)[b]) for b in range(F.shape[0])]
        return tuple(np.stack([o[i] for o in outs]) for i in range(3))
    m, nx = G.shape
    s = G @ x0 + f
    g = cond["g_x0"] @ x0 + cond["g_f"]
    if uprev is not None:
        Sk = cond["S"]
        N, nu = Sk.shape[0], Sk.shape[1]
        e0 = np.zeros(N * nu, dtype=F.dtype)
        e0[:nu] = np.asarray(uprev).astype(F.dtype)
        g = g - F.T @ (_rate_difference(N, nx, nu, F.dtype).T @ (_blkdiag_dense(Sk) @ e0))
    if xref is not None or uref is not None:
        n = F.shape[1]
        # (N, nu) from the shapes: m = N (nu + nx), n = N nu
        N = (m - n) // nx
        nu = n // N
        yref = np.zeros((N, nu + nx), dtype=F.dtype)
        if uref is not None:
            yref[:, :nu] = uref
        if xref is not None:
            yref[:, nu:] = xref
        g = g - F.T @ (cond["H_sp"] @ yref.reshape(-1))
    return g, np.asarray(l_add, dtype=F.dtype) - s, np.asarray(u_add, dtype=F.dtype) - s


def rate_constraints(cond, x0, uprev, dlo, dhi):
    """(A_r, l_r, u_r) of the slew-rate rows dlo_k <= u_k - u_{k-1} <= dhi_k, u_{-1} = uprev, on the maps of ``condense_ltv``
    (numpy, by the definitions: D formed densely).  With y = F v + s:  A_r = D F,  l_r = dlo - D s + [uprev; 0; ...],
    u_r = dhi - D s + [uprev; 0; ...]  (N nu rows; u_k is the plant's input -K x_k + v_k).  One instance: x0 [nx], uprev [nu],
    dlo, dhi [N nu]; or ``cond`` with a batch axis, x0 [B, nx], uprev [B, nu], dlo / dhi [B, N nu] or shared [N nu]."""
    F, G, f = cond["F"], cond["G"], cond["f"]
    x0, uprev = np.asarray(x0).astype(F.dtype), np.asarray(uprev).astype(F.dtype)
    if F.ndim == 3:
        outs = [rate_constraints({k: v[b] for k, v in cond.items() if k in ("F", "G", "f")}, x0[b], uprev[b],
                                 np.asarray(dlo)[b] if np.ndim(dlo) == 2 else dlo, np.asarray(dhi)[b] if np.ndim(dhi) == 2 else dhi)
                for b in range(F.shape[0])]
        return tuple(np.stack([o[i] for o in outs]) for i in range(3))
    m, nx = G.shape
    n = F.shape[1]
    N = (m - n) // nx
    nu = n // N
    if uprev.shape != (nu,):
        raise ValueError("uprev has shape %s, expected (%d,)" % (uprev.shape, nu))
    dlo, dhi = np.asarray(dlo).astype(F.dtype), np.asarray(dhi).astype(F.dtype)
    if dlo.shape != (n,) or dhi.shape != (n,):
        raise ValueError("dlo, dhi have shapes %s, %s, expected (%d,)" % (dlo.shape, dhi.shape, n))
    D = _rate_difference(N, nx, nu, F.dtype)
    ds = D @ (G @ x0 + f)
    e0 = np.zeros(n, dtype=F.dtype)
    e0[:nu] = uprev
    return D @ F, dlo - ds + e0, dhi - ds + e0


_LTV_VJP_KEYS = ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R", "Qf", "l_add", "u_add", "K")


def condense_ltv_vjp(Ad, Bd, Q, R, Qf=None, x0=None, l_add=None, u_add=None, K=None, c=None, xref=None, uref=None,
                     dH=None, dA=None, dg=None, dl=None, du=None, S=None, uprev=None, dA_r=None, dl_r=None, du_r=None):
    """Reverse of ``condense_ltv`` + ``ltv_vectors`` on the host (numpy): the cotangents dH [n, n], dA [m, n], dg [n],
    dl, du [m] of (H, A, g, l, u) (an absent one is zero) mapped back to the inputs.  One instance, or a leading batch axis
    on Ad, Bd (and on c, x0, xref, uref, the cotangents, and l_add / u_add when they are [B, m]).  Returns a dict with the
    gradients of Ad, Bd, c, x0, xref, uref, l_add, u_add (batched like the inputs; l_add / u_add summed over the batch when
    shared) and of Q, R, Qf, K (summed over the batch; Q, R, Qf symmetric).  K is a reparametrisation -- u_0 = v_0 - K x0 does
    not depend on it in exact arithmetic -- so its entry only states the derivative of the condensing outputs.
    Stage weights (``condense_ltv``): the gradients of Q, R come back in the shape the weights were given -- per stage the
    symmetrised diagonal block of Sb, stacked over the batch for [B, N, ., .], summed over it for [N, ., .] -- and a staged Q has
    no "Qf" entry.

    With S = H_sp, Hs = sym(dH), e = G x0 + f - yref, T = F Hs:
        Fb = dA + 2 S T + (S e) dg',  eb = S F dg,  sb = eb - dl - du,  x0b = G'sb,  yrefb = -eb,  [Gb | fb] = sb [x0' | 1],
        Sb = F T' + (F dg) e' (its diagonal blocks give Rb, Qb, Qfb),
    and the reverse sweep over the stages, Lam = the x_N rows of Yb = [Fb | Gb | fb], X_k = the x_k rows of [F | G | f]:
        k = N-1 .. 0:  Aclb = Lam X_k',  Adb_k = Aclb,  Bdb_k = Lam[:, k nu:(k+1) nu] - Aclb K',  cb_k = Lam[:, f],
                       Lam <- Acl_k' Lam - K' Yb[u_k rows] + Yb[x_k rows]   (k >= 1).

    Input rates (any of ``S``, ``uprev``, ``dA_r``, ``dl_r``, ``du_r`` given): the reverse of ``condense_ltv(S=)`` +
    ``ltv_vectors(uprev=)`` + ``rate_constraints``, written by the definitions with a dense D = ``_rate_difference``.  dH, dg are
    then the cotangents of the rate problem's H, g; dA_r [N nu, n], dl_r, du_r [N nu] those of (A_r, l_r, u_r); S [nu, nu],
    [N, nu, nu] or [B, N, nu, nu] (absent: zero, the rows alone), uprev [nu] ([B, nu]; absent: zero).  With Sig = blkdiag(S_k),
    a = [uprev; 0; ...], dF = D F, r = D s - a, q = D F dg, t = dl_r + du_r, M = dF Hs, Z = dA_r + Sig (2 M + r dg'):
        dA + D'Z in the place of dA,   dl + D'(t - Sig q) in the place of dl   (the gradient of l_add stays dl),
        Sb_k = sym(M_k dF_k' + q_k r_k'),   uprevb = t_0 - S_0 q_0,   dlob = dl_r,   dhib = du_r,
    and the dict gains S (in the shape S was given: summed over the stages for [nu, nu], over the batch without a batch axis),
    uprev, dlo, dhi (per instance)."""
    Ad, Bd = np.asarray(Ad), np.asarray(Bd)
    Q, R = np.asarray(Q), np.asarray(R)
    rate = any(v is not None for v in (S, uprev, dA_r, dl_r, du_r))
    if rate:
        S = np.zeros((Bd.shape[-1], Bd.shape[-1])) if S is None else np.asarray(S)
        _rate_weight_shapes(Bd.shape[-1], Ad.shape[-3], S, B=Ad.shape[0] if Ad.ndim == 4 else None)
    if Ad.ndim == 4:
        B = Ad.shape[0]
        at = lambda a, b: None if a is None else np.asarray(a)[b]
        lu = lambda a, b: np.asarray(a)[b] if np.ndim(a) == 2 else a
        wt = lambda W, b: W[b] if W.ndim == 4 else W
        if _ltv_staged(Q, R):
            _ltv_stage_shapes(Ad.shape[2], Bd.shape[3], Ad.shape[1], Q, R, Qf if Qf is None else np.asarray(Qf), B=B)
        outs = [condense_ltv_vjp(Ad[b], Bd[b], wt(Q, b), wt(R, b), Qf, np.asarray(x0)[b], lu(l_add, b), lu(u_add, b), K=K,
                                 c=at(c, b), xref=at(xref, b), uref=at(uref, b), dH=at(dH, b), dA=at(dA, b), dg=at(dg, b),
                                 dl=at(dl, b), du=at(du, b), S=wt(S, b) if rate else None, uprev=at(uprev, b), dA_r=at(dA_r, b),
                                 dl_r=at(dl_r, b), du_r=at(du_r, b)) for b in range(B)]
        res = {}
        if rate:
            res["S"] = np.stack([o["S"] for o in outs])
            res["S"] = res["S"] if S.ndim == 4 else res["S"].sum(0)
            res.update({k: np.stack([o[k] for o in outs]) for k in ("uprev", "dlo", "dhi")})
        for k in _LTV_VJP_KEYS:
            if k not in outs[0]:                               # (staged Q: no Qf)
                continue
            shared = ((k == "Q" and Q.ndim < 4) or (k == "R" and R.ndim < 4) or k in ("Qf", "K")
                      or (k == "l_add" and np.ndim(l_add) == 1) or (k == "u_add" and np.ndim(u_add) == 1))
            st = np.stack([o[k] for o in outs])
            res[k] = st.sum(0) if shared else st
        return res
    dt = np.result_type(Ad.dtype, np.float64)                  # float64, or wider when the caller passes longdouble
    N, nx, nu = Ad.shape[0], Ad.shape[1], Bd.shape[2]
    blk, n, m = nx + nu, N * nu, N * (nx + nu)
    cast = lambda a, shape: np.zeros(shape, dtype=dt) if a is None else np.asarray(a).astype(dt).reshape(shape)
    Ad, Bd = Ad.astype(dt), Bd.astype(dt)
    Kz, x0 = cast(K, (nu, nx)), cast(x0, (nx,))
    xref, uref = cast(xref, (N, nx)), cast(uref, (N, nu))
    Hb, Ab, gb, lb, ub = cast(dH, (n, n)), cast(dA, (m, n)), cast(dg, (n,)), cast(dl, (m,)), cast(du, (m,))
    cond = condense_ltv(Ad, Bd, Q.astype(dt), R.astype(dt), None if Qf is None else np.asarray(Qf).astype(dt), K=Kz,
                        c=None if c is None else np.asarray(c).astype(dt))
    F, G, f, S_sp = cond["F"], cond["G"], cond["f"], cond["H_sp"]
    e = G @ x0 + f - np.hstack([uref, xref]).reshape(-1)
    Hs = (Hb + Hb.T) / 2
    T = F @ Hs
    rate_out, lb_in = {}, lb
    if rate:
        Sr = S.astype(dt)
        Sk = np.stack([Sr] * N) if Sr.ndim == 2 else Sr
        D, Sig = _rate_difference(N, nx, nu, dt), _blkdiag_dense(Sk)
        a0 = np.zeros(n, dtype=dt)
        a0[:nu] = cast(uprev, (nu,))
        Arb, lrb, urb = cast(dA_r, (n, n)), cast(dl_r, (n,)), cast(du_r, (n,))
        dF, r, q, t = D @ F, D @ (G @ x0 + f) - a0, D @ (F @ gb), lrb + urb
        M = dF @ Hs
        Ab = Ab + D.T @ (Arb + Sig @ (2 * M + np.outer(r, gb)))
        lb = lb + D.T @ (t - Sig @ q)
        Sb = np.stack([M[k * nu:(k + 1) * nu] @ dF[k * nu:(k + 1) * nu].T + np.outer(q[k * nu:(k + 1) * nu], r[k * nu:(k + 1) * nu])
                       for k in range(N)])
        Sb = (Sb + np.swapaxes(Sb, 1, 2)) / 2
        rate_out = dict(S=Sb.sum(0) if Sr.ndim == 2 else Sb, uprev=t[:nu] - Sk[0] @ q[:nu], dlo=lrb, dhi=urb)
    Fb = Ab + 2 * (S_sp @ T) + np.outer(S_sp @ e, gb)
    eb = S_sp @ (F @ gb)
    sb = eb - lb - ub
    Yb = np.hstack([Fb, np.outer(sb, x0), sb[:, None]])
    Fg = F @ gb
    Rb, Qb, Qfb = np.zeros((nu, nu), dtype=dt), np.zeros((nx, nx), dtype=dt), np.zeros((nx, nx), dtype=dt)
    Rst, Qst = np.zeros((N, nu, nu), dtype=dt), np.zeros((N, nx, nx), dtype=dt)
    for k in range(N):                                         # only the diagonal blocks of Sb = F T' + (F dg) e' are needed
        rk = slice(k * blk, (k + 1) * blk)
        Sk = F[rk] @ T[rk].T + np.outer(Fg[rk], e[rk])
        Rb += Sk[:nu, :nu]
        xb = Sk[nu:, nu:]
        Rst[k], Qst[k] = (Sk[:nu, :nu] + Sk[:nu, :nu].T) / 2, (xb + xb.T) / 2
        if k == N - 1:
            Qfb += xb
        else:
            Qb += xb
    Rb, Qb, Qfb = ((W + W.T) / 2 for W in (Rb, Qb, Qfb))
    weights = dict(Q=Qst if Q.ndim == 3 else Qb, R=Rst if R.ndim == 3 else Rb)
    if Q.ndim == 2:
        weights["Qf"] = Qfb
    Y = np.hstack([F, G, f[:, None]])
    X0 = np.zeros((nx, n + nx + 1), dtype=dt)
    X0[:, n:n + nx] = np.eye(nx, dtype=dt)
    X = [X0] + [Y[k * blk + nu:(k + 1) * blk] for k in range(N)]
    Adb, Bdb, cb, Kb = np.zeros_like(Ad), np.zeros_like(Bd), np.zeros((N, nx), dtype=dt), np.zeros((nu, nx), dtype=dt)
    Lam = Yb[(N - 1) * blk + nu:N * blk].copy()
    for k in range(N - 1, -1, -1):
        Yu = Yb[k * blk:k * blk + nu]
        Aclb = Lam @ X[k].T
        Adb[k] = Aclb
        Bdb[k] = Lam[:, k * nu:(k + 1) * nu] - Aclb @ Kz.T
        cb[k] = Lam[:, -1]
        Kb -= Yu @ X[k].T + Bd[k].T @ Aclb
        if k >= 1:
            Lam = (Ad[k] - Bd[k] @ Kz).T @ Lam - Kz.T @ Yu + Yb[(k - 1) * blk + nu:k * blk]
    yr = (-eb).reshape(N, blk)
    return dict(Ad=Adb, Bd=Bdb, c=cb, x0=G.T @ sb, xref=yr[:, nu:].copy(), uref=yr[:, :nu].copy(), l_add=lb_in, u_add=ub, K=Kb,
                **weights, **rate_out)


# Stage constraints: instead of the box on y, stage k carries nc rows  lo_k <= E_k [u_k ; x_{k+1}] <= hi_k  (m_c = N nc rows).
# With y = F v + s, s = G x0 + f:  A_c = E F (block row k = E_k F_k),  l_c = lo - E s,  u_c = hi - E s;  H and g are unchanged.
# stage_constraints / stage_constraints_vjp are the host statements, stage_*_device the device calls (C-ABI rqp_ltv_stage_*).

STAGE_LIMITS = dict(nc=32, m_c=640)                           # what the device kernels hold (rqp_abi.h)


def _stage_check_sizes(N, nc):
    L = STAGE_LIMITS
    if nc < 1 or nc > L["nc"] or N * nc > L["m_c"]:
        raise ValueError("unsupported stage constraints (horizon=%d, nc=%d): the device kernels hold 1 <= nc <= %d rows per "
                         "stage and m_c = horizon nc <= %d" % (N, nc, L["nc"], L["m_c"]))


def _stage_blocks(F, E):
    N, nc, blk = E.shape
    if F.shape[0] != N * blk:
        raise ValueError("E has shape %s, expected [N, nc, nu + nx] with N (nu + nx) = %d" % (tuple(E.shape), F.shape[0]))
    return N, nc, blk


def stage_constraints(cond, E, x0, lo, hi):
    """(A_c, l_c, u_c) of the stage constraints lo_k <= E_k [u_k ; x_{k+1}] <= hi_k on the maps of ``condense_ltv`` (numpy, the
    formulas as written above).  One instance: E [N, nc, nu + nx], x0 [nx], lo, hi [N nc]; or ``cond`` with a batch axis, x0
    [B, nx], E with or without it (shared), lo / hi [B, N nc] or shared [N nc]."""
    F, G, f = cond["F"], cond["G"], cond["f"]
    E, x0 = np.asarray(E).astype(F.dtype), np.asarray(x0).astype(F.dtype)
    if F.ndim == 3:
        outs = [stage_constraints({k: (v if k == "H_sp" else v[b]) for k, v in cond.items()}, E[b] if E.ndim == 4 else E, x0[b],
                                  np.asarray(lo)[b] if np.ndim(lo) == 2 else lo, np.asarray(hi)[b] if np.ndim(hi) == 2 else hi)
                for b in range(F.shape[0])]
        return tuple(np.stack([o[i] for o in outs]) for i in range(3))
    if E.ndim != 3:
        raise ValueError("E has shape %s, expected [N, nc, nu + nx]" % (tuple(E.shape),))
    N, nc, blk = _stage_blocks(F, E)
    lo, hi = np.asarray(lo).astype(F.dtype), np.asarray(hi).astype(F.dtype)
    if lo.shape != (N * nc,) or hi.shape != (N * nc,):
        raise ValueError("lo, hi have shapes %s, %s, expected (%d,)" % (lo.shape, hi.shape, N * nc))
    s = G @ x0 + f
    A_c = np.concatenate([E[k] @ F[k * blk:(k + 1) * blk] for k in range(N)])
    Es = np.concatenate([E[k] @ s[k * blk:(k + 1) * blk] for k in range(N)])
    return A_c, lo - Es, hi - Es


def stage_constraints_vjp(cond, E, x0, dA_c=None, dl_c=None, du_c=None):
    """Reverse of ``stage_constraints`` (numpy): the cotangents dA_c [N nc, n], dl_c, du_c [N nc] (an absent one is zero)
    mapped to (dA_full [m, n], dl_full [m], dE [N, nc, nu + nx], dlo, dhi).  With t = dl_c + du_c:
        dA_full_k = E_k' dA_c,k,   dl_full_k = E_k' t_k,   dE_k = dA_c,k F_k' - t_k s_k',   dlo = dl_c,   dhi = du_c.
    dA_full and dl_full are the ``dA`` and ``dl`` of ``condense_ltv_vjp`` (``du=None`` there), which maps them on to the plant.
    With a batch axis on ``cond``: everything per instance; dE is summed over the batch when E is shared, dlo / dhi stay per
    instance (the sum for shared bounds is the caller's)."""
    F, G, f = cond["F"], cond["G"], cond["f"]
    E, x0 = np.asarray(E).astype(F.dtype), np.asarray(x0).astype(F.dtype)
    if F.ndim == 3:
        at = lambda a, b: None if a is None else np.asarray(a)[b]
        outs = [stage_constraints_vjp({k: (v if k == "H_sp" else v[b]) for k, v in cond.items()}, E[b] if E.ndim == 4 else E,
                                      x0[b], at(dA_c, b), at(dl_c, b), at(du_c, b)) for b in range(F.shape[0])]
        res = [np.stack([o[i] for o in outs]) for i in range(5)]
        if E.ndim == 3:
            res[2] = res[2].sum(0)
        return tuple(res)
    N, nc, blk = _stage_blocks(F, E)
    n = F.shape[1]
    cast = lambda a, shape: np.zeros(shape, dtype=F.dtype) if a is None else np.asarray(a).astype(F.dtype).reshape(shape)
    Ab, lb, ub = cast(dA_c, (N * nc, n)), cast(dl_c, (N * nc,)), cast(du_c, (N * nc,))
    t = lb + ub
    s = G @ x0 + f
    dA_full, dl_full, dE = np.zeros_like(F), np.zeros_like(f), np.zeros_like(E)
    for k in range(N):
        rk, ck = slice(k * blk, (k + 1) * blk), slice(k * nc, (k + 1) * nc)
        dA_full[rk] = E[k].T @ Ab[ck]
        dl_full[rk] = E[k].T @ t[ck]
        dE[k] = Ab[ck] @ F[rk].T - np.outer(t[ck], s[rk])
    return dA_full, dl_full, dE, lb, ub


class _LtvWeights(object):
    """Q, R, Qf (and K) as float64 device tensors (what the C-ABI reads), cached per device."""

    def __init__(self, nx, nu, Q, R, Qf, K):
        self.Q, self.R, self.Qf, self.K = _ltv_weights(nx, nu, Q, R, Qf, K)
        self._dev = {}

    def on(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)
            self._dev[key] = tuple(t(a) for a in (self.Q, self.R, self.Qf, self.K))
        return self._dev[key]


class _LtvTensorWeights(_LtvWeights):
    """Q, R, Qf (K) that already are float64 device tensors (the autograd path: the weights are torch inputs)."""

    def __init__(self, Q, R, Qf, K):
        self._t = (Q, R, Qf, K)

    def on(self, device):
        return self._t


class _LtvStageWeights(_LtvWeights):
    """Stage weights Q [B, N, nx, nx], R [B, N, nu, nu] (and K) as float64 contiguous device tensors, what the C-ABI reads
    with RQP_LTV_STAGE_WEIGHTS.  Given as numpy arrays or tensors, [B, N, ., .] or [N, ., .]; one of Q, R may be a shared
    matrix (a shared Q comes with Qf and is repeated as Q, ..., Q, Qf).  The expansion to [B, N, ., .] is done on the device;
    the symmetric part of every block is used (numpy blocks must be symmetric up to rounding, as the shared weights)."""

    staged = True

    def __init__(self, nx, nu, N, Q, R, Qf, K):
        arr = lambda W: W if hasattr(W, "detach") or W is None else np.asarray(W, dtype=np.float64)
        Q, R, Qf = arr(Q), arr(R), arr(Qf)
        self.batch = _ltv_stage_shapes(nx, nu, N, Q, R, Qf, B=max((W.shape[0] for W in (Q, R) if len(W.shape) == 4), default=None))
        for name, W in (("Q", Q), ("R", R), ("Qf", Qf)):
            if isinstance(W, np.ndarray):
                Wt = np.swapaxes(W, -1, -2)
                if np.abs(W - Wt).max() > 1e-9 * max(np.abs(W).max(), 1e-300):
                    raise ValueError("%s must be symmetric (every block)" % name)
        if K is not None and not hasattr(K, "detach"):
            K = np.asarray(K, dtype=np.float64)
        if K is not None and tuple(K.shape) != (nu, nx):
            raise ValueError("K has shape %s, expected (%d, %d)" % (tuple(K.shape), nu, nx))
        self.N, self.Q, self.R, self.Qf, self.K = N, Q, R, Qf, K
        self._dev = {}

    def on(self, device, B):
        import torch
        if self.batch is not None and self.batch != B:
            raise ValueError("the kept stage weights are for a batch of %d, the stages for %d" % (self.batch, B))
        key = (str(device), B)
        if key not in self._dev:
            t = lambda a: None if a is None else torch.as_tensor(a).detach().to(device=device, dtype=torch.float64)
            Q, R, Qf, K = (t(a) for a in (self.Q, self.R, self.Qf, self.K))
            if Q.dim() == 2:
                Q = torch.cat([Q.expand(self.N - 1, -1, -1), Qf.unsqueeze(0)])
            if R.dim() == 2:
                R = R.expand(self.N, -1, -1)

            def full(W):                       # [B, N, ., .], the symmetric part of every block
                W = W if W.dim() == 4 else W.unsqueeze(0).expand(B, -1, -1, -1)
                return (0.5 * (W + W.transpose(-1, -2))).contiguous()

            self._dev = {key: (full(Q), full(R), None, None if K is None else K.contiguous())}   # (one batch size at a time)
        return self._dev[key]


class _LtvStageTensorWeights(_LtvStageWeights):
    """Stage weights that already are symmetric float64 contiguous device tensors [B, N, ., .] (the autograd path)."""

    def __init__(self, Q, R, K):
        self._t = (Q, R, None, K)

    def on(self, device, B):
        return self._t


def _ltv_weights_on(weights, nx, nu, N, B, device):
    """(Q, R, Qf, K, staged) device tensors of ``weights``: an ``_LtvWeights``, or (Q, R, Qf, K) with shared or staged Q, R."""
    w = weights
    if not isinstance(w, _LtvWeights):
        Q, R, Qf, K = w
        w = _LtvStageWeights(nx, nu, N, Q, R, Qf, K) if _ltv_staged(Q, R) else _LtvWeights(nx, nu, Q, R, Qf, K)
    staged = getattr(w, "staged", False)
    return (w.on(device, B) if staged else w.on(device)) + (staged,)


def ltv_adjoint_workspace(batch, nx, nu, horizon, device):
    """The float64 workspace of ``condense_ltv_adjoint_device`` for these sizes (a device tensor)."""
    import ctypes
    import torch
    from reluqp import _cabi
    _ltv_check_sizes(nx, nu, horizon)
    lib = _cabi.load()
    dims = _cabi.LtvDims(batch=batch, nx=nx, nu=nu, horizon=horizon, dtype=_cabi.RQP_F64, flags=0)
    nbytes = ctypes.c_size_t()
    _cabi.check(None, lib.rqp_ltv_adjoint_workspace_bytes(ctypes.byref(dims), ctypes.byref(nbytes)),
                "rqp_ltv_adjoint_workspace_bytes", handleless=True)
    return torch.empty(nbytes.value // 8, dtype=torch.float64, device=device)


def ltv_adjoint_rate_workspace(batch, nx, nu, horizon, device):
    """The float64 workspace of ``condense_ltv_adjoint_rate_device`` for these sizes (a device tensor): that of
    ``ltv_adjoint_workspace`` and 2 N nu doubles per instance; it serves ``condense_ltv_adjoint_device`` as well."""
    import ctypes
    import torch
    from reluqp import _cabi
    _ltv_check_sizes(nx, nu, horizon)
    lib = _cabi.load()
    dims = _cabi.LtvDims(batch=batch, nx=nx, nu=nu, horizon=horizon, dtype=_cabi.RQP_F64, flags=0)
    nbytes = ctypes.c_size_t()
    _cabi.check(None, lib.rqp_ltv_adjoint_rate_workspace_bytes(ctypes.byref(dims), ctypes.byref(nbytes)),
                "rqp_ltv_adjoint_rate_workspace_bytes", handleless=True)
    return torch.empty(nbytes.value // 8, dtype=torch.float64, device=device)


LTV_ADJOINT_OUTPUTS = ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R", "Qf")
LTV_RATE_ADJOINT_OUTPUTS = LTV_ADJOINT_OUTPUTS + ("S", "uprev")


def condense_ltv_adjoint_rate_device(Ad, Bd, x0, weights, workspace, adjoint_workspace, S, uprev, xref=None, uref=None, dH=None,
                                     dA=None, dg=None, dl=None, du=None, dA_r=None, dl_r=None, du_r=None, row0=0, want=None):
    """Reverse of ``condense_ltv_device(S=)`` + ``ltv_vectors_device(S=, uprev=)`` + ``rate_rows_device`` +
    ``rate_bounds_device`` on the device (C-ABI rqp_ltv_condense_adjoint_rate; the host statement is ``condense_ltv_vjp`` with
    its rate keywords).  As ``condense_ltv_adjoint_device``, and: ``S`` from ``rate_weight_device``, ``uprev`` [B, nu];
    ``workspace`` from either way of condensing this linearisation; ``adjoint_workspace`` from ``ltv_adjoint_rate_workspace``;
    dH, dg the cotangents of the rate problem's H, g; dA, dl, du those of the base rows; dA_r [B, mt, n], dl_r, du_r [B, mt] those
    of the rate rows, which are rows row0 .. row0 + N nu of every instance (mt = N nu and row0 = 0: the rate rows alone; else
    the tails of the whole QP's cotangents, read in place).  ``want`` may also name "S" ([B, N, nu, nu] float64, per instance
    and stage) and "uprev" ([B, nu])."""
    return _ltv_adjoint_call(Ad, Bd, x0, weights, workspace, adjoint_workspace, xref, uref, dH, dA, dg, dl, du, want,
                             rate=dict(S=S, uprev=uprev, dA_r=dA_r, dl_r=dl_r, du_r=du_r, row0=int(row0)))


def condense_ltv_adjoint_device(Ad, Bd, x0, weights, workspace, adjoint_workspace, xref=None, uref=None, dH=None, dA=None,
                                dg=None, dl=None, du=None, want=None):
    """Reverse of ``condense_ltv_device`` + ``ltv_vectors_device`` on the device (C-ABI rqp_ltv_condense_adjoint; the host
    statement is ``condense_ltv_vjp``).  ``workspace`` is the forward workspace as ``condense_ltv_device`` left it for these
    Ad, Bd (c); dH [B, n, n], dA [B, m, n], dg [B, n], dl, du [B, m] are the cotangents (None = zero), device tensors of
    Ad's precision.  ``want`` names the gradients to compute (None: all): a dict of those comes back (Ad, Bd, c, x0, xref, uref in Ad's
    precision; Q, R, Qf float64, summed over the batch).  Stage weights (``_LtvStageWeights``, or staged Q, R in the tuple): Q, R
    come back [B, N, ., .] float64, each block its own instance's and stage's, and "Qf" cannot be wanted.  Enqueued on the
    current stream."""
    return _ltv_adjoint_call(Ad, Bd, x0, weights, workspace, adjoint_workspace, xref, uref, dH, dA, dg, dl, du, want)


def _ltv_adjoint_call(Ad, Bd, x0, weights, workspace, adjoint_workspace, xref, uref, dH, dA, dg, dl, du, want, rate=None):
    """The two device adjoints: ``rate`` None is rqp_ltv_condense_adjoint, else rqp_ltv_condense_adjoint_rate."""
    import ctypes
    import torch
    from reluqp import _cabi
    B, N, nx, nu = _ltv_shapes(Ad, Bd)
    _ltv_check_sizes(nx, nu, N)
    if not torch.is_tensor(Ad) or Ad.device.type != "cuda":
        raise _cabi.RqpUnavailable("condense_ltv_adjoint%s_device needs device tensors; the host restatement is condense_ltv_vjp"
                                   % ("" if rate is None else "_rate"))
    dtype, device = Ad.dtype, Ad.device
    n, m = N * nu, N * (nx + nu)
    Q, R, Qf, K, staged = _ltv_weights_on(weights, nx, nu, N, B, device)
    known = LTV_ADJOINT_OUTPUTS if rate is None else LTV_RATE_ADJOINT_OUTPUTS
    if want is None:                           # every gradient there is
        want = tuple(k for k in known if not (staged and k == "Qf"))
    unknown = [k for k in want if k not in known]
    if unknown:
        raise ValueError("unknown gradient name(s) %s; known: %s" % (unknown, known))
    if staged and "Qf" in want:
        raise ValueError("stage weights have no Qf: its gradient is that of Q[:, N-1]")
    opt = lambda t, shape, name: None if t is None else _ltv_in(t, shape, dtype, device, name)
    Ad, Bd, x0 = opt(Ad, (B, N, nx, nx), "Ad"), opt(Bd, (B, N, nx, nu), "Bd"), opt(x0, (B, nx), "x0")
    xref, uref = opt(xref, (B, N, nx), "xref"), opt(uref, (B, N, nu), "uref")
    dH, dA, dg = opt(dH, (B, n, n), "dH"), opt(dA, (B, m, n), "dA"), opt(dg, (B, n), "dg")
    dl, du = opt(dl, (B, m), "dl"), opt(du, (B, m), "du")
    shapes = dict(Ad=(B, N, nx, nx), Bd=(B, N, nx, nu), c=(B, N, nx), x0=(B, nx), xref=(B, N, nx), uref=(B, N, nu),
                  Q=(nx, nx), R=(nu, nu), Qf=(nx, nx))
    if staged:
        shapes.update(Q=(B, N, nx, nx), R=(B, N, nu, nu))
    shapes.update(S=(B, N, nu, nu), uprev=(B, nu))
    out = {k: torch.empty(shapes[k], dtype=torch.float64 if k in ("Q", "R", "Qf", "S") else dtype, device=device) for k in want}
    rio = None
    if rate is not None:
        rio, row0 = _cabi.LtvRateAdjointIO(), rate["row0"]
        rio.S = _rate_tensor(rate["S"], (B, N, nu, nu), device).data_ptr()
        rio.uprev = _ltv_in(rate["uprev"], (B, nu), dtype, device, "uprev").data_ptr()
        keep = []                              # (the tensors whose addresses rio holds stay alive until the call)
        for name, row in (("dA_r", (n,)), ("dl_r", ()), ("du_r", ())):
            t = rate[name]
            if t is None:
                continue
            t = torch.as_tensor(t).to(device=device, dtype=dtype).contiguous()
            if t.dim() != 2 + len(row) or t.shape[0] != B or tuple(t.shape[2:]) != row or row0 < 0 or row0 + n > t.shape[1]:
                raise ValueError("%s has shape %s, expected [%d, mt%s] with the %d rate rows from row %d on"
                                 % (name, tuple(t.shape), B, ", %d" % n if row else "", n, row0))
            keep.append(t)
            per_row = n if row else 1
            setattr(rio, name, t.data_ptr() + row0 * per_row * t.element_size())
            setattr(rio, "dA_stride" if row else "dl_stride", t.shape[1] * per_row)
        if rate["dl_r"] is not None and rate["du_r"] is not None and rate["dl_r"].shape[1] != rate["du_r"].shape[1]:
            raise ValueError("dl_r and du_r must have the same shape")
        for k in ("S", "uprev"):
            if k in out:
                setattr(rio, "d" + k, out[k].data_ptr())
    io = _cabi.LtvAdjointIO()
    for name, t in (("Ad", Ad), ("Bd", Bd), ("x0", x0), ("xref", xref), ("uref", uref), ("Q", Q), ("R", R), ("Qf", Qf), ("K", K),
                    ("workspace", workspace), ("dH", dH), ("dA", dA), ("dg", dg), ("dl", dl), ("du", du),
                    ("adjoint_workspace", adjoint_workspace)):
        setattr(io, name, None if t is None else t.data_ptr())
    for k, t in out.items():
        if k not in ("S", "uprev"):
            setattr(io, "d" + k, t.data_ptr())
    flags = ((_cabi.LTV_HAS_K if K is not None else 0) | (_cabi.LTV_HAS_XREF if xref is not None else 0)
             | (_cabi.LTV_HAS_UREF if uref is not None else 0) | (_cabi.LTV_STAGE_WEIGHTS if staged else 0))
    dims = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64 if dtype == torch.float64 else _cabi.RQP_F32,
                         flags=flags)
    lib = _cabi.load()
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        if rio is None:
            _cabi.check(None, lib.rqp_ltv_condense_adjoint(ctypes.byref(dims), device.index or 0, ctypes.byref(io), stream),
                        "rqp_ltv_condense_adjoint", handleless=True)
        else:
            _cabi.check(None, lib.rqp_ltv_condense_adjoint_rate(ctypes.byref(dims), device.index or 0, ctypes.byref(io),
                                                                ctypes.byref(rio), stream),
                        "rqp_ltv_condense_adjoint_rate", handleless=True)
    return out


class LTVCondenser(object):
    """What ``reluqp.layer.LTVCondenseFunction`` keeps between calls: the sizes, the shared gain K, and per (batch, device)
    one forward workspace, one adjoint workspace and scratch H / A.  The forward workspace (F, H_sp F, [G | f]: the largest
    tensors of the condensing) is never cloned: ``stamp`` says which forward's linearisation it holds, and a backward whose
    forward has been overwritten by a later one condenses its saved (small) inputs again before it differentiates.
    Memory: a slot lives as long as the condenser and holds 8 (2 m n + (m + n)(nx + 1)) bytes per instance forward and
    8 (m n + 4 m + N (nu^2 + nx^2)) bytes per instance adjoint workspace (0.45 MB + 0.22 MB at (12, 4, 20)), for every distinct
    (batch, device, dtype) the layer has seen; ``release()`` drops them.  The H / A outputs that a re-condense discards are
    allocated by the first backward that needs one."""

    def __init__(self, nx, nu, horizon, K=None):
        nx, nu, horizon = int(nx), int(nu), int(horizon)
        _ltv_check_sizes(nx, nu, horizon)
        self.nx, self.nu, self.horizon = nx, nu, horizon
        self.n, self.m = horizon * nu, horizon * (nx + nu)
        if K is not None:
            if getattr(K, "requires_grad", False):
                raise ValueError("K cannot require a gradient: the pre-stabilising gain is a reparametrisation of the inputs "
                                 "(u_0 = v_0 - K x0 does not depend on it), pass K.detach()")
            K = np.asarray(K.detach().cpu() if hasattr(K, "detach") else K, dtype=np.float64)
            if K.shape != (nu, nx):
                raise ValueError("K has shape %s, expected (%d, %d)" % (K.shape, nu, nx))
        self.K = K
        self._slots = {}
        self._count = 0

    def slot(self, B, device, dtype):
        import torch
        key = (B, str(device), dtype)
        if key not in self._slots:
            self._slots[key] = dict(ws=ltv_workspace(B, self.nx, self.nu, self.horizon, device),
                                    adj=ltv_adjoint_workspace(B, self.nx, self.nu, self.horizon, device),
                                    H=None, A=None,
                                    K=None if self.K is None else torch.as_tensor(self.K, dtype=torch.float64, device=device),
                                    stamp=0, adj_for=(B, device))
        return self._slots[key]

    def recondense_outputs(self, slot, B, device, dtype):
        import torch
        if slot["H"] is None:
            slot["H"] = torch.empty((B, self.n, self.n), dtype=dtype, device=device)
            slot["A"] = torch.empty((B, self.m, self.n), dtype=dtype, device=device)
        return slot["H"], slot["A"]

    def rate_adjoint_workspace(self, slot):
        """The slot's adjoint workspace, grown once to what rqp_ltv_condense_adjoint_rate needs (it serves the plain call too)."""
        if not slot.get("adj_rate"):
            B, device = slot["adj_for"]
            slot["adj"], slot["adj_rate"] = ltv_adjoint_rate_workspace(B, self.nx, self.nu, self.horizon, device), True
        return slot["adj"]

    def release(self):
        """Drop every workspace (the next forward allocates again; a pending backward of an earlier forward must not follow)."""
        self._slots = {}

    def next_stamp(self):
        self._count += 1
        return self._count


def ltv_workspace(batch, nx, nu, horizon, device):
    """The float64 workspace of ``condense_ltv_device`` / ``ltv_vectors_device`` for these sizes (a device tensor)."""
    import ctypes
    import torch
    from reluqp import _cabi
    _ltv_check_sizes(nx, nu, horizon)
    lib = _cabi.load()
    dims = _cabi.LtvDims(batch=batch, nx=nx, nu=nu, horizon=horizon, dtype=_cabi.RQP_F64, flags=0)
    nbytes = ctypes.c_size_t()
    _cabi.check(None, lib.rqp_ltv_workspace_bytes(ctypes.byref(dims), ctypes.byref(nbytes)), "rqp_ltv_workspace_bytes", handleless=True)
    return torch.empty(nbytes.value // 8, dtype=torch.float64, device=device)


def _ltv_out(t, shape, dtype, device, name):
    import torch
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), device))
    return t


def _ltv_in(t, shape, dtype, device, name):
    import torch
    t = torch.as_tensor(t).to(device=device, dtype=dtype).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


def rate_weight_device(S, nu, N, B, device):
    """S [nu, nu], [N, nu, nu] or [B, N, nu, nu] (numpy or tensor) as the C-ABI reads it: a float64 contiguous device tensor
    [B, N, nu, nu], the symmetric part of every block (numpy blocks must be symmetric up to rounding, like the other weights).
    The expansion is done on the device."""
    import torch
    if not hasattr(S, "detach"):
        S = np.asarray(S, dtype=np.float64)
        if S.ndim >= 2 and np.abs(S - np.swapaxes(S, -1, -2)).max() > 1e-9 * max(np.abs(S).max(), 1e-300):
            raise ValueError("S must be symmetric (every block)")
    _rate_weight_shapes(nu, N, S, B=B)
    S = torch.as_tensor(S).detach().to(device=device, dtype=torch.float64)
    S = S.expand(B, N, nu, nu)
    return (0.5 * (S + S.transpose(-1, -2))).contiguous()


def condense_ltv_device(Ad, Bd, weights, workspace, c=None, H=None, A=None, S=None):
    """H [B, n, n], A [B, m, n] of the condensed LTV QPs, built on the device (C-ABI rqp_ltv_condense) from device tensors
    Ad [B, N, nx, nx], Bd [B, N, nx, nu] (c [B, N, nx]) of the output precision (float32 or float64).  ``weights`` is
    ``(Q, R, Qf, K)`` (numpy, K may be None) or an ``_LtvWeights``; staged Q [B, N, nx, nx] or [N, nx, nx] and / or R in the tuple
    (then Qf = None for a staged Q), or an ``_LtvStageWeights``, select the stage-weight kernels (RQP_LTV_STAGE_WEIGHTS);
    ``workspace`` from ``ltv_workspace`` carries the maps the vector step needs.  ``H`` / ``A``: optional output tensors.
    ``S``: a rate weight from ``rate_weight_device`` ([B, N, nu, nu] float64 on the device) adds the input-rate cost
    (C-ABI rqp_ltv_condense_rate); the workspace then serves ``ltv_vectors_device(..., S=, uprev=)`` only, and its adjoint is
    ``condense_ltv_adjoint_rate_device``.
    Enqueued on the current stream; returns (H, A)."""
    import ctypes
    import torch
    from reluqp import _cabi
    B, N, nx, nu = _ltv_shapes(Ad, Bd)
    _ltv_check_sizes(nx, nu, N)
    if not torch.is_tensor(Ad) or Ad.device.type != "cuda":
        raise _cabi.RqpUnavailable("condense_ltv_device needs device tensors; the host restatement is condense_ltv")
    dtype, device = Ad.dtype, Ad.device
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("Ad must be float32 or float64")
    Q, R, Qf, K, staged = _ltv_weights_on(weights, nx, nu, N, B, device)
    n, m = N * nu, N * (nx + nu)
    Ad, Bd = _ltv_in(Ad, (B, N, nx, nx), dtype, device, "Ad"), _ltv_in(Bd, (B, N, nx, nu), dtype, device, "Bd")
    c = None if c is None else _ltv_in(c, (B, N, nx), dtype, device, "c")
    H, A = _ltv_out(H, (B, n, n), dtype, device, "H"), _ltv_out(A, (B, m, n), dtype, device, "A")
    flags = ((_cabi.LTV_HAS_K if K is not None else 0) | (_cabi.LTV_HAS_C if c is not None else 0)
             | (_cabi.LTV_STAGE_WEIGHTS if staged else 0))
    dims = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64 if dtype == torch.float64 else _cabi.RQP_F32,
                         flags=flags)
    lib = _cabi.load()
    if S is not None:
        S = _rate_tensor(S, (B, N, nu, nu), device)
        with torch.cuda.device(device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            _cabi.check(None, lib.rqp_ltv_condense_rate(ctypes.byref(dims), device.index or 0, _cabi.ptr(Ad), _cabi.ptr(Bd),
                                                        _cabi.ptr(c), _cabi.ptr(Q), _cabi.ptr(R), _cabi.ptr(Qf), _cabi.ptr(K),
                                                        _cabi.ptr(S), _cabi.ptr(H), _cabi.ptr(A), _cabi.ptr(workspace), stream),
                        "rqp_ltv_condense_rate", handleless=True)
        return H, A
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _cabi.check(None, lib.rqp_ltv_condense(ctypes.byref(dims), device.index or 0, _cabi.ptr(Ad), _cabi.ptr(Bd), _cabi.ptr(c),
                                               _cabi.ptr(Q), _cabi.ptr(R), _cabi.ptr(Qf), _cabi.ptr(K), _cabi.ptr(H), _cabi.ptr(A),
                                               _cabi.ptr(workspace), stream), "rqp_ltv_condense", handleless=True)
    return H, A


def _rate_tensor(S, shape, device):
    import torch
    if (not torch.is_tensor(S) or S.dtype != torch.float64 or S.device != device or tuple(S.shape) != tuple(shape)
            or not S.is_contiguous()):
        raise ValueError("S must be a contiguous float64 tensor of shape %s on %s (rate_weight_device)" % (tuple(shape), device))
    return S


def ltv_vectors_device(dims5, x0, l_add, u_add, weights, workspace, xref=None, uref=None, g=None, l=None, u=None, S=None,
                       uprev=None):
    """g [B, n], l, u [B, m] from the workspace of the last ``condense_ltv_device`` (C-ABI rqp_ltv_vectors).
    ``dims5`` = (nx, nu, horizon, has_K, has_c) of that call; x0 [B, nx] (xref [B, N, nx], uref [B, N, nu]) device tensors of the
    output precision, l_add / u_add [m] or [B, m]; ``weights`` as in that call (stage weights: the same ones, for H_sp yref).
    A workspace of ``condense_ltv_device(..., S=)`` needs the same ``S`` and ``uprev`` [B, nu] here (C-ABI rqp_ltv_vectors_rate).
    Enqueued on the current stream; returns (g, l, u)."""
    import ctypes
    import torch
    from reluqp import _cabi
    nx, nu, N, has_K, has_c = dims5
    if (S is None) != (uprev is None):
        raise ValueError("S and uprev go together: both for a workspace condensed with a rate weight, else neither")
    if not torch.is_tensor(x0) or x0.device.type != "cuda":
        raise _cabi.RqpUnavailable("ltv_vectors_device needs device tensors; the host restatement is ltv_vectors")
    dtype, device, B = x0.dtype, x0.device, x0.shape[0]
    n, m = N * nu, N * (nx + nu)
    x0 = _ltv_in(x0, (B, nx), dtype, device, "x0")
    xref = None if xref is None else _ltv_in(xref, (B, N, nx), dtype, device, "xref")
    uref = None if uref is None else _ltv_in(uref, (B, N, nu), dtype, device, "uref")
    batched = torch.as_tensor(l_add).dim() == 2
    l_add = _ltv_in(l_add, (B, m) if batched else (m,), dtype, device, "l_add")
    u_add = _ltv_in(u_add, (B, m) if batched else (m,), dtype, device, "u_add")
    Q, R, Qf, _, staged = _ltv_weights_on(weights, nx, nu, N, B, device)
    g, l, u = (_ltv_out(g, (B, n), dtype, device, "g"), _ltv_out(l, (B, m), dtype, device, "l"),
               _ltv_out(u, (B, m), dtype, device, "u"))
    flags = ((_cabi.LTV_HAS_K if has_K else 0) | (_cabi.LTV_HAS_C if has_c else 0) | (_cabi.LTV_HAS_XREF if xref is not None else 0)
             | (_cabi.LTV_HAS_UREF if uref is not None else 0) | (_cabi.LTV_BOUNDS_BATCHED if batched else 0)
             | (_cabi.LTV_STAGE_WEIGHTS if staged else 0))
    dims = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64 if dtype == torch.float64 else _cabi.RQP_F32,
                         flags=flags)
    lib = _cabi.load()
    if S is not None:
        S, uprev = _rate_tensor(S, (B, N, nu, nu), device), _ltv_in(uprev, (B, nu), dtype, device, "uprev")
        with torch.cuda.device(device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            _cabi.check(None, lib.rqp_ltv_vectors_rate(ctypes.byref(dims), device.index or 0, _cabi.ptr(x0), _cabi.ptr(xref),
                                                       _cabi.ptr(uref), _cabi.ptr(l_add), _cabi.ptr(u_add), _cabi.ptr(Q), _cabi.ptr(R),
                                                       _cabi.ptr(Qf), _cabi.ptr(S), _cabi.ptr(uprev), _cabi.ptr(workspace),
                                                       _cabi.ptr(g), _cabi.ptr(l), _cabi.ptr(u), stream),
                        "rqp_ltv_vectors_rate", handleless=True)
        return g, l, u
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _cabi.check(None, lib.rqp_ltv_vectors(ctypes.byref(dims), device.index or 0, _cabi.ptr(x0), _cabi.ptr(xref), _cabi.ptr(uref),
                                              _cabi.ptr(l_add), _cabi.ptr(u_add), _cabi.ptr(Q), _cabi.ptr(R), _cabi.ptr(Qf),
                                              _cabi.ptr(workspace), _cabi.ptr(g), _cabi.ptr(l), _cabi.ptr(u), stream),
                    "rqp_ltv_vectors", handleless=True)
    return g, l, u


def _rate_call(dims4, dtype, device, what):
    import torch
    from reluqp import _cabi
    B, nx, nu, N = (int(v) for v in dims4)
    _ltv_check_sizes(nx, nu, N)
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("dtype must be float32 or float64")
    if torch.device(device).type != "cuda":
        raise _cabi.RqpUnavailable("%s needs device tensors; the host restatement is rate_constraints" % what)
    dims = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64 if dtype == torch.float64 else _cabi.RQP_F32, flags=0)
    return _cabi.load(), dims


def _rate_tail(t, shape, row0, dtype, device, name):
    """The tensor the rate rows go into and the element offset of its row ``row0``: ``t`` [B, mt, ...] contiguous with
    row0 + N nu <= mt, or None: a new one that holds the rate rows alone."""
    import torch
    if t is None:
        if row0:
            raise ValueError("row0 needs the tensor to write into")
        return torch.empty(shape, dtype=dtype, device=device)
    ok = (t.dtype == dtype and t.device == device and t.is_contiguous() and t.dim() == len(shape) and t.shape[0] == shape[0]
          and tuple(t.shape[2:]) == tuple(shape[2:]) and 0 <= row0 and row0 + shape[1] <= t.shape[1])
    if not ok:
        raise ValueError("%s must be a contiguous %s tensor [%d, mt, ...] on %s with room for %d rows from row %d on"
                         % (name, dtype, shape[0], device, shape[1], row0))
    return t


def rate_rows_device(dims4, workspace, dtype, A_r=None, row0=0):
    """A_r,k = F[u_k] - F[u_{k-1}] [B, N nu, n] from the workspace of the last ``condense_ltv_device`` (C-ABI rqp_ltv_rate_rows).
    ``dims4`` = (B, nx, nu, horizon) of that call, ``dtype`` the output precision.  ``A_r``: optional contiguous tensor
    [B, mt, n] to write into, the rate rows landing in its rows row0 .. row0 + N nu of every instance (the others are not
    touched).  Enqueued on the current stream; returns the tensor written into (entries right of the staircase: exact zeros)."""
    import ctypes
    import torch
    from reluqp import _cabi
    device = workspace.device
    lib, dims = _rate_call(dims4, dtype, device, "rate_rows_device")
    n = dims.horizon * dims.nu
    A_r = _rate_tail(A_r, (dims.batch, n, n), row0, dtype, device, "A_r")
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _cabi.check(None, lib.rqp_ltv_rate_rows(ctypes.byref(dims), device.index or 0, _cabi.ptr(workspace),
                                                ctypes.c_void_p(A_r.data_ptr() + row0 * n * A_r.element_size()),
                                                A_r.shape[1] * n, stream), "rqp_ltv_rate_rows", handleless=True)
    return A_r


def rate_bounds_device(dims4, x0, uprev, dlo, dhi, workspace, l_r=None, u_r=None, row0=0):
    """l_r,k = dlo_k - ds_k + [k = 0] uprev, u_r likewise with dhi [B, N nu], ds the differences of s = G x0 + f of the
    workspace over the u rows (C-ABI rqp_ltv_rate_bounds).  x0 [B, nx], uprev [B, nu]; dlo, dhi [N nu] or [B, N nu] (infinite
    entries stay infinite).  ``l_r`` / ``u_r``: optional contiguous tensors [B, mt] to write into, from entry row0 on.
    Enqueued on the current stream; returns (l_r, u_r)."""
    import ctypes
    import torch
    from reluqp import _cabi
    if not torch.is_tensor(x0):
        raise ValueError("x0 must be a torch tensor")
    dtype, device = x0.dtype, x0.device
    lib, dims = _rate_call(dims4, dtype, device, "rate_bounds_device")
    B, n = dims.batch, dims.horizon * dims.nu
    x0, uprev = _ltv_in(x0, (B, dims.nx), dtype, device, "x0"), _ltv_in(uprev, (B, dims.nu), dtype, device, "uprev")
    batched = torch.as_tensor(dlo).dim() == 2
    dlo = _ltv_in(dlo, (B, n) if batched else (n,), dtype, device, "dlo")
    dhi = _ltv_in(dhi, (B, n) if batched else (n,), dtype, device, "dhi")
    if batched:
        dims.flags |= _cabi.LTV_BOUNDS_BATCHED
    if (l_r is None) != (u_r is None):
        raise ValueError("l_r and u_r go together")
    l_r, u_r = _rate_tail(l_r, (B, n), row0, dtype, device, "l_r"), _rate_tail(u_r, (B, n), row0, dtype, device, "u_r")
    if l_r.shape != u_r.shape:
        raise ValueError("l_r and u_r must have the same shape")
    at = lambda t: ctypes.c_void_p(t.data_ptr() + row0 * t.element_size())
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _cabi.check(None, lib.rqp_ltv_rate_bounds(ctypes.byref(dims), device.index or 0, _cabi.ptr(x0), _cabi.ptr(uprev),
                                                  _cabi.ptr(dlo), _cabi.ptr(dhi), _cabi.ptr(workspace), at(l_r), at(u_r),
                                                  l_r.shape[1], stream), "rqp_ltv_rate_bounds", handleless=True)
    return l_r, u_r


def _stage_call(dims4, E, what):
    """Common front of the stage_*_device wrappers: (lib, LtvDims without the bounds flag, nc, E, dtype, device)."""
    import torch
    from reluqp import _cabi
    B, nx, nu, N = (int(v) for v in dims4)
    _ltv_check_sizes(nx, nu, N)
    if not torch.is_tensor(E):
        raise ValueError("E must be a torch tensor")
    dtype, device = E.dtype, E.device
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("E must be float32 or float64")
    if E.dim() not in (3, 4) or tuple(E.shape[-3::2]) != (N, nu + nx) or (E.dim() == 4 and E.shape[0] != B):
        raise ValueError("E has shape %s, expected [%d, nc, %d] or [%d, %d, nc, %d]" % (tuple(E.shape), N, nu + nx, B, N, nu + nx))
    nc = int(E.shape[-2])
    _stage_check_sizes(N, nc)
    if device.type != "cuda":
        raise _cabi.RqpUnavailable("%s needs device tensors; the host restatement is stage_constraints%s"
                                   % (what, "_vjp" if "adjoint" in what else ""))
    dims = _cabi.LtvDims(batch=B, nx=nx, nu=nu, horizon=N, dtype=_cabi.RQP_F64 if dtype == torch.float64 else _cabi.RQP_F32,
                         flags=_cabi.LTV_STAGE_SHARED_E if E.dim() == 3 else 0)
    return _cabi.load(), dims, nc, E.contiguous(), dtype, device


def stage_rows_device(dims4, E, workspace, A_c=None):
    """A_c = E F [B, N nc, n] from the workspace of the last ``condense_ltv_device`` (C-ABI rqp_ltv_stage_rows).  ``dims4`` =
    (B, nx, nu, horizon) of that call; E [B, N, nc, nu + nx] or shared [N, nc, nu + nx], a device tensor of the output
    precision.  Enqueued on the current stream; returns A_c (its entries right of the staircase are exact zeros)."""
    import ctypes
    import torch
    from reluqp import _cabi
    lib, dims, nc, E, dtype, device = _stage_call(dims4, E, "stage_rows_device")
    A_c = _ltv_out(A_c, (dims.batch, dims.horizon * nc, dims.horizon * dims.nu), dtype, device, "A_c")
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _cabi.check(None, lib.rqp_ltv_stage_rows(ctypes.byref(dims), device.index or 0, nc, _cabi.ptr(E), _cabi.ptr(workspace),
                                                 _cabi.ptr(A_c), stream), "rqp_ltv_stage_rows", handleless=True)
    return A_c


def stage_vectors_device(dims4, E, x0, lo, hi, workspace, l_c=None, u_c=None):
    """l_c = lo - E s, u_c = hi - E s [B, N nc] with s = G x0 + f of the workspace (C-ABI rqp_ltv_stage_vectors).  x0 [B, nx];
    lo, hi [N nc] or [B, N nc] (infinite entries stay infinite).  Enqueued on the current stream; returns (l_c, u_c)."""
    import ctypes
    import torch
    from reluqp import _cabi
    lib, dims, nc, E, dtype, device = _stage_call(dims4, E, "stage_vectors_device")
    B, mc = dims.batch, dims.horizon * nc
    x0 = _ltv_in(x0, (B, dims.nx), dtype, device, "x0")
    batched = torch.as_tensor(lo).dim() == 2
    lo = _ltv_in(lo, (B, mc) if batched else (mc,), dtype, device, "lo")
    hi = _ltv_in(hi, (B, mc) if batched else (mc,), dtype, device, "hi")
    if batched:
        dims.flags |= _cabi.LTV_BOUNDS_BATCHED
    l_c, u_c = _ltv_out(l_c, (B, mc), dtype, device, "l_c"), _ltv_out(u_c, (B, mc), dtype, device, "u_c")
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _cabi.check(None, lib.rqp_ltv_stage_vectors(ctypes.byref(dims), device.index or 0, nc, _cabi.ptr(E), _cabi.ptr(x0),
                                                    _cabi.ptr(lo), _cabi.ptr(hi), _cabi.ptr(workspace), _cabi.ptr(l_c),
                                                    _cabi.ptr(u_c), stream), "rqp_ltv_stage_vectors", handleless=True)
    return l_c, u_c


STAGE_ADJOINT_OUTPUTS = ("dA_full", "dl_full", "dE")


def stage_adjoint_device(dims4, E, x0, workspace, dA_c=None, dl_c=None, du_c=None, want=STAGE_ADJOINT_OUTPUTS, out=None):
    """Reverse of ``stage_rows_device`` + ``stage_vectors_device`` (C-ABI rqp_ltv_stage_adjoint; the host statement is
    ``stage_constraints_vjp``).  ``workspace`` is the forward workspace of this linearisation; dA_c [B, N nc, n], dl_c, du_c
    [B, N nc] are the cotangents (None = zero).  Returns a dict of the outputs ``want`` names: dA_full [B, m, n] and dl_full
    [B, m] (the ``dA``, ``dl`` of ``condense_ltv_adjoint_device``), dE [B, N, nc, nu + nx] (per instance also for a shared E).
    ``out``: optional dict of tensors to write into.  Enqueued on the current stream."""
    import ctypes
    import torch
    from reluqp import _cabi
    lib, dims, nc, E, dtype, device = _stage_call(dims4, E, "stage_adjoint_device")
    unknown = [k for k in want if k not in STAGE_ADJOINT_OUTPUTS]
    if unknown:
        raise ValueError("unknown output name(s) %s; known: %s" % (unknown, STAGE_ADJOINT_OUTPUTS))
    B, N, nx, nu = dims.batch, dims.horizon, dims.nx, dims.nu
    n, m, mc = N * nu, N * (nx + nu), N * nc
    x0 = _ltv_in(x0, (B, nx), dtype, device, "x0")
    opt = lambda t, shape, name: None if t is None else _ltv_in(t, shape, dtype, device, name)
    dA_c, dl_c, du_c = opt(dA_c, (B, mc, n), "dA_c"), opt(dl_c, (B, mc), "dl_c"), opt(du_c, (B, mc), "du_c")
    shapes = dict(dA_full=(B, m, n), dl_full=(B, m), dE=(B, N, nc, nu + nx))
    res = {k: _ltv_out(None if out is None else out.get(k), shapes[k], dtype, device, k) for k in want}
    io = _cabi.LtvStageAdjointIO()
    for name, t in (("E", E), ("x0", x0), ("workspace", workspace), ("dA_c", dA_c), ("dl_c", dl_c), ("du_c", du_c)):
        setattr(io, name, None if t is None else t.data_ptr())
    for k, t in res.items():
        setattr(io, k, t.data_ptr())
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _cabi.check(None, lib.rqp_ltv_stage_adjoint(ctypes.byref(dims), device.index or 0, nc, ctypes.byref(io), stream),
                    "rqp_ltv_stage_adjoint", handleless=True)
    return res


class BatchedLTVMPC(object):
    """Closed-loop MPC on a batch of plants that each have their own, time-varying linearisation.

    ``linearize(Ad, Bd, c=None)`` condenses the batch on the device (first call: ``ReLU_QP.setup`` with per-instance
    matrices; later calls: ``update(Hx=, Ax=)``, which re-factors on the device and keeps the ADMM state), ``step(x)`` builds
    (g, l, u) for the current states on the device, ``update(g, l, u)``, warm-started ``solve()``, and returns the first input
    u_0 = v_0 - K x [B, nu] (a device tensor) and the ``Results``.  Weights Q, R, Qf and the pre-stabilising gain K are shared
    by the batch; the box |u| <= u_max, |x| <= x_max is ``box_constraints``.  Only the solver's public setup / update /
    solve are called, so every solver option (``precision``, ``polish``, ``sensitivity``, ``devices`` ...) works unchanged.

    ``stage_rows=nc`` replaces the box by nc rows per stage, lo_k <= E_k [u_k ; x_{k+1}] <= hi_k (``stage_constraints``;
    u_max and x_max must then be None): ``linearize(Ad, Bd, c=None, E=None)`` takes E [B, N, nc, nu + nx] or shared [N, nc,
    nu + nx] and ``step(x, ..., lo=None, hi=None)`` the bounds [B, N nc] or [N nc]; each is required on first use and kept
    until replaced.  The QPs then have ``m = N nc`` rows (A_c = E F is built on the device, rqp_ltv_stage_rows).

    Stage weights: ``linearize(..., Q=, R=)`` takes Q [B, N, nx, nx] or [N, nx, nx] (Q_k weighs x_{k+1}; Q[..., N-1, :, :] is the
    terminal weight) and / or R [B, N, nu, nu] or [N, nu, nu], numpy or tensors, kept until replaced like E.  Until one is
    given the constructor's shared (Q, R, Qf) apply, on the shared-weight kernels; given only one of them, the other repeats
    the constructor's (Q as Q, ..., Q, Qf).

    Input rates (``rate_constraints``; both act on the plant's input u_k = -K x_k + v_k and start from the input applied before
    stage 0): ``rate_weight=S`` [nu, nu] adds the move-suppression cost 1/2 sum_k (u_k - u_{k-1})' S (u_k - u_{k-1});
    ``linearize(..., S=)`` takes S [B, N, nu, nu], [N, nu, nu] or [nu, nu], kept until replaced.  ``du_max=`` (a scalar or [nu];
    inf: rows whose bounds come later) appends N nu slew-rate rows |u_k - u_{k-1}| <= du_max after the box or the stage rows,
    ``m = m0 + N nu``; ``step(x, ..., du_lo=, du_hi=)`` replaces their bounds ([N nu] or [B, N nu], kept until replaced).
    ``step(..., u_prev=)`` [B, nu] is required on the first step and defaults to the u_0 the previous step returned afterwards.
    With rate rows the base rows are built in a buffer of their own and copied into the larger A, l, u (one strided copy of
    B m0 n entries per ``linearize``, of 2 B m0 per step).  Without any rate argument the driver makes the calls it always made."""

    def __init__(self, nx, nu, horizon, Q, R, Qf, u_max=None, x_max=None, K=None, solver=None, stage_rows=None, rate_weight=None,
                 du_max=None, **solver_kw):
        nx, nu, horizon = int(nx), int(nu), int(horizon)
        _ltv_check_sizes(nx, nu, horizon)
        self.nx, self.nu, self.horizon = nx, nu, horizon
        self.n, self.m = horizon * nu, horizon * (nx + nu)
        self.stage_rows = None if stage_rows is None else int(stage_rows)
        if self.stage_rows is not None:
            if u_max is not None or x_max is not None:
                raise ValueError("stage_rows replaces the box: u_max and x_max must be None (write the box as rows of E)")
            _stage_check_sizes(horizon, self.stage_rows)
            self.m_box, self.m = self.m, horizon * self.stage_rows
            u_max = x_max = 0.0                # (the box vectors only feed the scratch l, u of rqp_ltv_vectors)
        elif u_max is None or x_max is None:
            raise ValueError("u_max and x_max are required without stage_rows")
        self._E = self._lo = self._hi = None
        self._Qs = self._Rs = self._stage_weights = None
        self._S = self._S_dev = self._uprev = self._du_lo = self._du_hi = None
        if rate_weight is not None:
            self._S = np.asarray(rate_weight, dtype=np.float64)
            if self._S.shape != (nu, nu):
                raise ValueError("rate_weight has shape %s, expected (%d, %d) (stage-varying S: linearize(S=))" % (self._S.shape, nu, nu))
            if np.abs(self._S - self._S.T).max() > 1e-9 * max(np.abs(self._S).max(), 1e-300):
                raise ValueError("rate_weight must be symmetric")
        self.m_base, self.rate_rows = self.m, du_max is not None
        if self.rate_rows:
            du = np.asarray(du_max, dtype=np.float64)
            if du.shape not in ((), (nu,)) or np.isnan(du).any() or (du < 0).any():
                raise ValueError("du_max must be a non-negative scalar or [%d]" % nu)
            self._du = np.tile(np.broadcast_to(du, (nu,)), horizon)
            self.m = self.m_base + horizon * nu
            if self.m > LTV_LIMITS["m"]:
                raise ValueError("unsupported size: %d base rows + %d rate rows = %d, the QPs hold m <= %d"
                                 % (self.m_base, horizon * nu, self.m, LTV_LIMITS["m"]))
        self.weights = _LtvWeights(nx, nu, Q, R, Qf, K)
        self.K = self.weights.K
        _, l_add, u_add = box_constraints(nx, nu, horizon, u_max, x_max)
        self.l_add, self.u_add = l_add, u_add
        self.solver, self.solver_kw = solver, dict(solver_kw)
        self._ready = False
        self._lin = None                       # (has_c,) of the current linearisation
        self._buf = None

    def _place(self):
        """(device, dtype) of the tensors the driver builds: the solver's device / precision options."""
        import torch
        kw = self.solver_kw
        dtype = kw.get("precision", torch.float64)
        if kw.get("devices"):
            d = kw["devices"][0]
            device = d if isinstance(d, torch.device) else torch.device("cuda", int(d))
        else:
            device = torch.device(kw.get("device", "cuda:0"))
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device, dtype

    def _buffers(self, B, device, dtype):
        import torch
        if self._buf is None or self._buf["B"] != B:
            e = lambda *s: torch.empty(s, dtype=dtype, device=device)
            self._buf = dict(B=B, ws=ltv_workspace(B, self.nx, self.nu, self.horizon, device), H=e(B, self.n, self.n),
                             A=e(B, self.m, self.n), g=e(B, self.n), l=e(B, self.m), u=e(B, self.m),
                             l_add=torch.as_tensor(self.l_add, dtype=dtype, device=device),
                             u_add=torch.as_tensor(self.u_add, dtype=dtype, device=device),
                             Kt=None if self.K is None else torch.as_tensor(self.K.T.copy(), dtype=dtype, device=device))
            if self.stage_rows is not None:    # what rqp_ltv_condense / rqp_ltv_vectors write besides H and g: A = F, the box l, u
                self._buf.update(A_box=e(B, self.m_box, self.n), l_box=e(B, self.m_box), u_box=e(B, self.m_box))
            if self.rate_rows:                 # the base rows, copied into the head of A, l, u; the rate rows are written in place
                self._buf.update(A_base=e(B, self.m_base, self.n), l_base=e(B, self.m_base), u_base=e(B, self.m_base),
                                 du_lo=torch.as_tensor(-self._du, dtype=dtype, device=device),
                                 du_hi=torch.as_tensor(self._du, dtype=dtype, device=device))
                self._buf["A_rows"], self._buf["l_rows"], self._buf["u_rows"] = (self._buf[k + "_base"] for k in "Alu")
            else:
                self._buf["A_rows"], self._buf["l_rows"], self._buf["u_rows"] = (self._buf[k] for k in "Alu")
        return self._buf

    def _stage_input(self, t, shapes, name, device, dtype):
        import torch
        t = torch.as_tensor(t).to(device=device, dtype=dtype).contiguous()
        if tuple(t.shape) not in shapes:
            raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), " or ".join(str(s) for s in shapes)))
        return t

    def _handover(self, device):
        """devices=[...]: the shards run on their own streams, so what this stream built must be complete first."""
        import torch
        if self.solver_kw.get("devices"):
            torch.cuda.current_stream(device).synchronize()

    def _weights(self):
        return self.weights if self._stage_weights is None else self._stage_weights

    def linearize(self, Ad, Bd, c=None, E=None, Q=None, R=None, S=None):
        """New stage matrices Ad [B, N, nx, nx], Bd [B, N, nx, nu] (c [B, N, nx]): H and A of every instance are rebuilt on the
        device; the solver is set up on the first ``step`` (it needs g, l, u) and re-factored, state kept, afterwards.
        With ``stage_rows``: E [B, N, nc, nu + nx] or [N, nc, nu + nx], kept until replaced.
        Stage weights Q [B, N, nx, nx] or [N, nx, nx], R [B, N, nu, nu] or [N, nu, nu]: kept until replaced.
        Rate weight S [B, N, nu, nu], [N, nu, nu] or [nu, nu]: kept until replaced (before the first one: ``rate_weight``)."""
        import torch
        from reluqp import _cabi
        B, N, nx, nu = _ltv_shapes(Ad, Bd)
        if (N, nx, nu) != (self.horizon, self.nx, self.nu):
            raise ValueError("stages of shape (N=%d, nx=%d, nu=%d), expected (%d, %d, %d)" % (N, nx, nu, self.horizon, self.nx, self.nu))
        if c is not None and tuple(c.shape) != (B, N, nx):
            raise ValueError("c has shape %s, expected %s" % (tuple(c.shape), (B, N, nx)))
        nc = self.stage_rows
        if nc is None and E is not None:
            raise ValueError("E needs BatchedLTVMPC(stage_rows=nc)")
        if nc is not None:
            if E is None and self._E is None:
                raise ValueError("stage_rows: the first linearize() needs E")
            if E is not None:
                blk = nx + nu
                if tuple(E.shape) not in ((B, N, nc, blk), (N, nc, blk)):
                    raise ValueError("E has shape %s, expected %s or %s" % (tuple(E.shape), (B, N, nc, blk), (N, nc, blk)))
            elif self._E.dim() == 4 and self._E.shape[0] != B:
                raise ValueError("the kept E is for a batch of %d, the stages for %d" % (self._E.shape[0], B))
        if Q is not None or R is not None:
            for name, W, d in (("Q", Q, nx), ("R", R, nu)):
                if W is not None and tuple(W.shape) not in ((B, N, d, d), (N, d, d)):
                    raise ValueError("%s has shape %s, expected %s or %s" % (name, tuple(W.shape), (B, N, d, d), (N, d, d)))
            Qs, Rs = (self._Qs if Q is None else Q), (self._Rs if R is None else R)
            w = self.weights                   # a weight never given repeats the constructor's shared one
            self._stage_weights = _LtvStageWeights(nx, nu, N, w.Q if Qs is None else Qs, w.R if Rs is None else Rs,
                                                   w.Qf if Qs is None else None, self.K)
            self._Qs, self._Rs = Qs, Rs
        if self._stage_weights is not None and self._stage_weights.batch not in (None, B):
            raise ValueError("the kept stage weights are for a batch of %d, the stages for %d" % (self._stage_weights.batch, B))
        if S is not None and tuple(S.shape) not in ((B, N, nu, nu), (N, nu, nu), (nu, nu)):
            raise ValueError("S has shape %s, expected %s, %s or %s" % (tuple(S.shape), (B, N, nu, nu), (N, nu, nu), (nu, nu)))
        if S is None and self._S is not None and len(self._S.shape) == 4 and self._S.shape[0] != B:
            raise ValueError("the kept rate weight is for a batch of %d, the stages for %d" % (self._S.shape[0], B))
        if not torch.cuda.is_available():
            raise _cabi.RqpUnavailable("BatchedLTVMPC needs a HIP device; the MI355X build has no CPU path")
        device, dtype = self._place()
        buf = self._buffers(B, device, dtype)
        to = lambda t: torch.as_tensor(t).to(device=device, dtype=dtype)
        if S is not None:
            self._S, self._S_dev = S, None
        if self._S is not None and (self._S_dev is None or self._S_dev.shape[0] != B):
            self._S_dev = rate_weight_device(self._S, nu, N, B, device)
        condense_ltv_device(to(Ad), to(Bd), self._weights(), buf["ws"], c=None if c is None else to(c), H=buf["H"],
                            A=buf["A_rows"] if nc is None else buf["A_box"], S=self._S_dev)
        if nc is not None:
            if E is not None:
                self._E = to(E).contiguous()
            stage_rows_device((B, nx, nu, N), self._E, buf["ws"], A_c=buf["A_rows"])
        if self.rate_rows:
            buf["A"][:, :self.m_base].copy_(buf["A_base"])
            rate_rows_device((B, nx, nu, N), buf["ws"], dtype, A_r=buf["A"], row0=self.m_base)
        self._lin = (c is not None,)
        if self._ready:
            self._handover(device)
            self.solver.update(Hx=buf["H"], Ax=buf["A"])
        return None

    def qp_vectors(self, x, xref=None, uref=None, lo=None, hi=None, u_prev=None, du_lo=None, du_hi=None):
        """(g, l, u) device tensors of the QPs for the states x [B, nx] under the current linearisation (``stage_rows``: with
        the bounds lo, hi [B, N nc] or [N nc], kept until replaced; input rates: with u_prev [B, nu] and the rate bounds
        du_lo, du_hi [B, N nu] or [N nu], kept until replaced)."""
        import torch
        rate = self._S is not None or self.rate_rows
        if not rate and (u_prev is not None or du_lo is not None or du_hi is not None):
            raise ValueError("u_prev, du_lo, du_hi need BatchedLTVMPC(rate_weight=) / (du_max=) or linearize(S=)")
        if not self.rate_rows and (du_lo is not None or du_hi is not None):
            raise ValueError("du_lo, du_hi need BatchedLTVMPC(du_max=) (du_max=inf: rows whose bounds are given here)")
        if rate and u_prev is None and self._uprev is None:
            raise ValueError("input rates: the first step() needs u_prev")
        if self.stage_rows is not None and ((lo is None and self._lo is None) or (hi is None and self._hi is None)):
            raise ValueError("stage_rows: the first step() needs lo and hi")
        if self._lin is None:
            raise RuntimeError("BatchedLTVMPC: linearize() first")
        device, dtype = self._place()
        buf = self._buf
        to = lambda t: None if t is None else torch.as_tensor(t).to(device=device, dtype=dtype)
        x = to(x)
        if tuple(x.shape) != (buf["B"], self.nx):
            raise ValueError("x has shape %s, expected %s" % (tuple(x.shape), (buf["B"], self.nx)))
        nc = self.stage_rows
        if nc is None and (lo is not None or hi is not None):
            raise ValueError("lo, hi need BatchedLTVMPC(stage_rows=nc)")
        if rate:
            if u_prev is not None:
                self._uprev = self._stage_input(u_prev, ((buf["B"], self.nu),), "u_prev", device, dtype)
            elif tuple(self._uprev.shape) != (buf["B"], self.nu):
                raise ValueError("the kept u_prev is for a batch of %d, the states for %d" % (self._uprev.shape[0], buf["B"]))
            for name, t in (("du_lo", du_lo), ("du_hi", du_hi)):
                if t is not None:
                    setattr(self, "_" + name, self._stage_input(t, ((buf["B"], self.n), (self.n,)), name, device, dtype))
        rate_kw = dict(S=self._S_dev, uprev=self._uprev) if self._S is not None else {}
        if nc is None:
            g, l, u = ltv_vectors_device((self.nx, self.nu, self.horizon, self.K is not None, self._lin[0]), x, buf["l_add"],
                                         buf["u_add"], self._weights(), buf["ws"], xref=to(xref), uref=to(uref), g=buf["g"],
                                         l=buf["l_rows"], u=buf["u_rows"], **rate_kw)
        else:
            for name, t in (("lo", lo), ("hi", hi)):
                if t is not None:
                    setattr(self, "_" + name, self._stage_input(t, ((buf["B"], self.m_base), (self.m_base,)), name, device, dtype))
            if self._lo.dim() != self._hi.dim():
                raise ValueError("lo and hi must both be [B, N nc] or both [N nc]")
            g, _, _ = ltv_vectors_device((self.nx, self.nu, self.horizon, self.K is not None, self._lin[0]), x, buf["l_add"],
                                         buf["u_add"], self._weights(), buf["ws"], xref=to(xref), uref=to(uref), g=buf["g"],
                                         l=buf["l_box"], u=buf["u_box"], **rate_kw)
            l, u = stage_vectors_device((buf["B"], self.nx, self.nu, self.horizon), self._E, x, self._lo, self._hi, buf["ws"],
                                        l_c=buf["l_rows"], u_c=buf["u_rows"])
        if self.rate_rows:
            dlo, dhi = (buf["du_lo"] if self._du_lo is None else self._du_lo), (buf["du_hi"] if self._du_hi is None else self._du_hi)
            if dlo.dim() != dhi.dim():
                raise ValueError("du_lo and du_hi must both be [B, N nu] or both [N nu]")
            buf["l"][:, :self.m_base].copy_(buf["l_base"])
            buf["u"][:, :self.m_base].copy_(buf["u_base"])
            l, u = rate_bounds_device((buf["B"], self.nx, self.nu, self.horizon), x, self._uprev, dlo, dhi, buf["ws"], l_r=buf["l"],
                                      u_r=buf["u"], row0=self.m_base)
        return g, l, u

    def step(self, x, xref=None, uref=None, lo=None, hi=None, u_prev=None, du_lo=None, du_hi=None):
        """One control step for the states x [B, nx] (references xref [B, N, nx] for x_1 .. x_N, uref [B, N, nu]; with
        ``stage_rows`` the bounds lo, hi; with input rates u_prev [B, nu], required on the first step, afterwards the u_0 the
        previous step returned unless given, and the rate bounds du_lo, du_hi): returns (u_0 [B, nu] device tensor, Results)."""
        import torch
        g, l, u = self.qp_vectors(x, xref, uref, lo, hi, u_prev, du_lo, du_hi)
        device, dtype = self._place()
        buf = self._buf
        self._handover(device)
        if not self._ready:
            import reluqp.reluqpth as reluqpth
            self.solver = self.solver or reluqpth.ReLU_QP()
            kw = dict(self.solver_kw)
            if not kw.get("devices"):
                kw["device"] = device
            self.solver.setup(buf["H"], g, buf["A"], l, u, **kw)
            self._ready = True
        else:
            self.solver.update(g=g, l=l, u=u)
        res = self.solver.solve()
        v0 = res.x[:, :self.nu].to(device)
        x = torch.as_tensor(x).to(device=device, dtype=dtype)
        u0 = v0.clone() if buf["Kt"] is None else v0 - x @ buf["Kt"]      # (never a view of the solver's result buffer)
        if self._S is not None or self.rate_rows:
            self._uprev = u0.detach().clone()  # the next step's u_{-1} (the caller may change u0)
        return u0, res

    def simulate(self, x0, steps, plant, relinearize_every=1, xref=None, uref=None, u_prev=None):
        """Closed loop on the device: ``plant(x, u) -> (x_next, Ad, Bd, c)`` is a torch callable returning the next states and
        the linearisation to use from them (Ad [B, N, nx, nx], Bd [B, N, nx, nu], c [B, N, nx] or None).  The linearisation
        is refreshed every ``relinearize_every`` steps; ``linearize()`` must have been called for the first one.
        Input rates: ``u_prev`` [B, nu] is the input applied before the first step; every later step starts from the one before.
        Returns (states [steps + 1, B, nx], inputs [steps, B, nu], iterations [steps, B]) as device tensors."""
        import torch
        device, dtype = self._place()
        x = torch.as_tensor(x0).to(device=device, dtype=dtype)
        xs, us, its = [x], [], []
        for k in range(steps):
            u0, res = self.step(x, xref=xref, uref=uref, u_prev=u_prev if k == 0 else None)
            x, Ad, Bd, c = plant(x, u0)
            if (k + 1) % relinearize_every == 0 and k + 1 < steps:
                self.linearize(Ad, Bd, c)
            xs.append(x)
            us.append(u0)
            its.append(res.info.iter.to(device).clone())
        return torch.stack(xs), torch.stack(us), torch.stack(its)
