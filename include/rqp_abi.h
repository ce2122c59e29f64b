/*
 * rqp_abi.h -- C ABI of librqp_hip.so, the MI355X (gfx950) ReLU-QP hot path.
 *
 * The reference (gstoica27/ReLUQP-py) has NO foreign-function interface: its hot
 * path is the Python class reluqp.reluqpth.ReLU_QP calling torch.  This header is
 * therefore the boundary a maintainer would bind *under* that class (ctypes stub in
 * INTEGRATION.md); each entry point names the reference method it replaces
 * (paths relative to /root/reference/ReLU-QP-py/reluqp/).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / C++ types cross the ABI.
 *  - Every `const void*` / `void*` data pointer is a DEVICE pointer (e.g.
 *    torch.Tensor.data_ptr()) of element type `dims.dtype` unless stated; the caller
 *    owns all of them.  The library owns only its workspace (packed H/A copies, the
 *    K(rho) table, per-instance ADMM state), allocated in rqp_setup, freed in
 *    rqp_destroy.
 *  - `stream` is a hipStream_t passed as void* (0 = default stream).  All work is
 *    enqueued on it; nothing synchronises the host except where stated.
 *  - Every function returns 0 on success or a negative rqp_error; nothing throws.
 *  - A handle is not thread-safe: one handle per host thread / GPU.
 *  - Batched: every instance b in [0,batch) has its own g,l,u, state, rho index,
 *    iteration count and exit; H and A are per instance, or shared by all instances
 *    (dims.shared_mats = 1, then H is [n,n] and A is [m,n]).
 */
#ifndef RQP_ABI_H
#define RQP_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rqp_handle rqp_handle;

enum rqp_dtype { RQP_F32 = 0, RQP_F64 = 1 };

/* Storage type of the preconditioner tile K_j in the register-resident kernels (BASELINE
 * config 5, SURVEY.md 7.3 "matrix tile fp16, x/z/lam and residual fp32").  K only
 * preconditions the residual correction dx = -K d: its rounding
 * changes the convergence rate, never the fixed point; H, A and every residual stay in
 * dims.dtype.  RQP_TILE_F16 needs dims.dtype == RQP_F32.  The MFMA kernel (shared H, A)
 * takes the same fp16-rounded K into its float32 operand image.                        */
enum rqp_tile_dtype {
    RQP_TILE_SAME = 0,
    RQP_TILE_F16 = 1,
    /* Shared-(H, A) batches on the MFMA kernel: every matrix tile ([A; H'], A, K_j) and every vector operand is kept as two
     * bf16 planes (hi + mid = 16 significant bits) and every product runs as three v_mfma_f32_16x16x32_bf16 with float32
     * accumulation -- the 16-bit matrix pipe (16x the float32 MFMA rate); state, residuals and the checks stay float32.
     * Same recurrence as the float32 kernel; operand error 2^-16 relative (stated tolerance: eps_abs >= 1e-5).  Needs
     * dims.dtype == RQP_F32, shared_mats, n <= 80, m <= 320 (the MFMA kernel's shapes).                                     */
    RQP_TILE_BF16 = 2
};

/* Solve-kernel request (rqp_dims.kernel).  AUTO = measured dispatch by size / batch /
 * sharing; an explicit kernel that cannot hold the problem makes rqp_setup return
 * RQP_ERR_UNSUPPORTED (nothing falls back silently).                                    */
enum rqp_kernel {
    RQP_KERNEL_AUTO = 0,
    RQP_KERNEL_GENERIC = 1,   /* streaming, any n, m, f32/f64                              */
    RQP_KERNEL_RESIDENT = 2,  /* A, K in VGPRs, one workgroup per instance (f32; f64 tile) */
    RQP_KERNEL_WAVE = 3,      /* one wavefront per instance, small problems                */
    RQP_KERNEL_MFMA = 4       /* shared (H, A), f32: batch on the MFMA N axis -- operands in registers (n <= 80,
                               * m <= 320), else streamed from L2 as non-zero 16 x 16 blocks (n <= 320, m <= 640);
                               * f64: streamed operands on v_mfma_f64_16x16x4_f64 (n <= 160, m <= 320)              */
};

enum rqp_error {
    RQP_OK = 0,
    RQP_ERR_ARG = -1,        /* null pointer / bad dimension / bad setting       */
    RQP_ERR_STATE = -2,      /* call order (e.g. solve before setup)             */
    RQP_ERR_HIP = -3,        /* a HIP runtime call failed: see rqp_last_error    */
    RQP_ERR_OOM = -4,        /* workspace allocation failed                      */
    RQP_ERR_UNSUPPORTED = -5 /* size / mode no kernel of this build covers        */
};

/* per-instance exit status written to rqp_info.status (reluqpth.py:236,245) */
enum rqp_status {
    RQP_STATUS_SOLVED = 0,          /* "solved"             */
    RQP_STATUS_MAX_ITER = 1,        /* "max_iters_reached"  */
    RQP_STATUS_NAN = 2,             /* "nan_detected": a residual of the last check is NaN (Q17 made visible;
                                       only raised when the iteration budget is spent -- the loop control is
                                       the reference's)                                                        */
    RQP_STATUS_PRIMAL_INFEASIBLE = 3, /* "primal_infeasible": certificate found (check_infeasibility)          */
    RQP_STATUS_DUAL_INFEASIBLE = 4,   /* "dual_infeasible"                                                     */
    RQP_STATUS_WINDOW_PASSES = 5,   /* "window_passes_exhausted": a windowed handle under rqp_set_window_passes(P >= 1)
                                       whose instance still waited for a re-window after the last of the P passes.
                                       x, z, lam are its exact state at the stop, iter the iterations run so far,
                                       rho_ind / rho_estimate as at the stop; pri_res, dua_res, obj_val are NaN (not
                                       evaluated).  The next solve continues it like any other instance.           */
    RQP_STATUS_UNSOLVED = -1        /* never solved          */
};

typedef struct rqp_dims {
    int32_t n;            /* decision variables   (QP.nx, classes.py:29)              */
    int32_t m;            /* constraints          (QP.nc, classes.py:30)              */
    int32_t batch;        /* independent instances (>= 1)                             */
    int32_t shared_mats;  /* 1: one (H, A) shared by all instances (linear MPC)       */
    int32_t dtype;        /* rqp_dtype of every data pointer                          */
    int32_t kernel;       /* rqp_kernel request (0 = auto)                            */
    int32_t tile_dtype;   /* rqp_tile_dtype of the resident K tile (0 = same as dtype) */
    int32_t flags;        /* RQP_FLAG_* bits (0 = defaults)                           */
} rqp_dims;

/* rqp_dims.flags */
enum {
    RQP_FLAG_LOW_MEMORY = 1,  /* resident float32 kernel: keep K(rho) as the row-major table (n x ldn per entry) and load it
                                 from there, instead of the larger lane-linear register image (padded to the kernel's tile):
                                 less workspace for ~1 % more solve time; results are bit-identical.  (A windowed handle
                                 holds ONE of the two: by default the factor kernel writes the register image directly.)  */
    RQP_FLAG_FULL_LADDER = 2  /* build K(rho) for EVERY entry of the rho ladder of every matrix, as the reference does
                                 (reluqpth.py:52-78).  Default for batches of >= 32 per-instance matrices on the resident
                                 float32 / streaming kernels: a WINDOW of 5 entries around each instance's index
                                 (rho_ind0 - 1 .. rho_ind0 + 3 at setup; a solve visits 2-4 entries).  An instance whose
                                 index leaves its window exits with its exact state, rqp_solve re-factors a window around
                                 the new index and continues it -- results are bit-identical to the full ladder, setup and
                                 workspace shrink by ~3x, and rqp_solve synchronises `stream` once per pass (it cannot be
                                 captured into a HIP graph: use this flag there, or rqp_set_window_passes).          */
};

/* Settings of classes.py:32-65 that reach the device (same names, same defaults). */
typedef struct rqp_settings {
    double rho;                    /* 0.1   */
    double rho_min;                /* 1e-6  */
    double rho_max;                /* 1e6   */
    double sigma;                  /* 1e-6  */
    double adaptive_rho_tolerance; /* 5     */
    double eps_abs;                /* 1e-3  */
    double eq_tol;                 /* 1e-6  */
    int32_t adaptive_rho;          /* 1     */
    int32_t max_iter;              /* 4000  */
    int32_t check_interval;        /* 25    */
    int32_t warm_starting;         /* 1     */
    /* --- extensions (all default to the reference's behaviour) --- */
    double eps_rel;                /* 0: absolute test only (reluqpth.py:233).  > 0: OSQP-style
                                      pri < eps_abs*sqrt(m) + eps_rel*max(|Ax|,|z|),
                                      dua < eps_abs*sqrt(n) + eps_rel*max(|Hx|,|A'lam|,|g|)  (inf-norms)   */
    double eps_prim_inf;           /* 1e-4  certificate tolerances (check_infeasibility)                    */
    double eps_dual_inf;           /* 1e-4  */
    int32_t scaling;               /* 0: none (the reference's `scaling` is an unused TODO, reluqpth.py:105);
                                      k > 0: k Ruiz equilibration passes at setup; results, residuals and the
                                      termination test in the caller's (un-scaled) units                       */
    int32_t check_infeasibility;   /* 0.  1: OSQP's primal / dual infeasibility certificates.  The streaming kernel
                                      (RQP_KERNEL_GENERIC) tests them at every check and exits at the first one that
                                      holds; the register-resident / wavefront / MFMA kernels keep their loops
                                      untouched: an instance that spends max_iter (or ends nan_detected) is examined
                                      once, after the launch, and labelled -- it has then run its whole budget.
                                      AUTO therefore dispatches a handle with this option to the streaming kernel;
                                      the other kernels take it on explicit request only.                          */
} rqp_settings;

/* Per-instance results of one solve (classes.py:67-88), struct of DEVICE arrays,
 * each of length `batch`; any pointer may be NULL to skip that field.           */
typedef struct rqp_info {
    int32_t* iter;         /* Info.iter                                             */
    int32_t* status;       /* rqp_status                                            */
    int32_t* rho_ind;      /* rho index after the solve (ReLU_QP.rho_ind)           */
    double* pri_res;       /* Info.pri_res                                          */
    double* dua_res;       /* Info.dua_res                                          */
    double* rho_estimate;  /* Info.rho_estimate                                     */
    double* obj_val;       /* Info.obj_val = 1/2 x'Hx + g'x   (reluqpth.py:320-322)  */
    /* optional per-check trace, [batch][trace_cap][4] doubles:
     * (pri, dua, rho_estimate, rho index before the move), check c = iteration
     * (c+1)*check_interval; rows past the last check are left untouched.         */
    double* trace;
    int32_t trace_cap;
    int32_t reserved;
} rqp_info;

/* Fill *s with the defaults of classes.py:32-65. */
int rqp_default_settings(rqp_settings* s);

/* ReLU_QP.__init__ + Settings (reluqpth.py:93-100,128-142): validates dims and
 * settings, builds the rho ladder (setup_rhos, reluqpth.py:20-38) and binds `device`. */
int rqp_create(rqp_handle** out, const rqp_dims* dims, const rqp_settings* settings, int device);

/* ReLU_QP.setup (reluqpth.py:102-157): QP.__init__ casts (classes.py:4-30), the
 * per-rho KKT inverses of ReLU_Layer.setup_matrices (reluqpth.py:40-78; here
 * K_j = (H + sigma I + A' diag(rho_j c) A)^-1 for every ladder entry, c_i = 1e3 on
 * rows with u_i - l_i <= eq_tol), zero state and rho_ind = argmin|rhos - rho|.
 * H [batch|1][n][n], g [batch][n], A [batch|1][m][n], l,u [batch][m], row-major.
 * The inputs are read by kernels enqueued on `stream` (every one of them more than once:
 * some handles keep no copy of A and build A'cA and the register image of A straight from
 * the caller's buffer): they must stay valid and unchanged until that work has completed,
 * like the operands of any stream-ordered call.  Nothing is read after that.           */
int rqp_setup(rqp_handle* h, const void* H, const void* g, const void* A, const void* l,
              const void* u, void* stream);

/* ReLU_QP.update (reluqpth.py:159-183): new g and/or l and/or u ([batch][n] /
 * [batch][m]); NULL = unchanged.  State is untouched.                           */
int rqp_update(rqp_handle* h, const void* g, const void* l, const void* u, void* stream);

/* ReLU_QP.update(Hx=, Ax=) -- rejected upstream (`assert`, reluqpth.py:176-177), SURVEY.md
 * 8(f)-4: new H and/or A (same shapes as in rqp_setup; NULL = unchanged).  Re-runs the
 * device setup chain (pack -> A'cA -> K(rho) ladder -> kernel images) on the existing
 * workspace; g, l, u, the equality pattern c, the ADMM state and the rho indices are kept,
 * i.e. the next solve is warm-started exactly like after rqp_update.  With
 * settings.scaling > 0 BOTH raw matrices must be given (the packed copies are scaled):
 * the problem is re-equilibrated and the stored vectors and state move to the new scaled
 * space (the call then synchronises `stream`).                                           */
int rqp_update_mats(rqp_handle* h, const void* H, const void* A, void* stream);

/* Parametric form of ReLU_QP.update for linear MPC (the x0 update of the reference's driver,
 * loose_code/RandomLinMPC.py / SURVEY.md Appendix C, evaluated on the device in one pass):
 *   g[b] = Gg p[b],   l[b] = l0 + Glu p[b],   u[b] = u0 + Glu p[b]
 * p [batch][np] (np <= 64), Gg [n][np], Glu [m][np], l0/u0 [m], all device pointers in the
 * handle's dtype.  Same effect as rqp_update with those vectors; state is untouched.       */
int rqp_update_affine(rqp_handle* h, const void* p, int32_t np, const void* Gg, const void* Glu,
                      const void* l0, const void* u0, void* stream);

/* ReLU_QP.update_settings (reluqpth.py:185-199, whose whitelist is max_iter, eps_abs, verbose,
 * check_interval).  Changeable after setup: max_iter, eps_abs, check_interval, warm_starting and
 * the extension fields eps_rel, check_infeasibility, eps_prim_inf, eps_dual_inf.  A difference in
 * any other field (rho, rho_min, rho_max, sigma, adaptive_rho, adaptive_rho_tolerance, eq_tol,
 * scaling -- they shape the K(rho) ladder built at setup) returns RQP_ERR_ARG (the reference
 * raises ValueError).                                                                          */
int rqp_update_settings(rqp_handle* h, const rqp_settings* settings);

/* ReLU_QP.warm_start (reluqpth.py:251-276) with Q6 fixed (values are written into
 * the iterate).  x [batch][n], z, lam [batch][m]; NULL = unchanged.  `rho` selects
 * rho_ind = argmin|rhos - rho| for every instance when has_rho != 0.              */
int rqp_warm_start(rqp_handle* h, const void* x, const void* z, const void* lam, int has_rho,
                   double rho, void* stream);

/* ReLU_QP.clear_primal_dual (reluqpth.py:324-333): zero state, reset rho index.  */
int rqp_clear_primal_dual(rqp_handle* h, void* stream);

/* ReLU_QP.solve + update_results (reluqpth.py:201-249,278-305): the whole ADMM
 * loop of every instance -- iterate (jit_forward :84-89), every check_interval
 * iterations compute_residuals (:307-318), rho-index move (:223-227), termination
 * (:233) -- in ONE kernel launch, one workgroup (or wavefront, or MFMA column) per
 * instance, no host round trip.  Small follow-up launches on the same stream where
 * they apply: the dispatch-order ranking for the next solve, the straggler pass of a
 * shared-matrix batch, the certificate pass (check_infeasibility), the un-scaling.
 * Writes x [batch][n], z [batch][m], lam [batch][m] (the state's dual, Q7/Q16) and
 * *info; any of them may be NULL.  Asynchronous on `stream`.                      */
int rqp_solve(rqp_handle* h, void* x, void* z, void* lam, const rqp_info* info, void* stream);

/* k plain iterations at each instance's current rho index, no checks: exactly k
 * applications of ReLU_Layer.forward (reluqpth.py:80-89).  For parity tests.     */
int rqp_iterate(rqp_handle* h, int32_t k, void* stream);

/* ReLU_QP.compute_residuals + compute_J (reluqpth.py:307-322) on the current
 * state with carried estimate rho_in (host scalar): pri, dua, rho_out, obj are
 * device arrays [batch] of doubles (NULL to skip).                               */
int rqp_compute_residuals(rqp_handle* h, double rho_in, double* pri, double* dua,
                          double* rho_out, double* obj, void* stream);

/* Copy the current state out (x [batch][n], z, lam [batch][m] in dims.dtype,
 * rho_ind [batch] int32); NULL to skip.                                           */
int rqp_get_state(rqp_handle* h, void* x, void* z, void* lam, int32_t* rho_ind, void* stream);

/* The rho ladder (host doubles).  *count receives its length; rhos may be NULL.  */
int rqp_get_rhos(const rqp_handle* h, double* rhos, int32_t cap, int32_t* count);

/* K_j of instance b (ReLU_Layer.kkt_rhs_invs[j], reluqpth.py:56) -> out [n][n]
 * in dims.dtype (device pointer).  For parity tests.                              */
int rqp_get_K(rqp_handle* h, int32_t b, int32_t j, void* out, void* stream);

/* Dispatch order of the per-instance kernels.  After every solve the library ranks the instances by
 * the iteration count they just needed and issues the next launch longest-first (pure scheduling:
 * results never depend on it; it pays when consecutive solves resemble each other -- closed loops,
 * parameter sweeps).  mode 1 = on (default), 0 = off: every launch in grid order, nothing recorded
 * (a handle then behaves at every solve like a fresh handle on a fresh batch), 2 = forget the
 * recorded order now and stay on.  No reference counterpart (one QP per object there).            */
int rqp_dispatch_history(rqp_handle* h, int32_t mode);

/* Inspection hook for the tests: the workgroup -> instance permutation the NEXT launch would use and the
 * iteration counts it was ranked by (device arrays [batch] of int32, NULL to skip).  *valid (host)
 * receives 1 when a recorded order exists, else 0 (then nothing is copied).                       */
int rqp_get_dispatch(rqp_handle* h, int32_t* order, int32_t* last_iter, int32_t* valid, void* stream);

/* K(rho) slots per matrix of this handle: *slots = the ladder length (whole ladder) or the window size
 * (see RQP_FLAG_FULL_LADDER); wbase (device int32 [batch], NULL to skip; windowed handles only) receives the
 * ladder index of slot 0 of every instance's window.  For tests.                                        */
int rqp_get_window(rqp_handle* h, int32_t* slots, int32_t* wbase, void* stream);

/* Fixed-pass window protocol of a windowed handle (see RQP_FLAG_FULL_LADDER).  passes = 0 (default): rqp_solve
 * reads the count of instances that left their window after every pass and synchronises `stream`; it refuses
 * HIP-graph capture (RQP_ERR_UNSUPPORTED).  passes = P >= 1: rqp_solve enqueues the first launch, then P
 * continuation passes (re-window, re-factor of the moved windows, continuation launch), then a finalize kernel --
 * one fixed, data-independent chain on `stream` with no host read-back, so it can be captured; a pass with
 * nothing to continue exits in every kernel after one load of the pass count.  Results are bit-identical to
 * passes = 0 whenever P is at least the number of passes the solve needs; an instance still waiting after pass P
 * reports RQP_STATUS_WINDOW_PASSES.  A pass count that never runs out: the rho index moves by at most one entry
 * per check and a re-centred window [ri - 2, ri + 2] (clipped to the ladder) is left after >= 3 moves, plus one
 * pass for an instance that enters the solve outside its window:
 *     P = 1 + ceil(floor(max_iter / check_interval) / 3)        (55 for the defaults 4000 / 25)
 * Call after rqp_create or rqp_setup, outside any capture.  Accepted and without effect on handles that are not
 * windowed (they are capturable as they are).  h == NULL or passes < 0: RQP_ERR_ARG.                        */
int rqp_set_window_passes(rqp_handle* h, int32_t passes);

/* OSQP-style solution polishing (OSQP settings polish, delta, polish_refine_iter; defaults 0, 1e-6, 3).  After the ADMM
 * loop, every instance whose exit is RQP_STATUS_SOLVED guesses its active set from the final iterate (z, lam) in the space
 * the kernels iterate in -- lower-active: z_i - l_i < -lam_i; upper-active: u_i - z_i < lam_i (rows not lower-active) --
 * solves the reduced KKT system [[H + delta I, A_a'], [A_a, -delta I]] [x; y_a] = [-g; b_a] (b_i = l_i / u_i), runs
 * refine_iter steps of iterative refinement against [[H, A_a'], [A_a, 0]], and forms z = clip(A x, l, u) and y = y_a on the
 * active rows (0 elsewhere) projected onto the sign cone of its row (<= 0 lower, >= 0 upper, free where l_i == u_i).
 * pri_res, dua_res and obj_val of that point are evaluated in float64 in the caller's units; it is ACCEPTED (status_polish
 * 1) when both residuals are below the ADMM ones, or one is and the other ADMM residual is already < 1e-10 (OSQP's rule):
 * x, z, lam and info pri_res, dua_res, obj_val are then replaced.  Otherwise status_polish = -1 and every output is the
 * ADMM one bit for bit; instances not solved report 0.  iter, status, rho_ind, rho_estimate and the handle's ADMM state
 * (rqp_get_state, the next warm start) never change.  float64 for every dtype / tile_dtype.
 * Call before rqp_setup to reserve the workspace (per-instance float64 A' diag(w) A and M^-1, processed in chunks of at
 * most 1 GiB; a windowed float32 handle then keeps its row-major copy of A).  After setup it switches polish on or off,
 * and changes delta / refine_iter, only on a handle set up with it (else RQP_ERR_STATE).  delta <= 0 or refine_iter < 0:
 * RQP_ERR_ARG.  Synchronous; not callable during a stream capture.  A polished solve is as capturable as a plain one; the
 * captured chain holds enable, delta and refine_iter as they were at capture: recapture after changing them.            */
int rqp_set_polish(rqp_handle* h, int32_t enable, double delta, int32_t refine_iter);

/* Polish results of the last rqp_solve, copied (asynchronously, on `stream`) into DEVICE arrays; either may be NULL:
 * status_polish [batch] int32: 1 accepted, -1 rejected, 0 not attempted (instance not solved, or polish switched off);
 * active [batch][m] int8: -1 lower-active, +1 upper-active, 0 inactive (0 on instances not attempted).
 * RQP_ERR_STATE on a handle not set up with polish.                                                                      */
int rqp_get_polish(rqp_handle* h, int32_t* status_polish, int8_t* active, void* stream);

/* Adjoint of a solve (reverse-mode derivatives; DESIGN.md section 5 "Adjoint (autograd)").  At a solution with
 * sym(H) x + g + A' y = 0, active set a (rows A_a on bounds b_a) and incoming dL/dx = dx, dL/dy = dy, it solves
 *     [[sym(H), A_a'], [A_a, 0]] [rx; ry_a] = -[dx; dy_a]
 * (regularised by delta and eliminated like polish, then refine_iter steps of iterative refinement against this system) and
 * returns dg = rx;  dl_i = -ry_i on lower-active rows, du_i = -ry_i on upper-active rows (0 elsewhere);
 * dH = (rx x' + x rx') / 2;  dA = ybar rx' + ry x'  (ybar = y on active rows, 0 elsewhere; ry = 0 off the active set).
 * An equality row (l_i == u_i) gives its gradient to the bound the sign of y names (the one-sided derivative).  A degenerate
 * active set (more than n rows, or dependent rows) has no unique multipliers: the result is the solution of the
 * delta-regularised system, and adj_res shows how far it is from solving the unregularised one.
 * Every pointer is a DEVICE pointer in dims.dtype unless typed otherwise; arithmetic is float64.                             */
typedef struct rqp_adjoint_io {
    const void *H, *A;           /* the caller's matrices, shapes and layout as in rqp_setup ([n][n] / [m][n] when shared) */
    const void *l, *u;           /* [batch][m]                                                                           */
    const void *x, *z, *y;       /* the solution to differentiate at: [batch][n], [batch][m], [batch][m]                 */
    const int32_t* status;       /* [batch] rqp_status of that solve, NULL = all treated as solved                        */
    const int8_t* active;        /* [batch][m] -1 / 0 / +1, NULL = classified from (z, y, l, u) with polish's rule        */
    const void *dx, *dy;         /* dL/dx [batch][n] (required), dL/dy [batch][m] or NULL                                 */
    void *dH, *dg, *dA, *dl, *du;/* outputs in dims.dtype, NULL to skip; dH, dA summed over the batch on shared handles    */
    int8_t* active_out;          /* [batch][m] the set used, NULL to skip                                                 */
    int32_t* adj_status;         /* [batch] 1 computed, 0 skipped (status != solved: every gradient of it is 0)           */
    double* adj_res;             /* [batch] relative residual of the refined adjoint system (NaN when skipped)            */
} rqp_adjoint_io;

/* Reserve (before rqp_setup) the adjoint's workspace: the caller's sym(H) and A packed to the handle's row pitch, float64
 * A_a' A_a and M^-1 = (sym(H) + delta I + A_a' A_a / delta)^-1 for chunks of the batch (polish's buffers when polish is
 * reserved too), and four float64 rows per instance.  Handles without it allocate nothing for the adjoint.  After setup the
 * call only changes delta and refine_iter (defaults 1e-6, 3), on a handle set up with it (else RQP_ERR_STATE).  delta <= 0 or
 * refine_iter < 0: RQP_ERR_ARG.  Synchronous; not callable during a stream capture.                                          */
int rqp_set_adjoint(rqp_handle* h, int32_t enable, double delta, int32_t refine_iter);

/* Differentiate a solve of this handle's shape at the caller's data (io): nothing of the handle's state is read -- not its
 * packed (possibly Ruiz-scaled) matrices, not its vectors, not its rho window -- so any earlier solve of any handle of the
 * same dims can be differentiated, and several of them by successive calls.  A fixed, data-independent chain of launches on
 * `stream` (pack, masked gram, factor, k_adjoint per chunk; then the matrix gradients: a streaming outer-product kernel for
 * per-instance matrices, a float64-MFMA reduction over the batch in a fixed order for shared ones -- bitwise reproducible);
 * capturable in a HIP graph.  RQP_ERR_ARG: h, io, io->dx, x, y, H or A NULL, or z, l or u NULL without io->active.
 * RQP_ERR_STATE: the handle is not set up, or was set up without rqp_set_adjoint.                                            */
int rqp_adjoint(rqp_handle* h, const rqp_adjoint_io* io, void* stream);

/* Forward-mode sensitivities of a solve (JVPs; DESIGN.md section 5 "Forward sensitivities").  At a solution with
 * sym(H) x + g + A' y = 0 and active set a (classified and signed as rqp_adjoint does; ybar = y on a, 0 elsewhere), the
 * tangents (dH, dg, dA, dl, du) of the data give, per direction,
 *     [[sym(H), A_a'], [A_a, 0]] [dx; dy_a] = [-(sym(dH) x + dg + dA' ybar);  db_a - dA_a x],   dy = 0 off a,
 *     dz = A dx + dA x,
 * with db_i = dl_i on lower-active rows and du_i on upper-active ones (an equality row takes the bound the sign of y names).
 * The system is the adjoint's, solved the same way (regularised by delta, refine_iter refinement steps; the adjoint's delta
 * and refine_iter, rqp_set_adjoint), for blocks of 16 directions against one M^-1 per instance.  A degenerate active set
 * gives the delta-regularised answer; sens_res shows how far it is from solving the unregularised system.
 * Every array has the direction axis LAST: dg [batch][n][ndir], dl / du [batch][m][ndir], dH [batch][n][n][ndir],
 * dA [batch][m][n][ndir]; a tangent whose bit is set in shared_tangents has no batch axis ([n][ndir], ...) and is used by
 * every instance.  Column j of every output depends on direction j alone: bitwise the same in any ndir.
 * DEVICE pointers in dims.dtype unless typed otherwise; arithmetic is float64.                                              */
#define RQP_SENS_SHARED_DH 1
#define RQP_SENS_SHARED_DG 2
#define RQP_SENS_SHARED_DA 4
#define RQP_SENS_SHARED_DL 8
#define RQP_SENS_SHARED_DU 16
typedef struct rqp_sensitivity_io {
    const void *H, *A;           /* the caller's matrices, shapes and layout as in rqp_setup ([n][n] / [m][n] when shared) */
    const void *l, *u;           /* [batch][m]                                                                           */
    const void *x, *z, *y;       /* the solution to differentiate at: [batch][n], [batch][m], [batch][m]                 */
    const int32_t* status;       /* [batch] rqp_status of that solve, NULL = all treated as solved                        */
    const int8_t* active;        /* [batch][m] -1 / 0 / +1, NULL = classified from (z, y, l, u) with polish's rule        */
    int32_t ndir;                /* directions (>= 1)                                                                     */
    int32_t shared_tangents;     /* RQP_SENS_SHARED_* bits: those tangents have no batch axis                             */
    const void *dH, *dg, *dA, *dl, *du; /* tangents, direction axis last; NULL = zero                                     */
    void *dx;                    /* [batch][n][ndir] output (required)                                                   */
    void *dy, *dz;               /* [batch][m][ndir] outputs, NULL to skip                                               */
    int8_t* active_out;          /* [batch][m] the set used, NULL to skip                                                 */
    int32_t* sens_status;        /* [batch] 1 computed, 0 skipped (status != solved: every output of it is 0)             */
    double* sens_res;            /* [batch] max over directions of the relative residual (NaN when skipped)              */
} rqp_sensitivity_io;

/* Reserve (before rqp_setup) the sensitivities' workspace: the adjoint's packed matrices, G_a, M^-1 (shared with the
 * adjoint and polish when those are reserved too), the active-row lists and one chunk of float64 direction blocks.
 * Handles without it allocate nothing for it.  After setup: RQP_OK if the state matches, else RQP_ERR_STATE.          */
int rqp_set_sensitivity(rqp_handle* h, int32_t enable);

/* Sensitivities of a solve of this handle's shape at the caller's data (io); as rqp_adjoint, nothing of the handle's state
 * is read.  A fixed, data-independent chain on `stream` (classify, pack; per chunk masked gram, factor, then one
 * right-hand-side and one solve launch per block of 16 directions); capturable in a HIP graph.  RQP_ERR_ARG: h, io,
 * io->dx, x, y, H or A NULL, ndir < 1, or z, l or u NULL without io->active.  RQP_ERR_STATE: the handle is not set up,
 * or was set up without rqp_set_sensitivity.                                                                            */
int rqp_sensitivity(rqp_handle* h, const rqp_sensitivity_io* io, void* stream);

/* ---- Condensing linear time-varying MPC problems on the device (DESIGN.md section 5 "LTV condensing") ----
 * Per instance b and stage k = 0 .. horizon-1:  x_{k+1} = A_k x_k + B_k u_k + c_k,  u_k = -K x_k + v_k, box constraints
 * l_add <= y <= u_add on y = [u_0, x_1, u_1, x_2, ..., u_{N-1}, x_N] (m = horizon (nu + nx)), decision variables
 * v = [v_0 .. v_{N-1}] (n = horizon nu), weights H_sp = blkdiag(R, Q, ..., R, Qf).  With y = F v + G x0 + f:
 *     H = sym(F' H_sp F),  A = F,  g = F' H_sp (G x0 + f - yref),  l / u = l_add / u_add - (G x0 + f),
 * yref = [uref_0, xref_1, ...]; the first input is u_0 = v_0 - K x0.  These functions take no handle: they write plain
 * row-major tensors in the layouts rqp_setup / rqp_update_mats / rqp_update read ([batch][n][n], [batch][m][n],
 * [batch][n], [batch][m]), usable with any handle of dims (n, m, batch, shared_mats = 0, dtype).
 * Batched inputs and all outputs are DEVICE arrays of dims.dtype; the shared weights Q [nx][nx], R [nu][nu], Qf [nx][nx]
 * (symmetric) and K [nu][nx] are DEVICE arrays of double whatever dims.dtype.  Arithmetic is float64; every output is rounded
 * once.  Everything is enqueued on `stream` of `device`: no host synchronisation, no allocation -- the float64 workspace
 * (rqp_ltv_workspace_bytes) belongs to the caller and carries F, H_sp F, [G | f] and F' H_sp [G | f] from rqp_ltv_condense to
 * any number of rqp_ltv_vectors calls.  Sizes: nx <= 16, nu <= 8, horizon <= 32, n <= 160, m <= 640, else
 * RQP_ERR_UNSUPPORTED.  A failure's text: rqp_last_error(NULL) (per host thread, cleared at the entry of each rqp_ltv_* call).
 * The calling thread's current HIP device is the same after the call as before it.
 *
 * Stage weights (DESIGN.md section 5 "LTV condensing, stage weights"): with RQP_LTV_STAGE_WEIGHTS the cost is per instance and
 * per stage, H_sp = blkdiag(R_0, Q_0, R_1, Q_1, ..., R_{N-1}, Q_{N-1}) of instance b: R_k weighs u_k, Q_k weighs x_{k+1}, so
 * Q_{N-1} is the terminal weight.  Q is then [batch][horizon][nx][nx] and R [batch][horizon][nu][nu] (DEVICE, double, every block
 * symmetric: read as given), Qf is not read and may be NULL.  rqp_ltv_condense, rqp_ltv_vectors (for H_sp yref) and
 * rqp_ltv_condense_adjoint honour the flag, and a workspace must be read with the flag it was written with; the workspace sizes
 * do not depend on it; the rqp_ltv_stage_* calls read only the workspace, accept the flag and ignore it.  Without the flag
 * nothing changes: the same kernels, the same bits.  Repeated blocks (Q_k = Q, Q_{N-1} = Qf, R_k = R) give the bits of the
 * shared call.                                                                                                               */
#define RQP_LTV_HAS_K 1            /* K is given (else K = 0)                                              */
#define RQP_LTV_HAS_C 2            /* c [batch][horizon][nx] is given (else c = 0)                         */
#define RQP_LTV_HAS_XREF 4         /* rqp_ltv_vectors: xref [batch][horizon][nx] (x_1 .. x_N) is given     */
#define RQP_LTV_HAS_UREF 8         /* rqp_ltv_vectors: uref [batch][horizon][nu] is given                  */
#define RQP_LTV_BOUNDS_BATCHED 16  /* l_add, u_add are [batch][m] (else [m], shared)                       */
#define RQP_LTV_STAGE_WEIGHTS 128  /* Q is [batch][horizon][nx][nx], R [batch][horizon][nu][nu] (double); Qf is not read */
typedef struct rqp_ltv_dims {
    int32_t batch, nx, nu, horizon;
    int32_t dtype;               /* rqp_dtype of the batched inputs and of every output                  */
    int32_t flags;               /* RQP_LTV_* bits; a set bit makes its pointer mandatory                */
} rqp_ltv_dims;

/* Bytes of workspace rqp_ltv_condense / rqp_ltv_vectors need for these dims (the flags do not change it). */
int rqp_ltv_workspace_bytes(const rqp_ltv_dims* dims, size_t* bytes);

/* Transition + Hessian step: Ad [batch][horizon][nx][nx], Bd [batch][horizon][nx][nu] (and c, K by the flags) ->
 * H [batch][n][n] (bitwise symmetric), A [batch][m][n] (= F; its structural zeros are exact), and the workspace.    */
int rqp_ltv_condense(const rqp_ltv_dims* dims, int device, const void* Ad, const void* Bd, const void* c,
                     const double* Q, const double* R, const double* Qf, const double* K,
                     void* H, void* A, void* workspace, void* stream);

/* Vector step from the workspace of the last rqp_ltv_condense with the same dims (its HAS_K / HAS_C flags included):
 * x0 [batch][nx] (and xref, uref by the flags; l_add, u_add [m] or [batch][m]) -> g [batch][n], l, u [batch][m].      */
int rqp_ltv_vectors(const rqp_ltv_dims* dims, int device, const void* x0, const void* xref, const void* uref,
                    const void* l_add, const void* u_add, const double* Q, const double* R, const double* Qf,
                    const void* workspace, void* g, void* l, void* u, void* stream);

/* Reverse mode of the condensing (DESIGN.md section 5 "LTV condensing, adjoint"): the cotangents of (H, A, g, l, u) mapped back
 * to the inputs of rqp_ltv_condense + rqp_ltv_vectors.  With S = H_sp, Hs = (dH + dH') / 2, e = G x0 + f - yref, T = F Hs:
 *     Fb = dA + 2 S T + (S e) dg',  eb = S F dg,  sb = eb - dl - du,  dx0 = G'sb,  dyref = -eb,  [Gb | fb] = sb [x0' | 1],
 *     Sb_kk = F_k T_k' + (F dg)_k e_k'  (diagonal blocks; dR = sum of the u blocks, dQ / dQf of the x blocks, symmetrised),
 * then, Yb = [Fb | Gb | fb] and X_k = the x_k rows of [F | G | f] (X_0 = [0 | I | 0]), the sweep over the stages
 *     Lam = Yb[x_N rows];  k = N-1 .. 0:  dAd_k = Lam X_k',  dBd_k = Lam[:, k nu:(k+1) nu] - dAd_k K',  dc_k = Lam[:, f],
 *                                         Lam <- (A_k - B_k K)' Lam - K' Yb[u_k rows] + Yb[x_k rows]   (k >= 1).
 * Whatever finite values dA holds at the structural zeros of A = F are not read.  K gets no gradient (a reparametrisation:
 * u_0 = v_0 - K x0 does not depend on it); the gradients of l_add, u_add are dl, du themselves.
 * Pointers are DEVICE pointers; the batched ones are in dims.dtype, the weights and their gradients double.               */
typedef struct rqp_ltv_adjoint_io {
    const void *Ad, *Bd, *c;     /* the forward inputs of that linearisation (c is not read: f is in the workspace)      */
    const void *x0, *xref, *uref;/* [batch][nx], and by the flags [batch][horizon][nx], [batch][horizon][nu]             */
    const double *Q, *R, *Qf, *K;/* as in rqp_ltv_condense (K by RQP_LTV_HAS_K)                                          */
    const void* workspace;       /* the forward workspace as rqp_ltv_condense left it for these Ad, Bd, c (read only)    */
    const void *dH, *dA, *dg, *dl, *du; /* cotangents [batch][n][n], [batch][m][n], [batch][n], [batch][m] x 2; NULL = 0 */
    void *dAd, *dBd, *dc;        /* outputs [batch][horizon][nx][nx], [..][nx][nu], [..][nx]; NULL = not wanted          */
    void *dx0, *dxref, *duref;   /* outputs shaped like x0, xref, uref; NULL = not wanted                                */
    double *dQ, *dR, *dQf;       /* outputs [nx][nx], [nu][nu], [nx][nx], summed over the batch, symmetric; NULL = not wanted */
                                 /* RQP_LTV_STAGE_WEIGHTS: dQ [batch][horizon][nx][nx], dR [batch][horizon][nu][nu], each block  */
                                 /* the symmetrised Sb_kk block of its own instance and stage, no batch sum; dQf must be NULL    */
    void* adjoint_workspace;     /* rqp_ltv_adjoint_workspace_bytes, the caller's; contents need not survive the call    */
} rqp_ltv_adjoint_io;

/* Bytes of the adjoint's own workspace for these dims (the flags do not change it). */
int rqp_ltv_adjoint_workspace_bytes(const rqp_ltv_dims* dims, size_t* bytes);

/* dims as in the forward calls (flags: HAS_K, HAS_XREF, HAS_UREF say which of K, xref, uref are read; HAS_C and BOUNDS_BATCHED
 * are accepted and change nothing).  Same contract as the forward: float64 arithmetic, every output rounded once, enqueued on
 * `stream` of `device` with no allocation and no host synchronisation, a fixed launch chain that depends on dims and on which
 * pointers are NULL only (capturable in a HIP graph), the caller's current device restored.  Work that only serves outputs that
 * are not wanted is skipped (dx0 / dxref / duref alone: one kernel; no dAd, dBd, dc: no sweep).  No atomics: the batch sums of
 * dQ, dR, dQf are added in a fixed order and two calls give the same bits (RQP_LTV_STAGE_WEIGHTS: there is no sum, one kernel
 * symmetrises the per-stage blocks into dQ, dR).  RQP_ERR_ARG: io, Ad, Bd, x0, Q, R, Qf (without RQP_LTV_STAGE_WEIGHTS),
 * workspace or adjoint_workspace NULL, a flag names an input whose pointer is NULL, or dQf given with RQP_LTV_STAGE_WEIGHTS. */
int rqp_ltv_condense_adjoint(const rqp_ltv_dims* dims, int device, const rqp_ltv_adjoint_io* io, void* stream);

/* ---- Stage constraints of LTV MPC problems (DESIGN.md section 5 "LTV condensing, stage constraints") ----
 * Instead of the box on y, every stage k of every instance carries nc rows  lo_k <= E_k [u_k ; x_{k+1}] <= hi_k
 * (E_k [nc][nu + nx]; u_k is the plant's input -K x_k + v_k), m_c = horizon nc rows in all.  With y = F v + s, s = G x0 + f as
 * rqp_ltv_condense left them in the workspace (only read here):
 *     A_c = E F  (block row k = E_k times the rows k (nu + nx) .. of F),   l_c = lo - E s,   u_c = hi - E s;
 * H and g are those of rqp_ltv_condense / rqp_ltv_vectors.  Block row k of A_c is summed over the columns < (k + 1) nu, where F
 * can be non-zero, and is exactly zero to the right whatever E holds; an infinite lo / hi entry comes back infinite.
 * E is [batch][horizon][nc][nu + nx], or [horizon][nc][nu + nx] with RQP_LTV_STAGE_SHARED_E; lo, hi are [m_c], or [batch][m_c]
 * with RQP_LTV_BOUNDS_BATCHED; outputs A_c [batch][m_c][n], l_c, u_c [batch][m_c].  Everything batched is a DEVICE array of
 * dims.dtype.  The contract of the other rqp_ltv_* calls holds: float64 arithmetic, every output rounded once, enqueued on
 * `stream` of `device`, no allocation, no host synchronisation, no atomics, a launch chain that depends on dims, nc and on which
 * pointers are NULL only (capturable in a HIP graph), the caller's current device restored, rqp_last_error(NULL).
 * Sizes: those of rqp_ltv_condense and 1 <= nc <= 32, m_c <= 640, else RQP_ERR_UNSUPPORTED.  RQP_ERR_ARG: a NULL pointer
 * that is not marked optional.  RQP_LTV_STAGE_SHARED_E is a flag of these three calls only.                                  */
#define RQP_LTV_STAGE_SHARED_E 32  /* E is [horizon][nc][nu+nx] (else [batch][...])                        */
int rqp_ltv_stage_rows(const rqp_ltv_dims* dims, int device, int32_t nc, const void* E, const void* workspace, void* A_c,
                       void* stream);
int rqp_ltv_stage_vectors(const rqp_ltv_dims* dims, int device, int32_t nc, const void* E, const void* x0, const void* lo,
                          const void* hi, const void* workspace, void* l_c, void* u_c, void* stream);

/* Reverse mode of the two calls above, t = dl_c + du_c:
 *     dA_full = E' dA_c (block row k = E_k' dA_c,k; exact zeros right of the staircase),   dl_full = E' t,
 *     dE_k = dA_c,k F_k' - t_k s_k'   (per instance also when E is shared: the batch sum is the caller's).
 * dA_full and dl_full are the dA and dl of rqp_ltv_condense_adjoint (du = NULL there: l = l_add - s there, l_c = lo - E s here);
 * the gradients of lo, hi are dl_c, du_c themselves.  Whatever finite values dA_c holds right of the staircase are not read.  */
typedef struct rqp_ltv_stage_adjoint_io {
    const void *E, *x0;          /* as in the forward calls                                                              */
    const void* workspace;       /* the forward workspace as rqp_ltv_condense left it for this linearisation (read only) */
    const void *dA_c, *dl_c, *du_c; /* cotangents [batch][m_c][n], [batch][m_c] x 2; NULL = 0                            */
    void *dA_full, *dl_full, *dE;/* outputs [batch][m][n], [batch][m], [batch][horizon][nc][nu+nx]; NULL = not wanted    */
} rqp_ltv_stage_adjoint_io;
int rqp_ltv_stage_adjoint(const rqp_ltv_dims* dims, int device, int32_t nc, const rqp_ltv_stage_adjoint_io* io, void* stream);

/* ---- Input-rate (delta u) cost and bounds of LTV MPC problems (DESIGN.md section 5 "LTV condensing, input rates") ----
 * The cost of rqp_ltv_condense plus a move-suppression term, and slew-rate rows, both on the plant's input u_k = -K x_k + v_k and
 * both anchored to the input applied before stage 0, uprev [batch][nu] (dims.dtype):
 *     J = 1/2 (y - yref)' H_sp (y - yref) + 1/2 sum_k (u_k - u_{k-1})' S_k (u_k - u_{k-1}),    u_{-1} = uprev,
 *     dlo_k <= u_k - u_{k-1} <= dhi_k     (horizon nu rows).
 * With F[u_k] the nu rows k (nu + nx) .. of F, dF_k = F[u_k] - F[u_{k-1}] (dF_0 = F[u_0]) and ds_k likewise of s = G x0 + f:
 *     W_rate = H_sp F, its u rows plus S_k dF_k - S_{k+1} dF_{k+1} (S_N = 0),   H = sym(W_rate' F),   gmap = W_rate' [G | f],
 *     g = gmap [x0; 1] - F' (H_sp yref),  g[0:nu] -= S_0 uprev   (yref does not enter the rate term; g is rounded once),
 *     A_r,k = dF_k (exact zeros in the columns >= (k + 1) nu),   l_r,k = dlo_k - ds_k + [k = 0] uprev,   u_r,k likewise with dhi_k.
 * S is [batch][horizon][nu][nu], DEVICE, double, every block symmetric: read as given, like the stage weights.  dlo, dhi are
 * [horizon nu], or [batch][horizon nu] with RQP_LTV_BOUNDS_BATCHED (dims.dtype); an infinite entry comes back infinite.
 * RQP_LTV_STAGE_WEIGHTS and HAS_K / HAS_C / HAS_XREF / HAS_UREF work as in the plain calls; the workspace is that of
 * rqp_ltv_workspace_bytes, its size unchanged.  The contract of the other rqp_ltv_* calls holds: float64 arithmetic, every output
 * rounded once, enqueued on `stream` of `device`, no allocation, no host synchronisation, no atomics, a launch chain that depends
 * on dims and NULL pointers only (capturable in a HIP graph), no scratch, the caller's current device restored,
 * rqp_last_error(NULL).  Sizes: those of rqp_ltv_condense, else RQP_ERR_UNSUPPORTED.  RQP_ERR_ARG: a required pointer (S and
 * uprev among them) is NULL.
 *
 * A workspace written by rqp_ltv_condense_rate holds W_rate and gmap of the rate problem.  It must be read by
 * rqp_ltv_vectors_rate, not rqp_ltv_vectors (which would leave S_0 uprev out of g), and its reverse mode is
 * rqp_ltv_condense_adjoint_rate (below), not rqp_ltv_condense_adjoint, which reads W as H_sp F and knows no rate term.  F and
 * [G | f] in it are those of rqp_ltv_condense: the rqp_ltv_stage_* calls, rqp_ltv_rate_rows, rqp_ltv_rate_bounds and
 * rqp_ltv_condense_adjoint_rate read only them and work on the workspace of either condense call.  The plain entry points and
 * their launch chains are unchanged.                                                                                         */
int rqp_ltv_condense_rate(const rqp_ltv_dims* dims, int device, const void* Ad, const void* Bd, const void* c,
                          const double* Q, const double* R, const double* Qf, const double* K, const double* S,
                          void* H, void* A, void* workspace, void* stream);
int rqp_ltv_vectors_rate(const rqp_ltv_dims* dims, int device, const void* x0, const void* xref, const void* uref,
                         const void* l_add, const void* u_add, const double* Q, const double* R, const double* Qf,
                         const double* S, const void* uprev, const void* workspace, void* g, void* l, void* u, void* stream);
/* The rate rows.  A_r: horizon nu rows of n entries per instance, l_r / u_r: horizon nu entries per instance (dims.dtype);
 * instance b starts inst_stride ELEMENTS after instance b - 1, so the rows can land directly in the tail of a
 * [batch][m0 + horizon nu][n] matrix (inst_stride = (m0 + horizon nu) n, A_r = its address + m0 n elements) and of
 * [batch][m0 + horizon nu] vectors; nothing between the rows of two instances is written.  inst_stride smaller than one
 * instance's rows: RQP_ERR_ARG; larger than 640 rows (n or 1 elements each): RQP_ERR_UNSUPPORTED, the QP would exceed m = 640. */
int rqp_ltv_rate_rows(const rqp_ltv_dims* dims, int device, const void* workspace, void* A_r, int64_t inst_stride, void* stream);
int rqp_ltv_rate_bounds(const rqp_ltv_dims* dims, int device, const void* x0, const void* uprev, const void* dlo,
                        const void* dhi, const void* workspace, void* l_r, void* u_r, int64_t inst_stride, void* stream);

/* Reverse mode of the rate terms (DESIGN.md section 5 "LTV condensing, input rates, adjoint"): rqp_ltv_condense_adjoint for a
 * problem built by rqp_ltv_condense_rate + rqp_ltv_vectors_rate (+ rqp_ltv_rate_rows + rqp_ltv_rate_bounds).  io is that call's:
 * dH, dg are the cotangents of the rate problem's H and g, dA, dl, du those of the base rows (A = F and the box, or the dA_full /
 * dl_full of rqp_ltv_stage_adjoint); rate_io adds S, uprev, the cotangents of (A_r, l_r, u_r) and the outputs dS, duprev.  With
 * dF_k, ds_k as above, Hs = (dH + dH') / 2, q_k = (F dg)[u_k] - (F dg)[u_{k-1}], r_k = ds_k - [k = 0] uprev, t = dl_r + du_r and
 * M_k = dF_k Hs, the formulas of rqp_ltv_condense_adjoint gain
 *     Fb[u_k rows] += Z_k - Z_{k+1},   Z_k = dA_r,k + S_k (2 M_k + r_k dg')   (Z_N = 0),
 *     sb[u_k rows] += w_k - w_{k+1},   w_k = S_k q_k - t_k   (w_N = 0; before dx0 = G'sb and [Gb | fb] = sb [x0' | 1]),
 *     dS_k = sym(M_k dF_k' + q_k r_k')  (per instance and stage, bitwise symmetric),   duprev = t_0 - S_0 q_0;
 * eb = H_sp F dg (dxref, duref) and Sb_kk (dQ, dR, dQf) are those of the plain call: dQ, dR, dQf come back with its bits.  The
 * gradients of dlo, dhi are dl_r, du_r themselves.  The rate addend to Fb is formed and added in float64 whatever dims.dtype.
 * Whatever finite values dA_r holds right of the staircase (columns >= (k + 1) nu of block row k) are not read.
 * io->workspace may come from rqp_ltv_condense or rqp_ltv_condense_rate of this linearisation: only F and [G | f] are read.
 * io->adjoint_workspace needs rqp_ltv_adjoint_rate_workspace_bytes (that of the plain call and 2 horizon nu doubles per instance).
 * dA_r / dl_r, du_r: instance b starts dA_stride / dl_stride ELEMENTS after instance b - 1, as inst_stride of the forward row
 * calls, so they can be the tails of [batch][m0 + horizon nu][n] and [batch][m0 + horizon nu] cotangents; a stride is checked
 * only when one of its pointers is given (smaller than one instance's rows: RQP_ERR_ARG; more than 640 rows: RQP_ERR_UNSUPPORTED).
 * The contract of the other rqp_ltv_* calls holds: float64 arithmetic, every output rounded once, no allocation, no host
 * synchronisation, no atomics, no scratch, a launch chain fixed by dims and by which pointers are NULL (that of
 * rqp_ltv_condense_adjoint with its first kernel replaced and one kernel added before the sweep; capturable in a HIP graph), the
 * caller's current device restored, rqp_last_error(NULL).  RQP_ERR_ARG: what rqp_ltv_condense_adjoint rejects, or rate_io, S or
 * uprev NULL.  RQP_ERR_UNSUPPORTED: the sizes of rqp_ltv_condense_rate.                                                       */
typedef struct rqp_ltv_rate_adjoint_io {
    const double* S;             /* [batch][horizon][nu][nu] double, as in rqp_ltv_condense_rate                          */
    const void* uprev;           /* [batch][nu]                                                                           */
    const void *dA_r, *dl_r, *du_r; /* cotangents of the rate rows: horizon nu rows of n / horizon nu entries; NULL = 0   */
    int64_t dA_stride, dl_stride;/* elements between the instances of dA_r, and of dl_r / du_r                            */
    double* dS;                  /* output [batch][horizon][nu][nu], no batch sum; NULL = not wanted                      */
    void* duprev;                /* output [batch][nu]; NULL = not wanted                                                 */
} rqp_ltv_rate_adjoint_io;
int rqp_ltv_adjoint_rate_workspace_bytes(const rqp_ltv_dims* dims, size_t* bytes);
int rqp_ltv_condense_adjoint_rate(const rqp_ltv_dims* dims, int device, const rqp_ltv_adjoint_io* io,
                                  const rqp_ltv_rate_adjoint_io* rate_io, void* stream);

/* Which solve kernel the handle dispatches to ("generic", "resident", ...).       */
const char* rqp_kernel_name(const rqp_handle* h);

int rqp_destroy(rqp_handle* h);

const char* rqp_strerror(int err);
/* Text of the last failure on this handle (HIP error string etc.); h == NULL: of the last failed handle-less call
 * (rqp_ltv_*) on this host thread.                                                                                */
const char* rqp_last_error(const rqp_handle* h);
/* Library / ABI version, e.g. "rqp-hip 0.1 gfx950".                               */
const char* rqp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RQP_ABI_H */
