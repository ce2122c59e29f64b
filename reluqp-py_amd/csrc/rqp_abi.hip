// rqp_abi.hip -- the extern "C" boundary declared in include/rqp_abi.h.
// Host orchestration only: argument validation, workspace ownership, kernel dispatch.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

#include <map>
#include <mutex>
#include <utility>

#include "rqp_common.h"

hipError_t rqp_raise_lds_limit(const void* fn, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> limit;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = limit[std::make_pair(fn, dev)];
    if (bytes <= cur) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) cur = bytes;
    return e;
}

std::vector<double> rqp_diag_run(hipStream_t s, size_t groups, int waves, int slots, const std::function<void(unsigned long long*)>& launch) {
    unsigned long long* ticks = nullptr;
    const size_t cnt = groups * waves * slots;
    if (hipMalloc((void**)&ticks, cnt * 8) != hipSuccess) return {};
    launch(ticks);
    (void)hipStreamSynchronize(s);
    std::vector<unsigned long long> hb(cnt);
    (void)hipMemcpy(hb.data(), ticks, cnt * 8, hipMemcpyDeviceToHost);
    (void)hipFree(ticks);
    std::vector<double> tot((size_t)waves * slots, 0.0);
    for (int w = 0; w < waves; ++w)
        for (size_t g = 0; g < groups; ++g)
            for (int e = 0; e < slots; ++e) tot[(size_t)w * slots + e] += (double)hb[(g * waves + w) * slots + e];
    return tot;
}

#define RQP_VERSION "rqp-hip 0.3 gfx950"

namespace {

int fail_hip(rqp_handle* h, hipError_t e, const char* what) {
    if (h) h->err = std::string(what) + ": " + hipGetErrorString(e);
    return (e == hipErrorOutOfMemory) ? RQP_ERR_OOM : RQP_ERR_HIP;
}
int fail_arg(rqp_handle* h, const char* what) {
    if (h) h->err = what;
    return RQP_ERR_ARG;
}
int fail_state(rqp_handle* h, const char* what) {
    if (h) h->err = what;
    return RQP_ERR_STATE;
}
int fail_unsupported(rqp_handle* h, const char* what) {
    if (h) h->err = what;
    return RQP_ERR_UNSUPPORTED;
}

#define HIP_TRY(h, call)                                      \
    do {                                                      \
        hipError_t e__ = (call);                              \
        if (e__ != hipSuccess) return fail_hip(h, e__, #call); \
    } while (0)

bool settings_valid(const rqp_settings& s) {
    return s.rho > 0 && s.rho_min > 0 && s.rho_max >= s.rho_min && s.sigma >= 0 && s.adaptive_rho_tolerance > 1 &&
           s.eps_abs >= 0 && s.max_iter >= 0 && s.check_interval >= 1 && s.eps_rel >= 0 && s.eps_prim_inf >= 0 &&
           s.eps_dual_inf >= 0 && s.scaling >= 0;
}

// setup_rhos, reluqpth.py:20-38: repeated division / multiplication in doubles, sorted.
std::vector<double> build_rhos(const rqp_settings& s) {
    std::vector<double> r{s.rho};
    if (s.adaptive_rho) {
        double v = s.rho / s.adaptive_rho_tolerance;
        while (v >= s.rho_min) {
            r.push_back(v);
            v = v / s.adaptive_rho_tolerance;
        }
        v = s.rho * s.adaptive_rho_tolerance;
        while (v <= s.rho_max) {
            r.push_back(v);
            v = v * s.adaptive_rho_tolerance;
        }
        std::sort(r.begin(), r.end());
    }
    return r;
}

int argmin_abs(const std::vector<double>& r, double v) {   // np.argmin(np.abs(rhos - v)): first minimum
    int best = 0;
    double bd = std::fabs(r[0] - v);
    for (size_t i = 1; i < r.size(); ++i) {
        double d = std::fabs(r[i] - v);
        if (d < bd) {
            bd = d;
            best = (int)i;
        }
    }
    return best;
}

// The ADMM kernels, by rqp_kernel_id.
const rqp_kernel_desc rqp_kernels[RQP_K_COUNT] = {
    /* RQP_K_GENERIC */ {"generic", rqp_launch_solve_generic, nullptr, nullptr, nullptr},
    /* RQP_K_RES2    */ {"resident2", rqp_launch_solve_res2, nullptr, nullptr, nullptr},
    /* RQP_K_RES64   */ {"resident64", rqp_launch_solve_res64, nullptr, nullptr, nullptr},
    /* RQP_K_WAVE    */ {"wave", rqp_launch_solve_wave, nullptr, nullptr, nullptr},
    /* RQP_K_MFMA    */ {"mfma", rqp_launch_solve_mfma, rqp_mfma_img_elems, rqp_prepare_mfma, rqp_launch_pack_mfma},
    /* RQP_K_MFMA16  */ {"mfma16", rqp_launch_solve_mfma16, rqp_mfma16_img_elems, rqp_prepare_mfma16, rqp_launch_pack_mfma16},
    /* RQP_K_MFMAL   */ {"mfmal", rqp_launch_solve_mfmal, rqp_mfmal_img_elems, rqp_prepare_mfmal, rqp_launch_pack_mfmal},
    /* RQP_K_MFMAD   */ {"mfmad", rqp_launch_solve_mfmad, rqp_mfmad_img_elems, rqp_prepare_mfmad, rqp_launch_pack_mfmad},
};

// solve kernel: shared-(H, A) batches in 16-instance tiles on the matrix pipe, with an operand image (W1img); solve() only
bool tile_kernel(const rqp_handle* h) { return rqp_kernels[h->solve_kernel].pack != nullptr; }
// ... whose operands stream from L2 (slots grouped by starting rho index)
bool streams_operands(const rqp_handle* h) { return h->solve_kernel == RQP_K_MFMAL || h->solve_kernel == RQP_K_MFMAD; }
// k_admm_res2 runs on this handle -- as its solve kernel, or behind a tile kernel -- and so the handle keeps its register images
bool uses_res2(const rqp_handle* h) { return h->aux_kernel == RQP_K_RES2; }

// Handle-owned device memory: every allocation is recorded by the field that holds it; free_ws needs no list of its own.
template <class T>
hipError_t dev_alloc(rqp_handle* h, T** field, size_t bytes) {
    const hipError_t e = hipMalloc((void**)field, bytes);
    if (e == hipSuccess) h->owned.push_back((void**)field);
    return e;
}

void free_ws(rqp_handle* h) {
    // hipFree is one of the calls that invalidate a stream capture in progress (global / thread-local capture modes).  A handle
    // may be destroyed while this thread captures something else (a Python finaliser, an explicit `del`): free under the
    // relaxed mode, which exists for exactly this.
    hipStreamCaptureMode cmode = hipStreamCaptureModeRelaxed;
    const bool swapped = hipThreadExchangeStreamCaptureMode(&cmode) == hipSuccess;
    for (void** p : h->owned) {
        (void)hipFree(*p);
        *p = nullptr;
    }
    h->owned.clear();
    h->adj_G = h->adj_Minv = nullptr;             // (aliases of polish's buffers when not in `owned`)
    if (h->ncont_h) (void)hipHostFree(h->ncont_h);
    if (swapped) (void)hipThreadExchangeStreamCaptureMode(&cmode);
    h->ncont_h = nullptr;
    h->windowed = false;
    h->borrow_A = false;
    h->kpack_direct = false;
    h->is_setup = false;
    h->order_valid = false;
    h->solve_kernel = h->aux_kernel = RQP_K_GENERIC;
}

// mode 0 (the cont = 2 passes of a windowed handle included) runs on the solve kernel, iterate / residuals on the auxiliary one
hipError_t launch_solve(const rqp_handle* h, const SolveArgs& a, hipStream_t s) {
    return rqp_kernels[a.mode == 0 ? h->solve_kernel : h->aux_kernel].solve(h, a, s);
}

SolveArgs make_solve_args(const rqp_handle* h) {
    SolveArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = h->n; a.m = h->m; a.ldn = h->ldn; a.ldm = h->ldm; a.nrho = h->nrho; a.B = h->B;
    a.max_iter = h->st.max_iter;
    a.check_interval = h->st.check_interval;
    a.warm_starting = h->st.warm_starting;
    a.rho_ind0 = h->rho_ind0;
    a.sigma = h->st.sigma;
    a.tol = h->st.adaptive_rho_tolerance;
    a.rho_min = h->st.rho_min;
    a.rho_max = h->st.rho_max;
    a.thr_p = h->st.eps_abs * std::sqrt((double)h->m);   // reluqpth.py:233
    a.thr_d = h->st.eps_abs * std::sqrt((double)h->n);
    a.eps_rel = h->st.eps_rel;
    a.check_infeas = h->st.check_infeasibility;
    a.eps_pinf = h->st.eps_prim_inf;
    a.eps_dinf = h->st.eps_dual_inf;
    a.Ht = h->Ht; a.A = h->A; a.At = h->At; a.K = h->K;
    const bool sh = h->dims.shared_mats != 0;
    a.sH = sh ? 0 : (size_t)h->n * h->ldn;
    a.sA = sh ? 0 : (size_t)h->m * h->ldn;
    a.sAt = sh ? 0 : (size_t)h->n * h->ldm;
    a.sK = sh ? 0 : (size_t)h->kwin * h->n * h->ldn;
    a.kwin = h->kwin;
    if (h->windowed) {
        a.wbase = h->wbase_d;
        a.ax = h->ax_d;
        a.cstat = h->cstat_d;
        a.ncont = h->ncont_d;
        a.cont_iter = h->cont_iter_d;
        a.cont_rho = h->cont_rho_d;
    }
    a.g = h->g; a.l = h->l; a.u = h->u; a.c = h->c;
    a.rhos = h->rhos_d;
    if (h->st.scaling > 0) { a.scD = h->Dsc; a.scE = h->Esc; a.scC = h->csc; }
    a.x = h->x; a.z = h->z; a.lam = h->lam; a.rho_ind = h->rho_ind;
    return a;
}


SetupArgs make_setup_args(const rqp_handle* h, const void* H, const void* g, const void* A, const void* l, const void* u) {
    SetupArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = h->n; a.m = h->m; a.ldn = h->ldn; a.ldm = h->ldm; a.nrho = h->nrho; a.B = h->B; a.nmat = h->nmat;
    a.sigma = h->st.sigma;
    a.eq_tol = h->st.eq_tol;
    a.H_in = H; a.A_in = A; a.g_in = g; a.l_in = l; a.u_in = u;
    a.Ht = h->Ht; a.A = h->borrow_A ? const_cast<void*>(A) : h->A; a.At = h->At; a.K = h->K; a.g = h->g; a.l = h->l; a.u = h->u; a.c = h->c;
    a.G = h->G;
    a.rhos = h->rhos_d;
    a.fscratch = h->fscratch;
    a.kwin = h->kwin;
    a.wbase = h->windowed ? h->wbase_d : nullptr;
    return a;
}

// Kernel selection (rqp_dims.kernel; AUTO = measured crossovers).  Pure function of the handle: no environment.
int select_kernels(rqp_handle* h) {
    h->solve_kernel = h->aux_kernel = RQP_K_GENERIC;
    const bool res2_fits = rqp_res2_fits(h), res64_fits = rqp_res64_fits(h), wave_fits = rqp_wave_fits(h);
    const bool mfma_fits = rqp_mfma_fits(h), mfmal_fits = rqp_mfmal_fits(h), mfmad_fits = rqp_mfmad_fits(h);
    const bool f16 = h->dims.tile_dtype == RQP_TILE_F16, bf16 = h->dims.tile_dtype == RQP_TILE_BF16;
    // ---- the request, after the tile formats' say
    int req = h->dims.kernel;
    if (f16) {                                    // the fp16 K tile lives in the register-resident kernel; the MFMA kernel takes
                                                  // the same rounded K into its float32 operand image (k_pack_mfma)
        const bool mfma_ok = mfma_fits && res2_fits;
        if (req == RQP_KERNEL_AUTO && res2_fits && !(mfma_ok && h->B >= 2048 && (h->n > 56 || h->m > 128))) req = RQP_KERNEL_RESIDENT;
        if (req != RQP_KERNEL_RESIDENT && !((req == RQP_KERNEL_MFMA || req == RQP_KERNEL_AUTO) && mfma_ok))
            return fail_unsupported(h, "tile_dtype = f16 needs the resident kernel (float32, n <= 104, m <= 320) or the MFMA kernel");
    }
    if (bf16) {                                   // the bf16-plane tile exists in the MFMA kernel only: an explicit request for it
        if (!mfma_fits || (req != RQP_KERNEL_AUTO && req != RQP_KERNEL_MFMA))
            return fail_unsupported(h, "tile_dtype = bf16 needs the MFMA kernel: float32, shared (H, A), n <= 80, m <= 320");
        req = RQP_KERNEL_MFMA;
    }
    // ---- the solve kernel
    rqp_kernel_id k = RQP_K_GENERIC;
    switch (req) {
        case RQP_KERNEL_GENERIC:
            break;
        case RQP_KERNEL_RESIDENT:
            if (res2_fits) k = RQP_K_RES2;
            else if (res64_fits) k = RQP_K_RES64;
            else return fail_unsupported(h, "kernel=resident: needs n <= 104, m <= 320");
            break;
        case RQP_KERNEL_WAVE:
            if (!wave_fits) return fail_unsupported(h, "kernel=wave: needs n <= 32, m <= 64 (float32 also n <= 32, m <= 128 and 56 < n <= 64, m <= 128)");
            k = RQP_K_WAVE;
            break;
        case RQP_KERNEL_MFMA:
            if (mfma_fits && bf16) k = RQP_K_MFMA16;                          // (bf16 was refused above where mfma_fits does not hold)
            else if (mfma_fits) k = RQP_K_MFMA;                               // operands resident in registers
            else if (mfmal_fits) k = RQP_K_MFMAL;                             // operands streamed from L2 (rqp_mfmal.hip)
            else if (mfmad_fits) k = RQP_K_MFMAD;                             // float64 MFMA, streamed operands (rqp_mfmad.hip)
            else return fail_unsupported(h, "kernel=mfma: needs shared (H, A) and float32 with n <= 320, m <= 640 (bf16 tile: n <= 80, m <= 320) "
                                            "or float64 with n <= 160, m <= 320");
            break;
        default: {
            // shared-(H,A) batches large enough to fill the chip with 16-instance tiles go to the MFMA kernel: from ~2k
            // instances (below, the per-instance kernels still win; crossover measured on the condensed-MPC shape: 1024 ->
            // resident 1.7x faster, 2048 -> even cold / MFMA 1.3x closed loop, 3072 -> MFMA 1.35x / 1.8x) and only for
            // problems beyond the small / mid per-instance tiles -- the MFMA tile costs the same whatever the problem size
            // (minus skipped zero groups); on n=30, m=60 the one-wavefront kernel is 3-4x faster, on n=20, m=80 the mid
            // resident tile is on par (measured)
            const bool mfma_pays = h->B >= 2048 && (h->n > 56 || h->m > 128);
            // check_infeasibility: only the streaming kernel tests the certificates at every check (an infeasible instance
            // leaves at the first check where one holds, like the oracle; the other kernels would run it to max_iter first)
            if (h->st.check_infeasibility)
                break;
            if (mfma_fits && mfma_pays)
                k = RQP_K_MFMA;
            else if (mfmal_fits && !res2_fits && !wave_fits)
                k = RQP_K_MFMAL;                 // beyond every resident tile (the sparse linear-MPC form): 16-instance MFMA tiles with
                                                 // streamed operands instead of the streaming kernel's 2 MB of matrices per instance-iteration
                                                 // (any batch: ONE instance solves in 1.0 ms against 2.8 ms, tools/mfmal_check.py 1)
            else if (mfmad_fits && ((mfma_pays && h->B >= 3072) || (!res64_fits && !wave_fits)))
                k = RQP_K_MFMAD;                 // float64 shared batches: 16-instance tiles on v_mfma_f64_16x16x4_f64 from ~3k instances
                                                 // (measured on the condensed-MPC shape: 4096 -> 1.5x the float64 resident kernel; at
                                                 // 2048 one resident instance per CU still wins), or whenever no resident kernel fits
            else if (wave_fits)                  // small problems: one wavefront per instance
                k = RQP_K_WAVE;
            else if (res2_fits)
                k = RQP_K_RES2;
            else if (res64_fits)                 // float64 (the reference's default precision) at the headline sizes
                k = RQP_K_RES64;
        }
    }
    h->solve_kernel = k;
    // ---- the auxiliary kernel: the resident kernels run every mode themselves; iterate / residuals and the hand-off of a TILE-kernel
    // handle run on the float32 resident tile when one fits; those of every other handle -- a wave handle too -- on the streaming kernel
    if (k == RQP_K_RES2 || k == RQP_K_RES64) h->aux_kernel = k;
    else if (tile_kernel(h) && res2_fits) h->aux_kernel = RQP_K_RES2;
    if (f16 && !uses_res2(h)) return fail_unsupported(h, "tile_dtype = f16 needs the resident kernel");
    // ---- what follows from the two
    // RQP_FLAG_LOW_MEMORY: the float32 resident kernel reads K from the row-major table (no effect on the other kernels, which
    // have no packed copy of it; the fp16 tile IS the smaller copy)
    h->k_direct = (h->dims.flags & RQP_FLAG_LOW_MEMORY) && uses_res2(h) && !f16;
    // rho-ladder window (rqp_common.h): batches of per-instance matrices whose solve kernel runs the exit-and-continue protocol
    // (resident float32 / float64 tiles, one-wavefront kernel, streaming kernel).  Not with check_infeasibility (its certificate pass reads K at the final index)
    // and not on request (RQP_FLAG_FULL_LADDER: rqp_solve then never synchronises the host, e.g. for graph capture).
    h->windowed = !h->dims.shared_mats && h->nmat >= 32 && h->nrho > RQP_WINDOW && !(h->dims.flags & RQP_FLAG_FULL_LADDER) &&
                  !h->st.check_infeasibility && !tile_kernel(h);
    h->kwin = h->windowed ? RQP_WINDOW : h->nrho;
    // (rqp_common.h; not on a handle set up for polishing, which reads the row-major A after every solve)
    h->borrow_A = h->windowed && uses_res2(h) && h->st.scaling <= 0 && h->ldn == h->n && !h->polish_reserved;
    h->kpack_direct = h->windowed && uses_res2(h) && !h->k_direct && !f16;
    return RQP_OK;
}

// kpack_direct handles: the factor kernel's output is the register image of k_admm_res2
void set_kp_image(const rqp_handle* h, SetupArgs& f) {
    if (!h->kpack_direct) return;
    f.kp_img = h->Kpack;
    rqp_res2_kp_layout(h, &f.kp_cw, &f.kp_kr, &f.kp_kc);
}

// pack (QP.__init__ casts) -> G = A'cA -> K_j ladder -> kernel images, for new H and/or A (NULL: keep the packed copy).
// Shared by rqp_setup and rqp_update_mats.
int build_matrices(rqp_handle* h, const SetupArgs& a, hipStream_t s) {
    HIP_TRY(h, rqp_launch_pack_mats(h, a, s));
    if (h->st.scaling > 0) HIP_TRY(h, rqp_launch_ruiz(h, s));       // Ht, A, At scaled in place; D, E, c kept for the boundary
    if (a.A) HIP_TRY(h, rqp_launch_gram(h, a, s));                  // (NULL: a handle without a copy of A that keeps its A -- G = A'cA stands)
    if (uses_res2(h) && !h->Apack) {                                // (before the factor launch: kpack_direct writes Kpack there)
        size_t ae, ke, he;
        rqp_res2_pack_elems(h, &ae, &ke, &he);
        HIP_TRY(h, dev_alloc(h, &h->Apack, ae * sizeof(float)));
        if (ke) HIP_TRY(h, dev_alloc(h, &h->Kpack, ke * sizeof(float)));   // (none with RQP_FLAG_LOW_MEMORY)
        HIP_TRY(h, dev_alloc(h, &h->Hpack, he * sizeof(float)));
        if (h->dims.tile_dtype == RQP_TILE_F16) HIP_TRY(h, dev_alloc(h, &h->Kscale, (size_t)h->nmat * h->nrho * sizeof(float)));
        HIP_TRY(h, rqp_prepare_res2(h));
    }
    {
        SetupArgs f = a;
        set_kp_image(h, f);
        HIP_TRY(h, rqp_launch_factor(h, f, s));
    }
    if (uses_res2(h)) HIP_TRY(h, rqp_launch_pack_res2(h, a.A, nullptr, nullptr, s));
    if (h->solve_kernel == RQP_K_RES64) HIP_TRY(h, rqp_prepare_res64(h));
    if (tile_kernel(h)) {
        const rqp_kernel_desc& k = rqp_kernels[h->solve_kernel];
        if (!h->W1img) {
            HIP_TRY(h, dev_alloc(h, &h->W1img, k.img_elems(h) * sizeof(float)));
            HIP_TRY(h, dev_alloc(h, &h->queue, sizeof(int)));
            HIP_TRY(h, k.prepare(h));
        }
        HIP_TRY(h, k.pack(h, s));
    }
    return RQP_OK;
}

// ---- rqp_setup's workspace, in steps.  Each returns at its first failure; rqp_setup then releases everything (free_ws).

// matrices, vectors, ADMM state, the rho ladder, and what the solve kernel's launch order needs
int alloc_core(rqp_handle* h, hipStream_t s) {
    const size_t n = h->n, m = h->m, B = h->B, nm = h->nmat, e = h->esz;
    HIP_TRY(h, dev_alloc(h, &h->Ht, nm * n * h->ldn * e));
    if (!h->borrow_A) HIP_TRY(h, dev_alloc(h, &h->A, nm * m * h->ldn * e));     // (rqp_common.h: borrow_A)
    // A' (the streaming kernel's A dx operand and the wavefront kernel's column role): not on a windowed resident handle, whose
    // solve / iterate / residuals all run on k_admm_res2 / k_admm_res64 (neither reads A') and which refuses the certificate pass
    // (float32: 0.5 GB and 0.4 ms at B = 4096; float64: 1 GB and 1 ms)
    const bool resident_solve = h->solve_kernel == RQP_K_RES2 || h->solve_kernel == RQP_K_RES64;
    if (!(h->windowed && resident_solve)) HIP_TRY(h, dev_alloc(h, &h->At, nm * n * h->ldm * e));
    if (!h->kpack_direct) {   // (+ a zeroed tail: the low-memory K load of the resident kernel reads up to one vector past a row's end)
        const size_t kb = nm * h->kwin * n * h->ldn * e;
        HIP_TRY(h, dev_alloc(h, &h->K, kb + 256));
        HIP_TRY(h, hipMemsetAsync((char*)h->K + kb, 0, 256, s));
    }
    HIP_TRY(h, dev_alloc(h, &h->g, B * n * e));
    for (void** v : {&h->l, &h->u, &h->c}) HIP_TRY(h, dev_alloc(h, v, B * m * e));
    HIP_TRY(h, dev_alloc(h, &h->G, nm * n * n * sizeof(double)));
    HIP_TRY(h, dev_alloc(h, &h->x, B * n * sizeof(double)));
    for (double** v : {&h->z, &h->lam}) HIP_TRY(h, dev_alloc(h, v, B * m * sizeof(double)));
    HIP_TRY(h, dev_alloc(h, &h->rho_ind, B * sizeof(int32_t)));
    HIP_TRY(h, dev_alloc(h, &h->rhos_d, h->nrho * sizeof(double)));
    HIP_TRY(h, hipMemcpyAsync(h->rhos_d, h->rhos.data(), h->nrho * sizeof(double), hipMemcpyHostToDevice, s));
    const size_t lds_need = (n * n + 2 * n) * sizeof(double);
    if (lds_need > 160 * 1024 - 512) {   // factor scratch in global memory
        h->fscratch_elems = nm * h->kwin * n * n;
        HIP_TRY(h, dev_alloc(h, &h->fscratch, h->fscratch_elems * sizeof(double)));
    }
    HIP_TRY(h, dev_alloc(h, &h->flag_d, sizeof(int32_t)));
    if (h->st.scaling > 0) {
        HIP_TRY(h, dev_alloc(h, &h->Dsc, nm * n * sizeof(double)));
        HIP_TRY(h, dev_alloc(h, &h->Esc, nm * m * sizeof(double)));
        HIP_TRY(h, dev_alloc(h, &h->csc, nm * sizeof(double)));
    }
    if (streams_operands(h) && h->B > 16)          // slot order of the streamed-operand MFMA kernels (grouped by starting rho index)
        HIP_TRY(h, dev_alloc(h, &h->order_d, B * sizeof(int32_t)));
    if (h->solve_kernel == RQP_K_MFMAL && h->B > 16) {   // regrouped cold solve (rqp_mfmal.hip): exact state of the instances between its two launches
        HIP_TRY(h, dev_alloc(h, &h->ax_d, B * m * sizeof(double)));
        HIP_TRY(h, dev_alloc(h, &h->cont_rho_d, B * sizeof(double)));
        HIP_TRY(h, dev_alloc(h, &h->key_d, B * sizeof(int32_t)));
    }
    if (!tile_kernel(h) && h->B >= (h->solve_kernel == RQP_K_RES64 ? 2 : 4) * h->ncu) {   // dispatch order (see rqp_common.h): batches that outlast one wave of workgroups
        HIP_TRY(h, dev_alloc(h, &h->order_d, B * sizeof(int32_t)));
        HIP_TRY(h, dev_alloc(h, &h->last_iter_d, B * sizeof(int32_t)));
    }
    return RQP_OK;
}

// rho-ladder window: every window starts around rho_ind0; the exit-and-continue state of the instances
int alloc_window(rqp_handle* h, hipStream_t s) {
    const size_t m = h->m, B = h->B, nm = h->nmat;
    const int w0 = std::min(std::max(h->rho_ind0 - 1, 0), h->nrho - h->kwin);
    HIP_TRY(h, dev_alloc(h, &h->wbase_d, nm * sizeof(int32_t)));
    HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)h->wbase_d, w0, nm, s));
    HIP_TRY(h, dev_alloc(h, &h->ax_d, B * m * sizeof(double)));
    HIP_TRY(h, dev_alloc(h, &h->cstat_d, B * sizeof(int32_t)));
    HIP_TRY(h, hipMemsetAsync(h->cstat_d, 0, B * sizeof(int32_t), s));
    HIP_TRY(h, dev_alloc(h, &h->ncont_d, 2 * sizeof(int32_t)));
    HIP_TRY(h, hipHostMalloc((void**)&h->ncont_h, sizeof(int32_t), hipHostMallocDefault));
    HIP_TRY(h, dev_alloc(h, &h->cont_iter_d, B * sizeof(int32_t)));
    HIP_TRY(h, dev_alloc(h, &h->cont_rho_d, B * sizeof(double)));
    return RQP_OK;
}

// The factor kernels read rho from the ladder array: a one-element "ladder" holding 1 / delta.  The value is copied from this
// stack frame, so the stream is drained before returning.
int alloc_inv_delta(rqp_handle* h, double** field, double delta, hipStream_t s) {
    const double idel = 1.0 / delta;
    HIP_TRY(h, dev_alloc(h, field, sizeof(double)));
    HIP_TRY(h, hipMemcpyAsync(*field, &idel, sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return RQP_OK;
}

// solution polishing (rqp_polish.hip): chunked float64 workspace, per-instance results
int alloc_polish(rqp_handle* h, hipStream_t s) {
    const size_t n = h->n, m = h->m, B = h->B;
    if (rqp_polish_lds_bytes(h) > 160 * 1024)
        return fail_unsupported(h, "rqp_setup: polish needs 8 (4 n + 4 m + 264) bytes of LDS, above 160 KB");
    h->polish_chunk = rqp_polish_chunk(h);
    const size_t pc = h->polish_chunk;
    HIP_TRY(h, dev_alloc(h, &h->polish_G, pc * n * n * sizeof(double)));
    HIP_TRY(h, dev_alloc(h, &h->polish_Minv, pc * n * h->ldn * sizeof(double)));
    if (const int rc = alloc_inv_delta(h, &h->polish_rho, h->polish_delta, s)) return rc;
    HIP_TRY(h, dev_alloc(h, &h->polish_status, B * sizeof(int32_t)));
    HIP_TRY(h, hipMemsetAsync(h->polish_status, 0, B * sizeof(int32_t), s));
    HIP_TRY(h, dev_alloc(h, &h->polish_act, B * m));
    HIP_TRY(h, hipMemsetAsync(h->polish_act, 0, B * m, s));
    HIP_TRY(h, dev_alloc(h, &h->polish_flag, B * sizeof(int32_t)));
    HIP_TRY(h, dev_alloc(h, &h->polish_st_in, B * sizeof(int32_t)));
    HIP_TRY(h, dev_alloc(h, &h->polish_res_in, 3 * B * sizeof(double)));
    return RQP_OK;
}

// adjoint (rqp_adjoint.hip) and forward sensitivities (rqp_sens.hip): packed caller matrices, G_a and M^-1 per chunk
int alloc_adjoint(rqp_handle* h, hipStream_t s) {
    const size_t n = h->n, m = h->m, B = h->B, e = h->esz;
    if (h->adj_reserved && rqp_adjoint_lds_bytes(h) > 160 * 1024)
        return fail_unsupported(h, "rqp_setup: the adjoint needs 8 (4 n + 4 m + 264) bytes of LDS, above 160 KB");
    if (h->sens_reserved && rqp_sens_lds_bytes(h) > 160 * 1024)
        return fail_unsupported(h, "rqp_setup: the sensitivities need 384 ceil16(n) + 2 KB of LDS, above 160 KB");
    h->adj_chunk = rqp_polish_chunk(h);
    const size_t pc = h->adj_chunk, pm = h->dims.shared_mats ? 1 : pc;
    HIP_TRY(h, dev_alloc(h, &h->adj_Ht, pm * n * h->ldn * e));
    HIP_TRY(h, dev_alloc(h, &h->adj_A, pm * m * h->ldn * e));
    if (h->polish_reserved) {               // (same chunk rule: polish's buffers hold one chunk of either) aliases, not allocations
        h->adj_G = h->polish_G;
        h->adj_Minv = h->polish_Minv;
    } else {
        HIP_TRY(h, dev_alloc(h, &h->adj_G, pc * n * n * sizeof(double)));
        HIP_TRY(h, dev_alloc(h, &h->adj_Minv, pc * n * h->ldn * sizeof(double)));
    }
    if (const int rc = alloc_inv_delta(h, &h->adj_rho, h->adj_delta, s)) return rc;
    HIP_TRY(h, dev_alloc(h, &h->adj_flag, B * sizeof(int32_t)));
    HIP_TRY(h, dev_alloc(h, &h->adj_act, B * m));
    if (h->adj_reserved)                    // per-instance rows of the matrix gradients
        HIP_TRY(h, dev_alloc(h, &h->adj_rows, B * (2 * n + 2 * m) * sizeof(double)));
    if (h->sens_reserved) {                 // active-row lists, one chunk of direction blocks
        for (int32_t** v : {&h->sens_idx, &h->sens_pos}) HIP_TRY(h, dev_alloc(h, v, B * m * sizeof(int32_t)));
        HIP_TRY(h, dev_alloc(h, &h->sens_na, B * sizeof(int32_t)));
        HIP_TRY(h, dev_alloc(h, &h->sens_ws, pc * rqp_sens_ws_doubles(h) * sizeof(double)));
    }
    return RQP_OK;
}

// straggler hand-off (SolveArgs) of a tile kernel to k_admm_res2: one tile per CU at most
int alloc_handoff(rqp_handle* h) {
    h->handoff_cols = 0;
    if (!(tile_kernel(h) && uses_res2(h) && (h->B + 15) / 16 <= h->ncu)) return RQP_OK;
    HIP_TRY(h, dev_alloc(h, &h->cont_iter_d, (size_t)h->B * sizeof(int32_t)));
    if (!h->cont_rho_d)                     // (k_admm_mfmal's regrouped cold solve has one already; a solve uses it for one of the two)
        HIP_TRY(h, dev_alloc(h, &h->cont_rho_d, (size_t)h->B * sizeof(double)));
    h->handoff_cols = 6;    // measured on the config-3 batch: 4.7 M QP/s without, 5.0 M at 2-4, 6.2 M at 6-10, 5.5 M at 12 (tools/)
    if (const char* ho = getenv("RQP_TUNE_HANDOFF")) h->handoff_cols = atoi(ho);   // (tuning aid of tools/mfma16_check.py, not a dispatch input)
    return RQP_OK;
}

// rqp_setup behind its argument checks, on an empty handle.  A failure may leave a partial workspace behind: the caller frees it.
int setup_workspace(rqp_handle* h, const void* H, const void* g, const void* A, const void* l, const void* u, hipStream_t s) {
    const auto t_begin = std::chrono::steady_clock::now();
    int rc = select_kernels(h);
    if (rc != RQP_OK) return rc;
    // the streaming kernel backs every handle (iterate / residuals modes, sizes beyond the tiles): its vectors must fit LDS
    if (const size_t lds = rqp_generic_lds_bytes(h); lds > 160 * 1024) {
        char buf[256];
        snprintf(buf, sizeof(buf), "rqp_setup: n=%d, m=%d needs %zu B of LDS for the vector state of the streaming kernel "
                 "(limit 163840 B per workgroup)", h->n, h->m, lds);
        return fail_unsupported(h, buf);
    }
    HIP_TRY(h, rqp_prepare_generic(h));
    rc = alloc_core(h, s);
    if (rc == RQP_OK && h->windowed) rc = alloc_window(h, s);
    if (rc == RQP_OK && h->polish_reserved) rc = alloc_polish(h, s);
    if (rc == RQP_OK && (h->adj_reserved || h->sens_reserved)) rc = alloc_adjoint(h, s);
    if (rc == RQP_OK) rc = alloc_handoff(h);
    if (rc != RQP_OK) return rc;
    SetupArgs a = make_setup_args(h, H, g, A, l, u);
    HIP_TRY(h, rqp_launch_pack_vecs(h, a, s));
    if (h->dims.shared_mats && h->B > 1) {
        // K is built from ONE equality pattern c (rho x 1e3 on rows with u - l <= eq_tol, reluqpth.py:54); the kernels
        // scale rho by every instance's own c.  A shared-matrix batch must therefore share the pattern.
        int32_t bad = 0;
        HIP_TRY(h, rqp_launch_check_shared_c(h, h->flag_d, s));
        HIP_TRY(h, hipMemcpyAsync(&bad, h->flag_d, sizeof(bad), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        if (bad)
            return fail_unsupported(h, "rqp_setup: shared (H, A) batch whose instances differ in which rows are equalities (u - l <= eq_tol); "
                                       "K(rho) is built per matrix, so pass H and A with a batch dimension for such a batch");
    }
    const auto t_alloc = std::chrono::steady_clock::now();
    if ((rc = build_matrices(h, a, s)) != RQP_OK) return rc;
    if (h->st.scaling > 0) HIP_TRY(h, rqp_launch_scale_vecs(h, h->g, h->l, h->u, s));    // g <- c D g, l/u <- E l/u
    h->is_setup = true;
    h->cold_state = true;
    if ((rc = rqp_clear_primal_dual(h, s)) != RQP_OK) return rc;    // zero state, rho_ind0 (reluqpth.py:148-153)
    if (h->debug & 1) {                         // host-side split of a setup call (synchronous, debug only)
        const auto t_enq = std::chrono::steady_clock::now();
        (void)hipStreamSynchronize(s);
        const auto t_end = std::chrono::steady_clock::now();
        auto ms = [](auto a0, auto a1) { return std::chrono::duration<double, std::milli>(a1 - a0).count(); };
        fprintf(stderr, "[rqp] setup host split: allocate %.2f ms, enqueue %.2f ms, device drain %.2f ms\n", ms(t_begin, t_alloc),
                ms(t_alloc, t_enq), ms(t_enq, t_end));
    }
    return RQP_OK;
}

}  // namespace

extern "C" {

int rqp_default_settings(rqp_settings* s) {
    if (!s) return RQP_ERR_ARG;
    s->rho = 0.1;            // classes.py:36-46
    s->rho_min = 1e-6;
    s->rho_max = 1e6;
    s->sigma = 1e-6;
    s->adaptive_rho_tolerance = 5;
    s->eps_abs = 1e-3;
    s->eq_tol = 1e-6;
    s->adaptive_rho = 1;
    s->max_iter = 4000;
    s->check_interval = 25;
    s->warm_starting = 1;
    s->eps_rel = 0.0;        // extensions: off = the reference's behaviour
    s->eps_prim_inf = 1e-4;
    s->eps_dual_inf = 1e-4;
    s->scaling = 0;
    s->check_infeasibility = 0;
    return RQP_OK;
}

int rqp_create(rqp_handle** out, const rqp_dims* dims, const rqp_settings* settings, int device) {
    if (!out || !dims || !settings) return RQP_ERR_ARG;
    *out = nullptr;
    if (dims->n < 1 || dims->m < 1 || dims->batch < 1) return RQP_ERR_ARG;
    if (dims->dtype != RQP_F32 && dims->dtype != RQP_F64) return RQP_ERR_ARG;
    if (dims->kernel < RQP_KERNEL_AUTO || dims->kernel > RQP_KERNEL_MFMA) return RQP_ERR_ARG;
    if (dims->tile_dtype != RQP_TILE_SAME &&
        !((dims->tile_dtype == RQP_TILE_F16 || dims->tile_dtype == RQP_TILE_BF16) && dims->dtype == RQP_F32)) return RQP_ERR_ARG;
    if (!settings_valid(*settings)) return RQP_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RQP_ERR_HIP;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device) != hipSuccess) return RQP_ERR_HIP;
    rqp_handle* h = new rqp_handle();
    h->ncu = pr.multiProcessorCount;
    {   // diagnostics only (occupancy print / s_memtime build); read once, never consulted for kernel selection
        const char* d1 = getenv("RQP_DEBUG");
        const char* d2 = getenv("RQP_DIAG");
        h->debug = ((d1 && d1[0] == '1') ? 1 : 0) | ((d2 && d2[0] == '1') ? 2 : 0);
    }
    h->dims = *dims;
    h->st = *settings;
    h->device = device;
    h->n = dims->n; h->m = dims->m; h->B = dims->batch;
    h->nmat = dims->shared_mats ? 1 : dims->batch;
    h->esz = dims->dtype == RQP_F32 ? 4 : 8;
    h->ldn = rqp_round_up(h->n, 4);
    h->ldm = rqp_round_up(h->m, 4);
    h->rhos = build_rhos(*settings);
    h->nrho = (int)h->rhos.size();
    h->rho_ind0 = argmin_abs(h->rhos, settings->rho);     // reluqpth.py:153
    *out = h;
    return RQP_OK;
}

int rqp_destroy(rqp_handle* h) {
    if (!h) return RQP_ERR_ARG;
    (void)hipSetDevice(h->device);
    free_ws(h);
    delete h;
    return RQP_OK;
}

int rqp_setup(rqp_handle* h, const void* H, const void* g, const void* A, const void* l, const void* u,
              void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!H || !g || !A || !l || !u) return fail_arg(h, "rqp_setup: null input pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    free_ws(h);
    const int rc = setup_workspace(h, H, g, A, l, u, (hipStream_t)stream);
    if (rc != RQP_OK) free_ws(h);               // every failure past this point leaves an empty handle; h->err says why
    return rc;
}

int rqp_update_mats(rqp_handle* h, const void* H, const void* A, void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    if (!H && !A) return RQP_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipSetDevice(h->device));
    SetupArgs a = make_setup_args(h, H, nullptr, A, nullptr, nullptr);
    if (h->st.scaling <= 0) return build_matrices(h, a, s);             // state, rho indices, g, l, u, c untouched
    // With Ruiz scaling the packed copies are D H D / E A D: a new matrix changes D, E, c, so BOTH raw matrices are needed, and
    // the handle's vectors and state move from the old scaled space to the new one.
    if (!H || !A) return fail_unsupported(h, "rqp_update_mats with scaling needs both H and A (the packed copies are scaled)");
    const size_t nm = h->nmat, nD = nm * h->n, nE = nm * h->m;
    double* old = nullptr;
    HIP_TRY(h, hipMalloc((void**)&old, (nD + nE + nm) * sizeof(double)));
    hipError_t e1 = hipMemcpyAsync(old, h->Dsc, nD * sizeof(double), hipMemcpyDeviceToDevice, s);
    hipError_t e2 = hipMemcpyAsync(old + nD, h->Esc, nE * sizeof(double), hipMemcpyDeviceToDevice, s);
    hipError_t e3 = hipMemcpyAsync(old + nD + nE, h->csc, nm * sizeof(double), hipMemcpyDeviceToDevice, s);
    int rc = (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) ? fail_hip(h, hipErrorUnknown, "copy of the scaling factors") : RQP_OK;
    if (rc == RQP_OK) rc = build_matrices(h, a, s);                      // pack -> Ruiz (new D, E, c) -> gram -> factor -> images
    if (rc == RQP_OK && rqp_launch_rescale(h, old, old + nD, old + nD + nE, s) != hipSuccess) rc = fail_hip(h, hipGetLastError(), "k_rescale");
    (void)hipStreamSynchronize(s);                                       // `old` is freed below
    (void)hipFree(old);
    return rc;
}

int rqp_update(rqp_handle* h, const void* g, const void* l, const void* u, void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    if (!g && !l && !u) return RQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, rqp_launch_vec_update(h, g, l, u, (hipStream_t)stream));
    if (h->st.scaling > 0)
        HIP_TRY(h, rqp_launch_scale_vecs(h, g ? h->g : nullptr, l ? h->l : nullptr, u ? h->u : nullptr, (hipStream_t)stream));
    return RQP_OK;
}

int rqp_update_affine(rqp_handle* h, const void* p, int32_t np, const void* Gg, const void* Glu, const void* l0,
                      const void* u0, void* stream) {
    if (!h || !p || !Gg || !Glu || !l0 || !u0 || np <= 0 || np > 64) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, rqp_launch_affine_update(h, p, np, Gg, Glu, l0, u0, (hipStream_t)stream));
    if (h->st.scaling > 0) HIP_TRY(h, rqp_launch_scale_vecs(h, h->g, h->l, h->u, (hipStream_t)stream));
    return RQP_OK;
}

int rqp_update_settings(rqp_handle* h, const rqp_settings* s) {
    if (!h || !s) return RQP_ERR_ARG;
    const rqp_settings& o = h->st;
    if (s->rho != o.rho || s->rho_min != o.rho_min || s->rho_max != o.rho_max || s->sigma != o.sigma ||
        s->adaptive_rho != o.adaptive_rho || s->adaptive_rho_tolerance != o.adaptive_rho_tolerance ||
        s->eq_tol != o.eq_tol || s->scaling != o.scaling)
        return fail_arg(h, "rqp_update_settings: only max_iter, eps_abs, eps_rel, check_interval, warm_starting, "
                           "check_infeasibility, eps_prim_inf, eps_dual_inf may change");
    if (s->max_iter < 0 || s->check_interval < 1 || s->eps_abs < 0 || s->eps_rel < 0 || s->eps_prim_inf < 0 || s->eps_dual_inf < 0)
        return fail_arg(h, "rqp_update_settings: bad value");
    if (h->windowed && s->check_infeasibility)
        return fail_unsupported(h, "rqp_update_settings: check_infeasibility on a handle set up with a rho-ladder window; "
                                   "pass check_infeasibility (or RQP_FLAG_FULL_LADDER) at setup");
    h->st.eps_rel = s->eps_rel;
    h->st.check_infeasibility = s->check_infeasibility;
    h->st.eps_prim_inf = s->eps_prim_inf;
    h->st.eps_dual_inf = s->eps_dual_inf;
    h->st.max_iter = s->max_iter;
    h->st.eps_abs = s->eps_abs;
    h->st.check_interval = s->check_interval;
    h->st.warm_starting = s->warm_starting;
    return RQP_OK;
}

int rqp_warm_start(rqp_handle* h, const void* x, const void* z, const void* lam, int has_rho, double rho,
                   void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    HIP_TRY(h, hipSetDevice(h->device));
    const int ri = has_rho ? argmin_abs(h->rhos, rho) : 0;          // reluqpth.py:273-274
    HIP_TRY(h, rqp_launch_state_set(h, x, z, lam, has_rho, ri, (hipStream_t)stream));
    if (x || z || lam) h->cold_state = false;   // (a rho alone moves every instance to one index: still the common state)
    if (h->st.scaling > 0 && (x || z || lam))      // caller space -> scaled space
        HIP_TRY(h, rqp_launch_scale_state(h, x ? h->x : nullptr, z ? h->z : nullptr, lam ? h->lam : nullptr, (hipStream_t)stream));
    return RQP_OK;
}

int rqp_clear_primal_dual(rqp_handle* h, void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemsetAsync(h->x, 0, (size_t)h->B * h->n * sizeof(double), s));
    HIP_TRY(h, hipMemsetAsync(h->z, 0, (size_t)h->B * h->m * sizeof(double), s));
    HIP_TRY(h, hipMemsetAsync(h->lam, 0, (size_t)h->B * h->m * sizeof(double), s));
    HIP_TRY(h, rqp_launch_state_set(h, nullptr, nullptr, nullptr, 1, h->rho_ind0, s));
    h->cold_state = true;
    return RQP_OK;
}

// Windowed handles: re-centre and re-factor the windows of the marked instances (cstat = 1): k_rewindow -> K_j of the new
// windows -> their kernel images.  Every kernel filters on cstat, so nothing here needs the host to know which instances.
// gate (fixed-pass protocol): the pass's pending count -- every kernel returns at once when it is 0.
static int refactor_windows(rqp_handle* h, int all, const int32_t* gate, hipStream_t s) {
    HIP_TRY(h, rqp_launch_rewindow(h, all, gate, s));
    SetupArgs f = make_setup_args(h, nullptr, nullptr, nullptr, nullptr, nullptr);
    f.only = h->cstat_d;
    f.gate = gate;
    set_kp_image(h, f);
    HIP_TRY(h, rqp_launch_factor(h, f, s));
    if (uses_res2(h)) HIP_TRY(h, rqp_launch_pack_res2(h, nullptr, h->cstat_d, gate, s));
    return RQP_OK;
}

int rqp_solve(rqp_handle* h, void* x, void* z, void* lam, const rqp_info* info, void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    SolveArgs a = make_solve_args(h);
    a.mode = 0;
    a.cold = h->cold_state ? 1 : 0;
    h->cold_state = !h->st.warm_starting;          // (a cold-start handle clears its state in the kernel)
    a.out_x = x; a.out_z = z; a.out_lam = lam;
    if (info) a.info = *info;
    if (a.info.trace && a.info.trace_cap < 1) return fail_arg(h, "rqp_solve: trace without capacity");
    if (h->order_d && h->last_iter_d && h->use_history) {
        a.order = h->order_valid ? h->order_d : nullptr;
        a.last_iter = h->last_iter_d;
    }
    const bool fixed_passes = h->windowed && h->window_passes > 0;   // rqp_set_window_passes: no host read-back
    if (h->windowed) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (!fixed_passes && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail_unsupported(h, "rqp_solve: a windowed handle synchronises the stream (rho-ladder window); set up with "
                                       "RQP_FLAG_FULL_LADDER, or call rqp_set_window_passes, to capture solves into a HIP graph");
        HIP_TRY(h, hipMemsetAsync(h->ncont_d, 0, sizeof(int32_t), s));
    }
    // Infeasibility certificates: the streaming kernel tests them at every check; the register-resident / MFMA kernels
    // keep their loops untouched and a mode-3 pass of the streaming kernel examines the instances that ran out of iterations.
    const bool post_cert = h->st.check_infeasibility && a.info.status && h->solve_kernel != RQP_K_GENERIC;
    if (post_cert) a.keep_state = 1;
    // Solution polishing reads the final iterate of every instance: with warm_starting = 0 the state is kept through the chain
    // and cleared after the polish kernels (what the solve kernels would have done at their exit).  (On k_admm_mfmal this turns
    // off the regrouped two-launch cold solve, whose exact continuation gives the same results: tests/test_polish_gpu.py.)
    const bool polish = h->polish_reserved && h->polish_on;
    const bool polish_keep = polish && !h->st.warm_starting;
    if (polish_keep) a.keep_state = 1;
    const bool handoff = h->handoff_cols > 0 && a.info.status != nullptr;      // (alloc_handoff: tile kernels backed by k_admm_res2)
    if (handoff) {
        a.handoff_cols = h->handoff_cols;
        a.cont_iter = h->cont_iter_d;
        a.cont_rho = h->cont_rho_d;
        a.keep_state = 1;                           // the continue pass clears what warm_starting = 0 asks to clear
    }
    if (polish) {                                   // (after the choices above, which follow the caller's info): internal buffers for
        if (!a.info.status) a.info.status = h->polish_st_in;                 // the ADMM results polish needs
        if (!a.info.pri_res) a.info.pri_res = h->polish_res_in;
        if (!a.info.dua_res) a.info.dua_res = h->polish_res_in + h->B;
        if (!a.info.obj_val) a.info.obj_val = h->polish_res_in + 2 * h->B;
    }
    HIP_TRY(h, launch_solve(h, a, s));
    if (handoff) {                                  // stragglers finish on the per-instance resident kernel
        SolveArgs c = a;
        c.cont = 1;
        c.handoff_cols = 0;
        c.keep_state = (post_cert || polish_keep) ? 1 : 0;
        c.order = nullptr;
        c.last_iter = nullptr;
        HIP_TRY(h, rqp_kernels[h->aux_kernel].solve(h, c, s));
    }
    const bool ranks = h->order_d && h->last_iter_d && h->use_history;   // rank the instances by what they just needed: next launch goes longest-first
    if (fixed_passes) {
        // The same continuation passes as the host loop below, a fixed number of them, each behind a gate kernel that turns the
        // previous launch's count into the pass's pending count: in a pass with nothing pending every kernel returns after
        // one load.  One linear chain on `s`, no host read-back (capturable).  The ranking runs once, after the finalize
        // kernel (the continuation launches issue in grid order; only the next solve's launch reads the order).
        SolveArgs c = a;
        c.cont = 2;
        c.order = nullptr;
        c.gate = h->ncont_d + 1;
        for (int p = 0; p < h->window_passes; ++p) {
            HIP_TRY(h, rqp_launch_window_gate(h, s));
            const int rc = refactor_windows(h, 0, c.gate, s);
            if (rc != RQP_OK) return rc;
            HIP_TRY(h, launch_solve(h, c, s));
        }
        HIP_TRY(h, rqp_launch_window_finalize(h, a, s));
        if (ranks) {
            HIP_TRY(h, rqp_launch_order_lpt(h, s));
            h->order_valid = true;
        }
    } else if (h->windowed) {
        // instances whose rho index left their window stopped with their exact state: new windows, then they continue
        // (at most one window move per `RQP_WINDOW / 2` index moves, i.e. per >= 2 checks of an instance).  The ranking is
        // enqueued BEFORE the host reads the count (nothing left the window in the common case: the host's wake-up latency
        // then hides behind it) and again after a continuation pass.
        if (ranks) HIP_TRY(h, rqp_launch_order_lpt(h, s));
        for (;;) {
            HIP_TRY(h, hipMemcpyAsync(h->ncont_h, h->ncont_d, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(h, hipStreamSynchronize(s));
            if (*h->ncont_h <= 0) break;
            const int rc = refactor_windows(h, 0, nullptr, s);
            if (rc != RQP_OK) return rc;
            HIP_TRY(h, hipMemsetAsync(h->ncont_d, 0, sizeof(int32_t), s));
            SolveArgs c = a;
            c.cont = 2;
            c.order = nullptr;
            HIP_TRY(h, launch_solve(h, c, s));
            if (ranks) HIP_TRY(h, rqp_launch_order_lpt(h, s));
        }
        if (ranks) h->order_valid = true;
    }
    if (post_cert) {
        SolveArgs c = a;
        c.mode = 3;
        c.order = nullptr;
        c.last_iter = nullptr;
        c.keep_state = polish_keep ? 1 : 0;
        HIP_TRY(h, rqp_launch_solve_generic(h, c, s));
    }
    if (polish) {                                   // before the un-scaling: the polished outputs are in the scaled space
        HIP_TRY(h, rqp_launch_polish(h, a, s));
    } else if (h->polish_reserved) {                // switched off: "not attempted" for every instance
        HIP_TRY(h, hipMemsetAsync(h->polish_status, 0, (size_t)h->B * sizeof(int32_t), s));
        HIP_TRY(h, hipMemsetAsync(h->polish_act, 0, (size_t)h->B * h->m, s));
    }
    if (polish_keep) {                              // clear_primal_dual (reluqpth.py:324-333), as the kernels do with keep_state = 0
        HIP_TRY(h, hipMemsetAsync(h->x, 0, (size_t)h->B * h->n * sizeof(double), s));
        HIP_TRY(h, hipMemsetAsync(h->z, 0, (size_t)h->B * h->m * sizeof(double), s));
        HIP_TRY(h, hipMemsetAsync(h->lam, 0, (size_t)h->B * h->m * sizeof(double), s));
        HIP_TRY(h, rqp_launch_state_set(h, nullptr, nullptr, nullptr, 1, h->rho_ind0, s));
    }
    if (ranks && !h->windowed) {
        HIP_TRY(h, rqp_launch_order_lpt(h, s));
        h->order_valid = true;
    }
    if (h->st.scaling > 0)                          // x = D xb, z = zb / E, lam = E lamb / c, obj / c
        HIP_TRY(h, rqp_launch_unscale_out(h, x, z, lam, a.info.obj_val, s));
    return RQP_OK;
}

int rqp_iterate(rqp_handle* h, int32_t k, void* stream) {
    if (!h || k < 0) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    HIP_TRY(h, hipSetDevice(h->device));
    SolveArgs a = make_solve_args(h);
    a.mode = 1;
    a.max_iter = k;
    h->cold_state = false;
    if (h->windowed) {                              // (test hook: no exit-and-continue here -- every window is centred first)
        const int rc = refactor_windows(h, 1, nullptr, (hipStream_t)stream);
        if (rc != RQP_OK) return rc;
    }
    HIP_TRY(h, launch_solve(h, a, (hipStream_t)stream));
    return RQP_OK;
}

int rqp_compute_residuals(rqp_handle* h, double rho_in, double* pri, double* dua, double* rho_out, double* obj,
                          void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    HIP_TRY(h, hipSetDevice(h->device));
    SolveArgs a = make_solve_args(h);
    a.mode = 2;
    a.rho_in = rho_in;
    a.r_pri = pri; a.r_dua = dua; a.r_rho = rho_out; a.r_obj = obj;
    HIP_TRY(h, launch_solve(h, a, (hipStream_t)stream));
    if (h->st.scaling > 0 && obj) HIP_TRY(h, rqp_launch_unscale_out(h, nullptr, nullptr, nullptr, obj, (hipStream_t)stream));
    return RQP_OK;
}

int rqp_get_state(rqp_handle* h, void* x, void* z, void* lam, int32_t* rho_ind, void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, rqp_launch_state_get(h, x, z, lam, rho_ind, (hipStream_t)stream));
    if (h->st.scaling > 0) HIP_TRY(h, rqp_launch_unscale_out(h, x, z, lam, nullptr, (hipStream_t)stream));
    return RQP_OK;
}

int rqp_get_rhos(const rqp_handle* h, double* rhos, int32_t cap, int32_t* count) {
    if (!h) return RQP_ERR_ARG;
    if (count) *count = h->nrho;
    if (rhos) {
        if (cap < h->nrho) return RQP_ERR_ARG;
        for (int i = 0; i < h->nrho; ++i) rhos[i] = h->rhos[i];
    }
    return RQP_OK;
}

int rqp_get_K(rqp_handle* h, int32_t b, int32_t j, void* out, void* stream) {
    if (!h || !out) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    if (b < 0 || b >= h->B || j < 0 || j >= h->nrho) return fail_arg(h, "rqp_get_K: index out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t mat = h->dims.shared_mats ? 0 : (size_t)b, one = (size_t)h->n * h->ldn;
    if (!h->windowed) {
        HIP_TRY(h, rqp_launch_get_K(h, (const char*)h->K + (mat * h->nrho + j) * one * h->esz, out, s));
        return RQP_OK;
    }
    // windowed handle: the entry may not exist in the table -- factor this one (matrix, rho) pair into a scratch matrix
    void* tmp = nullptr;
    double* fs = nullptr;
    HIP_TRY(h, hipMalloc(&tmp, one * h->esz));
    SetupArgs f = make_setup_args(h, nullptr, nullptr, nullptr, nullptr, nullptr);
    f.nmat = 1;
    f.kwin = 1;
    f.wbase = nullptr;
    f.only = nullptr;
    f.Ht = (char*)h->Ht + mat * one * h->esz;
    f.G = h->G + mat * (size_t)h->n * h->n;
    f.K = tmp;
    f.rhos = h->rhos_d + j;
    int rc = RQP_OK;
    if (h->fscratch) {                              // (large n: the factor kernel works in a global scratch slab)
        if (hipMalloc((void**)&fs, (size_t)h->n * h->n * sizeof(double)) != hipSuccess) rc = RQP_ERR_OOM;
        f.fscratch = fs;
    }
    if (rc == RQP_OK && rqp_launch_factor(h, f, s) != hipSuccess) rc = fail_hip(h, hipGetLastError(), "factor (rqp_get_K)");
    if (rc == RQP_OK && rqp_launch_get_K(h, tmp, out, s) != hipSuccess) rc = fail_hip(h, hipGetLastError(), "k_get_K");
    (void)hipStreamSynchronize(s);
    (void)hipFree(tmp);
    if (fs) (void)hipFree(fs);
    return rc;
}

int rqp_get_window(rqp_handle* h, int32_t* slots, int32_t* wbase, void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    if (slots) *slots = h->kwin;
    if (wbase && h->windowed) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpyAsync(wbase, h->wbase_d, (size_t)h->nmat * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return RQP_OK;
}

int rqp_set_window_passes(rqp_handle* h, int32_t passes) {
    if (!h) return RQP_ERR_ARG;
    if (passes < 0) return fail_arg(h, "rqp_set_window_passes: passes < 0");
    h->window_passes = passes;
    return RQP_OK;
}

int rqp_set_polish(rqp_handle* h, int32_t enable, double delta, int32_t refine_iter) {
    if (!h) return RQP_ERR_ARG;
    if (!(delta > 0) || refine_iter < 0) return fail_arg(h, "rqp_set_polish: delta <= 0 or refine_iter < 0");
    if (!h->is_setup) {                             // before rqp_setup: reserve (or not) the workspace
        h->polish_reserved = h->polish_on = enable != 0;
        h->polish_delta = delta;
        h->polish_refine = refine_iter;
        return RQP_OK;
    }
    if (!h->polish_reserved)
        return fail_state(h, "rqp_set_polish: the handle was set up without polish (call rqp_set_polish before rqp_setup)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (delta != h->polish_delta) {
        const double idel = 1.0 / delta;
        HIP_TRY(h, hipMemcpy(h->polish_rho, &idel, sizeof(double), hipMemcpyHostToDevice));
    }
    h->polish_on = enable != 0;
    h->polish_delta = delta;
    h->polish_refine = refine_iter;
    return RQP_OK;
}

int rqp_get_polish(rqp_handle* h, int32_t* status_polish, int8_t* active, void* stream) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup || !h->polish_reserved) return fail_state(h, "rqp_get_polish: the handle was not set up with polish");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (status_polish)
        HIP_TRY(h, hipMemcpyAsync(status_polish, h->polish_status, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (active) HIP_TRY(h, hipMemcpyAsync(active, h->polish_act, (size_t)h->B * h->m, hipMemcpyDeviceToDevice, s));
    return RQP_OK;
}

int rqp_set_adjoint(rqp_handle* h, int32_t enable, double delta, int32_t refine_iter) {
    if (!h) return RQP_ERR_ARG;
    if (!(delta > 0) || refine_iter < 0) return fail_arg(h, "rqp_set_adjoint: delta <= 0 or refine_iter < 0");
    if (!h->is_setup) {                             // before rqp_setup: reserve (or not) the workspace
        h->adj_reserved = enable != 0;
        h->adj_delta = delta;
        h->adj_refine = refine_iter;
        return RQP_OK;
    }
    if (!h->adj_reserved && !h->sens_reserved)      // (delta and refine_iter are the sensitivities' too)
        return fail_state(h, "rqp_set_adjoint: the handle was set up without the adjoint (call rqp_set_adjoint before rqp_setup)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (delta != h->adj_delta) {
        const double idel = 1.0 / delta;
        HIP_TRY(h, hipMemcpy(h->adj_rho, &idel, sizeof(double), hipMemcpyHostToDevice));
    }
    h->adj_delta = delta;
    h->adj_refine = refine_iter;
    return RQP_OK;
}

int rqp_adjoint(rqp_handle* h, const rqp_adjoint_io* io, void* stream) {
    if (!h || !io) return RQP_ERR_ARG;
    if (!io->dx || !io->x || !io->y || !io->H || !io->A) return fail_arg(h, "rqp_adjoint: dx, x, y, H and A are required");
    if (!io->active && (!io->z || !io->l || !io->u))
        return fail_arg(h, "rqp_adjoint: z, l and u are required when no active set is given");
    if (!h->is_setup || !h->adj_reserved)
        return fail_state(h, "rqp_adjoint: the handle was not set up with the adjoint (rqp_set_adjoint before rqp_setup)");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, rqp_launch_adjoint(h, *io, (hipStream_t)stream));
    return RQP_OK;
}

int rqp_set_sensitivity(rqp_handle* h, int32_t enable) {
    if (!h) return RQP_ERR_ARG;
    if (!h->is_setup) {                             // before rqp_setup: reserve (or not) the workspace
        h->sens_reserved = enable != 0;
        return RQP_OK;
    }
    if (h->sens_reserved != (enable != 0))
        return fail_state(h, "rqp_set_sensitivity: the reservation is fixed at rqp_setup (call rqp_set_sensitivity before it)");
    return RQP_OK;
}

int rqp_sensitivity(rqp_handle* h, const rqp_sensitivity_io* io, void* stream) {
    if (!h || !io) return RQP_ERR_ARG;
    if (!io->dx || !io->x || !io->y || !io->H || !io->A) return fail_arg(h, "rqp_sensitivity: dx, x, y, H and A are required");
    if (io->ndir < 1) return fail_arg(h, "rqp_sensitivity: ndir < 1");
    if (!io->active && (!io->z || !io->l || !io->u))
        return fail_arg(h, "rqp_sensitivity: z, l and u are required when no active set is given");
    if (!h->is_setup || !h->sens_reserved)
        return fail_state(h, "rqp_sensitivity: the handle was not set up with sensitivities (rqp_set_sensitivity before rqp_setup)");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, rqp_launch_sensitivity(h, *io, (hipStream_t)stream));
    return RQP_OK;
}

int rqp_dispatch_history(rqp_handle* h, int32_t mode) {
    if (!h || mode < 0 || mode > 2) return RQP_ERR_ARG;
    h->order_valid = false;
    if (mode != 2) h->use_history = mode == 1;
    return RQP_OK;
}

int rqp_get_dispatch(rqp_handle* h, int32_t* order, int32_t* last_iter, int32_t* valid, void* stream) {
    if (!h || !valid) return RQP_ERR_ARG;
    if (!h->is_setup) return RQP_ERR_STATE;
    *valid = (h->order_d && h->order_valid) ? 1 : 0;
    if (!*valid) return RQP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nb = (size_t)h->B * sizeof(int32_t);
    if (order) HIP_TRY(h, hipMemcpyAsync(order, h->order_d, nb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (last_iter) HIP_TRY(h, hipMemcpyAsync(last_iter, h->last_iter_d, nb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RQP_OK;
}

const char* rqp_kernel_name(const rqp_handle* h) { return h ? rqp_kernels[h->solve_kernel].name : ""; }

const char* rqp_strerror(int err) {
    switch (err) {
        case RQP_OK: return "ok";
        case RQP_ERR_ARG: return "invalid argument";
        case RQP_ERR_STATE: return "invalid call order (setup first)";
        case RQP_ERR_HIP: return "HIP runtime error";
        case RQP_ERR_OOM: return "out of device memory";
        case RQP_ERR_UNSUPPORTED: return "unsupported";
        default: return "unknown error";
    }
}

// ---- LTV condensing: handle-less (the product is plain tensors); a failure's text is kept per host thread
static thread_local std::string ltv_err;
static int ltv_fail(int code, const std::string& what) {
    ltv_err = what;
    return code;
}
static int ltv_check(const rqp_ltv_dims* d, const char* fn) {
    if (const char* w = rqp_ltv_check_dims(d)) return ltv_fail(RQP_ERR_ARG, std::string(fn) + ": " + w);
    if (const char* w = rqp_ltv_check_size(d)) return ltv_fail(RQP_ERR_UNSUPPORTED, std::string(fn) + ": " + w);
    return RQP_OK;
}
// The launches run with `device` current; the calling thread's current device is put back afterwards (LtvDevice's destructor).
struct LtvDevice {
    int prev = -1;
    int enter(int device, const char* fn) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
            return ltv_fail(RQP_ERR_HIP, std::string(fn) + ": no such HIP device");
        int cur = 0;
        hipError_t e = hipGetDevice(&cur);
        if (e == hipSuccess && cur != device) {
            e = hipSetDevice(device);
            if (e == hipSuccess) prev = cur;
        }
        if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
        return RQP_OK;
    }
    ~LtvDevice() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int rqp_ltv_workspace_bytes(const rqp_ltv_dims* dims, size_t* bytes) {
    ltv_err.clear();
    if (!bytes) return ltv_fail(RQP_ERR_ARG, "rqp_ltv_workspace_bytes: bytes is NULL");
    if (int rc = ltv_check(dims, "rqp_ltv_workspace_bytes")) return rc;
    *bytes = rqp_ltv_ws_bytes(dims);
    return RQP_OK;
}

int rqp_ltv_condense(const rqp_ltv_dims* dims, int device, const void* Ad, const void* Bd, const void* c, const double* Q,
                     const double* R, const double* Qf, const double* K, void* H, void* A, void* workspace, void* stream) {
    ltv_err.clear();
    if (int rc = ltv_check(dims, "rqp_ltv_condense")) return rc;
    const bool staged = (dims->flags & RQP_LTV_STAGE_WEIGHTS) != 0;      // Q, R per (instance, stage); Qf is not read
    if (!Ad || !Bd || !Q || !R || (!Qf && !staged) || !H || !A || !workspace)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_condense: Ad, Bd, Q, R, Qf, H, A and workspace are required");
    if (((dims->flags & RQP_LTV_HAS_K) && !K) || ((dims->flags & RQP_LTV_HAS_C) && !c))
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_condense: a flag names an input whose pointer is NULL");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_condense")) return rc;
    hipError_t e = rqp_ltv_launch_condense(dims, Ad, Bd, c, Q, R, Qf, K, H, A, workspace, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_condense: ") + hipGetErrorString(e));
    return RQP_OK;
}

int rqp_ltv_vectors(const rqp_ltv_dims* dims, int device, const void* x0, const void* xref, const void* uref, const void* l_add,
                    const void* u_add, const double* Q, const double* R, const double* Qf, const void* workspace, void* g, void* l,
                    void* u, void* stream) {
    ltv_err.clear();
    if (int rc = ltv_check(dims, "rqp_ltv_vectors")) return rc;
    const bool staged = (dims->flags & RQP_LTV_STAGE_WEIGHTS) != 0;
    if (!x0 || !l_add || !u_add || !Q || !R || (!Qf && !staged) || !workspace || !g || !l || !u)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_vectors: x0, l_add, u_add, Q, R, Qf, workspace, g, l and u are required");
    if (((dims->flags & RQP_LTV_HAS_XREF) && !xref) || ((dims->flags & RQP_LTV_HAS_UREF) && !uref))
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_vectors: a flag names an input whose pointer is NULL");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_vectors")) return rc;
    hipError_t e = rqp_ltv_launch_vectors(dims, x0, (dims->flags & RQP_LTV_HAS_XREF) ? xref : nullptr,
                                          (dims->flags & RQP_LTV_HAS_UREF) ? uref : nullptr, l_add, u_add, Q, R, Qf, workspace, g, l,
                                          u, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_vectors: ") + hipGetErrorString(e));
    return RQP_OK;
}

int rqp_ltv_adjoint_workspace_bytes(const rqp_ltv_dims* dims, size_t* bytes) {
    ltv_err.clear();
    if (!bytes) return ltv_fail(RQP_ERR_ARG, "rqp_ltv_adjoint_workspace_bytes: bytes is NULL");
    if (int rc = ltv_check(dims, "rqp_ltv_adjoint_workspace_bytes")) return rc;
    *bytes = rqp_ltv_adj_ws_bytes(dims);
    return RQP_OK;
}

int rqp_ltv_condense_adjoint(const rqp_ltv_dims* dims, int device, const rqp_ltv_adjoint_io* io, void* stream) {
    ltv_err.clear();
    if (int rc = ltv_check(dims, "rqp_ltv_condense_adjoint")) return rc;
    const bool staged = (dims->flags & RQP_LTV_STAGE_WEIGHTS) != 0;
    if (!io || !io->Ad || !io->Bd || !io->x0 || !io->Q || !io->R || (!io->Qf && !staged) || !io->workspace || !io->adjoint_workspace)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_condense_adjoint: io, Ad, Bd, x0, Q, R, Qf, workspace and adjoint_workspace are required");
    if (staged && io->dQf)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_condense_adjoint: RQP_LTV_STAGE_WEIGHTS has no Qf, dQf must be NULL (the terminal "
                                     "block's gradient is dQ[b][horizon - 1])");
    if (((dims->flags & RQP_LTV_HAS_K) && !io->K) || ((dims->flags & RQP_LTV_HAS_XREF) && !io->xref) ||
        ((dims->flags & RQP_LTV_HAS_UREF) && !io->uref))
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_condense_adjoint: a flag names an input whose pointer is NULL");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_condense_adjoint")) return rc;
    hipError_t e = rqp_ltv_launch_condense_adjoint(dims, io, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_condense_adjoint: ") + hipGetErrorString(e));
    return RQP_OK;
}

// Stage constraints: dims as in the calls above plus RQP_LTV_STAGE_SHARED_E, a flag of these three entry points alone (the
// shared checks see the dims without it, so they keep refusing it everywhere else).
static int ltv_stage_check(const rqp_ltv_dims* dims, int32_t nc, const char* fn) {
    if (!dims) return ltv_fail(RQP_ERR_ARG, std::string(fn) + ": dims is NULL");
    rqp_ltv_dims d = *dims;
    d.flags &= ~RQP_LTV_STAGE_SHARED_E;
    if (int rc = ltv_check(&d, fn)) return rc;
    if (const char* w = rqp_ltv_stage_check_size(dims, nc)) return ltv_fail(RQP_ERR_UNSUPPORTED, std::string(fn) + ": " + w);
    return RQP_OK;
}

int rqp_ltv_stage_rows(const rqp_ltv_dims* dims, int device, int32_t nc, const void* E, const void* workspace, void* A_c,
                       void* stream) {
    ltv_err.clear();
    if (int rc = ltv_stage_check(dims, nc, "rqp_ltv_stage_rows")) return rc;
    if (!E || !workspace || !A_c) return ltv_fail(RQP_ERR_ARG, "rqp_ltv_stage_rows: E, workspace and A_c are required");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_stage_rows")) return rc;
    hipError_t e = rqp_ltv_launch_stage_rows(dims, nc, E, workspace, A_c, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_stage_rows: ") + hipGetErrorString(e));
    return RQP_OK;
}

int rqp_ltv_stage_vectors(const rqp_ltv_dims* dims, int device, int32_t nc, const void* E, const void* x0, const void* lo,
                          const void* hi, const void* workspace, void* l_c, void* u_c, void* stream) {
    ltv_err.clear();
    if (int rc = ltv_stage_check(dims, nc, "rqp_ltv_stage_vectors")) return rc;
    if (!E || !x0 || !lo || !hi || !workspace || !l_c || !u_c)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_stage_vectors: E, x0, lo, hi, workspace, l_c and u_c are required");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_stage_vectors")) return rc;
    hipError_t e = rqp_ltv_launch_stage_vectors(dims, nc, E, x0, lo, hi, workspace, l_c, u_c, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_stage_vectors: ") + hipGetErrorString(e));
    return RQP_OK;
}

int rqp_ltv_stage_adjoint(const rqp_ltv_dims* dims, int device, int32_t nc, const rqp_ltv_stage_adjoint_io* io, void* stream) {
    ltv_err.clear();
    if (int rc = ltv_stage_check(dims, nc, "rqp_ltv_stage_adjoint")) return rc;
    if (!io || !io->E || !io->x0 || !io->workspace)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_stage_adjoint: io, E, x0 and workspace are required");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_stage_adjoint")) return rc;
    hipError_t e = rqp_ltv_launch_stage_adjoint(dims, nc, io, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_stage_adjoint: ") + hipGetErrorString(e));
    return RQP_OK;
}

// Input rates: the dims and flags of the plain calls; sizes checked against the rate kernels' own limits as well.
static int ltv_rate_check(const rqp_ltv_dims* dims, const char* fn) {
    if (int rc = ltv_check(dims, fn)) return rc;
    if (const char* w = rqp_ltv_rate_check_size(dims)) return ltv_fail(RQP_ERR_UNSUPPORTED, std::string(fn) + ": " + w);
    return RQP_OK;
}
// The N nu rows of one instance lie inst_stride elements after those of the one before: at least their own size, and with
// whatever the caller keeps in front of them no more than m = 640 rows.
static int ltv_rate_stride(const rqp_ltv_dims* dims, int64_t inst_stride, int64_t row_len, const char* fn) {
    const int64_t rows = (int64_t)dims->horizon * dims->nu;
    if (inst_stride < rows * row_len)
        return ltv_fail(RQP_ERR_ARG, std::string(fn) + ": inst_stride is smaller than the horizon nu rows of one instance");
    if (inst_stride > 640 * row_len)
        return ltv_fail(RQP_ERR_UNSUPPORTED, std::string(fn) + ": inst_stride spans more than m = 640 rows per instance");
    return RQP_OK;
}

int rqp_ltv_condense_rate(const rqp_ltv_dims* dims, int device, const void* Ad, const void* Bd, const void* c, const double* Q,
                          const double* R, const double* Qf, const double* K, const double* S, void* H, void* A, void* workspace,
                          void* stream) {
    ltv_err.clear();
    if (int rc = ltv_rate_check(dims, "rqp_ltv_condense_rate")) return rc;
    const bool staged = (dims->flags & RQP_LTV_STAGE_WEIGHTS) != 0;
    if (!Ad || !Bd || !Q || !R || (!Qf && !staged) || !S || !H || !A || !workspace)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_condense_rate: Ad, Bd, Q, R, Qf, S, H, A and workspace are required");
    if (((dims->flags & RQP_LTV_HAS_K) && !K) || ((dims->flags & RQP_LTV_HAS_C) && !c))
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_condense_rate: a flag names an input whose pointer is NULL");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_condense_rate")) return rc;
    hipError_t e = rqp_ltv_launch_condense_rate(dims, Ad, Bd, c, Q, R, Qf, K, S, H, A, workspace, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_condense_rate: ") + hipGetErrorString(e));
    return RQP_OK;
}

int rqp_ltv_vectors_rate(const rqp_ltv_dims* dims, int device, const void* x0, const void* xref, const void* uref,
                         const void* l_add, const void* u_add, const double* Q, const double* R, const double* Qf, const double* S,
                         const void* uprev, const void* workspace, void* g, void* l, void* u, void* stream) {
    ltv_err.clear();
    if (int rc = ltv_rate_check(dims, "rqp_ltv_vectors_rate")) return rc;
    const bool staged = (dims->flags & RQP_LTV_STAGE_WEIGHTS) != 0;
    if (!x0 || !l_add || !u_add || !Q || !R || (!Qf && !staged) || !S || !uprev || !workspace || !g || !l || !u)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_vectors_rate: x0, l_add, u_add, Q, R, Qf, S, uprev, workspace, g, l and u are required");
    if (((dims->flags & RQP_LTV_HAS_XREF) && !xref) || ((dims->flags & RQP_LTV_HAS_UREF) && !uref))
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_vectors_rate: a flag names an input whose pointer is NULL");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_vectors_rate")) return rc;
    hipError_t e = rqp_ltv_launch_vectors_rate(dims, x0, (dims->flags & RQP_LTV_HAS_XREF) ? xref : nullptr,
                                               (dims->flags & RQP_LTV_HAS_UREF) ? uref : nullptr, l_add, u_add, Q, R, Qf, S, uprev,
                                               workspace, g, l, u, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_vectors_rate: ") + hipGetErrorString(e));
    return RQP_OK;
}

int rqp_ltv_rate_rows(const rqp_ltv_dims* dims, int device, const void* workspace, void* A_r, int64_t inst_stride, void* stream) {
    ltv_err.clear();
    if (int rc = ltv_rate_check(dims, "rqp_ltv_rate_rows")) return rc;
    if (int rc = ltv_rate_stride(dims, inst_stride, (int64_t)dims->horizon * dims->nu, "rqp_ltv_rate_rows")) return rc;
    if (!workspace || !A_r) return ltv_fail(RQP_ERR_ARG, "rqp_ltv_rate_rows: workspace and A_r are required");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_rate_rows")) return rc;
    hipError_t e = rqp_ltv_launch_rate_rows(dims, workspace, A_r, inst_stride, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_rate_rows: ") + hipGetErrorString(e));
    return RQP_OK;
}

int rqp_ltv_rate_bounds(const rqp_ltv_dims* dims, int device, const void* x0, const void* uprev, const void* dlo, const void* dhi,
                        const void* workspace, void* l_r, void* u_r, int64_t inst_stride, void* stream) {
    ltv_err.clear();
    if (int rc = ltv_rate_check(dims, "rqp_ltv_rate_bounds")) return rc;
    if (int rc = ltv_rate_stride(dims, inst_stride, 1, "rqp_ltv_rate_bounds")) return rc;
    if (!x0 || !uprev || !dlo || !dhi || !workspace || !l_r || !u_r)
        return ltv_fail(RQP_ERR_ARG, "rqp_ltv_rate_bounds: x0, uprev, dlo, dhi, workspace, l_r and u_r are required");
    LtvDevice on;
    if (int rc = on.enter(device, "rqp_ltv_rate_bounds")) return rc;
    hipError_t e = rqp_ltv_launch_rate_bounds(dims, x0, uprev, dlo, dhi, workspace, l_r, u_r, inst_stride, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string("rqp_ltv_rate_bounds: ") + hipGetErrorString(e));
    return RQP_OK;
}

int rqp_ltv_adjoint_rate_workspace_bytes(const rqp_ltv_dims* dims, size_t* bytes) {
    ltv_err.clear();
    if (!bytes) return ltv_fail(RQP_ERR_ARG, "rqp_ltv_adjoint_rate_workspace_bytes: bytes is NULL");
    if (int rc = ltv_rate_check(dims, "rqp_ltv_adjoint_rate_workspace_bytes")) return rc;
    *bytes = rqp_ltv_rate_adj_ws_bytes(dims);
    return RQP_OK;
}

int rqp_ltv_condense_adjoint_rate(const rqp_ltv_dims* dims, int device, const rqp_ltv_adjoint_io* io,
                                  const rqp_ltv_rate_adjoint_io* rate_io, void* stream) {
    const char* fn = "rqp_ltv_condense_adjoint_rate";
    ltv_err.clear();
    if (int rc = ltv_rate_check(dims, fn)) return rc;
    const bool staged = (dims->flags & RQP_LTV_STAGE_WEIGHTS) != 0;
    if (!io || !io->Ad || !io->Bd || !io->x0 || !io->Q || !io->R || (!staged && !io->Qf) || !io->workspace || !io->adjoint_workspace)
        return ltv_fail(RQP_ERR_ARG, std::string(fn) + ": io, Ad, Bd, x0, Q, R, Qf, workspace and adjoint_workspace are required");
    if (!rate_io || !rate_io->S || !rate_io->uprev)
        return ltv_fail(RQP_ERR_ARG, std::string(fn) + ": rate_io, S and uprev are required");
    if (staged && io->dQf)
        return ltv_fail(RQP_ERR_ARG, std::string(fn) + ": RQP_LTV_STAGE_WEIGHTS has no Qf, dQf must be NULL (the terminal "
                                     "weight's gradient is the last stage of dQ)");
    if (((dims->flags & RQP_LTV_HAS_K) && !io->K) || ((dims->flags & RQP_LTV_HAS_XREF) && !io->xref) ||
        ((dims->flags & RQP_LTV_HAS_UREF) && !io->uref))
        return ltv_fail(RQP_ERR_ARG, std::string(fn) + ": a flag names an input whose pointer is NULL");
    if (rate_io->dA_r)
        if (int rc = ltv_rate_stride(dims, rate_io->dA_stride, (int64_t)dims->horizon * dims->nu, fn)) return rc;
    if (rate_io->dl_r || rate_io->du_r)
        if (int rc = ltv_rate_stride(dims, rate_io->dl_stride, 1, fn)) return rc;
    LtvDevice on;
    if (int rc = on.enter(device, fn)) return rc;
    hipError_t e = rqp_ltv_launch_condense_adjoint_rate(dims, io, rate_io, (hipStream_t)stream);
    if (e != hipSuccess) return ltv_fail(RQP_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
    return RQP_OK;
}

const char* rqp_last_error(const rqp_handle* h) { return h ? h->err.c_str() : ltv_err.c_str(); }

const char* rqp_version(void) { return RQP_VERSION; }

}  // extern "C"
