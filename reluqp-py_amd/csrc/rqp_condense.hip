// rqp_condense.hip -- condensed MPC QPs of a batch of linear time-varying plants, built on the device
// (rqp_ltv_condense / rqp_ltv_vectors, DESIGN.md section 5 "LTV condensing").
//
// Per instance, stages k = 0 .. N-1:  x_{k+1} = A_k x_k + B_k u_k + c_k,  u_k = -K x_k + v_k  (K shared, may be zero).
// With Acl_k = A_k - B_k K and y = [u_0, x_1, u_1, x_2, ..., u_{N-1}, x_N] (m = N (nu + nx) rows), v = [v_0 .. v_{N-1}] (n = N nu):
//     y = F v + G x0 + f,
//     H = sym(F' H_sp F),  A = F,  g = F' H_sp (G x0 + f - yref),  l / u = l_add / u_add - (G x0 + f),
// H_sp = blkdiag(R, Q, ..., R, Qf) (Q, R, Qf symmetric).  All arithmetic is float64; every output is written once, in T.
// RQP_LTV_STAGE_WEIGHTS: H_sp = blkdiag(R_0, Q_0, ..., R_{N-1}, Q_{N-1}) per instance, Q [B][N][nx][nx], R [B][N][nu][nu], Qf not
// read (DESIGN.md section 5 "LTV condensing, stage weights").  The weight source is a template parameter (STAGED) of the kernels
// that read weights: the shared-weight instantiations are the kernels they were.
//
// Three kernels:
//   k_ltv_transition  one workgroup per instance, ONE THREAD PER COLUMN of [F | G | f] (n + nx + 1 chains).  Column j nu + c
//                     of F is the response to a unit v_j[c]: zero before stage j, (e_c, B_j e_c) at stage j, then
//                     (u, x) <- (-K x, Acl_k x).  G's column i is the same chain started from x_0 = e_i at stage 0, f the one
//                     started from 0 and driven by c_k.  The chains of different columns are independent; all of them read
//                     the same Acl_k (LDS, zero-padded to NXP x NXP, broadcast reads).  A thread keeps its x in registers and
//                     writes one entry of every row: the lanes of a wave write adjacent columns of one row (coalesced).
//                     It writes A = F (T), F and W = H_sp F (float64 workspace; the block product is on the thread's own
//                     column) and [G | f] (float64 workspace, [m][nx + 1]).
//   k_ltv_hess        H = sym(W' F) and [F' H_sp G | F' H_sp f] = W' [G | f] on v_mfma_f64_16x16x4_f64, one wave per pair of
//                     16 x 16 output tiles of one tile row I (upper tiles J >= I only, plus the [G | f] tiles).  Operand
//                     lanes as in k_gram_mfma (rqp_setup.hip): lane (kq, i16) holds W[k0 + kq][16 I + i16] (A operand) and
//                     F[k0 + kq][16 J + i16] (B operand), straight from global memory with clamped indices.  Column block j
//                     of F is zero above row j (nu + nx): the k loop of tile (I, J) starts at floor(16 J / nu) (nu + nx),
//                     known from (N, nx, nu) alone.
//   k_ltv_vectors     s = G x0 + f, l / u = l_add / u_add - s, g = (F' H_sp G) x0 + F' H_sp f - F' (H_sp yref): one pass over
//                     [G | f] (and over F when references are given), no matrix products of the condensing repeated.
// Input rates (rqp_ltv_condense_rate / rqp_ltv_vectors_rate, DESIGN.md section 5 "LTV condensing, input rates"): k_rate_w
// (rqp_rate.hip) amends W between the first two kernels; k_ltv_hess<T, true> and k_ltv_vectors<T, STAGED, LtvRateArgs> are for those
// calls alone, the plain calls launch the kernels they always did.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "rqp_common.h"

namespace {

typedef double cd4 __attribute__((ext_vector_type(4)));
constexpr int LTV_NUP = 8;        // nu padded (register arrays)

// Stage weights are read straight from global memory.  Every lane of the workgroup reads the same entry of the same block, and
// the kernels never write the weights: through the constant address space such a load is a scalar load (one per wave, SGPR
// operands of the FMAs), not 64 vector lanes of the same address.
typedef const __attribute__((address_space(4))) double* ltv_kptr;
__device__ __forceinline__ ltv_kptr ltv_uniform(const double* p) { return (ltv_kptr)p; }

struct LtvArgs {
    int B, nx, nu, N, n, m, blk, has_c, has_K, lu_batched;
    const void *Ad, *Bd, *c;                 // [B][N][nx][nx], [B][N][nx][nu], [B][N][nx] (T)
    const double *Q, *R, *Qf, *K;            // [nx][nx], [nu][nu], [nx][nx], [nu][nx] (K NULL: zero); STAGED: Q [B][N][nx][nx],
                                             // R [B][N][nu][nu], Qf not read
    void *H, *A;                             // [B][n][n], [B][m][n] (T)
    double *F, *W, *Gf, *gmap;               // workspace: [B][m][n], [B][m][n], [B][m][nx + 1], [B][n][nx + 1]
    const void *x0, *xref, *uref, *ladd, *uadd;   // [B][nx], [B][N][nx], [B][N][nu], [m] | [B][m]
    void *g, *l, *u;                         // [B][n], [B][m], [B][m] (T)
};

// ------------------------------------------------------------------------------------------------------------- transition
// LDS (doubles): Acl [N][NXP][NXP], K [NUP][NXP], R [NUP][NUP], Q [NXP][NXP], Qf [NXP][NXP], all zero-padded (every inner product
// has compile-time bounds and the padding contributes exact zeros), then the threads' state columns [NXP + NUP][threads].
// STAGED: no R, Q, Qf in LDS (all stages of an instance would not fit beside Acl at the limit shape, and a per-stage slot would
// need a barrier inside the stage loop, after the surplus threads have returned).  Stage k's blocks are read from global memory
// at wave-uniform addresses instead (ltv_uniform); the inner products keep their compile-time bounds and their order, the
// padding terms multiply an exact zero as they do in LDS, so repeated shared blocks give the shared kernel's bits.
template <typename T, int NXP, bool STAGED>
__global__ void __launch_bounds__(192) k_ltv_transition(LtvArgs a) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, blk = a.blk, nxa = nx + 1;
    double* Acl = lds;
    double* Ks = Acl + (size_t)N * NXP * NXP;
    double* Rs = Ks + LTV_NUP * NXP;
    double* Qs = Rs + LTV_NUP * LTV_NUP;
    double* Qfs = Qs + NXP * NXP;
    const T* Ad = (const T*)a.Ad + (size_t)b * N * nx * nx;
    const T* Bd = (const T*)a.Bd + (size_t)b * N * nx * nu;

    for (int e = tid; e < LTV_NUP * NXP; e += nt) {
        const int r = e / NXP, i = e % NXP;
        Ks[e] = (a.has_K && r < nu && i < nx) ? a.K[r * nx + i] : 0.0;
    }
    if constexpr (!STAGED) {
        for (int e = tid; e < LTV_NUP * LTV_NUP; e += nt) {
            const int r = e / LTV_NUP, s = e % LTV_NUP;
            Rs[e] = (r < nu && s < nu) ? a.R[r * nu + s] : 0.0;
        }
        for (int e = tid; e < NXP * NXP; e += nt) {
            const int r = e / NXP, i = e % NXP;
            const bool in = r < nx && i < nx;
            Qs[e] = in ? a.Q[r * nx + i] : 0.0;
            Qfs[e] = in ? a.Qf[r * nx + i] : 0.0;
        }
    }
    __syncthreads();
    for (int e = tid; e < N * NXP * NXP; e += nt) {                      // Acl_k = A_k - B_k K
        const int k = e / (NXP * NXP), r = (e / NXP) % NXP, i = e % NXP;
        double v = 0.0;
        if (r < nx && i < nx) {
            v = (double)Ad[((size_t)k * nx + r) * nx + i];
            if (a.has_K)
                for (int s = 0; s < nu; ++s) v -= (double)Bd[((size_t)k * nx + r) * nu + s] * Ks[s * NXP + i];
        }
        Acl[e] = v;
    }
    __syncthreads();

    const int col = tid;
    if (col >= n + nxa) return;
    const bool isF = col < n, isf = col == n + nx;
    const int j = isF ? col / nu : -1, cc = isF ? col % nu : 0;          // the chain starts at stage j (G, f: before stage 0)
    // The thread's state lives twice: x, uu in registers (compile-time indices: the operands of the unrolled inner products) and
    // in its own LDS column xl, ul (run-time row index r of the rolled row loops).  Rolled rows keep the kernel at a few dozen
    // VGPRs; fully unrolled, the NXP^2 LDS reads of a stage were scheduled ahead of their use and spilled.
    double* xl = (STAGED ? Rs : Qfs + NXP * NXP) + tid;                  // xl[r * nt], r < NXP
    double* ul = xl + (size_t)NXP * nt;                                  // ul[r * nt], r < NUP
    double x[NXP], uu[LTV_NUP];
#pragma unroll
    for (int i = 0; i < NXP; ++i) {
        x[i] = (!isF && !isf && i == col - n) ? 1.0 : 0.0;
        xl[i * nt] = x[i];
    }
#pragma unroll
    for (int r = 0; r < LTV_NUP; ++r) ul[r * nt] = 0.0;
    const T* cv = a.has_c ? (const T*)a.c + (size_t)b * N * nx : nullptr;
    T* Ao = (T*)a.A + (size_t)b * a.m * n;
    double* Fo = a.F + (size_t)b * a.m * n;
    double* Wo = a.W + (size_t)b * a.m * n;
    double* Go = a.Gf + (size_t)b * a.m * nxa;

    for (int k = 0; k < N; ++k) {
        const double* Ak = Acl + (size_t)k * NXP * NXP;
        if (k == j) {                                                    // unit input v_j[cc]
            ul[cc * nt] = 1.0;
            for (int r = 0; r < nx; ++r) xl[r * nt] = (double)Bd[((size_t)k * nx + r) * nu + cc];
        } else if (k > j) {
#pragma unroll 1
            for (int r = 0; r < nu; ++r) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < NXP; ++i) s -= Ks[r * NXP + i] * x[i];
                ul[r * nt] = s;
            }
#pragma unroll 1
            for (int r = 0; r < nx; ++r) {
                double s = (isf && a.has_c) ? (double)cv[(size_t)k * nx + r] : 0.0;
#pragma unroll
                for (int i = 0; i < NXP; ++i) s += Ak[r * NXP + i] * x[i];
                xl[r * nt] = s;
            }
        }                                                                // (k < j: above the block diagonal, the state is still zero)
#pragma unroll
        for (int i = 0; i < NXP; ++i) x[i] = xl[i * nt];
#pragma unroll
        for (int r = 0; r < LTV_NUP; ++r) uu[r] = ul[r * nt];
        const size_t row0 = (size_t)k * blk;
        if (isF) {
            size_t o = row0 * n + col;                                   // one running offset: rows are n apart
            if constexpr (STAGED) {
                const ltv_kptr Rk = ltv_uniform(a.R + ((size_t)b * N + k) * nu * nu);
                const ltv_kptr Qk = ltv_uniform(a.Q + ((size_t)b * N + k) * nx * nx);
#pragma unroll 1
                for (int r = 0; r < nu; ++r) {
                    double w = 0.0;
#pragma unroll
                    for (int s = 0; s < LTV_NUP; ++s) {                  // index clamped into the row, a padding term switched off
                        const double q = Rk[r * nu + min(s, nu - 1)];
                        w += (s < nu ? q : 0.0) * uu[s];
                    }
                    const double v = ul[r * nt];
                    Ao[o] = (T)v;
                    Fo[o] = v;
                    Wo[o] = w;
                    o += n;
                }
#pragma unroll 1
                for (int r = 0; r < nx; ++r) {
                    double w = 0.0;
#pragma unroll
                    for (int i = 0; i < NXP; ++i) {
                        const double q = Qk[r * nx + min(i, nx - 1)];
                        w += (i < nx ? q : 0.0) * x[i];
                    }
                    const double v = xl[r * nt];
                    Ao[o] = (T)v;
                    Fo[o] = v;
                    Wo[o] = w;
                    o += n;
                }
            } else {
                const double* Qk = (k == N - 1) ? Qfs : Qs;
#pragma unroll 1
                for (int r = 0; r < nu; ++r) {
                    double w = 0.0;
#pragma unroll
                    for (int s = 0; s < LTV_NUP; ++s) w += Rs[r * LTV_NUP + s] * uu[s];
                    const double v = ul[r * nt];
                    Ao[o] = (T)v;
                    Fo[o] = v;
                    Wo[o] = w;
                    o += n;
                }
#pragma unroll 1
                for (int r = 0; r < nx; ++r) {
                    double w = 0.0;
#pragma unroll
                    for (int i = 0; i < NXP; ++i) w += Qk[r * NXP + i] * x[i];
                    const double v = xl[r * nt];
                    Ao[o] = (T)v;
                    Fo[o] = v;
                    Wo[o] = w;
                    o += n;
                }
            }
        } else {
            for (int r = 0; r < nu; ++r) Go[(row0 + r) * nxa + (col - n)] = ul[r * nt];
            for (int r = 0; r < nx; ++r) Go[(row0 + nu + r) * nxa + (col - n)] = xl[r * nt];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- Hessian
// Tile row I (16 rows of H) has the slots [G | f] (NA = ceil((nx + 1) / 16) tiles: two when nx = 16), (I, I), (I, I + 1), ...,
// (I, RT - 1); an item is two consecutive slots of one row, so the dense [G | f] tiles come first and pair with each other or
// with the diagonal tile: all of them start at the first non-zero row of W's column block.  A wave keeps 2 accumulators and
// loads 3 operands per k-step of 4 rows (2 and 1 when the row's last item has a single slot).
template <bool TWO>
__device__ __forceinline__ void ltv_hess_loop(const double* __restrict__ W, int n, int cw, const double* __restrict__ P0, int ld0,
                                              int c0, const double* __restrict__ P1, int ld1, int c1, int klo, int m, int kq,
                                              cd4& acc0, cd4& acc1) {
    for (int k0 = klo; k0 < m; k0 += 16) {
        double w[4], f0[4], f1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                                    // branch-free: rows clamped, a row >= m switched off in w
            const int k = k0 + 4 * u + kq, kc = min(k, m - 1);
            const double wv = W[(size_t)kc * n + cw];
            w[u] = (k < m) ? wv : 0.0;
            f0[u] = P0[(size_t)kc * ld0 + c0];
            if constexpr (TWO) f1[u] = P1[(size_t)kc * ld1 + c1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], f0[u], acc0, 0, 0, 0);
            if constexpr (TWO) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u], f1[u], acc1, 0, 0, 0);
        }
    }
}

// LEAD (rqp_ltv_condense_rate): W has been amended by the rate terms (rqp_rate.hip) and its staircase leads F's by one stage:
// column c of W (stage j = c / nu) is non-zero from the u rows of stage j - 1 on.  The H tiles take klo from F's column block
// J >= I and stay as they are; the [G | f] tiles take it from W's column block I and start one stage earlier.
template <typename T, bool LEAD = false>
__global__ void __launch_bounds__(64) k_ltv_hess(LtvArgs a, int RT, int NA, int nitems) {
#if defined(__gfx950__)
    const int b = blockIdx.x / nitems, lane = threadIdx.x, i16 = lane & 15, kq = lane >> 4;
    int it = blockIdx.x % nitems, I = 0;
    while (it >= (NA + RT - I + 1) / 2) { it -= (NA + RT - I + 1) / 2; ++I; }   // (NA + RT - I slots in row I)
    const int n = a.n, m = a.m, nxa = a.nx + 1, s0 = 2 * it, s1 = 2 * it + 1;
    const bool two = s1 < NA + RT - I, aug0 = s0 < NA, aug1 = s1 < NA;
    const int J0 = aug0 ? s0 : I + s0 - NA, J1 = aug1 ? s1 : I + s1 - NA;   // [G | f] tile index, or tile column J >= I of H
    const double* W = a.W + (size_t)b * m * n;
    const double* F = a.F + (size_t)b * m * n;
    const double* Gf = a.Gf + (size_t)b * m * nxa;
    const int cw = min(16 * I + i16, n - 1);
    const double* P0 = aug0 ? Gf : F;
    const double* P1 = aug1 ? Gf : F;
    const int ld0 = aug0 ? nxa : n, c0 = min(16 * J0 + i16, ld0 - 1);
    const int ld1 = aug1 ? nxa : n, c1 = min(16 * J1 + i16, ld1 - 1);
    // first row that can be non-zero in either operand: column 16 J of F (and of W) belongs to stage floor(16 J / nu)
    int klo = ((16 * (aug0 ? I : J0)) / a.nu) * a.blk & ~3;
    if constexpr (LEAD) klo = aug0 ? (max((16 * I) / a.nu - 1, 0) * a.blk & ~3) : klo;
    cd4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    if (two) ltv_hess_loop<true>(W, n, cw, P0, ld0, c0, P1, ld1, c1, klo, m, kq, acc0, acc1);
    else ltv_hess_loop<false>(W, n, cw, P0, ld0, c0, P1, ld1, c1, klo, m, kq, acc0, acc1);
    // D layout: register r of lane (kq, i16) is row kq + 4 r, column i16 of the tile
    T* H = (T*)a.H + (size_t)b * n * n;
    auto store = [&](cd4 acc, int J) __attribute__((always_inline)) {
        if (J == I) {                                                    // diagonal tile: 0.5 (D + D'), the transpose by lane shuffles
            double tr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int src = (i16 & 3) * 16 + kq + 4 * r;             // lane holding row i16 (register i16 >> 2), column kq + 4 r
                double v = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double s = __shfl(acc[q], src, 64);
                    v = ((i16 >> 2) == q) ? s : v;
                }
                tr[r] = v;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = 0.5 * (acc[r] + tr[r]);
        }
        const int c = 16 * J + i16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * I + kq + 4 * r;
            if (row < n && c < n) {
                H[(size_t)row * n + c] = (T)acc[r];
                if (J != I) H[(size_t)c * n + row] = (T)acc[r];         // the lower triangle is the mirror image: H == H' bitwise
            }
        }
    };
    double* gm = a.gmap + (size_t)b * n * nxa;
    auto store_aug = [&](cd4 acc, int Ja) __attribute__((always_inline)) {
        const int c = 16 * Ja + i16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * I + kq + 4 * r;
            if (row < n && c < nxa) gm[(size_t)row * nxa + c] = acc[r];
        }
    };
    if (aug0) store_aug(acc0, J0);
    else store(acc0, J0);
    if (two) {
        if (aug1) store_aug(acc1, J1);
        else store(acc1, J1);
    }
#endif
}

// ---------------------------------------------------------------------------------------------------------------- vectors
// LDS (doubles): x0 [nx], yref [m], t = H_sp yref [m]
// ARGS = LtvRateArgs (rqp_ltv_vectors_rate): the workspace holds W_rate and gmap of the rate problem; g[0:nu] -= S_0 uprev
// before the one rounding (F[u_0] = [I 0] exactly).  The plain calls keep ARGS = LtvArgs: their kernel arguments, and their code.
struct LtvRateArgs : LtvArgs {
    const double* S;                         // [B][N][nu][nu]
    const void* uprev;                       // [B][nu] (T)
};

template <typename T, bool STAGED, typename ARGS = LtvArgs>
__global__ void __launch_bounds__(256) k_ltv_vectors(ARGS a) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, m = a.m, blk = a.blk, nxa = nx + 1;
    double* xs = lds;
    double* yr = xs + nx;
    double* ts = yr + m;
    const bool refs = a.xref || a.uref;
    for (int i = tid; i < nx; i += nt) xs[i] = (double)((const T*)a.x0)[(size_t)b * nx + i];
    if (refs)
        for (int row = tid; row < m; row += nt) {
            const int k = row / blk, r = row % blk;
            double v = 0.0;
            if (r < nu) { if (a.uref) v = (double)((const T*)a.uref)[((size_t)b * N + k) * nu + r]; }
            else if (a.xref) v = (double)((const T*)a.xref)[((size_t)b * N + k) * nx + (r - nu)];
            yr[row] = v;
        }
    __syncthreads();
    const double* Gf = a.Gf + (size_t)b * m * nxa;
    const T* la = (const T*)a.ladd + (a.lu_batched ? (size_t)b * m : 0);
    const T* ua = (const T*)a.uadd + (a.lu_batched ? (size_t)b * m : 0);
    for (int row = tid; row < m; row += nt) {
        const double* gr = Gf + (size_t)row * nxa;
        double s = gr[nx];
        for (int i = 0; i < nx; ++i) s += gr[i] * xs[i];
        ((T*)a.l)[(size_t)b * m + row] = (T)((double)la[row] - s);
        ((T*)a.u)[(size_t)b * m + row] = (T)((double)ua[row] - s);
        if (refs) {                                                      // t = H_sp yref by its diagonal blocks
            const int k = row / blk, r = row % blk;
            double t = 0.0;
            if (r < nu) {
                const double* Rk = STAGED ? a.R + ((size_t)b * N + k) * nu * nu : a.R;
                for (int q = 0; q < nu; ++q) t += Rk[r * nu + q] * yr[k * blk + q];
            } else {
                const double* Qk = STAGED ? a.Q + ((size_t)b * N + k) * nx * nx : ((k == N - 1) ? a.Qf : a.Q);
                for (int q = 0; q < nx; ++q) t += Qk[(r - nu) * nx + q] * yr[k * blk + nu + q];
            }
            ts[row] = t;
        }
    }
    __syncthreads();
    const double* gm = a.gmap + (size_t)b * n * nxa;
    const double* F = a.F + (size_t)b * m * n;
    for (int col = tid; col < n; col += nt) {
        const double* gr = gm + (size_t)col * nxa;
        double s = gr[nx];
        for (int i = 0; i < nx; ++i) s += gr[i] * xs[i];
        if (refs) {
            double acc = 0.0;
            for (int row = (col / nu) * blk; row < m; ++row) acc += F[(size_t)row * n + col] * ts[row];   // rows above: zeros of F
            s -= acc;
        }
        if constexpr (std::is_same<ARGS, LtvRateArgs>::value) {
            if (col < nu) {
                const double* S0 = a.S + (size_t)b * N * nu * nu + (size_t)col * nu;
                double acc = 0.0;
                for (int q = 0; q < nu; ++q) acc += S0[q] * (double)((const T*)a.uprev)[(size_t)b * nu + q];
                s -= acc;
            }
        }
        ((T*)a.g)[(size_t)b * n + col] = (T)s;
    }
}

int nxp_of(int nx) { return (nx + 3) / 4 * 4; }
size_t transition_lds(int N, int nxp, int threads, bool staged) {
    const size_t weights = staged ? 0 : LTV_NUP * LTV_NUP + 2 * nxp * nxp;
    return sizeof(double) * ((size_t)N * nxp * nxp + LTV_NUP * nxp + weights + (size_t)(nxp + LTV_NUP) * threads);
}

LtvArgs base_args(const rqp_ltv_dims* d, void* ws) {
    LtvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = d->batch; a.nx = d->nx; a.nu = d->nu; a.N = d->horizon;
    a.blk = d->nx + d->nu; a.n = d->horizon * d->nu; a.m = d->horizon * a.blk;
    a.has_c = (d->flags & RQP_LTV_HAS_C) != 0;
    a.has_K = (d->flags & RQP_LTV_HAS_K) != 0;
    a.lu_batched = (d->flags & RQP_LTV_BOUNDS_BATCHED) != 0;
    double* w = (double*)ws;
    const size_t B = d->batch, mn = (size_t)a.m * a.n;
    a.F = w;
    a.W = a.F + B * mn;
    a.Gf = a.W + B * mn;
    a.gmap = a.Gf + B * a.m * (a.nx + 1);
    return a;
}

template <typename T, int NXP, bool STAGED>
hipError_t launch_transition(const LtvArgs& a, hipStream_t s) {
    const int threads = (a.n + a.nx + 1 + 63) / 64 * 64;
    const size_t lds = transition_lds(a.N, NXP, threads, STAGED);
    if (lds > 48 * 1024) {
        hipError_t e = rqp_raise_lds_limit((const void*)k_ltv_transition<T, NXP, STAGED>, lds);
        if (e != hipSuccess) return e;
    }
    k_ltv_transition<T, NXP, STAGED><<<a.B, threads, lds, s>>>(a);
    return hipGetLastError();
}

template <typename T, bool STAGED>
hipError_t launch_transition_t(const LtvArgs& a, hipStream_t s) {
    switch (nxp_of(a.nx)) {
        case 4: return launch_transition<T, 4, STAGED>(a, s);
        case 8: return launch_transition<T, 8, STAGED>(a, s);
        case 12: return launch_transition<T, 12, STAGED>(a, s);
        default: return launch_transition<T, 16, STAGED>(a, s);
    }
}

}  // namespace

const char* rqp_ltv_check_dims(const rqp_ltv_dims* d) {
    if (!d) return "dims is NULL";
    if (d->batch < 1 || d->nx < 1 || d->nu < 1 || d->horizon < 1) return "batch, nx, nu and horizon must be >= 1";
    if (d->dtype != RQP_F32 && d->dtype != RQP_F64) return "dtype must be RQP_F32 or RQP_F64";
    if (d->flags & ~(RQP_LTV_HAS_K | RQP_LTV_HAS_C | RQP_LTV_HAS_XREF | RQP_LTV_HAS_UREF | RQP_LTV_BOUNDS_BATCHED | RQP_LTV_STAGE_WEIGHTS))
        return "unknown flag";
    return nullptr;
}

const char* rqp_ltv_check_size(const rqp_ltv_dims* d) {
    if (d->nx > 16 || d->nu > LTV_NUP || d->horizon > 32 || d->horizon * d->nu > 160 || d->horizon * (d->nx + d->nu) > 640)
        return "LTV condensing holds nx <= 16, nu <= 8, horizon <= 32, n = horizon nu <= 160, m = horizon (nx + nu) <= 640";
    return nullptr;
}

size_t rqp_ltv_ws_bytes(const rqp_ltv_dims* d) {
    const size_t B = d->batch, n = (size_t)d->horizon * d->nu, m = (size_t)d->horizon * (d->nx + d->nu), nxa = d->nx + 1;
    return sizeof(double) * B * (2 * m * n + m * nxa + n * nxa);
}

void rqp_ltv_ws_maps(const rqp_ltv_dims* d, const void* ws, const double** F, const double** Gf) {
    const LtvArgs a = base_args(d, const_cast<void*>(ws));
    *F = a.F;
    *Gf = a.Gf;
}

double* rqp_ltv_ws_w(const rqp_ltv_dims* d, void* ws) { return base_args(d, ws).W; }

// S != NULL: the rate call (k_rate_w between the two kernels, k_ltv_hess<T, true>); else the plain chain, as it was.
static hipError_t launch_condense(const rqp_ltv_dims* d, const void* Ad, const void* Bd, const void* c, const double* Q,
                                  const double* R, const double* Qf, const double* K, const double* S, void* H, void* A, void* ws,
                                  hipStream_t s) {
    LtvArgs a = base_args(d, ws);
    a.Ad = Ad; a.Bd = Bd; a.c = c; a.Q = Q; a.R = R; a.Qf = Qf; a.K = K; a.H = H; a.A = A;
    hipError_t e;
    if (d->flags & RQP_LTV_STAGE_WEIGHTS)
        e = (d->dtype == RQP_F32) ? launch_transition_t<float, true>(a, s) : launch_transition_t<double, true>(a, s);
    else
        e = (d->dtype == RQP_F32) ? launch_transition_t<float, false>(a, s) : launch_transition_t<double, false>(a, s);
    if (e != hipSuccess) return e;
    const int RT = (a.n + 15) / 16;
    const int NA = (a.nx + 1 + 15) / 16;                                 // tiles of [G | f]: 2 when nx = 16
    int nitems = 0;
    for (int I = 0; I < RT; ++I) nitems += (NA + RT - I + 1) / 2;
    const unsigned grid = (unsigned)((size_t)a.B * nitems);
    if (S) {
        e = rqp_ltv_launch_rate_w(d, S, ws, s);
        if (e != hipSuccess) return e;
        if (d->dtype == RQP_F32) k_ltv_hess<float, true><<<grid, 64, 0, s>>>(a, RT, NA, nitems);
        else k_ltv_hess<double, true><<<grid, 64, 0, s>>>(a, RT, NA, nitems);
        return hipGetLastError();
    }
    if (d->dtype == RQP_F32) k_ltv_hess<float><<<grid, 64, 0, s>>>(a, RT, NA, nitems);
    else k_ltv_hess<double><<<grid, 64, 0, s>>>(a, RT, NA, nitems);
    return hipGetLastError();
}

hipError_t rqp_ltv_launch_condense(const rqp_ltv_dims* d, const void* Ad, const void* Bd, const void* c, const double* Q,
                                   const double* R, const double* Qf, const double* K, void* H, void* A, void* ws, hipStream_t s) {
    return launch_condense(d, Ad, Bd, c, Q, R, Qf, K, nullptr, H, A, ws, s);
}

hipError_t rqp_ltv_launch_condense_rate(const rqp_ltv_dims* d, const void* Ad, const void* Bd, const void* c, const double* Q,
                                        const double* R, const double* Qf, const double* K, const double* S, void* H, void* A,
                                        void* ws, hipStream_t s) {
    return launch_condense(d, Ad, Bd, c, Q, R, Qf, K, S, H, A, ws, s);
}

hipError_t rqp_ltv_launch_vectors_rate(const rqp_ltv_dims* d, const void* x0, const void* xref, const void* uref, const void* l_add,
                                       const void* u_add, const double* Q, const double* R, const double* Qf, const double* S,
                                       const void* uprev, const void* ws, void* g, void* l, void* u, hipStream_t s) {
    LtvRateArgs a;
    static_cast<LtvArgs&>(a) = base_args(d, const_cast<void*>(ws));
    a.x0 = x0; a.xref = xref; a.uref = uref; a.ladd = l_add; a.uadd = u_add; a.Q = Q; a.R = R; a.Qf = Qf; a.g = g; a.l = l; a.u = u;
    a.S = S; a.uprev = uprev;
    const size_t lds = sizeof(double) * (size_t)(a.nx + 2 * a.m);
    if (d->flags & RQP_LTV_STAGE_WEIGHTS) {
        if (d->dtype == RQP_F32) k_ltv_vectors<float, true, LtvRateArgs><<<a.B, 256, lds, s>>>(a);
        else k_ltv_vectors<double, true, LtvRateArgs><<<a.B, 256, lds, s>>>(a);
    } else {
        if (d->dtype == RQP_F32) k_ltv_vectors<float, false, LtvRateArgs><<<a.B, 256, lds, s>>>(a);
        else k_ltv_vectors<double, false, LtvRateArgs><<<a.B, 256, lds, s>>>(a);
    }
    return hipGetLastError();
}

hipError_t rqp_ltv_launch_vectors(const rqp_ltv_dims* d, const void* x0, const void* xref, const void* uref, const void* l_add,
                                  const void* u_add, const double* Q, const double* R, const double* Qf, const void* ws, void* g,
                                  void* l, void* u, hipStream_t s) {
    LtvArgs a = base_args(d, const_cast<void*>(ws));
    a.x0 = x0; a.xref = xref; a.uref = uref; a.ladd = l_add; a.uadd = u_add; a.Q = Q; a.R = R; a.Qf = Qf; a.g = g; a.l = l; a.u = u;
    const size_t lds = sizeof(double) * (size_t)(a.nx + 2 * a.m);
    if (d->flags & RQP_LTV_STAGE_WEIGHTS) {
        if (d->dtype == RQP_F32) k_ltv_vectors<float, true><<<a.B, 256, lds, s>>>(a);
        else k_ltv_vectors<double, true><<<a.B, 256, lds, s>>>(a);
    } else {
        if (d->dtype == RQP_F32) k_ltv_vectors<float, false><<<a.B, 256, lds, s>>>(a);
        else k_ltv_vectors<double, false><<<a.B, 256, lds, s>>>(a);
    }
    return hipGetLastError();
}
