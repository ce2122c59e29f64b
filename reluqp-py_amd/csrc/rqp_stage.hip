// rqp_stage.hip -- stage constraints of batched LTV MPC problems (rqp_ltv_stage_rows / rqp_ltv_stage_vectors /
// rqp_ltv_stage_adjoint, DESIGN.md section 5 "LTV condensing, stage constraints").
//
// Every stage k = 0 .. N-1 of every instance carries a block E_k [nc][nu + nx] that replaces the identity rows of the box:
//     lo_k <= E_k [u_k ; x_{k+1}] <= hi_k,   m_c = N nc rows.
// With y = F v + s, s = G x0 + f as rqp_ltv_condense left them in the forward workspace (F [B][m][n], [G | f] [B][m][nx + 1],
// float64; the kernels here only read them):
//     A_c = E F  (block row k = E_k F_k, F_k = rows k (nu + nx) .. of F),   l_c = lo - E s,   u_c = hi - E s.
// Column block j of F is zero above stage j, so block row k of A_c is non-zero in the columns < (k + 1) nu only ("left of the
// staircase"): the sums run there and exact zeros are written to the right, whatever E holds.
// Reverse, t = dl_c + du_c:   dA_full_k = E_k' dA_c,k,   dl_full_k = E_k' t_k,   dE_k = dA_c,k F_k' - t_k s_k'
// (dA_full, dl_full are the dA, dl of rqp_ltv_condense_adjoint: l = l_add - s there, l_c = lo - E s here).
// All arithmetic is float64; every output is written once, in T.  No atomics, no allocation, nothing read back.
//
// Three kernels:
//   k_stage_rows     one workgroup per (instance, stage), one thread per column.  E_k sits in LDS as [nu + nx][NCP] (zero-padded
//                    to NCP = 4, 8, 16 or 32 rows, read as broadcasts, two doubles per read); a thread keeps the NCP sums of its
//                    column in registers and walks down the nu + nx rows of F_k: the lanes of a wave read adjacent columns of
//                    one row of F and write adjacent columns of one row of A_c.  F is read once, left of the staircase only.
//   k_stage_vectors  one workgroup per instance: s = G x0 + f into LDS (the sum order of k_ltv_vectors), then one thread per
//                    row of E.  An infinite bound passes through the subtraction as it is.
//   k_stage_adjoint  one workgroup of 256 threads per (instance, stage).  dA_full: a thread holds the nc entries of its column
//                    of dA_c,k in registers and writes one entry of each of the nu + nx rows.  dE: the columns left of the
//                    staircase go through LDS in chunks of 64 ([nu + nx][65] of F_k, [NCP][65] of dA_c,k, odd row length: no
//                    bank conflicts), every thread owns up to three of the nc (nu + nx) outputs and adds its chunk in a fixed
//                    order.  s_k and t_k are rebuilt by the workgroup itself (a few hundred flops).
#include <algorithm>
#include <cstring>

#include "rqp_common.h"

namespace {

constexpr int STG_NC = 32;         // rows per stage
constexpr int STG_BLK = 24;        // nu + nx
constexpr int STG_M = 640;         // m and m_c
constexpr int STG_NX = 16;
constexpr int STG_CH = 64;         // columns per LDS chunk of the dE pass
constexpr int STG_LD = STG_CH + 1;

struct StageArgs {
    int B, nx, nu, N, n, m, blk, nc, mc, e_shared, lu_batched;
    const void *E, *x0, *lo, *hi;            // [B | 1][N][nc][blk], [B][nx], [B | 1][mc] (T)
    const double *F, *Gf;                    // forward workspace: [B][m][n], [B][m][nx + 1]
    void *Ac, *lc, *uc;                      // [B][mc][n], [B][mc] (T)
    const void *dAc, *dlc, *duc;             // cotangents (T), NULL = 0
    void *dA, *dl, *dE;                      // [B][m][n], [B][m], [B][N][nc][blk] (T), NULL = not wanted
};

template <typename T>
__device__ __forceinline__ const T* stage_block(const StageArgs& a, int b, int k) {
    return (const T*)a.E + ((size_t)(a.e_shared ? 0 : b) * a.N + k) * a.nc * a.blk;
}

// E_k -> LDS [blk][NCP], rows >= nc zero
template <typename T, int NCP>
__device__ __forceinline__ void stage_load_E(const T* E, int nc, int blk, double* Es, int tid, int nt) {
    for (int e = tid; e < blk * NCP; e += nt) {
        const int i = e / NCP, r = e % NCP;
        Es[e] = (r < nc) ? (double)E[r * blk + i] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------------------- rows
template <typename T, int NCP>
__global__ void __launch_bounds__(192) k_stage_rows(StageArgs a) {
    __shared__ double Es[STG_BLK * NCP];
    const int b = blockIdx.x / a.N, k = blockIdx.x % a.N, tid = threadIdx.x;
    const int n = a.n, blk = a.blk, nc = a.nc;
    stage_load_E<T, NCP>(stage_block<T>(a, b, k), nc, blk, Es, tid, blockDim.x);
    __syncthreads();
    const int col = tid;
    if (col >= n) return;
    double acc[NCP];
#pragma unroll
    for (int r = 0; r < NCP; ++r) acc[r] = 0.0;
    if (col < (k + 1) * a.nu) {                                          // left of the staircase
        const double* Fk = a.F + ((size_t)b * a.m + (size_t)k * blk) * n + col;
#pragma unroll 2
        for (int i = 0; i < blk; ++i) {
            const double f = Fk[(size_t)i * n];
#pragma unroll
            for (int r = 0; r < NCP; ++r) acc[r] += Es[i * NCP + r] * f;
        }
    }
    T* out = (T*)a.Ac + ((size_t)b * a.mc + (size_t)k * nc) * n + col;
#pragma unroll
    for (int r = 0; r < NCP; ++r)
        if (r < nc) out[(size_t)r * n] = (T)acc[r];
}

// ---------------------------------------------------------------------------------------------------------------- vectors
template <typename T>
__global__ void __launch_bounds__(256) k_stage_vectors(StageArgs a) {
    __shared__ double xs[STG_NX];
    __shared__ double ss[STG_M];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int nx = a.nx, m = a.m, blk = a.blk, nc = a.nc, mc = a.mc, nxa = nx + 1;
    if (tid < nx) xs[tid] = (double)((const T*)a.x0)[(size_t)b * nx + tid];
    __syncthreads();
    const double* Gf = a.Gf + (size_t)b * m * nxa;
    for (int row = tid; row < m; row += nt) {
        const double* gr = Gf + (size_t)row * nxa;
        double s = gr[nx];
        for (int i = 0; i < nx; ++i) s += gr[i] * xs[i];
        ss[row] = s;
    }
    __syncthreads();
    const T* E = stage_block<T>(a, b, 0);                                // [mc][blk]: row r belongs to stage r / nc
    const T* lo = (const T*)a.lo + (a.lu_batched ? (size_t)b * mc : 0);
    const T* hi = (const T*)a.hi + (a.lu_batched ? (size_t)b * mc : 0);
    for (int r = tid; r < mc; r += nt) {
        const T* Er = E + (size_t)r * blk;
        const double* sk = ss + (r / nc) * blk;
        double e = 0.0;
        for (int i = 0; i < blk; ++i) e += (double)Er[i] * sk[i];
        ((T*)a.lc)[(size_t)b * mc + r] = (T)((double)lo[r] - e);
        ((T*)a.uc)[(size_t)b * mc + r] = (T)((double)hi[r] - e);
    }
}

// ---------------------------------------------------------------------------------------------------------------- adjoint
template <typename T, int NCP>
__global__ void __launch_bounds__(256) k_stage_adjoint(StageArgs a) {
    __shared__ double Es[STG_BLK * NCP];
    __shared__ double Fs[STG_BLK * STG_LD];
    __shared__ double Ds[NCP * STG_LD];
    __shared__ double ts[NCP], sk[STG_BLK], xs[STG_NX];
    const int b = blockIdx.x / a.N, k = blockIdx.x % a.N, tid = threadIdx.x, nt = 256;
    const int nx = a.nx, n = a.n, m = a.m, blk = a.blk, nc = a.nc, mc = a.mc, nxa = nx + 1;
    const int lim = (k + 1) * a.nu;                                      // columns left of the staircase
    stage_load_E<T, NCP>(stage_block<T>(a, b, k), nc, blk, Es, tid, nt);
    if (tid < NCP) {                                                     // t_k = dl_c + du_c (an absent one is zero)
        double t = 0.0;
        if (tid < nc) {
            const size_t o = (size_t)b * mc + (size_t)k * nc + tid;
            t = (a.dlc ? (double)((const T*)a.dlc)[o] : 0.0) + (a.duc ? (double)((const T*)a.duc)[o] : 0.0);
        }
        ts[tid] = t;
    }
    if (tid < nx) xs[tid] = (double)((const T*)a.x0)[(size_t)b * nx + tid];
    __syncthreads();
    if (tid < blk) {                                                     // s_k = (G x0 + f)_k and dl_full_k = E_k' t_k
        const size_t row = (size_t)b * m + (size_t)k * blk + tid;
        const double* gr = a.Gf + row * nxa;
        double s = gr[nx];
        for (int i = 0; i < nx; ++i) s += gr[i] * xs[i];
        sk[tid] = s;
        if (a.dl) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < NCP; ++r) v += Es[tid * NCP + r] * ts[r];
            ((T*)a.dl)[row] = (T)v;
        }
    }
    const T* dAc = a.dAc ? (const T*)a.dAc + ((size_t)b * mc + (size_t)k * nc) * n : nullptr;
    if (a.dA && tid < n) {                                               // dA_full_k = E_k' dA_c,k, one column per thread
        const int col = tid;
        const bool left = col < lim;
        double d[NCP];
#pragma unroll
        for (int r = 0; r < NCP; ++r) d[r] = (left && dAc && r < nc) ? (double)dAc[(size_t)r * n + col] : 0.0;
        T* out = (T*)a.dA + ((size_t)b * m + (size_t)k * blk) * n + col;
#pragma unroll 2
        for (int i = 0; i < blk; ++i) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < NCP; ++r) v += Es[i * NCP + r] * d[r];
            out[(size_t)i * n] = left ? (T)v : (T)0.0;
        }
    }
    if (!a.dE) return;                                                   // (uniform: the barriers below are reached by all or none)
    const int no = nc * blk;                                             // <= 3 * 256 outputs
    const double* Fk = a.F + ((size_t)b * m + (size_t)k * blk) * n;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < lim; c0 += STG_CH) {
        const int w = min(STG_CH, lim - c0);
        __syncthreads();                                                 // the previous chunk has been consumed (first pass: sk, ts)
        for (int e = tid; e < blk * STG_CH; e += nt) {
            const int i = e / STG_CH, c = e % STG_CH;
            Fs[i * STG_LD + c] = (c < w) ? Fk[(size_t)i * n + c0 + c] : 0.0;
        }
        for (int e = tid; e < nc * STG_CH; e += nt) {
            const int r = e / STG_CH, c = e % STG_CH;
            Ds[r * STG_LD + c] = (c < w && dAc) ? (double)dAc[(size_t)r * n + c0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int o = tid + nt * q;
            if (o < no) {
                const double* dr = Ds + (o / blk) * STG_LD;
                const double* fr = Fs + (o % blk) * STG_LD;
                double s = acc[q];
                for (int c = 0; c < w; ++c) s += dr[c] * fr[c];
                acc[q] = s;
            }
        }
    }
    __syncthreads();                                                     // (lim >= 1: the loop ran; sk, ts are visible)
    T* dE = (T*)a.dE + ((size_t)b * a.N + k) * no;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int o = tid + nt * q;
        if (o < no) dE[o] = (T)(acc[q] - ts[o / blk] * sk[o % blk]);
    }
}

StageArgs stage_args(const rqp_ltv_dims* d, int nc, const void* ws) {
    StageArgs a;
    memset(&a, 0, sizeof(a));
    a.B = d->batch; a.nx = d->nx; a.nu = d->nu; a.N = d->horizon;
    a.blk = d->nx + d->nu; a.n = d->horizon * d->nu; a.m = d->horizon * a.blk;
    a.nc = nc; a.mc = d->horizon * nc;
    a.e_shared = (d->flags & RQP_LTV_STAGE_SHARED_E) != 0;
    a.lu_batched = (d->flags & RQP_LTV_BOUNDS_BATCHED) != 0;
    rqp_ltv_ws_maps(d, ws, &a.F, &a.Gf);
    return a;
}

// KERNEL<T, NCP> for the runtime (dtype, nc)
#define STAGE_DISPATCH(KERNEL, grid, block)                                                          \
    do {                                                                                             \
        const bool f32 = d->dtype == RQP_F32;                                                        \
        if (a.nc <= 4) { if (f32) KERNEL<float, 4><<<grid, block, 0, s>>>(a); else KERNEL<double, 4><<<grid, block, 0, s>>>(a); }         \
        else if (a.nc <= 8) { if (f32) KERNEL<float, 8><<<grid, block, 0, s>>>(a); else KERNEL<double, 8><<<grid, block, 0, s>>>(a); }    \
        else if (a.nc <= 16) { if (f32) KERNEL<float, 16><<<grid, block, 0, s>>>(a); else KERNEL<double, 16><<<grid, block, 0, s>>>(a); } \
        else { if (f32) KERNEL<float, 32><<<grid, block, 0, s>>>(a); else KERNEL<double, 32><<<grid, block, 0, s>>>(a); }                 \
    } while (0)

}  // namespace

// The launch bounds and the fixed LDS arrays above hold what rqp_ltv_check_size admits today (n <= 160, nx <= 16, nx + nu <= 24,
// m <= 640); they are checked here again, so that raising the condensing's limits alone turns into this error, not an overrun.
static_assert(STG_NC * STG_BLK <= 3 * 256, "k_stage_adjoint: three outputs of dE per thread");
const char* rqp_ltv_stage_check_size(const rqp_ltv_dims* d, int nc) {
    if (nc < 1 || nc > STG_NC || (long long)d->horizon * nc > STG_M)
        return "stage constraints hold 1 <= nc <= 32 rows per stage and m_c = horizon nc <= 640";
    if (d->nx > STG_NX || d->nx + d->nu > STG_BLK || (long long)d->horizon * d->nu > 192 ||
        (long long)d->horizon * (d->nx + d->nu) > STG_M)
        return "stage constraints hold nx <= 16, nx + nu <= 24, n = horizon nu <= 192 and m = horizon (nx + nu) <= 640";
    return nullptr;
}

hipError_t rqp_ltv_launch_stage_rows(const rqp_ltv_dims* d, int nc, const void* E, const void* ws, void* Ac, hipStream_t s) {
    StageArgs a = stage_args(d, nc, ws);
    a.E = E; a.Ac = Ac;
    const unsigned grid = (unsigned)((size_t)a.B * a.N), block = (unsigned)((a.n + 63) / 64 * 64);
    STAGE_DISPATCH(k_stage_rows, grid, block);
    return hipGetLastError();
}

hipError_t rqp_ltv_launch_stage_vectors(const rqp_ltv_dims* d, int nc, const void* E, const void* x0, const void* lo, const void* hi,
                                        const void* ws, void* lc, void* uc, hipStream_t s) {
    StageArgs a = stage_args(d, nc, ws);
    a.E = E; a.x0 = x0; a.lo = lo; a.hi = hi; a.lc = lc; a.uc = uc;
    if (d->dtype == RQP_F32) k_stage_vectors<float><<<a.B, 256, 0, s>>>(a);
    else k_stage_vectors<double><<<a.B, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t rqp_ltv_launch_stage_adjoint(const rqp_ltv_dims* d, int nc, const rqp_ltv_stage_adjoint_io* io, hipStream_t s) {
    StageArgs a = stage_args(d, nc, io->workspace);
    a.E = io->E; a.x0 = io->x0; a.dAc = io->dA_c; a.dlc = io->dl_c; a.duc = io->du_c;
    a.dA = io->dA_full; a.dl = io->dl_full; a.dE = io->dE;
    if (!a.dA && !a.dl && !a.dE) return hipSuccess;
    const unsigned grid = (unsigned)((size_t)a.B * a.N);
    STAGE_DISPATCH(k_stage_adjoint, grid, 256);
    return hipGetLastError();
}
