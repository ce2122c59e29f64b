// rqp_rate.hip -- input-rate (delta u) cost and bounds of batched LTV MPC problems (rqp_ltv_condense_rate / rqp_ltv_rate_rows /
// rqp_ltv_rate_bounds, DESIGN.md section 5 "LTV condensing, input rates").
//
// With y = F v + s, s = G x0 + f as rqp_ltv_condense left them in the forward workspace, F[u_k] the nu rows k (nu + nx) .. of F:
//     dF_k = F[u_k] - F[u_{k-1}]  (dF_0 = F[u_0], dF_N = 0),      ds_k = s[u_k] - s[u_{k-1}]  (ds_0 = s[u_0]).
// Cost  1/2 sum_k (u_k - u_{k-1})' S_k (u_k - u_{k-1}),  u_{-1} = uprev:  the Hessian gains F' H_d F with H_d block tridiagonal on the
// u rows, so W = H_sp F is amended in place,
//     W[u_k rows] += S_k dF_k - S_{k+1} dF_{k+1}        (S_N = 0; the x rows of W stay),
// and k_ltv_hess (rqp_condense.hip) forms H = sym(W' F) and W' [G | f] from it as before.  Column c of the amended W (stage
// j = c / nu) is non-zero from the u rows of stage j - 1 on: W's staircase leads F's by one stage.
// Rows  dlo_k <= u_k - u_{k-1} <= dhi_k:   A_r,k = dF_k,   l_r,k = dlo_k - ds_k + [k = 0] uprev,   u_r,k likewise with dhi_k.
// dF_k is zero in the columns >= (k + 1) nu ("right of the staircase") and is written as exact zeros there.
// All arithmetic is float64; every output is written once, in T.  No atomics, no allocation, nothing read back.
//
// Three kernels:
//   k_rate_w       one workgroup per (instance, stage k), one thread per column c < min((k + 2) nu, n).  S_k and S_{k+1} sit in
//                  LDS, zero-padded to 8 x 8 (broadcast reads); a thread loads its entries of F[u_{k-1}], F[u_k], F[u_{k+1}] (the
//                  lanes of a wave read adjacent columns of one row), forms the two differences in registers and adds the two
//                  products to its nu entries of W[u_k rows] (read and written by this thread alone).  F is only read.
//   k_rate_rows    one workgroup per (instance, stage), one thread per column: nu rows of A_r, zeros right of the staircase.
//   k_rate_bounds  one workgroup per instance: s of the u rows into LDS (the sum order of k_ltv_vectors), then one thread per
//                  row.  An infinite bound passes through the subtraction as it is.
#include <cstring>

#include "rqp_common.h"

namespace {

constexpr int RATE_NUP = 8;        // nu padded
constexpr int RATE_NX = 16;
constexpr int RATE_N = 160;        // n = horizon nu

struct RateArgs {
    int B, nx, nu, N, n, m, blk, lu_batched;
    long long stride;                        // elements between instances of A_r / of l_r, u_r
    const double* S;                         // [B][N][nu][nu]
    const double *F, *Gf;                    // forward workspace: [B][m][n], [B][m][nx + 1]
    double* W;                               // forward workspace: [B][m][n], amended in place
    const void *x0, *uprev, *dlo, *dhi;      // [B][nx], [B][nu], [B | 1][n] (T)
    void *Ar, *lr, *ur;                      // [B] x stride (T)
};

// ---------------------------------------------------------------------------------------------------------------------- W
__global__ void __launch_bounds__(192) k_rate_w(RateArgs a) {
    __shared__ double S0[RATE_NUP * RATE_NUP], S1[RATE_NUP * RATE_NUP];
    const int b = blockIdx.x / a.N, k = blockIdx.x % a.N, tid = threadIdx.x;
    const int nu = a.nu, n = a.n, N = a.N;
    const bool last = k == N - 1;
    const double* Sk = a.S + ((size_t)b * N + k) * nu * nu;
    if (tid < RATE_NUP * RATE_NUP) {
        const int r = tid / RATE_NUP, s = tid % RATE_NUP;
        const bool in = r < nu && s < nu;
        S0[tid] = in ? Sk[r * nu + s] : 0.0;
        S1[tid] = (in && !last) ? Sk[nu * nu + r * nu + s] : 0.0;       // S_N = 0
    }
    __syncthreads();
    const int col = tid;
    if (col >= min((k + 2) * nu, n)) return;                             // right of W's (shifted) staircase: nothing to add
    const size_t urow = (size_t)b * a.m + (size_t)k * a.blk;            // first u row of stage k
    const double* Fk = a.F + urow * n + col;
    const double* Fm = k > 0 ? Fk - (size_t)a.blk * n : Fk;              // stage k - 1 (k = 0: not used)
    const double* Fp = last ? Fk : Fk + (size_t)a.blk * n;               // stage k + 1 (dF_N = 0)
    double d0[RATE_NUP], d1[RATE_NUP];
#pragma unroll
    for (int s = 0; s < RATE_NUP; ++s) {
        const size_t o = (size_t)min(s, nu - 1) * n;                     // index clamped into the block, a padding term switched off
        const double fk = Fk[o];
        const double fm = k > 0 ? Fm[o] : 0.0;
        const double fp = Fp[o];
        d0[s] = s < nu ? fk - fm : 0.0;
        d1[s] = s < nu ? fp - fk : 0.0;
    }
    double* Wk = a.W + urow * n + col;
#pragma unroll 1
    for (int r = 0; r < nu; ++r) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int s = 0; s < RATE_NUP; ++s) {
            t0 += S0[r * RATE_NUP + s] * d0[s];
            t1 += S1[r * RATE_NUP + s] * d1[s];
        }
        Wk[(size_t)r * n] = Wk[(size_t)r * n] + t0 - t1;
    }
}

// ------------------------------------------------------------------------------------------------------------------- rows
template <typename T>
__global__ void __launch_bounds__(192) k_rate_rows(RateArgs a) {
    const int b = blockIdx.x / a.N, k = blockIdx.x % a.N, col = threadIdx.x;
    const int nu = a.nu, n = a.n;
    if (col >= n) return;
    const bool left = col < (k + 1) * nu;                                // left of the staircase
    const double* Fk = a.F + ((size_t)b * a.m + (size_t)k * a.blk) * n + col;
    const double* Fm = k > 0 ? Fk - (size_t)a.blk * n : Fk;
    T* out = (T*)a.Ar + (size_t)b * a.stride + (size_t)k * nu * n + col;
    for (int r = 0; r < nu; ++r) {
        double v = 0.0;
        if (left) v = Fk[(size_t)r * n] - (k > 0 ? Fm[(size_t)r * n] : 0.0);
        out[(size_t)r * n] = (T)v;
    }
}

// ----------------------------------------------------------------------------------------------------------------- bounds
template <typename T>
__global__ void __launch_bounds__(256) k_rate_bounds(RateArgs a) {
    __shared__ double xs[RATE_NX];
    __shared__ double su[RATE_N];                                        // s of the u rows: su[k nu + r] = s[k blk + r]
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int nx = a.nx, nu = a.nu, n = a.n, nxa = nx + 1;
    if (tid < nx) xs[tid] = (double)((const T*)a.x0)[(size_t)b * nx + tid];
    __syncthreads();
    const double* Gf = a.Gf + (size_t)b * a.m * nxa;
    for (int e = tid; e < n; e += nt) {
        const double* gr = Gf + (size_t)((e / nu) * a.blk + e % nu) * nxa;
        double s = gr[nx];
        for (int i = 0; i < nx; ++i) s += gr[i] * xs[i];
        su[e] = s;
    }
    __syncthreads();
    const T* lo = (const T*)a.dlo + (a.lu_batched ? (size_t)b * n : 0);
    const T* hi = (const T*)a.dhi + (a.lu_batched ? (size_t)b * n : 0);
    T* lr = (T*)a.lr + (size_t)b * a.stride;
    T* ur = (T*)a.ur + (size_t)b * a.stride;
    for (int e = tid; e < n; e += nt) {
        const double ds = su[e] - (e >= nu ? su[e - nu] : 0.0);
        const double up = e < nu ? (double)((const T*)a.uprev)[(size_t)b * nu + e] : 0.0;
        lr[e] = (T)((double)lo[e] - ds + up);
        ur[e] = (T)((double)hi[e] - ds + up);
    }
}

RateArgs rate_args(const rqp_ltv_dims* d, const void* ws) {
    RateArgs a;
    memset(&a, 0, sizeof(a));
    a.B = d->batch; a.nx = d->nx; a.nu = d->nu; a.N = d->horizon;
    a.blk = d->nx + d->nu; a.n = d->horizon * d->nu; a.m = d->horizon * a.blk;
    a.lu_batched = (d->flags & RQP_LTV_BOUNDS_BATCHED) != 0;
    rqp_ltv_ws_maps(d, ws, &a.F, &a.Gf);
    return a;
}

}  // namespace

// The launch bounds and the fixed LDS arrays above hold what rqp_ltv_check_size admits today (nu <= 8, nx <= 16, n <= 160); they
// are checked here again, so that raising the condensing's limits alone turns into this error, not an overrun.
const char* rqp_ltv_rate_check_size(const rqp_ltv_dims* d) {
    if (d->nu > RATE_NUP || d->nx > RATE_NX || (long long)d->horizon * d->nu > RATE_N)
        return "input rates hold nu <= 8, nx <= 16 and n = horizon nu <= 160";
    return nullptr;
}

hipError_t rqp_ltv_launch_rate_w(const rqp_ltv_dims* d, const double* S, void* ws, hipStream_t s) {
    RateArgs a = rate_args(d, ws);
    a.S = S;
    a.W = rqp_ltv_ws_w(d, ws);
    const unsigned grid = (unsigned)((size_t)a.B * a.N), block = (unsigned)((a.n + 63) / 64 * 64);
    k_rate_w<<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t rqp_ltv_launch_rate_rows(const rqp_ltv_dims* d, const void* ws, void* Ar, long long inst_stride, hipStream_t s) {
    RateArgs a = rate_args(d, ws);
    a.Ar = Ar; a.stride = inst_stride;
    const unsigned grid = (unsigned)((size_t)a.B * a.N), block = (unsigned)((a.n + 63) / 64 * 64);
    if (d->dtype == RQP_F32) k_rate_rows<float><<<grid, block, 0, s>>>(a);
    else k_rate_rows<double><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t rqp_ltv_launch_rate_bounds(const rqp_ltv_dims* d, const void* x0, const void* uprev, const void* dlo, const void* dhi,
                                      const void* ws, void* lr, void* ur, long long inst_stride, hipStream_t s) {
    RateArgs a = rate_args(d, ws);
    a.x0 = x0; a.uprev = uprev; a.dlo = dlo; a.dhi = dhi; a.lr = lr; a.ur = ur; a.stride = inst_stride;
    if (d->dtype == RQP_F32) k_rate_bounds<float><<<a.B, 256, 0, s>>>(a);
    else k_rate_bounds<double><<<a.B, 256, 0, s>>>(a);
    return hipGetLastError();
}
