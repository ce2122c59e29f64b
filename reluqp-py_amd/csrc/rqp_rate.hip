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
//
// Reverse mode (rqp_ltv_condense_adjoint_rate, DESIGN.md section 5 "LTV condensing, input rates, adjoint").  With Hs = sym(dH),
// q_k = (F dg)[u_k] - (F dg)[u_{k-1}], r_k = ds_k - [k = 0] uprev, t = dl_r + du_r, M_k = dF_k Hs, the rate terms add
//     Fb[u_k rows] += Z_k - Z_{k+1},  Z_k = dA_r,k + S_k (2 M_k + r_k dg')  (Z_N = 0),      sb[u_k rows] += w_k - w_{k+1},
//     w_k = S_k q_k - t_k  (w_N = 0),      dS_k = sym(M_k dF_k' + q_k r_k'),      duprev = -w_0
// to the adjoint of rqp_condense_adj.hip, whose seed, blocks, sweep and weight kernels run unchanged around two kernels here:
//   k_rate_adj_vectors  in the place of k_ltva_vectors, one workgroup per instance.  F dg and s as there (a wave per row); W is
//                  not read (in a rate workspace it is W_rate): eb = H_sp (F dg) by the diagonal blocks, like S e.  Then q, r
//                  (kept in the adjoint workspace for k_rate_adj), w, duprev, and sb with the rate addend, dx0 = G'sb.
//   k_rate_adj     after k_ltva_blocks, one workgroup per (instance, stage k), one thread per column c < (k + 1) nu.  dF_k and
//                  dF_{k+1} sit in LDS, transposed and zero-padded to 2, 4 or 8 rows (a thread reads the entries of a column j
//                  as broadcast 16-byte reads), S_k, S_{k+1} zero-padded to 8 x 8.  The thread forms column c of M_k and M_{k+1}
//                  (Hs symmetrised on load; T = F Hs of k_ltva_seed stops at F's staircase and cannot be differenced), adds
//                  Z_k - Z_{k+1} to its nu entries of Fb[u_k rows] (written by k_ltva_blocks of the same (instance, stage), touched
//                  by no other thread) and leaves its column of M_k in LDS; nu^2 threads then sum M_k dF_k' over the columns in
//                  order and symmetrise: dS_k is bitwise symmetric.  dA_r is read left of the staircase only.
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

// ---------------------------------------------------------------------------------------------------------------- adjoint
struct RateAdjArgs {
    int B, nx, nu, N, n, m, blk, staged, need_fb, has_T;
    long long sA, sv;                                 // elements between instances of dA_r / of dl_r, du_r
    const void *x0, *xref, *uref, *uprev;             // forward inputs (T)
    const double *Q, *R, *Qf, *S;                     // staged: Q [B][N][nx][nx], R [B][N][nu][nu], Qf not read; S [B][N][nu][nu]
    const double *F, *Gf;                             // forward workspace: [B][m][n], [B][m][nx + 1]
    const void *dH, *dg, *dl, *du, *dAr, *dlr, *dur;  // cotangents (T), NULL = zero
    void *dx0, *dxref, *duref, *duprev;               // outputs (T), NULL = not wanted
    double* dS;                                       // [B][N][nu][nu], NULL = not wanted
    double *Fb, *vec, *qr;                            // adjoint workspace: [B][m][n], [B][4][m] (rows as k_ltva_vectors), [B][2][n]
};

enum { RV_E = 0, RV_SE = 1, RV_FG = 2, RV_SB = 3 };  // the rows of vec, as rqp_condense_adj.hip reads them

// LDS (doubles): x0 [nx], dg [n], e, F dg, sb [m] each, s of the u rows, q, r, w [n] each, partial sums of dx0 [16][16]
template <typename T>
__global__ void __launch_bounds__(256) k_rate_adj_vectors(RateAdjArgs a) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, m = a.m, blk = a.blk, nxa = nx + 1;
    double* xs = lds;
    double* gbs = xs + nx;
    double* es = gbs + n;
    double* fgs = es + m;
    double* sbs = fgs + m;
    double* su = sbs + m;
    double* qs = su + n;
    double* rs = qs + n;
    double* wv = rs + n;
    double* part = wv + n;
    for (int i = tid; i < nx; i += 256) xs[i] = (double)((const T*)a.x0)[(size_t)b * nx + i];
    for (int c = tid; c < n; c += 256) gbs[c] = a.dg ? (double)((const T*)a.dg)[(size_t)b * n + c] : 0.0;
    __syncthreads();
    const double* F = a.F + (size_t)b * m * n;
    const double* Gf = a.Gf + (size_t)b * m * nxa;
    double* vec = a.vec + (size_t)b * 4 * m;
    for (int row = wave; row < m; row += 4) {
        const int k = row / blk, r = row - k * blk, cl = (k + 1) * nu;   // columns >= cl of this row are zero in F
        double fg = 0.0;
        if (a.dg)
            for (int c = lane; c < cl; c += 64) fg += F[(size_t)row * n + c] * gbs[c];
        double s = (lane < nx) ? Gf[(size_t)row * nxa + lane] * xs[lane] : (lane == nx ? Gf[(size_t)row * nxa + nx] : 0.0);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            fg += __shfl_xor(fg, off, 64);
            s += __shfl_xor(s, off, 64);
        }
        if (lane == 0) {
            double yr = 0.0;
            if (r < nu) { if (a.uref) yr = (double)((const T*)a.uref)[((size_t)b * N + k) * nu + r]; }
            else if (a.xref) yr = (double)((const T*)a.xref)[((size_t)b * N + k) * nx + (r - nu)];
            const double e = s - yr;
            es[row] = e;
            fgs[row] = fg;
            if (r < nu) su[k * nu + r] = s;
            vec[RV_E * m + row] = e;
            vec[RV_FG * m + row] = fg;
        }
    }
    __syncthreads();
    double* qr = a.qr + (size_t)b * 2 * n;
    for (int e = tid; e < n; e += 256) {                                 // q = D (F dg), r = D s - [uprev; 0; ...]
        const int k = e / nu, r = e - k * nu;
        const double q = fgs[k * blk + r] - (k > 0 ? fgs[(k - 1) * blk + r] : 0.0);
        const double rr = su[e] - (k > 0 ? su[e - nu] : (double)((const T*)a.uprev)[(size_t)b * nu + e]);
        qs[e] = q;
        rs[e] = rr;
        qr[e] = q;
        qr[n + e] = rr;
    }
    __syncthreads();
    for (int e = tid; e < n; e += 256) {                                 // w_k = S_k q_k - t_k;  duprev = t_0 - S_0 q_0
        const int k = e / nu, r = e - k * nu;
        const double* Sk = a.S + ((size_t)b * N + k) * nu * nu;
        double v = 0.0;
        for (int q = 0; q < nu; ++q) v += Sk[r * nu + q] * qs[k * nu + q];
        const double tl = a.dlr ? (double)((const T*)a.dlr)[(size_t)b * a.sv + e] : 0.0;
        const double tu = a.dur ? (double)((const T*)a.dur)[(size_t)b * a.sv + e] : 0.0;
        const double w = v - (tl + tu);
        wv[e] = w;
        if (k == 0 && a.duprev) ((T*)a.duprev)[(size_t)b * nu + e] = (T)(-w);
    }
    __syncthreads();
    for (int row = tid; row < m; row += 256) {                           // S e and eb = H_sp (F dg) by the diagonal blocks
        const int k = row / blk, r = row - k * blk;
        double t = 0.0, eb = 0.0, rate = 0.0;
        if (r < nu) {
            const double* Rk = a.staged ? a.R + ((size_t)b * N + k) * nu * nu : a.R;
            for (int q = 0; q < nu; ++q) {
                t += Rk[r * nu + q] * es[k * blk + q];
                eb += Rk[r * nu + q] * fgs[k * blk + q];
            }
            rate = wv[k * nu + r] - (k < N - 1 ? wv[(k + 1) * nu + r] : 0.0);
        } else {
            const double* Qk = a.staged ? a.Q + ((size_t)b * N + k) * nx * nx : ((k == N - 1) ? a.Qf : a.Q);
            for (int q = 0; q < nx; ++q) {
                t += Qk[(r - nu) * nx + q] * es[k * blk + nu + q];
                eb += Qk[(r - nu) * nx + q] * fgs[k * blk + nu + q];
            }
        }
        const double lb = a.dl ? (double)((const T*)a.dl)[(size_t)b * m + row] : 0.0;
        const double ub = a.du ? (double)((const T*)a.du)[(size_t)b * m + row] : 0.0;
        const double sb = (eb - lb - ub) + rate;
        sbs[row] = sb;
        vec[RV_SE * m + row] = t;
        vec[RV_SB * m + row] = sb;
        if (r < nu) { if (a.duref) ((T*)a.duref)[((size_t)b * N + k) * nu + r] = (T)(-eb); }
        else if (a.dxref) ((T*)a.dxref)[((size_t)b * N + k) * nx + (r - nu)] = (T)(-eb);
    }
    if (a.dx0) {                                                         // dx0 = G'sb: 16 row groups, added in a fixed order
        __syncthreads();
        const int i = tid & 15, rg = tid >> 4;
        double p = 0.0;
        if (i < nx)
            for (int row = rg; row < m; row += 16) p += Gf[(size_t)row * nxa + i] * sbs[row];
        part[rg * 16 + i] = p;
        __syncthreads();
        if (tid < nx) {
            double sum = 0.0;
            for (int q = 0; q < 16; ++q) sum += part[q * 16 + tid];
            ((T*)a.dx0)[(size_t)b * nx + tid] = (T)sum;
        }
    }
}

// NUP = nu padded to 2, 4 or 8: the rows of dF a thread reads per column j and the register arrays (the LDS reads of dF bound
// the M loop, so they are not padded further than needed).
// LDS (doubles): dF_k', dF_{k+1}' [n][NUP] (transposed, zero-padded), M_k [nu][n], S_k, S_{k+1}, P [8][8] each, q_k, r_k, r_{k+1} [8] each
template <typename T, int NUP>
__global__ void __launch_bounds__(192) k_rate_adj(RateAdjArgs a) {
    extern __shared__ double lds[];
    const int b = blockIdx.x / a.N, k = blockIdx.x % a.N, tid = threadIdx.x, nt = blockDim.x;
    const int nu = a.nu, n = a.n, N = a.N, m = a.m, blk = a.blk;
    const bool last = k == N - 1;
    const int c0 = (k + 1) * nu, c1 = last ? 0 : (k + 2) * nu;           // staircases of dF_k and dF_{k+1} (dF_N = 0); c1 <= n
    double* D0 = lds;
    double* D1 = D0 + (size_t)n * NUP;
    double* Mk = D1 + (size_t)n * NUP;
    double* S0 = Mk + (size_t)nu * n;
    double* S1 = S0 + RATE_NUP * RATE_NUP;
    double* P = S1 + RATE_NUP * RATE_NUP;
    double* q0 = P + RATE_NUP * RATE_NUP;
    double* r0 = q0 + RATE_NUP;
    double* r1 = r0 + RATE_NUP;
    const double* Sk = a.S + ((size_t)b * N + k) * nu * nu;
    const double* qr = a.qr + (size_t)b * 2 * n;
    if (tid < RATE_NUP * RATE_NUP) {
        const int r = tid / RATE_NUP, s = tid % RATE_NUP;
        const bool in = r < nu && s < nu;
        S0[tid] = in ? Sk[r * nu + s] : 0.0;
        S1[tid] = (in && !last) ? Sk[nu * nu + r * nu + s] : 0.0;       // S_N = 0
    }
    if (tid < RATE_NUP) {
        q0[tid] = tid < nu ? qr[k * nu + tid] : 0.0;
        r0[tid] = tid < nu ? qr[n + k * nu + tid] : 0.0;
        r1[tid] = (tid < nu && !last) ? qr[n + (k + 1) * nu + tid] : 0.0;
    }
    const double* Fk = a.F + ((size_t)b * m + (size_t)k * blk) * n;      // F[u_k]
    for (int idx = tid; idx < n * NUP; idx += nt) {
        const int j = idx / NUP, s = idx % NUP;
        double fk = 0.0, fm = 0.0, fp = 0.0;
        if (s < nu) {
            const size_t o = (size_t)s * n + j;
            if (j < c0) fk = Fk[o];
            if (j < c0 - nu) fm = Fk[o - (size_t)blk * n];               // F[u_{k-1}] (k >= 1 here: c0 - nu = k nu)
            if (j < c1) fp = Fk[o + (size_t)blk * n];                    // F[u_{k+1}] (not the last stage here)
        }
        D0[idx] = fk - fm;
        D1[idx] = j < c1 ? fp - fk : 0.0;
    }
    __syncthreads();
    const int c = tid;
    const bool on = c < c0;
    double m0[NUP], m1[NUP];
#pragma unroll
    for (int s = 0; s < NUP; ++s) m0[s] = m1[s] = 0.0;
    if (on && a.has_T) {                                                 // column c of M_k = dF_k Hs and M_{k+1} = dF_{k+1} Hs
        const T* dH = (const T*)a.dH + (size_t)b * n * n;
#pragma unroll 4
        for (int j = 0; j < c0; ++j) {                                   // (unrolled: the loads of four rows of dH are in flight together)
            const double h = 0.5 * ((double)dH[(size_t)j * n + c] + (double)dH[(size_t)c * n + j]);
#pragma unroll
            for (int s = 0; s < NUP; ++s) {
                m0[s] += D0[j * NUP + s] * h;
                m1[s] += D1[j * NUP + s] * h;
            }
        }
        for (int j = c0; j < c1; ++j) {
            const double h = 0.5 * ((double)dH[(size_t)j * n + c] + (double)dH[(size_t)c * n + j]);
#pragma unroll
            for (int s = 0; s < NUP; ++s) m1[s] += D1[j * NUP + s] * h;
        }
    }
    if (on) {
#pragma unroll
        for (int s = 0; s < NUP; ++s)
            if (s < nu) Mk[s * n + c] = m0[s];
        if (a.need_fb) {                                                 // Fb[u_k rows][c] += Z_k - Z_{k+1}
            const double gc = a.dg ? (double)((const T*)a.dg)[(size_t)b * n + c] : 0.0;
            double v0[NUP], v1[NUP];
#pragma unroll
            for (int s = 0; s < NUP; ++s) {
                v0[s] = 2.0 * m0[s] + r0[s] * gc;
                v1[s] = 2.0 * m1[s] + r1[s] * gc;
            }
            const T* dAr = a.dAr ? (const T*)a.dAr + (size_t)b * a.sA + (size_t)k * nu * n + c : nullptr;
            double* Fb = a.Fb + ((size_t)b * m + (size_t)k * blk) * n + c;
#pragma unroll 1
            for (int r = 0; r < nu; ++r) {
                double z0 = 0.0, z1 = 0.0;
#pragma unroll
                for (int s = 0; s < NUP; ++s) {
                    z0 += S0[r * RATE_NUP + s] * v0[s];
                    z1 += S1[r * RATE_NUP + s] * v1[s];
                }
                if (dAr) {
                    z0 += (double)dAr[(size_t)r * n];
                    if (!last) z1 += (double)dAr[(size_t)(nu + r) * n];
                }
                Fb[(size_t)r * n] = Fb[(size_t)r * n] + (z0 - z1);
            }
        }
    }
    if (a.dS) {                                                          // dS_k = sym(M_k dF_k' + q_k r_k'), columns in order
        __syncthreads();
        const int r = tid / nu, s = tid - r * nu;
        if (tid < nu * nu) {
            double v = 0.0;
            for (int j = 0; j < c0; ++j) v += Mk[r * n + j] * D0[j * NUP + s];
            P[r * RATE_NUP + s] = v + q0[r] * r0[s];
        }
        __syncthreads();
        if (tid < nu * nu) a.dS[(((size_t)b * N + k) * nu + r) * nu + s] = 0.5 * (P[r * RATE_NUP + s] + P[s * RATE_NUP + r]);
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

// The adjoint workspace of the rate call: that of rqp_ltv_condense_adjoint, then q and r [B][2][n].
size_t rqp_ltv_rate_adj_ws_bytes(const rqp_ltv_dims* d) {
    return rqp_ltv_adj_ws_bytes(d) + sizeof(double) * 2 * (size_t)d->batch * d->horizon * d->nu;
}

namespace {

struct RateAdjCall {
    RateAdjArgs a;
    bool f32;
};

hipError_t rate_adj_vectors(void* ctx, hipStream_t s) {
    const RateAdjCall* c = (const RateAdjCall*)ctx;
    const RateAdjArgs& a = c->a;
    const size_t lds = sizeof(double) * (size_t)(a.nx + 5 * a.n + 3 * a.m + 256);
    if (c->f32) k_rate_adj_vectors<float><<<a.B, 256, lds, s>>>(a);
    else k_rate_adj_vectors<double><<<a.B, 256, lds, s>>>(a);
    return hipGetLastError();
}

hipError_t rate_adj_rows(void* ctx, int need_fb, hipStream_t s) {
    RateAdjCall c = *(const RateAdjCall*)ctx;
    RateAdjArgs& a = c.a;
    a.need_fb = need_fb;
    const int nup = a.nu <= 2 ? 2 : (a.nu <= 4 ? 4 : RATE_NUP);
    const size_t lds = sizeof(double) * ((size_t)a.n * (2 * nup + a.nu) + 3 * RATE_NUP * RATE_NUP + 3 * RATE_NUP);
    const unsigned grid = (unsigned)((size_t)a.B * a.N), block = (unsigned)((a.n + 63) / 64 * 64);
    if (c.f32) {
        if (nup == 2) k_rate_adj<float, 2><<<grid, block, lds, s>>>(a);
        else if (nup == 4) k_rate_adj<float, 4><<<grid, block, lds, s>>>(a);
        else k_rate_adj<float, RATE_NUP><<<grid, block, lds, s>>>(a);
    } else {
        if (nup == 2) k_rate_adj<double, 2><<<grid, block, lds, s>>>(a);
        else if (nup == 4) k_rate_adj<double, 4><<<grid, block, lds, s>>>(a);
        else k_rate_adj<double, RATE_NUP><<<grid, block, lds, s>>>(a);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t rqp_ltv_launch_condense_adjoint_rate(const rqp_ltv_dims* d, const rqp_ltv_adjoint_io* io,
                                                const rqp_ltv_rate_adjoint_io* rio, hipStream_t s) {
    RateAdjCall c;
    memset(&c, 0, sizeof(c));
    RateAdjArgs& a = c.a;
    c.f32 = d->dtype == RQP_F32;
    a.B = d->batch; a.nx = d->nx; a.nu = d->nu; a.N = d->horizon;
    a.blk = d->nx + d->nu; a.n = d->horizon * d->nu; a.m = d->horizon * a.blk;
    a.staged = (d->flags & RQP_LTV_STAGE_WEIGHTS) != 0;
    a.has_T = io->dH != nullptr;
    a.sA = rio->dA_stride; a.sv = rio->dl_stride;
    a.x0 = io->x0; a.uprev = rio->uprev;
    a.xref = (d->flags & RQP_LTV_HAS_XREF) ? io->xref : nullptr;
    a.uref = (d->flags & RQP_LTV_HAS_UREF) ? io->uref : nullptr;
    a.Q = io->Q; a.R = io->R; a.Qf = io->Qf; a.S = rio->S;
    rqp_ltv_ws_maps(d, io->workspace, &a.F, &a.Gf);
    a.dH = io->dH; a.dg = io->dg; a.dl = io->dl; a.du = io->du;
    a.dAr = rio->dA_r; a.dlr = rio->dl_r; a.dur = rio->du_r;
    a.dx0 = io->dx0; a.dxref = io->dxref; a.duref = io->duref; a.duprev = rio->duprev;
    a.dS = rio->dS;
    rqp_ltv_adj_ws_maps(d, io->adjoint_workspace, &a.Fb, &a.vec);
    a.qr = (double*)io->adjoint_workspace + rqp_ltv_adj_ws_bytes(d) / sizeof(double);
    rqp_ltv_adj_hooks hk;
    hk.ctx = &c;
    hk.vectors = rate_adj_vectors;
    hk.rows = rate_adj_rows;
    hk.rows_alone = rio->dS != nullptr;
    return rqp_ltv_launch_condense_adjoint_hooked(d, io, &hk, s);
}
