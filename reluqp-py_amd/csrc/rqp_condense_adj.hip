// rqp_condense_adj.hip -- reverse mode of the LTV condensing (rqp_ltv_condense_adjoint, DESIGN.md section 5 "LTV condensing,
// adjoint"): the cotangents (dH, dA, dg, dl, du) of the condensed QP mapped back to the stage matrices, the vectors and the weights.
//
// Notation of rqp_condense.hip: y = F v + G x0 + f, S = H_sp, W = S F, H = sym(F'SF), A = F, s = G x0 + f, e = s - yref,
// g = F'S e, l / u = l_add / u_add - s.  With Hs = (dH + dH') / 2 and T = F Hs:
//     Fb = dA + 2 S T + (S e) dg',   eb = W dg,   sb = eb - dl - du,   dx0 = G'sb,   dyref = -eb,   [Gb | fb] = sb [x0' | 1],
//     Sb_kk = F_k T_k' + (F dg)_k e_k'   (diagonal blocks: dR = sum of the u blocks, dQ / dQf of the x blocks, symmetrised),
// and with Yb = [Fb | Gb | fb], X_k = the x_k rows of [F | G | f] (X_0 = [0 | I | 0]) the sweep over the stages
//     Lam = Yb[x_N rows];  k = N-1 .. 0:  Aclb = Lam X_k',  dAd_k = Aclb,  dBd_k = Lam[:, k nu : (k+1) nu] - Aclb K',
//                                         dc_k = Lam[:, f];   Lam <- Acl_k' Lam - K' Yb[u_k rows] + Yb[x_k rows]  (k >= 1).
// F, W, [G | f] are read from the forward workspace.  All arithmetic is float64; every output is rounded once.  No atomics: the
// batch sums of the weight gradients are added in a fixed order, so two calls give the same bits.
//
// Kernels (a fixed chain; a kernel whose results nobody asked for is not launched):
//   k_ltva_vectors   one workgroup per instance.  A wave per row of W / F: eb = W dg, F dg (lanes over the columns below the
//                    staircase, butterfly sum), s from [G | f]; then S e by the diagonal blocks and dx0 = G'sb in 16 fixed
//                    row groups.  Writes dx0, dxref, duref and the rows e, S e, F dg, sb of the adjoint workspace.
//   k_ltva_seed      T = F Hs on v_mfma_f64_16x16x4_f64, one wave per pair of 16 x 16 tiles, operand lanes as in k_ltv_hess:
//                    lane (kq, i16) holds F[16 I + i16][j0 + kq] (A operand) and Hs[j0 + kq][16 J + i16] (B operand, symmetrised
//                    on load).  Row block k of F ends at column (k + 1) nu: tiles to the right of the staircase are skipped
//                    and the inner loop stops at the staircase of the tile's last row.
//   k_ltva_blocks    one workgroup per (instance, stage): T_k and F_k (blk rows, the columns below the staircase) in LDS;
//                    Fb_k = dA_k + 2 S_k T_k + (S e)_k dg' written over T_k, and the nu^2 + nx^2 entries of Sb_kk that the
//                    weights need, per (instance, stage).
//   k_ltva_sweep     one workgroup per instance, ONE THREAD PER COLUMN of Lam (n + nx + 1 columns), the mirror of
//                    k_ltv_transition: the thread's column of Lam in registers, Acl_k' and K in LDS (broadcast reads), rolled
//                    row loops.  Aclb = Lam X_k' is summed over the columns in a fixed order from the LDS images of Lam and
//                    X_k (the columns of stages >= k are zero in X_k and are skipped).
//   k_ltva_wsum1/2   the weight gradients: per-(instance, stage) entries -> 256 partial sums over fixed slices of the batch
//                    -> one sum in a fixed order, symmetrised.
//   k_ltva_wstage    RQP_LTV_STAGE_WEIGHTS instead of the two sums: the entries of every (instance, stage), symmetrised, are the
//                    outputs dR [B][N][nu][nu], dQ [B][N][nx][nx] themselves.
// With RQP_LTV_STAGE_WEIGHTS, Q and R are [B][N][..][..] and the kernels that read weights (k_ltva_vectors, k_ltva_blocks) index
// the block of their instance and stage: a template parameter (STAGED), the shared-weight instantiations are what they were.
#include <algorithm>
#include <cstring>

#include "rqp_common.h"

namespace {

typedef double cd4 __attribute__((ext_vector_type(4)));
constexpr int LTV_NUP = 8;         // nu padded (register arrays), as rqp_condense.hip
constexpr int WSUM_SLICES = 256;   // first stage of the batch sums

struct LtvAdjArgs {
    int B, nx, nu, N, n, m, blk, has_K, need_fb, need_w, has_T;
    const void *Ad, *Bd, *x0, *xref, *uref;           // forward inputs (T)
    const double *Q, *R, *Qf, *K;                     // STAGED: Q [B][N][nx][nx], R [B][N][nu][nu], Qf not read
    const double *F, *W, *Gf;                         // forward workspace: [B][m][n], [B][m][n], [B][m][nx + 1]
    const void *dH, *dA, *dg, *dl, *du;               // cotangents (T), NULL = zero
    void *dAd, *dBd, *dc, *dx0, *dxref, *duref;       // outputs (T), NULL = not wanted
    double *dQ, *dR, *dQf;                            // batch sums, NULL = not wanted; STAGED: dQ, dR shaped like Q, R, no sum
    double *TF, *vec, *wpart, *wsl;                   // adjoint workspace: [B][m][n], [B][4][m], [B][N][wsz], [slices][2][wsz]
};

enum { V_E = 0, V_SE = 1, V_FG = 2, V_SB = 3 };

// ---------------------------------------------------------------------------------------------------------------- vectors
// LDS (doubles): x0 [nx], dg [n], e [m], sb [m], partial sums of dx0 [16][16]
template <typename T, bool STAGED>
__global__ void __launch_bounds__(256) k_ltva_vectors(LtvAdjArgs a) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, m = a.m, blk = a.blk, nxa = nx + 1;
    double* xs = lds;
    double* gbs = xs + nx;
    double* es = gbs + n;
    double* sbs = es + m;
    double* part = sbs + m;
    for (int i = tid; i < nx; i += 256) xs[i] = (double)((const T*)a.x0)[(size_t)b * nx + i];
    for (int c = tid; c < n; c += 256) gbs[c] = a.dg ? (double)((const T*)a.dg)[(size_t)b * n + c] : 0.0;
    __syncthreads();
    const double* F = a.F + (size_t)b * m * n;
    const double* W = a.W + (size_t)b * m * n;
    const double* Gf = a.Gf + (size_t)b * m * nxa;
    double* vec = a.vec + (size_t)b * 4 * m;
    for (int row = wave; row < m; row += 4) {
        const int k = row / blk, r = row - k * blk, cl = (k + 1) * nu;   // columns >= cl of this row are zero in F and W
        double fg = 0.0, eb = 0.0;
        if (a.dg)
            for (int c = lane; c < cl; c += 64) {
                fg += F[(size_t)row * n + c] * gbs[c];
                eb += W[(size_t)row * n + c] * gbs[c];
            }
        double s = (lane < nx) ? Gf[(size_t)row * nxa + lane] * xs[lane] : (lane == nx ? Gf[(size_t)row * nxa + nx] : 0.0);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            fg += __shfl_xor(fg, off, 64);
            eb += __shfl_xor(eb, off, 64);
            s += __shfl_xor(s, off, 64);
        }
        if (lane == 0) {
            double yr = 0.0;
            if (r < nu) { if (a.uref) yr = (double)((const T*)a.uref)[((size_t)b * N + k) * nu + r]; }
            else if (a.xref) yr = (double)((const T*)a.xref)[((size_t)b * N + k) * nx + (r - nu)];
            const double lb = a.dl ? (double)((const T*)a.dl)[(size_t)b * m + row] : 0.0;
            const double ub = a.du ? (double)((const T*)a.du)[(size_t)b * m + row] : 0.0;
            const double e = s - yr, sb = eb - lb - ub;
            es[row] = e;
            sbs[row] = sb;
            vec[V_E * m + row] = e;
            vec[V_FG * m + row] = fg;
            vec[V_SB * m + row] = sb;
            if (r < nu) { if (a.duref) ((T*)a.duref)[((size_t)b * N + k) * nu + r] = (T)(-eb); }
            else if (a.dxref) ((T*)a.dxref)[((size_t)b * N + k) * nx + (r - nu)] = (T)(-eb);
        }
    }
    __syncthreads();
    for (int row = tid; row < m; row += 256) {                           // S e by the diagonal blocks
        const int k = row / blk, r = row - k * blk;
        double t = 0.0;
        if (r < nu) {
            const double* Rk = STAGED ? a.R + ((size_t)b * N + k) * nu * nu : a.R;
            for (int q = 0; q < nu; ++q) t += Rk[r * nu + q] * es[k * blk + q];
        } else {
            const double* Qk = STAGED ? a.Q + ((size_t)b * N + k) * nx * nx : ((k == N - 1) ? a.Qf : a.Q);
            for (int q = 0; q < nx; ++q) t += Qk[(r - nu) * nx + q] * es[k * blk + nu + q];
        }
        vec[V_SE * m + row] = t;
    }
    if (a.dx0) {                                                         // dx0 = G'sb: 16 row groups, added in a fixed order
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

// ------------------------------------------------------------------------------------------------------------------- seed
template <typename T>
__global__ void __launch_bounds__(64) k_ltva_seed(LtvAdjArgs a, int RTm, int JP) {
#if defined(__gfx950__)
    const int b = blockIdx.x / (RTm * JP), rem = blockIdx.x % (RTm * JP), I = rem / JP, jp = rem % JP;
    const int lane = threadIdx.x, i16 = lane & 15, kq = lane >> 4;
    const int n = a.n, m = a.m;
    const int kend = (min(16 * I + 15, m - 1) / a.blk + 1) * a.nu;       // staircase of the tile's last row (<= n)
    const int J0 = 2 * jp, J1 = 2 * jp + 1;
    if (16 * J0 >= kend) return;                                         // (uniform) both tiles right of the staircase
    const bool two = 16 * J1 < kend;
    const double* F = a.F + (size_t)b * m * n;
    const T* dH = (const T*)a.dH + (size_t)b * n * n;
    const int row = min(16 * I + i16, m - 1);
    const int c0 = min(16 * J0 + i16, n - 1), c1 = min(16 * J1 + i16, n - 1);
    cd4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < kend; j0 += 16) {
        double f[4], h0[4], h1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                                    // branch-free: indices clamped, a column >= kend switched off in f
            const int j = j0 + 4 * u + kq, jc = min(j, n - 1);
            const double fv = F[(size_t)row * n + jc];
            f[u] = (j < kend) ? fv : 0.0;
            h0[u] = 0.5 * ((double)dH[(size_t)jc * n + c0] + (double)dH[(size_t)c0 * n + jc]);
            h1[u] = 0.5 * ((double)dH[(size_t)jc * n + c1] + (double)dH[(size_t)c1 * n + jc]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(f[u], h0[u], acc0, 0, 0, 0);
            if (two) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(f[u], h1[u], acc1, 0, 0, 0);
        }
    }
    // D layout: register r of lane (kq, i16) is row kq + 4 r, column i16 of the tile
    double* To = a.TF + (size_t)b * m * n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ro = 16 * I + kq + 4 * r;
        if (ro < m) {
            if (16 * J0 + i16 < n) To[(size_t)ro * n + 16 * J0 + i16] = acc0[r];
            if (two && 16 * J1 + i16 < n) To[(size_t)ro * n + 16 * J1 + i16] = acc1[r];
        }
    }
#endif
}

// ----------------------------------------------------------------------------------------------------------------- blocks
// LDS (doubles): T_k [blk][ld], F_k [blk][ld] (ld odd), R [nu][nu], Q_k [nx][nx], (S e)_k, e_k, (F dg)_k [blk] each, dg [n]
template <typename T, bool STAGED>
__global__ void __launch_bounds__(256) k_ltva_blocks(LtvAdjArgs a, int ld) {
    extern __shared__ double lds[];
    const int b = blockIdx.x / a.N, k = blockIdx.x % a.N, tid = threadIdx.x;
    const int nx = a.nx, nu = a.nu, n = a.n, m = a.m, blk = a.blk;
    const int cl = (k + 1) * nu, row0 = k * blk, wsz = nu * nu + nx * nx;
    double* Tk = lds;
    double* Fk = Tk + (size_t)blk * ld;
    double* Rs = Fk + (size_t)blk * ld;
    double* Qs = Rs + nu * nu;
    double* Sek = Qs + nx * nx;
    double* ek = Sek + blk;
    double* Fgk = ek + blk;
    double* gbs = Fgk + blk;
    const double* Qk = STAGED ? a.Q + (size_t)blockIdx.x * nx * nx : ((k == a.N - 1) ? a.Qf : a.Q);   // (blockIdx.x = b N + k)
    const double* Rk = STAGED ? a.R + (size_t)blockIdx.x * nu * nu : a.R;
    const double* vec = a.vec + (size_t)b * 4 * m;
    for (int e = tid; e < nu * nu; e += 256) Rs[e] = Rk[e];
    for (int e = tid; e < nx * nx; e += 256) Qs[e] = Qk[e];
    for (int r = tid; r < blk; r += 256) {
        Sek[r] = vec[V_SE * m + row0 + r];
        ek[r] = vec[V_E * m + row0 + r];
        Fgk[r] = vec[V_FG * m + row0 + r];
    }
    for (int c = tid; c < cl; c += 256) gbs[c] = a.dg ? (double)((const T*)a.dg)[(size_t)b * n + c] : 0.0;
    double* TF = a.TF + ((size_t)b * m + row0) * n;
    const double* F = a.F + ((size_t)b * m + row0) * n;
    for (int idx = tid; idx < blk * cl; idx += 256) {
        const int r = idx / cl, c = idx - r * cl;
        Tk[r * ld + c] = a.has_T ? TF[(size_t)r * n + c] : 0.0;
        Fk[r * ld + c] = F[(size_t)r * n + c];
    }
    __syncthreads();
    if (a.need_fb) {
        const T* dA = a.dA ? (const T*)a.dA + ((size_t)b * m + row0) * n : nullptr;
        for (int idx = tid; idx < blk * cl; idx += 256) {
            const int r = idx / cl, c = idx - r * cl;
            double v = 0.0;
            if (r < nu) {
                for (int q = 0; q < nu; ++q) v += Rs[r * nu + q] * Tk[q * ld + c];
            } else {
                for (int q = 0; q < nx; ++q) v += Qs[(r - nu) * nx + q] * Tk[(nu + q) * ld + c];
            }
            const double ab = dA ? (double)dA[(size_t)r * n + c] : 0.0;
            TF[(size_t)r * n + c] = ab + 2.0 * v + Sek[r] * gbs[c];     // Fb over T (every T_k entry is in LDS by now)
        }
    }
    if (a.need_w) {
        double* wp = a.wpart + ((size_t)b * a.N + k) * wsz;
        for (int e = tid; e < wsz; e += 256) {
            int r, s;
            if (e < nu * nu) { r = e / nu; s = e - r * nu; }
            else { const int q = e - nu * nu; r = nu + q / nx; s = nu + q % nx; }
            double v = 0.0;
            for (int c = 0; c < cl; ++c) v += Fk[r * ld + c] * Tk[s * ld + c];
            wp[e] = v + Fgk[r] * ek[s];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ sweep
// LDS (doubles): Lam [NXP][LD], X_k [NXP][LD] (LD = threads + 1, odd), Acl_k' [NXP][NXP], Aclb [NXP][NXP], K [NUP][NXP]
// (zero-padded), sb [m], x0 [nx].
template <typename T, int NXP>
__global__ void __launch_bounds__(192) k_ltva_sweep(LtvAdjArgs a) {
    extern __shared__ double lds[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, LD = nt + 1;
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, m = a.m, blk = a.blk, nxa = nx + 1, ncol = n + nxa;
    double* Ls = lds;
    double* Xs = Ls + (size_t)NXP * LD;
    double* AclT = Xs + (size_t)NXP * LD;
    double* Ab = AclT + NXP * NXP;
    double* Ks = Ab + NXP * NXP;
    double* sbs = Ks + LTV_NUP * NXP;
    double* xs0 = sbs + m;
    const T* Ad = (const T*)a.Ad + (size_t)b * N * nx * nx;
    const T* Bd = (const T*)a.Bd + (size_t)b * N * nx * nu;
    const double* F = a.F + (size_t)b * m * n;
    const double* Gf = a.Gf + (size_t)b * m * nxa;
    const double* Fb = a.TF + (size_t)b * m * n;
    for (int e = tid; e < LTV_NUP * NXP; e += nt) {
        const int r = e / NXP, i = e % NXP;
        Ks[e] = (a.has_K && r < nu && i < nx) ? a.K[r * nx + i] : 0.0;
    }
    for (int r = tid; r < m; r += nt) sbs[r] = a.vec[((size_t)b * 4 + V_SB) * m + r];
    for (int i = tid; i < nx; i += nt) xs0[i] = (double)((const T*)a.x0)[(size_t)b * nx + i];
    __syncthreads();

    const int col = tid;
    const bool on = col < ncol, isF = col < n;
    // entry (row, col) of Yb = [Fb | sb x0' | sb]; Fb is only defined below the staircase (zero to the right of it)
    auto yb = [&](int row) __attribute__((always_inline)) -> double {
        if (isF) return (col < (row / blk + 1) * nu) ? Fb[(size_t)row * n + col] : 0.0;
        return (col < n + nx) ? sbs[row] * xs0[col - n] : sbs[row];
    };
    double lam[NXP];
#pragma unroll
    for (int i = 0; i < NXP; ++i) lam[i] = 0.0;
    if (on) {
#pragma unroll
        for (int i = 0; i < NXP; ++i)
            if (i < nx) lam[i] = yb((N - 1) * blk + nu + i);
    }
    for (int k = N - 1; k >= 0; --k) {
        __syncthreads();                                                 // the previous stage has finished with the LDS images
        for (int e = tid; e < NXP * NXP; e += nt) {                      // Acl_k' = (A_k - B_k K)'
            const int r = e / NXP, i = e % NXP;
            double v = 0.0;
            if (r < nx && i < nx) {
                v = (double)Ad[((size_t)k * nx + r) * nx + i];
                if (a.has_K)
                    for (int s = 0; s < nu; ++s) v -= (double)Bd[((size_t)k * nx + r) * nu + s] * Ks[s * NXP + i];
            }
            AclT[i * NXP + r] = v;
        }
#pragma unroll
        for (int i = 0; i < NXP; ++i) Ls[i * LD + tid] = lam[i];
#pragma unroll 1
        for (int i = 0; i < nx; ++i) {                                   // this thread's column of X_k
            double x = 0.0;
            if (on) {
                if (k == 0) x = (col == n + i) ? 1.0 : 0.0;
                else {
                    const size_t row = (size_t)(k - 1) * blk + nu + i;
                    x = isF ? F[row * n + col] : Gf[row * nxa + (col - n)];
                }
            }
            Xs[i * LD + tid] = x;
        }
        __syncthreads();
        for (int e = tid; e < nx * nx; e += nt) {                        // Aclb = Lam X_k': F columns of stages < k, then [G | f]
            const int r = e / nx, i = e - r * nx;
            const double* lr = Ls + (size_t)r * LD;
            const double* xr = Xs + (size_t)i * LD;
            double s = 0.0;
            for (int c = 0; c < k * nu; ++c) s += lr[c] * xr[c];
            for (int c = n; c < ncol; ++c) s += lr[c] * xr[c];
            Ab[r * NXP + i] = s;
        }
        __syncthreads();
        if (a.dAd)
            for (int e = tid; e < nx * nx; e += nt)
                ((T*)a.dAd)[((size_t)b * N + k) * nx * nx + e] = (T)Ab[(e / nx) * NXP + e % nx];
        if (a.dBd)
            for (int e = tid; e < nx * nu; e += nt) {
                const int r = e / nu, s = e - r * nu;
                double v = Ls[r * LD + k * nu + s];
                for (int i = 0; i < nx; ++i) v -= Ab[r * NXP + i] * Ks[s * NXP + i];
                ((T*)a.dBd)[((size_t)b * N + k) * nx * nu + e] = (T)v;
            }
        if (a.dc)
            for (int r = tid; r < nx; r += nt) ((T*)a.dc)[((size_t)b * N + k) * nx + r] = (T)Ls[r * LD + n + nx];
        if (k >= 1 && on) {                                              // Lam <- Acl_k' Lam - K' Yb[u_k rows] + Yb[x_k rows]
            double yu[LTV_NUP];
#pragma unroll
            for (int s = 0; s < LTV_NUP; ++s) yu[s] = (s < nu) ? yb(k * blk + s) : 0.0;
#pragma unroll 1
            for (int i = 0; i < nx; ++i) {
                double v = yb((k - 1) * blk + nu + i);
#pragma unroll
                for (int r = 0; r < NXP; ++r) v += AclT[i * NXP + r] * lam[r];
#pragma unroll
                for (int s = 0; s < LTV_NUP; ++s) v -= Ks[s * NXP + i] * yu[s];
                Xs[i * LD + tid] = v;                                    // (the thread's own column: X_k is no longer read)
            }
#pragma unroll
            for (int i = 0; i < NXP; ++i)
                if (i < nx) lam[i] = Xs[i * LD + tid];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ weight sums
// wpart [B][N][wsz] (wsz = nu^2 + nx^2: the u block, then the x block of Sb_kk).  Stage 1: slice j adds the instances j, j + S,
// j + 2 S, ... stage by stage, the x block of the last stage apart (Qf): wsl [S][2][wsz].  Stage 2: the slices in order.
__global__ void __launch_bounds__(256) k_ltva_wsum1(LtvAdjArgs a, int slices) {
    const int j = blockIdx.x, wsz = a.nu * a.nu + a.nx * a.nx;
    for (int e = threadIdx.x; e < wsz; e += 256) {
        double s0 = 0.0, s1 = 0.0;
        for (int b = j; b < a.B; b += slices) {
            const double* wp = a.wpart + (size_t)b * a.N * wsz + e;
            for (int k = 0; k < a.N - 1; ++k) s0 += wp[(size_t)k * wsz];
            const double last = wp[(size_t)(a.N - 1) * wsz];
            if (e < a.nu * a.nu) s0 += last;
            else s1 += last;
        }
        a.wsl[((size_t)j * 2 + 0) * wsz + e] = s0;
        a.wsl[((size_t)j * 2 + 1) * wsz + e] = s1;
    }
}

// LDS (doubles): [2][wsz]
__global__ void __launch_bounds__(256) k_ltva_wsum2(LtvAdjArgs a, int slices) {
    extern __shared__ double lds[];
    const int nx = a.nx, nu = a.nu, wsz = nu * nu + nx * nx;
    for (int e = threadIdx.x; e < 2 * wsz; e += 256) {
        const int half = e / wsz, q = e - half * wsz;
        double p[4] = {0.0, 0.0, 0.0, 0.0};                              // four interleaved chains, joined in a fixed order
        for (int j = 0; j < slices; ++j) p[j & 3] += a.wsl[((size_t)j * 2 + half) * wsz + q];
        lds[e] = (p[0] + p[1]) + (p[2] + p[3]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nu * nu; e += 256) {
        const int r = e / nu, s = e - r * nu;
        if (a.dR) a.dR[e] = 0.5 * (lds[r * nu + s] + lds[s * nu + r]);
    }
    for (int e = threadIdx.x; e < nx * nx; e += 256) {
        const int r = e / nx, s = e - r * nx, o = nu * nu;
        if (a.dQ) a.dQ[e] = 0.5 * (lds[o + r * nx + s] + lds[o + s * nx + r]);
        if (a.dQf) a.dQf[e] = 0.5 * (lds[wsz + o + r * nx + s] + lds[wsz + o + s * nx + r]);
    }
}

// Stage weights: one workgroup per (instance, stage), its wpart entries symmetrised into its blocks of dR and dQ.
__global__ void __launch_bounds__(256) k_ltva_wstage(LtvAdjArgs a) {
    const int nx = a.nx, nu = a.nu, wsz = nu * nu + nx * nx;
    const double* wp = a.wpart + (size_t)blockIdx.x * wsz;               // (blockIdx.x = b N + k)
    if (a.dR)
        for (int e = threadIdx.x; e < nu * nu; e += 256) {
            const int r = e / nu, s = e - r * nu;
            a.dR[(size_t)blockIdx.x * nu * nu + e] = 0.5 * (wp[r * nu + s] + wp[s * nu + r]);
        }
    if (a.dQ)
        for (int e = threadIdx.x; e < nx * nx; e += 256) {
            const int r = e / nx, s = e - r * nx, o = nu * nu;
            a.dQ[(size_t)blockIdx.x * nx * nx + e] = 0.5 * (wp[o + r * nx + s] + wp[o + s * nx + r]);
        }
}

int nxp_of(int nx) { return (nx + 3) / 4 * 4; }

template <typename T, int NXP>
hipError_t launch_sweep(const LtvAdjArgs& a, hipStream_t s) {
    const int threads = (a.n + a.nx + 1 + 63) / 64 * 64;
    const size_t lds = sizeof(double) * (2 * (size_t)NXP * (threads + 1) + 2 * NXP * NXP + LTV_NUP * NXP + a.m + a.nx);
    if (lds > 48 * 1024) {
        hipError_t e = rqp_raise_lds_limit((const void*)k_ltva_sweep<T, NXP>, lds);
        if (e != hipSuccess) return e;
    }
    k_ltva_sweep<T, NXP><<<a.B, threads, lds, s>>>(a);
    return hipGetLastError();
}

// `hk` (rqp_ltv_condense_adjoint_rate, rqp_rate.hip): its vectors kernel runs in the place of k_ltva_vectors and its rows kernel
// after k_ltva_blocks, before the sweep reads Fb.  NULL: the chain of rqp_ltv_condense_adjoint, launch by launch what it was.
template <typename T, bool STAGED>
hipError_t launch_adjoint_t(LtvAdjArgs& a, const rqp_ltv_adj_hooks* hk, hipStream_t s) {
    const int wsz = a.nu * a.nu + a.nx * a.nx;
    const bool sweep = a.dAd || a.dBd || a.dc, weights = a.dQ || a.dR || a.dQf;
    a.need_fb = sweep;
    a.need_w = weights;
    a.has_T = a.dH != nullptr;
    hipError_t e;
    if (hk) e = hk->vectors(hk->ctx, s);
    else {
        k_ltva_vectors<T, STAGED><<<a.B, 256, sizeof(double) * (size_t)(a.nx + a.n + 2 * a.m + 256), s>>>(a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    if (!sweep && !weights) return (hk && hk->rows_alone) ? hk->rows(hk->ctx, 0, s) : e;
    if (a.has_T) {
        const int RTm = (a.m + 15) / 16, JP = ((a.n + 15) / 16 + 1) / 2;
        k_ltva_seed<T><<<(unsigned)((size_t)a.B * RTm * JP), 64, 0, s>>>(a, RTm, JP);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int ld = a.n | 1;
    const size_t blds = sizeof(double) * (2 * (size_t)a.blk * ld + wsz + 3 * a.blk + a.n);
    if (blds > 48 * 1024) {
        e = rqp_raise_lds_limit((const void*)k_ltva_blocks<T, STAGED>, blds);
        if (e != hipSuccess) return e;
    }
    k_ltva_blocks<T, STAGED><<<(unsigned)((size_t)a.B * a.N), 256, blds, s>>>(a, ld);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (hk && (sweep || hk->rows_alone) && (e = hk->rows(hk->ctx, sweep ? 1 : 0, s)) != hipSuccess) return e;
    if (sweep) {
        switch (nxp_of(a.nx)) {
            case 4: e = launch_sweep<T, 4>(a, s); break;
            case 8: e = launch_sweep<T, 8>(a, s); break;
            case 12: e = launch_sweep<T, 12>(a, s); break;
            default: e = launch_sweep<T, 16>(a, s); break;
        }
        if (e != hipSuccess) return e;
    }
    if (weights && STAGED) {
        k_ltva_wstage<<<(unsigned)((size_t)a.B * a.N), 256, 0, s>>>(a);
        e = hipGetLastError();
    } else if (weights) {
        const int slices = std::min(a.B, WSUM_SLICES);
        k_ltva_wsum1<<<slices, 256, 0, s>>>(a, slices);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ltva_wsum2<<<1, 256, sizeof(double) * 2 * wsz, s>>>(a, slices);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace

size_t rqp_ltv_adj_ws_bytes(const rqp_ltv_dims* d) {
    const size_t B = d->batch, N = d->horizon, n = N * d->nu, m = N * (d->nx + d->nu);
    const size_t wsz = (size_t)d->nu * d->nu + (size_t)d->nx * d->nx;
    return sizeof(double) * (B * (m * n + 4 * m + N * wsz) + (size_t)WSUM_SLICES * 2 * wsz);
}

void rqp_ltv_adj_ws_maps(const rqp_ltv_dims* d, void* aw, double** Fb, double** vec) {
    const size_t B = d->batch, N = d->horizon;
    *Fb = (double*)aw;
    *vec = *Fb + B * (N * (d->nx + d->nu)) * (N * d->nu);
}

hipError_t rqp_ltv_launch_condense_adjoint(const rqp_ltv_dims* d, const rqp_ltv_adjoint_io* io, hipStream_t s) {
    return rqp_ltv_launch_condense_adjoint_hooked(d, io, nullptr, s);
}

hipError_t rqp_ltv_launch_condense_adjoint_hooked(const rqp_ltv_dims* d, const rqp_ltv_adjoint_io* io, const rqp_ltv_adj_hooks* hk,
                                                  hipStream_t s) {
    LtvAdjArgs a;
    memset(&a, 0, sizeof(a));
    a.B = d->batch; a.nx = d->nx; a.nu = d->nu; a.N = d->horizon;
    a.blk = d->nx + d->nu; a.n = d->horizon * d->nu; a.m = d->horizon * a.blk;
    a.has_K = (d->flags & RQP_LTV_HAS_K) != 0;
    a.Ad = io->Ad; a.Bd = io->Bd; a.x0 = io->x0;
    a.xref = (d->flags & RQP_LTV_HAS_XREF) ? io->xref : nullptr;
    a.uref = (d->flags & RQP_LTV_HAS_UREF) ? io->uref : nullptr;
    a.Q = io->Q; a.R = io->R; a.Qf = io->Qf; a.K = io->K;
    const size_t B = d->batch, mn = (size_t)a.m * a.n, wsz = (size_t)a.nu * a.nu + (size_t)a.nx * a.nx;
    const double* w = (const double*)io->workspace;                      // the forward layout (rqp_condense.hip: F, W, [G | f], gmap)
    a.F = w;
    a.W = w + B * mn;
    a.Gf = w + 2 * B * mn;
    a.dH = io->dH; a.dA = io->dA; a.dg = io->dg; a.dl = io->dl; a.du = io->du;
    a.dAd = io->dAd; a.dBd = io->dBd; a.dc = io->dc; a.dx0 = io->dx0; a.dxref = io->dxref; a.duref = io->duref;
    a.dQ = io->dQ; a.dR = io->dR; a.dQf = io->dQf;
    double* aw = (double*)io->adjoint_workspace;
    a.TF = aw;
    a.vec = a.TF + B * mn;
    a.wpart = a.vec + B * 4 * a.m;
    a.wsl = a.wpart + B * a.N * wsz;
    if (d->flags & RQP_LTV_STAGE_WEIGHTS)
        return (d->dtype == RQP_F32) ? launch_adjoint_t<float, true>(a, hk, s) : launch_adjoint_t<double, true>(a, hk, s);
    return (d->dtype == RQP_F32) ? launch_adjoint_t<float, false>(a, hk, s) : launch_adjoint_t<double, false>(a, hk, s);
}
