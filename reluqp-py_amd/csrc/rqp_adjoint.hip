// rqp_adjoint.hip -- reverse-mode derivatives of a batched solve (rqp_adjoint, DESIGN.md section 5 "Adjoint (autograd)").
//
// At a solution with sym(H) x + g + A' y = 0 and active set a, the incoming (dx, dy) = (dL/dx, dL/dy) define the adjoint
// system [[sym(H), A_a'], [A_a, 0]] [rx; ry_a] = -[dx; dy_a].  It is solved exactly like polish solves its reduced KKT
// system: regularised by delta, ry eliminated,
//     M rx = r1 + A_a' r2 / delta,   ry_a = (A_a rx - r2) / delta,   (r1, r2) = (-dx, -dy_a),
//     M = sym(H) + delta I + (1 / delta) A' diag(w) A   (w_i = 1 on active rows),
// then refine_iter steps of iterative refinement against the unregularised system.  The masked float64-MFMA gram and the
// factor dispatch of the setup path build M^-1 (float64 output), chunk by chunk.  Then
//     dg = rx,  dl / du = -ry on lower / upper-active rows,  dH = (rx x' + x rx') / 2,  dA = ybar rx' + ry x'.
// Everything reads the CALLER's (H, A, l, u, x, z, y) -- packed here to the handle's row pitch -- never the handle's own
// (possibly scaled) copies.  The chain is data-independent (fixed chunk count, every kernel gated on the per-instance flag):
// rqp_adjoint can be captured in a HIP graph.  Arithmetic is float64 whatever dims.dtype is.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rqp_kkt.h"

namespace {

struct AdjArgs {
    int n, m, ldn, B, b0, refine, shared;
    double delta;
    const void *Ht, *A;                      // packed caller matrices of the chunk ([chunk | 1][n][ldn], [chunk | 1][m][ldn])
    const void *x, *y, *dx, *dy;             // caller [B][n] / [B][m] (dy may be NULL)
    const int8_t* act;                       // [B][m]
    const int32_t* flag;                     // [B]
    const double* Minv;                      // [chunk][n][ldn], instance b0 + blockIdx.x
    void *dg, *dl, *du;                      // caller outputs [B][n] / [B][m] (NULL: skipped)
    int32_t* adj_status;                     // [B] (NULL: skipped)
    double* adj_res;                         // [B] (NULL: skipped)
    double* rows;                            // [B][2 n + 2 m]: rx, x, ry, ybar
};

// ---------------------------------------------------------------------------------------------------------------- pack
// Ht = sym(H) = (H + H')/2 and A with the rows padded to ldn (the setup packers' formulas, k_sym_h / k_pack_mats), for `cnt`
// matrices of the caller's buffers starting at matrix `off`.  One workgroup per matrix; H staged through LDS when it fits.
template <typename T, bool LDS_H>
__global__ void __launch_bounds__(256) k_adj_pack(int n, int m, int ldn, const T* __restrict__ H_in, const T* __restrict__ A_in,
                                                  T* __restrict__ Ht, T* __restrict__ Ap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char adj_pack_raw[];
    const int mat = blockIdx.x, t = threadIdx.x;
    const T* H = H_in + (size_t)mat * n * n;
    const T* A = A_in + (size_t)mat * m * n;
    T* ht = Ht + (size_t)mat * n * ldn;
    T* ap = Ap + (size_t)mat * m * ldn;
    if constexpr (LDS_H) {
        T* st = (T*)adj_pack_raw;
        for (int i = t; i < n * n; i += 256) st[i] = H[i];
        __syncthreads();
        for (int i = t; i < n * ldn; i += 256) {
            const int r = i / ldn, c = i - r * ldn;
            ht[i] = (c < n) ? T(0.5) * (st[c * n + r] + st[r * n + c]) : T(0);
        }
    } else {
        for (int i = t; i < n * ldn; i += 256) {
            const int r = i / ldn, c = i - r * ldn;
            ht[i] = (c < n) ? T(0.5) * (H[(size_t)c * n + r] + H[(size_t)r * n + c]) : T(0);
        }
    }
    for (int i = t; i < m * ldn; i += 256) {
        const int r = i / ldn, c = i - r * ldn;
        ap[i] = (c < n) ? A[(size_t)r * n + c] : T(0);
    }
}

template <typename T>
hipError_t launch_pack(const rqp_handle* h, int cnt, const T* H, const T* A, T* Ht, T* Ap, hipStream_t s) {
    const size_t hb = (size_t)h->n * h->n * sizeof(T);
    if (hb <= 64 * 1024) {
        hipError_t e = rqp_raise_lds_limit((const void*)k_adj_pack<T, true>, hb);
        if (e != hipSuccess) return e;
        k_adj_pack<T, true><<<cnt, 256, hb, s>>>(h->n, h->m, h->ldn, H, A, Ht, Ap);
    } else {
        k_adj_pack<T, false><<<cnt, 256, 0, s>>>(h->n, h->m, h->ldn, H, A, Ht, Ap);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- classify
// flag = (status == solved); the active set from `active` or, in the caller's units, by polish's rule (k_polish_classify):
//   lower-active: z - l < -y;  upper-active (not lower): u - z < y;  inactive otherwise.  0 on skipped instances.
template <typename T>
__global__ void __launch_bounds__(PT) k_adj_classify(int B, int m, const int32_t* __restrict__ status,
                                                     const int8_t* __restrict__ active, const T* __restrict__ z,
                                                     const T* __restrict__ y, const T* __restrict__ l, const T* __restrict__ u,
                                                     int8_t* __restrict__ act, int8_t* __restrict__ act_out,
                                                     int32_t* __restrict__ flag) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool on = status ? status[b] == RQP_STATUS_SOLVED : true;
    if (tid == 0) flag[b] = on ? 1 : 0;
    const size_t o = (size_t)b * m;
    for (int i = tid; i < m; i += PT) {
        int8_t a = 0;
        if (on) {
            if (active) {
                const int8_t v = active[o + i];
                a = v < 0 ? -1 : (v > 0 ? 1 : 0);
            } else {
                const double zi = (double)z[o + i], yi = (double)y[o + i];
                const double li = (double)l[o + i], ui = (double)u[o + i];
                if (zi - li < -yi) a = -1;
                else if (ui - zi < yi) a = 1;
            }
        }
        act[o + i] = a;
        if (act_out) act_out[o + i] = a;
    }
}

// ------------------------------------------------------------------------------------ solve, refine, gradients (per instance)
// One workgroup per instance of the chunk.  LDS: rx, v, t1, t2 [n]; ry, r2, ax, e2 [m]; part [PT]; red [8] (doubles).
template <typename T>
__global__ void __launch_bounds__(PT) k_adjoint(AdjArgs p) {
    extern __shared__ __attribute__((aligned(16))) double asm_[];
    const int b = p.b0 + blockIdx.x;
    if (b >= p.B) return;
    const int n = p.n, m = p.m, ldn = p.ldn, tid = threadIdx.x;
    const size_t ldr = 2 * (size_t)n + 2 * (size_t)m;
    double* rows = p.rows + (size_t)b * ldr;          // rx [n], x [n], ry [m], ybar [m]
    if (!p.flag[b]) {                                 // (uniform) not solved: every gradient 0, residual NaN
        for (size_t i = tid; i < ldr; i += PT) rows[i] = 0.0;
        if (p.dg) for (int c = tid; c < n; c += PT) ((T*)p.dg)[(size_t)b * n + c] = T(0);
        if (p.dl) for (int i = tid; i < m; i += PT) ((T*)p.dl)[(size_t)b * m + i] = T(0);
        if (p.du) for (int i = tid; i < m; i += PT) ((T*)p.du)[(size_t)b * m + i] = T(0);
        if (tid == 0) {
            if (p.adj_status) p.adj_status[b] = 0;
            if (p.adj_res) p.adj_res[b] = __builtin_nan("");
        }
        return;
    }
    double* rx = asm_;
    double* v = rx + n;
    double* t1 = v + n;
    double* t2 = t1 + n;
    double* ry = t2 + n;
    double* r2 = ry + m;
    double* ax = r2 + m;
    double* e2 = ax + m;
    double* part = e2 + m;
    double* red = part + PT;
    const size_t mat = p.shared ? 0 : (size_t)blockIdx.x;
    const T* Ht = (const T*)p.Ht + mat * n * ldn;
    const T* A = (const T*)p.A + mat * m * ldn;
    const T* gx = (const T*)p.dx + (size_t)b * n;
    const T* gy = p.dy ? (const T*)p.dy + (size_t)b * m : nullptr;
    const int8_t* act = p.act + (size_t)b * m;
    const double* Mi = p.Minv + (size_t)blockIdx.x * n * ldn;
    const double idel = 1.0 / p.delta;

    // rx = M^-1 (r1 + A_a' r2 / delta),  ry_a = (A_a rx - r2) / delta,   (r1, r2) = (-dx, -dy_a)
    for (int i = tid; i < m; i += PT) {
        const double ri = (act[i] && gy) ? -(double)gy[i] : 0.0;
        r2[i] = ri;
        ax[i] = ri * idel;
    }
    __syncthreads();
    pcolmv<T>(A, ldn, m, n, ax, t1, part);                             // A_a' r2 / delta
    for (int c = tid; c < n; c += PT) v[c] = t1[c] - (double)gx[c];
    __syncthreads();
    pcolmv<double>(Mi, ldn, n, n, v, rx, part);
    prowmv<T>(A, ldn, m, n, rx, ax);
    for (int i = tid; i < m; i += PT) ry[i] = act[i] ? (ax[i] - r2[i]) * idel : 0.0;
    __syncthreads();

    // iterative refinement against [[sym(H), A_a'], [A_a, 0]] (k_polish's steps): residual (e1, e2) of the unregularised
    // system, correction M drx = e1 + A_a' e2 / delta, dry = (A_a drx - e2) / delta
    for (int k = 0; k < p.refine; ++k) {
        pcolmv<T>(Ht, ldn, n, n, rx, t1, part);                        // H rx
        for (int i = tid; i < m; i += PT) {
            const bool a = act[i] != 0;
            const double ei = a ? r2[i] - ax[i] : 0.0;
            e2[i] = ei;
            ax[i] = a ? ry[i] - ei * idel : 0.0;                       // (ax is recomputed below)
        }
        __syncthreads();
        pcolmv<T>(A, ldn, m, n, ax, t2, part);                         // A_a' (ry - e2 / delta)
        for (int c = tid; c < n; c += PT) v[c] = -(double)gx[c] - t1[c] - t2[c];   // e1 + A_a' e2 / delta
        __syncthreads();
        pcolmv<double>(Mi, ldn, n, n, v, t1, part);                    // drx
        for (int c = tid; c < n; c += PT) rx[c] += t1[c];
        __syncthreads();
        prowmv<T>(A, ldn, m, n, t1, ax);                               // A drx
        for (int i = tid; i < m; i += PT) ry[i] = act[i] ? ry[i] + (ax[i] - e2[i]) * idel : 0.0;
        __syncthreads();
        prowmv<T>(A, ldn, m, n, rx, ax);                               // A rx
    }

    // relative residual |K [rx; ry] + [dx; dy_a]|_inf / max(1, |[dx; dy_a]|_inf)
    pcolmv<T>(Ht, ldn, n, n, rx, t1, part);                            // H rx
    pcolmv<T>(A, ldn, m, n, ry, t2, part);                             // A_a' ry (ry = 0 off the active set)
    double vr = 0.0, vg = 0.0;
    for (int c = tid; c < n; c += PT) {
        const double g = (double)gx[c];
        vr = nmax(vr, fabs(t1[c] + t2[c] + g));
        vg = nmax(vg, fabs(g));
    }
    for (int i = tid; i < m; i += PT) {
        if (act[i]) {
            const double g = -r2[i];
            vr = nmax(vr, fabs(ax[i] + g));
            vg = nmax(vg, fabs(g));
        }
    }
    const double rr = block_reduce<false>(vr, red);
    const double rg = block_reduce<false>(vg, red);

    // gradients and the float64 rows of the matrix-gradient kernels
    const T* xb = (const T*)p.x + (size_t)b * n;
    const T* yb = (const T*)p.y + (size_t)b * m;
    for (int c = tid; c < n; c += PT) {
        rows[c] = rx[c];
        rows[n + c] = (double)xb[c];
        if (p.dg) ((T*)p.dg)[(size_t)b * n + c] = (T)rx[c];
    }
    for (int i = tid; i < m; i += PT) {
        const int a = act[i];
        rows[2 * n + i] = ry[i];
        rows[2 * n + m + i] = a ? (double)yb[i] : 0.0;
        if (p.dl) ((T*)p.dl)[(size_t)b * m + i] = a < 0 ? (T)(-ry[i]) : T(0);
        if (p.du) ((T*)p.du)[(size_t)b * m + i] = a > 0 ? (T)(-ry[i]) : T(0);
    }
    if (tid == 0) {
        if (p.adj_status) p.adj_status[b] = 1;
        if (p.adj_res) p.adj_res[b] = rr / fmax(1.0, rg);
    }
}

// ------------------------------------------------------------------------------------ matrix gradients, per-instance (H, A)
// dH[b] = (rx x' + x rx') / 2 [n][n],  dA[b] = ybar rx' + ry x' [m][n]: one workgroup per instance, its four rows staged in
// LDS, the B (n^2 + m n) elements stored coalesced (row / column advanced incrementally, no division per element).
template <typename T>
__global__ void __launch_bounds__(256) k_adj_outer(int n, int m, const double* __restrict__ rows, T* __restrict__ dH,
                                                   T* __restrict__ dA) {
    extern __shared__ __attribute__((aligned(16))) double orow[];
    const int b = blockIdx.x, t = threadIdx.x;
    const size_t ldr = 2 * (size_t)n + 2 * (size_t)m;
    const double* src = rows + (size_t)b * ldr;
    for (size_t i = t; i < ldr; i += 256) orow[i] = src[i];
    __syncthreads();
    const double* rx = orow;
    const double* x = orow + n;
    const double* ry = orow + 2 * n;
    const double* yb = ry + m;
    const int dr = 256 / n, dc = 256 - dr * n;
    if (dH) {
        T* out = dH + (size_t)b * n * n;
        int r = t / n, c = t - r * n;
        for (int i = t; i < n * n; i += 256) {
            out[i] = (T)(0.5 * (rx[r] * x[c] + x[r] * rx[c]));
            c += dc;
            r += dr;
            if (c >= n) { c -= n; ++r; }
        }
    }
    if (dA) {
        T* out = dA + (size_t)b * m * n;
        int r = t / n, c = t - r * n;
        for (int i = t; i < m * n; i += 256) {
            out[i] = (T)(yb[r] * rx[c] + ry[r] * x[c]);
            c += dc;
            r += dr;
            if (c >= n) { c -= n; ++r; }
        }
    }
}

// --------------------------------------------------------------------------- matrix gradients, shared (H, A): batch GEMMs
// out[r][c] = scale * sum_b (U1[b][r] V1[b][c] + U2[b][r] V2[b][c]) on v_mfma_f64_16x16x4_f64, inner dimension = the batch:
//   dH = (R' X + X' R) / 2   (U1, V1, U2, V2 = rx, x, x, rx; scale 1/2),   dA = Ybar' R + Ry' X   (ybar, rx, ry, x; scale 1).
// One workgroup per 16 x 16 output tile (grid.y: the dH row tiles, then the dA row tiles), its four waves on four fixed
// quarters of the batch, the quarters added in LDS in a fixed order: no atomics, bitwise-reproducible.  Fragment layout as in
// k_gram_mfma (rqp_setup.hip): lane (kq, i16) holds U[b0 + kq][16 I + i16] (A operand) and V[b0 + kq][16 J + i16] (B operand);
// register r of the result is row kq + 4 r, column i16 of the tile.
typedef double adj_d4 __attribute__((ext_vector_type(4)));

template <typename T>
__global__ void __launch_bounds__(256) k_adj_gemm(int n, int m, int B, const double* __restrict__ rows, T* __restrict__ dH,
                                                  T* __restrict__ dA) {
    __shared__ adj_d4 partial[3][64];
    const int ntile = (n + 15) / 16;
    const int J = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, kq = lane >> 4;
    const bool isH = (int)blockIdx.y < ntile;
    const int I = isH ? (int)blockIdx.y : (int)blockIdx.y - ntile;
    T* out = isH ? dH : dA;
    if (!out) return;                                                  // (uniform) that gradient is not requested
    const int R = isH ? n : m;
    const size_t ldr = 2 * (size_t)n + 2 * (size_t)m;
    const int ru = min(16 * I + i16, R - 1), cv = min(16 * J + i16, n - 1);   // (clamped: rows / columns past the end are not stored)
    // column offsets in a row: rx 0, x n, ry 2 n, ybar 2 n + m
    const size_t u1 = isH ? (size_t)ru : 2 * (size_t)n + m + ru;
    const size_t v1 = isH ? (size_t)n + cv : (size_t)cv;
    const size_t u2 = isH ? (size_t)n + ru : 2 * (size_t)n + ru;
    const size_t v2 = isH ? (size_t)cv : (size_t)n + cv;
    const int q = ((B + 15) / 16) * 4;                                 // rows per wave (a multiple of 4)
    const int bb = min(wave * q, B), be = min(bb + q, B);
    adj_d4 acc = (adj_d4){0.0, 0.0, 0.0, 0.0};
    for (int b0 = bb; b0 < be; b0 += 16) {
        double a1[4], w1[4], a2[4], w2[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int b = b0 + 4 * s + kq;
            const bool in = b < be;
            const double* rb = rows + (size_t)(in ? b : bb) * ldr;
            a1[s] = in ? rb[u1] : 0.0;
            w1[s] = in ? rb[v1] : 0.0;
            a2[s] = in ? rb[u2] : 0.0;
            w2[s] = in ? rb[v2] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], w1[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[s], w2[s], acc, 0, 0, 0);
        }
    }
    if (wave > 0) partial[wave - 1][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    const double scale = isH ? 0.5 : 1.0;
    const int c = 16 * J + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * I + kq + 4 * r;
        const double sum = ((acc[r] + partial[0][lane][r]) + partial[1][lane][r]) + partial[2][lane][r];
        if (row < R && c < n) out[(size_t)row * n + c] = (T)(scale * sum);
    }
}

template <typename T>
hipError_t launch_adjoint_t(rqp_handle* h, const rqp_adjoint_io& io, hipStream_t s) {
    const int n = h->n, m = h->m, B = h->B, ldn = h->ldn;
    const bool sh = h->dims.shared_mats != 0;
    k_adj_classify<T><<<B, PT, 0, s>>>(B, m, io.status, io.active, (const T*)io.z, (const T*)io.y, (const T*)io.l,
                                       (const T*)io.u, h->adj_act, io.active_out, h->adj_flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sh) {                                                          // one shared matrix: packed once
        e = launch_pack<T>(h, 1, (const T*)io.H, (const T*)io.A, (T*)h->adj_Ht, (T*)h->adj_A, s);
        if (e != hipSuccess) return e;
    }
    const size_t lds = rqp_adjoint_lds_bytes(h);
    e = rqp_raise_lds_limit((const void*)k_adjoint<T>, lds);
    if (e != hipSuccess) return e;
    AdjArgs p;
    p.n = n; p.m = m; p.ldn = ldn; p.B = B; p.refine = h->adj_refine; p.shared = sh ? 1 : 0;
    p.delta = h->adj_delta;
    p.Ht = h->adj_Ht; p.A = h->adj_A;
    p.x = io.x; p.y = io.y; p.dx = io.dx; p.dy = io.dy;
    p.act = h->adj_act; p.flag = h->adj_flag; p.Minv = h->adj_Minv;
    p.dg = io.dg; p.dl = io.dl; p.du = io.du;
    p.adj_status = io.adj_status; p.adj_res = io.adj_res;
    p.rows = h->adj_rows;
    const int chunk = h->adj_chunk;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int cb = std::min(chunk, B - b0);
        if (!sh) {
            e = launch_pack<T>(h, cb, (const T*)io.H + (size_t)b0 * n * n, (const T*)io.A + (size_t)b0 * m * n, (T*)h->adj_Ht,
                               (T*)h->adj_A, s);
            if (e != hipSuccess) return e;
        }
        SetupArgs f;
        memset(&f, 0, sizeof(f));
        f.n = n; f.m = m; f.ldn = ldn; f.ldm = h->ldm; f.nrho = 1; f.B = B; f.nmat = cb;
        f.sigma = h->adj_delta;
        f.Ht = h->adj_Ht;
        f.A = h->adj_A;
        f.G = h->adj_G;
        f.K = h->adj_Minv;
        f.rhos = h->adj_rho;
        f.fscratch = h->adj_G;                 // (as polish: the factor's global slab may be G_a itself, kwin = 1)
        f.kwin = 1;
        f.only = h->adj_flag + b0;
        f.mats_shared = sh ? 1 : 0;
        f.k_f64 = 1;
        f.pw_act = h->adj_act + (size_t)b0 * m;
        e = rqp_launch_gram_masked(h, f, s);
        if (e != hipSuccess) return e;
        e = rqp_launch_factor(h, f, s);
        if (e != hipSuccess) return e;
        p.b0 = b0;
        k_adjoint<T><<<cb, PT, lds, s>>>(p);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!io.dH && !io.dA) return hipSuccess;
    if (sh) {
        const int nt = (n + 15) / 16, mt = (m + 15) / 16;
        dim3 grid(nt, nt + mt);
        k_adj_gemm<T><<<grid, 256, 0, s>>>(n, m, B, h->adj_rows, (T*)io.dH, (T*)io.dA);
    } else {
        const size_t olds = (2 * (size_t)n + 2 * (size_t)m) * sizeof(double);
        e = rqp_raise_lds_limit((const void*)k_adj_outer<T>, olds);
        if (e != hipSuccess) return e;
        k_adj_outer<T><<<B, 256, olds, s>>>(n, m, h->adj_rows, (T*)io.dH, (T*)io.dA);
    }
    return hipGetLastError();
}

}  // namespace

size_t rqp_adjoint_lds_bytes(const rqp_handle* h) { return (4 * (size_t)h->n + 4 * (size_t)h->m + PT + 8) * sizeof(double); }

hipError_t rqp_launch_adj_pack(const rqp_handle* h, int cnt, const void* H, const void* A, hipStream_t s) {
    if (h->esz == 4) return launch_pack<float>(h, cnt, (const float*)H, (const float*)A, (float*)h->adj_Ht, (float*)h->adj_A, s);
    return launch_pack<double>(h, cnt, (const double*)H, (const double*)A, (double*)h->adj_Ht, (double*)h->adj_A, s);
}

hipError_t rqp_launch_adjoint(rqp_handle* h, const rqp_adjoint_io& io, hipStream_t s) {
    return h->esz == 4 ? launch_adjoint_t<float>(h, io, s) : launch_adjoint_t<double>(h, io, s);
}
