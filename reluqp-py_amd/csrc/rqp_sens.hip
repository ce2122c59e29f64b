// rqp_sens.hip -- forward-mode sensitivities of a batched solve (rqp_sensitivity, DESIGN.md section 5 "Forward sensitivities").
//
// At a solution with sym(H) x + g + A' y = 0 and active set a (the adjoint's classification and sign convention; ybar = y on
// a, 0 elsewhere), tangents (dH, dg, dA, dl, du) -- db_i = dl_i on lower-active rows, du_i on upper-active ones -- give
//     [[sym(H), A_a'], [A_a, 0]] [dx; dy_a] = [r1; r2] = [-(sym(dH) x + dg + dA' ybar);  db_a - dA_a x],
//     dy_i = 0 off a,   dz = A dx + dA x.
// This is the adjoint's matrix (the KKT matrix is symmetric): the same masked gram and factor build M^-1 =
// (sym(H) + delta I + A_a' A_a / delta)^-1 once per chunk, and the system is solved exactly like k_adjoint solves its own,
//     dx = M^-1 (r1 + A_a' r2 / delta),   dy_a = (A_a dx - r2) / delta,
// then refine_iter steps of iterative refinement against the unregularised matrix -- for 16 directions at a time, the
// directions on the N axis of v_mfma_f64_16x16x4_f64.  Every product is an n x n x 16 or m_a x n x 16 tile GEMM:
//     M^-1 V and sym(H) X (n x n, float64 / dims.dtype),  A_a X (m_a x n),  A_a' W (n x m_a).
// Column j of every result depends on direction j alone (an MFMA output column reads one B column; every other step is
// elementwise or a per-column sum in a fixed order): a direction gives the same bits whichever block it shares.
//
// Layout.  One workgroup (4 waves) per instance; the waves split the 16-row output tiles of each product.  The n-side blocks
// X, V, T ([n16][16] float64, n16 = n rounded up to 16) live in LDS: 384 n16 bytes (43 KB at n = 100; 123 KB at the sparse
// MPC's n = 320).  The row-side blocks are compacted to the m_a active rows (index list built by k_sens_classify) and kept in a
// per-instance global workspace, L2-resident while the workgroup runs: r2, Y = dy_a and AX = A_a X ([m][16] float64 each,
// m_a rows used), with r1 ([n][16]) and q = dA x ([m][16], for dz) from k_sens_rhs.  Widening the adjoint's eight LDS vectors
// to 16 columns would need 128 (4 n + 4 m) bytes -- 200 KB at (100, 300), 450 KB at (320, 560) -- above the 160 KB of a CU.
// Everything reads the CALLER's data, packed like the adjoint's; the chain is data-independent (capturable).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rqp_kkt.h"

namespace {

constexpr int ND = 16;    // directions per block: the N axis of one MFMA tile
typedef double sd4 __attribute__((ext_vector_type(4)));

struct SensArgs {
    int n, m, ldn, B, b0, refine, shared, ndir, d0, nd, tshared, want_q;
    double delta;
    const void *Ht, *A;                      // packed caller matrices of the chunk ([chunk | 1][n][ldn], [chunk | 1][m][ldn])
    const void *x, *y;                       // caller [B][n], [B][m]
    const void *dH, *dg, *dA, *dl, *du;      // caller tangents, direction axis last (NULL: zero)
    const int8_t* act;                       // [B][m]
    const int32_t* flag;                     // [B]
    const int32_t *idx, *pos, *na;           // [B][m] active row list, [B][m] row -> list position (-1), [B] list length
    const double* Minv;                      // [chunk][n][ldn]
    double* ws;                              // [chunk][n + 4 m][16]: r1, r2, Y, AX, q
    void *dx, *dy, *dz;                      // caller outputs [B][n | m][ndir] (dy, dz NULL: skipped)
    int32_t* sens_status;                    // [B] (NULL: skipped)
    double* sens_res;                        // [B] (NULL: skipped)
};

// --------------------------------------------------------------------------------------------------------------- classify
// The adjoint's rule (k_adj_classify): flag = (status == solved); the set from `active` or lower-active z - l < -y,
// upper-active (not lower) u - z < y.  Plus the list of active rows in ascending order (a wave-ballot prefix sum).
template <typename T>
__global__ void __launch_bounds__(PT) k_sens_classify(int B, int m, const int32_t* __restrict__ status,
                                                      const int8_t* __restrict__ active, const T* __restrict__ z,
                                                      const T* __restrict__ y, const T* __restrict__ l, const T* __restrict__ u,
                                                      int8_t* __restrict__ act, int8_t* __restrict__ act_out,
                                                      int32_t* __restrict__ flag, int32_t* __restrict__ idx,
                                                      int32_t* __restrict__ pos, int32_t* __restrict__ na) {
    __shared__ int wcnt[PT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool on = status ? status[b] == RQP_STATUS_SOLVED : true;
    if (tid == 0) flag[b] = on ? 1 : 0;
    const size_t o = (size_t)b * m;
    int base = 0;
    for (int i0 = 0; i0 < m; i0 += PT) {
        const int i = i0 + tid;
        int8_t a = 0;
        if (on && i < m) {
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
        const unsigned long long bal = __ballot(a != 0);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wcnt[w];
        if (i < m) {
            act[o + i] = a;
            if (act_out) act_out[o + i] = a;
            pos[o + i] = a ? off + before : -1;
            if (a) idx[o + off + before] = i;
        }
        base += ((wcnt[0] + wcnt[1]) + wcnt[2]) + wcnt[3];
        __syncthreads();
    }
    if (tid == 0) na[b] = base;
}

// -------------------------------------------------------------------------------------------------------- right-hand sides
// One workgroup per instance of the chunk, thread (row group tid / 16, direction tid % 16).  Tangent element (row, col,
// direction d0 + d) of instance b; tangents flagged in tshared are read at instance 0.  Sums run over their index in order.
//   r1[c][d] = -(sum_k (dH[c][k] + dH[k][c]) / 2 x[k] + dg[c] + sum_j dA[idx j][c] y[idx j])
//   r2[j][d] = db[idx j] - sum_k dA[idx j][k] x[k]        q[i][d] = sum_k dA[i][k] x[k]   (want_q)
// Directions d >= nd of the block are 0.
template <typename T>
__global__ void __launch_bounds__(PT) k_sens_rhs(SensArgs p) {
    extern __shared__ __attribute__((aligned(16))) double srhs[];
    const int b = p.b0 + blockIdx.x;
    if (b >= p.B || !p.flag[b]) return;
    const int n = p.n, m = p.m, tid = threadIdx.x, d = tid & (ND - 1), rg = tid / ND;
    const int cnt = p.na[b];
    double* xs = srhs;                                     // x [n], ybar [m]
    double* ys = xs + n;
    const T* xb = (const T*)p.x + (size_t)b * n;
    const T* yb = (const T*)p.y + (size_t)b * m;
    const int8_t* act = p.act + (size_t)b * m;
    for (int c = tid; c < n; c += PT) xs[c] = (double)xb[c];
    for (int i = tid; i < m; i += PT) ys[i] = act[i] ? (double)yb[i] : 0.0;
    __syncthreads();
    const int32_t* idx = p.idx + (size_t)b * m;
    const bool live = d < p.nd;
    const size_t nd = p.ndir, dd = (size_t)p.d0 + d;
    auto inst = [&](int bit) { return (p.tshared & bit) ? (size_t)0 : (size_t)b; };
    const T* dH = p.dH ? (const T*)p.dH + inst(RQP_SENS_SHARED_DH) * n * n * nd : nullptr;
    const T* dg = p.dg ? (const T*)p.dg + inst(RQP_SENS_SHARED_DG) * n * nd : nullptr;
    const T* dA = p.dA ? (const T*)p.dA + inst(RQP_SENS_SHARED_DA) * m * n * nd : nullptr;
    const T* dl = p.dl ? (const T*)p.dl + inst(RQP_SENS_SHARED_DL) * m * nd : nullptr;
    const T* du = p.du ? (const T*)p.du + inst(RQP_SENS_SHARED_DU) * m * nd : nullptr;
    double* ws = p.ws + (size_t)blockIdx.x * (n + 4 * (size_t)m) * ND;
    double* r1 = ws;
    double* r2 = r1 + (size_t)n * ND;
    double* q = r2 + 3 * (size_t)m * ND;
    for (int c = rg; c < n; c += PT / ND) {
        double acc = 0.0;
        if (live) {
            if (dH)
                for (int k = 0; k < n; ++k)
                    acc = fma(0.5 * ((double)dH[((size_t)c * n + k) * nd + dd] + (double)dH[((size_t)k * n + c) * nd + dd]), xs[k], acc);
            if (dg) acc += (double)dg[(size_t)c * nd + dd];
            if (dA)
                for (int j = 0; j < cnt; ++j) {
                    const int i = idx[j];
                    acc = fma((double)dA[((size_t)i * n + c) * nd + dd], ys[i], acc);
                }
        }
        r1[(size_t)c * ND + d] = -acc;
    }
    for (int j = rg; j < cnt; j += PT / ND) {
        const int i = idx[j];
        double v = 0.0;
        if (live) {
            const T* db = act[i] < 0 ? dl : du;
            double ax = 0.0;
            if (dA)
                for (int k = 0; k < n; ++k) ax = fma((double)dA[((size_t)i * n + k) * nd + dd], xs[k], ax);
            v = (db ? (double)db[(size_t)i * nd + dd] : 0.0) - ax;
        }
        r2[(size_t)j * ND + d] = v;
    }
    if (p.want_q)
        for (int i = rg; i < m; i += PT / ND) {
            double ax = 0.0;
            if (live && dA)
                for (int k = 0; k < n; ++k) ax = fma((double)dA[((size_t)i * n + k) * nd + dd], xs[k], ax);
            q[(size_t)i * ND + d] = ax;
        }
}

// ------------------------------------------------------------------------------------------------------- tile products
// v_mfma_f64_16x16x4_f64 fragments (as k_adj_gemm): lane (kq = lane / 16, i16 = lane % 16) holds A[row i16][k kq] and
// B[k kq][column i16]; result register r is row kq + 4 r, column i16.  Columns are the 16 directions throughout.

// out[c][d] = sum_r Mat[r][c] Bm[r][d]  (c < n16; Mat n x n, pitch ld; Bm, out: LDS [n16][16]).  Rows c >= n come out 0.
template <typename MT>
__device__ void mul_nn(const MT* __restrict__ Mat, int ld, int n, const double* Bm, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, i16 = lane & 15;
    const int nt = (n + 15) / 16;
    for (int I = wave; I < nt; I += PT / 64) {
        const int c = 16 * I + i16;
        const bool cin = c < n;
        const MT* col = Mat + (cin ? c : 0);
        sd4 acc = (sd4){0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < n; k += 4) {
            const int r = k + kq;
            const bool in = r < n;
            const double a = (in && cin) ? (double)col[(size_t)r * ld] : 0.0;
            const double bv = in ? Bm[r * ND + i16] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(16 * I + kq + 4 * q) * ND + i16] = acc[q];
    }
}

// Row-side epilogues of mul_rows: acc = (A_a X)[j][d] at element e = j * 16 + d of the instance's blocks.
enum { ROWS_INIT = 0, ROWS_CORR = 1, ROWS_SET = 2, ROWS_DZ = 3 };

// acc[j][d] = sum_c A[row j][c] Bm[c][d] for j < cnt (row j = idx[j], or j when idx is NULL); Bm: LDS [n16][16].
//   INIT: AX = acc, Y = (acc - r2) / delta      CORR: Y += (acc - (r2 - AX)) / delta      SET: AX = acc
//   DZ:   out[row j][d0 + d] = acc (+ q[j][d])  (d < nd; the caller's dz)
template <int MODE, typename T>
__device__ void mul_rows(const T* __restrict__ A, int ld, int n, const int32_t* __restrict__ idx, int cnt, const double* Bm,
                         const double* __restrict__ r2, double* __restrict__ AX, double* __restrict__ Y, double idel,
                         const double* __restrict__ q, T* __restrict__ out, size_t ndir, int d0, int nd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, i16 = lane & 15;
    const int jt = (cnt + 15) / 16;
    for (int J = wave; J < jt; J += PT / 64) {
        const int j = 16 * J + i16;
        const bool jin = j < cnt;
        const T* row = A + (size_t)(jin ? (idx ? idx[j] : j) : 0) * ld;
        sd4 acc = (sd4){0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < n; k += 4) {
            const int c = k + kq;
            const bool in = c < n;
            const double a = (in && jin) ? (double)row[c] : 0.0;
            const double bv = in ? Bm[c * ND + i16] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int jr = 16 * J + kq + 4 * s;
            if (jr >= cnt) continue;
            const size_t e = (size_t)jr * ND + i16;
            if constexpr (MODE == ROWS_INIT) {
                AX[e] = acc[s];
                Y[e] = (acc[s] - r2[e]) * idel;
            } else if constexpr (MODE == ROWS_CORR) {
                Y[e] = Y[e] + (acc[s] - (r2[e] - AX[e])) * idel;
            } else if constexpr (MODE == ROWS_SET) {
                AX[e] = acc[s];
            } else {
                if (i16 < nd) {
                    const int i = idx ? idx[jr] : jr;
                    out[(size_t)i * ndir + d0 + i16] = (T)(q ? acc[s] + q[e] : acc[s]);
                }
            }
        }
    }
}

// Column side of A_a: out[c][d] = sum_j A[idx j][c] W[j][d] (c < n16; out: LDS), W from the row-side blocks:
//   W_R2: r2 / delta      W_REF: Y - (r2 - AX) / delta      W_Y: Y
enum { W_R2 = 0, W_REF = 1, W_Y = 2 };

template <int WM, typename T>
__device__ void mul_cols(const T* __restrict__ A, int ld, int n, const int32_t* __restrict__ idx, int cnt,
                         const double* __restrict__ r2, const double* __restrict__ AX, const double* __restrict__ Y, double idel,
                         double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4, i16 = lane & 15;
    const int nt = (n + 15) / 16;
    for (int I = wave; I < nt; I += PT / 64) {
        const int c = 16 * I + i16;
        const bool cin = c < n;
        sd4 acc = (sd4){0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < cnt; k += 4) {
            const int j = k + kq;
            const bool in = j < cnt;
            const size_t e = (size_t)(in ? j : 0) * ND + i16;
            const double a = (in && cin) ? (double)A[(size_t)idx[j] * ld + c] : 0.0;
            double w = 0.0;
            if (in) {
                if constexpr (WM == W_R2) w = r2[e] * idel;
                else if constexpr (WM == W_REF) w = Y[e] - (r2[e] - AX[e]) * idel;
                else w = Y[e];
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(16 * I + kq + 4 * q) * ND + i16] = acc[q];
    }
}

// ------------------------------------------------------------------------------------ solve, refine, outputs (per instance)
// One workgroup per instance of the chunk, one block of up to 16 directions (d0, nd).  LDS: X, V, T [n16][16]; part [PT]
// (doubles).  Rows n..n16 of X, V, T are written by the products (as 0) and never read as operands.
template <typename T>
__global__ void __launch_bounds__(PT) k_sens_solve(SensArgs p) {
    extern __shared__ __attribute__((aligned(16))) double ssm[];
    const int b = p.b0 + blockIdx.x;
    if (b >= p.B) return;
    const int n = p.n, m = p.m, ldn = p.ldn, tid = threadIdx.x, nd = p.nd, d0 = p.d0;
    const size_t ndir = p.ndir;
    if (!p.flag[b]) {                                 // (uniform) not solved: zero tangents, status 0, residual NaN
        for (int e = tid; e < n * ND; e += PT)
            if ((e & (ND - 1)) < nd) ((T*)p.dx)[((size_t)b * n + e / ND) * ndir + d0 + (e & (ND - 1))] = T(0);
        for (int e = tid; e < m * ND; e += PT) {
            if ((e & (ND - 1)) >= nd) continue;
            const size_t o = ((size_t)b * m + e / ND) * ndir + d0 + (e & (ND - 1));
            if (p.dy) ((T*)p.dy)[o] = T(0);
            if (p.dz) ((T*)p.dz)[o] = T(0);
        }
        if (tid == 0) {
            if (p.sens_status) p.sens_status[b] = 0;
            if (p.sens_res) p.sens_res[b] = __builtin_nan("");
        }
        return;
    }
    const int n16 = (n + 15) / 16 * 16;
    double* X = ssm;
    double* V = X + n16 * ND;
    double* Tb = V + n16 * ND;
    double* part = Tb + n16 * ND;
    const size_t mat = p.shared ? 0 : (size_t)blockIdx.x;
    const T* Ht = (const T*)p.Ht + mat * n * ldn;
    const T* A = (const T*)p.A + mat * m * ldn;
    const double* Mi = p.Minv + (size_t)blockIdx.x * n * ldn;
    const int32_t* idx = p.idx + (size_t)b * m;
    const int cnt = p.na[b];
    double* r1 = p.ws + (size_t)blockIdx.x * (n + 4 * (size_t)m) * ND;
    double* r2 = r1 + (size_t)n * ND;
    double* Y = r2 + (size_t)m * ND;
    double* AX = Y + (size_t)m * ND;
    double* q = AX + (size_t)m * ND;
    const double idel = 1.0 / p.delta;

    // X = M^-1 (r1 + A_a' r2 / delta),  Y = (A_a X - r2) / delta
    mul_cols<W_R2, T>(A, ldn, n, idx, cnt, r2, AX, Y, idel, Tb);
    __syncthreads();
    for (int e = tid; e < n * ND; e += PT) V[e] = r1[e] + Tb[e];
    __syncthreads();
    mul_nn<double>(Mi, ldn, n, V, X);
    __syncthreads();
    mul_rows<ROWS_INIT, T>(A, ldn, n, idx, cnt, X, r2, AX, Y, idel, nullptr, nullptr, 0, 0, 0);
    __syncthreads();

    // iterative refinement (k_adjoint's steps): E2 = r2 - AX, V = r1 - H X - A_a' (Y - E2 / delta), D = M^-1 V,
    // Y += (A_a D - E2) / delta, X += D, AX = A_a X
    for (int k = 0; k < p.refine; ++k) {
        mul_nn<T>(Ht, ldn, n, X, Tb);                                        // H X
        mul_cols<W_REF, T>(A, ldn, n, idx, cnt, r2, AX, Y, idel, V);         // A_a' (Y - E2 / delta)
        __syncthreads();
        for (int e = tid; e < n * ND; e += PT) V[e] = r1[e] - Tb[e] - V[e];
        __syncthreads();
        mul_nn<double>(Mi, ldn, n, V, Tb);                                   // D
        __syncthreads();
        mul_rows<ROWS_CORR, T>(A, ldn, n, idx, cnt, Tb, r2, AX, Y, idel, nullptr, nullptr, 0, 0, 0);
        for (int e = tid; e < n * ND; e += PT) X[e] += Tb[e];
        __syncthreads();
        mul_rows<ROWS_SET, T>(A, ldn, n, idx, cnt, X, r2, AX, Y, idel, nullptr, nullptr, 0, 0, 0);
        __syncthreads();
    }

    // relative residual per direction |K [X; Y] - [r1; r2]|_inf / max(1, |[r1; r2]|_inf), the maximum over the block
    mul_nn<T>(Ht, ldn, n, X, Tb);                                            // H X
    mul_cols<W_Y, T>(A, ldn, n, idx, cnt, r2, AX, Y, idel, V);               // A_a' Y
    __syncthreads();
    double vr = 0.0, vg = 0.0;                                               // (thread tid: direction tid % 16 throughout)
    for (int e = tid; e < n * ND; e += PT) {
        vr = nmax(vr, fabs(Tb[e] + V[e] - r1[e]));
        vg = nmax(vg, fabs(r1[e]));
    }
    for (int e = tid; e < cnt * ND; e += PT) {
        vr = nmax(vr, fabs(AX[e] - r2[e]));
        vg = nmax(vg, fabs(r2[e]));
    }
    part[tid] = vr;
    __syncthreads();
    if (tid < ND) {
        for (int s = 1; s < PT / ND; ++s) vr = nmax(vr, part[s * ND + tid]);
    }
    __syncthreads();
    part[tid] = vg;
    __syncthreads();
    if (tid < ND) {
        for (int s = 1; s < PT / ND; ++s) vg = nmax(vg, part[s * ND + tid]);
    }
    __syncthreads();
    if (tid < ND) part[tid] = tid < nd ? vr / fmax(1.0, vg) : 0.0;
    __syncthreads();
    if (tid == 0) {
        double r = part[0];
        for (int d = 1; d < ND; ++d) r = nmax(r, part[d]);
        if (p.sens_status) p.sens_status[b] = 1;
        if (p.sens_res) p.sens_res[b] = d0 == 0 ? r : nmax(p.sens_res[b], r);
    }

    // outputs: dx, dy (0 off the active set), dz = A X + dA x
    for (int e = tid; e < n * ND; e += PT)
        if ((e & (ND - 1)) < nd) ((T*)p.dx)[((size_t)b * n + e / ND) * ndir + d0 + (e & (ND - 1))] = (T)X[e];
    if (p.dy) {
        const int32_t* pos = p.pos + (size_t)b * m;
        for (int e = tid; e < m * ND; e += PT) {
            const int d = e & (ND - 1), i = e / ND;
            if (d >= nd) continue;
            const int j = pos[i];
            ((T*)p.dy)[((size_t)b * m + i) * ndir + d0 + d] = j >= 0 ? (T)Y[(size_t)j * ND + d] : T(0);
        }
    }
    if (p.dz)
        mul_rows<ROWS_DZ, T>(A, ldn, n, nullptr, m, X, nullptr, nullptr, nullptr, 0.0, p.want_q ? q : nullptr,
                             (T*)p.dz + (size_t)b * m * ndir, ndir, d0, nd);
}

template <typename T>
hipError_t launch_sens_t(rqp_handle* h, const rqp_sensitivity_io& io, hipStream_t s) {
    const int n = h->n, m = h->m, B = h->B, ldn = h->ldn;
    const bool sh = h->dims.shared_mats != 0;
    k_sens_classify<T><<<B, PT, 0, s>>>(B, m, io.status, io.active, (const T*)io.z, (const T*)io.y, (const T*)io.l,
                                        (const T*)io.u, h->adj_act, io.active_out, h->adj_flag, h->sens_idx, h->sens_pos,
                                        h->sens_na);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sh) {                                                          // one shared matrix: packed once
        e = rqp_launch_adj_pack(h, 1, io.H, io.A, s);
        if (e != hipSuccess) return e;
    }
    const size_t lds = rqp_sens_lds_bytes(h), rlds = ((size_t)n + m) * sizeof(double);
    e = rqp_raise_lds_limit((const void*)k_sens_solve<T>, lds);
    if (e != hipSuccess) return e;
    e = rqp_raise_lds_limit((const void*)k_sens_rhs<T>, rlds);
    if (e != hipSuccess) return e;
    SensArgs p;
    memset(&p, 0, sizeof(p));
    p.n = n; p.m = m; p.ldn = ldn; p.B = B; p.refine = h->adj_refine; p.shared = sh ? 1 : 0;
    p.ndir = io.ndir; p.tshared = io.shared_tangents;
    p.want_q = (io.dz && io.dA) ? 1 : 0;
    p.delta = h->adj_delta;
    p.Ht = h->adj_Ht; p.A = h->adj_A;
    p.x = io.x; p.y = io.y;
    p.dH = io.dH; p.dg = io.dg; p.dA = io.dA; p.dl = io.dl; p.du = io.du;
    p.act = h->adj_act; p.flag = h->adj_flag; p.idx = h->sens_idx; p.pos = h->sens_pos; p.na = h->sens_na;
    p.Minv = h->adj_Minv; p.ws = h->sens_ws;
    p.dx = io.dx; p.dy = io.dy; p.dz = io.dz;
    p.sens_status = io.sens_status; p.sens_res = io.sens_res;
    const int chunk = h->adj_chunk;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int cb = std::min(chunk, B - b0);
        if (!sh) {
            e = rqp_launch_adj_pack(h, cb, (const T*)io.H + (size_t)b0 * n * n, (const T*)io.A + (size_t)b0 * m * n, s);
            if (e != hipSuccess) return e;
        }
        SetupArgs f;                                                   // (the adjoint's gram and factor: one M^-1 per chunk)
        memset(&f, 0, sizeof(f));
        f.n = n; f.m = m; f.ldn = ldn; f.ldm = h->ldm; f.nrho = 1; f.B = B; f.nmat = cb;
        f.sigma = h->adj_delta;
        f.Ht = h->adj_Ht;
        f.A = h->adj_A;
        f.G = h->adj_G;
        f.K = h->adj_Minv;
        f.rhos = h->adj_rho;
        f.fscratch = h->adj_G;
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
        for (int d0 = 0; d0 < io.ndir; d0 += ND) {                     // one block of <= 16 directions against the same M^-1
            p.d0 = d0;
            p.nd = std::min(ND, io.ndir - d0);
            k_sens_rhs<T><<<cb, PT, rlds, s>>>(p);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
            k_sens_solve<T><<<cb, PT, lds, s>>>(p);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace

size_t rqp_sens_lds_bytes(const rqp_handle* h) {
    const size_t n16 = ((size_t)h->n + 15) / 16 * 16;
    return (3 * n16 * ND + PT) * sizeof(double);
}

size_t rqp_sens_ws_doubles(const rqp_handle* h) { return ((size_t)h->n + 4 * (size_t)h->m) * ND; }

hipError_t rqp_launch_sensitivity(rqp_handle* h, const rqp_sensitivity_io& io, hipStream_t s) {
    return h->esz == 4 ? launch_sens_t<float>(h, io, s) : launch_sens_t<double>(h, io, s);
}
