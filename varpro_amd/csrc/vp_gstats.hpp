// vp_gstats.hpp -- fit statistics of GLOBAL fits (one alpha shared by S right-hand sides; vp_global_statistics).
//
// == FitStatistics::try_calculate (src/statistics/mod.rs:352-441) on the equivalent single-RHS problem: observations vec(Y)
// (m S rows, stacked weights W), parameters theta = [c_1 .. c_S, alpha], model (I_S (x) Phi) vec(C), so
//      H = W [I_S (x) Phi | D],   D_s[:,k] = sum_{p in k} c_{s,j(p)} dPhi_p
//      sigma^2 = sum_s ||r_w,s||^2 / (m S - n S - q),   Cov = sigma^2 (H^T H)^-1,   band_{s,i} = sqrt(j_{s,i}^T Cov j_{s,i})
// without forming anything of size (n S + q)^2.  With W Phi = Q R, P_perp = I - Q Q^T:
//      E = R^-1 Q^T W dPhi (n x P),  G_p = P_perp W dPhi_p,  F_p = dPhi_p - Phi E[:,p] (unweighted),
//      K_s[:,k] = sum_{p in k} c_{s,j(p)} E[:,p]
//      M[k,l] = sum_{p in k, p' in l} (G_p^T G_p') sum_s c_{s,j(p)} c_{s,j(p')}      (Schur complement of H^T H)
//      Cov_aa = sigma^2 M^-1,  Cov(c_s,c_s) = sigma^2 R^-1 R^-T + K_s Cov_aa K_s^T,  Cov(c_s,alpha) = -K_s Cov_aa
//      band_{s,i}^2 = sigma^2 ||R^-T phi_i^T||^2 + u Cov_aa u^T,   u_k = sum_{p in k} c_{s,j(p)} F_p[i]
//                   = L_i + c_s^T N_i c_s,   N_i[j][j'] = sum_{p: j(p)=j, p': j(p')=j'} F_p[i] F_p'[i] Cov_aa[k(p)][k(p')]
// Model-agnostic: the kernels READ the unweighted columns Phi [B][n][rows], dPhi [B][P][rows] (a descriptor handle fills a
// workspace with its vp_basis kernel, a caller-evaluated handle holds them already).  Instantiated on the dtype only; n, q,
// P are run-time values (<= VP_MAX_BASIS, VP_MAX_PARAMS, VP_MAX_PAIRS).  Everything is accumulated in double.
//   gstats_prep   one workgroup per problem: Householder QR of W Phi over a global-memory workspace (the multi-dot sweep and
//                 reductions of vp_generic.hpp), R^-1, E, G^T G, and per row the leverage and F_p
//   gstats_reduce one workgroup per problem: sum_s c_s c_s^T in a fixed order, M, its Cholesky factor, Cov_aa, sigma^2, status;
//                 per row L_i and N_i (the band's row constants)
//   gstats_band   the hot path: grid (problem x RHS chunk, row tile); a lane holds its row's L_i and N_i in registers and
//                 walks the chunk's right-hand sides (c_s: wave-uniform loads), one coalesced non-temporal store per value
//   gstats_blocks grid (problem x 32 right-hand sides): the O(n^2 q) blocks Cov(c_s,c_s) and Cov(c_s,alpha)
#pragma once
#include "vp_generic.hpp"

namespace vp {

enum { VP_ST_GSTATS_FAILED = 4 }; // Underdetermined / MatrixInversion (src/statistics/mod.rs:15-25)

// type-erased launch record of vp_global_statistics (vp_api.hip); every pointer is a device pointer, already offset to the
// first problem of the launch
struct GStatsParams {
    int dtype, n, q, P;
    int32_t pb[VP_MAX_PAIRS], pp[VP_MAX_PAIRS]; // pair -> basis, parameter
    int m;             // rows of the handle
    int rows;          // rows per column of phi / dphi (< m: the rows beyond are zero)
    int64_t m_dof;     // the caller's rows (the degrees of freedom count these)
    int S;
    int64_t B;         // problems of this launch
    const void *phi, *dphi;  // [B][n][rows], [B][P][rows] UNweighted
    const void *w;           // [m] / [B][m] / null
    int64_t w_stride;
    const void *C;           // [B][S][n]
    const double *cost;      // [B] 1/2 sum_s ||r_w,s||^2
    const int32_t *status_in; // [B]
    double *ws_cols;   // [B][n + P][m] workspace
    double *ws_small;  // [B][kGsSmall]
    double *ws_rows;   // [B][1 + n(n+1)/2][m] or null (no band)
    void *cov_alpha;   // [B][q][q]
    double *chi2;      // [B]
    void *coef_cov;    // [B][S][n][n] or null
    void *coef_alpha_cov; // [B][S][n][q] or null
    void *band;        // [B][S][m] or null
    int32_t *status_out; // [B]
    hipStream_t stream;
};
int gstats_launch(const GStatsParams &p);

namespace gs {

constexpr int TB = gen::TB;
constexpr int NMAX = VP_MAX_BASIS, QMAX = VP_MAX_PARAMS, PMAX = VP_MAX_PAIRS;
constexpr int NNMAX = NMAX * (NMAX + 1) / 2;
// per-problem record in ws_small (doubles)
constexpr int OFF_RI = 0;                       // R^-1           [NMAX][NMAX]
constexpr int OFF_E = OFF_RI + NMAX * NMAX;     // E              [NMAX][PMAX]
constexpr int OFF_GG = OFF_E + NMAX * PMAX;     // G^T G          [PMAX][PMAX]
constexpr int OFF_RR = OFF_GG + PMAX * PMAX;    // R^-1 R^-T      [NMAX][NMAX]
constexpr int OFF_COV = OFF_RR + NMAX * NMAX;   // Cov_aa         [QMAX][QMAX]
constexpr int OFF_SIG2 = OFF_COV + QMAX * QMAX; // sigma^2 (NaN unless ok)
constexpr int OFF_OKR = OFF_SIG2 + 1;           // 1: every pivot of R non-zero and finite
constexpr int OFF_OK = OFF_OKR + 1;             // 1: status ok
constexpr int kGsSmall = OFF_OK + 8;
constexpr int kBandChunk = 64;   // right-hand sides per band workgroup
constexpr int kBlockRhs = TB / NMAX; // right-hand sides per blocks workgroup

template <typename T> struct GsArgs {
    int n, q, P, m, rows, S;
    int32_t pb[PMAX], pp[PMAX];
    int64_t B, m_dof, w_stride;
    int nchunk; // band: right-hand-side chunks per problem
    const T *phi, *dphi, *w, *C;
    const double *cost;
    const int32_t *status_in;
    double *ws_cols, *ws_small, *ws_rows;
    T *cov_alpha, *coef_cov, *coef_alpha_cov, *band;
    double *chi2;
    int32_t *status_out;
};

__host__ __device__ constexpr int n_tri(int n) { return n * (n + 1) / 2; }
// column of N_i[j][j'] (j <= j' < n) in the row workspace: column 0 is L_i
__host__ __device__ constexpr int tri_col(int j, int jp, int n) { return 1 + j * n - j * (j - 1) / 2 + (jp - j); }

template <typename T> __global__ void __launch_bounds__(TB) gstats_prep_kernel(const GsArgs<T> a) {
    __shared__ gen::GenShared<double> sh;
    __shared__ double Rm[NMAX][NMAX], Ri[NMAX][NMAX], E[NMAX][PMAX];
    __shared__ int s_okr;
    const int tid = (int)threadIdx.x, n = a.n, P = a.P, m = a.m, rows = a.rows, NC = a.n + a.P;
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;
    double *ws = a.ws_cols + b * (int64_t)NC * m;
    double *sm = a.ws_small + b * (int64_t)kGsSmall;
    auto col = [&](int c) { return ws + (int64_t)c * m; };
    const T *ph = a.phi + b * (int64_t)n * rows;
    const T *dp = a.dphi ? a.dphi + b * (int64_t)P * rows : nullptr;
    const T *wp = a.w ? a.w + b * a.w_stride : nullptr;
    // W Phi | W dPhi
    for (int i = tid; i < m; i += TB) {
        const bool in = i < rows;
        const double sc = wp ? (double)wp[i] : 1.0;
        for (int j = 0; j < n; ++j) col(j)[i] = in ? (double)ph[(int64_t)j * rows + i] * sc : 0.0;
        for (int p = 0; p < P; ++p) col(n + p)[i] = (in && dp) ? (double)dp[(int64_t)p * rows + i] * sc : 0.0;
    }
    __syncthreads();
    // Householder sweep of the n basis columns applied to the P derivative columns (vp_generic.hpp evaluate)
    for (int k = 0; k < n; ++k) {
        const int nv = NC - k;
        const double *ak = col(k);
        for (int v = 0; v < nv; ++v) {
            const double *cv = col(k + v);
            double acc = 0.0;
            for (int i = k + tid; i < m; i += TB) acc = tfma(ak[i], cv[i], acc);
            gen::reduce_put(sh, v, acc);
        }
        gen::reduce_finish(sh, nv);
        if (tid == 0) {
            const double alpha = ak[k], nrm2 = sh.red[0];
            const bool live = nrm2 > num<double>::norm2_min && is_finite(nrm2);
            const double sigma = live ? tsqrt(nrm2) : 0.0;
            const double beta = live ? -tcopysign(sigma, alpha) : ((nrm2 <= num<double>::norm2_min) ? alpha : nrm2);
            const double u = live ? alpha - beta : 0.0;
            const double gk = live ? 1.0 / (beta * u) : 0.0;
            Rm[k][k] = beta;
            sh.f[0] = u;
            for (int v = 1; v < nv; ++v) {
                const double top = col(k + v)[k];
                const double f = gk * tfma(-beta, top, sh.red[v]);
                sh.f[v] = f;
                if (k + v < n) Rm[k][k + v] = tfma(f, u, top);
                else col(k + v)[k] = tfma(f, u, top); // (row k of a derivative column: written below by the same value)
            }
        }
        __syncthreads();
        {
            double *akw = col(k);
            if (tid == 0) akw[k] = sh.f[0];
            __syncthreads();
            for (int i = k + 1 + tid; i < m; i += TB) {
                const double x = akw[i];
                for (int v = 1; v < nv; ++v) {
                    double *cj = col(k + v);
                    cj[i] = tfma(sh.f[v], x, cj[i]);
                }
            }
        }
        __syncthreads();
    }
    // R^-1 (upper triangular), then E = R^-1 (Q^T W dPhi)[0:n] and R^-1 R^-T
    if (tid == 0) {
        bool ok = true;
        for (int i = 0; i < n; ++i) ok = ok && Rm[i][i] != 0.0 && is_finite(Rm[i][i]);
        for (int i = 0; i < NMAX; ++i)
            for (int j = 0; j < NMAX; ++j) Ri[i][j] = 0.0;
        if (ok)
            for (int j = 0; j < n; ++j)
                for (int i = j; i >= 0; --i) {
                    double acc = (i == j) ? 1.0 : 0.0;
                    for (int l = i + 1; l <= j; ++l) acc = tfma(-Rm[i][l], Ri[l][j], acc);
                    Ri[i][j] = acc / Rm[i][i];
                }
        s_okr = ok ? 1 : 0;
        sm[OFF_OKR] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < NMAX * NMAX; e += TB) sm[OFF_RI + e] = Ri[e / NMAX][e % NMAX];
    for (int e = tid; e < n * P; e += TB) {
        const int r = e / P, p = e - r * P;
        double acc = 0.0;
        for (int l = r; l < n; ++l) acc = tfma(Ri[r][l], col(n + p)[l], acc);
        E[r][p] = acc;
        sm[OFF_E + r * PMAX + p] = acc;
    }
    for (int e = tid; e < n * n; e += TB) {
        const int r = e / n, c = e - r * n;
        double acc = 0.0;
        for (int l = (r > c ? r : c); l < n; ++l) acc = tfma(Ri[r][l], Ri[c][l], acc);
        sm[OFF_RR + r * NMAX + c] = acc;
    }
    // G^T G over the rows >= n of Q^T W dPhi (= Q_2^T W dPhi), in rounds of at most MAXV values
    {
        const int npp = n_tri(P);
        for (int v0 = 0; v0 < npp; v0 += gen::MAXV) {
            const int cnt = npp - v0 < gen::MAXV ? npp - v0 : gen::MAXV;
            for (int v = 0; v < cnt; ++v) {
                int p = 0, rem = v0 + v;
                while (rem >= P - p) {
                    rem -= P - p;
                    ++p;
                }
                const int pq = p + rem;
                const double *x = col(n + p), *y = col(n + pq);
                double acc = 0.0;
                for (int i = n + tid; i < m; i += TB) acc = tfma(x[i], y[i], acc);
                gen::reduce_put(sh, v, acc);
            }
            gen::reduce_finish(sh, cnt);
            if (tid < cnt) {
                int p = 0, rem = v0 + tid;
                while (rem >= P - p) {
                    rem -= P - p;
                    ++p;
                }
                const int pq = p + rem;
                sm[OFF_GG + p * PMAX + pq] = sh.red[tid];
                sm[OFF_GG + pq * PMAX + p] = sh.red[tid];
            }
        }
    }
    __syncthreads();
    // per row (band only): leverage ||R^-T phi_i^T||^2 -> column 0, F_p = dPhi_p - Phi E[:,p] -> column n + p
    if (a.ws_rows) {
        for (int i = tid; i < m; i += TB) {
            const bool in = i < rows;
            double lev = 0.0;
            for (int c = 0; c < n; ++c) {
                double v = 0.0;
                for (int r = 0; r <= c; ++r) v = tfma(Ri[r][c], in ? (double)ph[(int64_t)r * rows + i] : 0.0, v);
                lev = tfma(v, v, lev);
            }
            for (int p = 0; p < P; ++p) {
                double f = (in && dp) ? (double)dp[(int64_t)p * rows + i] : 0.0;
                for (int r = 0; r < n; ++r) f = tfma(-(in ? (double)ph[(int64_t)r * rows + i] : 0.0), E[r][p], f);
                col(n + p)[i] = f;
            }
            col(0)[i] = s_okr ? lev : 0.0;
        }
    }
}

template <typename T> __global__ void __launch_bounds__(TB) gstats_reduce_kernel(const GsArgs<T> a) {
    __shared__ double part[NNMAX][TB / 64], A[NMAX][NMAX], Cov[QMAX][QMAX];
    __shared__ double M[QMAX][QMAX], L[QMAX][QMAX], Li[QMAX][QMAX]; // (thread 0's work arrays: LDS, not scratch)
    __shared__ double s_sig2;
    __shared__ int s_ok;
    const int tid = (int)threadIdx.x, n = a.n, q = a.q, P = a.P, m = a.m, S = a.S;
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;
    double *sm = a.ws_small + b * (int64_t)kGsSmall;
    // A = sum_s c_s c_s^T: right-hand side s to thread s mod TB, then the wave sums and the TB / 64 wave totals in a fixed
    // order -- bit-deterministic
    {
        double acc[NNMAX];
#pragma unroll
        for (int t = 0; t < NNMAX; ++t) acc[t] = 0.0;
        const T *Cb = a.C + b * (int64_t)S * n;
        for (int s = tid; s < S; s += TB) {
            double c[NMAX];
#pragma unroll
            for (int j = 0; j < NMAX; ++j) c[j] = j < n ? (double)Cb[(int64_t)s * n + j] : 0.0;
#pragma unroll
            for (int j = 0, t = 0; j < NMAX; ++j)
#pragma unroll
                for (int jp = j; jp < NMAX; ++jp, ++t) acc[t] = tfma(c[j], c[jp], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < NNMAX; ++t) {
            const double v = wave_sum(acc[t]);
            if ((tid & 63) == 0) part[t][tid >> 6] = v;
        }
        __syncthreads();
        if (tid < NNMAX) {
            int j = 0, rem = tid;
            while (rem >= NMAX - j) {
                rem -= NMAX - j;
                ++j;
            }
            const int jp = j + rem;
            double v = part[tid][0];
            for (int wv = 1; wv < TB / 64; ++wv) v += part[tid][wv];
            A[j][jp] = v;
            A[jp][j] = v;
        }
        __syncthreads();
    }
    // M (Schur complement of H^T H), Cholesky in double, Cov_aa = sigma^2 M^-1
    if (tid == 0) {
        for (int k = 0; k < q; ++k)
            for (int l = 0; l < q; ++l) M[k][l] = 0.0;
        for (int p = 0; p < P; ++p)
            for (int pq = 0; pq < P; ++pq)
                M[a.pp[p]][a.pp[pq]] = tfma(sm[OFF_GG + p * PMAX + pq], A[a.pb[p]][a.pb[pq]], M[a.pp[p]][a.pp[pq]]);
        bool ok = true;
        for (int j = 0; j < q; ++j) {
            double d = M[j][j];
            for (int l = 0; l < j; ++l) d = tfma(-L[j][l], L[j][l], d);
            ok = ok && d > 0.0 && is_finite(d);
            const double ljj = ok ? tsqrt(d) : 1.0;
            L[j][j] = ljj;
            for (int i = j + 1; i < q; ++i) {
                double v = M[i][j];
                for (int l = 0; l < j; ++l) v = tfma(-L[i][l], L[j][l], v);
                L[i][j] = v / ljj;
            }
        }
        // L^-1 (lower), M^-1 = L^-T L^-1
        for (int j = 0; j < q; ++j)
            for (int i = 0; i < q; ++i) {
                if (i < j) {
                    Li[i][j] = 0.0;
                    continue;
                }
                double acc = (i == j) ? 1.0 : 0.0;
                for (int l = j; l < i; ++l) acc = tfma(-L[i][l], Li[l][j], acc);
                Li[i][j] = acc / L[i][i];
            }
        const int64_t dof = a.m_dof * (int64_t)S - (int64_t)n * S - q;
        ok = ok && dof > 0 && a.status_in[b] == VP_ST_OK && sm[OFF_OKR] != 0.0;
        const double nanv = 0.0 / 0.0;
        const double sig2 = ok ? 2.0 * a.cost[b] / (double)dof : nanv;
        for (int k = 0; k < QMAX; ++k)
            for (int l = 0; l < QMAX; ++l) {
                double v = 0.0;
                if (k < q && l < q)
                    for (int i = (k > l ? k : l); i < q; ++i) v = tfma(Li[i][k], Li[i][l], v);
                v = (k < q && l < q) ? (ok ? sig2 * v : nanv) : 0.0;
                Cov[k][l] = v;
                sm[OFF_COV + k * QMAX + l] = v;
                if (k < q && l < q) a.cov_alpha[b * q * q + k * q + l] = (T)v;
            }
        sm[OFF_SIG2] = sig2;
        sm[OFF_OK] = ok ? 1.0 : 0.0;
        a.chi2[b] = sig2;
        a.status_out[b] = ok ? VP_ST_OK : VP_ST_GSTATS_FAILED;
        s_sig2 = sig2;
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    // the band's row constants: L_i = sigma^2 lev_i, N_i[j][j'] (j < j' counted twice: c^T N c sums the upper triangle)
    if (a.ws_rows) {
        const double *ws = a.ws_cols + b * (int64_t)(n + P) * m;
        double *wr = a.ws_rows + b * (int64_t)(1 + n_tri(n)) * m;
        const double sig2 = s_sig2;
        const bool ok = s_ok != 0;
        for (int i = tid; i < m; i += TB) {
            wr[i] = ok ? sig2 * ws[i] : 0.0 / 0.0;
            for (int j = 0; j < n; ++j)
                for (int jp = j; jp < n; ++jp) {
                    double v = 0.0;
                    for (int p = 0; p < P; ++p) {
                        if (a.pb[p] != j) continue;
                        const double fp = ws[(int64_t)(n + p) * m + i];
                        double u = 0.0;
                        for (int pq = 0; pq < P; ++pq)
                            if (a.pb[pq] == jp) u = tfma(ws[(int64_t)(n + pq) * m + i], Cov[a.pp[p]][a.pp[pq]], u);
                        v = tfma(fp, u, v);
                    }
                    wr[(int64_t)tri_col(j, jp, n) * m + i] = (j == jp) ? v : 2.0 * v;
                }
        }
    }
}

// band_{s,i} = sqrt(L_i + c_s^T N_i c_s): one row per lane, the chunk's right-hand sides in a loop
template <typename T> __global__ void __launch_bounds__(TB) gstats_band_kernel(const GsArgs<T> a) {
    const int64_t bx = blockIdx.x;
    const int64_t b = bx / a.nchunk;
    const int ch = (int)(bx - b * a.nchunk);
    const int n = a.n, m = a.m, S = a.S;
    const int i = (int)blockIdx.y * TB + (int)threadIdx.x;
    const bool in = i < m;
    const int ic = in ? i : 0;
    const double *wr = a.ws_rows + b * (int64_t)(1 + n_tri(n)) * m;
    const double L = wr[ic];
    double N[NNMAX];
#pragma unroll
    for (int j = 0, t = 0; j < NMAX; ++j)
#pragma unroll
        for (int jp = j; jp < NMAX; ++jp, ++t) N[t] = jp < n ? wr[(int64_t)tri_col(j, jp, n) * m + ic] : 0.0;
    const int s0 = ch * kBandChunk, s1 = (s0 + kBandChunk < S) ? s0 + kBandChunk : S;
    // the chunk's coefficients staged in LDS once (one coalesced load): the loop below then waits on no memory load
    __shared__ double sc[kBandChunk][NMAX];
    const T *Cb = a.C + (b * (int64_t)S + s0) * n;
    for (int e = (int)threadIdx.x; e < (s1 - s0) * n; e += TB) sc[e / n][e % n] = (double)Cb[e];
    __syncthreads();
    T *out = a.band + b * (int64_t)S * m;
#pragma unroll 2
    for (int s = s0; s < s1; ++s) {
        double c[NMAX];
#pragma unroll
        for (int j = 0; j < NMAX; ++j) c[j] = j < n ? sc[s - s0][j] : 0.0;
        double v = L;
#pragma unroll
        for (int j = 0, t = 0; j < NMAX; ++j) {
            if (j >= n) break;
            double inner = 0.0;
#pragma unroll
            for (int jp = j; jp < NMAX; ++jp, ++t)
                if (jp < n) inner = tfma(N[t], c[jp], inner);
            v = tfma(c[j], inner, v);
        }
        if (in) __builtin_nontemporal_store((T)tsqrt(v), out + (int64_t)s * m + i);
    }
}

// Cov(c_s, alpha) = -K_s Cov_aa and Cov(c_s, c_s) = sigma^2 R^-1 R^-T + K_s Cov_aa K_s^T; lane (s, a) owns row a of both
template <typename T> __global__ void __launch_bounds__(TB) gstats_blocks_kernel(const GsArgs<T> a) {
    __shared__ double E[NMAX][PMAX], Cov[QMAX][QMAX], RR[NMAX][NMAX], Ksh[kBlockRhs][NMAX][QMAX];
    __shared__ double s_sig2;
    __shared__ int s_ok;
    const int tid = (int)threadIdx.x, n = a.n, q = a.q, P = a.P, S = a.S;
    const int nblk = (S + kBlockRhs - 1) / kBlockRhs;
    const int64_t b = blockIdx.x / nblk;
    const int sblk = (int)(blockIdx.x - b * nblk);
    const double *sm = a.ws_small + b * (int64_t)kGsSmall;
    for (int e = tid; e < NMAX * PMAX; e += TB) E[e / PMAX][e % PMAX] = sm[OFF_E + e];
    for (int e = tid; e < QMAX * QMAX; e += TB) Cov[e / QMAX][e % QMAX] = sm[OFF_COV + e];
    for (int e = tid; e < NMAX * NMAX; e += TB) RR[e / NMAX][e % NMAX] = sm[OFF_RR + e];
    if (tid == 0) {
        s_sig2 = sm[OFF_SIG2];
        s_ok = sm[OFF_OK] != 0.0 ? 1 : 0;
    }
    __syncthreads();
    const int sl = tid / NMAX, r = tid - sl * NMAX;
    const int s = sblk * kBlockRhs + sl;
    const bool live = r < n && s < S;
    const T *cs = a.C + (b * (int64_t)S + (live ? s : 0)) * n;
    double K[QMAX];
#pragma unroll
    for (int l = 0; l < QMAX; ++l) K[l] = 0.0;
    if (live)
        for (int p = 0; p < P; ++p) {
            const double v = (double)cs[a.pb[p]] * E[r][p];
            const int k = a.pp[p];
#pragma unroll
            for (int l = 0; l < QMAX; ++l) K[l] += (k == l) ? v : 0.0;
        }
#pragma unroll
    for (int l = 0; l < QMAX; ++l) Ksh[sl][r][l] = K[l];
    __syncthreads();
    if (!live) return;
    const double nanv = 0.0 / 0.0;
    const bool ok = s_ok != 0;
    double X[QMAX];
#pragma unroll
    for (int l = 0; l < QMAX; ++l) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < QMAX; ++k) acc = tfma(K[k], Cov[k][l], acc);
        X[l] = acc;
    }
    const int64_t row = (b * (int64_t)S + s) * n + r;
    if (a.coef_alpha_cov) {
#pragma unroll
        for (int l = 0; l < QMAX; ++l)
            if (l < q) a.coef_alpha_cov[row * q + l] = (T)(ok ? -X[l] : nanv);
    }
    if (a.coef_cov) {
        for (int c = 0; c < n; ++c) {
            double v = s_sig2 * RR[r][c];
#pragma unroll
            for (int l = 0; l < QMAX; ++l) v = tfma(X[l], Ksh[sl][c][l], v);
            a.coef_cov[row * n + c] = (T)(ok ? v : nanv);
        }
    }
}

template <typename T> int launch_gstats(const GStatsParams &p) {
    GsArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.n = p.n;
    a.q = p.q;
    a.P = p.P;
    a.m = p.m;
    a.rows = p.rows;
    a.S = p.S;
    for (int i = 0; i < p.P; ++i) {
        a.pb[i] = p.pb[i];
        a.pp[i] = p.pp[i];
    }
    a.B = p.B;
    a.m_dof = p.m_dof;
    a.w_stride = p.w_stride;
    a.nchunk = (p.S + kBandChunk - 1) / kBandChunk;
    a.phi = (const T *)p.phi;
    a.dphi = (const T *)p.dphi;
    a.w = (const T *)p.w;
    a.C = (const T *)p.C;
    a.cost = p.cost;
    a.status_in = p.status_in;
    a.ws_cols = p.ws_cols;
    a.ws_small = p.ws_small;
    a.ws_rows = p.band ? p.ws_rows : nullptr;
    a.cov_alpha = (T *)p.cov_alpha;
    a.chi2 = p.chi2;
    a.coef_cov = (T *)p.coef_cov;
    a.coef_alpha_cov = (T *)p.coef_alpha_cov;
    a.band = (T *)p.band;
    a.status_out = p.status_out;
    if (a.B <= 0) return VP_ERR_OK;
    if (a.n < 1 || a.n > NMAX || a.q < 0 || a.q > QMAX || a.P < 0 || a.P > PMAX || a.B > 0x7fffffff) return VP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((gstats_prep_kernel<T>), dim3((unsigned)a.B), dim3(TB), 0, p.stream, a);
    hipLaunchKernelGGL((gstats_reduce_kernel<T>), dim3((unsigned)a.B), dim3(TB), 0, p.stream, a);
    if (a.band) {
        const int64_t gx = a.B * (int64_t)a.nchunk;
        if (gx > 0x7fffffff) return VP_ERR_UNSUPPORTED;
        hipLaunchKernelGGL((gstats_band_kernel<T>), dim3((unsigned)gx, (unsigned)((a.m + TB - 1) / TB)), dim3(TB), 0, p.stream, a);
    }
    if (a.coef_cov || a.coef_alpha_cov) {
        const int64_t gx = a.B * (int64_t)((a.S + kBlockRhs - 1) / kBlockRhs);
        if (gx > 0x7fffffff) return VP_ERR_UNSUPPORTED;
        hipLaunchKernelGGL((gstats_blocks_kernel<T>), dim3((unsigned)gx), dim3(TB), 0, p.stream, a);
    }
    return launch_status();
}

} // namespace gs
} // namespace vp
