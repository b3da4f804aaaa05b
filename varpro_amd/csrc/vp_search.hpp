// vp_search.hpp -- the kernels of vp_search: rank K candidate parameter vectors per problem by the projected objective
// 1/2 ||P_perp(alpha) y_w||^2 and leave the best one of every problem in the handle.
//
// SHARED ROUTE (candidates, grid and weights shared by the batch).  The objective depends on a candidate only through
// range(W Phi(alpha_k)), so the K factorisations are made once and a problem's work is a projection onto K small
// orthonormal bases:
//   (a) cols_fill (vp_cols.hpp) evaluates Phi of the K candidates as if they were K problems            [K][n][m]
//   (b) orthonormalize_kernel: one workgroup per candidate weights its n columns and orthonormalises them by modified
//       Gram-Schmidt applied twice.  A direction whose remainder is <= 64 eps times the column's norm is dropped (zeros):
//       the score is then that of the reduced basis == the cost of the minimum-norm solution.  A candidate with a
//       non-finite column is marked and scores -inf.
//   (c) rank_kernel: s(b,k) = sum_s sum_j (q_kj . y_w,b,s)^2 -- ONE matrix product (B S x m)(m x K n) whose epilogue
//       squares and adds; the cost is 1/2 (||y_w||^2 - s), so the best candidate has the LARGEST score.
//   (d) the ordinary evaluation at the winners (vp_api.hip).
//
// Layout of Q: candidates in groups of 16, basis-major inside a group -- column ((g n + j) 16 + c) is basis j of candidate
// 16 g + c -- each column ldq = ceil16(m) long, zero beyond m; K is padded to a multiple of 16 with zero columns that are
// marked like non-finite candidates.  A 16-wide output tile of the product is then basis j of 16 candidates, and a
// candidate's score is the ELEMENT-WISE sum of squares over the n accumulator tiles of its group: no cross-lane work and
// no dependence on the accumulator's lane map other than which (row, column) an element is.
//
// rank_kernel is an MFMA kernel (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32).  On gfx950 the fp64 matrix rate equals
// the fp64 vector rate, so MFMA buys no flops; it buys ISSUE slots and register bandwidth: one instruction is 1 024 FMAs
// fed by two operand registers, where a register-tiled VALU kernel issues 16 v_fma_f64 per lane for the same work and
// needs its operands broadcast across lanes first (Y rows and Q columns are both contiguous in k, the reduction index).
// Both operands of the 16x16x4 form hold ONE element per lane, element (row|col = lane & 15, k = lane >> 4); a sum over k
// does not care in which order k is visited, so lane (r, h) loads the four CONSECUTIVE elements k0 + 4 h .. k0 + 4 h + 3 of
// its row (32 bytes, one 128-byte line per row and 16-row chunk) and feeds element e to the e-th of four MFMAs -- A and B
// permute k alike.  A wavefront owns RT x 16 rows of Y_w (problems) and walks over candidate groups; the four wavefronts
// of a workgroup take groups g = wave, wave + 4, ... of the SAME rows, so Y_w is fetched from memory once per four groups
// (the other three hit the cache) and a workgroup ends with the winners of its rows: no atomics, no score matrix.
// Ties go to the lowest candidate index.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/varpro_hip.h"
#include "vp_kernels.hpp" // launch_status()

namespace vp {

// type-erased launch record of the shared route (host side); every pointer is a device pointer
struct SearchParams {
    int dtype;
    int n;            // basis functions
    int K, Kpad;      // candidates, rounded up to a multiple of 16
    int m, ldq;       // rows, ceil16(m)
    int64_t B;
    int S;
    const void *phi;  // [K][n][m] unweighted columns of the candidates
    const void *w;    // [m] shared weights or null
    void *Q;          // [Kpad/16][n][16][ldq], zero-filled by the caller
    int32_t *bad;     // [Kpad], filled with 1 by the caller; (b) clears the finite candidates
    const void *yw;   // [B][S][m]
    void *scores;     // S > 1: [B S][Kpad] of the handle's dtype
    int32_t *index;   // [B] winners, -1: no finite candidate
    hipStream_t stream;
};
int search_orthonormalize(const SearchParams &p);
int search_rank(const SearchParams &p);
// d_alpha[b] = cand[b or 0][k]  (k >= 0: that candidate for every problem; k < 0: candidate max(index[b], 0))
int search_gather(int dtype, const void *cand, int64_t K, int q, int per_problem, int64_t k, const int32_t *index, int64_t B,
                  void *alpha, hipStream_t stream);
// candidate loop: the running minimum after the cost-only evaluation of candidate k (k == 0 initialises)
int search_loop_update(const double *cost, const int32_t *status, int64_t k, int64_t B, double *best, int32_t *index,
                       hipStream_t stream);

namespace search {

template <typename T> struct Eps;
template <> struct Eps<double> {
    static constexpr double value = 2.220446049250313e-16;
};
template <> struct Eps<float> {
    static constexpr float value = 1.1920928955078125e-07f;
};
__device__ __forceinline__ double ssqrt(const double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float ssqrt(const float x) { return __builtin_sqrtf(x); }
template <typename T> __device__ __forceinline__ bool finite(const T x) { return x - x == T(0); }

// sum over the 256 threads of a workgroup, the same bits in every thread (xor butterflies add commutatively)
template <typename T> __device__ __forceinline__ T block_sum(T v, T *sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ... and the maximum (of values that are not NaN)
template <typename T> __device__ __forceinline__ T block_max(T v, T *sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const T a = sh[0] > sh[1] ? sh[0] : sh[1], b = sh[2] > sh[3] ? sh[2] : sh[3];
    return a > b ? a : b;
}

// (b) one workgroup of 256 threads per candidate.  A thread owns rows tid, tid + 256, ... of every column: the only
// traffic between threads is the sums.
template <typename T>
__global__ void __launch_bounds__(256) orthonormalize_kernel(const T *__restrict__ phi, const T *__restrict__ w, T *__restrict__ Q,
                                                             int32_t *__restrict__ bad, const int n, const int m, const int ldq) {
    __shared__ T sh[4];
    const int k = (int)blockIdx.x, g = k >> 4, c = k & 15;
    const int tid = (int)threadIdx.x;
    T *const q0 = Q + ((int64_t)g * n * 16 + c) * ldq; // column j: q0 + j * 16 * ldq
    const int64_t cs = (int64_t)16 * ldq;
    unsigned kept = 0; // bit l: direction l is in the basis
    bool ok = true;
    for (int j = 0; j < n && ok; ++j) {
        const T *pj = phi + ((int64_t)k * n + j) * m;
        T *qj = q0 + j * cs;
        // the column's largest magnitude (inf for a NaN or an infinity): the ELEMENTS decide whether the column is finite,
        // and the column is scaled by it before anything is squared -- a finite column never overflows into "not finite"
        T amax = T(0);
        for (int i = tid; i < m; i += 256) {
            const T v = w ? w[i] * pj[i] : pj[i];
            const T a = finite(v) ? (v < T(0) ? -v : v) : T(__builtin_inff());
            amax = a > amax ? a : amax;
        }
        amax = block_max(amax, sh);
        if (!finite(amax)) {
            ok = false;
            break;
        }
        const T inv = amax > T(0) ? T(1) / amax : T(0);
        T ss = T(0);
        for (int i = tid; i < m; i += 256) {
            const T v = (w ? w[i] * pj[i] : pj[i]) * inv;
            qj[i] = v;
            ss += v * v;
        }
        const T norm0 = ssqrt(block_sum(ss, sh));
        for (int pass = 0; pass < 2; ++pass)
            for (int l = 0; l < j; ++l) {
                if (!((kept >> l) & 1u)) continue;
                const T *ql = q0 + l * cs;
                T d = T(0);
                for (int i = tid; i < m; i += 256) d += ql[i] * qj[i];
                d = block_sum(d, sh);
                for (int i = tid; i < m; i += 256) qj[i] -= d * ql[i];
            }
        T rr = T(0);
        for (int i = tid; i < m; i += 256) rr += qj[i] * qj[i];
        const T rem = ssqrt(block_sum(rr, sh));
        const bool keep = rem > T(64) * Eps<T>::value * norm0; // (false for a zero column)
        if (keep) kept |= 1u << j;
        const T scale = keep ? T(1) / rem : T(0);
        for (int i = tid; i < m; i += 256) qj[i] = keep ? qj[i] * scale : T(0);
    }
    if (!ok) // a non-finite column: the candidate's columns are cleared and it stays marked
        for (int j = 0; j < n; ++j)
            for (int i = tid; i < m; i += 256) q0[j * cs + i] = T(0);
    if (tid == 0) bad[k] = ok ? 0 : 1;
}

// ---- (c) ------------------------------------------------------------------------------------------------------------
template <typename T> struct Mfma;
template <> struct Mfma<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mac(const double a, const double b, const acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // accumulator element `reg` of lane group h = lane >> 4 is row h + 4 reg (column lane & 15)
    static __device__ __forceinline__ int row(const int h, const int reg) { return h + 4 * reg; }
};
template <> struct Mfma<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mac(const float a, const float b, const acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // ... and here row 4 h + reg
    static __device__ __forceinline__ int row(const int h, const int reg) { return 4 * h + reg; }
};

// four consecutive elements of a row: 16-byte vectors where the row is known to be 16-byte aligned
template <typename T, bool VEC> __device__ __forceinline__ void load4(const T *__restrict__ p, T (&v)[4]) {
    if constexpr (VEC) {
        constexpr int VW = 16 / (int)sizeof(T);
        typedef T vec_t __attribute__((ext_vector_type(VW)));
#pragma unroll
        for (int e = 0; e < 4; e += VW) {
            const vec_t x = *reinterpret_cast<const vec_t *>(p + e);
#pragma unroll
            for (int f = 0; f < VW; ++f) v[e + f] = x[f];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p[e];
    }
}

template <typename T> struct RankArgs {
    const T *yw;     // [rows][m]
    const T *Q;      // [G][n][16][ldq]
    const int32_t *bad;
    T *scores;       // SCORES: [rows][Kpad]
    int32_t *index;  // !SCORES: [rows]
    int64_t rows;
    int m, ldq, G;
};

// the better of two (score, candidate) pairs: the larger score, at equal scores the lower index
template <typename T> __device__ __forceinline__ void take_better(T &s, int &i, const T so, const int io) {
    if (so > s || (so == s && io < i)) {
        s = so;
        i = io;
    }
}

// N basis functions, RT row tiles of 16 rows per wavefront; VEC: rows of Y_w are 16-byte aligned; SCORES: write the scores
// of every (row, candidate) instead of the winner (S > 1: the sum over the right-hand sides comes first)
template <typename T, int N, int RT, bool VEC, bool SCORES>
__global__ void __launch_bounds__(256) rank_kernel(const RankArgs<T> a) {
    typedef typename Mfma<T>::acc_t acc_t;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int r = lane & 15, h = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * (RT * 16);
    const int m = a.m;
    const T *arow[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        int64_t row = row0 + rt * 16 + r;
        if (row >= a.rows) row = a.rows - 1; // (loaded, never stored)
        arow[rt] = a.yw + row * m + 4 * h;
    }
    const T ninf = -__builtin_inff();
    T best[RT][4];
    int bidx[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            best[rt][e] = ninf;
            bidx[rt][e] = -1;
        }
    const int mfull = m & ~15;
    for (int g = wave; g < a.G; g += 4) {
        const T *brow = a.Q + ((int64_t)g * N * 16 + r) * a.ldq + 4 * h; // basis j: + j * 16 * ldq
        const int64_t bs = (int64_t)16 * a.ldq;
        acc_t acc[RT][N];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int j = 0; j < N; ++j) acc[rt][j] = acc_t{T(0), T(0), T(0), T(0)};
        T av[RT][4], bv[N][4];
        if (mfull > 0) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) load4<T, VEC>(arow[rt], av[rt]);
#pragma unroll
            for (int j = 0; j < N; ++j) load4<T, true>(brow + j * bs, bv[j]);
        }
        for (int k0 = 0; k0 < mfull; k0 += 16) {
            // the next chunk's operands are on their way while this chunk's MFMAs run
            T an[RT][4], bn[N][4];
            const int k1 = k0 + 16 < mfull ? k0 + 16 : k0;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) load4<T, VEC>(arow[rt] + k1, an[rt]);
#pragma unroll
            for (int j = 0; j < N; ++j) load4<T, true>(brow + j * bs + k1, bn[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int j = 0; j < N; ++j) acc[rt][j] = Mfma<T>::mac(av[rt][e], bv[j][e], acc[rt][j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) av[rt][e] = an[rt][e];
#pragma unroll
                for (int j = 0; j < N; ++j) bv[j][e] = bn[j][e];
            }
        }
        if (mfull < m) { // the last, partial chunk: Y_w is masked beyond its row, Q is zero there
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int e = 0; e < 4; ++e) av[rt][e] = mfull + 4 * h + e < m ? arow[rt][mfull + e] : T(0);
#pragma unroll
            for (int j = 0; j < N; ++j) load4<T, true>(brow + j * bs + mfull, bv[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int j = 0; j < N; ++j) acc[rt][j] = Mfma<T>::mac(av[rt][e], bv[j][e], acc[rt][j]);
        }
        // this lane's column of the tiles is candidate 16 g + r
        const int cand = g * 16 + r;
        const bool isbad = a.bad[cand] != 0;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                T s = T(0);
#pragma unroll
                for (int j = 0; j < N; ++j) s = __builtin_fma(acc[rt][j][e], acc[rt][j][e], s);
                if (isbad) s = ninf;
                if constexpr (SCORES) {
                    const int64_t row = row0 + rt * 16 + Mfma<T>::row(h, e);
                    if (row < a.rows) a.scores[row * ((int64_t)a.G * 16) + cand] = s;
                } else {
                    if (s > best[rt][e]) { // (groups ascend: the first of equal scores stays)
                        best[rt][e] = s;
                        bidx[rt][e] = cand;
                    }
                }
            }
    }
    if constexpr (!SCORES) {
        __shared__ T sh_s[4][RT * 16];
        __shared__ int sh_i[4][RT * 16];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                T s = best[rt][e];
                int i = bidx[rt][e];
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) { // over the 16 candidates of the lanes that share h
                    const T so = __shfl_xor(s, off);
                    const int io = __shfl_xor(i, off);
                    take_better(s, i, so, io);
                }
                if (r == 0) {
                    sh_s[wave][rt * 16 + Mfma<T>::row(h, e)] = s;
                    sh_i[wave][rt * 16 + Mfma<T>::row(h, e)] = i;
                }
            }
        __syncthreads();
        const int t = (int)threadIdx.x;
        if (t < RT * 16 && row0 + t < a.rows) {
            T s = sh_s[0][t];
            int i = sh_i[0][t];
#pragma unroll
            for (int wv = 1; wv < 4; ++wv) take_better(s, i, sh_s[wv][t], sh_i[wv][t]);
            a.index[row0 + t] = i;
        }
    }
}

// S > 1: s(b,k) = sum_s scores[b S + s][k] in the handle's dtype, then the winner; one workgroup per problem
template <typename T>
__global__ void __launch_bounds__(256) reduce_scores_kernel(const T *__restrict__ scores, const int S, const int K, const int Kpad,
                                                            int32_t *__restrict__ index) {
    __shared__ T sh_s[256];
    __shared__ int sh_i[256];
    const int64_t b = blockIdx.x;
    const int tid = (int)threadIdx.x;
    T best = -__builtin_inff();
    int bi = -1;
    for (int k = tid; k < K; k += 256) {
        T s = T(0);
        for (int rhs = 0; rhs < S; ++rhs) s += scores[(b * S + rhs) * Kpad + k];
        if (s > best) {
            best = s;
            bi = k;
        }
    }
    sh_s[tid] = best;
    sh_i[tid] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) take_better(sh_s[tid], sh_i[tid], sh_s[tid + off], sh_i[tid + off]);
        __syncthreads();
    }
    if (tid == 0) index[b] = sh_i[0];
}

// ---- the small kernels both routes share ------------------------------------------------------------------------------
// alpha[b][:] = cand[b (per problem) or 0][k][:] ; k < 0: the winner index[b], candidate 0 where there is none
template <typename T>
__global__ void __launch_bounds__(256) gather_kernel(const T *__restrict__ cand, const int64_t K, const int q, const int per_problem,
                                                     const int64_t k, const int32_t *__restrict__ index, const int64_t total,
                                                     T *__restrict__ alpha) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / q;
    const int c = (int)(i - b * q);
    int64_t kk = k;
    if (kk < 0) {
        kk = index[b];
        if (kk < 0) kk = 0;
    }
    alpha[i] = cand[((per_problem ? b * K : 0) + kk) * q + c];
}

template <typename T, int N, bool VEC, bool SCORES> int launch_rank_n(const RankArgs<T> &a, hipStream_t stream) {
    constexpr int RT = N <= 4 ? 4 : 2;
    const int64_t blocks = (a.rows + RT * 16 - 1) / (RT * 16);
    if (blocks > 0x7fffffff) return VP_ERR_INVALID;
    hipLaunchKernelGGL((rank_kernel<T, N, RT, VEC, SCORES>), dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return launch_status();
}
template <typename T, bool VEC, bool SCORES> int launch_rank_v(const int n, const RankArgs<T> &a, hipStream_t stream) {
    switch (n) {
    case 1: return launch_rank_n<T, 1, VEC, SCORES>(a, stream);
    case 2: return launch_rank_n<T, 2, VEC, SCORES>(a, stream);
    case 3: return launch_rank_n<T, 3, VEC, SCORES>(a, stream);
    case 4: return launch_rank_n<T, 4, VEC, SCORES>(a, stream);
    case 5: return launch_rank_n<T, 5, VEC, SCORES>(a, stream);
    case 6: return launch_rank_n<T, 6, VEC, SCORES>(a, stream);
    case 7: return launch_rank_n<T, 7, VEC, SCORES>(a, stream);
    case 8: return launch_rank_n<T, 8, VEC, SCORES>(a, stream);
    default: return VP_ERR_INVALID;
    }
}

template <typename T> int launch_rank(const SearchParams &p) {
    if (p.B <= 0 || p.K <= 0) return VP_ERR_OK;
    RankArgs<T> a;
    a.yw = (const T *)p.yw;
    a.Q = (const T *)p.Q;
    a.bad = p.bad;
    a.scores = (T *)p.scores;
    a.index = p.index;
    a.rows = p.B * p.S;
    a.m = p.m;
    a.ldq = p.ldq;
    a.G = p.Kpad / 16;
    const bool vec = (reinterpret_cast<uintptr_t>(p.yw) & 15) == 0 && ((size_t)p.m * sizeof(T)) % 16 == 0;
    int rc;
    if (p.S > 1) {
        rc = vec ? launch_rank_v<T, true, true>(p.n, a, p.stream) : launch_rank_v<T, false, true>(p.n, a, p.stream);
        if (rc != VP_ERR_OK) return rc;
        hipLaunchKernelGGL(reduce_scores_kernel<T>, dim3((unsigned)p.B), dim3(256), 0, p.stream, (const T *)p.scores, p.S, p.K,
                           p.Kpad, p.index);
        return launch_status();
    }
    return vec ? launch_rank_v<T, true, false>(p.n, a, p.stream) : launch_rank_v<T, false, false>(p.n, a, p.stream);
}

template <typename T> int launch_orthonormalize(const SearchParams &p) {
    if (p.K <= 0) return VP_ERR_OK;
    hipLaunchKernelGGL(orthonormalize_kernel<T>, dim3((unsigned)p.K), dim3(256), 0, p.stream, (const T *)p.phi, (const T *)p.w,
                       (T *)p.Q, p.bad, p.n, p.m, p.ldq);
    return launch_status();
}

template <typename T>
int launch_gather(const void *cand, int64_t K, int q, int per_problem, int64_t k, const int32_t *index, int64_t B, void *alpha,
                  hipStream_t stream) {
    const int64_t total = B * q;
    if (total <= 0) return VP_ERR_OK;
    hipLaunchKernelGGL(gather_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const T *)cand, K, q,
                       per_problem, k, index, total, (T *)alpha);
    return launch_status();
}

} // namespace search
} // namespace vp
