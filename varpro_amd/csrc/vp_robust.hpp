// vp_robust.hpp -- robust re-weighting of a single-RHS batch (vp_robust_reweight): M-estimator weights (Huber, Cauchy, Tukey)
// from the residuals of the current best fit, with the scale of the residuals estimated per problem on the device.  A fit with
// the weights w = w0 sqrt(psi(u)/u), u = w0 (y - f)/s, held fixed, repeated with the weights re-formed from its result, has
// the M-estimating equations sum_i psi(u_i) w0_i df_i/dtheta = 0 as its fixed point: the LM kernels are untouched, the
// robust fit is this kernel between their launches.
//
//   e_i = w0_i (y_i - f_i)                                  (the difference first, then the product; w0 null: 1)
//   s   = scale (fixed)   or   1.482602218505602 med,  med = 0.5 (a[(me-1)/2] + a[me/2]) of the sorted |e_i| of the me rows
//                                                      with w0_i != 0  (rows of weight 0 are how a ragged length is written)
//   u_i = |e_i| / s,  t = u/k
//   Huber   sqrt(omega) = u <= k ? 1 : sqrt(k/u)           rho = u <= k ? u^2/2 : k u - k^2/2
//   Cauchy  sqrt(omega) = sqrt(1/(1 + t t))                rho = k^2/2 log1p(t^2)
//   Tukey   sqrt(omega) = t >= 1 ? 0 : (1 - t)(1 + t)      rho = t >= 1 ? k^2/6 : k^2/6 (1 - (1 - t^2)^3)
//   w_i = w0_i sqrt(omega_i),  Y_w,i = w_i y_i;            s == 0 (more than half of the residuals are 0, or me == 0):
//                                                          w = w0, Y_w = w0 y, scale 0, rho 0
// Every comparison is written so that a NaN goes through.  A residual that is not finite gives NaN weights -- to the whole
// problem where the scale is estimated (its scale is NaN), to its row where the scale is fixed -- so that the next
// evaluation latches the problem instead of giving an infinite residual the weight 0.  Divisions and square roots are the
// compiler's full-precision ones; rho is formed from u in fp64 for both dtypes and summed in a fixed order.
//
// Work sharing is that of vp_poisson.hpp: ONE WAVEFRONT per problem, four problems per 256-thread workgroup, a lane owns a
// 16-byte group of every tile of 64 groups, element-wise where m or an alignment forbids; no atomics, no LDS, and nothing
// depends on which wave or launch runs a problem.
//
// The median is an exact selection, not a sort.  The key of a row is the bit pattern of |e_i| as an unsigned integer --
// for non-negative IEEE values unsigned order is numeric order, -0 has become +0, a denormal is just a small key -- and
// all-ones for a row that does not count (w0 = 0, or beyond m).  The order statistic of rank r is the largest v with
// #{key < v} <= r: v is built from the most significant bit down, each bit one compare per key and one popcount of the
// wave's ballot, summed on the scalar unit (63 steps in fp64, 31 in fp32: the sign bit is 0).  The second middle statistic
// (me even) equals the first if #{key <= a1} > me/2 and is otherwise the minimum of the keys above a1: one more pass.
// Where the keys fit -- m <= RES_ROWS = 1024, sixteen per lane -- they stay in registers (RES); longer problems keep them in
// their own row of w, which the same lanes overwrite with the weights afterwards (every lane reads back only what it wrote
// itself), and each step streams the row from the cache.  A problem whose status is non-zero returns before touching w.
#pragma once
#include "vp_poisson.hpp"

namespace vp {

// type-erased launch record (host side); every pointer is a device pointer
struct RobustParams {
    int dtype;
    const void *Y;          // [B][m] observations
    const void *F;          // [B][m] unweighted best fit
    const void *w0;         // [B][m] base weights or null (unit)
    const int32_t *status;  // [B]
    void *w, *yw;           // [B][m] out
    double *scale_out;      // [B] out or null
    double *rho_out;        // [B] out or null
    int loss;               // VP_ROBUST_*
    double k;               // tuning constant, > 0
    double scale;           // > 0: fixed; 0: the normalised median of |e| per problem
    int m;
    int64_t B;
    hipStream_t stream;
};
int robust_reweight_launch(const RobustParams &p);

namespace robust {

using cols::Vec;
using poisson::load_group;

constexpr int RES_ROWS = 1024; // the longest problem whose keys stay in registers

template <typename T> struct Key;
template <> struct Key<double> {
    typedef uint64_t type;
    typedef uint64_t group __attribute__((ext_vector_type(2)));
    static constexpr int BITS = 63;
    static __device__ __forceinline__ uint64_t of(double x) { return (uint64_t)__double_as_longlong(x); }
    static __device__ __forceinline__ double value(uint64_t k) { return __longlong_as_double((long long)k); }
};
template <> struct Key<float> {
    typedef uint32_t type;
    typedef uint32_t group __attribute__((ext_vector_type(4)));
    static constexpr int BITS = 31;
    static __device__ __forceinline__ uint32_t of(float x) { return __float_as_uint(x); }
    static __device__ __forceinline__ float value(uint32_t k) { return __uint_as_float(k); }
};

template <typename T> struct Args {
    const T *Y, *F, *w0;
    const int32_t *status;
    T *w, *yw;
    double *scale_out, *rho_out;
    int64_t first, end; // problems first .. end-1 belong to this launch
    T k, scale;
    int loss, m;
};

// lanes whose predicate holds, counted on the scalar unit (all 64 lanes are active wherever this is called)
__device__ __forceinline__ int wave_count(const bool p) { return __builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); }

// sqrt(omega) and rho of one row from a = |e| (s > 0, or NaN)
template <typename T> __device__ __forceinline__ void weight_term(const T a, const T s, const T k, const int loss, T &sw, double &rho) {
    const T u = a / s;
    const double ud = (double)u, kd = (double)k;
    if (loss == VP_ROBUST_HUBER) {
        sw = u <= k ? T(1) : tsqrt(k / u);
        rho = ud <= kd ? 0.5 * ud * ud : kd * ud - 0.5 * kd * kd;
    } else if (loss == VP_ROBUST_CAUCHY) {
        const T t = u / k;
        sw = tsqrt(T(1) / (T(1) + t * t));
        const double td = ud / kd;
        rho = 0.5 * kd * kd * log1p(td * td);
    } else {
        const T t = u / k;
        sw = t >= T(1) ? T(0) : (T(1) - t) * (T(1) + t);
        const double td = ud / kd, q = 1.0 - td * td;
        rho = td >= 1.0 ? kd * kd / 6.0 : kd * kd / 6.0 * (1.0 - q * q * q);
    }
    if (!is_finite(a)) { // (an infinite residual must not pass as weight 0)
        sw = T(0) / T(0);
        rho = __builtin_nan("");
    }
}

// (Y and yw carry no __restrict__: a caller may hand the same array to both, every element is read and written by one thread)
template <typename T, bool VEC, bool MAD, bool RES> __global__ void __launch_bounds__(256) robust_reweight_kernel(const Args<T> a) {
    using K = Key<T>;
    using UT = typename K::type;
    constexpr int VW = Vec<T>::VW, TILE = 64 * VW, RES_TILES = RES_ROWS / TILE;
    constexpr UT NOKEY = ~UT(0);
    const int lane = lane_id();
    const int64_t b = a.first + (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (b >= a.end) return;
    if (a.status[b] != 0) { // a failed round must not poison the next one
        const double nan = __builtin_nan("");
        if (lane == 0) {
            if (a.scale_out) a.scale_out[b] = nan;
            if (a.rho_out) a.rho_out[b] = nan;
        }
        return;
    }
    const int m = a.m, loss = a.loss;
    const T k = a.k;
    const T *y = a.Y + b * m, *f = a.F + b * m;
    const T *w0 = a.w0 ? a.w0 + b * m : nullptr;
    T *w = a.w + b * m, *yw = a.yw + b * m;
    UT *kbuf = reinterpret_cast<UT *>(w); // the streamed form's keys
    const int tiles = (m + TILE - 1) / TILE;

    // e of the group at row i, and the base weights it was formed with (rows beyond m: w0 = 0, e = 0)
    auto residuals = [&](const int i, T (&yv)[VW], T (&wv)[VW], T (&ev)[VW]) {
        T fv[VW];
        load_group<T, VEC>(y, i, m, yv);
        load_group<T, VEC>(f, i, m, fv);
        if (w0) load_group<T, VEC>(w0, i, m, wv);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            if (!w0) wv[e] = T(1);
            if (!VEC && i + e >= m) wv[e] = T(0), yv[e] = T(0), fv[e] = T(0);
            const T d = yv[e] - fv[e];
            ev[e] = wv[e] * d;
        }
    };
    auto load_keys = [&](const int i, UT (&kv)[VW]) {
        if constexpr (VEC) {
            const typename K::group v = *reinterpret_cast<const typename K::group *>(kbuf + i);
#pragma unroll
            for (int e = 0; e < VW; ++e) kv[e] = v[e];
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) kv[e] = i + e < m ? kbuf[i + e] : NOKEY;
        }
    };

    T s = a.scale;
    [[maybe_unused]] UT keys[RES ? RES_TILES : 1][VW];
    if constexpr (MAD) {
        // ---- phase 1: residuals -> keys; the rows that count; one ballot for a residual that is not finite
        int me = 0;
        bool bad = false;
        auto form_keys = [&](const int i, UT (&kv)[VW]) {
            T yv[VW], wv[VW], ev[VW];
            residuals(i, yv, wv, ev);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                bad = bad || !is_finite(ev[e]);
                kv[e] = wv[e] != T(0) ? K::of(tabs(ev[e])) : NOKEY;
            }
        };
        if constexpr (RES) {
#pragma unroll
            for (int g = 0; g < RES_TILES; ++g) {
                const int i = g * TILE + VW * lane;
                UT kv[VW];
#pragma unroll
                for (int e = 0; e < VW; ++e) kv[e] = NOKEY;
                if (g < tiles) { // (wave-uniform)
                    if (i < m) form_keys(i, kv);
#pragma unroll
                    for (int e = 0; e < VW; ++e) me += wave_count(kv[e] != NOKEY);
                }
#pragma unroll
                for (int e = 0; e < VW; ++e) keys[g][e] = kv[e];
            }
        } else {
            for (int base = 0; base < m; base += TILE) {
                const int i = base + VW * lane;
                UT kv[VW];
#pragma unroll
                for (int e = 0; e < VW; ++e) kv[e] = NOKEY;
                if (i < m) {
                    form_keys(i, kv);
                    if constexpr (VEC) {
                        typename K::group v;
#pragma unroll
                        for (int e = 0; e < VW; ++e) v[e] = kv[e];
                        *reinterpret_cast<typename K::group *>(kbuf + i) = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < VW; ++e)
                            if (i + e < m) kbuf[i + e] = kv[e];
                    }
                }
#pragma unroll
                for (int e = 0; e < VW; ++e) me += wave_count(kv[e] != NOKEY);
            }
        }
        // ---- phase 2: the two middle order statistics of the me keys
        // each(fn): fn(key) over every key of the problem, all lanes active (rows that do not count hold NOKEY)
        auto each = [&](auto &&fn) {
            if constexpr (RES) {
#pragma unroll
                for (int g = 0; g < RES_TILES; ++g)
                    if (g < tiles) {
#pragma unroll
                        for (int e = 0; e < VW; ++e) fn(keys[g][e]);
                    }
            } else {
                for (int base = 0; base < m; base += TILE) {
                    const int i = base + VW * lane;
                    UT kv[VW];
#pragma unroll
                    for (int e = 0; e < VW; ++e) kv[e] = NOKEY;
                    if (i < m) load_keys(i, kv);
#pragma unroll
                    for (int e = 0; e < VW; ++e) fn(kv[e]);
                }
            }
        };
        if (wave_count(bad) != 0) {
            s = T(0) / T(0);
        } else if (me == 0) {
            s = T(0);
        } else {
            const int r1 = (me - 1) / 2, r2 = me / 2;
            UT a1 = 0;
            for (int bit = K::BITS - 1; bit >= 0; --bit) {
                const UT trial = a1 | (UT(1) << bit);
                int below = 0;
                each([&](const UT key) { below += wave_count(key < trial); });
                if (below <= r1) a1 = trial;
            }
            UT a2 = a1;
            if (r2 != r1) {
                int upto = 0;
                UT above = NOKEY;
                each([&](const UT key) {
                    upto += wave_count(key <= a1);
                    above = key > a1 && key < above ? key : above;
                });
                if (upto <= r2) { // the next key up: the minimum over the wave (me > upto: one exists)
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const UT o = (UT)__shfl_xor((unsigned long long)above, d, 64);
                        above = o < above ? o : above;
                    }
                    a2 = above;
                }
            }
            const T med = T(0.5) * (K::value(a1) + K::value(a2));
            s = T(1.482602218505602) * med;
        }
    }

    // ---- phase 3: the weights, the weighted data, rho
    double rsum = 0.0;
    auto form_weights = [&](const int i, [[maybe_unused]] const UT (&held)[VW]) {
        T yv[VW], wv[VW], ev[VW], ov[VW], ywv[VW];
        [[maybe_unused]] UT kv[VW];
        if constexpr (MAD && !RES) load_keys(i, kv);
        if constexpr (MAD) {
            load_group<T, VEC>(y, i, m, yv);
            if (w0) load_group<T, VEC>(w0, i, m, wv);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                if (!w0) wv[e] = T(1);
                const UT key = RES ? held[e] : kv[e];
                ev[e] = key != NOKEY ? K::value(key) : T(0); // |e|; a row of weight 0 has e = 0 (or the problem is NaN already)
            }
        } else {
            residuals(i, yv, wv, ev);
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            T sw = T(1);
            double rho = 0.0;
            if (!(MAD && s == T(0))) weight_term(tabs(ev[e]), s, k, loss, sw, rho);
            ov[e] = wv[e] * sw;
            ywv[e] = ov[e] * yv[e];
            if (VEC || i + e < m) rsum += rho;
        }
        cols::store_group<T, VEC, false>(w, i, m, ov);
        cols::store_group<T, VEC, false>(yw, i, m, ywv);
    };
    if constexpr (RES) {
#pragma unroll
        for (int g = 0; g < RES_TILES; ++g) {
            const int i = g * TILE + VW * lane;
            if (g < tiles && i < m) form_weights(i, keys[g]);
        }
    } else {
        for (int base = 0; base < m; base += TILE) {
            const int i = base + VW * lane;
            if (i < m) form_weights(i, keys[0]);
        }
    }
    rsum = wave_sum(rsum);
    if (lane == 0) {
        if (a.scale_out) a.scale_out[b] = (double)s;
        if (a.rho_out) a.rho_out[b] = rsum;
    }
}

template <typename T> int launch(const RobustParams &p) {
    if (p.B <= 0 || p.m <= 0) return VP_ERR_OK;
    if (!p.Y || !p.F || !p.status || !p.w || !p.yw) return VP_ERR_INVALID;
    // 16-byte groups: m a multiple of the group (every problem's rows then start 16-byte aligned) and every array aligned
    auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool vec = p.m % Vec<T>::VW == 0 && al16(p.Y) && al16(p.F) && al16(p.w0) && al16(p.w) && al16(p.yw);
    const bool mad = p.scale == 0.0, res = p.m <= RES_ROWS;
    Args<T> a;
    a.Y = (const T *)p.Y;
    a.F = (const T *)p.F;
    a.w0 = (const T *)p.w0;
    a.status = p.status;
    a.w = (T *)p.w;
    a.yw = (T *)p.yw;
    a.scale_out = p.scale_out;
    a.rho_out = p.rho_out;
    a.k = (T)p.k;
    a.scale = (T)p.scale;
    a.loss = p.loss;
    a.m = p.m;
    // (4 problems per workgroup)
    return cols::launch_chunks(p.B, (int64_t)0x7fffffff, [&](const int64_t first, const int64_t nb) {
        a.first = first;
        a.end = first + nb;
        const dim3 grid((unsigned)((nb + 3) / 4)), block(256);
        cols::select_variant(
            [&](auto V, auto M, auto R) {
                // (a fixed scale has no keys to hold: one kernel for every length)
                constexpr bool RESIDENT = M.value && R.value;
                if constexpr (M.value || !R.value)
                    hipLaunchKernelGGL((robust_reweight_kernel<T, V.value, M.value, RESIDENT>), grid, block, 0, p.stream, a);
            },
            vec, mad, mad ? res : false);
    });
}

} // namespace robust
} // namespace vp
