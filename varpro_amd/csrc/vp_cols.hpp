// vp_cols.hpp -- the column kernel of DEVICE-COLUMN handles: descriptors that contain VP_BASIS_GAUSS / VP_BASIS_LORENTZ /
// VP_BASIS_LINEAR.  One kernel family evaluates the UNWEIGHTED basis matrix Phi [B][n][m] and the derivative columns dPhi
// [B][p][m] (pairs in model order, basis-major: vp_basis' layout) of a run-time descriptor into device memory; everything
// downstream of the columns is done by the caller-evaluated kernels (vp_ext.hpp, vp_blk_ext.hpp, vp_extfit.hpp, ...) exactly
// as for a caller's columns.  All eight device kinds are evaluated here, so a descriptor may mix a Gaussian with an
// exponential tail and a baseline.
// (The IRF reconvolution kinds are not pointwise functions of t: their columns come from the scan kernel of vp_irf.hpp,
// launched behind this one by cols_fill; launch_fill below keeps them out of the descriptor this kernel sees.)
//
// Work sharing: a THREAD owns one 16-byte row group (2 fp64 / 4 fp32 rows) of one problem and walks over ALL basis functions
// there: the exponential / the reciprocal of a basis function is computed once and shared by its value and both derivatives,
// every store is one 16-byte vector (element-wise where m is not a multiple of the group or an array is not 16-byte aligned).
// 256-thread workgroups are dispatched in address order over (problem, piece of 256 groups).  The descriptor travels in the
// kernel arguments: the kind of a basis function is uniform over the wavefront, the switch below is a scalar branch.
//
// Index list: with `list` / `count` (device pointers) only problems list[0 .. *count) are evaluated -- in a fit that is the
// active set the LM step kernel maintains, read on the device; the grid covers the host's upper bound of the count and
// workgroups beyond the count retire at once.
//
// Box bounds (vp_set_bounds): during a bounded fit the LM drivers iterate on an INTERNAL vector u, and the bounded sibling
// of the kernel reads u where the kernel reads alpha, forms alpha_k = g(u_k) per parameter (bound_map below: the MINUIT /
// lmfit maps), evaluates the basis functions at alpha exactly as the unbounded kernel does and multiplies every stored
// derivative column by dalpha_k/du_k of its parameter.  Nothing downstream of the columns knows about the bounds.
//
// Fixed parameters (vp_batch_create_fixed): the handle IS the reduced model -- its parameter vector holds the free
// parameters only, in model order -- and only this kernel and the scan kernel know the full descriptor.  The fixed sibling
// of the bounded kernel reads full parameter k through a map in its argument record: the free vector's entry src[k] (alpha,
// or u of a bounded fit), or, src[k] < 0, the fixed value values[problem][k] -- indexed by the PROBLEM, not by the slot of
// the active list.  Derivative columns are written for free parameters only and numbered by counting free pairs.  The
// selection is uniform over the workgroup.  An unbounded fixed fit runs the sibling with an infinite box (the identity of
// bound_map), so there is one fixed kernel per (dtype, store form), not two.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/varpro_hip.h"
#include "vp_kernels.hpp" // launch_status()
#include "vp_model.hpp"

namespace vp {

// type-erased launch record (host side); every pointer is a device pointer
struct ColsParams {
    int dtype;
    vp_model_desc model;   // the descriptor (all eight device kinds)
    const void *t;         // [m] or [B][t_stride]
    int64_t t_stride;      // 0: shared grid
    const void *alpha;     // [B][q]
    void *phi;             // [B][n_phi_cols][m] or null
    void *dphi;            // [B][p][m] or null
    int skip_invariant;    // VP_BASIS_SKIP_INVARIANT: Phi without its VP_BASIS_CONST columns
    int nt;                // 1: non-temporal stores (the library's default, measured: DESIGN.md section 3f), 0: ordinary
    int m;                 // rows per column
    int64_t B;             // problems (without a list), else the upper bound of *count the grid covers
    const int32_t *list;   // null: problems 0 .. B-1
    const int32_t *count;  // device count of the list (read by the kernel)
    const void *lo, *hi;   // both non-null: `alpha` holds INTERNAL parameters u, the bounded kernel maps them; [q] or [B][q]
    int64_t bound_stride;  // 0: one box for all problems, q: per problem
    const void *irf;       // descriptors with an IRF kind: the response, [m] or [B][irf_stride] (vp_irf.hpp)
    int64_t irf_stride;    // 0: one response for all problems
    double irf_period;     // VP_BASIS_EXP_DECAY_IRF_PERIODIC: the period in grid units, 0: the record is one period
    // descriptors with a shifted IRF kind (vp_irf_shift.hpp): the handle's buffers for the shifted response and its derivative
    void *irf_g, *irf_dg;  // [B][irf_gs] each, 16-byte aligned, indexed by the problem
    int64_t irf_gs;        // m rounded up to a 16-byte group
    hipStream_t stream;
    // fixed parameters (vp_batch_create_fixed): `model` is the FULL descriptor, `alpha` (and lo / hi, which this form always
    // needs: an infinite box where the fit has none) is [B][q_free] over the free parameters in model order
    const int32_t *fix_src;  // host, [model.n_params]: index into the free vector, < 0: fixed; null: nothing is fixed
    const void *fix_values;  // device, [model.n_params] or [B][fix_stride]: entries of free parameters are not read
    int64_t fix_stride;      // 0: one set of values for all problems
    int q_free;
};
// every column of the descriptor: cols_fill_kernel for the pointwise kinds, then the scan kernel for the IRF kinds
int cols_fill(const ColsParams &p);
int irf_cols_fill(const ColsParams &p); // the columns of the IRF kinds alone (vp_irf.hpp)
// the same two for a record with fix_src (the fixed siblings: vp_inst_cols_fixed.hip)
int cols_fill_fixed(const ColsParams &p);
int irf_cols_fill_fixed(const ColsParams &p);
// g and g' of the shifted IRF kinds into p.irf_g / p.irf_dg (vp_inst_irf_shift.hip); delta_param: delta's index among the
// descriptor's parameters; want_dg: g' as well (never written for a delta that p.fix_src fixes)
int irf_resample(const ColsParams &p, int delta_param, bool want_dg);
inline bool is_irf_shift_kind(const int kind) {
    return kind == VP_BASIS_EXP_DECAY_IRF_SHIFT || kind == VP_BASIS_IRF_SHIFT || kind == VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT;
}
inline bool is_irf_kind(const int kind) {
    return kind == VP_BASIS_EXP_DECAY_IRF || kind == VP_BASIS_IRF || kind == VP_BASIS_EXP_DECAY_IRF_PERIODIC || is_irf_shift_kind(kind);
}
// the shift parameter of a descriptor: delta's index, -1 without a shifted kind (creation checks that there is only one)
inline int irf_shift_param(const vp_model_desc &model) {
    for (int j = 0; j < model.n_basis && j < VP_MAX_BASIS; ++j)
        if (is_irf_shift_kind(model.kind[j])) return model.param[j][model.kind[j] == VP_BASIS_IRF_SHIFT ? 0 : 1];
    return -1;
}
// the column numbering of a descriptor: phi_col[j] the Phi column of function j (-1: skipped, a VP_BASIS_CONST under
// skip_invariant), first_pair[j] its first derivative column in dPhi (pairs in model order), and the totals.  fix_src
// (ColsParams): only the pairs of free parameters have a column
struct ColumnMap {
    int phi_col[VP_MAX_BASIS], first_pair[VP_MAX_BASIS];
    int n_phi_cols, n_pairs;
};
inline ColumnMap column_map(const vp_model_desc &model, const int skip_invariant, const int32_t *fix_src = nullptr) {
    ColumnMap c;
    c.n_phi_cols = c.n_pairs = 0;
    for (int j = 0; j < VP_MAX_BASIS; ++j) {
        c.phi_col[j] = -1;
        c.first_pair[j] = c.n_pairs;
        if (j >= model.n_basis) continue;
        if (!(skip_invariant && model.kind[j] == VP_BASIS_CONST)) c.phi_col[j] = c.n_phi_cols++;
        for (int k = 0; k < VP_MAX_BASIS_PARAMS; ++k)
            if (model.param[j][k] >= 0 && !(fix_src && fix_src[model.param[j][k]] < 0)) ++c.n_pairs;
    }
    return c;
}
// in place on x [B][q] (the handle's dtype): x <- g^-1(x) (to_internal != 0) or x <- g(x), the maps of bound_map / bound_unmap
int bounds_transform(int dtype, void *x, const void *lo, const void *hi, int64_t bound_stride, int q, int64_t B, int to_internal,
                     hipStream_t stream);

namespace cols {

template <typename T> struct ColsArgs {
    vp_model_desc mdl;
    int phi_col[VP_MAX_BASIS]; // output column of basis j in Phi, -1: skipped
    int n_phi_cols, n_pairs;
    const T *t;
    const T *alpha;
    T *phi, *dphi;
    const int32_t *list, *count;
    int64_t t_stride, first; // first: problem (or list slot) of workgroup 0
    int m, blocks_per_problem;
};
// the bounded kernel's record: `alpha` holds the internal parameters u
template <typename T> struct ColsBoundArgs : ColsArgs<T> {
    const T *lo, *hi;     // [q] or [B][bound_stride]; an infinite entry: no bound on that side
    int64_t bound_stride; // 0: shared
};
// the fixed kernel's record: `alpha`, lo and hi are [.][q_free] over the free parameters
template <typename T> struct ColsFixedArgs : ColsBoundArgs<T> {
    const T *values;               // [q] or [B][val_stride] over the FULL parameters
    int64_t val_stride;            // 0: shared
    int q_free;
    int32_t src[VP_MAX_PARAMS];    // full parameter k: its index in the free vector, < 0: fixed
};

template <typename T> struct Vec;
template <> struct Vec<double> {
    static constexpr int VW = 2;
    typedef double type __attribute__((ext_vector_type(2)));
};
template <> struct Vec<float> {
    static constexpr int VW = 4;
    typedef float type __attribute__((ext_vector_type(4)));
};

// one column's row group: a 16-byte store (VEC) or element-wise stores of the rows below m
template <typename T, bool VEC, bool NT>
__device__ __forceinline__ void store_group(T *__restrict__ col, const int i, const int m, const T (&v)[Vec<T>::VW]) {
    constexpr int VW = Vec<T>::VW;
    if constexpr (VEC) {
        typename Vec<T>::type x;
#pragma unroll
        for (int e = 0; e < VW; ++e) x[e] = v[e];
        if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<typename Vec<T>::type *>(col + i));
        else *reinterpret_cast<typename Vec<T>::type *>(col + i) = x;
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
            if (i + e < m) {
                if constexpr (NT) __builtin_nontemporal_store(v[e], col + i + e);
                else col[i + e] = v[e];
            }
    }
}

// exp with the limits of an infinite argument: texp forms x - k ln 2 with k = rint(x log2 e), which is inf - inf there.  A
// Gaussian of width 0 has the argument -inf away from its centre and is 0 there, as for a caller's exp().
template <typename T> __device__ __forceinline__ T cexp(const T x) {
    const T v = texp(x);
    return __builtin_isinf(x) ? (x > T(0) ? x : T(0)) : v;
}

// ---- box bounds as a smooth re-parameterisation alpha = g(u) (the maps of MINUIT / lmfit), per parameter ----------------
//   no bound     alpha = u                                   dalpha/du = 1
//   lo and hi    alpha = lo + (hi - lo)/2 (sin u + 1)        dalpha/du = (hi - lo)/2 cos u
//   lo only      alpha = lo - 1 + sqrt(u^2 + 1)              dalpha/du = u / sqrt(u^2 + 1)
//   hi only      alpha = hi + 1 - sqrt(u^2 + 1)              dalpha/du = -u / sqrt(u^2 + 1)
// The value is clamped to [lo, hi] afterwards: rounding never puts a parameter outside its box (a NaN stays a NaN).  ONE
// function serves the column kernel and the map kernel, so the alpha a bounded fit returns is the point at which the fit's
// columns were evaluated; the FMA is explicit so that no compiler decision can make the two differ.
template <typename T> __device__ __forceinline__ T bound_clamp(const T a, const T lo, const T hi) {
    return a < lo ? lo : (a > hi ? hi : a);
}
template <typename T> __device__ __forceinline__ void bound_map(const T u, const T lo, const T hi, T &alpha, T &dalpha_du) {
    const bool has_lo = !__builtin_isinf(lo), has_hi = !__builtin_isinf(hi);
    if (has_lo && has_hi) {
        T sn, cs;
        tsincos(u, sn, cs);
        const T half = T(0.5) * (hi - lo);
        alpha = bound_clamp(tfma(half, sn + T(1), lo), lo, hi);
        dalpha_du = half * cs;
    } else if (has_lo || has_hi) {
        // beyond 2^27 (fp64) / 2^13 (fp32) u^2 + 1 rounds to u^2: |u| itself, which does not overflow
        const T au = u < T(0) ? -u : u;
        const T s = au >= T(sizeof(T) == 8 ? 134217728.0 : 8192.0) ? au : tsqrt(tfma(u, u, T(1)));
        alpha = bound_clamp(has_lo ? (lo - T(1)) + s : (hi + T(1)) - s, lo, hi);
        dalpha_du = has_lo ? u / s : -(u / s);
    } else {
        alpha = u;
        dalpha_du = T(1);
    }
}
// u = g^-1(alpha); alpha is clamped to the box first
__device__ __forceinline__ double tasin(const double x) { return asin(x); }
__device__ __forceinline__ float tasin(const float x) { return asinf(x); }
template <typename T> __device__ __forceinline__ T bound_unmap(const T alpha, const T lo, const T hi) {
    const bool has_lo = !__builtin_isinf(lo), has_hi = !__builtin_isinf(hi);
    const T a = bound_clamp(alpha, lo, hi);
    if (has_lo && has_hi) return tasin(bound_clamp(T(2) * (a - lo) / (hi - lo) - T(1), T(-1), T(1)));
    if (has_lo || has_hi) {
        const T d = has_lo ? (a - lo) + T(1) : (hi - a) + T(1); // >= 1
        return tsqrt(d - T(1)) * tsqrt(d + T(1)); // sqrt(d^2 - 1) without the square: finite for every finite d
    }
    return a;
}

// value and derivatives of ONE basis function at one grid value: f, d0 = df/dp0, d1 = df/dp1 (include/varpro_hip.h).
// The same statements serve the vector and the element-wise variant: a column does not depend on how it was stored.
template <typename T>
__device__ __forceinline__ void basis_at(const int kind, const T t, const T p0, const T p1, const T c0, const T c1, T &f, T &d0,
                                         T &d1) {
    f = T(1);
    d0 = d1 = T(0);
    switch (kind) {
    case VP_BASIS_EXP_DECAY: { // c0 = 1/p0^2
        f = cexp(-(t / p0));
        d0 = (f * t) * c0;
        break;
    }
    case VP_BASIS_EXP_RATE: {
        f = cexp(-(p0 * t));
        d0 = -(t * f);
        break;
    }
    case VP_BASIS_EXP_COS: {
        const T e = cexp(-(p0 * t));
        T sn, cs;
        tsincos(p1 * t, sn, cs);
        f = e * cs;
        d0 = -(t * f);
        d1 = -(t * (e * sn));
        break;
    }
    case VP_BASIS_SIN_PHASE: {
        T sn, cs;
        tsincos(__builtin_fma(p0, t, p1), sn, cs);
        f = sn;
        d0 = t * cs;
        d1 = cs;
        break;
    }
    case VP_BASIS_GAUSS: { // c0 = 1/p1^2, c1 = 1/p1^3
        const T d = t - p0;
        const T z = d / p1;
        f = cexp(-(T(0.5) * (z * z)));
        d0 = (f * d) * c0;
        d1 = (f * (d * d)) * c1;
        break;
    }
    case VP_BASIS_LORENTZ: { // c0 = p1^2
        const T d = t - p0;
        const T dd = d * d;
        const T r = T(1) / (dd + c0);
        const T rr = r * r;
        f = c0 * r;
        d0 = ((T(2) * c0) * d) * rr;
        d1 = ((T(2) * p1) * dd) * rr;
        break;
    }
    case VP_BASIS_LINEAR: f = t; break;
    default: break; // VP_BASIS_CONST
    }
}

// The body of both entry points below.  BND: a.alpha holds the INTERNAL parameters u of a bounded fit -- alpha_k = g(u_k) in
// front of each basis function (per problem, not per row: uniform over the workgroup) and the chain rule on its derivative
// columns; everything else is the same statements for both, so a new kind or option of this route is written once.  Sharing
// the body does change the unbounded kernels' instruction text (operands move) but not what they cost: registers, spills and
// scratch are equal, the instruction count within one, the columns bit-equal and the device time of the fill and of a fit
// inside the spread of the separate kernels' own rounds (profiles/cols_shared_body_*.json).
// FIX (with BND): the fixed sibling -- a parameter comes from the free vector through a.src or from a.values, and only free
// parameters have derivative columns.
template <typename T, bool VEC, bool NT, bool BND, bool FIX = false, typename Args>
__device__ __forceinline__ void cols_fill_body(const Args &a) {
    static_assert(BND || !FIX, "the fixed sibling derives from the bounded body");
    constexpr int VW = Vec<T>::VW;
    const unsigned bpp = (unsigned)a.blocks_per_problem;
    const unsigned slot_local = blockIdx.x / bpp;
    const int piece = (int)(blockIdx.x - slot_local * bpp);
    const int i = VW * (piece * 256 + (int)threadIdx.x);
    const int m = a.m;
    if (i >= m) return;
    int64_t b = a.first + (int64_t)slot_local;
    if (a.list) {
        if (b >= (int64_t)*a.count) return;
        b = a.list[b];
    }
    const T *tg = a.t + b * a.t_stride + i;
    T tt[VW];
    if constexpr (VEC) {
        const typename Vec<T>::type tv = *reinterpret_cast<const typename Vec<T>::type *>(tg);
#pragma unroll
        for (int e = 0; e < VW; ++e) tt[e] = tv[e];
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) tt[e] = tg[i + e < m ? e : 0];
    }
    const int n = a.mdl.n_basis;
    int q = a.mdl.n_params;
    if constexpr (FIX) q = a.q_free;
    const T *al = a.alpha + b * q; // (BND: internal parameters)
    const T *fv = nullptr;
    if constexpr (FIX) fv = a.values + b * a.val_stride; // (b: the problem, also under an active list)
    const T *lo = nullptr, *hi = nullptr;
    if constexpr (BND) lo = a.lo + b * a.bound_stride, hi = a.hi + b * a.bound_stride;
    T *phi = a.phi ? a.phi + b * (int64_t)a.n_phi_cols * m : nullptr;
    T *dphi = a.dphi ? a.dphi + b * (int64_t)a.n_pairs * m : nullptr;
    int pair = 0;
    for (int j = 0; j < n; ++j) {
        const int kind = a.mdl.kind[j];
        const int i0 = a.mdl.param[j][0], i1 = a.mdl.param[j][1];
        T p0 = T(0), p1 = T(0), s0 = T(1), s1 = T(1); // s: dalpha/du
        bool free0 = i0 >= 0, free1 = i1 >= 0;        // the parameter has a derivative column
        if constexpr (FIX) {
            if (i0 >= 0) {
                const int k0 = a.src[i0];
                if (k0 >= 0) bound_map<T>(al[k0], lo[k0], hi[k0], p0, s0);
                else p0 = fv[i0], free0 = false;
            }
            if (i1 >= 0) {
                const int k1 = a.src[i1];
                if (k1 >= 0) bound_map<T>(al[k1], lo[k1], hi[k1], p1, s1);
                else p1 = fv[i1], free1 = false;
            }
        } else if constexpr (BND) {
            if (i0 >= 0) bound_map<T>(al[i0], lo[i0], hi[i0], p0, s0);
            if (i1 >= 0) bound_map<T>(al[i1], lo[i1], hi[i1], p1, s1);
        } else {
            p0 = i0 >= 0 ? al[i0] : T(0), p1 = i1 >= 0 ? al[i1] : T(0);
        }
        // what the rows of this group share: the reciprocals of the derivative scalings
        T c0 = T(0), c1 = T(0);
        if (kind == VP_BASIS_EXP_DECAY) {
            c0 = T(1) / (p0 * p0);
        } else if (kind == VP_BASIS_GAUSS) {
            const T s2 = p1 * p1;
            c0 = T(1) / s2;
            c1 = T(1) / (s2 * p1);
        } else if (kind == VP_BASIS_LORENTZ) {
            c0 = p1 * p1;
        }
        T f[VW], d0[VW], d1[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            basis_at<T>(kind, tt[e], p0, p1, c0, c1, f[e], d0[e], d1[e]);
            if constexpr (BND) {
                d0[e] *= s0;
                d1[e] *= s1;
            }
        }
        if (phi && a.phi_col[j] >= 0) store_group<T, VEC, NT>(phi + (int64_t)a.phi_col[j] * m, i, m, f);
        if (free0) {
            if (dphi) store_group<T, VEC, NT>(dphi + (int64_t)pair * m, i, m, d0);
            ++pair;
        }
        if (free1) {
            if (dphi) store_group<T, VEC, NT>(dphi + (int64_t)pair * m, i, m, d1);
            ++pair;
        }
    }
}
template <typename T, bool VEC, bool NT> __global__ void __launch_bounds__(256) cols_fill_kernel(const ColsArgs<T> a) {
    cols_fill_body<T, VEC, NT, false>(a);
}
template <typename T, bool VEC, bool NT>
__global__ void __launch_bounds__(256) cols_fill_bounded_kernel(const ColsBoundArgs<T> a) {
    cols_fill_body<T, VEC, NT, true>(a);
}
template <typename T, bool VEC, bool NT>
__global__ void __launch_bounds__(256) cols_fill_fixed_kernel(const ColsFixedArgs<T> a) {
    cols_fill_body<T, VEC, NT, true, true>(a);
}

// x <- g^-1(x) (INV) or x <- g(x), one thread per parameter of one problem
template <typename T, bool INV>
__global__ void __launch_bounds__(256) bounds_map_kernel(T *__restrict__ x, const T *__restrict__ lo, const T *__restrict__ hi,
                                                         const int64_t bound_stride, const int q, const int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / q;
    const int64_t k = b * bound_stride + (i - b * q);
    if constexpr (INV) {
        x[i] = bound_unmap<T>(x[i], lo[k], hi[k]);
    } else {
        T alpha, scale;
        bound_map<T>(x[i], lo[k], hi[k], alpha, scale);
        x[i] = alpha;
    }
}
template <typename T>
int launch_bounds_transform(void *x, const void *lo, const void *hi, int64_t bound_stride, int q, int64_t B, int to_internal,
                            hipStream_t stream) {
    const int64_t total = B * q;
    if (total <= 0) return VP_ERR_OK;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (to_internal) hipLaunchKernelGGL((bounds_map_kernel<T, true>), grid, block, 0, stream, (T *)x, (const T *)lo, (const T *)hi, bound_stride, q, total);
    else hipLaunchKernelGGL((bounds_map_kernel<T, false>), grid, block, 0, stream, (T *)x, (const T *)lo, (const T *)hi, bound_stride, q, total);
    return launch_status();
}

// ---- what the launches of this header and of vp_irf.hpp share ----------------------------------------------------------
// fn(std::bool_constant...) with the compile-time form of the run-time switches, in their order
template <typename F> void select_variant(F &&fn) { fn(); }
template <typename F, typename... Rest> void select_variant(F &&fn, const bool first, const Rest... rest) {
    if (first) select_variant([&](auto... c) { fn(std::true_type{}, c...); }, rest...);
    else select_variant([&](auto... c) { fn(std::false_type{}, c...); }, rest...);
}
// 16-byte groups need m to be a multiple of the group and every array (`src`: the array the kernel reads row-wise; each
// column starts a multiple of m from its base) 16-byte aligned
template <typename T> bool vec_groups(const ColsParams &p, const void *src, const int64_t src_stride) {
    auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    return p.m % Vec<T>::VW == 0 && al16(src) && al16(p.phi) && al16(p.dphi) && (src_stride % Vec<T>::VW) == 0;
}
// launch(first, nb) over the B problems in pieces of at most per_launch: what one grid of at most 2^31 - 1 workgroups covers
template <typename F> int launch_chunks(const int64_t B, const int64_t per_launch, F &&launch) {
    for (int64_t first = 0; first < B; first += per_launch) {
        launch(first, B - first < per_launch ? B - first : per_launch);
        if (hipGetLastError() != hipSuccess) return VP_ERR_HIP;
    }
    return VP_ERR_OK;
}

// FIX: the record has fix_src -- the fixed sibling alone (its instantiations live in a unit of their own)
template <typename T, bool FIX = false> int launch_fill(const ColsParams &p) {
    constexpr int VW = Vec<T>::VW;
    if (p.B <= 0 || p.m <= 0 || (!p.phi && !p.dphi)) return VP_ERR_OK;
    if (FIX && !(p.fix_src && p.fix_values && p.lo && p.hi)) return VP_ERR_INVALID;
    std::conditional_t<FIX, ColsFixedArgs<T>, ColsBoundArgs<T>> a; // (the unbounded kernel takes its ColsArgs part)
    const ColumnMap map = column_map(p.model, p.skip_invariant, FIX ? p.fix_src : nullptr);
    if constexpr (FIX) {
        a.values = (const T *)p.fix_values;
        a.val_stride = p.fix_stride;
        a.q_free = p.q_free;
        for (int k = 0; k < VP_MAX_PARAMS; ++k) a.src[k] = k < p.model.n_params ? p.fix_src[k] : -1;
    }
    // the parameter has a derivative column
    auto is_free = [&](const int k) { return k >= 0 && !(FIX && p.fix_src[k] < 0); };
    const int npairs = map.n_pairs;
    a.n_phi_cols = map.n_phi_cols;
    a.n_pairs = npairs;
    a.t = (const T *)p.t;
    a.alpha = (const T *)p.alpha;
    a.phi = map.n_phi_cols > 0 ? (T *)p.phi : nullptr;
    a.list = p.list;
    a.count = p.count;
    a.t_stride = p.t_stride;
    a.m = p.m;
    a.blocks_per_problem = (p.m + 256 * VW - 1) / (256 * VW);
    a.lo = (const T *)p.lo;
    a.hi = (const T *)p.hi;
    a.bound_stride = p.bound_stride;
    if (!a.phi && !(npairs > 0 && p.dphi)) return VP_ERR_OK;
    const bool vec = vec_groups<T>(p, p.t, p.t_stride), bounded = p.lo && p.hi;
    // one launch over the functions a.mdl lists, its derivative columns from pair `pair0` of the problem on
    auto launch = [&](const int pair0) -> int {
        a.dphi = npairs > 0 && p.dphi ? (T *)p.dphi + (int64_t)pair0 * p.m : nullptr;
        if (!a.phi && !a.dphi) return VP_ERR_OK;
        return launch_chunks(p.B, (int64_t)0x7fffffff / a.blocks_per_problem, [&](const int64_t first, const int64_t nb) {
            a.first = first;
            const dim3 grid((unsigned)(nb * a.blocks_per_problem)), block(256);
            if constexpr (FIX) {
                select_variant([&](auto V, auto N) { hipLaunchKernelGGL((cols_fill_fixed_kernel<T, V.value, N.value>), grid, block, 0, p.stream, a); },
                               vec, p.nt != 0);
            } else {
                select_variant(
                    [&](auto V, auto N, auto BD) {
                        if constexpr (BD.value) hipLaunchKernelGGL((cols_fill_bounded_kernel<T, V.value, N.value>), grid, block, 0, p.stream, a);
                        else hipLaunchKernelGGL((cols_fill_kernel<T, V.value, N.value>), grid, block, 0, p.stream, static_cast<const ColsArgs<T> &>(a));
                    },
                    vec, p.nt != 0, bounded);
            }
        });
    };
    // The kernel numbers its derivative columns by counting the parameters of the functions it walks, so the functions of
    // the IRF kinds -- whose columns come from the scan kernel (vp_irf.hpp) -- are taken out of the descriptor it sees: a
    // VP_BASIS_IRF simply (it has no parameters), and at every VP_BASIS_EXP_DECAY_IRF[_PERIODIC] the descriptor is cut, the run of
    // functions behind it going to a launch of its own whose dPhi starts at that run's first pair.  A descriptor without
    // these kinds is one run: the launch it always was.  (FIX: first_pair counts the FREE pairs in front of the run.)
    // The shifted kinds cut the descriptor as well -- VP_BASIS_IRF_SHIFT too: unlike VP_BASIS_IRF it HAS a pair.
    a.mdl = p.model;
    int run = 0, run_pair0 = 0;
    bool stores = false; // the run has a column to write
    auto flush = [&]() -> int {
        int rc = VP_ERR_OK;
        if (run > 0 && stores) {
            a.mdl.n_basis = run;
            for (int j = run; j < VP_MAX_BASIS; ++j) a.phi_col[j] = -1;
            rc = launch(run_pair0);
        }
        run = 0;
        stores = false;
        return rc;
    };
    for (int j = 0; j < p.model.n_basis; ++j) {
        const int kind = p.model.kind[j];
        if (kind == VP_BASIS_IRF) continue;
        if (kind == VP_BASIS_EXP_DECAY_IRF || kind == VP_BASIS_EXP_DECAY_IRF_PERIODIC || is_irf_shift_kind(kind)) {
            if (int rc = flush()) return rc;
            continue;
        }
        if (run == 0) run_pair0 = map.first_pair[j];
        a.mdl.kind[run] = kind;
        for (int k = 0; k < VP_MAX_BASIS_PARAMS; ++k) a.mdl.param[run][k] = p.model.param[j][k];
        a.phi_col[run] = map.phi_col[j];
        if ((a.phi && map.phi_col[j] >= 0) || (p.dphi && (is_free(p.model.param[j][0]) || is_free(p.model.param[j][1])))) stores = true;
        ++run;
    }
    if (int rc = flush()) return rc;
    return VP_ERR_OK;
}

} // namespace cols
} // namespace vp
