// vp_cols.hpp -- the column kernel of DEVICE-COLUMN handles: descriptors that contain VP_BASIS_GAUSS / VP_BASIS_LORENTZ /
// VP_BASIS_LINEAR.  One kernel family evaluates the UNWEIGHTED basis matrix Phi [B][n][m] and the derivative columns dPhi
// [B][p][m] (pairs in model order, basis-major: vp_basis' layout) of a run-time descriptor into device memory; everything
// downstream of the columns is done by the caller-evaluated kernels (vp_ext.hpp, vp_blk_ext.hpp, vp_extfit.hpp, ...) exactly
// as for a caller's columns.  All eight device kinds are evaluated here, so a descriptor may mix a Gaussian with an
// exponential tail and a baseline.
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
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/varpro_hip.h"
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
    hipStream_t stream;
};
int cols_fill(const ColsParams &p);

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

template <typename T, bool VEC, bool NT> __global__ void __launch_bounds__(256) cols_fill_kernel(const ColsArgs<T> a) {
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
    const int n = a.mdl.n_basis, q = a.mdl.n_params;
    const T *al = a.alpha + b * q;
    T *phi = a.phi ? a.phi + b * (int64_t)a.n_phi_cols * m : nullptr;
    T *dphi = a.dphi ? a.dphi + b * (int64_t)a.n_pairs * m : nullptr;
    int pair = 0;
    for (int j = 0; j < n; ++j) {
        const int kind = a.mdl.kind[j];
        const int i0 = a.mdl.param[j][0], i1 = a.mdl.param[j][1];
        const T p0 = i0 >= 0 ? al[i0] : T(0), p1 = i1 >= 0 ? al[i1] : T(0);
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
        for (int e = 0; e < VW; ++e) basis_at<T>(kind, tt[e], p0, p1, c0, c1, f[e], d0[e], d1[e]);
        if (phi && a.phi_col[j] >= 0) store_group<T, VEC, NT>(phi + (int64_t)a.phi_col[j] * m, i, m, f);
        if (i0 >= 0) {
            if (dphi) store_group<T, VEC, NT>(dphi + (int64_t)pair * m, i, m, d0);
            ++pair;
        }
        if (i1 >= 0) {
            if (dphi) store_group<T, VEC, NT>(dphi + (int64_t)pair * m, i, m, d1);
            ++pair;
        }
    }
}

template <typename T> int launch_fill(const ColsParams &p) {
    constexpr int VW = Vec<T>::VW;
    if (p.B <= 0 || p.m <= 0 || (!p.phi && !p.dphi)) return VP_ERR_OK;
    ColsArgs<T> a;
    a.mdl = p.model;
    int ncols = 0, npairs = 0;
    for (int j = 0; j < VP_MAX_BASIS; ++j) {
        a.phi_col[j] = -1;
        if (j >= p.model.n_basis) continue;
        if (!(p.skip_invariant && p.model.kind[j] == VP_BASIS_CONST)) a.phi_col[j] = ncols++;
        for (int k = 0; k < VP_MAX_BASIS_PARAMS; ++k)
            if (p.model.param[j][k] >= 0) ++npairs;
    }
    a.n_phi_cols = ncols;
    a.n_pairs = npairs;
    a.t = (const T *)p.t;
    a.alpha = (const T *)p.alpha;
    a.phi = ncols > 0 ? (T *)p.phi : nullptr;
    a.dphi = npairs > 0 ? (T *)p.dphi : nullptr;
    a.list = p.list;
    a.count = p.count;
    a.t_stride = p.t_stride;
    a.m = p.m;
    a.blocks_per_problem = (p.m + 256 * VW - 1) / (256 * VW);
    if (!a.phi && !a.dphi) return VP_ERR_OK;
    // 16-byte groups need m to be a multiple of the group and every array (each column starts a multiple of m from its base)
    // 16-byte aligned
    auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool vec = p.m % VW == 0 && al16(p.t) && al16(p.phi) && al16(p.dphi) && (p.t_stride % VW) == 0;
    const int64_t per_launch = ((int64_t)0x7fffffff / a.blocks_per_problem); // problems one grid can cover
    for (int64_t first = 0; first < p.B; first += per_launch) {
        const int64_t nb = p.B - first < per_launch ? p.B - first : per_launch;
        a.first = first;
        const dim3 grid((unsigned)(nb * a.blocks_per_problem)), block(256);
        if (vec) {
            if (p.nt) hipLaunchKernelGGL((cols_fill_kernel<T, true, true>), grid, block, 0, p.stream, a);
            else hipLaunchKernelGGL((cols_fill_kernel<T, true, false>), grid, block, 0, p.stream, a);
        } else {
            if (p.nt) hipLaunchKernelGGL((cols_fill_kernel<T, false, true>), grid, block, 0, p.stream, a);
            else hipLaunchKernelGGL((cols_fill_kernel<T, false, false>), grid, block, 0, p.stream, a);
        }
        if (hipGetLastError() != hipSuccess) return VP_ERR_HIP;
    }
    return VP_ERR_OK;
}

} // namespace cols
} // namespace vp
