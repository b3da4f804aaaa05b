// vp_poisson.hpp -- Poisson re-weighting of a single-RHS batch (vp_poisson_reweight): weights from the counts (Neyman) or
// from the current best fit (model / Pearson weighting), the weighted data, and the Poisson deviance and Pearson X^2 of the
// fit, in ONE pass over the arrays.  Iterating {fit with w = 1/sqrt(f) held fixed, re-form f} has the Poisson score equations
// sum_i (y_i - f_i)/f_i df_i/dtheta = 0 as its fixed point: the LM kernels are untouched, the maximum-likelihood fit is this
// kernel between their launches.
//
//   v_i = max(y_i, floor)  (Neyman)   or   max(f_i, floor)  (model);      w_i = 1/sqrt(v_i);      Y_w,i = w_i y_i
//   model mode, with ft = max(f, floor):   D = 2 sum [ y ln(y/ft) - (y - ft) ]  (the logarithmic term is 0 for y <= 0)
//                                          X^2 = sum (y - ft)^2 / ft
// 1/sqrt is the compiler's full-precision square root (within one unit in the last place) followed by the correctly rounded
// division, not v_rsq: the kernel moves four or five arrays and has the arithmetic to spare, and a host mirror in the same
// dtype reproduces w to those two roundings (tests/test_gpu_poisson.py states the bound).  max is written
// `x < floor ? floor : x`, so a NaN goes through; a v that is not finite gives w = NaN (an infinite count or fit must latch
// the problem at its next evaluation, like every other non-finite input, instead of passing as weight 0).
// D and X^2 are accumulated in fp64 for both dtypes.
//
// Work sharing: ONE WAVEFRONT per problem, four problems per 256-thread workgroup.  A lane owns a 16-byte group (2 fp64 /
// 4 fp32 rows) of every tile of 64 groups -- a load or store is 1 KB contiguous per wave instruction -- element-wise where m
// is not a multiple of the group or an array is not 16-byte aligned (the vec_groups rule of the column kernels).  A lane adds
// its terms tile by tile, the 64 partial sums go through wave_sum's fixed tree: no atomics, no LDS, and a result does not
// depend on the launch geometry (which wave runs a problem changes nothing).  Stores are ordinary: the fit reads w and Y_w next.
// A problem whose status is non-zero in model mode (its fit is not a fit) keeps its w and Y_w and gets NaN sums.
#pragma once
#include "vp_cols.hpp"
#include "vp_device.hpp"

namespace vp {

// type-erased launch record (host side); every pointer is a device pointer
struct PoissonParams {
    int dtype;
    const void *Y;          // [B][m] counts
    const void *F;          // [B][m] unweighted best fit, null: Neyman mode
    const int32_t *status;  // [B], read in model mode
    void *w, *yw;           // [B][m] out
    double *deviance;       // [B] out or null (model mode)
    double *pearson;        // [B] out or null (model mode)
    double floor;
    int m;
    int64_t B;
    hipStream_t stream;
};
int poisson_reweight_launch(const PoissonParams &p);

namespace poisson {

using cols::Vec;

template <typename T> struct Args {
    const T *Y, *F;
    const int32_t *status;
    T *w, *yw;
    double *deviance, *pearson;
    int64_t first, end; // problems first .. end-1 belong to this launch
    T floor;
    int m;
};

template <typename T, bool VEC>
__device__ __forceinline__ void load_group(const T *src, const int i, const int m, T (&x)[Vec<T>::VW]) {
    constexpr int VW = Vec<T>::VW;
    if constexpr (VEC) {
        const typename Vec<T>::type v = *reinterpret_cast<const typename Vec<T>::type *>(src + i);
#pragma unroll
        for (int e = 0; e < VW; ++e) x[e] = v[e];
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) x[e] = i + e < m ? src[i + e] : T(1);
    }
}

// (Y and yw carry no __restrict__: a caller may hand the same array to both, every element is read and written by one thread)
template <typename T, bool VEC, bool MODEL> __global__ void __launch_bounds__(256) poisson_reweight_kernel(const Args<T> a) {
    constexpr int VW = Vec<T>::VW, TILE = 64 * VW;
    const int lane = lane_id();
    const int64_t b = a.first + (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (b >= a.end) return;
    if constexpr (MODEL) {
        if (a.status[b] != 0) { // a failed round must not poison the next one
            const double nan = __builtin_nan("");
            if (lane == 0) {
                if (a.deviance) a.deviance[b] = nan;
                if (a.pearson) a.pearson[b] = nan;
            }
            return;
        }
    }
    const int m = a.m;
    const T floor = a.floor;
    const T *y = a.Y + b * m;
    const T *f = MODEL ? a.F + b * m : nullptr;
    T *w = a.w + b * m, *yw = a.yw + b * m;
    double dsum = 0.0, xsum = 0.0;
    for (int base = 0; base < m; base += TILE) {
        const int i = base + VW * lane;
        if (i < m) {
            T yv[VW], fv[VW], wv[VW], ywv[VW];
            load_group<T, VEC>(y, i, m, yv);
            if constexpr (MODEL) load_group<T, VEC>(f, i, m, fv);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                const T x = MODEL ? fv[e] : yv[e];
                const T v = x < floor ? floor : x; // (a NaN stays)
                const T r = T(1) / tsqrt(v);
                wv[e] = is_finite(v) ? r : T(0) / T(0);
                ywv[e] = wv[e] * yv[e];
                if constexpr (MODEL) {
                    if (VEC || i + e < m) {
                        const double yd = (double)yv[e], fd = (double)v;
                        const double diff = yd - fd;
                        const double lg = yd > 0.0 ? yd * log(yd / fd) : 0.0;
                        dsum += lg - diff;
                        xsum += diff * diff / fd;
                    }
                }
            }
            cols::store_group<T, VEC, false>(w, i, m, wv);
            cols::store_group<T, VEC, false>(yw, i, m, ywv);
        }
    }
    if constexpr (MODEL) {
        double s[2] = {dsum, xsum};
        wave_allreduce(s);
        if (lane == 0) {
            if (a.deviance) a.deviance[b] = 2.0 * s[0];
            if (a.pearson) a.pearson[b] = s[1];
        }
    }
}

template <typename T> int launch(const PoissonParams &p) {
    if (p.B <= 0 || p.m <= 0) return VP_ERR_OK;
    if (!p.Y || !p.w || !p.yw || (p.F && !p.status)) return VP_ERR_INVALID;
    // 16-byte groups: m a multiple of the group (every problem's rows then start 16-byte aligned) and every array aligned
    auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool vec = p.m % Vec<T>::VW == 0 && al16(p.Y) && al16(p.F) && al16(p.w) && al16(p.yw);
    Args<T> a;
    a.Y = (const T *)p.Y;
    a.F = (const T *)p.F;
    a.status = p.status;
    a.w = (T *)p.w;
    a.yw = (T *)p.yw;
    a.deviance = p.deviance;
    a.pearson = p.pearson;
    a.floor = (T)p.floor;
    a.m = p.m;
    // (4 problems per workgroup)
    return cols::launch_chunks(p.B, (int64_t)0x7fffffff, [&](const int64_t first, const int64_t nb) {
        a.first = first;
        a.end = first + nb;
        const dim3 grid((unsigned)((nb + 3) / 4)), block(256);
        cols::select_variant(
            [&](auto V, auto M) { hipLaunchKernelGGL((poisson_reweight_kernel<T, V.value, M.value>), grid, block, 0, p.stream, a); },
            vec, p.F != nullptr);
    });
}

} // namespace poisson
} // namespace vp
