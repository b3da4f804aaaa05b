// vp_irf_shift.hpp -- the resample kernel of the shifted IRF kinds (VP_BASIS_EXP_DECAY_IRF_SHIFT, VP_BASIS_IRF_SHIFT,
// VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT; include/varpro_hip.h, "Shifted IRF reconvolution").
//
// For a shift delta (grid units; s = delta/dt bins, positive: later) the shifted response is g_i = r(i - s), r the
// Catmull-Rom cubic through the samples, zero outside the record:
//   o = floor(-s), f = -s - o in [0, 1]                                      (uniform over the problem)
//   g_i  =           sum_{a=-1..2} w_a(f)  irf_{i+o+a}
//   g'_i = -(1/dt)   sum_{a=-1..2} w'_a(f) irf_{i+o+a}                       = dg_i/ddelta
// Every column of a shifted kind is an EXISTING scan (vp_irf.hpp) over g or g': the recurrences and the steady-state carry
// are linear in the response.  So the feature is this pointwise kernel, which writes g and g' per problem into two buffers
// of the handle ([B][ms], ms = m rounded up to a 16-byte group), and host routing (launch_irf).
//
// Work sharing is that of cols_fill_kernel: a THREAD owns one 16-byte row group of one problem; 256-thread workgroups over
// (problem, piece of 256 groups).  The buffers are the handle's own, 16-byte aligned with a row stride of whole groups, so
// every store is one 16-byte vector; rows m .. ms-1 are written as zeros and never read.  The four taps of the VW rows of a
// group are VW + 3 contiguous elements (5 fp64 / 7 fp32), loaded once, element-wise: o is arbitrary, so the run has no
// alignment.  Ordinary stores: the scan reads g / g' in the next launch on the same stream.
//
// Uniform over the problem: delta from `alpha` (through bound_map under a bounded fit -- g' is multiplied by ddelta/du HERE,
// the scan needs no chain rule for delta), or, fixed on a fixed handle, from `values` indexed by the PROBLEM (then dg is
// null: no g' is written); dt as the scan kernel forms it; o, f and the eight weights.  The active list is honoured and the
// buffers are indexed by the problem, not the slot.  A non-finite s gives NaN rows (latched per problem downstream),
// |s| >= m + 2 exact zeros; f = 0 gives w = (0, 1, 0, 0) exactly, so delta = 0 reproduces the response bit for bit.
#pragma once
#include "vp_cols.hpp"
#include "vp_device.hpp"

namespace vp {
namespace cols {

template <typename T> struct ResampleArgs {
    const T *t, *alpha, *irf;
    const T *lo, *hi;   // both non-null: `alpha` holds internal parameters (bound_map)
    const T *values;    // fixed_param >= 0: [q_full] or [B][val_stride]
    T *g, *dg;          // [B][ms]; dg null: delta is fixed, or no derivative is wanted
    const int32_t *list, *count;
    int64_t t_stride, irf_stride, bound_stride, val_stride, first;
    int m, ms, q, param, fixed_param, blocks_per_problem; // param: delta's index in `alpha`; fixed_param: in `values`, < 0: free
};

__device__ __forceinline__ double tfloor(const double x) { return __builtin_floor(x); }
__device__ __forceinline__ float tfloor(const float x) { return __builtin_floorf(x); }
__device__ __forceinline__ double tabs(const double x) { return __builtin_fabs(x); }
__device__ __forceinline__ float tabs(const float x) { return __builtin_fabsf(x); }

template <typename T> __global__ void __launch_bounds__(256) irf_resample_kernel(const ResampleArgs<T> a) {
    constexpr int VW = Vec<T>::VW;
    const unsigned bpp = (unsigned)a.blocks_per_problem;
    const unsigned slot_local = blockIdx.x / bpp;
    const int piece = (int)(blockIdx.x - slot_local * bpp);
    const int i = VW * (piece * 256 + (int)threadIdx.x);
    const int m = a.m;
    if (i >= a.ms) return;
    int64_t b = a.first + (int64_t)slot_local;
    if (a.list) {
        if (b >= (int64_t)*a.count) return;
        b = a.list[b];
    }
    // ---- what the problem's rows share ----
    T delta, ddelta_du = T(1);
    if (a.fixed_param >= 0) {
        delta = a.values[b * a.val_stride + a.fixed_param]; // (b: the problem, also under an active list)
    } else {
        delta = a.alpha[b * a.q + a.param];
        if (a.lo && a.hi) bound_map<T>(delta, a.lo[b * a.bound_stride + a.param], a.hi[b * a.bound_stride + a.param], delta, ddelta_du);
    }
    const T *tg = a.t + b * a.t_stride;
    const T dt = (tg[m - 1] - tg[0]) / T(m - 1); // (m >= 2: creation refuses the shifted kinds on one sample)
    const T ns = -(delta / dt);
    T go[VW], dgo[VW];
    if (!(tabs(ns) < T(m + 2))) {
        // beyond the record on either side: exact zeros; a non-finite shift: NaN rows
        const T v = tabs(ns) <= (sizeof(T) == 8 ? T(1.7976931348623157e308) : T(3.4028234663852886e38)) ? T(0) : T(0) / T(0);
#pragma unroll
        for (int e = 0; e < VW; ++e) go[e] = dgo[e] = v;
    } else {
        const T fl = tfloor(ns);
        const int o = (int)fl; // |o| <= m + 2
        const T f = ns - fl;   // exact; 1 where -s is a tiny negative number: w = (0, 0, 1, 0), the limit
        const T h = T(0.5), ff = f * f;
        const T w0 = h * (f * ((T(2) - f) * f - T(1))), w1 = h * (ff * (T(3) * f - T(5)) + T(2));
        const T w2 = h * (f * ((T(4) - T(3) * f) * f + T(1))), w3 = h * (ff * (f - T(1)));
        const T d0 = h * ((T(4) - T(3) * f) * f - T(1)), d1 = h * (f * (T(9) * f - T(10)));
        const T d2 = h * ((T(8) - T(9) * f) * f + T(1)), d3 = h * (f * (T(3) * f - T(2)));
        const T *irf = a.irf + b * a.irf_stride;
        T x[VW + 3];
#pragma unroll
        for (int e = 0; e < VW + 3; ++e) {
            const int k = i + o - 1 + e;
            x[e] = (k >= 0 && k < m) ? irf[k] : T(0);
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            const bool row = i + e < m;
            const T v = ((w0 * x[e] + w1 * x[e + 1]) + w2 * x[e + 2]) + w3 * x[e + 3];
            const T d = ((d0 * x[e] + d1 * x[e + 1]) + d2 * x[e + 2]) + d3 * x[e + 3];
            go[e] = row ? v : T(0);
            dgo[e] = row ? (-d / dt) * ddelta_du : T(0);
        }
    }
    const int64_t at = b * (int64_t)a.ms;
    store_group<T, true, false>(a.g + at, i, a.ms, go);
    if (a.dg) store_group<T, true, false>(a.dg + at, i, a.ms, dgo);
}

// g (and g', `want_dg` and delta free) of p.B problems into p.irf_g / p.irf_dg; delta_param: delta's FULL parameter index
template <typename T> int launch_resample(const ColsParams &p, const int delta_param, const bool want_dg) {
    constexpr int VW = Vec<T>::VW;
    if (p.B <= 0 || p.m <= 0) return VP_ERR_OK;
    if (!p.irf || !p.irf_g || !p.irf_dg || p.m < 2 || p.irf_gs < p.m || p.irf_gs % VW != 0 || delta_param < 0 ||
        delta_param >= p.model.n_params)
        return VP_ERR_INVALID;
    ResampleArgs<T> a;
    a.t = (const T *)p.t;
    a.alpha = (const T *)p.alpha;
    a.irf = (const T *)p.irf;
    a.lo = (const T *)p.lo;
    a.hi = (const T *)p.hi;
    a.values = (const T *)p.fix_values;
    a.g = (T *)p.irf_g;
    a.dg = want_dg ? (T *)p.irf_dg : nullptr;
    a.list = p.list;
    a.count = p.count;
    a.t_stride = p.t_stride;
    a.irf_stride = p.irf_stride;
    a.bound_stride = p.bound_stride;
    a.val_stride = p.fix_stride;
    a.m = p.m;
    a.ms = (int)p.irf_gs;
    a.q = p.fix_src ? p.q_free : p.model.n_params;
    a.param = delta_param;
    a.fixed_param = -1;
    if (p.fix_src) {
        if (!p.fix_values) return VP_ERR_INVALID;
        if (p.fix_src[delta_param] < 0) a.fixed_param = delta_param, a.param = 0, a.dg = nullptr;
        else a.param = p.fix_src[delta_param];
    }
    a.blocks_per_problem = (a.ms + 256 * VW - 1) / (256 * VW);
    return launch_chunks(p.B, (int64_t)0x7fffffff / a.blocks_per_problem, [&](const int64_t first, const int64_t nb) {
        a.first = first;
        const dim3 grid((unsigned)(nb * a.blocks_per_problem)), block(256);
        hipLaunchKernelGGL((irf_resample_kernel<T>), grid, block, 0, p.stream, a);
    });
}

} // namespace cols
} // namespace vp
