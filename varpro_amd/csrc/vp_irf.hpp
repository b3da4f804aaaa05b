// vp_irf.hpp -- the columns of the IRF reconvolution kinds (VP_BASIS_EXP_DECAY_IRF, VP_BASIS_IRF,
// VP_BASIS_EXP_DECAY_IRF_PERIODIC) of device-column handles.
//
// A reconvolved exponential is not a pointwise function of t: on a uniform grid of step dt, with rho = exp(-dt/tau),
//   Phi_i        = sum_{k<=i} irf_k rho^(i-k)              F_i = irf_i + rho F_{i-1},        F_{-1} = 0
//   dPhi_i/dtau  = dt/tau^2 H_i,  H_i = sum_k (i-k) rho^(i-k) irf_k     H_i = rho (H_{i-1} + F_{i-1})
// (rectangle rule: lag 0 included, no factor dt -- the linear coefficient absorbs it).  cols_fill_kernel gives a thread a row
// group and cannot compute this; the kernel here is a scan of that two-state linear recurrence and fills ONLY the columns of
// the IRF kinds -- the other functions of the descriptor still come from cols_fill_kernel (vp_cols.hpp launch_fill),
// which leaves these columns alone.
//
// Work sharing: ONE WAVEFRONT walks one (problem, IRF-kind function) in tiles of 64 row groups (128 fp64 / 256 fp32 rows).
// A lane owns the 16-byte group cols_fill_kernel's thread owns, so an IRF load and a column store are 1 KB contiguous per wave
// instruction (element-wise where m is not a multiple of the group or an array is not 16-byte aligned).  Per tile
//   1. every lane runs the recurrence over its own rows from a zero start: the affine map of s rows is
//        (F, H) -> (rho^s F + F_loc, rho^s (H + s F) + H_loc)                     -- all lanes share rho
//   2. four DPP row_shr steps compose the lanes' maps inside each 16-lane row (factors rho^VW, ^2VW, ^4VW, ^8VW by repeated
//      squaring), v_readlane takes the four row totals and three wave-uniform compositions (factor rho^16VW) chain them behind
//      the carry of the previous tile -- no LDS, no barrier
//   3. a lane's incoming state is its row's prefix advanced by ITS factor exp(-(k VW dt)/tau), k = lane % 16 -- formed once
//      per function with the library's exp -- plus the exclusive in-row scan; from there it runs the recurrence over its
//      rows once more and stores them.  Lane 63's last row is the next tile's carry (it stays in registers).
// The function, tau and everything derived from them are wave-uniform (SGPRs / uniform VALU).  A problem's tiles run serially
// on its wave: rows are not split over several waves.
//
// Honoured as in cols_fill: the index list of a stepped fit, skip_invariant (through the column numbering), phi / dphi ==
// nullptr, per-problem grids (dt_b = (t_b[m-1] - t_b[0])/(m-1); m == 1: dt = 0), both dtypes, and the bounded form: tau = g(u)
// through bound_map, the derivative column multiplied by dtau/du.  tau <= 0 or NaN gives NaN columns (latched per problem
// downstream); a non-finite IRF entry makes every later row non-finite.
//
// VP_BASIS_EXP_DECAY_IRF_PERIODIC (include/varpro_hip.h, "Periodic IRF reconvolution"): the response repeats every period
// T = P dt, P >= m real bins, and the column is the steady state of the pulse train,
//   Phi_i = sum_{p>=0} sum_k irf_k rho^(i-k+pP)  (terms with i-k+pP >= 0)  = F_i^lin + rho^(i+1) F_{-1}
//   H_i   = H_i^lin + rho^(i+1) (H_{-1} + (i+1) F_{-1})
// -- the SAME recurrence, started from
//   A = F^lin_{m-1}, B = H^lin_{m-1};  g = P - m, e = exp(-(T - m dt)/tau) (1 when g = 0);  E = exp(-T/tau), D = -expm1(-T/tau)
//   F_{-1} = e A / D,   H_{-1} = (e/D) (g A + B + P E A / D)
// (D from expm1: 1 - exp cancels for tau >> T).  irf_cols_periodic_kernel is the scan above run twice over the response:
// pass 0 stores nothing and keeps, in the lane that owns row m-1, the state AT that
// row -- the zero padding of the last tile never enters the totals -- one v_readlane pair delivers (A, B), the carry is formed
// from wave-uniform values, and pass 1 is the scan of kind 9 from that carry.  The response is read twice (the second time
// from cache), nothing is written twice; no LDS, no barrier.  period == 0: T = m dt_b; T < m dt (1 - 1e-6): NaN columns.
//
// The shifted kinds VP_BASIS_EXP_DECAY_IRF_SHIFT / VP_BASIS_IRF_SHIFT / VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT have no kernel
// here: launch_irf below sends them through these kernels as kinds 9 / 10 / 11 over the shifted response g and over
// dg/ddelta, which the resample kernel (vp_irf_shift.hpp) writes per problem first.
#pragma once
#include <type_traits>

#include "vp_cols.hpp"
#include "vp_device.hpp"

namespace vp {
namespace cols {

template <typename T> struct IrfArgs {
    const T *t, *alpha, *irf;
    T *phi, *dphi;
    const T *lo, *hi; // the bounded kernel only: `alpha` holds internal parameters
    const int32_t *list, *count;
    int64_t t_stride, irf_stride, bound_stride, first, slots; // slots: problems (or list slots) this launch covers
    int m, q, n_phi_cols, n_pairs, nf;                        // nf: functions of the IRF kinds that have something to store
    int kind[VP_MAX_BASIS], phi_col[VP_MAX_BASIS], pair[VP_MAX_BASIS], param[VP_MAX_BASIS];
};
// the fixed sibling's record (vp_batch_create_fixed; vp_cols.hpp): `alpha`, lo, hi and q are those of the FREE vector, param[f]
// indexes it and pair[f] counts free pairs -- unless the function's tau is fixed: then it comes from `values`, indexed by the
// problem and the FULL parameter fixed_param[f], and the function has no derivative column
template <typename T> struct IrfFixedArgs : IrfArgs<T> {
    const T *values;      // [q_full] or [B][val_stride]
    int64_t val_stride;   // 0: shared
    int fixed_param[VP_MAX_BASIS]; // < 0: tau is free
};

__device__ __forceinline__ double texpm1(const double x) { return expm1(x); }
__device__ __forceinline__ float texpm1(const float x) { return expm1f(x); }

constexpr int DPP_ROW_SHR = 0x110; // + distance 1..15: lane k of a 16-lane row reads lane k - d, lanes k < d read 0

// the IRF group of lane-row i (zeros beyond m)
template <typename T, bool VEC>
__device__ __forceinline__ void load_group(const T *__restrict__ src, const int i, const int m, T (&x)[Vec<T>::VW]) {
    constexpr int VW = Vec<T>::VW;
    if constexpr (VEC) {
        typename Vec<T>::type v;
#pragma unroll
        for (int e = 0; e < VW; ++e) v[e] = T(0);
        if (i < m) v = *reinterpret_cast<const typename Vec<T>::type *>(src + i);
#pragma unroll
        for (int e = 0; e < VW; ++e) x[e] = v[e];
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) x[e] = i + e < m ? src[i + e] : T(0);
    }
}

// The body of both entry points below.  PER: every function of the launch is a VP_BASIS_EXP_DECAY_IRF_PERIODIC (launch_irf),
// `period` in grid units or 0.  The tile loop is written once (`scan`): the zero-start kernel runs it once, the periodic
// kernel twice -- without stores for the totals at row m-1, then from the steady-state carry.  The entry points keep their
// names and argument records; the body is shared although that changes the zero-start kernels' instruction text, because
// it costs them nothing: no kernel of the family needs more registers, spills or scratch than with a body of its own (14 need
// 1 to 6 VGPRs fewer), the columns are bit-equal and the device time of the fill and of a fit lies inside the spread of the
// separate kernels' own rounds (profiles/cols_shared_body_*.json).
// Args = IrfFixedArgs (with BND): the fixed sibling -- a fixed tau is read from a.values and has no derivative column.
template <typename T, bool VEC, bool NT, bool BND, bool PER, typename Args>
__device__ __forceinline__ void irf_cols_body(const Args &a, const T period) {
    constexpr bool FIX = std::is_same<Args, IrfFixedArgs<T>>::value;
    static_assert(BND || !FIX, "the fixed sibling derives from the bounded body");
    constexpr int VW = Vec<T>::VW, TILE = 64 * VW;
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned wave = blockIdx.x * 4u + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned nf = (unsigned)a.nf;
    const unsigned slot_local = wave / nf;
    const int f = (int)(wave - slot_local * nf);
    if ((int64_t)slot_local >= a.slots) return;
    int64_t b = a.first + (int64_t)slot_local;
    if (a.list) {
        if (b >= (int64_t)*a.count) return;
        b = a.list[b];
    }
    const int m = a.m;
    const T *irf = a.irf + b * a.irf_stride;
    T *phi = (a.phi && a.phi_col[f] >= 0) ? a.phi + (b * (int64_t)a.n_phi_cols + a.phi_col[f]) * m : nullptr;
    if constexpr (!PER) {
        if (a.kind[f] == VP_BASIS_IRF) { // the response itself: a copy
            if (!phi) return;
            for (int base = 0; base < m; base += TILE) {
                const int i = base + VW * lane;
                T x[VW];
                load_group<T, VEC>(irf, i, m, x);
                if (i < m) store_group<T, VEC, NT>(phi, i, m, x);
            }
            return;
        }
    }
    T *dphi = a.dphi ? a.dphi + (b * (int64_t)a.n_pairs + a.pair[f]) * m : nullptr;
    // ---- what the function's rows share (wave-uniform) ----
    const int pi = a.param[f];
    T tau = a.alpha[b * a.q + pi], dtau_du = T(1);
    if constexpr (BND) bound_map<T>(tau, a.lo[b * a.bound_stride + pi], a.hi[b * a.bound_stride + pi], tau, dtau_du);
    if constexpr (FIX) {
        // (wave-uniform: f is.  The loads above read entry 0 of the free vector and of the box for such a function)
        if (a.fixed_param[f] >= 0) {
            tau = a.values[b * a.val_stride + a.fixed_param[f]]; // (b: the problem, also under an active list)
            dtau_du = T(1);
            dphi = nullptr;
        }
    }
    if (!(tau > T(0))) tau = T(0) / T(0); // tau <= 0, NaN: not a decay -- NaN columns
    const T *tg = a.t + b * a.t_stride;
    const T dt = m > 1 ? (tg[m - 1] - tg[0]) / T(m - 1) : T(0);
    const T span = T(m) * dt; // (PER) the record, and what the period adds to it
    T gap = T(0);
    if (PER && period > T(0)) {
        gap = period - span;
        if (gap < T(-1e-6) * span) tau = T(0) / T(0); // a period shorter than the record: NaN columns
        if (!(gap > T(0))) gap = T(0);                // (inside the tolerance of the uniformity check: one period)
    }
    const T rho = cexp(-(dt / tau)); // (tau -> 0+: exp(-inf) = 0, the column is the response)
    const T dscale = (dt / (tau * tau)) * dtau_du;
    // rho^(VW d), d = 1, 2, 4, 8, 16 lanes
    T pw[5];
    pw[0] = rho * rho;
    if constexpr (VW == 4) pw[0] *= pw[0];
#pragma unroll
    for (int s = 1; s < 5; ++s) pw[s] = pw[s - 1] * pw[s - 1];
    // the lane's own factor: k groups behind the first lane of its 16-lane row
    const int k = lane & 15, row = lane >> 4;
    const T kspan = T(VW * k);
    const T lf = k == 0 ? T(1) : cexp(-((kspan * dt) / tau));
    T cF = T(0), cH = T(0); // state at the end of the previous tile (uniform)
    T mF = T(0), mH = T(0); // (PER) the totals pass: the state at row m-1, in the lane that owns the row
    // one pass over the response from the carry (cF, cH): the columns, or (PER) the totals without stores
    auto scan = [&](auto stores) {
        constexpr bool STORE = decltype(stores)::value;
        T xn[VW];
        load_group<T, VEC>(irf, VW * lane, m, xn);
        for (int base = 0; base < m; base += TILE) {
            const int i = base + VW * lane;
            T x[VW];
#pragma unroll
            for (int e = 0; e < VW; ++e) x[e] = xn[e];
            if (base + TILE < m) load_group<T, VEC>(irf, i + TILE, m, xn); // (the next tile's group, in flight during the scan)
            // 1. the lane's rows from a zero start
            T F = T(0), H = T(0);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                H = rho * (H + F);
                F = tfma(rho, F, x[e]);
            }
            // 2. inclusive scan inside the 16-lane rows, then the rows behind the carry
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                T Fl, Hl;
                if (s == 0) Fl = dpp<DPP_ROW_SHR + 1>(F), Hl = dpp<DPP_ROW_SHR + 1>(H);
                else if (s == 1) Fl = dpp<DPP_ROW_SHR + 2>(F), Hl = dpp<DPP_ROW_SHR + 2>(H);
                else if (s == 2) Fl = dpp<DPP_ROW_SHR + 4>(F), Hl = dpp<DPP_ROW_SHR + 4>(H);
                else Fl = dpp<DPP_ROW_SHR + 8>(F), Hl = dpp<DPP_ROW_SHR + 8>(H);
                H = tfma(pw[s], tfma(T(VW << s), Fl, Hl), H);
                F = tfma(pw[s], Fl, F);
            }
            T pF = cF, pH = cH; // prefix of this lane's row
            {
                T qF = cF, qH = cH;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const T rF = readlane(F, 16 * r + 15), rH = readlane(H, 16 * r + 15);
                    qH = tfma(pw[4], tfma(T(16 * VW), qF, qH), rH);
                    qF = tfma(pw[4], qF, rF);
                    if (row > r) pF = qF, pH = qH;
                }
            }
            // 3. the lane's incoming state, its rows, the carry
            F = tfma(lf, pF, dpp<DPP_ROW_SHR + 1>(F));
            H = tfma(lf, tfma(kspan, pF, pH), dpp<DPP_ROW_SHR + 1>(H));
            T fo[VW], ho[VW];
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                H = rho * (H + F);
                F = tfma(rho, F, x[e]);
                fo[e] = F;
                ho[e] = dscale * H;
                if constexpr (!STORE)
                    if (i + e == m - 1) mF = F, mH = H;
            }
            if (STORE && i < m) {
                if (phi) store_group<T, VEC, NT>(phi, i, m, fo);
                if (dphi) store_group<T, VEC, NT>(dphi, i, m, ho);
            }
            cF = readlane(F, 63);
            cH = readlane(H, 63);
        }
    };
    if constexpr (PER) {
        scan(std::false_type{});
        // the steady-state carry from the totals at row m-1 (everything wave-uniform)
        const int owner = ((m - 1) % TILE) / VW;
        const T A = readlane(mF, owner), B = readlane(mH, owner);
        const T per = span + gap, g = gap / dt, arg = -(per / tau);
        const T e = gap > T(0) ? cexp(-(gap / tau)) : T(1);
        const T E = cexp(arg), D = -texpm1(arg);
        cF = (e * A) / D;
        cH = (e / D) * (g * A + B + (T(m) + g) * E * A / D);
    }
    scan(std::true_type{});
}
template <typename T, bool VEC, bool NT, bool BND> __global__ void __launch_bounds__(256) irf_cols_kernel(const IrfArgs<T> a) {
    irf_cols_body<T, VEC, NT, BND, false>(a, T(0));
}
template <typename T, bool VEC, bool NT, bool BND>
__global__ void __launch_bounds__(256) irf_cols_periodic_kernel(const IrfArgs<T> a, const T period) {
    irf_cols_body<T, VEC, NT, BND, true>(a, period);
}

template <typename T, bool VEC, bool NT>
__global__ void __launch_bounds__(256) irf_cols_fixed_kernel(const IrfFixedArgs<T> a) {
    irf_cols_body<T, VEC, NT, true, false>(a, T(0));
}
template <typename T, bool VEC, bool NT>
__global__ void __launch_bounds__(256) irf_cols_periodic_fixed_kernel(const IrfFixedArgs<T> a, const T period) {
    irf_cols_body<T, VEC, NT, true, true>(a, period);
}

// the columns of the IRF kinds: one launch of irf_cols_kernel over the functions of kinds 9 and 10, one of
// irf_cols_periodic_kernel over those of kind 11 (a descriptor may mix them; the pairs are numbered over the whole descriptor)
// FIX: the record has fix_src -- the fixed siblings alone (their instantiations live in a unit of their own)
//
// The shifted kinds 12 / 13 / 14 (vp_irf_shift.hpp) go to the SAME kernels as kinds 9 / 10 / 11, in passes of their own behind
// the resample kernel: a value pass over g (Phi and d/dtau where the unshifted kinds read the handle's response), and, where
// dPhi is wanted and delta is free, a derivative pass over g' in which the kernel's "Phi" is the dPhi array and a function's
// "Phi column" the pair (function, delta) -- the kernel's own derivative output is dropped (a.dphi = nullptr).
template <typename T, bool FIX = false> int launch_irf(const ColsParams &p) {
    if (p.B <= 0 || p.m <= 0 || (!p.phi && !p.dphi)) return VP_ERR_OK;
    if (!p.irf) return VP_ERR_INVALID;
    if (FIX && !(p.fix_src && p.fix_values && p.lo && p.hi)) return VP_ERR_INVALID;
    const bool bounded = p.lo && p.hi;
    const ColumnMap map = column_map(p.model, p.skip_invariant, FIX ? p.fix_src : nullptr);
    auto is_free = [&](const int k) { return k >= 0 && !(FIX && p.fix_src[k] < 0); }; // the parameter has a derivative column
    std::conditional_t<FIX, IrfFixedArgs<T>, IrfArgs<T>> a;
    if constexpr (FIX) {
        a.values = (const T *)p.fix_values;
        a.val_stride = p.fix_stride;
    }
    a.t = (const T *)p.t;
    a.alpha = (const T *)p.alpha;
    a.lo = (const T *)p.lo;
    a.hi = (const T *)p.hi;
    a.list = p.list;
    a.count = p.count;
    a.t_stride = p.t_stride;
    a.bound_stride = p.bound_stride;
    a.m = p.m;
    a.q = FIX ? p.q_free : p.model.n_params;
    a.n_pairs = map.n_pairs;
    const T period = (T)p.irf_period;
    enum { UNSHIFTED = 0, SHIFT_VALUE = 1, SHIFT_DELTA = 2 };
    // one pass over the response `src`: the functions of the unshifted kinds, or those of the shifted kinds as kinds 9 - 11
    auto run = [&](const int pass, const void *src, const int64_t src_stride) -> int {
        const bool vec = vec_groups<T>(p, src, src_stride);
        a.irf = (const T *)src;
        a.irf_stride = src_stride;
        if (pass == SHIFT_DELTA) {
            a.phi = (T *)p.dphi;
            a.n_phi_cols = map.n_pairs;
            a.dphi = nullptr;
        } else {
            a.phi = (T *)p.phi;
            a.n_phi_cols = map.n_phi_cols;
            a.dphi = map.n_pairs > 0 ? (T *)p.dphi : nullptr;
        }
        for (int periodic = 0; periodic < 2; ++periodic) {
            int nf = 0;
            for (int j = 0; j < p.model.n_basis && j < VP_MAX_BASIS; ++j) {
                int kind = p.model.kind[j]; // (as the kernel sees it)
                if (is_irf_shift_kind(kind) != (pass != UNSHIFTED)) continue;
                if (kind == VP_BASIS_EXP_DECAY_IRF_SHIFT) kind = VP_BASIS_EXP_DECAY_IRF;
                else if (kind == VP_BASIS_IRF_SHIFT) kind = VP_BASIS_IRF;
                else if (kind == VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT) kind = VP_BASIS_EXP_DECAY_IRF_PERIODIC;
                const bool wanted = periodic ? kind == VP_BASIS_EXP_DECAY_IRF_PERIODIC
                                             : (kind == VP_BASIS_IRF ? a.phi != nullptr : kind == VP_BASIS_EXP_DECAY_IRF);
                if (!wanted) continue;
                const int k = kind == VP_BASIS_IRF ? -1 : p.model.param[j][0]; // tau (a VP_BASIS_IRF reads no parameter)
                a.kind[nf] = kind;
                a.phi_col[nf] = map.phi_col[j];
                if (pass == SHIFT_DELTA) { // the pair (j, delta): behind the pair of tau where tau is free
                    if (!is_free(p.model.param[j][kind == VP_BASIS_IRF ? 0 : 1])) continue;
                    a.phi_col[nf] = map.first_pair[j] + (is_free(k) ? 1 : 0);
                }
                a.pair[nf] = map.first_pair[j];
                a.param[nf] = k >= 0 ? k : 0;
                if constexpr (FIX) {
                    a.fixed_param[nf] = k >= 0 && p.fix_src[k] < 0 ? k : -1;
                    a.param[nf] = k >= 0 && p.fix_src[k] >= 0 ? p.fix_src[k] : 0;
                }
                ++nf;
            }
            if (nf == 0) continue;
            for (int f = nf; f < VP_MAX_BASIS; ++f) a.kind[f] = a.phi_col[f] = a.pair[f] = a.param[f] = 0;
            if constexpr (FIX)
                for (int f = nf; f < VP_MAX_BASIS; ++f) a.fixed_param[f] = -1;
            a.nf = nf;
            // (4 waves per workgroup)
            const int rc = launch_chunks(p.B, (int64_t)0x7fffffff / nf, [&](const int64_t first, const int64_t nb) {
                a.first = first;
                a.slots = nb;
                const dim3 grid((unsigned)((nb * nf + 3) / 4)), block(256);
                if constexpr (FIX) {
                    select_variant(
                        [&](auto V, auto N, auto PER) {
                            if constexpr (PER.value) hipLaunchKernelGGL((irf_cols_periodic_fixed_kernel<T, V.value, N.value>), grid, block, 0, p.stream, a, period);
                            else hipLaunchKernelGGL((irf_cols_fixed_kernel<T, V.value, N.value>), grid, block, 0, p.stream, a);
                        },
                        vec, p.nt != 0, periodic != 0);
                } else {
                    select_variant(
                        [&](auto V, auto N, auto BD, auto PER) {
                            if constexpr (PER.value) hipLaunchKernelGGL((irf_cols_periodic_kernel<T, V.value, N.value, BD.value>), grid, block, 0, p.stream, a, period);
                            else hipLaunchKernelGGL((irf_cols_kernel<T, V.value, N.value, BD.value>), grid, block, 0, p.stream, a);
                        },
                        vec, p.nt != 0, bounded, periodic != 0);
                }
            });
            if (rc) return rc;
        }
        return VP_ERR_OK;
    };
    if (int rc = run(UNSHIFTED, p.irf, p.irf_stride)) return rc;
    const int delta = irf_shift_param(p.model);
    if (delta < 0) return VP_ERR_OK;
    if (!p.irf_g || !p.irf_dg) return VP_ERR_INVALID;
    const bool want_dg = p.dphi && is_free(delta);
    if (int rc = irf_resample(p, delta, want_dg)) return rc;
    if (int rc = run(SHIFT_VALUE, p.irf_g, p.irf_gs)) return rc;
    if (want_dg)
        if (int rc = run(SHIFT_DELTA, p.irf_dg, p.irf_gs)) return rc;
    return VP_ERR_OK;
}

} // namespace cols
} // namespace vp
