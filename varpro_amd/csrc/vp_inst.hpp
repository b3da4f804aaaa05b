// vp_inst.hpp -- instantiates one (dtype, model, R, W) register-resident kernel set and registers it.
#pragma once
#include "vp_fit2.hpp"
#include "vp_fitg.hpp"
#include "vp_lm_core.hpp"
#include "vp_mrhs.hpp"
#include "vp_stats.hpp"
#include "vp_registry.hpp"

namespace vp {
template <class M> int launch_fitg_entry(const LaunchParams &p) { return launch_fitg<M>(p, p.gram_dbg); }

// the groups of kernels a resident set carries, a compile-time mask: a launcher that is only named is instantiated with its kernel
enum : unsigned {
    SET_SINGLE = 1,  // evaluate, statistics, the wave(-group)-per-problem fit and, for models of fit_rescue_v, its scaled re-fit
    SET_SLOT = 2,    // the persistent slot kernel as `fit`
    SET_MRHS = 4,    // the multi-RHS kernels
    SET_GRAM = 8,    // fp32 only: the fp64-Gram fit (vp_fitg.hpp) as `fit`, in place of both Householder fit kernels
    SET_LDS_W = 16,  // records the LDS a weighted fit needs (multi-wave groups: find_kernels skips a set that cannot stage it)
};

// basis and best_fit are in every set
template <typename T, class M, int R, int W, unsigned PARTS>
KernelEntry resident_set(int dtype, int family, int a, int b, int c) {
    KernelEntry e{};
    e.dtype = dtype; e.family = family; e.a = a; e.b = b; e.c = c; e.R = R; e.W = W;
    e.basis = &launch_basis<T, M, R, W>;
    e.best_fit = &launch_best_fit<T, M, R, W>;
    if constexpr ((PARTS & SET_SINGLE) != 0) {
        e.evaluate = &launch_evaluate<T, M, R, W>;
        e.stats = &launch_stats<T, M, R, W>;
        if constexpr ((PARTS & SET_GRAM) == 0) {
            e.fit_single = &launch_fit<T, M, R, W>;
            if constexpr (fit_rescue_v<T, M>) e.fit_rescue = &launch_fit_rescue<T, M, R, W>;
        }
    }
    if constexpr ((PARTS & SET_SLOT) != 0) e.fit = &launch_fit2<T, M, R, W>;
    if constexpr ((PARTS & SET_GRAM) != 0) {
        static_assert(sizeof(T) == 4 && (PARTS & SET_SLOT) == 0, "the Gram fit is the fp32 set's only fit kernel");
        e.fit = &launch_fitg_entry<M>; e.gram_fit = 1;
    }
    if constexpr ((PARTS & SET_MRHS) != 0) {
        static_assert(W == 1, "the multi-RHS kernels are one-wave kernels");
        e.mrhs_factor = &launch_mrhs_factor<T, M, R>; e.mrhs_stream = &launch_mrhs_stream<T, M, R>;
        e.mrhs_lm = &launch_mrhs_lm<T, M, R>; e.mrhs_finish = &launch_mrhs_finish<T, M, R>;
        e.mrhs_state_bytes = mrhs_state_bytes<T, M>(); e.mrhs_gx_cap = mrhs_gx_cap<T, R>();
    }
    if constexpr ((PARTS & SET_LDS_W) != 0) e.fit_lds_w = fit_lds_bytes<T, M, R, W>(true);
    return e;
}
} // namespace vp

#define VP_CAT_(a, b) a##b
#define VP_CAT(a, b) VP_CAT_(a, b)
#define VP_REGISTER_SET(...) namespace vp { static Registrar VP_CAT(reg_, __COUNTER__)(__VA_ARGS__); }
#define VP_ME(NEXP, OFF) MultiExpModel<NEXP, (OFF) != 0>

#define VP_REGISTER_MULTIEXP(T, DT, NEXP, OFF, RR)                                                                     \
    VP_REGISTER_SET(resident_set<T, VP_ME(NEXP, OFF), RR, 1, SET_SINGLE | SET_SLOT | SET_MRHS>(DT, FAMILY_MULTIEXP, NEXP, OFF, 0))

#define VP_REGISTER_RT(T, DT, NN, QQ, PP, RR)                                                                          \
    VP_REGISTER_SET(resident_set<T, RtModel<NN, QQ, PP>, RR, 1, SET_SINGLE | SET_SLOT | SET_MRHS>(DT, FAMILY_RT, NN, QQ, PP))

// a set that only serves handles with several right-hand sides (S > 1): the MRHS kernels (+ basis / best_fit).  The
// single-RHS kernels of the triple exponential at 32 rows per lane spilled 400-940 VGPRs and were never selected
// (find_kernels hands single-RHS handles of that length the 4-wave set of 8 rows per lane)
#define VP_REGISTER_MULTIEXP_MRHS_ONLY(T, DT, NEXP, OFF, RR)                                                           \
    VP_REGISTER_SET(resident_set<T, VP_ME(NEXP, OFF), RR, 1, SET_MRHS>(DT, FAMILY_MULTIEXP, NEXP, OFF, 0))

// multi-wave groups (WW waves per problem): problems whose columns do not fit the registers of one wave
#define VP_REGISTER_MULTIEXP_W(T, DT, NEXP, OFF, RR, WW)                                                               \
    VP_REGISTER_SET(resident_set<T, VP_ME(NEXP, OFF), RR, WW, SET_SINGLE | SET_SLOT | SET_LDS_W>(DT, FAMILY_MULTIEXP, NEXP, OFF, 0))

// fp32, many columns x many rows: the FIT runs on the fp64 Gram matrix (vp_fitg.hpp: any grid, any weights; there is
// no fp32 Householder fit kernel for these shapes -- it lost 15 % of the fits and spilled 230-250 VGPRs);
// evaluate / basis / best_fit / statistics stay on the WW-wave Householder kernels
#define VP_REGISTER_MULTIEXP_W_GRAM(NEXP, OFF, RR, WW)                                                                 \
    VP_REGISTER_SET(resident_set<float, VP_ME(NEXP, OFF), RR, WW, SET_SINGLE | SET_GRAM>(VP_F32, FAMILY_MULTIEXP, NEXP, OFF, 0))

// run-time-descriptor models at larger m (WW waves per problem): single-RHS kernel set only, no slot kernel
#define VP_REGISTER_RT_W(T, DT, NN, QQ, PP, RR, WW)                                                                    \
    VP_REGISTER_SET(resident_set<T, RtModel<NN, QQ, PP>, RR, WW, SET_SINGLE | SET_LDS_W>(DT, FAMILY_RT, NN, QQ, PP))
