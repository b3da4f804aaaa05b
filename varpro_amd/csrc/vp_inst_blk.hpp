// vp_inst_blk.hpp -- registration of the LENGTH-AGNOSTIC kernel sets (vp_block.hpp): the set a single-RHS fit lands on when
// no register-resident set is long enough (capacity 2^26 rows: it loses against every resident set that covers m and wins
// where none does).  the trait-level evaluation streams as well (blk_evaluate_kernel); basis / best_fit / statistics / global fits run on the generic kernels.
#pragma once
#include "vp_block.hpp"
#include "vp_generic.hpp"
#include "vp_registry.hpp"

namespace vp {
namespace blk {
template <typename T, class M> int launch_evaluate_entry(const LaunchParams &p) {
    return launch_evaluate<T, M>(p, &::vp::gen::launch_evaluate<T>);
}
} // namespace blk
template <typename T, class M> KernelEntry blocked_set(int dtype, int family, int a, int b, int c) {
    KernelEntry e{};
    e.dtype = dtype; e.family = family; e.a = a; e.b = b; e.c = c; e.R = 1 << 20; e.W = 1;
    e.evaluate = &blk::launch_evaluate_entry<T, M>;
    e.basis = &gen::launch_basis<T>;
    e.fit_single = &blk::launch_fit<T, M>;
    if constexpr (fit_rescue_v<T, M>) e.fit_rescue = &blk::launch_fit_rescue<T, M>;
    e.best_fit = &gen::launch_best_fit<T>;
    e.mrhs_state_bytes = gen::mrhs_lm_state_bytes<T>();
    e.stats = &gen::launch_stats<T>;
    e.mrhs_fit_whole = &gen::launch_mrhs_fit<T>;
    e.uses_gen_ws = 1;
    return e;
}
} // namespace vp

#define VP_BLK_CAT_(a, b) a##b
#define VP_BLK_CAT(a, b) VP_BLK_CAT_(a, b)
#define VP_BLK_REGISTER(...) static ::vp::Registrar VP_BLK_CAT(vp_blk_reg_, __COUNTER__)(__VA_ARGS__);
#define VP_REGISTER_BLOCKED_MULTIEXP(T, DT, NEXP, OFF)                                                                 \
    VP_BLK_REGISTER(::vp::blocked_set<T, ::vp::MultiExpModel<NEXP, (OFF) != 0>>(DT, ::vp::FAMILY_MULTIEXP, NEXP, OFF, 0))
#define VP_REGISTER_BLOCKED_RT(T, DT, NN, QQ, PP)                                                                      \
    VP_BLK_REGISTER(::vp::blocked_set<T, ::vp::RtModel<NN, QQ, PP>>(DT, ::vp::FAMILY_RT, NN, QQ, PP))
