// generic fallback kernels (any descriptor, any m; vp_generic.hpp), f64 and f32
#include "vp_generic.hpp"
#include "vp_registry.hpp"

namespace vp {
template <typename T> static KernelEntry generic_set(int dtype) {
    KernelEntry e{};
    e.dtype = dtype; e.family = FAMILY_GENERIC; e.W = 1;
    e.evaluate = &gen::launch_evaluate<T>;
    e.basis = &gen::launch_basis<T>;
    e.fit_single = &gen::launch_fit<T>;
    e.best_fit = &gen::launch_best_fit<T>;
    e.mrhs_state_bytes = gen::mrhs_lm_state_bytes<T>();
    e.stats = &gen::launch_stats<T>;
    e.mrhs_fit_whole = &gen::launch_mrhs_fit<T>;
    e.uses_gen_ws = 1;
    return e;
}
const KernelEntry *generic_kernels(int dtype) {
    static const KernelEntry f64 = generic_set<double>(VP_F64), f32 = generic_set<float>(VP_F32);
    return dtype == VP_F64 ? &f64 : &f32;
}
} // namespace vp
