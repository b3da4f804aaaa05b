// the robust re-weighting kernel (vp_robust.hpp): fp64 / fp32 x {16-byte groups, element-wise} x {fixed scale, median of
// |e| with the keys in registers, median with the keys in the problem's row of w}
#include "vp_robust.hpp"

namespace vp {

int robust_reweight_launch(const RobustParams &p) {
    return p.dtype == VP_F64 ? robust::launch<double>(p) : robust::launch<float>(p);
}

} // namespace vp
