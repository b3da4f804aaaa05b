// the column kernel of device-column handles (vp_cols.hpp): fp64 / fp32 x {16-byte groups, element-wise} x {ordinary,
// non-temporal stores}.  The sin / cos of the two trigonometric kinds is inlined here (one small kernel per variant).
#define VP_INLINE_SINCOS 1
#include "vp_cols.hpp"

namespace vp {

int cols_fill(const ColsParams &p) {
    return p.dtype == VP_F64 ? cols::launch_fill<double>(p) : cols::launch_fill<float>(p);
}

} // namespace vp
