// the scan kernel of the IRF reconvolution kinds (vp_irf.hpp): fp64 / fp32 x {16-byte groups, element-wise} x {ordinary,
// non-temporal stores} x {unbounded, box bounds} x {zero start, periodic}
#include "vp_irf.hpp"

namespace vp {

int irf_cols_fill(const ColsParams &p) {
    return p.dtype == VP_F64 ? cols::launch_irf<double>(p) : cols::launch_irf<float>(p);
}

} // namespace vp
