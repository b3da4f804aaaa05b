// the resample kernel of the shifted IRF kinds (vp_irf_shift.hpp): fp64 / fp32.  A unit of its own, linked last: the older
// units' code objects stay as they are.
#include "vp_irf_shift.hpp"

namespace vp {

int irf_resample(const ColsParams &p, const int delta_param, const bool want_dg) {
    return p.dtype == VP_F64 ? cols::launch_resample<double>(p, delta_param, want_dg)
                             : cols::launch_resample<float>(p, delta_param, want_dg);
}

} // namespace vp
