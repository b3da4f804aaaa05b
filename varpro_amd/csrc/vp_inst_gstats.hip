// fit statistics of global fits (vp_gstats.hpp): model-agnostic, one set of kernels per dtype
#include "vp_gstats.hpp"

namespace vp {
int gstats_launch(const GStatsParams &p) {
    return p.dtype == VP_F64 ? gs::launch_gstats<double>(p) : gs::launch_gstats<float>(p);
}
} // namespace vp
