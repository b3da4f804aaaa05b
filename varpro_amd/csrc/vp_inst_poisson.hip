// the Poisson re-weighting kernel (vp_poisson.hpp): fp64 / fp32 x {16-byte groups, element-wise} x {Neyman, model}
#include "vp_poisson.hpp"

namespace vp {

int poisson_reweight_launch(const PoissonParams &p) {
    return p.dtype == VP_F64 ? poisson::launch<double>(p) : poisson::launch<float>(p);
}

} // namespace vp
