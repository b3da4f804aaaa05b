// the fixed siblings of the column kernel and of the IRF scan kernel (vp_batch_create_fixed; vp_cols.hpp, vp_irf.hpp): derived
// from the bounded bodies only -- fp64 / fp32 x {16-byte groups, element-wise} x {ordinary, non-temporal stores}, the scan
// kernel also x {zero start, periodic}: 8 + 16 kernels.  A unit of its own: the older units' code objects stay as they are.
#define VP_INLINE_SINCOS 1
#include "vp_irf.hpp"

namespace vp {

int cols_fill_fixed(const ColsParams &p) {
    if (int rc = p.dtype == VP_F64 ? cols::launch_fill<double, true>(p) : cols::launch_fill<float, true>(p)) return rc;
    for (int j = 0; j < p.model.n_basis; ++j)
        if (is_irf_kind(p.model.kind[j])) return irf_cols_fill_fixed(p);
    return VP_ERR_OK;
}

int irf_cols_fill_fixed(const ColsParams &p) {
    return p.dtype == VP_F64 ? cols::launch_irf<double, true>(p) : cols::launch_irf<float, true>(p);
}

} // namespace vp
