// the column kernel of device-column handles (vp_cols.hpp): fp64 / fp32 x {16-byte groups, element-wise} x {ordinary,
// non-temporal stores} x {unbounded, box bounds}, and the two map kernels of bounded fits.  The sin / cos of the two
// trigonometric kinds is inlined here (one small kernel per variant).
#define VP_INLINE_SINCOS 1
#include "vp_cols.hpp"

namespace vp {

int cols_fill(const ColsParams &p) {
    if (int rc = p.dtype == VP_F64 ? cols::launch_fill<double>(p) : cols::launch_fill<float>(p)) return rc;
    for (int j = 0; j < p.model.n_basis; ++j)
        if (is_irf_kind(p.model.kind[j])) return irf_cols_fill(p); // (their columns: the scan kernel, vp_inst_irf.hip)
    return VP_ERR_OK;
}

int bounds_transform(int dtype, void *x, const void *lo, const void *hi, int64_t bound_stride, int q, int64_t B, int to_internal,
                     hipStream_t stream) {
    return dtype == VP_F64 ? cols::launch_bounds_transform<double>(x, lo, hi, bound_stride, q, B, to_internal, stream)
                           : cols::launch_bounds_transform<float>(x, lo, hi, bound_stride, q, B, to_internal, stream);
}

} // namespace vp
