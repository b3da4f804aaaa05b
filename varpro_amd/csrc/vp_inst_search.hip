// the kernels of vp_search (vp_search.hpp): fp64 / fp32 x { orthonormalisation of the candidates' columns, the MFMA ranking
// kernel for n = 1 .. 8 x {16-byte, element-wise loads of Y_w} x {winner, score matrix}, the reduction of the score matrix
// over right-hand sides } and the two small kernels of the candidate loop.
#include "vp_search.hpp"

namespace vp {

namespace search {
// the running minimum of the candidate loop: a candidate counts when its evaluation is ok and its cost finite; strict
// "<" in ascending k keeps the lowest index among equal costs
__global__ void __launch_bounds__(256) loop_update_kernel(const double *__restrict__ cost, const int32_t *__restrict__ status,
                                                          const int k, const int64_t B, double *__restrict__ best,
                                                          int32_t *__restrict__ index) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    double bs = __builtin_inf();
    int bi = -1;
    if (k > 0) {
        bs = best[b];
        bi = index[b];
    }
    const double c = cost[b];
    if (status[b] == 0 && c - c == 0.0 && (bi < 0 || c < bs)) {
        bs = c;
        bi = k;
    }
    best[b] = bs;
    index[b] = bi;
}
} // namespace search

int search_orthonormalize(const SearchParams &p) {
    return p.dtype == VP_F64 ? search::launch_orthonormalize<double>(p) : search::launch_orthonormalize<float>(p);
}

int search_rank(const SearchParams &p) {
    return p.dtype == VP_F64 ? search::launch_rank<double>(p) : search::launch_rank<float>(p);
}

int search_gather(int dtype, const void *cand, int64_t K, int q, int per_problem, int64_t k, const int32_t *index, int64_t B,
                  void *alpha, hipStream_t stream) {
    return dtype == VP_F64 ? search::launch_gather<double>(cand, K, q, per_problem, k, index, B, alpha, stream)
                           : search::launch_gather<float>(cand, K, q, per_problem, k, index, B, alpha, stream);
}

int search_loop_update(const double *cost, const int32_t *status, int64_t k, int64_t B, double *best, int32_t *index,
                       hipStream_t stream) {
    if (B <= 0) return VP_ERR_OK;
    hipLaunchKernelGGL(search::loop_update_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, cost, status, (int)k, B,
                       best, index);
    return launch_status();
}

} // namespace vp
