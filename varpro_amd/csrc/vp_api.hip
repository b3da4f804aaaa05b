// vp_api.hip -- implementation of the C ABI declared in include/varpro_hip.h.
// Host-side state management + dispatch into the kernel registry.  No fallbacks: every compute
// entry point runs HIP kernels on a gfx950 device or returns an error.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/varpro_hip.h"
#include "../../include/varpro_hip_debug.h"
#include "vp_registry.hpp"
#include "vp_extfit_api.hpp"
#include "vp_mrhs.hpp"
#include "vp_gstats.hpp"
#include "vp_cols.hpp"
#include "vp_search.hpp"
#include "vp_poisson.hpp"
#include "vp_robust.hpp"

using namespace vp;

// global fit: identical consecutive fits (by their longest problem's evaluation count) before the captured graph drops its
// spare iteration (mrhs_fit)
#ifndef VP_MRHS_EXACT_AFTER
#define VP_MRHS_EXACT_AFTER 8
#endif

namespace {

thread_local std::string g_err;
thread_local int g_detail = 0;

int fail(int code, const std::string &msg, int detail = 0) {
    g_err = msg;
    g_detail = detail;
    return code;
}

#define VP_HIP(expr)                                                                                                  \
    do {                                                                                                              \
        hipError_t e__ = (expr);                                                                                      \
        if (e__ != hipSuccess)                                                                                        \
            return fail(VP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));                            \
    } while (0)

inline size_t tsize(int dtype) { return dtype == VP_F64 ? 8 : 4; }

// scoped device memory: every temporary of an entry point.  Freed at the end of its scope -- hipFree synchronises the
// device, so WHERE that scope ends relative to the work around it is part of an entry point's behaviour
struct DevMem {
    void *p = nullptr;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    int alloc(size_t bytes) {
        VP_HIP(hipMalloc(&p, bytes));
        return 0;
    }
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
};

// ---- small utility kernels (dtype-generic plumbing, not the hot path) ------------------------------
// (Y and Yw may be the same buffer -- vp_set_observations stages host data through Yw -- hence no __restrict__ on them:
// every element is read and written by the same thread)
template <typename T>
__global__ void weight_data_kernel(const T *Y, const T *__restrict__ w, T *Yw, int m, int64_t cols_per_problem,
                                   int64_t w_stride, int64_t total) {
    // Y_w = W * Y  (src/problem/builder.rs:307, src/util/mod.rs:86-95)
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t col = idx / m;
        const int i = (int)(idx - col * m);
        const int64_t b = col / cols_per_problem;
        Yw[idx] = w ? (T)(w[b * w_stride + i] * Y[idx]) : Y[idx];
    }
}

// per-problem reduction over the S right-hand sides: cost[b] = sum_s cost_bs ; status[b] = max_s status_bs
__global__ void reduce_rhs_kernel(const double *__restrict__ cost_bs, const int32_t *__restrict__ status_bs,
                                  double *__restrict__ cost_b, int32_t *__restrict__ status_b, int S, int64_t B) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    double acc = 0.0;
    int st = 0;
    // eight loads in flight per thread and trip (one dependent load per trip made this 24 us for S = 16384)
    for (int s0 = threadIdx.x; s0 < S; s0 += 8 * blockDim.x) {
        double c[8];
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = s0 + k * (int)blockDim.x;
            const bool in = s < S;
            c[k] = in ? cost_bs[b * S + s] : 0.0;
            v[k] = in ? status_bs[b * S + s] : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc += c[k];
            st = v[k] > st ? v[k] : st;
        }
    }
    __shared__ double sh[1024];
    __shared__ int shs[1024];
    sh[threadIdx.x] = acc;
    shs[threadIdx.x] = st;
    __syncthreads();
    for (int off = blockDim.x / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            sh[threadIdx.x] += sh[threadIdx.x + off];
            shs[threadIdx.x] = shs[threadIdx.x] > shs[threadIdx.x + off] ? shs[threadIdx.x] : shs[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (cost_b) cost_b[b] = sh[0];
        if (status_b) status_b[b] = shs[0];
    }
}

// {sum cost, #successful, #failed, sum n_evals} over the batch
__global__ void summary_kernel(const vp_report *__restrict__ rep, int64_t B, double *__restrict__ out4) {
    double c = 0, ok = 0, bad = 0, ev = 0;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
        const vp_report r = rep[b];
        if (r.objective == r.objective) c += r.objective;
        if (r.termination > 0) ok += 1.0;
        else bad += 1.0;
        ev += (double)r.n_evals;
    }
    __shared__ double sh[4][256];
    sh[0][threadIdx.x] = c;
    sh[1][threadIdx.x] = ok;
    sh[2][threadIdx.x] = bad;
    sh[3][threadIdx.x] = ev;
    __syncthreads();
    for (int off = blockDim.x / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) atomicAdd(&out4[k], sh[k][0]);
}

// Sum of the streaming kernel's per-workgroup partials in a fixed order: tot[b][i] = sum_g part[b][g][i].  Used
// when the right-hand sides are sharded over ranks: the totals are all-reduced (vp_set_rhs_allreduce) and the LM
// step then reads them as a single slot, so that every rank takes bit-identical decisions.
__global__ void mrhs_reduce_partials_kernel(const double *part, int gx, int nacc, int64_t B, double *tot) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= B * nacc) return;
    const int64_t b = idx / nacc;
    const int i = (int)(idx - b * nacc);
    double s = 0.0;
    for (int g = 0; g < gx; ++g) s += part[((size_t)b * nacc + i) * gx + g]; // [b][accumulator][workgroup]
    tot[idx] = s;
}

// Uniform-grid check, once per handle: grid g passes if every t_i lies within 4 ulp-of-the-offset of the lattice
// t_0 + i*dt, dt = (t_{m-1} - t_0)/(m-1):   |t_i - (t_0 + i dt)| <= 4 eps |t_i - t_0|.
// That is what a linspace-type grid anchored at its first sample satisfies, and it bounds the argument error of
// the recurrence exp(-(t_0 + i dt)/tau) to 4 eps (t_i - t_0)/|tau| -- the size of the reference's own rounding of
// the quotient t_i/tau.  Grids with a large offset (|t_0| >> m dt) or irregular sampling fail and keep the
// per-row exponential.  One block per grid; *flag is AND-ed.
template <typename T> __global__ void grid_check_kernel(const T *t, int m, int64_t ngrids, int *flag) {
    const int64_t g = blockIdx.x;
    if (g >= ngrids) return;
    const T *tg = t + g * (int64_t)m;
    const double t0 = (double)tg[0];
    const double dt = ((double)tg[m - 1] - t0) / (double)(m - 1);
    // to the rounding of the grid's own type: 4 ulp of the distance from t_0
    const double tol = 4.0 * (sizeof(T) == 8 ? 2.220446049250313e-16 : 1.1920928955078125e-07);
    bool ok = (dt == dt) && (dt - dt == 0.0) && dt != 0.0;
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
        const double lat = __builtin_fma((double)i, dt, t0);
        const double dev = __builtin_fabs((double)tg[i] - lat);
        if (!(dev <= tol * __builtin_fabs((double)tg[i] - t0))) ok = false;
    }
    if (!ok) atomicAnd(flag, 0);
}

} // namespace

// ---- the handle ------------------------------------------------------------------------------------
// The captured graphs of the global fit (mrhs_fit_specialised) and the policy that decides their length.  The whole fit
// is ONE graph (`head`: init, `len` iterations, finish); a fit that outlasts it continues with replays of `tail`
// (kTailIters further iterations + finish).  Both hold the LM options by value.
struct MrhsGraphs {
    static constexpr int kFirstIters = 12, kTailIters = 12, kMinIters = 6, kMaxIters = 24;
    hipGraphExec_t head = nullptr, tail = nullptr;
    hipStream_t cap_stream = nullptr; // capture happens on a private stream: the handle's may be the null stream
    vp_lm_opts opts = {};             // the options both graphs were captured with
    int len = 0;                      // LM iterations `head` holds
    int next_len = 0;                 // ... and what the next capture should hold (0: no fit yet)
    int prev_nfev = 0;                // largest evaluation count of the previous fit, and for how many fits in a row it has
    int same_count = 0;               // been the same: a stream of fits of one length runs a graph WITHOUT the spare iteration
    bool failed = false;              // a capture failed: plain launches for the rest of the handle's life

    bool opts_changed(const vp_lm_opts &o) const { return !head || std::memcmp(&opts, &o, sizeof(o)) != 0; }
    int wanted_len() const { return next_len > 0 ? next_len : kFirstIters; }
    // Re-capture with hysteresis: on streaming data the longest fit moves by +-1 evaluation from one call to the next, and a
    // capture + instantiation costs as much as the fit it speeds up.  The head is re-captured when the options changed, when
    // the wanted length EXCEEDS the captured one (every further iteration would cost a replay of the tail graph) or falls
    // short of it by 4 or more (each idle iteration is two empty launches, ~10 us); the tail graph does not depend on the
    // length and is only re-captured with the options.
    // (A handle whose last VP_MRHS_EXACT_AFTER + 1 fits took the same number of evaluations drops the spare iteration -- two
    // empty launches, ~10 us of a 0.7 ms fit: the wanted length is then exact and the head is re-captured ONCE, down to that
    // length.  The exact length only ever SHRINKS the graph: a stream whose longest fit moves by +-1 every few calls
    // (A A A B A A A B) never reaches the run length, and after a miss the spare-iteration rule decides alone -- no
    // recapture per fluctuation.)
    bool head_stale(const vp_lm_opts &o) const {
        const int want = wanted_len();
        const bool exact = same_count >= VP_MRHS_EXACT_AFTER;
        return opts_changed(o) || want > len || want + 4 <= len || (exact && want < len);
    }
    // after a graph fit whose longest problem took nfev_max evaluations: the next capture holds as many iterations, plus
    // one spare unless the run of equal fits is long enough
    void observe(int nfev_max) {
        same_count = (nfev_max == prev_nfev) ? same_count + 1 : 0;
        prev_nfev = nfev_max;
        const int want = nfev_max + (same_count >= VP_MRHS_EXACT_AFTER ? 0 : 1);
        next_len = want < kMinIters ? kMinIters : (want > kMaxIters ? kMaxIters : want);
    }
    void drop() {
        if (head) (void)hipGraphExecDestroy(head);
        if (tail) (void)hipGraphExecDestroy(tail);
        head = tail = nullptr;
    }
};

// (hidden: the members below are this file's business, the library exports the C functions only)
struct __attribute__((visibility("hidden"))) vp_batch {
    vp_model_desc model = {};
    int dtype = 0;
    int64_t m = 0, S = 0, B = 0;
    int n = 0, q = 0, p = 0;
    int flags = 0;
    int device = 0;
    double eps = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    const KernelEntry *kern = nullptr;
    // Every device / pinned allocation of the handle is made through alloc / ensure / alloc_pinned and recorded here;
    // vp_batch_destroy frees the lists.  The typed pointers below are views: two of them may name one allocation.
    std::vector<void *> owned_dev, owned_pinned;
    template <typename T> int alloc(T *&ptr, size_t bytes) {
        void *mem = nullptr;
        VP_HIP(hipMalloc(&mem, bytes));
        if (mem) owned_dev.push_back(mem);
        ptr = static_cast<T *>(mem);
        return 0;
    }
    // lazily allocated buffers: at the first call that needs them, kept for the handle's life
    template <typename T> int ensure(T *&ptr, size_t bytes) { return ptr ? 0 : alloc(ptr, bytes); }
    template <typename T> int alloc_pinned(T *&ptr, size_t bytes, unsigned hip_flags) {
        void *mem = nullptr;
        VP_HIP(hipHostMalloc(&mem, bytes, hip_flags));
        owned_pinned.push_back(mem);
        ptr = static_cast<T *>(mem);
        return 0;
    }
    // scratch whose size depends on a call's arguments (vp_search): grown on demand, the smaller block is released
    template <typename T> int grow(T *&ptr, size_t &cap, size_t bytes) {
        if (ptr && cap >= bytes) return 0;
        if (ptr) {
            for (size_t i = 0; i < owned_dev.size(); ++i)
                if (owned_dev[i] == (void *)ptr) {
                    owned_dev.erase(owned_dev.begin() + (std::ptrdiff_t)i);
                    break;
                }
            (void)hipFree(ptr);
            ptr = nullptr;
            cap = 0;
        }
        if (int rc = alloc(ptr, bytes ? bytes : 1)) return rc;
        cap = bytes;
        return 0;
    }
    // device state (== SeparableProblem + CachedCalculations for the whole batch)
    void *d_t = nullptr, *d_w = nullptr, *d_yw = nullptr;
    void *d_alpha = nullptr;          // [B][q]
    void *d_C = nullptr;              // [B][S][n]
    void *d_R = nullptr;              // [B][S][m]  lazily allocated residual cache
    double *d_cost_bs = nullptr;      // [B*S]
    int32_t *d_status_bs = nullptr;
    double *d_cost = nullptr;         // [B]   (the per-(b,s) arrays themselves when S == 1)
    int32_t *d_status = nullptr;      // [B]
    vp_report *d_report = nullptr;    // [B]
    double *d_sum4 = nullptr;
    bool grid_uniform = false; // every grid is t_0 + i*dt to rounding (grid_check_kernel): kernels may use the exp recurrence
    bool have_params = false;  // set_params/evaluate/fit has run
    bool r_valid = false;      // d_R matches d_alpha
    bool have_report = false;
    bool alpha_kept = false;   // vp_poisson_reweight: the evaluation is gone, d_alpha still holds the parameters (vp_params)
    void *d_pfit = nullptr;    // vp_poisson_reweight, model mode: [B][m] best fit the weights are formed from; at first use
    // timing
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms[3] = {-1.f, -1.f, -1.f};
    // multiple-right-hand-side path (S > 1): factor/stream/LM-step kernels + their workspace, and the captured graphs
    bool have_mrhs = false;
    MrhsWs mrhs = {};
    MrhsGraphs graphs;
    int32_t *h_nactive = nullptr;     // pinned, device-mapped: the active count as the graph's last kernel leaves it
    int32_t *h_nactive_dev = nullptr; // its device address
    MrhsIo *h_io = nullptr;           // pinned, device-mapped: the caller's arrays of the current vp_fit (device-pointer handles)
    MrhsIo *h_io_dev = nullptr;
    // S-sharded global fits (vp_set_rhs_allreduce)
    vp_allreduce_fn rhs_allreduce = nullptr;
    void *rhs_allreduce_user = nullptr;
    int64_t rhs_global = 0;        // right-hand sides of the whole problem
    double *d_mrhs_tot = nullptr;  // [B][1 + n*n + p] totals of the reduced sums (all-reduced across ranks); generic kernels: [B][2 + q*q + q]
    void *d_gen_lm = nullptr;      // generic kernels, sharded right-hand sides: [B] LM state between the phases
    int32_t *d_gen_nactive = nullptr;
    // single-RHS fit kernel selection (vp_set_fit_kernel) and the slot kernel's problem queue
    int fit_kernel = 0;
    int *d_queue = nullptr;
    int num_cus = 0;
    void *d_gen_ws = nullptr; // generic fallback kernels: gen_blocks workspace slots of (n + 1 + p + q) columns x m
    int gen_blocks = 0;
    int64_t m_user = 0; // != 0: the caller's row count m < n; the handle works on m = n rows, the extra ones with zero weight
    // caller-evaluated model (vp_batch_create_external): shape + dependency-pair table, and where the columns of the
    // current parameters live (the caller's device arrays, or this handle's staged copies on host-pointer handles)
    bool external = false;
    int ext_np = 0;
    int32_t ext_pb[VP_MAX_PAIRS] = {}, ext_pp[VP_MAX_PAIRS] = {};
    const void *ext_phi = nullptr, *ext_dphi = nullptr;
    void *ext_phi_own = nullptr, *ext_dphi_own = nullptr;
    // device-column handle (a descriptor with VP_BASIS_GAUSS / _LORENTZ / _LINEAR): `external` is set as well -- everything
    // downstream of the columns is the caller-evaluated path -- and the columns come from the column kernel (vp_cols.hpp),
    // which evaluates col_model on the handle's grid into the two owned buffers
    bool devcols = false;
    vp_model_desc col_model = {};
    void *col_phi = nullptr, *col_dphi = nullptr; // [B][n][rows], [B][p][rows]; allocated at first use
    int col_look = 8;    // vp_fit: the host reads the active count every col_look steps (vp_debug_set_column_fit; measured)
    int col_nt = 1;      // stores of the column kernel: 1 = non-temporal, 0 = ordinary (vp_debug_set_column_fit; measured)
    // box bounds of vp_fit (vp_set_bounds): the fit iterates on internal parameters u, alpha = g(u) (vp_cols.hpp bound_map)
    bool bounded = false;
    void *d_lo = nullptr, *d_hi = nullptr; // [q] or [B][q] of the handle's dtype, rounded INTO the box
    int64_t bound_stride = 0;              // 0: one box for all problems, q: per problem
    // IRF reconvolution kinds (vp_irf.hpp): the instrument response of vp_set_irf, copied into a buffer of the handle
    bool irf_kinds = false;  // col_model contains VP_BASIS_EXP_DECAY_IRF / VP_BASIS_IRF
    bool have_irf = false;   // vp_set_irf has been called
    void *d_irf = nullptr;   // [rows] or [B][rows] of the handle's dtype (sized for the per-problem form at the first call)
    int64_t irf_stride = 0;  // 0: one response for all problems, rows: per problem
    // VP_BASIS_EXP_DECAY_IRF_PERIODIC: the period of vp_set_irf_period (0: the record is one period) and, for a host grid,
    // the longest record m dt_b of the batch (< 0: a device grid, the caller's contract)
    bool irf_periodic = false;
    double irf_period = 0.0, irf_span_max = -1.0;
    // shifted IRF kinds (vp_irf_shift.hpp): the shifted response g and dg/ddelta of every problem, written by the resample
    // kernel in front of the scans; [B][irf_gs] each, irf_gs = rows rounded up to a 16-byte group; allocated at first use
    bool irf_shift = false;
    void *d_irf_g = nullptr, *d_irf_dg = nullptr;
    // fixed nonlinear parameters (vp_batch_create_fixed): the handle is the REDUCED model -- q, p, the pair table and d_alpha
    // are those of the free parameters in model order; col_model stays the full descriptor and only the column kernels'
    // fixed siblings (vp_cols.hpp, vp_irf.hpp) read the map and the values
    bool fixed = false;
    int q_full = 0;
    int32_t fix_src[VP_MAX_PARAMS] = {};   // full parameter k: its index in the free vector, < 0: fixed
    void *d_fix_values = nullptr;          // [q_full] or [B][q_full] of the handle's dtype (sized for the per-problem form)
    int64_t fix_stride = 0;                // 0: one set of values for all problems, q_full: per problem
    void *d_inf_lo = nullptr, *d_inf_hi = nullptr; // [q]: the infinite box the siblings run with where the fit has none
    // batched reverse-communication LM fit of a caller-evaluated model (vp_fit_begin / vp_fit_step_with_basis / vp_fit_end)
    void *d_xf_state = nullptr;      // [B] LM records of the step kernel
    void *d_xf_trial = nullptr;      // [B][q] trial points of the last step
    int32_t *d_xf_want = nullptr;    // [B] what every problem wants next
    void *d_xf_ctrial = nullptr;     // [B][S][n] coefficients of the trial point (S > 1: generic step)
    int32_t *d_xf_active = nullptr;  // [2][B] compacted indices of the still-active problems, written alternately by the LM kernel
    int64_t xf_known_active = 0;     // the last active count the host read (an upper bound of the current one)
    int32_t *d_xf_nactive = nullptr; // device counter of the last step
    int32_t *h_xf_nactive = nullptr; // pinned host copy
    bool xf_running = false;         // between vp_fit_begin and vp_fit_end
    bool xf_init = false;            // the next step is the first
    int xf_flags = 0;
    int64_t xf_steps = 0;
    vp_lm_opts xf_opts = {};
    // vp_search (vp_search.hpp): the candidates' columns, their orthonormal bases, the marks of non-finite candidates, the
    // winners, the score matrix (S > 1) and the candidate loop's running minimum
    void *d_srch_phi = nullptr, *d_srch_q = nullptr, *d_srch_scores = nullptr;
    int32_t *d_srch_bad = nullptr, *d_srch_index = nullptr;
    double *d_srch_best = nullptr;
    size_t srch_phi_cap = 0, srch_q_cap = 0, srch_scores_cap = 0, srch_bad_cap = 0;
    float srch_ms[4] = {-1.f, -1.f, -1.f, -1.f}; // vp_set_timing: the shared route's four stages of the last vp_search
    // flag-and-refit of single-RHS fits (vp_fit.hpp jac_not_finite; rescue_refit below)
    int32_t *d_rescue = nullptr; // [2 + B]: two ping-pong counters + the flagged problems of the running fit
    void *d_rescue_ws = nullptr; // kRescueBlocks workspace slots of the generic fit kernel
    int rescue_slot = 0;         // the counter the NEXT fit appends to
    int32_t last_fit[4] = {0, 0, 0, 0}; // vp_debug_last_fit: the record of the launcher that issued the last fit's launch
    int32_t last_global[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // vp_debug_last_global: the records of the global-fit launchers
    bool rescue_off = false;     // vp_debug_set_refit(h, 0): fits keep the kernels' own `Numerical`
};

namespace {

bool device_ptrs(const vp_batch *h) { return (h->flags & VP_FLAG_DEVICE_PTRS) != 0; }

// input staging: user pointer -> device pointer usable on h->stream
struct InBuf {
    const void *dptr = nullptr;
    DevMem tmp;
    int init(vp_batch *h, const void *user, size_t bytes) {
        if (!user) {
            dptr = nullptr;
            return 0;
        }
        if (device_ptrs(h)) {
            dptr = user;
            return 0;
        }
        if (int rc = tmp.alloc(bytes ? bytes : 1)) return rc;
        VP_HIP(hipMemcpyAsync(tmp.p, user, bytes, hipMemcpyHostToDevice, h->stream));
        dptr = tmp.p;
        return 0;
    }
};

// output staging: kernels write to dptr; finish() lands the bytes in the user's buffer
struct OutBuf {
    void *dptr = nullptr;
    DevMem tmp;
    void *user = nullptr;
    size_t bytes = 0;
    int init(vp_batch *h, void *user_, size_t bytes_) {
        user = user_;
        bytes = bytes_;
        if (!user) return 0;
        if (device_ptrs(h)) {
            dptr = user;
            return 0;
        }
        if (int rc = tmp.alloc(bytes ? bytes : 1)) return rc;
        dptr = tmp.p;
        return 0;
    }
    int finish(vp_batch *h) {
        if (tmp.p) {
            VP_HIP(hipMemcpyAsync(user, tmp.p, bytes, hipMemcpyDeviceToHost, h->stream));
            VP_HIP(hipStreamSynchronize(h->stream));
        }
        return 0;
    }
};

int copy_out(vp_batch *h, void *user, const void *dev, size_t bytes);
// ---- m < n (an underdetermined linear sub-problem; the reference's SVD solve accepts it, src/solvers/levmar/mod.rs:51-54)
// The handle then works on n rows: the caller's m rows plus n - m rows of zero weight (zero rows change neither the
// minimum-norm coefficients nor the residual nor any singular value > 0).  Everything with a row dimension that crosses the
// ABI is padded on the way in and stripped on the way out.
__global__ void strip_rows_kernel(const unsigned *__restrict__ src, unsigned *__restrict__ dst, int64_t blocks, int words_user,
                                  int words_pad) {
    const int64_t total = blocks * words_user;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t blk = i / words_user;
        dst[i] = src[blk * words_pad + (i - blk * words_user)];
    }
}

// the LM crate's answer when there are fewer residuals than nonlinear parameters: one evaluation at the initial point,
// then TerminationReason::WrongDimensions (vp_lm_core.hpp lm_after_eval, first evaluation)
__global__ void wrong_dimensions_report_kernel(const double *__restrict__ cost, const int32_t *__restrict__ status, int64_t B,
                                               vp_report *__restrict__ rep, double *__restrict__ trace, int trace_rows, int q,
                                               int dtype, const void *__restrict__ alpha) {
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= B) return;
    vp_report r;
    const bool ok = status[b] == 0;
    r.termination = ok ? VP_TERM_WRONG_DIMENSIONS : VP_TERM_USER;
    r.n_evals = 1;
    r.objective = ok ? cost[b] : 0.0 / 0.0;
    rep[b] = r;
    if (trace && trace_rows > 0) { // vp_fit_trace: row 0 = [alpha_0, ||r||, ratio = NaN, delta, par] of the one evaluation
        double *tr = trace + (size_t)b * trace_rows * (q + 4);
        for (int k = 0; k < q; ++k)
            tr[k] = dtype == VP_F64 ? ((const double *)alpha)[b * q + k] : (double)((const float *)alpha)[b * q + k];
        tr[q] = ok ? sqrt(2.0 * cost[b]) : 0.0 / 0.0;
        tr[q + 1] = 0.0 / 0.0;
        tr[q + 2] = 0.0;
        tr[q + 3] = 0.0;
    }
}

// `blocks` blocks of the handle's m rows in device memory -> the caller's array of `blocks` blocks of ITS m rows
int copy_out_rows(vp_batch *h, void *user, const void *dev, size_t blocks) {
    if (!user) return 0;
    const size_t ts = tsize(h->dtype);
    if (!h->m_user) return copy_out(h, user, dev, blocks * (size_t)h->m * ts);
    const size_t bytes = blocks * (size_t)h->m_user * ts;
    DevMem tmp; // host-pointer handles: the packed rows on their way to the caller's host array
    void *packed = user;
    if (!device_ptrs(h)) {
        if (int rc = tmp.alloc(bytes ? bytes : 1)) return rc;
        packed = tmp.p;
    }
    const int wu = (int)(h->m_user * ts / 4), wp = (int)(h->m * ts / 4);
    const int64_t total = (int64_t)blocks * wu;
    hipLaunchKernelGGL(strip_rows_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 65536)), dim3(256), 0, h->stream,
                       (const unsigned *)dev, (unsigned *)packed, (int64_t)blocks, wu, wp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !device_ptrs(h)) {
        e = hipMemcpyAsync(user, packed, bytes, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (e != hipSuccess) return fail(VP_ERR_HIP, std::string("copy_out_rows: ") + hipGetErrorString(e));
    return 0;
}

// an output with a row dimension: `blocks` blocks of m rows.  Not padded: OutBuf as is.  Padded: the kernels write a
// private array of padded blocks, finish() strips it into the caller's
struct RowOut {
    OutBuf buf;
    DevMem pad;
    void *user = nullptr;
    size_t blocks = 0;
    void *dptr = nullptr;
    int init(vp_batch *h, void *user_, size_t blocks_) {
        user = user_;
        blocks = blocks_;
        if (!h->m_user) {
            const int rc = buf.init(h, user_, blocks_ * (size_t)h->m * tsize(h->dtype));
            dptr = buf.dptr;
            return rc;
        }
        if (!user) return 0;
        if (int rc = pad.alloc(blocks * (size_t)h->m * tsize(h->dtype))) return rc;
        dptr = pad.p;
        return 0;
    }
    int finish(vp_batch *h) {
        if (!h->m_user) return buf.finish(h);
        if (!user) return 0;
        return copy_out_rows(h, user, pad.p, blocks);
    }
};

int copy_out(vp_batch *h, void *user, const void *dev, size_t bytes) {
    if (!user) return 0;
    if (device_ptrs(h)) {
        VP_HIP(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToDevice, h->stream));
    } else {
        VP_HIP(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream));
    }
    return 0;
}

void fill_params(vp_batch *h, LaunchParams &p) {
    std::memset(&p, 0, sizeof(p));
    p.model = &h->model;
    p.t = h->d_t;
    p.w = h->d_w;
    p.yw = h->d_yw;
    p.alpha = h->d_alpha;
    p.m = (int)h->m;
    p.S = (int)h->S;
    p.B = h->B;
    p.t_stride = (h->flags & VP_FLAG_T_PER_PROBLEM) ? h->m : 0;
    p.w_stride = (h->flags & VP_FLAG_W_PER_PROBLEM) ? h->m : 0;
    p.eps = h->eps;
    p.grid_uniform = h->grid_uniform ? 1 : 0;
    p.stream = h->stream;
    p.queue = h->d_queue;
    p.num_cus = h->num_cus;
    p.gen_ws = h->d_gen_ws;
    p.gen_blocks = h->gen_blocks;
    p.fit_group = h->fit_kernel;
    p.ext = h->external ? 1 : 0;
    p.ext_np = h->ext_np;
    p.ext_pb = h->ext_pb;
    p.ext_pp = h->ext_pp;
    p.ext_phi = h->ext_phi;
    p.ext_dphi = h->ext_dphi;
    p.ext_rows = (int)(h->m_user ? h->m_user : h->m);
    p.last_global = h->last_global;
}

// the launch record of one step of the running reverse-communication fit (everything but where the trial points go)
void fill_ext_params(vp_batch *h, ExtFitParams &p) {
    std::memset(&p, 0, sizeof(p));
    p.dtype = h->dtype;
    p.n = h->n;
    p.q = h->q;
    p.np = h->ext_np;
    p.m = h->m;
    p.B = h->B;
    p.phi = h->ext_phi;
    p.dphi = h->ext_dphi;
    p.w = h->d_w;
    p.yw = h->d_yw;
    p.w_stride = (h->flags & VP_FLAG_W_PER_PROBLEM) ? h->m : 0;
    p.state = h->d_xf_state;
    p.alpha0 = h->d_alpha;
    p.alpha_best = h->d_alpha;
    p.C_best = h->d_C;
    p.cost = h->d_cost;
    p.status = h->d_status;
    p.report = h->d_report;
    p.nactive = h->d_xf_nactive;
    p.step = (int)(h->xf_steps & 1);
    p.pb = h->ext_pb;
    p.pp = h->ext_pp;
    p.eps = h->eps;
    p.opts = h->xf_opts;
    p.init = h->xf_init ? 1 : 0;
    p.lazy = (h->xf_flags & VP_FIT_DERIVATIVES_ON_ACCEPT) ? 1 : 0;
    p.S = h->S;
    p.gen_ws = h->d_gen_ws;
    p.gen_blocks = h->gen_blocks;
    p.C_trial = h->d_xf_ctrial;
    p.active_lists = h->d_xf_active;
    p.known_active = h->xf_known_active;
    p.stream = h->stream;
}

struct Timer {
    vp_batch *h;
    int which;
    Timer(vp_batch *h_, int w) : h(h_), which(w) {
        if (h->timing) (void)hipEventRecord(h->ev0, h->stream);
    }
    void stop() {
        if (h->timing) {
            (void)hipEventRecord(h->ev1, h->stream);
            (void)hipEventSynchronize(h->ev1);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
            h->last_ms[which] = ms;
        }
    }
};

int reduce_rhs(vp_batch *h, hipStream_t stream_override = nullptr, bool use_override = false) {
    if (h->S == 1) return 0; // d_cost / d_status alias the per-(b,s) arrays
    hipLaunchKernelGGL(reduce_rhs_kernel, dim3((unsigned)h->B), dim3(h->S > 2048 ? 1024 : 256), 0, use_override ? stream_override : h->stream, h->d_cost_bs,
                       h->d_status_bs, h->d_cost, h->d_status, (int)h->S, h->B);
    VP_HIP(hipGetLastError());
    return 0;
}

// workspace of the generic kernels (vp_generic.hpp): one slot of (n + 1 + p + q) columns per persistent workgroup; at most
// 1024 workgroups (never more than `work_items`) and 4 GiB
size_t gen_slot_bytes(const vp_batch *h) { return (size_t)(h->n + 1 + h->p + h->q) * (size_t)h->m * tsize(h->dtype); }
int alloc_gen_ws(vp_batch *h, int64_t work_items) {
    if (h->d_gen_ws) return 0;
    const size_t slot = gen_slot_bytes(h);
    int64_t blocks = std::min<int64_t>(work_items, 1024);
    while (blocks > 1 && (size_t)blocks * slot > ((size_t)4 << 30)) blocks /= 2;
    h->gen_blocks = (int)blocks;
    return h->alloc(h->d_gen_ws, (size_t)blocks * slot);
}
int ensure_gen_ws(vp_batch *h) { return h->kern->uses_gen_ws ? alloc_gen_ws(h, h->B * h->S) : 0; }

int ensure_R(vp_batch *h) { return h->ensure(h->d_R, (size_t)h->B * h->S * h->m * tsize(h->dtype)); }

// ---- device-column handles: the column kernel (vp_cols.hpp) ------------------------------------------------------------
// rows of a column: the caller's m (a handle padded for m < n keeps the caller's rows in its columns, like ext_rows)
int64_t col_rows(const vp_batch *h) { return h->m_user ? h->m_user : h->m; }
// shifted IRF kinds: the row stride of the handle's g / g' buffers (whole 16-byte groups), and the buffers themselves
int64_t irf_shift_stride(const vp_batch *h) {
    const int64_t vw = (int64_t)(16 / tsize(h->dtype));
    return (col_rows(h) + vw - 1) / vw * vw;
}
int ensure_irf_shift(vp_batch *h) {
    if (!h->irf_shift) return 0;
    const size_t bytes = (size_t)h->B * (size_t)irf_shift_stride(h) * tsize(h->dtype);
    if (int rc = h->ensure(h->d_irf_g, bytes)) return rc;
    return h->ensure(h->d_irf_dg, bytes);
}
// the launch record of the handle's model on the handle's grid; outputs and the problem selection are the caller's
void fill_cols_params(const vp_batch *h, ColsParams &c) {
    std::memset(&c, 0, sizeof(c));
    c.dtype = h->dtype;
    c.model = h->col_model;
    c.t = h->d_t;
    c.t_stride = (h->flags & VP_FLAG_T_PER_PROBLEM) ? h->m : 0;
    c.m = (int)col_rows(h);
    c.B = h->B;
    c.irf = h->d_irf;
    c.irf_stride = h->irf_stride;
    c.irf_period = h->irf_period;
    c.irf_g = h->d_irf_g;
    c.irf_dg = h->d_irf_dg;
    c.irf_gs = irf_shift_stride(h);
    c.stream = h->stream;
    if (h->fixed) { // the fixed siblings: alpha over the free parameters, an infinite box unless the caller sets the fit's
        c.fix_src = h->fix_src;
        c.fix_values = h->d_fix_values;
        c.fix_stride = h->fix_stride;
        c.q_free = h->q;
        c.lo = h->d_inf_lo;
        c.hi = h->d_inf_hi;
        c.bound_stride = 0;
    }
}
// every column of the handle's descriptor: the column kernels, or their fixed siblings
int handle_cols_fill(const ColsParams &c) { return c.fix_src ? cols_fill_fixed(c) : cols_fill(c); }
// a handle with an IRF kind cannot evaluate a column before vp_set_irf
#define VP_NEEDS_IRF(h, what)                                                                                          \
    if ((h)->irf_kinds && !(h)->have_irf)                                                                              \
    return fail(VP_ERR_INVALID, what ": the model has an IRF reconvolution kind (VP_BASIS_EXP_DECAY_IRF[_PERIODIC] / VP_BASIS_IRF) " \
                                     "and the handle has no instrument response yet: call vp_set_irf first")
// Phi and dPhi of `alpha_dev` [B][q] into the handle's own buffers, which become the columns of the caller-evaluated path.
// list / count (device): only these problems, `bound` an upper bound of *count; null: all B
// `internal`: alpha_dev holds the internal parameters of a bounded fit (the bounded column kernel maps them)
int fill_own_columns(vp_batch *h, const void *alpha_dev, const int32_t *list, const int32_t *count, int64_t bound,
                     const bool internal = false) {
    VP_NEEDS_IRF(h, "column evaluation");
    const size_t ts = tsize(h->dtype), rows = (size_t)col_rows(h);
    if (int rc = h->ensure(h->col_phi, (size_t)h->B * h->n * rows * ts)) return rc;
    if (h->ext_np > 0)
        if (int rc = h->ensure(h->col_dphi, (size_t)h->B * h->ext_np * rows * ts)) return rc;
    if (int rc = ensure_irf_shift(h)) return rc;
    ColsParams c;
    fill_cols_params(h, c);
    c.alpha = alpha_dev;
    c.phi = h->col_phi;
    c.dphi = h->col_dphi;
    c.list = list;
    c.count = count;
    c.nt = h->col_nt == 1 ? 1 : 0;
    if (internal) {
        c.lo = h->d_lo;
        c.hi = h->d_hi;
        c.bound_stride = h->bound_stride;
    }
    if (list) c.B = bound;
    if (int rc = handle_cols_fill(c)) return fail(rc, "column kernel launch failed");
    h->ext_phi = h->col_phi;
    h->ext_dphi = h->col_dphi;
    return 0;
}

// ---- the steps several entry points share ---------------------------------------------------------------------------
// the caller's parameters (device or host array, by the handle's flags) -> d_alpha
int upload_alpha(vp_batch *h, const void *alpha) {
    VP_HIP(hipMemcpyAsync(h->d_alpha, alpha, (size_t)h->B * h->q * tsize(h->dtype),
                          device_ptrs(h) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return 0;
}

vp_lm_opts opts_or_default(const vp_batch *h, const vp_lm_opts *opts) {
    vp_lm_opts o;
    if (opts) o = *opts;
    else vp_lm_opts_default(&o, h->dtype);
    return o;
}

// the handle's state after a completed fit: parameters and report are the fit's, the residual cache is not
void after_fit(vp_batch *h) {
    h->have_params = true;
    h->r_valid = false;
    h->have_report = true;
}
// ... and after anything that invalidates the cached evaluation / fit
void invalidate(vp_batch *h) {
    h->have_params = false;
    h->r_valid = false;
    h->have_report = false;
    h->alpha_kept = false;
}

// a fit's results into the caller's arrays (each may be null)
int copy_fit_out(vp_batch *h, void *alpha_out, void *C_out, vp_report *rep) {
    const size_t ts = tsize(h->dtype);
    if (int rc = copy_out(h, alpha_out, h->d_alpha, (size_t)h->B * h->q * ts)) return rc;
    if (int rc = copy_out(h, C_out, h->d_C, (size_t)h->B * h->S * h->n * ts)) return rc;
    return copy_out(h, rep, h->d_report, (size_t)h->B * sizeof(vp_report));
}

// the trace of a vp_fit_trace call: [B][trace_rows][q + 4] doubles, NaN-filled (rows never written read as NaN).
// tr.dptr stays null when no trace is wanted
int trace_begin(vp_batch *h, OutBuf &tr, double *trace_out, int trace_rows) {
    if (!trace_out || trace_rows <= 0) return 0;
    const size_t bytes = (size_t)h->B * (size_t)trace_rows * (h->q + 4) * sizeof(double);
    if (int rc = tr.init(h, trace_out, bytes)) return rc;
    VP_HIP(hipMemsetAsync(tr.dptr, 0xFF, bytes, h->stream));
    return 0;
}
void set_trace(LaunchParams &p, const OutBuf &tr, int trace_rows) {
    if (!tr.dptr) return;
    p.trace = (double *)tr.dptr;
    p.trace_rows = trace_rows;
}

// Y_w = W * Y into d_yw (ysrc may be d_yw itself)
int launch_weight_data(vp_batch *h, const void *ysrc) {
    const int64_t total = h->B * h->S * h->m;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 65536);
    const int64_t wstride = (h->flags & VP_FLAG_W_PER_PROBLEM) ? h->m : 0;
    if (h->dtype == VP_F64)
        hipLaunchKernelGGL(weight_data_kernel<double>, dim3(grid), dim3(256), 0, h->stream, (const double *)ysrc,
                           (const double *)h->d_w, (double *)h->d_yw, (int)h->m, h->S, wstride, total);
    else
        hipLaunchKernelGGL(weight_data_kernel<float>, dim3(grid), dim3(256), 0, h->stream, (const float *)ysrc,
                           (const float *)h->d_w, (float *)h->d_yw, (int)h->m, h->S, wstride, total);
    VP_HIP(hipGetLastError());
    return 0;
}

// {sum cost, #successful, #failed, sum n_evals} of the last fit into four doubles of device memory
int launch_summary(vp_batch *h, double *dev_out4) {
    VP_HIP(hipMemsetAsync(dev_out4, 0, 4 * sizeof(double), h->stream));
    const unsigned grid = (unsigned)std::min<int64_t>((h->B + 255) / 256, 1024);
    hipLaunchKernelGGL(summary_kernel, dim3(grid), dim3(256), 0, h->stream, h->d_report, h->B, dev_out4);
    VP_HIP(hipGetLastError());
    return 0;
}

// the per-problem status a statistics kernel writes: straight into the caller's device array, else into a temporary that
// finish() copies to the caller's host array (no caller array: discarded)
struct StatusOut {
    DevMem tmp;
    int32_t *dev = nullptr;
    int init(vp_batch *h, int32_t *status) {
        dev = status && device_ptrs(h) ? status : nullptr;
        if (dev) return 0;
        if (int rc = tmp.alloc((size_t)h->B * sizeof(int32_t))) return rc;
        dev = (int32_t *)tmp.p;
        return 0;
    }
    int finish(vp_batch *h, int32_t *status) {
        if (!status || device_ptrs(h)) return 0;
        VP_HIP(hipMemcpyAsync(status, dev, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream));
        return 0;
    }
};

// ... and the handle's own four doubles into the caller's host array
int read_sum4(vp_batch *h, double out[4]) {
    VP_HIP(hipMemcpyAsync(out, h->d_sum4, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    VP_HIP(hipStreamSynchronize(h->stream));
    return VP_ERR_OK;
}

// run the evaluate kernel at h->d_alpha; any output may be null
int run_evaluate(vp_batch *h, void *r_dev, void *J_dev, void *C_dev) {
    if (h->external && !h->ext_phi)
        return fail(VP_ERR_INVALID, "the columns of the handle's current parameters are not known (after vp_fit_end: call "
                                    "vp_set_params_with_basis with Phi / dPhi at the fitted parameters first)");
    if (h->external && !h->d_gen_ws &&
        !external_resident(h->dtype, h->n, h->ext_np, h->m, h->m_user ? h->m_user : h->m, J_dev != nullptr))
        if (int rc = ensure_gen_ws(h)) return rc;
    LaunchParams p;
    fill_params(h, p);
    p.r_out = r_dev;
    p.J_out = J_dev;
    p.C_out = C_dev;
    p.cost_out = h->d_cost_bs;
    p.status = h->d_status_bs;
    Timer tm(h, VP_KERNEL_EVALUATE);
    int rc;
    if (h->have_mrhs) {
        // S > 1: factor Phi once per problem, then ONE streaming pass over the S data columns
        p.mrhs_ws = &h->mrhs;
        p.mrhs_mode = 1;
        rc = h->kern->mrhs_factor(p);
        if (rc == VP_ERR_OK) rc = h->kern->mrhs_stream(p);
    } else {
        rc = h->kern->evaluate(p);
    }
    tm.stop();
    if (rc != VP_ERR_OK) return fail(rc, "evaluate kernel launch failed");
    return reduce_rhs(h);
}

// Every entry point runs with the handle's device current and leaves the calling thread's current device as it found
// it (a process that drives several GPUs -- torch with another current device, say -- must not see it change).
struct DeviceGuard {
    int prev = -1;
    bool armed = false;
    int enter(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) {
            VP_HIP(hipSetDevice(device));
            armed = prev >= 0;
        }
        return 0;
    }
    ~DeviceGuard() {
        if (armed) (void)hipSetDevice(prev);
    }
};

#define VP_ENTER(h)                                                                                                   \
    if (!(h)) return fail(VP_ERR_INVALID, "null handle");                                                             \
    DeviceGuard dev_guard__;                                                                                          \
    if (int rc__ = dev_guard__.enter((h)->device)) return rc__

// ---- global fit (S > 1): == LevMarSolver::fit for problems with multiple right-hand sides -------------------------------
// Two kernel families.  The generic fallback runs the whole fit in one launch (mrhs_fit_generic).  The specialised
// {factor, streaming reduction over Y, LM step} set is enqueued iteration by iteration, normally as a captured graph
// (mrhs_fit_specialised); all LM state stays on the device, the host only looks at the number of still-active problems.
struct MrhsFit {
    vp_batch *h;
    vp_lm_opts o;
    LaunchParams p; // launches on the handle's stream; a capture works on a copy with its own stream
    // right-hand sides sharded over ranks: the reduced sums of this rank's columns are totalled in a fixed order, summed
    // over the ranks by the caller's collective (RCCL all-reduce of B*nacc doubles per evaluation) and fed to the LM step
    // as a single slot; every rank then takes bit-identical decisions
    int nacc = 0;
    MrhsWs ws_tot = {};
};

// generic fallback kernels: the whole global fit is one launch (vp_generic.hpp, gen_mrhs_fit_kernel), which also leaves
// the coefficients / cost / status of every column at the final point
int mrhs_fit_generic(MrhsFit &f) {
    vp_batch *h = f.h;
    LaunchParams &p = f.p;
    p.alpha_out = h->d_alpha;
    p.C_out = h->d_C;
    p.cost_out = h->d_cost_bs;
    p.status = h->d_status_bs;
    p.report = h->d_report;
    // right-hand sides sharded over ranks: the same kernel in phases -- init, then per evaluation {sums of this rank's
    // columns, the caller's all-reduce of B*(2 + q*q + q) doubles, LM step on the totals (every rank takes bit-identical
    // decisions)}, then the per-column results at the final point
    const int nacc = 2 + h->q * h->q + h->q;
    if (h->rhs_allreduce) {
        if (int rc = h->ensure(h->d_gen_lm, (size_t)h->B * h->kern->mrhs_state_bytes)) return rc;
        if (int rc = h->ensure(h->d_mrhs_tot, (size_t)h->B * nacc * sizeof(double))) return rc;
        if (int rc = h->ensure(h->d_gen_nactive, sizeof(int32_t))) return rc;
        VP_HIP(hipMemsetAsync(h->d_gen_nactive, 0, sizeof(int32_t), h->stream));
        p.gen_lm_state = h->d_gen_lm;
        p.gen_acc = h->d_mrhs_tot;
        p.gen_nactive = h->d_gen_nactive;
        p.mrhs_S_global = h->rhs_global;
    }
    Timer tm(h, VP_KERNEL_FIT);
    if (!h->rhs_allreduce) {
        if (int rc = h->kern->mrhs_fit_whole(p)) return fail(rc, "generic global-fit launch failed");
    } else {
        p.gen_phase = 1;
        if (int rc = h->kern->mrhs_fit_whole(p)) return fail(rc, "generic global-fit (init) launch failed");
        const int max_iter = f.o.patience * (h->q + 1) + 2;
        for (int it = 0; it < max_iter; ++it) {
            p.gen_phase = 2;
            if (int rc = h->kern->mrhs_fit_whole(p)) return fail(rc, "generic global-fit (sums) launch failed");
            if (h->rhs_allreduce(h->d_mrhs_tot, h->B * nacc, (void *)h->stream, h->rhs_allreduce_user) != 0)
                return fail(VP_ERR_INVALID, "the right-hand-side all-reduce callback reported an error");
            p.gen_phase = 3;
            if (int rc = h->kern->mrhs_fit_whole(p)) return fail(rc, "generic global-fit (step) launch failed");
            if ((it & 3) == 3 || it + 1 == max_iter) {
                int32_t nact = 0;
                VP_HIP(hipMemcpyAsync(&nact, h->d_gen_nactive, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
                VP_HIP(hipStreamSynchronize(h->stream));
                if (nact <= 0) break;
            }
        }
        p.gen_phase = 4;
        if (int rc = h->kern->mrhs_fit_whole(p)) return fail(rc, "generic global-fit (results) launch failed");
    }
    tm.stop();
    return reduce_rhs(h);
}

// the first launch: LM state from alpha0 (the active count is SET there, no memset) + factorisation of alpha0
int mrhs_enqueue_init(MrhsFit &f, LaunchParams &lp) {
    lp.mrhs_init = 1;
    lp.alpha = f.h->d_alpha;
    lp.mrhs_io = f.h->h_io_dev;
    const int rc = f.h->kern->mrhs_lm(lp);
    lp.mrhs_init = 0;
    return rc ? fail(rc, "mrhs_step (init) launch failed") : 0;
}
// one LM iteration = TWO launches: the streaming pass at the trial point, then the LM step on its sums fused with the
// factorisation of the next trial point (mrhs_step_kernel).  The loop is device-driven: iterations are ENQUEUED with
// no host synchronisation in between -- a problem whose LM loop has terminated is skipped on the device
// (MrhsWs::done), so an iteration enqueued past the end costs two empty launches (~10 us).
int mrhs_enqueue_iteration(MrhsFit &f, LaunchParams &lp) {
    vp_batch *h = f.h;
    lp.alpha = h->mrhs.alpha_trial;
    lp.mrhs_mode = 0;
    if (int rc = h->kern->mrhs_stream(lp)) return fail(rc, "mrhs_stream launch failed");
    if (h->rhs_allreduce) {
        const int64_t total = h->B * f.nacc;
        hipLaunchKernelGGL(mrhs_reduce_partials_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                           lp.stream, (const double *)h->mrhs.acc, mrhs_gx(h->S, h->kern->gx_cap()), f.nacc, h->B,
                           h->d_mrhs_tot);
        VP_HIP(hipGetLastError());
        if (h->rhs_allreduce(h->d_mrhs_tot, total, (void *)lp.stream, h->rhs_allreduce_user) != 0)
            return fail(VP_ERR_INVALID, "the right-hand-side all-reduce callback reported an error");
        lp.mrhs_ws = &f.ws_tot;
        lp.mrhs_fws = &h->mrhs;
        lp.mrhs_gx = 1;
    }
    // the LM step on the sums of this pass + the factorisation of the next trial point (one launch)
    if (int rc = h->kern->mrhs_lm(lp)) return fail(rc, "mrhs_step launch failed");
    lp.mrhs_ws = &h->mrhs;
    lp.mrhs_fws = nullptr;
    lp.mrhs_gx = 0;
    return 0;
}
// final parameters + reports; coefficients, cost and status of every column at the final point come from the best
// point's pass (double-buffered per-column results, MrhsWs::cbuf) -- no further pass over Y.  The m x S residual
// matrix is produced on demand by vp_residuals, as after a single-RHS fit.  The finish kernel also leaves the active
// count in pinned host memory (no copy kernel for the host's look at it).
int mrhs_enqueue_finish(MrhsFit &f, LaunchParams &lp) {
    vp_batch *h = f.h;
    lp.alpha_out = h->d_alpha;
    lp.report = h->d_report;
    lp.C_out = h->d_C;
    lp.cost_out = h->d_cost_bs;
    lp.status = h->d_status_bs;
    lp.mrhs_hflag = h->h_nactive_dev;
    lp.mrhs_io = h->h_io_dev;
    if (int rc = h->kern->mrhs_finish(lp)) return fail(rc, "mrhs_finish launch failed");
    return reduce_rhs(h, lp.stream, true); // per-problem cost / status from the per-column ones
}

// [init,] `iters` iterations, finish as ONE instantiated graph.  Captured on the handle's private stream and replayed on
// the handle's own
bool mrhs_capture(MrhsFit &f, hipGraphExec_t &exec, const bool head, const int iters) {
    MrhsGraphs &gr = f.h->graphs;
    bool ok = true;
    if (!gr.cap_stream) ok = hipStreamCreateWithFlags(&gr.cap_stream, hipStreamNonBlocking) == hipSuccess;
    hipGraph_t g = nullptr;
    if (ok) ok = hipStreamBeginCapture(gr.cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        LaunchParams gp = f.p;
        gp.stream = gr.cap_stream;
        if (head) ok = mrhs_enqueue_init(f, gp) == 0;
        for (int it = 0; it < iters && ok; ++it) ok = mrhs_enqueue_iteration(f, gp) == 0;
        if (ok) ok = mrhs_enqueue_finish(f, gp) == 0;
        const bool ended = hipStreamEndCapture(gr.cap_stream, &g) == hipSuccess;
        ok = ok && ended && g != nullptr;
    }
    if (ok) ok = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    if (!ok) {
        (void)hipGetLastError();
        exec = nullptr;
    }
    return ok;
}
// bring the handle's graphs up to date with this fit's options and the length its predecessor asks for (MrhsGraphs: the
// policy); a failed capture leaves none, and plain launches for the rest of the handle's life
void mrhs_update_graphs(MrhsFit &f) {
    MrhsGraphs &gr = f.h->graphs;
    if (!gr.head_stale(f.o)) return;
    const bool opts_changed = gr.opts_changed(f.o);
    const int want = gr.wanted_len();
    if (gr.head) (void)hipGraphExecDestroy(gr.head);
    gr.head = nullptr;
    bool ok = mrhs_capture(f, gr.head, true, want);
    if (ok && (opts_changed || !gr.tail)) {
        if (gr.tail) (void)hipGraphExecDestroy(gr.tail);
        gr.tail = nullptr;
        ok = mrhs_capture(f, gr.tail, false, MrhsGraphs::kTailIters);
    }
    if (ok) {
        gr.opts = f.o;
        gr.len = want;
    } else {
        gr.drop();
        gr.failed = true;
    }
}

// The specialised kernel set.  The WHOLE fit as ONE captured HIP graph: init, `len` iterations, finish (no trace, no
// all-reduce callback: both put host state into the launch sequence).  Its length follows the handle's previous fit:
// repeated fits of similar data -- the streaming use this path is built for -- enqueue almost no idle iterations, and a
// fit that needs more continues with further replays of the iteration-only tail graph.
int mrhs_fit_specialised(MrhsFit &f) {
    vp_batch *h = f.h;
    LaunchParams &p = f.p;
    MrhsGraphs &gr = h->graphs;
    Timer tm(h, VP_KERNEL_FIT);
    const int max_iter = f.o.patience * (h->q + 1) + 2;
    f.nacc = 1 + h->n * h->n + h->p;
    f.ws_tot = h->mrhs;
    if (h->rhs_allreduce) {
        if (int rc = h->ensure(h->d_mrhs_tot, (size_t)h->B * f.nacc * sizeof(double))) return rc;
        f.ws_tot.acc = h->d_mrhs_tot;
        p.mrhs_S_global = h->rhs_global;
    }
    const bool want_graph = !p.trace && !h->rhs_allreduce && !gr.failed;
    if (want_graph) mrhs_update_graphs(f);
    if (want_graph && gr.head) {
        VP_HIP(hipGraphLaunch(gr.head, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream));
        for (int it = gr.len; *(volatile int32_t *)h->h_nactive > 0 && it < max_iter; it += MrhsGraphs::kTailIters) {
            VP_HIP(hipGraphLaunch(gr.tail, h->stream));
            VP_HIP(hipStreamSynchronize(h->stream));
        }
        gr.observe(((volatile int32_t *)h->h_nactive)[1]);
    } else {
        if (int rc = mrhs_enqueue_init(f, p)) return rc;
        int next_check = 12;
        for (int it = 0; it < max_iter;) {
            if (int rc = mrhs_enqueue_iteration(f, p)) return rc;
            ++it;
            if (it < next_check && it < max_iter) continue;
            next_check += 24;
            int32_t nact = 0;
            VP_HIP(hipMemcpyAsync(&nact, h->mrhs.nactive, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            VP_HIP(hipStreamSynchronize(h->stream));
            if (nact <= 0) break;
        }
        if (int rc = mrhs_enqueue_finish(f, p)) return rc;
        // device-pointer handles: the finish / gather kernels read the caller's array addresses from the pinned MrhsIo record
        // at EXECUTION time and nothing below waits for them on this path (no copies: they write the results themselves) --
        // a following vp_fit would overwrite the record under them
        if (device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream));
    }
    tm.stop();
    return 0;
}

int mrhs_fit(vp_batch *h, const vp_lm_opts *opts, void *alpha_inout, void *C_out, vp_report *rep, double *trace_out,
             int trace_rows) {
    if (!h->have_mrhs && !h->kern->mrhs_fit_whole) return fail(VP_ERR_UNSUPPORTED, "no MRHS kernels for this (model, m)");
    MrhsFit f;
    f.h = h;
    f.o = opts_or_default(h, opts);
    // device-pointer handles with the MRHS kernel set: the kernels read the initial parameters from, and write the results
    // into, the CALLER's arrays through a pinned record of their addresses (MrhsIo) -- no staging copies around the fit
    const bool use_io = device_ptrs(h) && h->have_mrhs;
    if (!h->h_nactive) {
        if (int rc = h->alloc_pinned(h->h_nactive, 2 * sizeof(int32_t), hipHostMallocMapped)) return rc;
        VP_HIP(hipHostGetDevicePointer((void **)&h->h_nactive_dev, h->h_nactive, 0));
        if (int rc = h->alloc_pinned(h->h_io, sizeof(MrhsIo), hipHostMallocMapped)) return rc;
        VP_HIP(hipHostGetDevicePointer((void **)&h->h_io_dev, h->h_io, 0));
        std::memset(h->h_io, 0, sizeof(MrhsIo));
    }
    if (use_io) {
        h->h_io->alpha_in = alpha_inout;
        h->h_io->alpha_out = alpha_inout;
        h->h_io->C_out = C_out;
        h->h_io->rep_out = rep;
    } else {
        std::memset(h->h_io, 0, sizeof(MrhsIo));
        if (int rc = upload_alpha(h, alpha_inout)) return rc;
    }
    fill_params(h, f.p);
    f.p.mrhs_ws = &h->mrhs;
    f.p.opts = &f.o;
    OutBuf tr;
    if (int rc = trace_begin(h, tr, trace_out, trace_rows)) return rc;
    set_trace(f.p, tr, trace_rows);
    if (int rc = h->have_mrhs ? mrhs_fit_specialised(f) : mrhs_fit_generic(f)) return rc;
    after_fit(h);
    if (!use_io)
        if (int rc = copy_fit_out(h, alpha_inout, C_out, rep)) return rc;
    return tr.finish(h);
}

// pad the row dimension of `blocks` blocks from m to mp rows with `fill` (host arrays of 4- or 8-byte elements)
void pad_rows_host(const void *src, void *dst, size_t blocks, int64_t m, int64_t mp, size_t ts, double fill) {
    for (size_t blk = 0; blk < blocks; ++blk) {
        std::memcpy((char *)dst + blk * mp * ts, (const char *)src + blk * m * ts, (size_t)m * ts);
        for (int64_t i = m; i < mp; ++i) {
            if (ts == 8) ((double *)dst)[blk * mp + i] = fill;
            else ((float *)dst)[blk * mp + i] = (float)fill;
        }
    }
}

// ---- m < n: the caller's arrays as host arrays of mp rows per block (tiny problems by construction: padded on the host).
// Grid: the last sample repeated; data: zeros; weights: zeros -- with unit weights on the caller's rows when it passed
// none and `unit_w` asks for them.  An absent array (t of a caller-evaluated model; t and w of vp_set_observations) is
// skipped.  Device arrays are read on `st`, with one synchronisation after the last of them.
struct PaddedInputs {
    std::vector<char> t, y, w;
};
int pad_inputs_host(PaddedInputs &out, bool on_device, hipStream_t st, size_t ts, int64_t m, int64_t mp, const void *t,
                    size_t t_blocks, const void *Y, size_t y_blocks, const void *w, size_t w_blocks, bool unit_w) {
    std::vector<char> th(t ? t_blocks * m * ts : 0), yh(y_blocks * m * ts), wh(w || unit_w ? w_blocks * m * ts : 0);
    const void *src[3] = {t, Y, w};
    std::vector<char> *host[3] = {&th, &yh, &wh};
    for (int k = 0; k < 3; ++k) {
        if (!src[k]) continue;
        if (on_device) VP_HIP(hipMemcpyAsync(host[k]->data(), src[k], host[k]->size(), hipMemcpyDeviceToHost, st));
        else std::memcpy(host[k]->data(), src[k], host[k]->size());
    }
    if (on_device) VP_HIP(hipStreamSynchronize(st));
    if (t) {
        out.t = std::vector<char>(t_blocks * mp * ts);
        for (size_t blk = 0; blk < t_blocks; ++blk) {
            const double last = ts == 8 ? ((const double *)th.data())[blk * m + m - 1] : (double)((const float *)th.data())[blk * m + m - 1];
            pad_rows_host(th.data() + blk * m * ts, out.t.data() + blk * mp * ts, 1, m, mp, ts, last);
        }
    }
    out.y = std::vector<char>(y_blocks * mp * ts);
    pad_rows_host(yh.data(), out.y.data(), y_blocks, m, mp, ts, 0.0);
    if (!wh.empty()) {
        if (!w)
            for (size_t i = 0; i < w_blocks * (size_t)m; ++i) {
                if (ts == 8) ((double *)wh.data())[i] = 1.0;
                else ((float *)wh.data())[i] = 1.0f;
            }
        out.w = std::vector<char>(w_blocks * mp * ts);
        pad_rows_host(wh.data(), out.w.data(), w_blocks, m, mp, ts, 0.0);
    }
    return 0;
}

} // namespace

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" {

const char *vp_last_error(void) { return g_err.c_str(); }
int vp_last_error_detail(void) { return g_detail; }
const char *vp_version(void) { return "varpro_hip 0.1.0 (gfx950)"; }

int vp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

void vp_lm_opts_default(vp_lm_opts *o, int dtype) {
    const double eps = dtype == VP_F32 ? (double)FLT_EPSILON : DBL_EPSILON;
    o->ftol = 30.0 * eps;
    o->xtol = 30.0 * eps;
    o->gtol = 30.0 * eps;
    o->stepbound = 100.0;
    o->patience = 100;
    o->scale_diag = 1;
}

// a caller-evaluated model: dependency pairs (basis, parameter) in the caller's order
struct ExtSpec {
    int np;
    const int32_t *pb, *pp;
};
// vp_batch_create_fixed: the mask over the descriptor's parameters (validated by the entry point)
struct FixSpec {
    const int32_t *fixed;
};
static int batch_create_impl(vp_batch **out, const vp_model_desc *model, int dtype, int64_t m, int64_t S, int64_t B,
                             const void *t, const void *Y, const void *w, double svd_epsilon, int flags, int device,
                             void *hip_stream, bool data_on_device, const ExtSpec *ext, const FixSpec *fix);

// both create entry points.  m < n: the reference solves the underdetermined linear sub-problem by its truncated SVD
// (minimum-norm coefficients, src/solvers/levmar/mod.rs:51-54).  Here: n - m extra rows of ZERO weight (grid value = the
// last sample, data 0) -- they change neither the minimum-norm solution, nor the residual, nor a non-zero singular value --
// and the handle strips them from every array that crosses the ABI (m_user).  A caller-evaluated model's Phi / dPhi keep
// THEIR m rows (LaunchParams::ext_rows), the kernels read the missing rows as zeros.
static int batch_create(vp_batch **out, const vp_model_desc *model, int dtype, int64_t m, int64_t S, int64_t B, const void *t,
                        const void *Y, const void *w, double svd_epsilon, int flags, int device, void *hip_stream,
                        const ExtSpec *ext, const FixSpec *fix = nullptr) {
    const bool dev_data = (flags & VP_FLAG_DEVICE_PTRS) != 0;
    double irf_span_max = -1.0; // a host grid: the longest record m dt_b (vp_set_irf_period checks the period against it)
    if (model && !ext && model->n_basis > 0 && model->n_basis <= VP_MAX_BASIS && m == 1)
        for (int j = 0; j < model->n_basis; ++j)
            if (model->kind[j] == VP_BASIS_EXP_DECAY_IRF_PERIODIC)
                return fail(VP_ERR_INVALID, "VP_BASIS_EXP_DECAY_IRF_PERIODIC needs m >= 2: one sample has dt = 0, the periodic sum "
                                            "diverges");
            else if (is_irf_shift_kind(model->kind[j]))
                return fail(VP_ERR_INVALID, "the shifted IRF kinds (VP_BASIS_EXP_DECAY_IRF_SHIFT / VP_BASIS_IRF_SHIFT / "
                                            "VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT) need m >= 2: one sample has dt = 0, the shift "
                                            "in bins is undefined");
    // one response, one shift: every function of a shifted kind names the same delta, nothing else depends on it
    if (model && !ext && model->n_basis > 0 && model->n_basis <= VP_MAX_BASIS) {
        const int delta = irf_shift_param(*model);
        for (int j = 0; delta >= 0 && j < model->n_basis; ++j) {
            const int kind = model->kind[j];
            const int own = !is_irf_shift_kind(kind) ? -1 : (kind == VP_BASIS_IRF_SHIFT ? 0 : 1); // the argument that is delta
            for (int k = 0; k < VP_MAX_BASIS_PARAMS; ++k)
                if (k == own ? model->param[j][k] != delta : model->param[j][k] == delta)
                    return fail(VP_ERR_INVALID, "the shifted IRF kinds: all functions of VP_BASIS_EXP_DECAY_IRF_SHIFT / VP_BASIS_IRF_SHIFT "
                                                "/ VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT must name the same shift parameter, and no "
                                                "other function or argument may be that parameter");
        }
    }
    // the IRF reconvolution kinds need a uniform grid; a host grid is checked here (a device grid is the caller's contract)
    if (model && !ext && t && !dev_data && m > 0 && B > 0 && (dtype == VP_F64 || dtype == VP_F32) && model->n_basis > 0 &&
        model->n_basis <= VP_MAX_BASIS) {
        bool irf = false;
        for (int j = 0; j < model->n_basis; ++j) irf = irf || is_irf_kind(model->kind[j]);
        const int64_t ngrids = (flags & VP_FLAG_T_PER_PROBLEM) ? B : 1;
        for (int64_t g = 0; irf && g < ngrids; ++g) {
            auto at = [&](int64_t i) {
                return dtype == VP_F64 ? ((const double *)t)[g * m + i] : (double)((const float *)t)[g * m + i];
            };
            const double t0 = at(0), dt = m > 1 ? (at(m - 1) - t0) / (double)(m - 1) : 0.0;
            for (int64_t i = 0; i < m; ++i)
                if (!(std::fabs(at(i) - t0 - (double)i * dt) <= 1e-6 * std::fabs(dt)) && m > 1)
                    return fail(VP_ERR_INVALID, "the IRF reconvolution kinds (VP_BASIS_EXP_DECAY_IRF / VP_BASIS_IRF) need a uniform "
                                                "grid: |t_i - t_0 - i dt| <= 1e-6 |dt| with dt = (t[m-1] - t[0]) / (m-1)");
            irf_span_max = std::max(irf_span_max, (double)m * dt);
        }
    }
    // (arguments batch_create_impl refuses go to it as they are, for its message)
    if (!out || !model || !Y || (!t && !ext) || m <= 0 || S <= 0 || B <= 0 || (dtype != VP_F64 && dtype != VP_F32) ||
        m >= model->n_basis || model->n_basis > VP_MAX_BASIS) {
        const int rc = batch_create_impl(out, model, dtype, m, S, B, t, Y, w, svd_epsilon, flags, device, hip_stream, dev_data, ext, fix);
        if (rc == VP_ERR_OK && out && *out) (*out)->irf_span_max = irf_span_max;
        return rc;
    }
    PaddedInputs pad;
    DeviceGuard guard;
    hipStream_t st = nullptr;
    if (dev_data) {
        if (vp_device_count() <= 0) return fail(VP_ERR_NO_DEVICE, "no HIP device visible");
        if (int rc = guard.enter(device)) return rc;
        st = (flags & VP_FLAG_OWN_STREAM) ? nullptr : (hipStream_t)hip_stream;
    }
    const size_t tb = (flags & VP_FLAG_T_PER_PROBLEM) ? (size_t)B : 1, wb = (flags & VP_FLAG_W_PER_PROBLEM) ? (size_t)B : 1;
    if (int rc = pad_inputs_host(pad, dev_data, st, tsize(dtype), m, model->n_basis, t, tb, Y, (size_t)B * S, w, wb, true))
        return rc;
    const int rc = batch_create_impl(out, model, dtype, model->n_basis, S, B, t ? pad.t.data() : nullptr, pad.y.data(),
                                     pad.w.data(), svd_epsilon, flags, device, hip_stream, false, ext, fix);
    if (rc == VP_ERR_OK) {
        (*out)->m_user = m;
        (*out)->irf_span_max = irf_span_max;
    }
    return rc;
}

int vp_batch_create(vp_batch **out, const vp_model_desc *model, int dtype, int64_t m, int64_t S, int64_t B,
                    const void *t, const void *Y, const void *w, double svd_epsilon, int flags, int device,
                    void *hip_stream) {
    return batch_create(out, model, dtype, m, S, B, t, Y, w, svd_epsilon, flags, device, hip_stream, nullptr);
}

// ---- fixed nonlinear parameters (vp_batch_create_fixed / vp_set_fixed_values) ----------------------------------------------
namespace {
// the caller's doubles into the handle's dtype, one thread per entry
__global__ void __launch_bounds__(256) fixed_values_kernel(const double *__restrict__ src, void *__restrict__ dst, const int dtype,
                                                           const int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (dtype == VP_F64) static_cast<double *>(dst)[i] = src[i];
    else static_cast<float *>(dst)[i] = (float)src[i];
}
// values [q_full] or [B][q_full] (host or device doubles, by the handle's flags) -> d_fix_values, on the handle's stream
int store_fixed_values(vp_batch *h, const double *values, const int per_problem) {
    bool any_fixed = false;
    for (int k = 0; k < h->q_full; ++k) any_fixed = any_fixed || h->fix_src[k] < 0;
    if (!any_fixed) return VP_ERR_OK; // (nothing reads them)
    if (!values) return fail(VP_ERR_INVALID, "fixed parameters need their values: null values");
    const int64_t total = (per_problem ? h->B : 1) * (int64_t)h->q_full;
    InBuf v;
    if (int rc = v.init(h, values, (size_t)total * sizeof(double))) return rc;
    hipLaunchKernelGGL(fixed_values_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, (const double *)v.dptr,
                       h->d_fix_values, h->dtype, total);
    VP_HIP(hipGetLastError());
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream)); // (the staging buffer goes out of scope)
    h->fix_stride = per_problem ? h->q_full : 0;
    return VP_ERR_OK;
}
} // namespace

int vp_batch_create_fixed(vp_batch **out, const vp_model_desc *model, int dtype, int64_t m, int64_t S, int64_t B, const void *t,
                          const void *Y, const void *w, double svd_epsilon, int flags, int device, void *hip_stream,
                          const int32_t *fixed, const double *values, int per_problem) {
    if (!out) return fail(VP_ERR_INVALID, "null output handle");
    *out = nullptr;
    if (!model) return fail(VP_ERR_INVALID, "null model");
    if (model->n_basis <= 0 || model->n_basis > VP_MAX_BASIS || model->n_params < 0 || model->n_params > VP_MAX_PARAMS)
        return fail(VP_ERR_INVALID, "model sizes out of range");
    for (int j = 0; j < model->n_basis; ++j)
        if (model->kind[j] == VP_BASIS_EXTERNAL)
            return fail(VP_ERR_UNSUPPORTED, "vp_batch_create_fixed: a caller-evaluated model (VP_BASIS_EXTERNAL) fixes its "
                                            "parameters in the caller's own evaluation");
    if (!fixed) return fail(VP_ERR_INVALID, "vp_batch_create_fixed: null mask");
    int n_fixed = 0;
    for (int k = 0; k < model->n_params; ++k) {
        if (fixed[k] != 0 && fixed[k] != 1) return fail(VP_ERR_INVALID, "vp_batch_create_fixed: a mask entry is 0 (free) or 1 (fixed)");
        n_fixed += fixed[k];
    }
    // (a descriptor without nonlinear parameters and its empty mask: an all-zero mask like any other)
    if (n_fixed > 0 && n_fixed == model->n_params) return fail(VP_ERR_INVALID, "vp_batch_create_fixed: no free parameter left");
    if (n_fixed > 0 && !values) return fail(VP_ERR_INVALID, "vp_batch_create_fixed: fixed parameters need their values: null values");
    const FixSpec fix{fixed};
    if (int rc = batch_create(out, model, dtype, m, S, B, t, Y, w, svd_epsilon, flags, device, hip_stream, nullptr, &fix)) return rc;
    vp_batch *h = *out;
    auto setup = [&]() -> int {
        DeviceGuard guard;
        if (int rc = guard.enter(h->device)) return rc;
        const size_t ts = tsize(h->dtype);
        if (int rc = h->alloc(h->d_fix_values, std::max<size_t>((size_t)h->B * h->q_full, 1) * ts)) return rc;
        // the infinite box: the identity of bound_map
        if (int rc = h->alloc(h->d_inf_lo, std::max<size_t>((size_t)h->q, 1) * ts)) return rc;
        if (int rc = h->alloc(h->d_inf_hi, std::max<size_t>((size_t)h->q, 1) * ts)) return rc;
        double lo64[VP_MAX_PARAMS], hi64[VP_MAX_PARAMS];
        float lo32[VP_MAX_PARAMS], hi32[VP_MAX_PARAMS];
        for (int k = 0; k < VP_MAX_PARAMS; ++k) {
            lo64[k] = -INFINITY, hi64[k] = INFINITY;
            lo32[k] = -INFINITY, hi32[k] = INFINITY;
        }
        const bool f64 = h->dtype == VP_F64;
        VP_HIP(hipMemcpyAsync(h->d_inf_lo, f64 ? (const void *)lo64 : (const void *)lo32, (size_t)h->q * ts, hipMemcpyHostToDevice, h->stream));
        VP_HIP(hipMemcpyAsync(h->d_inf_hi, f64 ? (const void *)hi64 : (const void *)hi32, (size_t)h->q * ts, hipMemcpyHostToDevice, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream)); // (the staging arrays go out of scope)
        return store_fixed_values(h, values, per_problem);
    };
    if (int rc = setup()) {
        vp_batch_destroy(h);
        *out = nullptr;
        return rc;
    }
    return VP_ERR_OK;
}

int vp_set_fixed_values(vp_batch *h, const double *values, int per_problem) {
    VP_ENTER(h);
    if (!h->fixed)
        return fail(VP_ERR_UNSUPPORTED, "vp_set_fixed_values: the handle was not created by vp_batch_create_fixed (the mask is part "
                                        "of the handle's shape)");
    // (defensive: vp_fit_begin is refused on device-column handles, which every fixed handle is, so no public call gets here)
    if (h->xf_running) return fail(VP_ERR_INVALID, "vp_set_fixed_values during a stepped fit");
    if (int rc = store_fixed_values(h, values, per_problem)) return rc;
    // the cached evaluation / fit and the handle's columns belong to the old values
    invalidate(h);
    h->ext_phi = nullptr;
    h->ext_dphi = nullptr;
    return VP_ERR_OK;
}

// == SeparableProblemBuilder::build (src/problem/builder.rs:278-324) for a model the caller evaluates: any
// SeparableNonlinearModel (src/model/mod.rs:239-363), known here by its shape and dependency-pair table only
int vp_batch_create_external(vp_batch **out, int32_t n_basis, int32_t n_params, int32_t n_pairs, const int32_t *pair_basis,
                             const int32_t *pair_param, int dtype, int64_t m, int64_t S, int64_t B, const void *Y,
                             const void *w, double svd_epsilon, int flags, int device, void *hip_stream) {
    if (!out) return fail(VP_ERR_INVALID, "null output handle");
    *out = nullptr;
    if (n_basis <= 0 || n_basis > VP_MAX_BASIS || n_params < 0 || n_params > VP_MAX_PARAMS)
        return fail(VP_ERR_INVALID, "model sizes out of range");
    if (n_pairs < 0 || n_pairs > VP_MAX_PAIRS || (n_pairs > 0 && (!pair_basis || !pair_param)))
        return fail(VP_ERR_INVALID, "too many dependency pairs (or a null pair table)");
    for (int i = 0; i < n_pairs; ++i) {
        if (pair_basis[i] < 0 || pair_basis[i] >= n_basis || pair_param[i] < 0 || pair_param[i] >= n_params)
            return fail(VP_ERR_INVALID, "dependency pair out of range");
        for (int k = 0; k < i; ++k)
            if (pair_basis[k] == pair_basis[i] && pair_param[k] == pair_param[i])
                return fail(VP_ERR_INVALID, "dependency pair listed twice");
    }
    if (flags & VP_FLAG_T_PER_PROBLEM) return fail(VP_ERR_INVALID, "a caller-evaluated model has no grid");
    vp_model_desc md;
    std::memset(&md, 0, sizeof(md));
    md.n_basis = n_basis;
    md.n_params = n_params;
    for (int j = 0; j < VP_MAX_BASIS; ++j) {
        md.kind[j] = j < n_basis ? VP_BASIS_EXTERNAL : 0;
        for (int a = 0; a < VP_MAX_BASIS_PARAMS; ++a) md.param[j][a] = -1;
    }
    const ExtSpec ext{n_pairs, pair_basis, pair_param};
    return batch_create(out, &md, dtype, m, S, B, nullptr, Y, w, svd_epsilon, flags, device, hip_stream, &ext);
}

// the handle's buffers, data and kernel-side state; on an error the caller destroys the handle
static int batch_init(vp_batch *h, const void *t, const void *Y, const void *w, void *hip_stream, const bool data_on_device) {
    const int flags = h->flags;
    const int64_t m = h->m, S = h->S, B = h->B;
    if (!(flags & VP_FLAG_OWN_STREAM)) {
        h->stream = (hipStream_t)hip_stream; // NULL == the null stream (PyTorch's default stream)
    } else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(VP_ERR_HIP, "hipStreamCreate failed");
        h->own_stream = true;
    }
    const size_t ts = tsize(h->dtype);
    const size_t t_elems = (size_t)((flags & VP_FLAG_T_PER_PROBLEM) ? B * m : m);
    const size_t w_elems = (size_t)((flags & VP_FLAG_W_PER_PROBLEM) ? B * m : m);
    const size_t y_elems = (size_t)B * S * m;
    const hipMemcpyKind kin = data_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (t) { // (a caller-evaluated model has no grid)
        if (int rc = h->alloc(h->d_t, t_elems * ts)) return rc;
        VP_HIP(hipMemcpyAsync(h->d_t, t, t_elems * ts, kin, h->stream));
    }
    if (w) {
        if (int rc = h->alloc(h->d_w, w_elems * ts)) return rc;
        VP_HIP(hipMemcpyAsync(h->d_w, w, w_elems * ts, kin, h->stream));
    }
    {
        // the two temporaries of create: freed (the staged data first) once the stream has drained
        DevMem gflag_mem, ytmp;
        int *d_gflag = nullptr;
        // (fp32 handles: only the Gram fit kernel, vp_fitg.hpp, uses the flag -- the other fp32 kernels have no recurrence)
        const bool try_uniform = t && m >= 3 && !(flags & VP_FLAG_NO_GRID_RECURRENCE);
        if (try_uniform) {
            const int one = 1;
            if (int rc = gflag_mem.alloc(sizeof(int))) return rc;
            d_gflag = (int *)gflag_mem.p;
            VP_HIP(hipMemcpyAsync(d_gflag, &one, sizeof(int), hipMemcpyHostToDevice, h->stream));
            const int64_t ngrids = (flags & VP_FLAG_T_PER_PROBLEM) ? B : 1;
            if (h->dtype == VP_F64)
                hipLaunchKernelGGL(grid_check_kernel<double>, dim3((unsigned)ngrids), dim3(256), 0, h->stream,
                                   (const double *)h->d_t, (int)m, ngrids, d_gflag);
            else
                hipLaunchKernelGGL(grid_check_kernel<float>, dim3((unsigned)ngrids), dim3(256), 0, h->stream,
                                   (const float *)h->d_t, (int)m, ngrids, d_gflag);
            VP_HIP(hipGetLastError());
        }
        if (int rc = h->alloc(h->d_yw, y_elems * ts)) return rc;
        // Y_w = W * Y
        const void *ysrc = Y;
        if (!data_on_device) {
            if (int rc = ytmp.alloc(y_elems * ts)) return rc;
            VP_HIP(hipMemcpyAsync(ytmp.p, Y, y_elems * ts, hipMemcpyHostToDevice, h->stream));
            ysrc = ytmp.p;
        }
        if (int rc = launch_weight_data(h, ysrc)) return rc;
        int gflag = 0;
        if (d_gflag) VP_HIP(hipMemcpyAsync(&gflag, d_gflag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream));
        h->grid_uniform = gflag != 0;
    }
    if (int rc = h->alloc(h->d_alpha, (size_t)std::max<int64_t>(1, B * h->q) * ts)) return rc;
    if (int rc = h->alloc(h->d_C, (size_t)B * S * h->n * ts)) return rc;
    if (int rc = h->alloc(h->d_cost_bs, (size_t)B * S * sizeof(double))) return rc;
    if (int rc = h->alloc(h->d_status_bs, (size_t)B * S * sizeof(int32_t))) return rc;
    if (S == 1) { // one column per problem: the per-problem arrays ARE the per-column ones (reduce_rhs has nothing to do)
        h->d_cost = h->d_cost_bs;
        h->d_status = h->d_status_bs;
    } else {
        if (int rc = h->alloc(h->d_cost, (size_t)B * sizeof(double))) return rc;
        if (int rc = h->alloc(h->d_status, (size_t)B * sizeof(int32_t))) return rc;
    }
    if (int rc = h->alloc(h->d_report, (size_t)B * sizeof(vp_report))) return rc;
    if (int rc = h->alloc(h->d_sum4, 4 * sizeof(double))) return rc;
    if (int rc = h->alloc(h->d_queue, sizeof(int))) return rc;
    // (caller-evaluated models allocate the generic workspace on first use: their resident kernels -- vp_ext.hpp -- need none)
    if (!h->external)
        if (int rc = ensure_gen_ws(h)) return rc;
    VP_HIP(hipEventCreate(&h->ev0));
    VP_HIP(hipEventCreate(&h->ev1));
    if (S > 1 && has_mrhs_set(h->kern)) {
        const int n_ = h->n, p_ = h->p, q_ = h->q;
        MrhsWs &ws = h->mrhs;
        if (int rc = h->alloc(ws.qthin, (size_t)B * n_ * m * ts)) return rc;
        if (int rc = h->alloc(ws.g, (size_t)B * std::max(1, p_) * m * ts)) return rc;
        if (int rc = h->alloc(ws.small, (size_t)B * mrhs_small_stride_rt(n_, p_) * sizeof(double))) return rc;
        if (int rc = h->alloc(ws.statusA, (size_t)B * sizeof(int32_t))) return rc;
        // partial-sum slots of the MODE 0 pass (the only writer): gx is fixed per handle -- min(ceil(S/8), the kernel set's
        // cap) -- not the upper bound VP_MRHS_GX_MAX (B = 70000, S = 2 needs 1 slot per problem, not 512)
        const int gx_acc = mrhs_gx(S, h->kern->gx_cap());
        if (gx_acc > VP_MRHS_GX_MAX) return fail(VP_ERR_INVALID, "internal: partial-sum slots per problem exceed VP_MRHS_GX_MAX");
        if (int rc = h->alloc(ws.acc, (size_t)B * gx_acc * (1 + n_ * n_ + p_) * sizeof(double))) return rc;
        if (int rc = h->alloc(ws.lm_state, (size_t)B * h->kern->mrhs_state_bytes)) return rc;
        if (int rc = h->alloc(ws.nactive, 2 * sizeof(int32_t))) return rc;
        if (int rc = h->alloc(ws.done, (size_t)B * sizeof(int32_t))) return rc;
        VP_HIP(hipMemsetAsync(ws.done, 0, (size_t)B * sizeof(int32_t), h->stream));
        if (int rc = h->alloc(ws.alpha_trial, (size_t)std::max<int64_t>(1, B * q_) * ts)) return rc;
        for (int i = 0; i < 2; ++i) {
            if (int rc = h->alloc(ws.cbuf[i], (size_t)B * S * n_ * ts)) return rc;
            if (int rc = h->alloc(ws.costbuf[i], (size_t)B * S * sizeof(double))) return rc;
            if (int rc = h->alloc(ws.stbuf[i], (size_t)B * S * sizeof(int32_t))) return rc;
        }
        if (int rc = h->alloc(ws.widx, (size_t)B * sizeof(int32_t))) return rc;
        if (int rc = h->alloc(ws.bidx, (size_t)B * sizeof(int32_t))) return rc;
        if (int rc = h->alloc(ws.jcond, (size_t)B * sizeof(double))) return rc;
        VP_HIP(hipMemsetAsync(ws.jcond, 0, (size_t)B * sizeof(double), h->stream));
        h->have_mrhs = true;
    }
    return VP_ERR_OK;
}

static int batch_create_impl(vp_batch **out, const vp_model_desc *model, int dtype, int64_t m, int64_t S, int64_t B,
                             const void *t, const void *Y, const void *w, double svd_epsilon, int flags, int device,
                             void *hip_stream, const bool data_on_device, const ExtSpec *ext, const FixSpec *fix) {
    if (!out) return fail(VP_ERR_INVALID, "null output handle");
    *out = nullptr;
    if (!model) return fail(VP_ERR_INVALID, "null model");
    if (dtype != VP_F64 && dtype != VP_F32) return fail(VP_ERR_INVALID, "bad dtype");
    // builder validation (src/problem/builder.rs:278-302)
    if (!Y) return fail(VP_ERR_INVALID, "Right hand side(s) not provided", VP_BUILD_Y_DATA_MISSING);
    if (m <= 0 || S <= 0 || B <= 0 || (!t && !ext))
        return fail(VP_ERR_INVALID, "x or y must have nonzero number of elements.", VP_BUILD_ZERO_LENGTH_VECTOR);
    if (model->n_basis <= 0 || model->n_basis > VP_MAX_BASIS || model->n_params < 0 ||
        model->n_params > VP_MAX_PARAMS)
        return fail(VP_ERR_INVALID, "model sizes out of range");
    int fa, fb, fc, npairs;
    if (ext) npairs = ext->np; // caller-evaluated model: shape and pair table only, nothing to classify
    else if (classify_model(*model, fa, fb, fc, npairs) < 0) return fail(VP_ERR_INVALID, "malformed model descriptor");
    if (npairs > VP_MAX_PAIRS) return fail(VP_ERR_INVALID, "too many dependency pairs");
    // a descriptor with a peak / baseline kind: a device-column handle -- the state vp_batch_create_external builds (shape +
    // the descriptor's pairs in model order) plus the grid and the descriptor for the column kernel
    bool devcols = false;
    if (!ext)
        for (int j = 0; j < model->n_basis; ++j)
            if (model->kind[j] == VP_BASIS_GAUSS || model->kind[j] == VP_BASIS_LORENTZ || model->kind[j] == VP_BASIS_LINEAR ||
                is_irf_kind(model->kind[j]))
                devcols = true;
    if (!ext && (flags & VP_FLAG_DEVICE_COLUMNS)) devcols = true; // ... or any descriptor, on request (the kernel evaluates all kinds)
    if (!ext && fix) devcols = true;                              // ... or with fixed parameters (vp_batch_create_fixed)
    // fixed parameters: the inner shape is the reduced model -- the free parameters in model order and their pairs
    int32_t fix_src[VP_MAX_PARAMS];
    int q_free = 0;
    for (int k = 0; k < VP_MAX_PARAMS; ++k) fix_src[k] = -1;
    for (int k = 0; k < model->n_params; ++k) fix_src[k] = (fix && fix->fixed[k]) ? -1 : q_free++;
    vp_model_desc shape_desc;
    int32_t dc_pb[VP_MAX_PAIRS], dc_pp[VP_MAX_PAIRS];
    ExtSpec dc_ext{0, dc_pb, dc_pp};
    const vp_model_desc *const descriptor = model;
    if (devcols) {
        for (int j = 0; j < model->n_basis; ++j)
            for (int k = 0; k < VP_MAX_BASIS_PARAMS; ++k)
                if (model->param[j][k] >= 0 && fix_src[model->param[j][k]] >= 0) {
                    dc_pb[dc_ext.np] = j;
                    dc_pp[dc_ext.np] = fix_src[model->param[j][k]];
                    ++dc_ext.np;
                }
        npairs = dc_ext.np;
        std::memset(&shape_desc, 0, sizeof(shape_desc)); // (as vp_batch_create_external describes a caller-evaluated model)
        shape_desc.n_basis = model->n_basis;
        shape_desc.n_params = q_free;
        for (int j = 0; j < VP_MAX_BASIS; ++j) {
            shape_desc.kind[j] = j < model->n_basis ? VP_BASIS_EXTERNAL : 0;
            for (int a = 0; a < VP_MAX_BASIS_PARAMS; ++a) shape_desc.param[j][a] = -1;
        }
        model = &shape_desc;
        ext = &dc_ext;
    }

    int ndev = vp_device_count();
    if (ndev <= 0) return fail(VP_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(VP_ERR_INVALID, "bad device index");
    DeviceGuard dev_guard__;
    if (int rc__ = dev_guard__.enter(device)) return rc__;
    hipDeviceProp_t prop;
    VP_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(VP_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");

    // a specialised (register-resident) kernel set if one is instantiated for this (dtype, model, m), else the generic
    // fallback kernels (vp_generic.hpp): any descriptor, any m -- slower, but never a CPU path and never "unsupported"
    const KernelEntry *kern = ext ? external_kernels(dtype) : find_kernels(dtype, *model, m, S, w != nullptr);
    if (!ext && (flags & VP_FLAG_STREAM_ROWS)) { // only the length-agnostic sets (capacity 2^26 rows) pass this length
        const KernelEntry *ks = find_kernels(dtype, *model, (int64_t)1 << 24, S, w != nullptr);
        if (ks) kern = ks;
    }
    if (!kern) kern = generic_kernels(dtype);
    // a global fit (S > 1) on a specialised set WITHOUT multiple-right-hand-side kernels (the multi-wave sets: double
    // exponential at 2048 < m <= 4096, the fp32 Gram shape) runs on the generic kernels as well
    if (!ext && S > 1 && !has_mrhs_set(kern) && !kern->mrhs_fit_whole) kern = generic_kernels(dtype);

    vp_batch *h = new vp_batch();
    h->model = *model;
    h->dtype = dtype;
    h->m = m;
    h->S = S;
    h->B = B;
    h->n = model->n_basis;
    h->q = model->n_params;
    h->p = npairs;
    h->flags = flags;
    h->device = device;
    h->num_cus = prop.multiProcessorCount;
    const double meps = dtype == VP_F32 ? (double)FLT_EPSILON : DBL_EPSILON;
    h->eps = svd_epsilon < 0 ? meps : std::fabs(svd_epsilon); // src/problem/builder.rs:246-251, 282
    h->kern = kern;
    if (ext) {
        h->external = true;
        h->ext_np = ext->np;
        for (int i = 0; i < ext->np; ++i) {
            h->ext_pb[i] = ext->pb[i];
            h->ext_pp[i] = ext->pp[i];
        }
    }
    if (devcols) {
        h->devcols = true;
        h->col_model = *descriptor;
        for (int j = 0; j < descriptor->n_basis; ++j)
            if (is_irf_kind(descriptor->kind[j])) h->irf_kinds = true;
        for (int j = 0; j < descriptor->n_basis; ++j)
            if (descriptor->kind[j] == VP_BASIS_EXP_DECAY_IRF_PERIODIC || descriptor->kind[j] == VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT)
                h->irf_periodic = true;
        h->irf_shift = irf_shift_param(*descriptor) >= 0;
        if (fix) {
            h->fixed = true;
            h->q_full = descriptor->n_params;
            for (int k = 0; k < VP_MAX_PARAMS; ++k) h->fix_src[k] = fix_src[k];
        }
    }
    if (int rc = batch_init(h, t, Y, w, hip_stream, data_on_device)) {
        vp_batch_destroy(h);
        return rc;
    }
    *out = h;
    return VP_ERR_OK;
}

void vp_batch_destroy(vp_batch *h) {
    if (!h) return;
    DeviceGuard dev_guard__;
    (void)dev_guard__.enter(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (void *mem : h->owned_dev) (void)hipFree(mem);
    for (void *mem : h->owned_pinned) (void)hipHostFree(mem);
    h->graphs.drop();
    if (h->graphs.cap_stream) (void)hipStreamDestroy(h->graphs.cap_stream);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// ---- caller-evaluated models (vp_batch_create_external) -----------------------------------------------------------
#define VP_NOT_EXTERNAL(h, what)                                                                                       \
    if ((h)->external && !(h)->devcols)                                                                                \
    return fail(VP_ERR_UNSUPPORTED, what ": the handle's model is evaluated by the caller (vp_set_params_with_basis / "   \
                                         "vp_evaluate_with_basis)")
// ... and the entries of caller-evaluated handles on a device-column handle
#define VP_NOT_DEVCOLS(h, what)                                                                                        \
    if ((h)->devcols)                                                                                                  \
    return fail(VP_ERR_UNSUPPORTED, what ": the handle's model is a descriptor the device evaluates (vp_set_params / "    \
                                         "vp_evaluate / vp_fit); only handles made by vp_batch_create_external take the "  \
                                         "caller's columns")

// where the kernels find the columns of the current parameters: the caller's device arrays, or staged copies of host arrays
static int ext_stage(vp_batch *h, const void *user, int64_t cols, const void *&dev, void *&own) {
    if (!user) {
        dev = nullptr;
        return 0;
    }
    if (device_ptrs(h)) {
        dev = user;
        return 0;
    }
    const size_t bytes = (size_t)h->B * (size_t)cols * (size_t)(h->m_user ? h->m_user : h->m) * tsize(h->dtype);
    if (int rc = h->ensure(own, bytes ? bytes : 1)) return rc;
    VP_HIP(hipMemcpyAsync(own, user, bytes, hipMemcpyHostToDevice, h->stream));
    dev = own;
    return 0;
}

static int copy_status(vp_batch *h, int32_t *status);

// everything of one evaluation at d_alpha into the caller's arrays (each may be null): vp_evaluate, vp_evaluate_with_basis
static int evaluate_at_alpha(vp_batch *h, void *r_out, void *J_out, void *C_out, double *cost_out, int32_t *status) {
    RowOut r, J;
    if (int rc = r.init(h, r_out, (size_t)h->B * h->S)) return rc;
    if (int rc = J.init(h, J_out, (size_t)h->B * h->q * h->S)) return rc;
    if (int rc = run_evaluate(h, r.dptr, J.dptr, h->d_C)) return rc;
    h->have_params = true;
    h->r_valid = false;
    if (int rc = r.finish(h)) return rc;
    if (int rc = J.finish(h)) return rc;
    if (int rc = copy_out(h, C_out, h->d_C, (size_t)h->B * h->S * h->n * tsize(h->dtype))) return rc;
    if (int rc = copy_out(h, cost_out, h->d_cost, (size_t)h->B * sizeof(double))) return rc;
    return copy_status(h, status);
}
// the residual cache and the coefficients at d_alpha: vp_set_params, vp_set_params_with_basis
static int cache_at_alpha(vp_batch *h) {
    if (int rc = ensure_R(h)) return rc;
    if (int rc = run_evaluate(h, h->d_R, nullptr, h->d_C)) return rc;
    h->have_params = true;
    h->r_valid = true;
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream)); // the caller may reuse its host arrays
    return VP_ERR_OK;
}

int vp_set_params_with_basis(vp_batch *h, const void *alpha, const void *Phi, const void *dPhi) {
    VP_ENTER(h);
    VP_NOT_DEVCOLS(h, "vp_set_params_with_basis");
    if (!h->external) return fail(VP_ERR_UNSUPPORTED, "vp_set_params_with_basis needs a handle made by vp_batch_create_external");
    if (!alpha || !Phi) return fail(VP_ERR_INVALID, "null alpha / Phi");
    if (int rc = upload_alpha(h, alpha)) return rc;
    if (int rc = ext_stage(h, Phi, h->n, h->ext_phi, h->ext_phi_own)) return rc;
    if (int rc = ext_stage(h, dPhi, h->ext_np, h->ext_dphi, h->ext_dphi_own)) return rc;
    return cache_at_alpha(h);
}

int vp_jacobian_with_derivatives(vp_batch *h, const void *dPhi, void *J_out, int32_t *status) {
    VP_ENTER(h);
    VP_NOT_DEVCOLS(h, "vp_jacobian_with_derivatives");
    if (!h->external) return fail(VP_ERR_UNSUPPORTED, "vp_jacobian_with_derivatives needs a handle made by vp_batch_create_external");
    if (!h->have_params) return copy_status(h, status) ? VP_ERR_HIP : VP_ERR_OK; // jacobian() before set_params(): None
    if (!dPhi && h->ext_np > 0) return fail(VP_ERR_INVALID, "null dPhi");
    if (int rc = ext_stage(h, dPhi, h->ext_np, h->ext_dphi, h->ext_dphi_own)) return rc;
    return vp_jacobian(h, J_out, status);
}

int vp_evaluate_with_basis(vp_batch *h, const void *alpha, const void *Phi, const void *dPhi, void *r_out, void *J_out,
                           void *C_out, double *cost_out, int32_t *status) {
    VP_ENTER(h);
    VP_NOT_DEVCOLS(h, "vp_evaluate_with_basis");
    if (!h->external) return fail(VP_ERR_UNSUPPORTED, "vp_evaluate_with_basis needs a handle made by vp_batch_create_external");
    if (!alpha || !Phi) return fail(VP_ERR_INVALID, "null alpha / Phi");
    if (J_out && !dPhi && h->ext_np > 0) return fail(VP_ERR_INVALID, "a Jacobian needs the derivative columns dPhi");
    if (int rc = upload_alpha(h, alpha)) return rc;
    if (int rc = ext_stage(h, Phi, h->n, h->ext_phi, h->ext_phi_own)) return rc;
    if (int rc = ext_stage(h, dPhi, h->ext_np, h->ext_dphi, h->ext_dphi_own)) return rc;
    if (int rc = evaluate_at_alpha(h, r_out, J_out, C_out, cost_out, status)) return rc;
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream));
    return VP_ERR_OK;
}

// ---- batched LM fit of a caller-evaluated model by reverse communication (vp_extfit.hpp) --------------------------
// == LevMarSolver::fit (src/solvers/levmar/mod.rs:238-254) over the trait surface (src/model/mod.rs:239-363)
static int xf_begin(vp_batch *h, const vp_lm_opts *opts, const void *alpha0, int flags);

int vp_fit_begin(vp_batch *h, const vp_lm_opts *opts, const void *alpha0, int flags) {
    VP_ENTER(h);
    VP_NOT_DEVCOLS(h, "vp_fit_begin");
    if (!h->external)
        return fail(VP_ERR_UNSUPPORTED, "vp_fit_begin needs a handle made by vp_batch_create_external (descriptor models: vp_fit)");
    return xf_begin(h, opts, alpha0, flags);
}

// (also the start of a device-column handle's vp_fit)
static int xf_begin(vp_batch *h, const vp_lm_opts *opts, const void *alpha0, int flags) {
    if (!alpha0) return fail(VP_ERR_INVALID, "null alpha0");
    if (flags & ~VP_FIT_DERIVATIVES_ON_ACCEPT) return fail(VP_ERR_INVALID, "unknown vp_fit_begin flag");
    if (h->q <= 0) return fail(VP_ERR_INVALID, "a fit needs at least one nonlinear parameter");
    if (h->m_user)
        return fail(VP_ERR_UNSUPPORTED, h->devcols ? "vp_fit of a model with VP_BASIS_GAUSS / _LORENTZ / _LINEAR needs m >= n (fewer "
                                                     "samples than basis functions: vp_evaluate and the trait-level calls work)"
                                                   : "the batched fit of caller-evaluated models needs m >= n");
    const size_t rec = external_fit_rec_bytes(h->dtype, h->n, h->ext_np, h->q, h->m);
    if (!rec) return fail(VP_ERR_UNSUPPORTED, "no LM step kernel for this number of parameters");
    const size_t ts = tsize(h->dtype);
    if (external_fit_generic(h->dtype, h->n, h->ext_np, h->q, h->m, h->S)) {
        // shapes outside the specialised tables / several right-hand sides: the generic step and its workspace
        if (int rc = alloc_gen_ws(h, h->B)) return rc; // (h->p == h->ext_np: one workspace slot per problem in flight)
        if (h->S > 1)
            if (int rc = h->ensure(h->d_xf_ctrial, (size_t)h->B * h->S * h->n * ts)) return rc;
    }
    // (each buffer guarded on its own: an allocation that fails half way leaves the handle in a state the next call completes)
    if (int rc = h->ensure(h->d_xf_state, (size_t)h->B * rec + 16)) return rc;
    if (int rc = h->ensure(h->d_xf_trial, (size_t)h->B * h->q * ts)) return rc;
    if (int rc = h->ensure(h->d_xf_want, (size_t)h->B * sizeof(int32_t))) return rc;
    if (int rc = h->ensure(h->d_xf_nactive, 2 * sizeof(int32_t))) return rc;
    if (!h->h_xf_nactive)
        if (int rc = h->alloc_pinned(h->h_xf_nactive, sizeof(int32_t), hipHostMallocDefault)) return rc;
    if (!h->d_xf_active) {
        // both lists start as the identity: an entry beyond a step's count is then always a valid (finished) problem index
        if (int rc = h->alloc(h->d_xf_active, (size_t)2 * h->B * sizeof(int32_t))) return rc;
        std::vector<int32_t> iota((size_t)2 * h->B);
        for (int64_t i = 0; i < 2 * h->B; ++i) iota[(size_t)i] = (int32_t)(i % h->B);
        VP_HIP(hipMemcpyAsync(h->d_xf_active, iota.data(), iota.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream));
    }
    h->xf_known_active = h->B;
    h->xf_opts = opts_or_default(h, opts);
    if (int rc = upload_alpha(h, alpha0)) return rc;
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream));
    VP_HIP(hipMemsetAsync(h->d_xf_nactive, 0, 2 * sizeof(int32_t), h->stream));
    h->xf_running = true;
    h->xf_init = true;
    h->xf_flags = flags;
    h->xf_steps = 0;
    invalidate(h);
    return VP_ERR_OK;
}

int vp_fit_step_with_basis(vp_batch *h, const void *Phi, const void *dPhi, void *alpha_trial_out, int32_t *want_out,
                           int64_t *n_active_out) {
    VP_ENTER(h);
    VP_NOT_DEVCOLS(h, "vp_fit_step_with_basis");
    if (!h->external || !h->xf_running) return fail(VP_ERR_INVALID, "vp_fit_step_with_basis without vp_fit_begin");
    if (!Phi) return fail(VP_ERR_INVALID, "null Phi");
    const bool lazy = (h->xf_flags & VP_FIT_DERIVATIVES_ON_ACCEPT) != 0;
    if (!dPhi && h->ext_np > 0 && (!lazy || h->xf_init))
        return fail(VP_ERR_INVALID, "null dPhi (only a VP_FIT_DERIVATIVES_ON_ACCEPT fit may omit it, and not in its first step)");
    if (int rc = ext_stage(h, Phi, h->n, h->ext_phi, h->ext_phi_own)) return rc;
    if (int rc = ext_stage(h, dPhi, h->ext_np, h->ext_dphi, h->ext_dphi_own)) return rc;
    const size_t ts = tsize(h->dtype);
    const bool direct = device_ptrs(h); // the kernel writes the caller's device arrays itself
    ExtFitParams p;
    fill_ext_params(h, p);
    p.alpha_trial = (direct && alpha_trial_out) ? alpha_trial_out : h->d_xf_trial;
    p.want = (direct && want_out) ? want_out : h->d_xf_want;
    Timer tm(h, VP_KERNEL_FIT);
    const int rc = external_fit_step(p);
    tm.stop();
    if (rc != VP_ERR_OK) return fail(rc, "fit step kernel launch failed");
    h->xf_init = false;
    h->xf_steps += 1;
    if (!direct) {
        if (alpha_trial_out)
            VP_HIP(hipMemcpyAsync(alpha_trial_out, h->d_xf_trial, (size_t)h->B * h->q * ts, hipMemcpyDeviceToHost, h->stream));
        if (want_out)
            VP_HIP(hipMemcpyAsync(want_out, h->d_xf_want, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    }
    if (n_active_out) {
        VP_HIP(hipMemcpyAsync(h->h_xf_nactive, h->d_xf_nactive + ((h->xf_steps - 1) & 1), sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream));
        *n_active_out = *h->h_xf_nactive;
        h->xf_known_active = *h->h_xf_nactive; // the next evaluation launch shrinks to it
    } else if (!direct) {
        VP_HIP(hipStreamSynchronize(h->stream)); // host arrays: the caller reads them (and reuses Phi / dPhi) right away
    }
    return VP_ERR_OK;
}

int vp_fit_active_set(vp_batch *h, int32_t *index_out, int32_t *count_out) {
    VP_ENTER(h);
    VP_NOT_DEVCOLS(h, "vp_fit_active_set");
    if (!h->external || !h->xf_running) return fail(VP_ERR_INVALID, "vp_fit_active_set without vp_fit_begin");
    if (h->xf_init) return fail(VP_ERR_INVALID, "vp_fit_active_set before the first vp_fit_step_with_basis");
    const int slot = (int)((h->xf_steps - 1) & 1); // the list and the counter the last step's LM kernel wrote
    if (int rc = copy_out(h, index_out, h->d_xf_active + (size_t)slot * h->B, (size_t)h->B * sizeof(int32_t))) return rc;
    if (int rc = copy_out(h, count_out, h->d_xf_nactive + slot, sizeof(int32_t))) return rc;
    return VP_ERR_OK;
}

int vp_fit_end(vp_batch *h, void *alpha_out, void *C_out, vp_report *rep) {
    VP_ENTER(h);
    VP_NOT_DEVCOLS(h, "vp_fit_end");
    if (!h->external || !h->xf_running) return fail(VP_ERR_INVALID, "vp_fit_end without vp_fit_begin");
    if (h->xf_init) return fail(VP_ERR_INVALID, "vp_fit_end before the first vp_fit_step_with_basis");
    h->xf_running = false;
    after_fit(h);
    // the columns the handle last saw belong to a trial point, not necessarily to the fitted one
    h->ext_phi = nullptr;
    h->ext_dphi = nullptr;
    return copy_fit_out(h, alpha_out, C_out, rep);
}

int vp_set_params(vp_batch *h, const void *alpha) {
    VP_ENTER(h);
    VP_NOT_EXTERNAL(h, "vp_set_params");
    VP_NEEDS_IRF(h, "vp_set_params");
    if (!alpha) return fail(VP_ERR_INVALID, "null alpha");
    if (int rc = upload_alpha(h, alpha)) return rc;
    if (h->devcols)
        if (int rc = fill_own_columns(h, h->d_alpha, nullptr, nullptr, h->B)) return rc;
    return cache_at_alpha(h);
}

int vp_params(vp_batch *h, void *alpha_out) {
    VP_ENTER(h);
    if (!h->have_params && !h->alpha_kept) return fail(VP_ERR_INVALID, "no parameters set yet");
    return copy_out(h, alpha_out, h->d_alpha, (size_t)h->B * h->q * tsize(h->dtype));
}

static int copy_status(vp_batch *h, int32_t *status) {
    if (!status) return 0;
    if (!h->have_params) {
        // residuals()/jacobian() before set_params: cached is None
        std::vector<int32_t> tmp((size_t)h->B, VP_ST_NOT_EVALUATED);
        if (device_ptrs(h)) {
            VP_HIP(hipMemcpyAsync(status, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice, h->stream));
            VP_HIP(hipStreamSynchronize(h->stream));
        } else {
            std::memcpy(status, tmp.data(), tmp.size() * 4);
        }
        return 0;
    }
    return copy_out(h, status, h->d_status, (size_t)h->B * sizeof(int32_t));
}

int vp_residuals(vp_batch *h, void *r_out, int32_t *status) {
    VP_ENTER(h);
    if (!h->have_params) return copy_status(h, status) ? VP_ERR_HIP : VP_ERR_OK;
    if (!h->r_valid) {
        if (int rc = ensure_R(h)) return rc;
        if (int rc = run_evaluate(h, h->d_R, nullptr, nullptr)) return rc;
        h->r_valid = true;
    }
    if (int rc = copy_out_rows(h, r_out, h->d_R, (size_t)h->B * h->S)) return rc;
    return copy_status(h, status);
}

int vp_jacobian(vp_batch *h, void *J_out, int32_t *status) {
    VP_ENTER(h);
    if (!h->have_params) return copy_status(h, status) ? VP_ERR_HIP : VP_ERR_OK;
    if (!J_out) return fail(VP_ERR_INVALID, "null J_out");
    if (h->external && h->ext_np > 0 && !h->ext_dphi)
        return fail(VP_ERR_INVALID, "no derivative columns at the current parameters: pass dPhi to vp_set_params_with_basis "
                                    "or call vp_jacobian_with_derivatives");
    RowOut J;
    if (int rc = J.init(h, J_out, (size_t)h->B * h->q * h->S)) return rc;
    if (int rc = run_evaluate(h, nullptr, J.dptr, nullptr)) return rc;
    if (int rc = J.finish(h)) return rc;
    return copy_status(h, status);
}

int vp_linear_coeffs(vp_batch *h, void *C_out, int32_t *status) {
    VP_ENTER(h);
    if (!h->have_params) return copy_status(h, status) ? VP_ERR_HIP : VP_ERR_OK;
    if (int rc = copy_out(h, C_out, h->d_C, (size_t)h->B * h->S * h->n * tsize(h->dtype))) return rc;
    return copy_status(h, status);
}

int vp_weighted_data(vp_batch *h, void *Yw_out) {
    VP_ENTER(h);
    return copy_out_rows(h, Yw_out, h->d_yw, (size_t)h->B * h->S);
}

int vp_set_observations(vp_batch *h, const void *Y) {
    VP_ENTER(h);
    if (!Y) return fail(VP_ERR_INVALID, "Right hand side(s) not provided", VP_BUILD_Y_DATA_MISSING);
    const size_t ts = tsize(h->dtype);
    const size_t y_elems = (size_t)h->B * h->S * h->m;
    // Y_w = W * Y straight into the handle's buffer; host pointers are staged through the buffer itself
    const void *ysrc = Y;
    PaddedInputs pad;
    if (h->m_user) { // m < n: pad the caller's rows on the host, then as a host array
        if (int rc = pad_inputs_host(pad, device_ptrs(h), h->stream, ts, h->m_user, h->m, nullptr, 0, Y, (size_t)h->B * h->S,
                                     nullptr, 0, false))
            return rc;
        VP_HIP(hipMemcpyAsync(h->d_yw, pad.y.data(), y_elems * ts, hipMemcpyHostToDevice, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream));
        ysrc = h->d_yw;
    } else if (!device_ptrs(h)) {
        VP_HIP(hipMemcpyAsync(h->d_yw, Y, y_elems * ts, hipMemcpyHostToDevice, h->stream));
        ysrc = h->d_yw; // in place: every element is read once and written once by the same thread
    }
    if (h->d_w || ysrc != h->d_yw)
        if (int rc = launch_weight_data(h, ysrc)) return rc;
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream)); // the caller may reuse its host buffer
    invalidate(h); // the cached evaluation / fit belongs to the old data
    return VP_ERR_OK;
}

int vp_cost(vp_batch *h, double *cost_out) {
    VP_ENTER(h);
    if (!h->have_params) return fail(VP_ERR_INVALID, "no parameters set yet");
    return copy_out(h, cost_out, h->d_cost, (size_t)h->B * sizeof(double));
}

int vp_evaluate(vp_batch *h, const void *alpha, void *r_out, void *J_out, void *C_out, double *cost_out,
                int32_t *status) {
    VP_ENTER(h);
    VP_NOT_EXTERNAL(h, "vp_evaluate");
    VP_NEEDS_IRF(h, "vp_evaluate");
    if (!alpha) return fail(VP_ERR_INVALID, "null alpha");
    if (int rc = upload_alpha(h, alpha)) return rc;
    if (h->devcols) {
        if (int rc = fill_own_columns(h, h->d_alpha, nullptr, nullptr, h->B)) return rc;
        if (int rc = evaluate_at_alpha(h, r_out, J_out, C_out, cost_out, status)) return rc;
        if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream));
        return VP_ERR_OK;
    }
    return evaluate_at_alpha(h, r_out, J_out, C_out, cost_out, status);
}

int vp_basis(vp_batch *h, const void *alpha, void *Phi_out, void *dPhi_out, int flags) {
    VP_ENTER(h);
    VP_NOT_EXTERNAL(h, "vp_basis");
    VP_NEEDS_IRF(h, "vp_basis");
    if (!alpha) return fail(VP_ERR_INVALID, "null alpha");
    const size_t ts = tsize(h->dtype);
    if (h->devcols) { // the column kernel straight into the caller's arrays (host-pointer handles: staged)
        const int nc = column_map(h->col_model, flags & VP_BASIS_SKIP_INVARIANT).n_phi_cols; // (fixing changes no Phi column)
        const size_t rows = (size_t)col_rows(h);
        InBuf a;
        if (int rc = a.init(h, alpha, (size_t)h->B * h->q * ts)) return rc;
        OutBuf phi, dphi;
        if (int rc = phi.init(h, Phi_out, (size_t)h->B * nc * rows * ts)) return rc;
        if (int rc = dphi.init(h, dPhi_out, (size_t)h->B * h->ext_np * rows * ts)) return rc;
        if (int rc = ensure_irf_shift(h)) return rc;
        ColsParams c;
        fill_cols_params(h, c);
        c.alpha = a.dptr;
        c.phi = phi.dptr;
        c.dphi = dphi.dptr;
        c.skip_invariant = (flags & VP_BASIS_SKIP_INVARIANT) ? 1 : 0;
        c.nt = h->col_nt == 0 ? 0 : 1;
        Timer tm(h, VP_KERNEL_BASIS);
        const int rc = handle_cols_fill(c);
        tm.stop();
        if (rc != VP_ERR_OK) return fail(rc, "column kernel launch failed");
        if (int rc2 = phi.finish(h)) return rc2;
        if (int rc2 = dphi.finish(h)) return rc2;
        if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream));
        return VP_ERR_OK;
    }
    int ncols = 0;
    for (int j = 0; j < h->n; ++j)
        if (!((flags & VP_BASIS_SKIP_INVARIANT) && h->model.kind[j] == VP_BASIS_CONST)) ++ncols;
    InBuf a;
    if (int rc = a.init(h, alpha, (size_t)h->B * h->q * ts)) return rc;
    RowOut phi, dphi;
    if (int rc = phi.init(h, Phi_out, (size_t)h->B * ncols)) return rc;
    if (int rc = dphi.init(h, dPhi_out, (size_t)h->B * h->p)) return rc;
    LaunchParams p;
    fill_params(h, p);
    p.alpha = a.dptr;
    p.Phi_out = phi.dptr;
    p.dPhi_out = dphi.dptr;
    p.basis_flags = flags;
    Timer tm(h, VP_KERNEL_BASIS);
    int rc = h->kern->basis(p);
    tm.stop();
    if (rc != VP_ERR_OK) return fail(rc, "basis kernel launch failed");
    if (int rc2 = phi.finish(h)) return rc2;
    if (int rc2 = dphi.finish(h)) return rc2;
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream));
    return VP_ERR_OK;
}

// vp_fit of a device-column handle: the stepped LM of caller-evaluated models (xf_begin / xf_step / vp_fit_end's state)
// with the column kernel in the caller's place.  Per step: the columns of the still-active problems at their trial points
// (the list and the count the previous step's LM kernel left on the device), then the step.  The host reads the active
// count every col_look steps (8 unless vp_debug_set_column_fit says otherwise) -- a synchronisation; the steps in between are enqueued blind, and a step past the end
// of every fit is two empty launches.  Every problem ends within patience*(q+1) evaluations, so the loop does.
namespace {
// one step of that loop: the LM step on the handle's own columns, the trial points stay on the device; `look`: read the
// active count (synchronises the stream)
// d_alpha <- g^-1(d_alpha) (to_internal) or g(d_alpha), in place on the handle's stream
int transform_alpha(vp_batch *h, const int to_internal) {
    if (int rc = bounds_transform(h->dtype, h->d_alpha, h->d_lo, h->d_hi, h->bound_stride, h->q, h->B, to_internal, h->stream))
        return fail(rc, "bounds map kernel launch failed");
    return VP_ERR_OK;
}
int devcols_step(vp_batch *h, const bool look, int64_t &n_active) {
    ExtFitParams p;
    fill_ext_params(h, p);
    p.alpha_trial = h->d_xf_trial;
    p.want = h->d_xf_want;
    if (int rc = external_fit_step(p)) return fail(rc, "fit step kernel launch failed");
    h->xf_init = false;
    h->xf_steps += 1;
    if (look) {
        VP_HIP(hipMemcpyAsync(h->h_xf_nactive, h->d_xf_nactive + ((h->xf_steps - 1) & 1), sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        VP_HIP(hipStreamSynchronize(h->stream));
        n_active = h->xf_known_active = *h->h_xf_nactive;
    }
    return VP_ERR_OK;
}
int devcols_fit(vp_batch *h, const vp_lm_opts *opts, void *alpha_inout, void *C_out, vp_report *rep) {
    if (!alpha_inout) return fail(VP_ERR_INVALID, "null alpha");
    VP_NEEDS_IRF(h, "vp_fit");
    if (int rc = xf_begin(h, opts, alpha_inout, 0)) return rc;
    const int64_t limit = 2 * ((int64_t)h->xf_opts.patience * (h->q + 1) + 2);
    Timer tm(h, VP_KERNEL_FIT);
    // box bounds: the LM drivers iterate on u = g^-1(alpha) -- d_alpha, the trial points and the best points are internal
    // until the loop has ended; only the column kernel knows
    const bool bnd = h->bounded;
    if (bnd)
        if (int rc = transform_alpha(h, 1)) {
            h->xf_running = false;
            return rc;
        }
    for (int64_t step = 1; step <= limit; ++step) {
        int rc;
        if (h->xf_init) {
            rc = fill_own_columns(h, h->d_alpha, nullptr, nullptr, h->B, bnd);
        } else {
            const int slot = (int)((h->xf_steps + 1) & 1); // what the previous step's LM kernel wrote
            const int64_t bound = h->xf_known_active < h->B ? std::max<int64_t>(h->xf_known_active, 1) : h->B;
            rc = fill_own_columns(h, h->d_xf_trial, h->d_xf_active + (size_t)slot * h->B, h->d_xf_nactive + slot, bound, bnd);
        }
        if (rc) {
            h->xf_running = false;
            return rc;
        }
        const bool look = step % h->col_look == 0 || step == limit;
        int64_t nact = -1;
        if (int rc2 = devcols_step(h, look, nact)) {
            h->xf_running = false;
            return rc2;
        }
        if (look && nact == 0) break;
    }
    h->xf_running = false;
    if (bnd) // back to the caller's parameters: the same map as the column kernel's, so alpha is the point of the last columns
        if (int rc = transform_alpha(h, 0)) return rc;
    after_fit(h);
    // the handle's state is the fitted point, its columns included (unbounded: d_alpha holds alpha again)
    if (int rc = fill_own_columns(h, h->d_alpha, nullptr, nullptr, h->B)) return rc;
    tm.stop();
    return copy_fit_out(h, alpha_inout, C_out, rep);
}
} // namespace

int vp_fit(vp_batch *h, const vp_lm_opts *opts, void *alpha_inout, void *C_out, vp_report *rep) {
    if (h && h->devcols) {
        VP_ENTER(h);
        return devcols_fit(h, opts, alpha_inout, C_out, rep);
    }
    return vp_fit_trace(h, opts, alpha_inout, C_out, rep, nullptr, 0);
}

// ---- flag-and-refit (round 6; vp_fit.hpp jac_not_finite) --------------------------------------------------------------
// A fit kernel that finds the Jacobian factor of an accepted point non-finite after an evaluation that was ok ends that fit,
// appends the problem to h->d_rescue and leaves its initial guess in h->d_alpha.  rescue_refit launches the generic fit
// kernel (any descriptor, any m, weights) over that list with power-of-two column scaling -- the reference's order of
// operations, D_k c first (src/solvers/levmar/mod.rs:156-171) -- from alpha0; it overwrites every output of those
// problems.  kRescueBlocks persistent workgroups: a launch with an empty list ends in the time of the launch itself
// (~3 us on the stream, no host synchronisation anywhere).
namespace {
constexpr int kRescueBlocks = 8;
int rescue_prepare(vp_batch *h, LaunchParams &p) {
    if (h->rescue_off || h->kern->family == FAMILY_GENERIC || h->kern->gram_fit) return 0; // (the generic kernel scales by itself)
    if (!h->d_rescue) {
        if (int rc = h->alloc(h->d_rescue, (size_t)(2 + h->B) * sizeof(int32_t))) return rc;
        VP_HIP(hipMemsetAsync(h->d_rescue, 0, 2 * sizeof(int32_t), h->stream));
        h->rescue_slot = 0;
    }
    if (int rc = h->ensure(h->d_rescue_ws, (size_t)kRescueBlocks * gen_slot_bytes(h))) return rc;
    p.rescue = h->d_rescue;
    p.rescue_slot = h->rescue_slot;
    return 0;
}
int rescue_refit(vp_batch *h, const LaunchParams &fit_params) {
    if (!fit_params.rescue) return 0;
    LaunchParams p = fit_params;
    // the first kFitRescueGrid flagged problems on the set's own wave-per-problem kernel with scaled derivative columns (a
    // flagged fit at ~4 us per evaluation: it must not outlast the batch it came from); whatever is left -- more problems
    // than that, weights, per-problem grids, models without that kernel -- on the generic kernel, which also zeroes the
    // list's other counter
    p.gen_list_first = 0;
    p.last_fit = nullptr; // (the record names the fit's own launch, not the re-fit of what it flagged)
    if (launch_fn fast = h->kern->fit_rescue) {
        const int rc = fast(p);
        if (rc == VP_ERR_OK) p.gen_list_first = kFitRescueGrid;
        else if (rc != VP_ERR_UNSUPPORTED) return rc;
    }
    p.rescue = nullptr;
    p.gen_ws = h->d_rescue_ws;
    p.gen_blocks = kRescueBlocks;
    p.gen_list = h->d_rescue;
    p.gen_list_slot = h->rescue_slot;
    p.gen_scale_cols = 1;
    h->rescue_slot ^= 1;
    return generic_kernels(h->dtype)->fit_single(p);
}
} // namespace

int vp_fit_trace(vp_batch *h, const vp_lm_opts *opts, void *alpha_inout, void *C_out, vp_report *rep,
                 double *trace_out, int trace_rows) {
    VP_ENTER(h);
    if (h->devcols)
        return fail(VP_ERR_UNSUPPORTED, "vp_fit_trace: a device-column handle (VP_BASIS_GAUSS / _LORENTZ / _LINEAR) fits by the "
                                        "stepped LM of caller-evaluated models, which records no trace");
    VP_NOT_EXTERNAL(h, "vp_fit");
    if (!alpha_inout) return fail(VP_ERR_INVALID, "null alpha");
    if (h->m_user && (int64_t)h->q > h->m_user * h->S) {
        // m < n AND fewer residuals than nonlinear parameters (the padded handle would count its own n rows): the reference's
        // LM driver evaluates once and reports WrongDimensions
        if (int rc = upload_alpha(h, alpha_inout)) return rc;
        if (int rc = run_evaluate(h, nullptr, nullptr, h->d_C)) return rc;
        OutBuf trw; // row 0 = the initial point (ratio = NaN)
        if (int rc = trace_begin(h, trw, trace_out, trace_rows)) return rc;
        hipLaunchKernelGGL(wrong_dimensions_report_kernel, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream,
                           (const double *)h->d_cost, (const int32_t *)h->d_status, h->B, h->d_report,
                           trw.dptr ? (double *)trw.dptr : nullptr, trace_rows, h->q, h->dtype, (const void *)h->d_alpha);
        VP_HIP(hipGetLastError());
        after_fit(h);
        if (int rc = copy_fit_out(h, nullptr, C_out, rep)) return rc; // (the parameters stay the caller's)
        return trw.finish(h);
    }
    if (h->S != 1) return mrhs_fit(h, opts, alpha_inout, C_out, rep, trace_out, trace_rows);
    if (!h->kern->fit && !h->kern->fit_single) return fail(VP_ERR_UNSUPPORTED, "no fit kernel for this model");
    const vp_lm_opts o = opts_or_default(h, opts);
    if (int rc = upload_alpha(h, alpha_inout)) return rc;
    LaunchParams p;
    fill_params(h, p);
    p.alpha_out = h->d_alpha;
    p.C_out = h->d_C;
    p.cost_out = h->d_cost_bs;
    p.status = h->d_status_bs;
    p.report = h->d_report;
    p.opts = &o;
    OutBuf tr;
    if (int rc = trace_begin(h, tr, trace_out, trace_rows)) return rc;
    set_trace(p, tr, trace_rows);
    // kern->fit is the persistent slot kernel (vp_fit2.hpp); it falls back to the one-problem-per-wave kernel
    // (vp_fit.hpp) by itself for the cases it does not cover (weights, per-problem grids, models without a trailing
    // constant column, batches smaller than the device's resident wave slots).  vp_set_fit_kernel overrides.
    launch_fn fit_fn = h->kern->fit ? h->kern->fit : h->kern->fit_single;
    if (int rc0 = rescue_prepare(h, p)) return rc0;
    int list_used = 0; // (set by the launcher when its kernel may append to the list)
    p.rescue_used = &list_used;
    p.last_fit = h->last_fit;
    Timer tm(h, VP_KERNEL_FIT);
    int rc = fit_fn(p);
    if (rc == VP_ERR_OK && list_used) rc = rescue_refit(h, p); // (the problems the fit kernel flagged and did not re-fit itself)
    tm.stop();
    if (rc != VP_ERR_OK) return fail(rc, "fit kernel launch failed");
    after_fit(h);
    if (int rc2 = copy_fit_out(h, alpha_inout, C_out, rep)) return rc2;
    return tr.finish(h);
}

int vp_set_bounds(vp_batch *h, const double *lower, const double *upper, int per_problem) {
    VP_ENTER(h);
    if (!h->devcols)
        return fail(VP_ERR_UNSUPPORTED, "vp_set_bounds needs a device-column handle: a descriptor with VP_BASIS_GAUSS / _LORENTZ / "
                                        "_LINEAR, or any descriptor created with VP_FLAG_DEVICE_COLUMNS");
    if (h->xf_running) return fail(VP_ERR_INVALID, "vp_set_bounds during a stepped fit");
    if (!lower && !upper) {
        h->bounded = false;
        return VP_ERR_OK;
    }
    if (!lower || !upper) return fail(VP_ERR_INVALID, "vp_set_bounds: lower and upper must both be given (or both be NULL)");
    const size_t count = (size_t)(per_problem ? h->B : 1) * (size_t)h->q;
    for (size_t i = 0; i < count; ++i)
        if (std::isnan(lower[i]) || std::isnan(upper[i]) || !(lower[i] < upper[i]))
            return fail(VP_ERR_INVALID, "vp_set_bounds: every parameter needs lower < upper (no NaN; -INFINITY / +INFINITY = unbounded)");
    // the box in the handle's dtype, rounded INTO the caller's box: a parameter inside the stored box is inside the caller's
    const size_t ts = tsize(h->dtype), bytes = count * ts;
    std::vector<unsigned char> host(2 * bytes);
    for (size_t i = 0; i < count; ++i) {
        if (h->dtype == VP_F64) {
            reinterpret_cast<double *>(host.data())[i] = lower[i];
            reinterpret_cast<double *>(host.data() + bytes)[i] = upper[i];
        } else {
            float lo = (float)lower[i], hi = (float)upper[i];
            if ((double)lo < lower[i]) lo = std::nextafterf(lo, INFINITY);
            if ((double)hi > upper[i]) hi = std::nextafterf(hi, -INFINITY);
            if (!(lo < hi)) return fail(VP_ERR_INVALID, "vp_set_bounds: the box is empty in the handle's fp32");
            reinterpret_cast<float *>(host.data())[i] = lo;
            reinterpret_cast<float *>(host.data() + bytes)[i] = hi;
        }
    }
    // (sized for the per-problem form at the first call: a later call may switch forms)
    if (int rc = h->ensure(h->d_lo, (size_t)h->B * h->q * ts)) return rc;
    if (int rc = h->ensure(h->d_hi, (size_t)h->B * h->q * ts)) return rc;
    h->bounded = false; // (until both arrays have arrived)
    VP_HIP(hipMemcpyAsync(h->d_lo, host.data(), bytes, hipMemcpyHostToDevice, h->stream));
    VP_HIP(hipMemcpyAsync(h->d_hi, host.data() + bytes, bytes, hipMemcpyHostToDevice, h->stream));
    VP_HIP(hipStreamSynchronize(h->stream)); // (the staging vector goes out of scope)
    h->bound_stride = per_problem ? h->q : 0;
    h->bounded = true;
    return VP_ERR_OK;
}

int vp_set_irf(vp_batch *h, const void *irf, int per_problem) {
    VP_ENTER(h);
    if (!h->irf_kinds)
        return fail(VP_ERR_INVALID, "vp_set_irf: the handle's model has no IRF reconvolution kind (VP_BASIS_EXP_DECAY_IRF / "
                                    "VP_BASIS_IRF)");
    if (h->xf_running) return fail(VP_ERR_INVALID, "vp_set_irf during a stepped fit");
    if (!irf) return fail(VP_ERR_INVALID, "vp_set_irf: null irf");
    const size_t ts = tsize(h->dtype), rows = (size_t)col_rows(h);
    // (sized for the per-problem form at the first call: a later call may switch forms)
    if (int rc = h->ensure(h->d_irf, (size_t)h->B * rows * ts)) return rc;
    h->have_irf = false; // (until the copy has been enqueued)
    VP_HIP(hipMemcpyAsync(h->d_irf, irf, (size_t)(per_problem ? h->B : 1) * rows * ts,
                          device_ptrs(h) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream)); // the caller may reuse its host buffer
    h->irf_stride = per_problem ? (int64_t)rows : 0;
    h->have_irf = true;
    // the cached evaluation / fit and the handle's columns belong to the old response
    invalidate(h);
    h->ext_phi = nullptr;
    h->ext_dphi = nullptr;
    return VP_ERR_OK;
}

int vp_set_irf_period(vp_batch *h, double period) {
    VP_ENTER(h);
    if (!h->irf_periodic)
        return fail(VP_ERR_INVALID, "vp_set_irf_period: the handle's model has no VP_BASIS_EXP_DECAY_IRF_PERIODIC");
    if (!(period >= 0.0)) return fail(VP_ERR_INVALID, "vp_set_irf_period: the period must be 0 (the record is one period) or positive");
    if (h->xf_running) return fail(VP_ERR_INVALID, "vp_set_irf_period during a stepped fit");
    if (period > 0.0 && h->irf_span_max >= 0.0 && period < h->irf_span_max * (1.0 - 1e-6))
        return fail(VP_ERR_INVALID, "vp_set_irf_period: the period is shorter than the record, period < m dt (1 - 1e-6)");
    h->irf_period = period;
    // the cached evaluation / fit and the handle's columns belong to the old period
    invalidate(h);
    h->ext_phi = nullptr;
    h->ext_dphi = nullptr;
    return VP_ERR_OK;
}

// ---- start-point search (vp_search.hpp) ---------------------------------------------------------------------------------
namespace {

// hipEvents around the stages of the shared route (vp_set_timing); without timing every call is a no-op
struct SearchClock {
    vp_batch *h;
    hipEvent_t ev[5] = {};
    int count = 0;
    explicit SearchClock(vp_batch *h_) : h(h_) {}
    void mark() {
        if (!h->timing || count >= 5) return;
        if (hipEventCreate(&ev[count]) != hipSuccess) return;
        (void)hipEventRecord(ev[count], h->stream);
        ++count;
    }
    ~SearchClock() {
        if (count == 5) {
            (void)hipEventSynchronize(ev[4]);
            for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&h->srch_ms[i], ev[i], ev[i + 1]);
        }
        for (int i = 0; i < count; ++i) (void)hipEventDestroy(ev[i]);
    }
};

// shared candidates, shared grid, shared (or no) weights: (a) columns of the K candidates, (b) their orthonormal bases,
// (c) the ranking product; leaves the winners in d_srch_index
int search_shared(vp_batch *h, const void *cand_dev, const int64_t K, SearchClock &clk) {
    const size_t ts = tsize(h->dtype);
    const int64_t Kpad = (K + 15) / 16 * 16, ldq = (h->m + 15) / 16 * 16;
    if (Kpad > 0x7fffffff || ldq > 0x7fffffff) return fail(VP_ERR_INVALID, "vp_search: K or m out of range");
    if (int rc = h->grow(h->d_srch_phi, h->srch_phi_cap, (size_t)K * h->n * h->m * ts)) return rc;
    if (int rc = h->grow(h->d_srch_q, h->srch_q_cap, (size_t)Kpad * h->n * ldq * ts)) return rc;
    if (int rc = h->grow(h->d_srch_bad, h->srch_bad_cap, (size_t)Kpad * sizeof(int32_t))) return rc;
    if (h->S > 1)
        if (int rc = h->grow(h->d_srch_scores, h->srch_scores_cap, (size_t)h->B * h->S * Kpad * ts)) return rc;
    clk.mark();
    ColsParams c;
    fill_cols_params(h, c);
    c.model = h->devcols ? h->col_model : h->model;
    c.t_stride = 0;
    c.alpha = cand_dev;
    c.phi = h->d_srch_phi;
    c.B = K; // (the kernel's "problem" is the candidate: fixed values must be shared, vp_search sees to it)
    if (int rc = handle_cols_fill(c)) return fail(rc, "column kernel launch failed");
    clk.mark();
    // zero columns beyond m and beyond K; every padded candidate marked, (b) clears the marks of the finite ones
    VP_HIP(hipMemsetAsync(h->d_srch_q, 0, (size_t)Kpad * h->n * ldq * ts, h->stream));
    VP_HIP(hipMemsetAsync(h->d_srch_bad, 1, (size_t)Kpad * sizeof(int32_t), h->stream));
    SearchParams p;
    std::memset(&p, 0, sizeof(p));
    p.dtype = h->dtype;
    p.n = h->n;
    p.K = (int)K;
    p.Kpad = (int)Kpad;
    p.m = (int)h->m;
    p.ldq = (int)ldq;
    p.B = h->B;
    p.S = (int)h->S;
    p.phi = h->d_srch_phi;
    p.w = h->d_w;
    p.Q = h->d_srch_q;
    p.bad = h->d_srch_bad;
    p.yw = h->d_yw;
    p.scores = h->d_srch_scores;
    p.index = h->d_srch_index;
    p.stream = h->stream;
    if (int rc = search_orthonormalize(p)) return fail(rc, "vp_search: orthonormalisation kernel launch failed");
    clk.mark();
    if (int rc = search_rank(p)) return fail(rc, "vp_search: ranking kernel launch failed");
    clk.mark();
    return VP_ERR_OK;
}

// everything else: K cost-only evaluations through the handle's own evaluate path and a running minimum
int search_loop(vp_batch *h, const void *cand_dev, const int64_t K, const int per_problem) {
    if (K > 0x7fffffff) return fail(VP_ERR_INVALID, "vp_search: K out of range");
    if (int rc = h->ensure(h->d_srch_best, (size_t)h->B * sizeof(double))) return rc;
    for (int64_t k = 0; k < K; ++k) {
        if (int rc = search_gather(h->dtype, cand_dev, K, h->q, per_problem, k, nullptr, h->B, h->d_alpha, h->stream))
            return fail(rc, "vp_search: gather kernel launch failed");
        if (h->devcols)
            if (int rc = fill_own_columns(h, h->d_alpha, nullptr, nullptr, h->B)) return rc;
        if (int rc = run_evaluate(h, nullptr, nullptr, h->d_C)) return rc;
        if (int rc = search_loop_update(h->d_cost, h->d_status, k, h->B, h->d_srch_best, h->d_srch_index, h->stream))
            return fail(rc, "vp_search: update kernel launch failed");
    }
    return VP_ERR_OK;
}

} // namespace

int vp_search(vp_batch *h, const void *cand, int64_t K, int flags, void *alpha_out, int32_t *index_out, double *cost_out) {
    VP_ENTER(h);
    if (h->xf_running) return fail(VP_ERR_INVALID, "vp_search during a stepped fit");
    VP_NOT_EXTERNAL(h, "vp_search");
    VP_NEEDS_IRF(h, "vp_search");
    if (h->rhs_allreduce)
        return fail(VP_ERR_UNSUPPORTED, "vp_search: the handle's right-hand sides are sharded over ranks (vp_set_rhs_allreduce)");
    if (!cand) return fail(VP_ERR_INVALID, "null cand");
    if (K < 1) return fail(VP_ERR_INVALID, "vp_search needs K >= 1 candidates");
    if (flags & ~VP_SEARCH_PER_PROBLEM) return fail(VP_ERR_INVALID, "unknown vp_search flag");
    const int per_problem = (flags & VP_SEARCH_PER_PROBLEM) ? 1 : 0;
    const size_t ts = tsize(h->dtype);
    if (int rc = h->ensure(h->d_srch_index, (size_t)h->B * sizeof(int32_t))) return rc;
    InBuf cd;
    if (int rc = cd.init(h, cand, (size_t)(per_problem ? h->B : 1) * (size_t)K * h->q * ts)) return rc;
    // from here on the cached evaluation is being replaced
    h->r_valid = false;
    const bool shared = !per_problem && !(h->flags & (VP_FLAG_T_PER_PROBLEM | VP_FLAG_W_PER_PROBLEM)) && !h->m_user &&
                        !(h->irf_kinds && h->irf_stride != 0) && // (a response per problem: the candidate loop, like a grid per problem)
                        !h->irf_shift &&                         // (a shifted kind: g belongs to the problem, not to the candidate)
                        !(h->fixed && h->fix_stride != 0);       // (fixed values per problem: the same)
    {
        SearchClock clk(h);
        if (shared) {
            if (int rc = search_shared(h, cd.dptr, K, clk)) return rc;
        } else {
            if (int rc = search_loop(h, cd.dptr, K, per_problem)) return rc;
        }
        // the winners become the handle's parameters (a problem without a finite candidate: its candidate 0), then the
        // evaluation of vp_set_params
        if (int rc = search_gather(h->dtype, cd.dptr, K, h->q, per_problem, -1, h->d_srch_index, h->B, h->d_alpha, h->stream))
            return fail(rc, "vp_search: gather kernel launch failed");
        if (h->devcols)
            if (int rc = fill_own_columns(h, h->d_alpha, nullptr, nullptr, h->B)) return rc;
        if (int rc = cache_at_alpha(h)) return rc;
        clk.mark();
    }
    if (int rc = copy_out(h, alpha_out, h->d_alpha, (size_t)h->B * h->q * ts)) return rc;
    if (int rc = copy_out(h, index_out, h->d_srch_index, (size_t)h->B * sizeof(int32_t))) return rc;
    return copy_out(h, cost_out, h->d_cost, (size_t)h->B * sizeof(double));
}

int vp_debug_search_ms(vp_batch *h, float ms_out[4]) {
    VP_ENTER(h);
    if (!ms_out) return fail(VP_ERR_INVALID, "null ms_out");
    for (int i = 0; i < 4; ++i) ms_out[i] = h->srch_ms[i];
    return VP_ERR_OK;
}

int vp_debug_set_column_fit(vp_batch *h, int look_every, int nontemporal) {
    VP_ENTER(h);
    if (!h->devcols) return fail(VP_ERR_UNSUPPORTED, "vp_debug_set_column_fit needs a device-column handle");
    if (look_every < 1 || nontemporal < 0 || nontemporal > 1) return fail(VP_ERR_INVALID, "vp_debug_set_column_fit: bad argument");
    h->col_look = look_every;
    h->col_nt = nontemporal;
    return VP_ERR_OK;
}

static void kernel_set_record(const KernelEntry &e, int32_t out[8]) {
    const int32_t rec[8] = {e.dtype, e.family, e.a, e.b, e.c, e.R, e.W, e.uses_gen_ws};
    for (int i = 0; i < 8; ++i) out[i] = rec[i];
}

int vp_debug_kernel_set(vp_batch *h, int32_t out[8]) {
    if (!h || !h->kern) return fail(VP_ERR_INVALID, "null handle");
    if (!out) return fail(VP_ERR_INVALID, "null out");
    kernel_set_record(*h->kern, out);
    return VP_ERR_OK;
}

int vp_debug_last_fit(vp_batch *h, int32_t out[4]) {
    if (!h) return fail(VP_ERR_INVALID, "null handle");
    if (!out) return fail(VP_ERR_INVALID, "null out");
    for (int i = 0; i < 4; ++i) out[i] = h->last_fit[i];
    return VP_ERR_OK;
}

int vp_debug_registry_entry(int index, int32_t out[8]) {
    if (!out) return fail(VP_ERR_INVALID, "null out");
    if (index < 0 || (size_t)index >= registry().size()) return fail(VP_ERR_INVALID, "no such registry entry");
    const KernelEntry &e = registry()[(size_t)index];
    kernel_set_record(e, out);
    return e.stats && e.evaluate ? 1 : 0;
}

int vp_debug_last_global(vp_batch *h, int32_t out[8]) {
    if (!h) return fail(VP_ERR_INVALID, "null handle");
    if (!out) return fail(VP_ERR_INVALID, "null out");
    for (int i = 0; i < 8; ++i) out[i] = h->last_global[i];
    return VP_ERR_OK;
}

int vp_debug_registry_has_global(int index) {
    if (index < 0 || (size_t)index >= registry().size()) return fail(VP_ERR_INVALID, "no such registry entry");
    return has_mrhs_set(&registry()[(size_t)index]) ? 1 : 0;
}

int vp_debug_set_refit(vp_batch *h, int enabled) {
    VP_ENTER(h);
    h->rescue_off = enabled == 0;
    return VP_ERR_OK;
}

int vp_debug_gram_evaluate(vp_batch *h, const void *alpha, double *out) {
    VP_ENTER(h);
    if (!alpha || !out) return fail(VP_ERR_INVALID, "null argument");
    if (h->external || h->S != 1 || !h->kern->gram_fit || !h->kern->fit)
        return fail(VP_ERR_UNSUPPORTED, "the handle's fit does not run on the Gram kernel (fp32, exponentials + offset beyond one wavefront)");
    const size_t ts = tsize(h->dtype);
    const int per = 1 + h->n + h->q + h->q * h->q;
    InBuf a;
    if (int rc = a.init(h, alpha, (size_t)h->B * h->q * ts)) return rc;
    OutBuf o;
    if (int rc = o.init(h, out, (size_t)h->B * per * sizeof(double))) return rc;
    const vp_lm_opts opt = opts_or_default(h, nullptr);
    LaunchParams p;
    fill_params(h, p);
    p.alpha_out = const_cast<void *>(a.dptr); // read only in this mode
    p.opts = &opt;
    p.gram_dbg = (double *)o.dptr;
    if (int rc = h->kern->fit(p)) return fail(rc, "Gram evaluation launch failed");
    return o.finish(h);
}

extern "C++" {
namespace {
// one lane per record: the Gram fit kernel's trust-region sub-problem (lmpar_chol, vp_fit.hpp) exactly as
// slot_scalar_phase<..., GRAM> instantiates it
template <int Q>
__global__ void debug_lmpar_gram_kernel(int64_t B, const double *Rj, const int32_t *ipvt, const double *diag, const double *qtb,
                                        const double *delta, const double *par_in, double *out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double r[Q][Q], dg[Q], qb[Q], step[Q];
    int ip[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        dg[i] = diag[b * Q + i];
        qb[i] = qtb[b * Q + i];
        ip[i] = ipvt[b * Q + i];
        step[i] = 0.0;
#pragma unroll
        for (int j = 0; j < Q; ++j) r[i][j] = Rj[(b * Q + i) * Q + j];
    }
    double dxnorm = 0.0;
    const double par = vp::lmpar_chol<double, Q, false, (Q > 3)>(r, ip, dg, qb, delta[b], par_in[b], step, dxnorm);
    double *o = out + b * (Q + 2);
    o[0] = par;
    o[1] = dxnorm;
#pragma unroll
    for (int i = 0; i < Q; ++i) o[2 + i] = step[i];
}
} // namespace
} // extern "C++"

int vp_debug_lmpar_gram(int64_t B, int q, const double *Rj, const int32_t *ipvt, const double *diag, const double *qtb,
                        const double *delta, const double *par_in, double *out) {
    if (B <= 0 || !Rj || !ipvt || !diag || !qtb || !delta || !par_in || !out) return fail(VP_ERR_INVALID, "null argument");
    if (q != 2 && q != 3 && q != 5) return fail(VP_ERR_UNSUPPORTED, "q must be 2, 3 or 5");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VP_ERR_NO_DEVICE, "no device");
    const size_t nq = (size_t)B * q;
    const size_t sizes[7] = {nq * q * sizeof(double), nq * sizeof(int32_t), nq * sizeof(double), nq * sizeof(double),
                             (size_t)B * sizeof(double), (size_t)B * sizeof(double), (size_t)B * (q + 2) * sizeof(double)};
    const void *src[6] = {Rj, ipvt, diag, qtb, delta, par_in};
    DevMem mem[7];
    void *d[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = VP_ERR_OK;
    for (int i = 0; i < 7 && rc == VP_ERR_OK; ++i) {
        if (mem[i].alloc(sizes[i]) != 0) rc = VP_ERR_HIP;
        d[i] = mem[i].p;
    }
    for (int i = 0; i < 6 && rc == VP_ERR_OK; ++i)
        if (hipMemcpy(d[i], src[i], sizes[i], hipMemcpyHostToDevice) != hipSuccess) rc = VP_ERR_HIP;
    if (rc == VP_ERR_OK) {
        const dim3 grid((unsigned)((B + 63) / 64)), block(64);
        auto go = [&](auto qc) {
            constexpr int Q = decltype(qc)::value;
            hipLaunchKernelGGL((debug_lmpar_gram_kernel<Q>), grid, block, 0, 0, B, (const double *)d[0], (const int32_t *)d[1],
                               (const double *)d[2], (const double *)d[3], (const double *)d[4], (const double *)d[5], (double *)d[6]);
        };
        if (q == 2) go(std::integral_constant<int, 2>());
        else if (q == 3) go(std::integral_constant<int, 3>());
        else go(std::integral_constant<int, 5>());
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d[6], sizes[6], hipMemcpyDeviceToHost) != hipSuccess) rc = VP_ERR_HIP;
    }
    return rc == VP_ERR_OK ? VP_ERR_OK : fail(rc, "vp_debug_lmpar_gram: HIP call failed");
}

int vp_set_rhs_allreduce(vp_batch *h, vp_allreduce_fn fn, void *user, int64_t global_rhs_count) {
    VP_ENTER(h);
    if (fn && h->devcols)
        return fail(VP_ERR_UNSUPPORTED, "right-hand-side sharding is not available on a device-column handle (VP_BASIS_GAUSS / "
                                        "_LORENTZ / _LINEAR), as on caller-evaluated handles");
    if (fn) {
        if (h->S <= 1 || (!h->have_mrhs && !h->kern->mrhs_fit_whole))
            return fail(VP_ERR_UNSUPPORTED, "right-hand-side sharding needs a handle with S > 1");
        if (global_rhs_count < h->S) return fail(VP_ERR_INVALID, "global_rhs_count smaller than the local S");
    }
    h->rhs_allreduce = fn;
    h->rhs_allreduce_user = user;
    h->rhs_global = fn ? global_rhs_count : 0;
    return VP_ERR_OK;
}

// UNWEIGHTED Phi(alpha) * C of the handle's current parameters into fit_dev [B][S][m] (device memory)
static int launch_best_fit(vp_batch *h, void *fit_dev) {
    LaunchParams p;
    fill_params(h, p);
    p.C_out = h->d_C; // input here
    p.r_out = fit_dev; // output
    int rc = h->kern->best_fit(p);
    if (rc != VP_ERR_OK) return fail(rc, "best_fit kernel launch failed");
    return VP_ERR_OK;
}

int vp_best_fit(vp_batch *h, void *fit_out) {
    VP_ENTER(h);
    if (!h->have_params) return fail(VP_ERR_INVALID, "no parameters set yet");
    if (!h->kern->best_fit) return fail(VP_ERR_UNSUPPORTED, "no best_fit kernel for this model");
    RowOut f;
    if (int rc = f.init(h, fit_out, (size_t)h->B * h->S)) return rc;
    if (int rc = launch_best_fit(h, f.dptr)) return rc;
    return f.finish(h);
}

// ---- weights between fits (vp_set_weights) and Poisson re-weighting on the device (vp_poisson.hpp) --------------------------
int vp_set_weights(vp_batch *h, const void *w, const void *Y) {
    VP_ENTER(h);
    if (!w || !Y) return fail(VP_ERR_INVALID, "vp_set_weights: null w or Y (the handle keeps only W*Y: pass the observations again)");
    if (!h->d_w)
        return fail(VP_ERR_INVALID, "vp_set_weights: the handle was created without weights (its kernel set is the one of unit "
                                    "weights); create it with a weights array");
    if (h->xf_running) return fail(VP_ERR_INVALID, "vp_set_weights during a stepped fit");
    if (h->m_user) return fail(VP_ERR_UNSUPPORTED, "vp_set_weights: not available on a handle padded for m < n");
    const size_t ts = tsize(h->dtype);
    const size_t w_elems = (size_t)((h->flags & VP_FLAG_W_PER_PROBLEM) ? h->B * h->m : h->m);
    const size_t y_elems = (size_t)h->B * h->S * h->m;
    const hipMemcpyKind kin = device_ptrs(h) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    VP_HIP(hipMemcpyAsync(h->d_w, w, w_elems * ts, kin, h->stream));
    // Y_w = W * Y as vp_set_observations forms it: host data is staged through the handle's buffer and weighted in place
    const void *ysrc = Y;
    if (!device_ptrs(h)) {
        VP_HIP(hipMemcpyAsync(h->d_yw, Y, y_elems * ts, hipMemcpyHostToDevice, h->stream));
        ysrc = h->d_yw;
    }
    if (int rc = launch_weight_data(h, ysrc)) return rc;
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream)); // the caller may reuse its host buffers
    invalidate(h); // the cached evaluation / fit belongs to the old weights
    return VP_ERR_OK;
}

int vp_poisson_reweight(vp_batch *h, const void *Y, int mode, double floor, double *deviance_out, double *pearson_out) {
    VP_ENTER(h);
    if (!Y) return fail(VP_ERR_INVALID, "vp_poisson_reweight: null Y");
    if (mode != VP_POISSON_NEYMAN && mode != VP_POISSON_MODEL) return fail(VP_ERR_INVALID, "vp_poisson_reweight: unknown mode");
    if (!(floor > 0.0) || !std::isfinite(floor)) return fail(VP_ERR_INVALID, "vp_poisson_reweight: the floor must be finite and > 0");
    const bool model = mode == VP_POISSON_MODEL;
    if (!model && (deviance_out || pearson_out))
        return fail(VP_ERR_INVALID, "vp_poisson_reweight: deviance and Pearson X^2 belong to a fit; both outputs must be NULL in "
                                    "Neyman mode");
    if (h->xf_running) return fail(VP_ERR_INVALID, "vp_poisson_reweight during a stepped fit");
    if (!h->d_w || !(h->flags & VP_FLAG_W_PER_PROBLEM))
        return fail(VP_ERR_INVALID, "vp_poisson_reweight: the handle must be created with VP_FLAG_W_PER_PROBLEM and a weights array");
    if (h->S != 1)
        return fail(VP_ERR_UNSUPPORTED, "vp_poisson_reweight: weights are per problem, not per right-hand side (S = 1 only)");
    if (h->m_user) return fail(VP_ERR_UNSUPPORTED, "vp_poisson_reweight: not available on a handle padded for m < n");
    if (model) {
        if (!h->have_params) return fail(VP_ERR_INVALID, "vp_poisson_reweight: model mode needs the fit of the current parameters (no parameters set yet)");
        if (h->external && !h->ext_phi)
            return fail(VP_ERR_INVALID, "vp_poisson_reweight: model mode needs the columns of the handle's current parameters "
                                        "(vp_set_params_with_basis at the fitted parameters first)");
        if (!h->kern->best_fit) return fail(VP_ERR_UNSUPPORTED, "no best_fit kernel for this model");
    }
    const size_t bytes = (size_t)h->B * h->m * tsize(h->dtype);
    InBuf y;
    OutBuf dev, pear;
    if (int rc = y.init(h, Y, bytes)) return rc;
    if (int rc = dev.init(h, deviance_out, (size_t)h->B * sizeof(double))) return rc;
    if (int rc = pear.init(h, pearson_out, (size_t)h->B * sizeof(double))) return rc;
    if (model) {
        if (int rc = h->ensure(h->d_pfit, bytes)) return rc;
        if (int rc = launch_best_fit(h, h->d_pfit)) return rc;
    }
    PoissonParams p;
    p.dtype = h->dtype;
    p.Y = y.dptr;
    p.F = model ? h->d_pfit : nullptr;
    p.status = h->d_status;
    p.w = h->d_w;
    p.yw = h->d_yw;
    p.deviance = (double *)dev.dptr;
    p.pearson = (double *)pear.dptr;
    p.floor = floor;
    p.m = (int)h->m;
    p.B = h->B;
    p.stream = h->stream;
    if (int rc = poisson_reweight_launch(p)) return fail(rc, "Poisson re-weighting kernel launch failed");
    // the cached evaluation belongs to the old weights; the parameters stay (vp_params), the next vp_fit can start from them
    const bool had_alpha = h->have_params || h->alpha_kept;
    invalidate(h);
    h->alpha_kept = had_alpha;
    if (int rc = dev.finish(h)) return rc;
    if (int rc = pear.finish(h)) return rc;
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream)); // the staged counts go out of scope
    return VP_ERR_OK;
}

// robust re-weighting on the device (vp_robust.hpp): the preconditions and the afterwards of vp_poisson_reweight in model mode
int vp_robust_reweight(vp_batch *h, const void *Y, const void *w0, int loss, double tuning, double scale, double *scale_out,
                       double *rho_out) {
    VP_ENTER(h);
    if (!Y) return fail(VP_ERR_INVALID, "vp_robust_reweight: null Y");
    if (loss != VP_ROBUST_HUBER && loss != VP_ROBUST_CAUCHY && loss != VP_ROBUST_TUKEY)
        return fail(VP_ERR_INVALID, "vp_robust_reweight: unknown loss");
    if (!(tuning >= 0.0) || !std::isfinite(tuning))
        return fail(VP_ERR_INVALID, "vp_robust_reweight: the tuning constant must be finite and > 0 (0: the 95 % efficiency value)");
    if (!(scale >= 0.0) || !std::isfinite(scale))
        return fail(VP_ERR_INVALID, "vp_robust_reweight: the scale must be finite and > 0 (0: the normalised median of |e| per problem)");
    if (h->xf_running) return fail(VP_ERR_INVALID, "vp_robust_reweight during a stepped fit");
    if (!h->d_w || !(h->flags & VP_FLAG_W_PER_PROBLEM))
        return fail(VP_ERR_INVALID, "vp_robust_reweight: the handle must be created with VP_FLAG_W_PER_PROBLEM and a weights array");
    if (h->S != 1)
        return fail(VP_ERR_UNSUPPORTED, "vp_robust_reweight: weights are per problem, not per right-hand side (S = 1 only)");
    if (h->m_user) return fail(VP_ERR_UNSUPPORTED, "vp_robust_reweight: not available on a handle padded for m < n");
    if (!h->have_params) return fail(VP_ERR_INVALID, "vp_robust_reweight needs the fit of the current parameters (no parameters set yet)");
    if (h->external && !h->ext_phi)
        return fail(VP_ERR_INVALID, "vp_robust_reweight needs the columns of the handle's current parameters "
                                    "(vp_set_params_with_basis at the fitted parameters first)");
    if (!h->kern->best_fit) return fail(VP_ERR_UNSUPPORTED, "no best_fit kernel for this model");
    static const double k95[3] = {1.345, 2.385, 4.685}; // 95 % efficiency at the normal distribution
    const size_t bytes = (size_t)h->B * h->m * tsize(h->dtype);
    InBuf y, base;
    OutBuf sc, rho;
    if (int rc = y.init(h, Y, bytes)) return rc;
    if (int rc = base.init(h, w0, bytes)) return rc;
    if (int rc = sc.init(h, scale_out, (size_t)h->B * sizeof(double))) return rc;
    if (int rc = rho.init(h, rho_out, (size_t)h->B * sizeof(double))) return rc;
    if (int rc = h->ensure(h->d_pfit, bytes)) return rc;
    if (int rc = launch_best_fit(h, h->d_pfit)) return rc;
    RobustParams p;
    p.dtype = h->dtype;
    p.Y = y.dptr;
    p.F = h->d_pfit;
    p.w0 = base.dptr;
    p.status = h->d_status;
    p.w = h->d_w;
    p.yw = h->d_yw;
    p.scale_out = (double *)sc.dptr;
    p.rho_out = (double *)rho.dptr;
    p.loss = loss;
    p.k = tuning == 0.0 ? k95[loss] : tuning;
    p.scale = scale;
    p.m = (int)h->m;
    p.B = h->B;
    p.stream = h->stream;
    if (int rc = robust_reweight_launch(p)) return fail(rc, "robust re-weighting kernel launch failed");
    // the cached evaluation belongs to the old weights; the parameters stay (vp_params), the next vp_fit can start from them
    const bool had_alpha = h->have_params || h->alpha_kept;
    invalidate(h);
    h->alpha_kept = had_alpha;
    if (int rc = sc.finish(h)) return rc;
    if (int rc = rho.finish(h)) return rc;
    if (!device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream)); // the staged arrays go out of scope
    return VP_ERR_OK;
}

int vp_weights(vp_batch *h, void *w_out) {
    VP_ENTER(h);
    if (!w_out) return fail(VP_ERR_INVALID, "vp_weights: null output");
    if (!h->d_w) return fail(VP_ERR_INVALID, "vp_weights: the handle was created without weights");
    return copy_out_rows(h, w_out, h->d_w, (h->flags & VP_FLAG_W_PER_PROBLEM) ? (size_t)h->B : (size_t)1);
}

int vp_statistics(vp_batch *h, void *cov_out, double *reduced_chi2_out, void *conf_sigma_out, int32_t *status) {
    VP_ENTER(h);
    if (!h->have_params) return fail(VP_ERR_INVALID, "no parameters set yet");
    if (h->S != 1) // src/solvers/levmar/mod.rs:271-273: statistics are single-RHS only
        return fail(VP_ERR_UNSUPPORTED, "fit statistics are only supported for a single right-hand side");
    if (!h->kern->stats) return fail(VP_ERR_UNSUPPORTED, "no statistics kernel for this model");
    if (h->external && h->ext_np > 0 && !h->ext_dphi)
        return fail(VP_ERR_INVALID, "fit statistics need the derivative columns at the current parameters (vp_set_params_with_basis with dPhi)");
    if (int rc = ensure_gen_ws(h)) return rc;
    if (!cov_out || !reduced_chi2_out) return fail(VP_ERR_INVALID, "null output");
    const size_t ts = tsize(h->dtype);
    const int k = h->n + h->q;
    OutBuf cov, chi2;
    RowOut sig;
    StatusOut st; // (declared last: its temporary is the first to go)
    if (int rc = cov.init(h, cov_out, (size_t)h->B * k * k * ts)) return rc;
    if (int rc = chi2.init(h, reduced_chi2_out, (size_t)h->B * sizeof(double))) return rc;
    if (int rc = sig.init(h, conf_sigma_out, (size_t)h->B)) return rc;
    if (int rc = st.init(h, status)) return rc;
    LaunchParams p;
    fill_params(h, p);
    p.C_out = h->d_C;
    p.cost_out = h->d_cost;
    p.status = h->d_status;
    p.cov_out = cov.dptr;
    p.chi2_out = (double *)chi2.dptr;
    p.sigma_out = sig.dptr;
    p.stats_status = st.dev;
    int rc = h->kern->stats(p);
    if (rc == VP_ERR_OK) rc = cov.finish(h);
    if (rc == VP_ERR_OK) rc = chi2.finish(h);
    if (rc == VP_ERR_OK) rc = sig.finish(h);
    if (rc == VP_ERR_OK) rc = st.finish(h, status);
    if (rc != VP_ERR_OK) return fail(rc, "statistics kernel failed");
    return VP_ERR_OK;
}

// == FitStatistics::try_calculate on the stacked single-RHS equivalent of a global fit (vp_gstats.hpp).  Problems go in
// chunks whose workspace (basis columns + the kernels' row workspaces) stays within kGsWsBytes.
int vp_global_statistics(vp_batch *h, void *cov_alpha_out, double *reduced_chi2_out, void *coef_cov_out,
                         void *coef_alpha_cov_out, void *conf_sigma_out, int32_t *status) {
    VP_ENTER(h);
    if (!h->have_params) return fail(VP_ERR_INVALID, "no parameters set yet");
    if (h->rhs_allreduce)
        return fail(VP_ERR_UNSUPPORTED, "global fit statistics of right-hand sides sharded over ranks (vp_set_rhs_allreduce) "
                                        "need a cross-rank reduction vp_global_statistics does not make");
    if (!cov_alpha_out || !reduced_chi2_out) return fail(VP_ERR_INVALID, "null output");
    if (h->external && !h->ext_phi)
        return fail(VP_ERR_INVALID, "global fit statistics need the columns at the current parameters (vp_set_params_with_basis "
                                    "with Phi and dPhi)");
    if (h->external && h->ext_np > 0 && !h->ext_dphi)
        return fail(VP_ERR_INVALID, "global fit statistics need the derivative columns at the current parameters "
                                    "(vp_set_params_with_basis with dPhi)");
    if (h->n > VP_MAX_BASIS || h->q > VP_MAX_PARAMS || h->p > VP_MAX_PAIRS || h->S > 0x7fffffff)
        return fail(VP_ERR_UNSUPPORTED, "global fit statistics: shape out of range");
    GStatsParams gp;
    std::memset(&gp, 0, sizeof(gp));
    gp.dtype = h->dtype;
    gp.n = h->n;
    gp.q = h->q;
    if (h->external) {
        gp.P = h->ext_np;
        for (int i = 0; i < h->ext_np; ++i) {
            gp.pb[i] = h->ext_pb[i];
            gp.pp[i] = h->ext_pp[i];
        }
    } else { // the descriptor's pairs in vp_basis' order (basis-major, argument slot within a basis)
        for (int j = 0; j < h->n; ++j)
            for (int k = 0; k < VP_MAX_BASIS_PARAMS; ++k)
                if (h->model.param[j][k] >= 0) {
                    gp.pb[gp.P] = j;
                    gp.pp[gp.P] = h->model.param[j][k];
                    ++gp.P;
                }
    }
    const size_t ts = tsize(h->dtype);
    const int64_t m = h->m, S = h->S, B = h->B, n = h->n, q = h->q, P = gp.P;
    gp.m = (int)m;
    gp.rows = h->external ? (int)(h->m_user ? h->m_user : m) : (int)m;
    gp.m_dof = h->m_user ? h->m_user : m;
    gp.S = (int)S;
    gp.w_stride = (h->flags & VP_FLAG_W_PER_PROBLEM) ? m : 0;
    gp.stream = h->stream;
    const bool band = conf_sigma_out != nullptr;
    // bytes of one problem's workspace: basis columns (descriptor handles) + prep columns + row constants + the small record
    const size_t per_b = (h->external ? 0 : (size_t)(n + P) * m * ts) + (size_t)(n + P) * m * 8 +
                         (band ? (size_t)(1 + n * (n + 1) / 2) * m * 8 : 0) + gs::kGsSmall * 8;
    constexpr size_t kGsWsBytes = (size_t)1 << 30;
    const int64_t bc = std::max<int64_t>(1, std::min<int64_t>(B, (int64_t)(kGsWsBytes / per_b)));
    OutBuf cov, chi2, cc, ca;
    RowOut sig;
    if (int rc = cov.init(h, cov_alpha_out, (size_t)B * q * q * ts)) return rc;
    if (int rc = chi2.init(h, reduced_chi2_out, (size_t)B * sizeof(double))) return rc;
    if (int rc = cc.init(h, coef_cov_out, (size_t)B * S * n * n * ts)) return rc;
    if (int rc = ca.init(h, coef_alpha_cov_out, (size_t)B * S * n * q * ts)) return rc;
    if (int rc = sig.init(h, conf_sigma_out, (size_t)B * S)) return rc;
    DevMem ws; // freed on every path, after the status temporary and before the output staging
    StatusOut st;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t sz_basis = h->external ? 0 : al((size_t)bc * (n + P) * m * ts), sz_cols = al((size_t)bc * (n + P) * m * 8),
                 sz_rows = band ? al((size_t)bc * (1 + n * (n + 1) / 2) * m * 8) : 0, sz_small = (size_t)bc * gs::kGsSmall * 8;
    if (int rc = ws.alloc(sz_basis + sz_cols + sz_rows + sz_small)) return rc;
    if (int rc = st.init(h, status)) return rc;
    char *wsb = (char *)ws.p;
    void *basis_ws = h->external ? nullptr : wsb;
    gp.ws_cols = (double *)(wsb + sz_basis);
    gp.ws_rows = band ? (double *)(wsb + sz_basis + sz_cols) : nullptr;
    gp.ws_small = (double *)(wsb + sz_basis + sz_cols + sz_rows);
    const char *wdev = (const char *)h->d_w;
    for (int64_t b0 = 0; b0 < B; b0 += bc) {
        const int64_t nb = std::min<int64_t>(bc, B - b0);
        if (h->external) {
            gp.phi = (const char *)h->ext_phi + (size_t)b0 * n * gp.rows * ts;
            gp.dphi = h->ext_dphi ? (const char *)h->ext_dphi + (size_t)b0 * P * gp.rows * ts : nullptr;
        } else { // the unweighted columns of this chunk at the handle's parameters: the set's own vp_basis kernel
            LaunchParams p;
            fill_params(h, p);
            p.B = nb;
            p.alpha = (const char *)h->d_alpha + (size_t)b0 * q * ts;
            p.t = (const char *)h->d_t + (size_t)b0 * p.t_stride * ts;
            p.w = h->d_w ? wdev + (size_t)b0 * p.w_stride * ts : nullptr;
            p.Phi_out = basis_ws;
            p.dPhi_out = (char *)basis_ws + (size_t)nb * n * m * ts;
            p.basis_flags = 0;
            if (int rc = h->kern->basis(p)) return fail(rc, "basis kernel launch failed");
            gp.phi = p.Phi_out;
            gp.dphi = P > 0 ? p.dPhi_out : nullptr;
        }
        gp.B = nb;
        gp.w = h->d_w ? wdev + (size_t)b0 * gp.w_stride * ts : nullptr;
        gp.C = (const char *)h->d_C + (size_t)b0 * S * n * ts;
        gp.cost = h->d_cost + b0;
        gp.status_in = h->d_status + b0;
        gp.cov_alpha = (char *)cov.dptr + (size_t)b0 * q * q * ts;
        gp.chi2 = (double *)chi2.dptr + b0;
        gp.coef_cov = cc.dptr ? (char *)cc.dptr + (size_t)b0 * S * n * n * ts : nullptr;
        gp.coef_alpha_cov = ca.dptr ? (char *)ca.dptr + (size_t)b0 * S * n * q * ts : nullptr;
        gp.band = sig.dptr ? (char *)sig.dptr + (size_t)b0 * S * m * ts : nullptr;
        gp.status_out = st.dev + b0;
        if (int rc = gstats_launch(gp)) return fail(rc, "global statistics kernels failed");
    }
    if (int rc = cov.finish(h)) return rc;
    if (int rc = chi2.finish(h)) return rc;
    if (int rc = cc.finish(h)) return rc;
    if (int rc = ca.finish(h)) return rc;
    if (int rc = sig.finish(h)) return rc;
    if (int rc = st.finish(h, status)) return rc;
    if (device_ptrs(h)) VP_HIP(hipStreamSynchronize(h->stream)); // (the workspace is freed on return)
    return VP_ERR_OK;
}

int vp_summary(vp_batch *h, double out[4]) {
    VP_ENTER(h);
    if (!h->have_report) return fail(VP_ERR_INVALID, "vp_summary requires a completed vp_fit");
    if (int rc = launch_summary(h, h->d_sum4)) return rc;
    return read_sum4(h, out);
}

// cond(J D^-1) as the Gram-based LM step of the last global fit saw it at its worst (MrhsWs::jcond)
int vp_global_fit_condition(vp_batch *h, double *cond_out) {
    VP_ENTER(h);
    if (!cond_out) return fail(VP_ERR_INVALID, "null output");
    if (!h->have_mrhs || !h->mrhs.jcond || !h->have_report)
        return fail(VP_ERR_INVALID, "vp_global_fit_condition requires a completed vp_fit on a handle with several right-hand sides "
                                    "(specialised kernel set)");
    return copy_out(h, cond_out, h->mrhs.jcond, (size_t)h->B * sizeof(double));
}

int vp_summary_device(vp_batch *h, double *dev_out4) {
    VP_ENTER(h);
    if (!h->have_report) return fail(VP_ERR_INVALID, "vp_summary_device requires a completed vp_fit");
    if (!dev_out4) return fail(VP_ERR_INVALID, "null output");
    return launch_summary(h, dev_out4);
}

// == the vp_reduce_cost of SURVEY.md 8(b): local aggregates + ONE RCCL all-reduce of 4 doubles on the handle's stream.
// RCCL is resolved at run time (the library itself does not link it).
typedef int (*vp_nccl_allreduce_t)(const void *, void *, size_t, int, int, void *, hipStream_t);
static vp_nccl_allreduce_t resolve_nccl_allreduce() {
    static vp_nccl_allreduce_t fn = nullptr;
    static bool tried = false;
    if (!tried) {
        tried = true;
        void *sym = dlsym(RTLD_DEFAULT, "ncclAllReduce"); // the host process links / has loaded RCCL
        if (!sym) {
            void *lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (lib) sym = dlsym(lib, "ncclAllReduce");
        }
        fn = reinterpret_cast<vp_nccl_allreduce_t>(sym);
    }
    return fn;
}

int vp_reduce_cost(vp_batch *h, void *rccl_comm, double out[4]) {
    VP_ENTER(h);
    if (!out) return fail(VP_ERR_INVALID, "null output");
    if (!h->have_report) return fail(VP_ERR_INVALID, "vp_reduce_cost requires a completed vp_fit");
    if (int rc = launch_summary(h, h->d_sum4)) return rc;
    if (rccl_comm) {
        vp_nccl_allreduce_t ar = resolve_nccl_allreduce();
        if (!ar) return fail(VP_ERR_UNSUPPORTED, "ncclAllReduce not found: link librccl or make librccl.so.1 loadable");
        const int rc = ar(h->d_sum4, h->d_sum4, 4, /*ncclDouble*/ 8, /*ncclSum*/ 0, rccl_comm, h->stream);
        if (rc != 0) return fail(VP_ERR_HIP, "ncclAllReduce failed with code " + std::to_string(rc));
    }
    return read_sum4(h, out);
}

int vp_set_fit_kernel(vp_batch *h, int which) {
    if (!h) return fail(VP_ERR_INVALID, "null handle");
    if (which != VP_FIT_KERNEL_AUTO && which != VP_FIT_KERNEL_WAVE && which != VP_FIT_KERNEL_SLOTS)
        return fail(VP_ERR_INVALID, "vp_set_fit_kernel: unknown kernel selector");
    h->fit_kernel = which;
    return VP_ERR_OK;
}

int vp_set_timing(vp_batch *h, int enable) {
    if (!h) return fail(VP_ERR_INVALID, "null handle");
    h->timing = enable != 0;
    return VP_ERR_OK;
}

int vp_last_kernel_ms(vp_batch *h, int which, float *ms) {
    if (!h || !ms || which < 0 || which > 2) return fail(VP_ERR_INVALID, "bad argument");
    *ms = h->last_ms[which];
    return VP_ERR_OK;
}

int vp_synchronize(vp_batch *h) {
    VP_ENTER(h);
    VP_HIP(hipStreamSynchronize(h->stream));
    return VP_ERR_OK;
}

} // extern "C"

// ---- registry ------------------------------------------------------------------------------------------
namespace vp {

std::vector<KernelEntry> &registry() {
    static std::vector<KernelEntry> r;
    return r;
}

static int kind_arity(int kind) {
    switch (kind) {
    case VP_BASIS_CONST: return 0;
    case VP_BASIS_EXP_DECAY:
    case VP_BASIS_EXP_RATE: return 1;
    case VP_BASIS_EXP_COS:
    case VP_BASIS_SIN_PHASE: return 2;
    case VP_BASIS_GAUSS:
    case VP_BASIS_LORENTZ: return 2;
    case VP_BASIS_LINEAR: return 0;
    case VP_BASIS_EXP_DECAY_IRF: return 1;
    case VP_BASIS_IRF: return 0;
    case VP_BASIS_EXP_DECAY_IRF_PERIODIC: return 1;
    case VP_BASIS_EXP_DECAY_IRF_SHIFT: return 2;
    case VP_BASIS_IRF_SHIFT: return 1;
    case VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT: return 2;
    default: return -1; // (VP_BASIS_EXTERNAL never reaches a descriptor: vp_batch_create_external only)
    }
}

int classify_model(const vp_model_desc &d, int &a, int &b, int &c, int &p_out) {
    int pairs = 0;
    for (int j = 0; j < d.n_basis; ++j) {
        const int ar = kind_arity(d.kind[j]);
        if (ar < 0) return -1;
        for (int k = 0; k < VP_MAX_BASIS_PARAMS; ++k) {
            const int pi = d.param[j][k];
            if (k < ar) {
                if (pi < 0 || pi >= d.n_params) return -1;
                ++pairs;
            } else if (pi >= 0) {
                return -1;
            }
        }
    }
    p_out = pairs;
    // multi-exponential family: exp(-t/alpha_j) for j = 0..q-1 in order, optional trailing constant
    bool multiexp = d.n_params >= 1 && (d.n_basis == d.n_params || d.n_basis == d.n_params + 1);
    if (multiexp) {
        for (int j = 0; j < d.n_params; ++j)
            if (d.kind[j] != VP_BASIS_EXP_DECAY || d.param[j][0] != j) multiexp = false;
        if (multiexp && d.n_basis == d.n_params + 1 && d.kind[d.n_params] != VP_BASIS_CONST) multiexp = false;
    }
    if (multiexp) {
        a = d.n_params;
        b = d.n_basis - d.n_params;
        c = 0;
        return FAMILY_MULTIEXP;
    }
    a = d.n_basis;
    b = d.n_params;
    c = pairs;
    return FAMILY_RT;
}

const KernelEntry *find_kernels(int dtype, const vp_model_desc &d, int64_t m, int64_t S, bool weighted) {
    int a, b, c, p;
    const int fam = classify_model(d, a, b, c, p);
    if (fam < 0) return nullptr;
    const KernelEntry *best = nullptr;
    // pass 0: exact family; pass 1: a multi-exponential model may also run on the runtime-model kernels -- where its own
    // family has no set for m, and also where it only has the length-agnostic one: that set loses against every resident set
    // that covers m (vp_inst_blk.hpp), whichever family registered it (triple exponential without offset at 128 < m <= 1024)
    for (int pass = 0; pass < 2 && (!best || best->uses_gen_ws); ++pass) {
        int f = fam, ka = a, kb = b, kc = c;
        if (pass == 1) {
            if (fam != FAMILY_MULTIEXP) break;
            f = FAMILY_RT;
            ka = d.n_basis;
            kb = d.n_params;
            kc = p;
        }
        for (const KernelEntry &e : registry()) {
            if (e.dtype != dtype || e.family != f || e.a != ka || e.b != kb || e.c != kc) continue;
            if ((int64_t)64 * e.R * e.W < m) continue;
            if (S == 1 && !e.evaluate) continue; // (a set that only carries multiple-right-hand-side kernels)
            // weighted problems: grid + weights + data column of 64 R W rows each must fit the 160 KiB of LDS the
            // one-problem-per-group fit kernel stages them in (KernelEntry::fit_lds_w: launch_fit's own expression)
            if (weighted && e.fit_lds_w > (size_t)160 * 1024) continue;
            // smallest capacity first.  Among equal capacities: a multiple-RHS handle takes the set that has MRHS kernels;
            // a single-RHS handle the one whose columns fit the registers (R <= 16 rows per lane -- the R = 32 sets spill
            // hundreds of VGPRs: triple exponential at m = 2048, 0.71 vs 0.10 ms per 16384 evaluations at m = 1024), else
            // the fewest waves per problem
            auto better = [&](const KernelEntry &x, const KernelEntry &y) {
                if (x.R * x.W != y.R * y.W) return x.R * x.W < y.R * y.W;
                if (S > 1 && (x.mrhs_stream != nullptr) != (y.mrhs_stream != nullptr)) return x.mrhs_stream != nullptr;
                if (S == 1 && (x.R <= 16) != (y.R <= 16)) return x.R <= 16;
                return x.W < y.W;
            };
            if (!best || better(e, *best)) best = &e;
        }
    }
    return best;
}

} // namespace vp
