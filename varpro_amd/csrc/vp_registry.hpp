// vp_registry.hpp -- table of compiled kernel instantiations and its lookup; plain host C++ (builders: vp_inst.hpp, vp_inst_blk.hpp)
#pragma once
#include <vector>

#include "../../include/varpro_hip.h"

namespace vp {

struct LaunchParams; // vp_kernels.hpp
typedef int (*launch_fn)(const LaunchParams &);

enum { FAMILY_MULTIEXP = 1, FAMILY_RT = 2, FAMILY_GENERIC = 3 };

constexpr int kMrhsGxCapDefault = 256; // MRHS streaming kernel: workgroups per problem of a set that names no cap of its own
// every launcher may be null (the set has no such kernel); an entry starts value-initialised and is filled by name
struct KernelEntry {
    int dtype;  // VP_F64 / VP_F32
    int family; // FAMILY_*
    int a, b, c; // MULTIEXP: (nexp, offset, 0)   RT: (n, q, p)
    int R;      // rows per lane
    int W;      // waves per problem; handles m <= 64*R*W
    launch_fn evaluate;
    launch_fn basis;
    launch_fn fit;      // persistent slot LM kernel (vp_fit2.hpp; falls back to fit_single by itself)
    launch_fn fit_single; // one-wavefront(-group)-per-problem LM (vp_fit.hpp)
    launch_fn fit_rescue; // fast re-fit of the problems fit_single flagged (fit_kernel<..., RESCUE>, vp_fit.hpp)
    launch_fn best_fit;
    // multiple-right-hand-side path (vp_mrhs.hpp); all null if not instantiated
    launch_fn mrhs_factor, mrhs_stream, mrhs_lm, mrhs_finish;
    size_t mrhs_state_bytes;
    launch_fn stats; // batched fit statistics (vp_stats.hpp)
    launch_fn mrhs_fit_whole; // S > 1 fit as ONE launch (generic fallback kernels only; null elsewhere)
    int gram_fit;       // 1: `fit` is the fp64-Gram kernel (vp_fitg.hpp), which also serves vp_debug_gram_evaluate
    int mrhs_gx_cap;    // MRHS streaming kernel: max workgroups (partial-sum slots) per problem; 0 = kMrhsGxCapDefault
    size_t fit_lds_w;   // dynamic LDS the single-RHS fit kernel needs for a WEIGHTED problem (0: not recorded, fits)
    int uses_gen_ws;    // 1: evaluate / stats / global fits of this set run on the generic kernels (vp_generic.hpp) and need
                        // their global-memory workspace (the generic set itself; the length-agnostic sets of vp_block.hpp)

    int gx_cap() const { return mrhs_gx_cap > 0 ? mrhs_gx_cap : kMrhsGxCapDefault; }
};
inline bool has_mrhs_set(const KernelEntry *k) { return k->mrhs_factor && k->mrhs_stream && k->mrhs_lm && k->mrhs_finish; }

std::vector<KernelEntry> &registry();

struct Registrar {
    explicit Registrar(const KernelEntry &e) { registry().push_back(e); }
};

// classify a public descriptor; returns family and its key (a,b,c); p_out = number of dependency pairs
int classify_model(const vp_model_desc &d, int &a, int &b, int &c, int &p_out);

// S: right-hand sides of the handle -- among sets of equal capacity a single-RHS handle prefers the one whose columns fit
// the registers (R <= 16: more waves per problem), a multiple-RHS handle the one that has MRHS kernels
// weighted: sets whose fit kernel cannot stage grid + weights + data of a weighted problem in the CU's LDS are skipped
const KernelEntry *find_kernels(int dtype, const vp_model_desc &d, int64_t m, int64_t S = 1, bool weighted = false);
// kernel set of a caller-evaluated model (vp_batch_create_external)
const KernelEntry *external_kernels(int dtype);
// true: an evaluation of this shape runs on a register-resident kernel (vp_ext.hpp) and needs no generic workspace
bool external_resident(int dtype, int n, int np, int64_t m, int64_t ext_rows, bool with_d);
// the generic fallback set (vp_generic.hpp): any descriptor, any m, single right-hand side fits
const KernelEntry *generic_kernels(int dtype);

} // namespace vp
