/*
 * varpro_hip_debug.h -- TEST HOOKS of libvarpro_hip.so.  Not part of the drop-in boundary (include/varpro_hip.h): these
 * two entries expose intermediate quantities of one kernel family to the parity tests (tests/test_gpu_gram_parity.py,
 * tests/test_gpu_lmpar_gram.py) and replace nothing in the reference.  A binding of the reference does not need them.
 */
#ifndef VARPRO_HIP_DEBUG_H
#define VARPRO_HIP_DEBUG_H

#include "varpro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Diagnostics for the fixed-alpha parity tests of the fp64-Gram fit kernel (VP_F32 handles whose fit runs on the normal
 * equations in double, see vp_set_fit_kernel): evaluates that kernel's formulation ONCE at alpha [B][q] and writes, per
 * problem, out[b] = { 1/2 ||r||^2, c (n), J^T r (q), J^T J (q x q, row-major) } as f64 -- the quantities the kernel
 * hands to its LM step, i.e. set_params + residuals + jacobian (src/solvers/levmar/mod.rs:42-73, 101-201) contracted
 * the way the LM driver consumes them.  Does not touch the handle's cached state.  VP_ERR_UNSUPPORTED for handles whose
 * fit does not use the Gram kernel.  `out` follows the handle's address space.
 */
int vp_debug_gram_evaluate(vp_batch *h, const void *alpha, double *out);

/*
 * Diagnostics for the parity test of the Gram fit kernel's LM step: the trust-region sub-problem of
 * LevenbergMarquardt::minimize (levenberg-marquardt 0.14 == MINPACK lmpar; call site src/solvers/levmar/mod.rs:247) as that
 * kernel solves it -- on the Cholesky factor of R^T R + par D^2 instead of qrsolv's Givens rotations (lmpar_chol,
 * varpro_amd/csrc/vp_fit.hpp) -- run once per record on the device.  HOST pointers; q in {2, 3, 5}.
 *   Rj [B][q][q] row-major upper-triangular factor of the pivoted Jacobian, ipvt [B][q], diag [B][q], qtb [B][q] (first q
 *   entries of Q^T f), delta [B], par_in [B]  ->  out [B][q + 2] = { par, ||diag .* step||, step (q, unpivoted order) }.
 */
int vp_debug_lmpar_gram(int64_t B, int q, const double *Rj, const int32_t *ipvt, const double *diag, const double *qtb,
                        const double *delta, const double *par_in, double *out);

/*
 * Diagnostics for the flag-and-refit tests: enabled != 0 (the default) lets vp_fit re-fit, in a second launch with
 * power-of-two column scaling, the problems whose Jacobian factor is not representable column by column -- the reference
 * forms D_k c before it projects (src/solvers/levmar/mod.rs:156-171); 0 returns what the fit kernels themselves report for
 * them (VP_TERM_NUMERICAL, parameters = the last accepted point).  Single-right-hand-side descriptor handles only.
 */
int vp_debug_set_refit(vp_batch *h, int enabled);

/*
 * Measurement switches of a device-column handle (VP_BASIS_GAUSS / _LORENTZ / _LINEAR; tools/peak_kinds_probe.py):
 * look_every >= 1: vp_fit reads the active count every look_every steps (default 8); results do not depend on it.
 * nontemporal: stores of the column kernel, 1 (default) non-temporal, 0 ordinary; values do not depend on it.
 */
int vp_debug_set_column_fit(vp_batch *h, int look_every, int nontemporal);

/*
 * Measurement of vp_search's shared route (tools/search_probe.py): with vp_set_timing(h, 1) the last vp_search leaves the
 * hipEvent times of its four stages in ms_out -- { candidate columns, orthonormalisation, ranking product, evaluation at
 * the winners } -- in milliseconds; -1 before the first such call.
 */
int vp_debug_search_ms(vp_batch *h, float ms_out[4]);

/*
 * Which compiled kernel set a handle runs on (tests/stats_cases.py: every case names the set it is meant to reach).
 * out = { dtype (VP_F64 / VP_F32), family, a, b, c, R, W, uses_gen_ws } of the handle's set:
 *   family 1: multi-exponential, (a, b, c) = (exponentials, offset 0/1, 0);  family 2: run-time descriptor, (a, b, c) =
 *   (basis functions, parameters, pairs);  family 3: the generic kernels (a = b = c = R = 0; caller-evaluated handles too);
 *   R rows per lane, W waves per problem: the set holds m <= 64 R W;  uses_gen_ws = 1 with family 1 or 2: a
 *   length-agnostic set (R = 2^20), whose statistics and best fit run on the generic kernels.
 * A plain read: no GPU work, no state.
 */
int vp_debug_kernel_set(vp_batch *h, int32_t out[8]);

/*
 * The same record for entry `index` of the table of registered sets, without a handle and without a device.  Returns 1
 * if the entry carries both an evaluation and a statistics kernel, i.e. a single-right-hand-side handle can land on it,
 * 0 if it serves handles with several right-hand sides only, VP_ERR_INVALID past the end of the table.
 */
int vp_debug_registry_entry(int index, int32_t out[8]);

/*
 * Which fit kernel the handle's last single-right-hand-side vp_fit / vp_fit_trace launched, written by the launcher that
 * issued the launch (so a slot-kernel launcher that hands the batch to the wave kernel reports the wave kernel):
 * out = { kernel, padding, weighted, 0 }
 *   kernel    0 = no fit yet, 1 = wave (one problem per wave group, vp_fit.hpp), 2 = slots (vp_fit2.hpp), 3 = Gram
 *             (vp_fitg.hpp: fp32 handle, fp64 Gram matrix), 4 = row-block / length-agnostic (vp_block.hpp), 5 = generic
 *   padding   the instantiation by length: 1 = m == 64 R W, 2 = m reaches the last register pair, 0 = general,
 *             -1 = not applicable (kernels 3, 4, 5)
 *   weighted  1 = the weighted instantiation (the Gram kernel's also masks a ragged last row group through the weights)
 * The re-fit of flagged problems is not recorded.  A plain read: no GPU work, no state.
 */
int vp_debug_last_fit(vp_batch *h, int32_t out[4]);

/*
 * The counterpart for handles with several right-hand sides (global fits, S > 1): what the launchers of that path issued
 * for the handle's vp_evaluate / vp_set_params / vp_residuals / vp_jacobian and vp_fit / vp_fit_trace calls so far, each
 * field written by the launcher that issued the launch:
 * out = { factor_waves, step_waves, fit_stream, eval_stream, gx_fit, gx_eval, 0, 0 }
 *   factor_waves  waves per problem of the factor kernel of the last evaluation: 1 or 4; 0 = none yet (a fit factors inside
 *                 its step kernel and leaves this field alone)
 *   step_waves    waves per problem of the LM step kernel of the last fit: 1 or 4; 0 = no fit yet
 *   fit_stream    the kernel of the fit's pass over the data columns, eval_stream that of the last evaluation:
 *                 0 = none yet, 1 = mrhs_stream_kernel, 2 = mrhs_coop_dma_kernel, 3 = mrhs_coop_out_kernel with J,
 *                 4 = mrhs_coop_out_kernel without J, 5 = the generic kernels (vp_generic.hpp)
 *   gx_fit, gx_eval  workgroups per problem of that pass (0 with the generic kernels)
 * A fit that replays a captured graph runs its launchers when the graph is captured, not when it is replayed: the record
 * is then that of the capture, which took the same decisions (the graph is captured for this handle's shapes and re-captured
 * when the options change).  A plain read: no GPU work, no state.
 */
int vp_debug_last_global(vp_batch *h, int32_t out[8]);

/*
 * Whether entry `index` of the table of registered sets carries the kernels of the multiple-right-hand-side path (factor,
 * stream, LM step, finish), i.e. a handle with S > 1 can land on it: 1 / 0, VP_ERR_INVALID past the end of the table.
 * Same index as vp_debug_registry_entry, whose record names the set.  No handle, no device.
 */
int vp_debug_registry_has_global(int index);

#ifdef __cplusplus
}
#endif
#endif /* VARPRO_HIP_DEBUG_H */
