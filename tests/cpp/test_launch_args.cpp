// The fillers of the kernel argument records (varpro_amd/csrc: fill_fit_args, fill_eval_args) and the padding-variant rule
// seen from a host program: the kernel headers are compiled for the host only, nothing is launched, no GPU is needed.
//   (a) every field of a filled record holds the LaunchParams field the table below names for it (every field the fillers
//       read holds a distinct sentinel: pointers base + k, integers 1000 + k, options and eps 0.5 + k);
//   (b) a record that was all 0x00 bytes and one that was all 0xFF bytes are byte-identical after the fill, padding included;
//   (c) padding_variant against the three inequalities written out here.
//   prints "<n> failure(s)"; exit status 1 on any
#include <cstdio>
#include <cstring>

#include "../../varpro_amd/csrc/vp_fit.hpp"

using namespace vp;

static int failures = 0;
static void expect(bool ok, const char *who, const char *what) {
    if (ok) return;
    ++failures;
    std::printf("FAIL %s: %s\n", who, what);
}
#define EXPECT(cond) expect((cond), who, #cond)

static char base[64]; // the pointer sentinels point into this array (never dereferenced)
template <typename P> static P ptr(int k) { return reinterpret_cast<P>(base + k); }

static vp_lm_opts g_opts;
static vp_model_desc g_desc;

// every field fill_fit_args / fill_eval_args read, each with its own sentinel
static LaunchParams sentinel_params() {
    LaunchParams p;
    std::memset(&p, 0, sizeof p);
    g_opts.ftol = 0.5 + 1;
    g_opts.xtol = 0.5 + 2;
    g_opts.gtol = 0.5 + 3;
    g_opts.stepbound = 0.5 + 4;
    g_opts.patience = 1000 + 1;
    g_opts.scale_diag = 1000 + 2;
    p.model = &g_desc;
    p.opts = &g_opts;
    p.t = ptr<const void *>(1);
    p.w = ptr<const void *>(2);
    p.yw = ptr<const void *>(3);
    p.alpha = ptr<const void *>(4);
    p.alpha_out = ptr<void *>(5);
    p.r_out = ptr<void *>(6);
    p.J_out = ptr<void *>(7);
    p.C_out = ptr<void *>(8);
    p.cost_out = ptr<double *>(9);
    p.status = ptr<int32_t *>(10);
    p.report = ptr<vp_report *>(11);
    p.trace = ptr<double *>(12);
    p.rescue = ptr<int32_t *>(13);
    p.eps = 0.5 + 5;
    p.m = 1000 + 3;
    p.S = 1000 + 4;
    p.B = 1000 + 5;
    p.t_stride = 1000 + 6;
    p.w_stride = 1000 + 7;
    p.trace_rows = 1000 + 8;
    p.grid_uniform = 1000 + 9;
    p.rescue_slot = 1000 + 10;
    return p;
}

// the run-time descriptor of the test: exponential, constant, exponential -- parameters 1 and 0 (a constant that is NOT last,
// so that the fit record's constant-first sweep order differs from the model's order)
static void rt_descriptor(vp_model_desc &d) {
    std::memset(&d, 0, sizeof d);
    d.n_basis = 3;
    d.n_params = 2;
    for (int j = 0; j < VP_MAX_BASIS; ++j)
        for (int a = 0; a < VP_MAX_BASIS_PARAMS; ++a) d.param[j][a] = -1;
    d.kind[0] = VP_BASIS_EXP_DECAY;
    d.kind[1] = VP_BASIS_CONST;
    d.kind[2] = VP_BASIS_EXP_DECAY;
    d.param[0][0] = 1;
    d.param[2][0] = 0;
}
using Rt = RtModel<3, 2, 2>;
using Me = MultiExpModel<2, true>;

// the bound model of a record: nothing to check for a static model; the run-time one column by column.  `swept`: the fit
// record (constant column first, out_index() leads back to the model's order); else the model's own order
template <class M> static void check_model(const M &mdl, bool swept, const char *who) {
    if constexpr (!M::kStatic) {
        const int order[3] = {swept ? 1 : 0, swept ? 0 : 1, 2}; // column -> basis function of the descriptor
        for (int k = 0; k < 3; ++k) {
            EXPECT(mdl.out_index(k) == order[k]);
            EXPECT(mdl.kind(k) == g_desc.kind[order[k]]);
            for (int a = 0; a < VP_MAX_BASIS_PARAMS; ++a) EXPECT(mdl.param(k, a) == g_desc.param[order[k]][a]);
        }
        // pairs in the descriptor's order: (basis 0, parameter 1), (basis 2, parameter 0); pair_basis() names the COLUMN
        EXPECT(mdl.pair_basis(0) == (swept ? 1 : 0) && mdl.pair_arg(0) == 0 && mdl.pair_param(0) == 1);
        EXPECT(mdl.pair_basis(1) == 2 && mdl.pair_arg(1) == 0 && mdl.pair_param(1) == 0);
    } else {
        (void)mdl, (void)swept, (void)who;
    }
}

template <typename T, class M> static void check_fit(const char *who) {
    const LaunchParams p = sentinel_params();
    FitArgs<T, M> a, z;
    std::memset(&a, 0x00, sizeof a);
    std::memset(&z, 0xFF, sizeof z);
    EXPECT(fill_fit_args(p, a));
    EXPECT(fill_fit_args(p, z));
    EXPECT(std::memcmp(&a, &z, sizeof a) == 0); // (b)
    // (a): the table, from launch_fit
    check_model(a.mdl, true, who);
    EXPECT(a.t == ptr<const T *>(1));
    EXPECT(a.w == ptr<const T *>(2));
    EXPECT(a.yw == ptr<const T *>(3));
    EXPECT(a.alpha == ptr<T *>(5)); // alpha_out: the fit reads its guess from and writes its result to the same array
    EXPECT(a.C_out == ptr<T *>(8));
    EXPECT(a.cost_out == ptr<double *>(9));
    EXPECT(a.status == ptr<int32_t *>(10));
    EXPECT(a.report == ptr<vp_report *>(11));
    EXPECT(a.m == 1000 + 3);
    EXPECT(a.B == 1000 + 5);
    EXPECT(a.t_stride == 1000 + 6);
    EXPECT(a.w_stride == 1000 + 7);
    EXPECT(a.eps == (T)(0.5 + 5));
    EXPECT(a.lm.ftol == (T)(0.5 + 1));
    EXPECT(a.lm.xtol == (T)(0.5 + 2));
    EXPECT(a.lm.gtol == (T)(0.5 + 3));
    EXPECT(a.lm.stepbound == (T)(0.5 + 4));
    EXPECT(a.lm.patience == 1000 + 1);
    EXPECT(a.lm.scale_diag == 1000 + 2);
    EXPECT(a.trace == ptr<double *>(12));
    EXPECT(a.trace_rows == 1000 + 8);
    EXPECT(a.grid_uniform == 1000 + 9);
    EXPECT(a.rescue == ptr<int32_t *>(13));
    EXPECT(a.rescue_slot == 1000 + 10);
}

template <typename T, class M> static void check_eval(const char *who) {
    const LaunchParams p = sentinel_params();
    EvalArgs<T, M> a, z;
    std::memset(&a, 0x00, sizeof a);
    std::memset(&z, 0xFF, sizeof z);
    EXPECT(fill_eval_args(p, a));
    EXPECT(fill_eval_args(p, z));
    EXPECT(std::memcmp(&a, &z, sizeof a) == 0); // (b)
    // (a): the table, from launch_evaluate
    check_model(a.mdl, false, who);
    EXPECT(a.t == ptr<const T *>(1));
    EXPECT(a.w == ptr<const T *>(2));
    EXPECT(a.yw == ptr<const T *>(3));
    EXPECT(a.alpha == ptr<const T *>(4));
    EXPECT(a.r_out == ptr<T *>(6));
    EXPECT(a.J_out == ptr<T *>(7));
    EXPECT(a.C_out == ptr<T *>(8));
    EXPECT(a.cost_out == ptr<double *>(9));
    EXPECT(a.status == ptr<int32_t *>(10));
    EXPECT(a.m == 1000 + 3);
    EXPECT(a.S == 1000 + 4);
    EXPECT(a.nprob == (int64_t)(1000 + 5) * (1000 + 4)); // B * S
    EXPECT(a.t_stride == 1000 + 6);
    EXPECT(a.w_stride == 1000 + 7);
    EXPECT(a.eps == (T)(0.5 + 5));
    EXPECT(a.grid_uniform == 1000 + 9);
}

template <typename T> static void check_lm_opts(const char *who) {
    sentinel_params();
    const LmOpts<T> o = lm_opts_from<T>(g_opts);
    EXPECT(o.ftol == (T)(0.5 + 1) && o.xtol == (T)(0.5 + 2) && o.gtol == (T)(0.5 + 3) && o.stepbound == (T)(0.5 + 4));
    EXPECT(o.patience == 1000 + 1 && o.scale_diag == 1000 + 2);
}

static void check_padding_variant() {
    const char *who = "padding_variant";
    const int Rs[4] = {1, 2, 4, 16}, Ws[2] = {1, 4};
    for (int R : Rs)
        for (int W : Ws) {
            const int ms[5] = {64 * R * W, 64 * R * W - 1, 64 * (R - 2) * W + 1, 64 * (R - 2) * W, 1};
            for (int m : ms) {
                const int want = (m == 64 * R * W) ? 1 : ((R > 2 && m > 64 * (R - 2) * W) ? 2 : 0);
                if (padding_variant(m, R, W) != want) {
                    std::printf("m = %d R = %d W = %d: %d, expected %d\n", m, R, W, padding_variant(m, R, W), want);
                    EXPECT(padding_variant(m, R, W) == want);
                }
            }
        }
}

int main() {
    rt_descriptor(g_desc); // (static models never read the descriptor)
    check_fit<double, Me>("fill_fit_args<double, MultiExpModel<2, true>>");
    check_fit<float, Me>("fill_fit_args<float, MultiExpModel<2, true>>");
    check_fit<double, Rt>("fill_fit_args<double, RtModel<3, 2, 2>>");
    check_fit<float, Rt>("fill_fit_args<float, RtModel<3, 2, 2>>");
    check_eval<double, Me>("fill_eval_args<double, MultiExpModel<2, true>>");
    check_eval<float, Me>("fill_eval_args<float, MultiExpModel<2, true>>");
    check_eval<double, Rt>("fill_eval_args<double, RtModel<3, 2, 2>>");
    check_eval<float, Rt>("fill_eval_args<float, RtModel<3, 2, 2>>");
    check_lm_opts<double>("lm_opts_from<double>");
    check_lm_opts<float>("lm_opts_from<float>");
    check_padding_variant();
    {
        // a descriptor of another size is refused, by both fillers
        const char *who = "descriptor of another size";
        g_desc.n_basis = 2;
        const LaunchParams p = sentinel_params();
        FitArgs<double, Rt> f;
        EvalArgs<double, Rt> e;
        EXPECT(!fill_fit_args(p, f));
        EXPECT(!fill_eval_args(p, e));
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
