// varpro.hpp -- C++17 host-side mirror of the reference's public surface over the C ABI (include/varpro_hip.h).
//
// The reference (geo-ant/varpro) is compiled code (Rust); its toolchain is absent from the build image, so the
// host side above the C ABI is written in C++ (header-only) with the reference's names, argument meaning and
// error behaviour:
//
//   varpro::SeparableModelBuilder / SeparableModel      src/model/builder/mod.rs:252-571, src/model/mod.rs:239-517
//   varpro::SeparableProblemBuilder / SeparableProblem  src/problem/builder.rs:116-324, src/problem.rs:57-212,
//                                                        impl LeastSquaresProblem: src/solvers/levmar/mod.rs:22-202
//   varpro::LevMarSolver / FitResult / MinimizationReport / LevenbergMarquardt
//                                                        src/solvers/levmar/mod.rs:204-315, src/fit.rs
//   varpro::BatchProblem                                 new: B independent problems per launch
//
// Rust's `Result<T, E>` / `Option<T>` map to exceptions / std::optional; matrices are column-major
// std::vector<double> exactly as nalgebra stores them.  Closures are replaced by basis kinds.
// Link with -lvarpro_hip (varpro_amd/lib).  No CPU fallback: without a gfx950 device every compute call throws.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/varpro_hip.h"

namespace varpro {

enum class Basis : int32_t {
    Const = VP_BASIS_CONST,
    ExpDecay = VP_BASIS_EXP_DECAY,
    ExpRate = VP_BASIS_EXP_RATE,
    ExpCos = VP_BASIS_EXP_COS,
    SinPhase = VP_BASIS_SIN_PHASE,
    Gauss = VP_BASIS_GAUSS,     // peak kinds: the device evaluates their columns into memory (device-column handles)
    Lorentz = VP_BASIS_LORENTZ,
    Linear = VP_BASIS_LINEAR,
    // IRF reconvolution on a uniform grid (BatchProblem::set_irf): the decay exp(-t/tau) convolved with the instrument
    // response -- sum_{k<=i} irf_k exp(-(i-k) dt/tau), no factor dt -- and the response itself (the scattered-light term)
    ExpDecayIrf = VP_BASIS_EXP_DECAY_IRF,
    Irf = VP_BASIS_IRF,
    // ... with the response repeating every period T >= m dt (BatchProblem::set_irf_period; default: the record is one period)
    ExpDecayIrfPeriodic = VP_BASIS_EXP_DECAY_IRF_PERIODIC,
    // ... on the response shifted by delta, the function's last parameter (grid units, positive: later; cubic interpolation,
    // zero outside the record).  All shifted functions of a model name the same delta; the library checks it at creation
    ExpDecayIrfShift = VP_BASIS_EXP_DECAY_IRF_SHIFT,                  // (tau, delta)
    IrfShift = VP_BASIS_IRF_SHIFT,                                    // (delta)
    ExpDecayIrfPeriodicShift = VP_BASIS_EXP_DECAY_IRF_PERIODIC_SHIFT  // (tau, delta)
};
inline int arity(Basis k) {
    switch (k) {
    case Basis::Const:
    case Basis::Linear:
    case Basis::Irf: return 0;
    case Basis::ExpDecay:
    case Basis::ExpRate:
    case Basis::ExpDecayIrf:
    case Basis::IrfShift:
    case Basis::ExpDecayIrfPeriodic: return 1;
    default: return 2;
    }
}

// == ModelBuildError (src/model/builder/error.rs): `variant` is the Rust enum variant name
struct ModelBuildError : std::runtime_error {
    std::string variant;
    ModelBuildError(std::string v, const std::string &msg) : std::runtime_error(v + ": " + msg), variant(std::move(v)) {}
};
// == ModelError (src/model/errors.rs): an error of the model AT EVALUATION time; UnexpectedFunctionOutput carries the
// expected and the actual column length (src/model/model_basis_function.rs:70)
struct ModelError : std::runtime_error {
    std::string variant;
    size_t function_index, expected_length, actual_length;
    ModelError(std::string v, size_t j, size_t expected, size_t actual)
        : std::runtime_error(v + ": basis function " + std::to_string(j) + " returned " + std::to_string(actual) + " elements, expected " +
                             std::to_string(expected)),
          variant(std::move(v)), function_index(j), expected_length(expected), actual_length(actual) {}
};
// == SeparableProblemBuilderError (src/problem/builder.rs:15-46)
struct SeparableProblemBuilderError : std::runtime_error {
    std::string variant;
    SeparableProblemBuilderError(std::string v, const std::string &msg)
        : std::runtime_error(v + ": " + msg), variant(std::move(v)) {}
};
// call-level failure of the C ABI (VP_ERR_*)
struct HipError : std::runtime_error {
    int code;
    HipError(int c, const std::string &msg) : std::runtime_error("varpro_hip error " + std::to_string(c) + ": " + msg), code(c) {}
};
inline void check(int rc) {
    if (rc != 0) throw HipError(rc, vp_last_error());
}

// == SeparableModel: the descriptor the builder produces + the SeparableNonlinearModel trait surface
class SeparableModel {
  public:
    std::vector<std::string> parameter_names;
    vp_model_desc desc{};
    std::vector<double> x;
    std::vector<double> alpha;

    size_t parameter_count() const { return (size_t)desc.n_params; }      // src/model/mod.rs:256
    size_t base_function_count() const { return (size_t)desc.n_basis; }   // :259
    size_t output_len() const { return x.size(); }                        // :263
    void set_params(const std::vector<double> &p) {                       // :266-267
        if (p.size() != parameter_count()) throw std::invalid_argument("IncorrectParameterCount");
        alpha = p;
    }
    const std::vector<double> &params() const { return alpha; }           // :271
};

// == SeparableModelBuilder (src/model/builder/mod.rs:338-525); errors are latched and reported by build()
class SeparableModelBuilder {
    struct Fn {
        std::vector<std::string> params;
        Basis kind;
        std::vector<std::string> derivs;
    };
    std::vector<std::string> names_;
    std::vector<Fn> fns_;
    std::vector<double> x_, init_;
    bool have_x_ = false, have_init_ = false, building_ = false;
    std::optional<ModelBuildError> err_;
    void fail(const char *v, const std::string &m) {
        if (!err_) err_.emplace(v, m);
    }
    static bool contains(const std::vector<std::string> &v, const std::string &s) {
        for (auto &e : v)
            if (e == s) return true;
        return false;
    }

  public:
    explicit SeparableModelBuilder(std::vector<std::string> parameter_names) : names_(std::move(parameter_names)) {
        if (names_.empty()) fail("EmptyParameters", "A function or model parameter list is empty!");
        for (size_t i = 0; i < names_.size(); ++i) {
            if (names_[i].find(',') != std::string::npos) fail("CommaInParameterNameNotAllowed", names_[i]);
            for (size_t j = i + 1; j < names_.size(); ++j)
                if (names_[i] == names_[j]) fail("DuplicateParameterNames", "Parameter list contains duplicates!");
        }
    }
    SeparableModelBuilder &invariant_function(Basis kind = Basis::Const) {
        if (err_) return *this;
        if (arity(kind) != 0) fail("IncorrectParameterCount", "invariant function takes no parameters");
        else fns_.push_back({{}, kind, {}});
        building_ = false;
        return *this;
    }
    SeparableModelBuilder &function(std::vector<std::string> params, Basis kind) {
        if (err_) return *this;
        if (params.empty()) return fail("EmptyParameters", "A function or model parameter list is empty!"), *this;
        for (size_t i = 0; i < params.size(); ++i) {
            for (size_t j = i + 1; j < params.size(); ++j)
                if (params[i] == params[j]) return fail("DuplicateParameterNames", "duplicates in function parameters"), *this;
            if (!contains(names_, params[i]))
                return fail("FunctionParameterNotInModel", "Function parameter '" + params[i] + "' is not part of the model parameters."), *this;
        }
        if ((size_t)arity(kind) != params.size()) return fail("IncorrectParameterCount", "Incorrect number of parameters for function"), *this;
        fns_.push_back({std::move(params), kind, {}});
        building_ = true;
        return *this;
    }
    SeparableModelBuilder &partial_deriv(const std::string &parameter) {
        if (err_) return *this;
        if (!building_) return fail("IllegalCallToPartialDeriv", "can only follow 'function' or 'partial_deriv'"), *this;
        Fn &f = fns_.back();
        if (!contains(f.params, parameter)) return fail("InvalidDerivative", "Parameter '" + parameter + "' does not exist in parameter list"), *this;
        if (contains(f.derivs, parameter)) return fail("DuplicateDerivative", "Derivative for parameter '" + parameter + "' was already provided!"), *this;
        f.derivs.push_back(parameter);
        return *this;
    }
    SeparableModelBuilder &independent_variable(std::vector<double> x) {
        x_ = std::move(x);
        have_x_ = true;
        building_ = false;
        return *this;
    }
    SeparableModelBuilder &initial_parameters(std::vector<double> p) {
        if (err_) return *this;
        if (p.size() != names_.size()) return fail("IncorrectParameterCount", "wrong number of initial parameters"), *this;
        init_ = std::move(p);
        have_init_ = true;
        building_ = false;
        return *this;
    }
    SeparableModel build() const {
        if (err_) throw *err_;
        if (fns_.empty()) throw ModelBuildError("EmptyModel", "Tried to construct model with no functions.");
        for (auto &f : fns_)
            for (auto &p : f.params)
                if (!contains(f.derivs, p)) throw ModelBuildError("MissingDerivative", "missing derivative for parameter '" + p + "'");
        for (auto &n : names_) {
            bool used = false;
            for (auto &f : fns_) used = used || contains(f.params, n);
            if (!used) throw ModelBuildError("UnusedParameter", "Model depends on parameter '" + n + "', but none of its functions use it.");
        }
        if (!have_x_) throw ModelBuildError("MissingX", "Missing vector for independent variable x");
        if (!have_init_) throw ModelBuildError("MissingInitialParameters", "Missing initial guesses for model parameters");
        if (fns_.size() > VP_MAX_BASIS || names_.size() > VP_MAX_PARAMS) throw ModelBuildError("IncorrectParameterCount", "model exceeds VP_MAX_BASIS/VP_MAX_PARAMS");
        SeparableModel m;
        m.parameter_names = names_;
        m.x = x_;
        m.alpha = init_;
        m.desc.n_basis = (int32_t)fns_.size();
        m.desc.n_params = (int32_t)names_.size();
        for (int j = 0; j < VP_MAX_BASIS; ++j) {
            m.desc.kind[j] = 0;
            for (int a = 0; a < VP_MAX_BASIS_PARAMS; ++a) m.desc.param[j][a] = -1;
        }
        for (size_t j = 0; j < fns_.size(); ++j) {
            m.desc.kind[j] = (int32_t)fns_[j].kind;
            for (size_t a = 0; a < fns_[j].params.size(); ++a)
                for (size_t k = 0; k < names_.size(); ++k)
                    if (names_[k] == fns_[j].params[a]) m.desc.param[j][a] = (int32_t)k;
        }
        return m;
    }
};

// == levenberg_marquardt::LevenbergMarquardt builder knobs (src/solvers/levmar/mod.rs:221-223)
struct LevenbergMarquardt {
    vp_lm_opts o;
    LevenbergMarquardt() { vp_lm_opts_default(&o, VP_F64); }
    LevenbergMarquardt &with_ftol(double v) { return o.ftol = v, *this; }
    LevenbergMarquardt &with_xtol(double v) { return o.xtol = v, *this; }
    LevenbergMarquardt &with_gtol(double v) { return o.gtol = v, *this; }
    LevenbergMarquardt &with_stepbound(double v) { return o.stepbound = v, *this; }
    LevenbergMarquardt &with_patience(int v) { return o.patience = v, *this; }
    LevenbergMarquardt &with_scale_diag(bool v) { return o.scale_diag = v ? 1 : 0, *this; }
};

// ---- Student-t quantile: the scalar the reference takes from the `distrs` crate (src/statistics/mod.rs:285-288) to
// turn the unscaled confidence sigma into confidence_band_radius(p) = sigma * t_ppf((1+p)/2, dof) ------------------
namespace detail {
// regularised incomplete beta function I_x(a, b) (Lentz continued fraction)
inline double betainc(double a, double b, double x) {
    if (x <= 0.0) return 0.0;
    if (x >= 1.0) return 1.0;
    const double lbeta = std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b);
    const double front = std::exp(a * std::log(x) + b * std::log1p(-x) - lbeta);
    auto cf = [](double a_, double b_, double x_) {
        const double tiny = 1e-300;
        double c = 1.0, d = 1.0 - (a_ + b_) * x_ / (a_ + 1.0);
        if (std::fabs(d) < tiny) d = tiny;
        d = 1.0 / d;
        double h = d;
        for (int m = 1; m <= 500; ++m) {
            const double m2 = 2.0 * m;
            double aa = m * (b_ - m) * x_ / ((a_ + m2 - 1.0) * (a_ + m2));
            d = 1.0 + aa * d;
            if (std::fabs(d) < tiny) d = tiny;
            c = 1.0 + aa / c;
            if (std::fabs(c) < tiny) c = tiny;
            d = 1.0 / d;
            h *= d * c;
            aa = -(a_ + m) * (a_ + b_ + m) * x_ / ((a_ + m2) * (a_ + m2 + 1.0));
            d = 1.0 + aa * d;
            if (std::fabs(d) < tiny) d = tiny;
            c = 1.0 + aa / c;
            if (std::fabs(c) < tiny) c = tiny;
            d = 1.0 / d;
            const double del = d * c;
            h *= del;
            if (std::fabs(del - 1.0) < 1e-16) break;
        }
        return h;
    };
    if (x < (a + 1.0) / (a + b + 2.0)) return front * cf(a, b, x) / a;
    return 1.0 - front * cf(b, a, 1.0 - x) / b;
}
inline double student_t_cdf(double t, double dof) {
    const double x = dof / (dof + t * t);
    const double tail = 0.5 * betainc(0.5 * dof, 0.5, x);
    return t >= 0.0 ? 1.0 - tail : tail;
}
} // namespace detail

// t such that P(T <= t) = p for Student's t with `dof` degrees of freedom (bisection on the CDF; |error| < 1e-12 t)
inline double student_t_quantile(double p, double dof) {
    if (!(p > 0.0 && p < 1.0) || !(dof > 0.0)) throw std::invalid_argument("student_t_quantile: p in (0,1), dof > 0");
    if (p == 0.5) return 0.0;
    const bool upper = p > 0.5;
    const double pp = upper ? p : 1.0 - p;
    double lo = 0.0, hi = 1.0;
    while (detail::student_t_cdf(hi, dof) < pp && hi < 1e300) hi *= 2.0;
    for (int it = 0; it < 200 && hi - lo > 1e-14 * hi; ++it) {
        const double mid = 0.5 * (lo + hi);
        (detail::student_t_cdf(mid, dof) < pp ? lo : hi) = mid;
    }
    const double t = 0.5 * (lo + hi);
    return upper ? t : -t;
}

// B independent problems x S right-hand sides on one GPU (host-pointer mode; fp64)
class BatchProblem {
    vp_batch *h_ = nullptr;
    bool weighted_ = false, w_per_problem_ = false; // created with weights / with one set per problem
    int q_full_ = 0;                                // the descriptor's parameters (a handle with fixed ones: q counts the free)

  public:
    int64_t m = 0, S = 1, B = 0;
    int n = 0, q = 0;
    BatchProblem() = default;
    BatchProblem(const SeparableModel &model, const std::vector<double> &Y, int64_t B_, int64_t S_,
                 const std::vector<double> *weights = nullptr, double epsilon = -1.0, int device = 0,
                 bool device_columns = false) { // device_columns: VP_FLAG_DEVICE_COLUMNS (any descriptor then takes set_bounds)
        m = (int64_t)model.output_len();
        B = B_;
        S = S_;
        n = model.desc.n_basis;
        q = model.desc.n_params;
        if ((int64_t)Y.size() != B * S * m) throw std::invalid_argument("Y must hold B*S*m values");
        // weights: m values shared by the batch, or B*m values, one set per problem (what poisson_reweight needs)
        weighted_ = weights != nullptr;
        w_per_problem_ = weights && (int64_t)weights->size() == B * m && B > 1;
        if (weights && (int64_t)weights->size() != m && !w_per_problem_) throw std::invalid_argument("weights must hold m or B*m values");
        check(vp_batch_create(&h_, &model.desc, VP_F64, m, S, B, model.x.data(), Y.data(), weights ? weights->data() : nullptr,
                              epsilon, VP_FLAG_OWN_STREAM | (device_columns ? VP_FLAG_DEVICE_COLUMNS : 0) |
                                           (w_per_problem_ ? VP_FLAG_W_PER_PROBLEM : 0), device, nullptr));
    }
    // Fixed nonlinear parameters (vp_batch_create_fixed): fixed[k] != 0 holds parameter k at values[k] (q values shared by
    // the batch, or B*q values, one set per problem; entries of free parameters are ignored).  The handle is the REDUCED
    // model: q counts the free parameters, and every method takes and returns them alone, in model order.
    BatchProblem(const SeparableModel &model, const std::vector<double> &Y, int64_t B_, int64_t S_, const std::vector<int32_t> &fixed,
                 const std::vector<double> &values, const std::vector<double> *weights = nullptr, double epsilon = -1.0,
                 int device = 0) {
        m = (int64_t)model.output_len();
        B = B_;
        S = S_;
        n = model.desc.n_basis;
        q_full_ = model.desc.n_params;
        if ((int64_t)Y.size() != B * S * m) throw std::invalid_argument("Y must hold B*S*m values");
        if ((int)fixed.size() != q_full_) throw std::invalid_argument("fixed must hold one entry per parameter");
        q = 0;
        for (int k = 0; k < q_full_; ++k) q += fixed[k] ? 0 : 1;
        const bool per_problem = B > 1 && (int64_t)values.size() == B * q_full_;
        if (q != q_full_ && (int64_t)values.size() != q_full_ && !per_problem) throw std::invalid_argument("values must hold q or B*q values");
        weighted_ = weights != nullptr;
        w_per_problem_ = weights && (int64_t)weights->size() == B * m && B > 1;
        if (weights && (int64_t)weights->size() != m && !w_per_problem_) throw std::invalid_argument("weights must hold m or B*m values");
        check(vp_batch_create_fixed(&h_, &model.desc, VP_F64, m, S, B, model.x.data(), Y.data(), weights ? weights->data() : nullptr,
                                    epsilon, VP_FLAG_OWN_STREAM | (w_per_problem_ ? VP_FLAG_W_PER_PROBLEM : 0), device, nullptr,
                                    fixed.data(), values.empty() ? nullptr : values.data(), per_problem ? 1 : 0));
    }
    // replace the fixed values between fits (vp_set_fixed_values): q_full or B*q_full values in the FULL parameter order
    void set_fixed_values(const std::vector<double> &values) {
        const bool per_problem = B > 1 && (int64_t)values.size() == B * q_full_;
        if ((int64_t)values.size() != q_full_ && !per_problem) throw std::invalid_argument("values must hold q or B*q values");
        check(vp_set_fixed_values(h_, values.data(), per_problem ? 1 : 0));
    }
    // Neyman weights of Poisson counts, w = 1/sqrt(max(y, 1)): the `weights` of a handle that fit_poisson will drive
    static std::vector<double> neyman_weights(const std::vector<double> &counts) {
        std::vector<double> w(counts.size());
        for (size_t i = 0; i < counts.size(); ++i) w[i] = 1.0 / std::sqrt(counts[i] < 1.0 ? 1.0 : counts[i]);
        return w;
    }
    BatchProblem(const BatchProblem &) = delete;
    BatchProblem &operator=(const BatchProblem &) = delete;
    BatchProblem(BatchProblem &&o) noexcept { *this = std::move(o); }
    BatchProblem &operator=(BatchProblem &&o) noexcept {
        std::swap(h_, o.h_);
        m = o.m, S = o.S, B = o.B, n = o.n, q = o.q;
        weighted_ = o.weighted_, w_per_problem_ = o.w_per_problem_;
        q_full_ = o.q_full_;
        return *this;
    }
    ~BatchProblem() {
        if (h_) vp_batch_destroy(h_);
    }
    vp_batch *handle() const { return h_; }
    void set_params(const std::vector<double> &alpha) { check(vp_set_params(h_, alpha.data())); }
    // next frame of a stream of same-shaped data: new observations, same model / grid / weights, no re-allocation
    void set_observations(const std::vector<double> &Y) {
        if ((int64_t)Y.size() != B * S * m) throw std::invalid_argument("Y must hold B*S*m values");
        check(vp_set_observations(h_, Y.data()));
    }
    // replace the weights of a handle created with weights, in the layout of creation (vp_set_weights); Y again: the handle
    // keeps only W Y
    void set_weights(const std::vector<double> &w, const std::vector<double> &Y) {
        if (!weighted_) throw std::invalid_argument("set_weights: the handle was created without weights");
        if ((int64_t)w.size() != (w_per_problem_ ? B * m : m)) throw std::invalid_argument("set_weights: the weights keep the layout of creation");
        if ((int64_t)Y.size() != B * S * m) throw std::invalid_argument("Y must hold B*S*m values");
        check(vp_set_weights(h_, w.data(), Y.data()));
    }
    // Poisson weights formed on the device (vp_poisson_reweight): 1/sqrt(max(v, floor)), v = the counts (VP_POISSON_NEYMAN) or
    // the handle's current best fit (VP_POISSON_MODEL, which also returns the deviance and Pearson's X^2 of that fit, [B] each)
    struct PoissonGoodness {
        std::vector<double> deviance, pearson;
    };
    PoissonGoodness poisson_reweight(const std::vector<double> &counts, int mode = VP_POISSON_MODEL, double floor = 1.0) {
        if (mode != VP_POISSON_NEYMAN && mode != VP_POISSON_MODEL) throw std::invalid_argument("poisson_reweight: unknown mode");
        if (!(floor > 0.0) || !std::isfinite(floor)) throw std::invalid_argument("poisson_reweight: the floor must be finite and > 0");
        if (S != 1) throw std::invalid_argument("poisson_reweight: weights are per problem, not per right-hand side (S = 1 only)");
        if (!w_per_problem_) throw std::invalid_argument("poisson_reweight: the handle needs per-problem weights (B*m values)");
        if ((int64_t)counts.size() != B * m) throw std::invalid_argument("counts must hold B*m values");
        PoissonGoodness g;
        if (mode == VP_POISSON_MODEL) g.deviance.resize((size_t)B), g.pearson.resize((size_t)B);
        check(vp_poisson_reweight(h_, counts.data(), mode, floor, mode == VP_POISSON_MODEL ? g.deviance.data() : nullptr,
                                  mode == VP_POISSON_MODEL ? g.pearson.data() : nullptr));
        return g;
    }
    // Poisson maximum-likelihood fit by iterated re-weighting (== the Python BatchProblem.fit_poisson): a Neyman-weighted fit
    // from alpha0, `rounds` fits at the weights of the previous fit, one more model re-weight and an evaluation -- the
    // result carries deviance, Pearson's X^2 and the reduced deviance D / (m - n - q) AT the returned point, which is the
    // handle's state (statistics(), best_fit() need no further call).  The default `rounds` is measured: DESIGN.md section 3i
    struct PoissonFit {
        std::vector<double> alpha, C; // [B][q], [B][n]
        std::vector<vp_report> report; // the last fit's
        std::vector<double> deviance, pearson, reduced_deviance; // [B]
    };
    static constexpr int kPoissonRounds = 9;
    PoissonFit fit_poisson(const std::vector<double> &counts, const std::vector<double> &alpha0, int rounds = kPoissonRounds,
                           double floor = 1.0, const LevenbergMarquardt &solver = LevenbergMarquardt()) {
        if (rounds < 0) throw std::invalid_argument("fit_poisson: rounds >= 0");
        PoissonFit r;
        r.alpha = alpha0;
        r.report.resize((size_t)B);
        r.C.resize((size_t)(B * n));
        poisson_reweight(counts, VP_POISSON_NEYMAN, floor);
        check(vp_fit(h_, &solver.o, r.alpha.data(), r.C.data(), r.report.data()));
        for (int k = 0; k < rounds; ++k) {
            poisson_reweight(counts, VP_POISSON_MODEL, floor);
            check(vp_fit(h_, &solver.o, r.alpha.data(), r.C.data(), r.report.data()));
        }
        // deviance and X^2 of the returned (alpha, C); the evaluation makes the handle's state that alpha at the final weights
        PoissonGoodness g = poisson_reweight(counts, VP_POISSON_MODEL, floor);
        check(vp_evaluate(h_, r.alpha.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
        r.reduced_deviance.resize((size_t)B);
        for (int64_t b = 0; b < B; ++b) r.reduced_deviance[(size_t)b] = g.deviance[(size_t)b] / (double)(m - n - q);
        r.deviance = std::move(g.deviance);
        r.pearson = std::move(g.pearson);
        return r;
    }
    // the handle's current weights (vp_weights), m or B*m values as created; after robust_reweight / fit_robust the outlier map
    std::vector<double> weights() {
        if (!weighted_) throw std::invalid_argument("weights: the handle was created without weights");
        std::vector<double> w((size_t)(w_per_problem_ ? B * m : m));
        check(vp_weights(h_, w.data()));
        return w;
    }
    // M-estimator weights from the residuals of the handle's current best fit, formed on the device (vp_robust_reweight):
    // w = w0 sqrt(omega(u)), u = w0 (y - f)/s; loss VP_ROBUST_HUBER / _CAUCHY / _TUKEY, tuning 0 = the 95 % efficiency constant,
    // scale 0 = the normalised median of |w0 (y - f)| per problem, base_weights null = 1 (they are passed again every round).
    // Returns s and sum rho(u) of the fit the weights were formed from, [B] each
    struct RobustScale {
        std::vector<double> scale, rho;
    };
    RobustScale robust_reweight(const std::vector<double> &Y, int loss = VP_ROBUST_HUBER, double tuning = 0.0, double scale = 0.0,
                                const std::vector<double> *base_weights = nullptr) {
        if (loss != VP_ROBUST_HUBER && loss != VP_ROBUST_CAUCHY && loss != VP_ROBUST_TUKEY) throw std::invalid_argument("robust_reweight: unknown loss");
        if (!(tuning >= 0.0) || !std::isfinite(tuning)) throw std::invalid_argument("robust_reweight: the tuning constant must be finite and > 0 (0: default)");
        if (!(scale >= 0.0) || !std::isfinite(scale)) throw std::invalid_argument("robust_reweight: the scale must be finite and > 0 (0: estimated)");
        if (S != 1) throw std::invalid_argument("robust_reweight: weights are per problem, not per right-hand side (S = 1 only)");
        if (!w_per_problem_) throw std::invalid_argument("robust_reweight: the handle needs per-problem weights (B*m values)");
        if ((int64_t)Y.size() != B * m) throw std::invalid_argument("Y must hold B*m values");
        if (base_weights && (int64_t)base_weights->size() != B * m) throw std::invalid_argument("the base weights must hold B*m values");
        RobustScale g;
        g.scale.resize((size_t)B), g.rho.resize((size_t)B);
        check(vp_robust_reweight(h_, Y.data(), base_weights ? base_weights->data() : nullptr, loss, tuning, scale, g.scale.data(),
                                 g.rho.data()));
        return g;
    }
    // Robust fit by iterated re-weighting, not an LM on rho (== the Python BatchProblem.fit_robust): a fit at the base weights
    // from alpha0, `rounds` times {robust_reweight, fit from the previous parameters}, one more re-weight and an evaluation --
    // scale, rho and the weights (the outlier map) belong to the returned point, which is the handle's state.  Tukey and
    // Cauchy are not convex: start them from a sensible fit.  statistics() afterwards is the covariance of the weighted
    // least-squares problem at the final weights, not a sandwich estimator.  The default `rounds` is measured: DESIGN.md 3j
    struct RobustFit {
        std::vector<double> alpha, C; // [B][q], [B][n]
        std::vector<vp_report> report; // the last fit's
        std::vector<double> scale, rho; // [B]
        std::vector<double> weights; // [B][m]
    };
    static constexpr int kRobustRounds = 14;
    RobustFit fit_robust(const std::vector<double> &Y, const std::vector<double> &alpha0, int loss = VP_ROBUST_HUBER,
                         double tuning = 0.0, double scale = 0.0, int rounds = kRobustRounds,
                         const std::vector<double> *base_weights = nullptr, const LevenbergMarquardt &solver = LevenbergMarquardt()) {
        if (rounds < 0) throw std::invalid_argument("fit_robust: rounds >= 0");
        const std::vector<double> unit(base_weights ? (size_t)0 : (size_t)(B * m), 1.0);
        const std::vector<double> &w0 = base_weights ? *base_weights : unit;
        RobustFit r;
        r.alpha = alpha0;
        r.report.resize((size_t)B);
        r.C.resize((size_t)(B * n));
        set_weights(w0, Y);
        check(vp_fit(h_, &solver.o, r.alpha.data(), r.C.data(), r.report.data()));
        for (int k = 0; k < rounds; ++k) {
            robust_reweight(Y, loss, tuning, scale, &w0);
            check(vp_fit(h_, &solver.o, r.alpha.data(), r.C.data(), r.report.data()));
        }
        RobustScale g = robust_reweight(Y, loss, tuning, scale, &w0);
        check(vp_evaluate(h_, r.alpha.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
        r.scale = std::move(g.scale);
        r.rho = std::move(g.rho);
        r.weights = weights();
        return r;
    }
    // box bounds of fit() on a device-column handle (vp_set_bounds): q values (one box for all problems) or B*q values
    // each; +-INFINITY = unbounded on that side.  The bounds stay set until clear_bounds()
    void set_bounds(const std::vector<double> &lower, const std::vector<double> &upper) {
        const bool per_problem = (int64_t)lower.size() == B * q && B > 1;
        if (lower.size() != upper.size() || ((int64_t)lower.size() != q && !per_problem))
            throw std::invalid_argument("bounds must hold q or B*q values each");
        check(vp_set_bounds(h_, lower.data(), upper.data(), per_problem ? 1 : 0));
    }
    void clear_bounds() { check(vp_set_bounds(h_, nullptr, nullptr, 0)); }
    // the instrument response of a model with Basis::ExpDecayIrf / Basis::Irf (vp_set_irf): m values shared by the batch or
    // B*m values; copied by the handle, may be replaced.  Needed before anything that evaluates the model
    void set_irf(const std::vector<double> &irf) {
        const bool per_problem = (int64_t)irf.size() == B * m && B > 1;
        if ((int64_t)irf.size() != m && !per_problem) throw std::invalid_argument("irf must hold m or B*m values");
        check(vp_set_irf(h_, irf.data(), per_problem ? 1 : 0));
    }
    // the period T >= m dt of Basis::ExpDecayIrfPeriodic in the units of the grid (vp_set_irf_period); 0: the record is one period
    void set_irf_period(double period) { check(vp_set_irf_period(h_, period)); }
    // start-point search (vp_search): per problem the best of K candidates by the projected objective; the handle is then
    // in the state of set_params(result.alpha).  candidates: K*q values shared by all problems, or B*K*q with per_problem
    struct SearchResult {
        std::vector<double> alpha;  // [B][q]
        std::vector<int32_t> index; // [B], -1: no finite candidate (alpha is then candidate 0)
        std::vector<double> cost;   // [B]
    };
    SearchResult search(const std::vector<double> &candidates, int64_t K, bool per_problem = false) {
        if (K < 1 || (int64_t)candidates.size() != (per_problem ? B : 1) * K * q)
            throw std::invalid_argument("candidates must hold K*q values (B*K*q per problem)");
        SearchResult r{std::vector<double>((size_t)(B * q)), std::vector<int32_t>((size_t)B), std::vector<double>((size_t)B)};
        check(vp_search(h_, candidates.data(), K, per_problem ? VP_SEARCH_PER_PROBLEM : 0, r.alpha.data(), r.index.data(),
                        r.cost.data()));
        return r;
    }
    std::vector<int32_t> status() const {
        std::vector<int32_t> st((size_t)B);
        check(vp_linear_coeffs(h_, nullptr, st.data()));
        return st;
    }
    std::vector<double> residuals() const {
        std::vector<double> r((size_t)(B * S * m));
        check(vp_residuals(h_, r.data(), nullptr));
        return r;
    }
    std::vector<double> jacobian() const {
        std::vector<double> J((size_t)(B * q * S * m));
        check(vp_jacobian(h_, J.data(), nullptr));
        return J;
    }
    std::vector<double> linear_coefficients() const {
        std::vector<double> C((size_t)(B * S * n));
        check(vp_linear_coeffs(h_, C.data(), nullptr));
        return C;
    }
    std::vector<double> best_fit() const {
        std::vector<double> f((size_t)(B * S * m));
        check(vp_best_fit(h_, f.data()));
        return f;
    }
    std::vector<vp_report> fit(std::vector<double> &alpha_inout, const LevenbergMarquardt &solver = LevenbergMarquardt()) {
        std::vector<vp_report> rep((size_t)B);
        check(vp_fit(h_, &solver.o, alpha_inout.data(), nullptr, rep.data()));
        return rep;
    }
    // == FitStatistics::try_calculate for every problem (src/statistics/mod.rs:352-441); single RHS only
    struct Statistics {
        std::vector<double> covariance;   // [B][(n+q)^2] column-major, ordering [linear coefficients, parameters]
        std::vector<double> reduced_chi2; // [B]
        std::vector<double> conf_sigma;   // [B][m]  multiply by the Student-t quantile for a confidence band
        std::vector<int32_t> status;      // [B]  0 ok, 4 = Underdetermined / MatrixInversion
        int64_t m = 0, dof = 0;
        // == FitStatistics::confidence_band_radius (src/statistics/mod.rs:271-304) of problem b
        std::vector<double> confidence_band_radius(int64_t b, double probability) const {
            if (!(probability > 0.0 && probability < 1.0)) throw std::invalid_argument("probability must be in (0,1)");
            const double tq = student_t_quantile(0.5 * (1.0 + probability), (double)dof);
            std::vector<double> r((size_t)m);
            for (int64_t i = 0; i < m; ++i) r[(size_t)i] = tq * conf_sigma[(size_t)(b * m + i)];
            return r;
        }
    };
    Statistics statistics() const {
        Statistics s;
        const size_t k = (size_t)(n + q);
        s.covariance.resize((size_t)B * k * k);
        s.reduced_chi2.resize((size_t)B);
        s.conf_sigma.resize((size_t)(B * m));
        s.status.resize((size_t)B);
        s.m = m;
        s.dof = m - (int64_t)k;
        check(vp_statistics(h_, s.covariance.data(), s.reduced_chi2.data(), s.conf_sigma.data(), s.status.data()));
        return s;
    }
    // statistics of a GLOBAL fit (any S): FitStatistics::try_calculate of the stacked problem, parameters [c_1 .. c_S, alpha]
    // (vp_global_statistics; the cross blocks Cov(c_s, c_t), s != t, are not produced)
    struct GlobalStatistics {
        std::vector<double> cov_alpha;      // [B][q][q]
        std::vector<double> reduced_chi2;   // [B]
        std::vector<double> coef_cov;       // [B][S][n][n]
        std::vector<double> coef_alpha_cov; // [B][S][n][q]
        std::vector<double> conf_sigma;     // [B][S][m] (empty unless asked for)
        std::vector<int32_t> status;        // [B]  0 ok, 4 = Underdetermined / MatrixInversion of the stacked problem
        int64_t m = 0, S = 1, dof = 0;
        // the Student-t scaled band of right-hand side s of problem b (src/statistics/mod.rs:271-304, stacked dof)
        std::vector<double> confidence_band_radius(int64_t b, int64_t s, double probability) const {
            if (!(probability > 0.0 && probability < 1.0)) throw std::invalid_argument("probability must be in (0,1)");
            if (conf_sigma.empty()) throw std::logic_error("global_statistics(true) computes the band");
            const double tq = student_t_quantile(0.5 * (1.0 + probability), (double)dof);
            std::vector<double> r((size_t)m);
            for (int64_t i = 0; i < m; ++i) r[(size_t)i] = tq * conf_sigma[(size_t)((b * S + s) * m + i)];
            return r;
        }
    };
    GlobalStatistics global_statistics(bool want_confidence_sigma = false) const {
        GlobalStatistics g;
        g.cov_alpha.resize((size_t)(B * q * q));
        g.reduced_chi2.resize((size_t)B);
        g.coef_cov.resize((size_t)(B * S * n * n));
        g.coef_alpha_cov.resize((size_t)(B * S * n * q));
        if (want_confidence_sigma) g.conf_sigma.resize((size_t)(B * S * m));
        g.status.resize((size_t)B);
        g.m = m;
        g.S = S;
        g.dof = m * S - (int64_t)n * S - q;
        check(vp_global_statistics(h_, g.cov_alpha.data(), g.reduced_chi2.data(), g.coef_cov.data(), g.coef_alpha_cov.data(),
                                   want_confidence_sigma ? g.conf_sigma.data() : nullptr, g.status.data()));
        return g;
    }
    // one global fit sharded by right-hand sides over ranks: `fn` sums `count` device doubles over all ranks on
    // the given HIP stream (ncclAllReduce on RCCL); see include/varpro_hip.h
    void set_rhs_allreduce(vp_allreduce_fn fn, void *user, int64_t global_rhs_count) {
        check(vp_set_rhs_allreduce(h_, fn, user, global_rhs_count));
    }
};

// ---- models OUTSIDE the descriptor language: the reference's closure-based `SeparableModel` (src/model/mod.rs:367-517),
// built as `SeparableModelBuilder::function(params, f).partial_deriv(param, df)` (src/model/builder/mod.rs:338-525) with REAL
// C++ callables.  f(x, params) -> m values.  The model is evaluated where it lives (the host); everything downstream of
// eval() / eval_partial_deriv(k) runs on the device (vp_batch_create_external, include/varpro_hip.h).
class ClosureModel {
  public:
    using Fn = std::function<std::vector<double>(const std::vector<double> &x, const std::vector<double> &params)>;

  private:
    struct Basis_ {
        std::vector<int> idx;        // model parameter indices of the function's parameter list
        Fn f;
        std::map<int, Fn> derivs;    // model parameter index -> d f / d parameter
    };
    std::vector<std::string> names_;
    std::vector<double> x_;
    std::vector<Basis_> fns_;
    int find(const std::string &nm) const {
        for (size_t i = 0; i < names_.size(); ++i)
            if (names_[i] == nm) return (int)i;
        return -1;
    }

  public:
    ClosureModel(std::vector<std::string> parameter_names, std::vector<double> x) : names_(std::move(parameter_names)), x_(std::move(x)) {
        if (names_.empty()) throw ModelBuildError("EmptyParameters", "A function or model parameter list is empty!");
        for (size_t i = 0; i < names_.size(); ++i) {
            if (names_[i].find(',') != std::string::npos)
                throw ModelBuildError("CommaInParameterNameNotAllowed", "Parameter names may not contain comma separator");
            for (size_t j = 0; j < i; ++j)
                if (names_[i] == names_[j]) throw ModelBuildError("DuplicateParameterNames", "Parameter list contains duplicates!");
        }
    }
    ClosureModel &invariant_function(Fn f) {
        fns_.push_back(Basis_{{}, std::move(f), {}});
        return *this;
    }
    ClosureModel &function(const std::vector<std::string> &params, Fn f) {
        if (params.empty()) throw ModelBuildError("EmptyParameters", "A function or model parameter list is empty!");
        Basis_ b;
        for (const auto &nm : params) {
            const int k = find(nm);
            if (k < 0) throw ModelBuildError("FunctionParameterNotInModel", "Function parameter '" + nm + "' is not part of the model parameters.");
            for (int kk : b.idx)
                if (kk == k) throw ModelBuildError("DuplicateParameterNames", "Parameter list contains duplicates!");
            b.idx.push_back(k);
        }
        b.f = std::move(f);
        fns_.push_back(std::move(b));
        return *this;
    }
    ClosureModel &partial_deriv(const std::string &param, Fn df) {
        if (fns_.empty() || fns_.back().idx.empty()) throw ModelBuildError("IllegalCallToPartialDeriv", "partial_deriv needs a preceding function");
        const int k = find(param);
        Basis_ &b = fns_.back();
        bool in = false;
        for (int kk : b.idx) in = in || kk == k;
        if (k < 0 || !in) throw ModelBuildError("InvalidDerivative", "Parameter '" + param + "' is not in the function's parameter list");
        if (b.derivs.count(k)) throw ModelBuildError("DuplicateDerivative", "Derivative for parameter '" + param + "' was already provided!");
        b.derivs[k] = std::move(df);
        return *this;
    }
    // == SeparableModelBuilder::build (src/model/builder/mod.rs:527-553)
    void validate() const {
        if (fns_.empty()) throw ModelBuildError("EmptyModel", "Tried to construct model with no functions.");
        std::vector<bool> used(names_.size(), false);
        for (const auto &b : fns_)
            for (int k : b.idx) {
                used[(size_t)k] = true;
                if (!b.derivs.count(k)) throw ModelBuildError("MissingDerivative", "missing derivative for parameter '" + names_[(size_t)k] + "'");
            }
        for (size_t k = 0; k < used.size(); ++k)
            if (!used[k]) throw ModelBuildError("UnusedParameter", "Parameter '" + names_[k] + "' is not used by any function of the model");
    }
    size_t parameter_count() const { return names_.size(); }
    size_t base_function_count() const { return fns_.size(); }
    size_t output_len() const { return x_.size(); }
    // the (basis j, parameter k) pairs with a non-zero derivative, in the column order of derivs()
    std::vector<std::pair<int, int>> pairs() const {
        std::vector<std::pair<int, int>> p;
        for (size_t j = 0; j < fns_.size(); ++j)
            for (int k : fns_[j].idx) p.emplace_back((int)j, k);
        return p;
    }
    // == eval() (src/model/mod.rs:441-471) for a batch of parameter sets alpha [B][q]: Phi [B][n][m], UNWEIGHTED
    std::vector<double> eval_batch(const std::vector<double> &alpha, int64_t B) const {
        const size_t q = names_.size(), n = fns_.size(), m = x_.size();
        std::vector<double> out((size_t)B * n * m);
        for (int64_t b = 0; b < B; ++b)
            for (size_t j = 0; j < n; ++j) {
                std::vector<double> pr;
                for (int k : fns_[j].idx) pr.push_back(alpha[(size_t)b * q + (size_t)k]);
                const std::vector<double> v = fns_[j].f(x_, pr);
                // == ModelError::UnexpectedFunctionOutput (src/model/model_basis_function.rs:70): a column of the wrong length is
                // an error of the model, never a write past (or short of) its slot
                if (v.size() != m) throw ModelError("UnexpectedFunctionOutput", j, m, v.size());
                std::copy(v.begin(), v.end(), out.begin() + ((size_t)b * n + j) * m);
            }
        return out;
    }
    // == the non-zero columns of eval_partial_deriv(k) (src/model/mod.rs:473-512) in pair order: dPhi [B][p][m]
    std::vector<double> derivs_batch(const std::vector<double> &alpha, int64_t B) const {
        const size_t q = names_.size(), m = x_.size();
        const auto prs = pairs();
        std::vector<double> out((size_t)B * prs.size() * m);
        for (int64_t b = 0; b < B; ++b)
            for (size_t p = 0; p < prs.size(); ++p) {
                const Basis_ &bs = fns_[(size_t)prs[p].first];
                std::vector<double> pr;
                for (int k : bs.idx) pr.push_back(alpha[(size_t)b * q + (size_t)k]);
                const std::vector<double> v = bs.derivs.at(prs[p].second)(x_, pr);
                if (v.size() != m) throw ModelError("UnexpectedDerivativeOutput", (size_t)prs[p].first, m, v.size());
                std::copy(v.begin(), v.end(), out.begin() + ((size_t)b * prs.size() + p) * m);
            }
        return out;
    }
};

// B problems of one closure model (single right-hand side, fp64, host-pointer mode): trait-level evaluation and the
// batched LM fit by reverse communication -- LevMarSolver::fit over any SeparableNonlinearModel
// (src/solvers/levmar/mod.rs:238-254): the LM drivers on the device, the model with the caller
class ExternalBatchProblem {
    vp_batch *h_ = nullptr;
    // the model is COPIED (closures are shared_ptr-backed std::function objects: cheap): a problem built from a temporary
    // model must not dangle, and the reference's problem owns its model too (src/problem.rs:55-70)
    std::shared_ptr<const ClosureModel> model_;

  public:
    int64_t m = 0, B = 0, S = 1;
    int n = 0, q = 0, np = 0;
    // Y: [B][S][m] -- S right-hand sides per problem share the nonlinear parameters (SeparableProblemBuilder::mrhs,
    // src/problem/builder.rs:194-225); S = 1: the single-right-hand-side problem
    ExternalBatchProblem(const ClosureModel &model, const std::vector<double> &Y, int64_t B_, const std::vector<double> *weights = nullptr,
                         double epsilon = -1.0, int device = 0, int64_t S_ = 1)
        : model_(std::make_shared<const ClosureModel>(model)) {
        model.validate();
        m = (int64_t)model.output_len();
        B = B_;
        S = S_;
        n = (int)model.base_function_count();
        q = (int)model.parameter_count();
        const auto prs = model.pairs();
        np = (int)prs.size();
        std::vector<int32_t> pb, pp;
        for (const auto &pr : prs) {
            pb.push_back(pr.first);
            pp.push_back(pr.second);
        }
        if ((int64_t)Y.size() != B * S * m) throw std::invalid_argument("Y must hold B*S*m values");
        check(vp_batch_create_external(&h_, n, q, np, pb.data(), pp.data(), VP_F64, m, S, B, Y.data(), weights ? weights->data() : nullptr,
                                       epsilon, VP_FLAG_OWN_STREAM, device, nullptr));
    }
    ExternalBatchProblem(const ExternalBatchProblem &) = delete;
    ExternalBatchProblem &operator=(const ExternalBatchProblem &) = delete;
    ~ExternalBatchProblem() {
        if (h_) vp_batch_destroy(h_);
    }
    struct Evaluation {
        std::vector<double> residuals, jacobian, coefficients, cost; // [B][m], [B][q][m], [B][n], [B]
        std::vector<int32_t> status;
    };
    // set_params + residuals + jacobian of every problem at alpha [B][q] (src/solvers/levmar/mod.rs:42-73, 91-95, 101-201)
    Evaluation evaluate(const std::vector<double> &alpha) const {
        const std::vector<double> Phi = model_->eval_batch(alpha, B), dPhi = model_->derivs_batch(alpha, B);
        Evaluation e;
        e.residuals.resize((size_t)(B * S * m));      // [B][S][m]
        e.jacobian.resize((size_t)(B * q * S * m));   // [B][q][S][m]
        e.coefficients.resize((size_t)(B * S * n));   // [B][S][n]
        e.cost.resize((size_t)(B * S));
        e.status.resize((size_t)(B * S));
        check(vp_evaluate_with_basis(h_, alpha.data(), Phi.data(), dPhi.data(), e.residuals.data(), e.jacobian.data(),
                                     e.coefficients.data(), e.cost.data(), e.status.data()));
        return e;
    }
    struct BatchFit {
        std::vector<double> nonlinear_parameters, linear_coefficients; // [B][q], [B][n]
        std::vector<vp_report> reports;                                // termination > 0 <=> FitResult Ok (:249-253)
        int steps = 0;
    };
    BatchFit fit(const std::vector<double> &alpha0, const LevenbergMarquardt &solver = LevenbergMarquardt(), bool derivatives_on_accept = false) {
        check(vp_fit_begin(h_, &solver.o, alpha0.data(), derivatives_on_accept ? VP_FIT_DERIVATIVES_ON_ACCEPT : 0));
        std::vector<double> trial = alpha0;
        std::vector<int32_t> want((size_t)B, VP_WANT_BASIS | VP_WANT_DERIVATIVES);
        int64_t active = B;
        BatchFit out;
        const int limit = 2 * (solver.o.patience * (q + 1) + 2);
        while (active > 0 && out.steps < limit) {
            // (the columns of every problem are evaluated: a model may skip the problems whose want word is 0)
            const std::vector<double> Phi = model_->eval_batch(trial, B), dPhi = model_->derivs_batch(trial, B);
            check(vp_fit_step_with_basis(h_, Phi.data(), dPhi.data(), trial.data(), want.data(), &active));
            ++out.steps;
        }
        out.nonlinear_parameters.resize((size_t)(B * q));
        out.linear_coefficients.resize((size_t)(B * S * n)); // [B][S][n]
        out.reports.resize((size_t)B);
        check(vp_fit_end(h_, out.nonlinear_parameters.data(), out.linear_coefficients.data(), out.reports.data()));
        return out;
    }
};

// == SeparableProblem (single problem, S right-hand sides); `None` of the reference == std::nullopt
class SeparableProblem {
    SeparableModel model_;
    BatchProblem batch_;
    std::optional<std::vector<double>> weights_;

  public:
    SeparableProblem(SeparableModel model, const std::vector<double> &Y, int64_t S, std::optional<std::vector<double>> weights,
                     double epsilon, bool device_columns = false)
        : model_(std::move(model)), batch_(model_, Y, 1, S, weights ? &*weights : nullptr, epsilon, 0, device_columns),
          weights_(std::move(weights)) {
        set_params(model_.params()); // build(): initial set_params (src/problem/builder.rs:321)
    }
    void set_params(const std::vector<double> &p) { // src/solvers/levmar/mod.rs:42-73
        model_.set_params(p);
        batch_.set_params(p);
    }
    const std::vector<double> &params() const { return model_.params(); } // :80-82
    std::optional<std::vector<double>> residuals() const {               // :91-95
        if (batch_.status()[0] != VP_ST_OK) return std::nullopt;
        return batch_.residuals();
    }
    std::optional<std::vector<double>> jacobian() const { // :101-201  (m*S) x q column-major
        if (batch_.status()[0] != VP_ST_OK) return std::nullopt;
        return batch_.jacobian();
    }
    std::optional<std::vector<double>> linear_coefficients() const { // src/problem.rs:142-183  n x S column-major
        if (batch_.status()[0] != VP_ST_OK) return std::nullopt;
        return batch_.linear_coefficients();
    }
    const SeparableModel &model() const { return model_; }
    SeparableModel &model_mut() { return model_; }
    BatchProblem &batch() { return batch_; }
    const BatchProblem &batch() const { return batch_; }
};

// == SeparableProblemBuilder::{new, mrhs, observations, weights, epsilon, build}
class SeparableProblemBuilder {
    SeparableModel model_;
    bool mrhs_;
    std::optional<std::vector<double>> Y_;
    int64_t S_ = 1;
    std::optional<std::vector<double>> weights_;
    double eps_ = -1.0;
    bool device_columns_ = false;
    std::optional<std::pair<std::vector<double>, std::vector<double>>> bounds_;
    SeparableProblemBuilder(SeparableModel m, bool mrhs) : model_(std::move(m)), mrhs_(mrhs) {}

  public:
    static SeparableProblemBuilder new_(SeparableModel m) { return SeparableProblemBuilder(std::move(m), false); }
    static SeparableProblemBuilder mrhs(SeparableModel m) { return SeparableProblemBuilder(std::move(m), true); }
    // single RHS: y (m values);  MRHS: Y column-major m x S
    SeparableProblemBuilder &observations(std::vector<double> Y, int64_t S = 1) {
        Y_ = std::move(Y);
        S_ = mrhs_ ? S : 1;
        return *this;
    }
    SeparableProblemBuilder &weights(std::vector<double> w) { return weights_ = std::move(w), *this; }
    SeparableProblemBuilder &epsilon(double e) { return eps_ = std::fabs(e), *this; }
    // additions to the reference's builder: VP_FLAG_DEVICE_COLUMNS, and box bounds on the nonlinear parameters (q values
    // each, +-INFINITY = unbounded; the model needs a peak / baseline kind or device_columns())
    SeparableProblemBuilder &device_columns(bool on = true) { return device_columns_ = on, *this; }
    SeparableProblemBuilder &bounds(std::vector<double> lower, std::vector<double> upper) {
        return bounds_ = std::make_pair(std::move(lower), std::move(upper)), *this;
    }
    SeparableProblem build() {
        if (!Y_) throw SeparableProblemBuilderError("YDataMissing", "Right hand side(s) not provided");
        const size_t xlen = model_.output_len();
        if (xlen == 0 || Y_->empty()) throw SeparableProblemBuilderError("ZeroLengthVector", "x or y must have nonzero number of elements.");
        if (Y_->size() != xlen * (size_t)S_)
            throw SeparableProblemBuilderError("InvalidLengthOfData", "Vectors x and y must have same lengths.");
        if (weights_ && weights_->size() != xlen)
            throw SeparableProblemBuilderError("InvalidLengthOfWeights", "The weights must have the same length as the data y.");
        SeparableProblem problem(model_, *Y_, S_, weights_, eps_, device_columns_);
        if (bounds_) problem.batch().set_bounds(bounds_->first, bounds_->second);
        return problem;
    }
};

// == MinimizationReport / FitResult (src/fit.rs)
struct MinimizationReport {
    int termination;
    int number_of_evaluations;
    double objective_function;
    bool was_successful() const { return termination > 0; }
};
struct FitResult {
    SeparableProblem problem;
    MinimizationReport minimization_report;
    const std::vector<double> &nonlinear_parameters() const { return problem.model().params(); } // src/fit.rs:113-115
    std::optional<std::vector<double>> linear_coefficients() const { return problem.linear_coefficients(); }
    std::optional<std::vector<double>> best_fit() const { // unweighted Phi C (src/fit.rs:55-59, 87-91)
        if (!problem.linear_coefficients()) return std::nullopt;
        return problem.batch().best_fit();
    }
    bool was_successful() const { return minimization_report.was_successful(); } // :120-122
};
// the Err(FitResult) arm of LevMarSolver::fit (src/solvers/levmar/mod.rs:248-253)
struct FitError : std::runtime_error {
    FitResult result;
    explicit FitError(FitResult r) : std::runtime_error("fit did not terminate successfully"), result(std::move(r)) {}
};

class LevMarSolver {
    LevenbergMarquardt solver_;

  public:
    LevMarSolver() = default;
    static LevMarSolver with_solver(LevenbergMarquardt s) {
        LevMarSolver l;
        l.solver_ = s;
        return l;
    }
    // consumes the problem; returns the FitResult on success, throws FitError(result) otherwise
    FitResult fit(SeparableProblem problem) const {
        std::vector<double> alpha = problem.params();
        std::vector<vp_report> rep = problem.batch().fit(alpha, solver_);
        problem.model_mut().set_params(alpha);
        FitResult res{std::move(problem), MinimizationReport{rep[0].termination, rep[0].n_evals, rep[0].objective}};
        if (!res.was_successful()) throw FitError(std::move(res));
        return res;
    }
};

} // namespace varpro
