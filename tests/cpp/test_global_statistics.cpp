// C++ mirror (varpro.hpp BatchProblem::global_statistics): a global fit of S = 3 double-exponential right-hand sides,
// its statistics and Student-t band; without a GPU the handle cannot be made and the program says so.
//   usage: test_global_statistics [gpu]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../varpro_amd/cpp/varpro.hpp"

using namespace varpro;

static int failures = 0;
#define EXPECT(cond)                                                                     \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);               \
            ++failures;                                                                  \
        }                                                                                \
    } while (0)

int main(int argc, char **argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    const int64_t m = 400, S = 3;
    std::vector<double> x((size_t)m), Y((size_t)(S * m));
    for (int64_t i = 0; i < m; ++i) x[(size_t)i] = 10.0 * (double)i / (double)(m - 1);
    for (int64_t s = 0; s < S; ++s)
        for (int64_t i = 0; i < m; ++i)
            Y[(size_t)(s * m + i)] = (1.0 + (double)s) * std::exp(-x[(size_t)i] / 1.0) + 2.0 * std::exp(-x[(size_t)i] / 4.0) +
                                     0.3 + 1e-2 * std::sin(78.233 * (double)(i + 1) * (double)(s + 2));
    SeparableModel model = SeparableModelBuilder({"tau1", "tau2"})
                               .initial_parameters({1.3, 3.2})
                               .function({"tau1"}, Basis::ExpDecay).partial_deriv("tau1")
                               .function({"tau2"}, Basis::ExpDecay).partial_deriv("tau2")
                               .invariant_function(Basis::Const)
                               .independent_variable(x)
                               .build();
    try {
        BatchProblem bp(model, Y, 1, S);
        std::vector<double> alpha = {1.3, 3.2};
        auto rep = bp.fit(alpha);
        EXPECT(rep[0].termination > 0);
        auto g = bp.global_statistics(true);
        EXPECT(g.status[0] == 0);
        EXPECT(g.dof == m * S - 3 * S - 2);
        EXPECT(g.cov_alpha[0] > 0 && g.cov_alpha[3] > 0 && std::fabs(g.cov_alpha[1] - g.cov_alpha[2]) <= 1e-12 * g.cov_alpha[0]);
        for (int64_t s = 0; s < S; ++s)
            for (int a = 0; a < 3; ++a) EXPECT(g.coef_cov[(size_t)((s * 3 + a) * 3 + a)] > 0);
        auto r = g.confidence_band_radius(0, 1, 0.9);
        EXPECT((int64_t)r.size() == m);
        const double tq = student_t_quantile(0.95, (double)g.dof);
        for (int64_t i = 0; i < m; ++i) EXPECT(std::fabs(r[(size_t)i] - tq * g.conf_sigma[(size_t)(m + i)]) <= 1e-14 * r[(size_t)i]);
        auto g0 = bp.global_statistics(false);
        EXPECT(g0.conf_sigma.empty());
        EXPECT(std::memcmp(g0.cov_alpha.data(), g.cov_alpha.data(), 4 * sizeof(double)) == 0);
        std::printf("global fit: tau = (%.6f, %.6f), sd = (%.3e, %.3e), reduced chi2 %.4e\n", alpha[0], alpha[1],
                    std::sqrt(g.cov_alpha[0]), std::sqrt(g.cov_alpha[3]), g.reduced_chi2[0]);
    } catch (const HipError &e) {
        std::printf("no device: %s\n", e.what());
        EXPECT(!gpu);
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
