// The kernel registry (varpro_amd/csrc/vp_registry.hpp) seen from a plain host program: no HIP header, no GPU.
//   usage: test_registry          check what the set builders guarantee; prints "<n> failure(s)"
//          test_registry --dump   one line per kernel set: registry() in order, then the generic and the external sets
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../varpro_amd/csrc/vp_registry.hpp"

using vp::KernelEntry;
using vp::launch_fn;

// the launcher's dynamic symbol; `local` for a function the library does not export
static std::string name_of(launch_fn f) {
    if (!f) return "null";
    Dl_info info;
    if (dladdr((void *)f, &info) && info.dli_sname && info.dli_saddr == (void *)f) return info.dli_sname;
    return "local";
}

static void dump(const char *table, size_t i, const KernelEntry &e) {
    std::printf("%s[%zu] dtype=%d family=%d a=%d b=%d c=%d R=%d W=%d mrhs_state_bytes=%zu gram_fit=%d mrhs_gx_cap=%d fit_lds_w=%zu "
                "uses_gen_ws=%d",
                table, i, e.dtype, e.family, e.a, e.b, e.c, e.R, e.W, e.mrhs_state_bytes, e.gram_fit, e.mrhs_gx_cap, e.fit_lds_w,
                e.uses_gen_ws);
    const struct {
        const char *slot;
        launch_fn f;
    } slots[] = {{"evaluate", e.evaluate},       {"basis", e.basis},
                 {"fit", e.fit},                 {"fit_single", e.fit_single},
                 {"fit_rescue", e.fit_rescue},   {"best_fit", e.best_fit},
                 {"mrhs_factor", e.mrhs_factor}, {"mrhs_stream", e.mrhs_stream},
                 {"mrhs_lm", e.mrhs_lm},         {"mrhs_finish", e.mrhs_finish},
                 {"stats", e.stats},             {"mrhs_fit_whole", e.mrhs_fit_whole}};
    for (const auto &s : slots) std::printf(" %s=%s", s.slot, name_of(s.f).c_str());
    std::printf("\n");
}

static int failures = 0;
static void expect(bool ok, size_t i, const char *what) {
    if (ok) return;
    ++failures;
    std::printf("FAIL registry[%zu]: %s\n", i, what);
}

int main(int argc, char **argv) {
    const std::vector<KernelEntry> &reg = vp::registry();
    if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) {
        for (size_t i = 0; i < reg.size(); ++i) dump("registry", i, reg[i]);
        const int dtypes[2] = {VP_F64, VP_F32};
        for (size_t i = 0; i < 2; ++i) dump("generic", i, *vp::generic_kernels(dtypes[i]));
        for (size_t i = 0; i < 2; ++i) dump("external", i, *vp::external_kernels(dtypes[i]));
        return 0;
    }
    expect(!reg.empty(), 0, "the registry is empty");
    for (size_t i = 0; i < reg.size(); ++i) {
        const KernelEntry &e = reg[i];
        expect(e.basis && e.best_fit, i, "basis and best_fit are in every set");
        const int n_mrhs = (e.mrhs_factor != nullptr) + (e.mrhs_stream != nullptr) + (e.mrhs_lm != nullptr) + (e.mrhs_finish != nullptr);
        expect(n_mrhs == 0 || n_mrhs == 4, i, "the multi-RHS launchers come as a group");
        expect(vp::has_mrhs_set(&e) == (n_mrhs == 4), i, "has_mrhs_set() names that group");
        if (n_mrhs == 4) expect(e.mrhs_state_bytes > 0, i, "a set with multi-RHS kernels states the size of their LM state");
        if (!e.evaluate) expect(!e.fit && !e.fit_single && !e.stats && !e.fit_rescue, i, "a set without evaluate has no single-RHS kernel");
        if (e.gram_fit) expect(e.fit && !e.fit_single, i, "the Gram fit is `fit` and replaces fit_single");
        if (e.fit_rescue)
            expect(e.fit_single && e.family == vp::FAMILY_MULTIEXP, i, "the scaled re-fit belongs to a multi-exponential set's fit_single");
        if (e.uses_gen_ws) expect(e.mrhs_fit_whole && !e.fit, i, "a set on the generic workspace fits S > 1 whole and has no slot kernel");
    }
    std::printf("%zu kernel sets, %d failure(s)\n", reg.size(), failures);
    return failures ? 1 : 0;
}
