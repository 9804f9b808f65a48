// vel_targets_check.cpp — beom_dense::vel_targets_zero (beom_amd/csrc/beom_dense_host.h) on arrays fnud(0:ndeg, nlay, 3) of
// exactly the caller's size (test_zero_lanes_cpu.py builds this with ASan and UBSan and runs it; exit status 0 = all held).
// The thickness targets (component 1) are never zero here: the scan must not look at them, and must look at every word of
// the two velocity components, slot 0 and the last slot of the last layer included.
#include "../beom_amd/csrc/beom_dense_host.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

namespace {

int g_checks = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                        \
            std::fprintf(stderr, "\n");                                               \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

// a heap array of exactly 3 * nlay * n1 doubles (a read past either end is ASan's to report): thickness targets 1000 + k,
// velocity targets +0
std::unique_ptr<double[]> targets(size_t n1, size_t nlay) {
    std::unique_ptr<double[]> f(new double[3 * nlay * n1]);
    for (size_t k = 0; k < 3 * nlay * n1; ++k) f[k] = k < nlay * n1 ? 1000.0 + (double)k : 0.0;
    return f;
}

size_t at(size_t n1, size_t nlay, size_t ip, size_t il, size_t iv) { return ip + n1 * (il + nlay * iv); }   // 0-based il, iv

void check(size_t n1, size_t nlay) {
    const auto zero = targets(n1, nlay);
    CHECK(beom_dense::vel_targets_zero(zero.get(), n1, nlay) == 1, "all +0, n1 %zu nlay %zu", n1, nlay);
    CHECK(beom_dense::vel_targets_zero(nullptr, n1, nlay) == 0, "no array");
    const double odd[3] = {-0.0, std::numeric_limits<double>::denorm_min(), std::numeric_limits<double>::quiet_NaN()};
    const char *const name[3] = {"-0.0", "a denormal", "a NaN"};
    CHECK(std::signbit(odd[0]) && odd[0] == 0.0 && odd[1] > 0.0 && odd[1] < std::numeric_limits<double>::min() && odd[2] != odd[2],
          "the three values are what they are called");
    const size_t slots[2] = {0, n1 - 1}, layers[2] = {0, nlay - 1};
    for (int v = 0; v < 3; ++v)
        for (size_t iv = 1; iv <= 2; ++iv)
            for (size_t ip : slots)
                for (size_t il : layers) {
                    const auto f = targets(n1, nlay);
                    f[at(n1, nlay, ip, il, iv)] = odd[v];
                    CHECK(beom_dense::vel_targets_zero(f.get(), n1, nlay) == 0, "%s at slot %zu, layer %zu, component %zu (n1 %zu, nlay %zu)",
                          name[v], ip, il + 1, iv + 1, n1, nlay);
                }
    // a zero thickness target of either sign is none of the scan's business
    const auto f = targets(n1, nlay);
    f[at(n1, nlay, n1 - 1, nlay - 1, 0)] = -0.0;
    f[0] = 0.0;
    CHECK(beom_dense::vel_targets_zero(f.get(), n1, nlay) == 1, "thickness targets are not scanned");
}

}  // namespace

int main() {
    for (size_t nlay : {(size_t)1, (size_t)4})
        for (size_t n1 : {(size_t)1, (size_t)2, (size_t)37})
            check(n1, nlay);
    std::printf("%d checks held\n", g_checks);
    return 0;
}
