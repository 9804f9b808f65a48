// step_plan_check.cpp — beom_plan::plan_step (beom_amd/csrc/beom_plan.h), the decision "which form does step tstp of this
// handle run", without a GPU (test_step_plan_cpu.py builds this with ASan and UBSan and runs it; exit status 0 = all held).
//
// 1. The invariants beom_engine.hip's dispatcher relies on, over combinations of the 24 boolean facts and options with
//    tstp 1..8, n_3d 1..2, nlay {1, 8, 9}, dvis {0, 1e-3, 2e-3}, svis {0, > 0}, mont_levels_valid 0..3 (g_fb = 1, bvis = 0,
//    ocrp = 0).  The whole product is 2^24 x 1152 = 1.9e10 plans, minutes of work: `step_plan_check full` walks all of it.
//    Without an argument the program walks three cuts through it that a test can afford (1.8e7 plans; under UBSan every
//    load of a bool is checked, which is most of what a plan costs):
//      A  at one setting of the other arguments (step 4 of eight layers, levels kept) every combination of the booleans
//         in which has_stress is what the engine makes it, the OR of the three terms and the three uploads (2^23),
//      B  all 1152 settings of the other arguments x every combination of the 8 options x 2^5 kinds of handle, in which
//         the booleans that stand for one cause move together (the four forcing flags; wind, bot, top and their fold),
//      C  the 1152 settings with g_fb, bvis, ocrp at both of their values, all options on and each one off, on six dense
//         handles: plain, with kept levels, with a lid, with uploaded stress arrays next to the engine's own terms and
//         without them, with a non-zero viscosity uploaded.
// 2. The rows DESIGN.md and the GPU tests state, with the expected values written here from those texts.
#include "../beom_amd/csrc/beom_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

using beom_plan::StepFacts;
using beom_plan::StepPlan;
using beom_plan::plan_step;

namespace {

long long g_checks = 0;
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

// the twelve instantiations of the fused u+v sweep per tile geometry and u/v order: (sf, prod, zv, hm, plain)
const bool kForms[12][5] = {
    {0, 1, 0, 0, 1}, {0, 1, 1, 0, 1}, {0, 1, 0, 1, 1}, {0, 1, 1, 1, 1},      // plain: zv x hm
    {0, 1, 0, 1, 0}, {0, 1, 1, 1, 0},                                      // hm
    {1, 1, 1, 0, 0}, {1, 1, 0, 0, 0}, {1, 0, 0, 0, 0},                      // k_uv_fused_sf: (prod, zv) = 11, 10, 00
    {0, 1, 1, 0, 0}, {0, 1, 0, 0, 0}, {0, 0, 0, 0, 0}};                     // general
bool is_form(bool sf, bool prod, bool zv, bool hm, bool plain) {
    for (const auto &k : kForms)
        if (k[0] == sf && k[1] == prod && k[2] == zv && k[3] == hm && k[4] == plain) return true;
    return false;
}

// bits 0..15: the handle, 16..23: the options
StepFacts facts(unsigned bits, int nlay, double dvis, double svis, int levels, double g_fb = 1.0, double bvis = 0.0, double ocrp = 0.0) {
    StepFacts f{};
    bool *const flag[24] = {&f.dense, &f.lid, &f.has_nudg, &f.has_tide, &f.has_stress, &f.has_bodf, &f.has_hto,
                            &f.wind, &f.bot, &f.top, &f.up_tt, &f.up_tb, &f.up_tu, &f.fold_static_ok, &f.visc_all_zero, &f.mont_keep,
                            &f.fuse, &f.fuse_uv, &f.fold_stress, &f.lean_d2h, &f.lean_visc, &f.mont_history, &f.plain_sweeps, &f.keep_diag};
    for (int b = 0; b < 24; ++b) *flag[b] = ((bits >> b) & 1u) != 0;
    f.nlay = nlay; f.dvis = dvis; f.svis = svis; f.bvis = bvis; f.g_fb = g_fb; f.ocrp = ocrp;
    f.mont_levels_valid = levels;
    return f;
}

void invariants(const StepFacts &f, int tstp, int n_3d) {
    const StepPlan p = plan_step(f, tstp, 0.0, 0.01, 0.05, 0.0, n_3d);
    const char *const fmt = "tstp %d n_3d %d nlay %d dvis %g svis %g levels %d";
#define WHERE fmt, tstp, n_3d, f.nlay, f.dvis, f.svis, f.mont_levels_valid
    CHECK(p.tstp == tstp && p.n_3d == n_3d && p.first3 == (tstp <= 3) && p.uv.first_x == (tstp % 2 == 0), WHERE);
    CHECK(!p.uv.zv || p.uv.prod, WHERE);
    CHECK(!p.uv.hm || p.uv.prod, WHERE);
    CHECK(!p.uv.plain || p.uv.prod, WHERE);
    CHECK(!p.uv.hm || (p.gene != 0.0 && !p.stress_fold && f.mont_levels_valid >= 3 && f.mont_keep && !p.needs_arrays), WHERE);
    CHECK(p.needs_arrays == !p.uv.hm, WHERE);
    CHECK(!p.uv.plain || (!p.stress_fold && !f.has_nudg && !f.has_tide && !f.has_stress && !f.has_bodf && !f.lid && f.svis == 0.0), WHERE);
    CHECK(!p.mont.zero_visc || !p.leith, WHERE);
    CHECK(!p.stress_fold || (!p.first3 && p.n_3d == 1 && p.uv.fused_uv), WHERE);
    CHECK(!(p.stress_fold && p.launch_stress), WHERE);
    CHECK(p.launch_visc == (!p.uv.prod && (p.first3 || p.leith || f.svis > 0.0)), WHERE);
    CHECK(p.uv.prod == p.mont.fused, WHERE);
    CHECK(!p.uv.prod || (f.nlay >= 1 && f.nlay <= 8), WHERE);
    CHECK(p.mont.fused || !(p.mont.keep_visc || p.mont.lean_d2h || p.mont.zero_visc || p.mont.plain), WHERE);
    CHECK(p.uv.fused_uv || !(p.uv.zv || p.uv.hm || p.uv.plain || p.stress_fold), WHERE);
    if (p.uv.fused_uv) {
        CHECK(is_form(p.stress_fold, p.uv.prod, p.uv.zv, p.uv.hm, p.uv.plain), WHERE);
        CHECK(beom_plan::uv_form_exists(p.stress_fold, p.uv.prod, p.uv.zv, p.uv.hm, p.uv.plain), WHERE);
    }
#undef WHERE
}

const int kNlay[3] = {1, 8, 9};
const double kDvis[3] = {0.0, 1.e-3, 2.e-3}, kSvis[2] = {0.0, 1.e-4};

// f(tstp, n_3d, nlay, dvis, svis, levels) for all 1152 settings
template <class F>
void for_arguments(F &&f) {
    for (int tstp = 1; tstp <= 8; ++tstp)
        for (int n_3d = 1; n_3d <= 2; ++n_3d)
            for (int nlay : kNlay)
                for (double dvis : kDvis)
                    for (double svis : kSvis)
                        for (int levels = 0; levels <= 3; ++levels) f(tstp, n_3d, nlay, dvis, svis, levels);
}

void enumerate(bool full) {
    if (full) {
        for_arguments([](int tstp, int n_3d, int nlay, double dvis, double svis, int levels) {
            for (unsigned bits = 0; bits < (1u << 24); ++bits) invariants(facts(bits, nlay, dvis, svis, levels), tstp, n_3d);
        });
        return;
    }
    for (unsigned bits = 0; bits < (1u << 24); ++bits)                                                    // A
        if (((bits & 0x10u) != 0) == ((bits & 0x1F80u) != 0)) invariants(facts(bits, 8, 0.0, 0.0, 3), 4, 1);
    // a kind of handle: bit 0 dense, 1 lid, 2 forcing, 3 stress terms (and they can fold), 4 mont_keep, 5 not visc_all_zero,
    // 6 uploads
    auto kind = [](unsigned k, unsigned options) {
        const bool forcing = k & 4u, terms = k & 8u, uploads = k & 64u;
        return (k & 3u) | (forcing ? 0x6Cu : 0u) | (terms ? 0x2380u : 0u) | (uploads ? 0x1C00u : 0u) | ((terms || uploads) ? 0x10u : 0u) |
               ((k & 16u) ? 0x8000u : 0u) | ((k & 32u) ? 0u : 0x4000u) | (options << 16);
    };
    for_arguments([&](int tstp, int n_3d, int nlay, double dvis, double svis, int levels) {
        for (unsigned options = 0; options < 256; ++options)                                                            // B
            for (unsigned k = 0; k < 32; ++k) invariants(facts(kind(k, options), nlay, dvis, svis, levels), tstp, n_3d);
        for (int off = -1; off < 8; ++off)                                                                              // C
            for (unsigned c = 0; c < 8; ++c)
                for (unsigned k : {0x01u, 0x11u, 0x03u, 0x49u, 0x41u, 0x21u})
                    invariants(facts(kind(k, off < 0 ? 0xFFu : 0xFFu & ~(1u << off)), nlay, dvis, svis, levels, c & 1 ? 0.0 : 1.0,
                                     c & 2 ? 1.e-4 : 0.0, c & 4 ? 1.0 : 0.0), tstp, n_3d);
    });
}

// ---- the rows the documents state ------------------------------------------------------------------------------------
StepFacts defaults(int nlay, double dvis) {      // a whole dense frame, no lid, no forcing, every option at its default
    StepFacts f{};
    f.dense = true; f.nlay = nlay; f.dvis = dvis; f.g_fb = 1.0;
    f.visc_all_zero = true; f.mont_keep = true;
    f.fuse = f.fuse_uv = f.fold_stress = f.lean_d2h = f.lean_visc = f.mont_history = f.plain_sweeps = true;
    return f;
}
StepFacts windy(int nlay) {                      // wind and bottom drag on constant fractions: the stress can fold
    StepFacts f = defaults(nlay, 0.0);
    f.wind = f.bot = f.has_stress = f.fold_static_ok = true;
    return f;
}
// steps 1..8 of one handle, one call each: the levels the buffers hold grow with the steps ("State machine")
template <class F>
void run8(StepFacts f, F &&row) {
    for (int tstp = 1; tstp <= 8; ++tstp) {
        const StepPlan p = plan_step(f, tstp, 0.0, 0.01, 0.05, 0.0, 1);
        row(tstp, p);
        if (f.mont_keep && f.mont_levels_valid < 3) ++f.mont_levels_valid;
    }
}

void rows() {
    // bench.py's flow (DESIGN.md "History from Montgomery"; test_gpu_plain_sweeps.py): steps 1-3 on the arrays with gene = 0,
    // every later step the form, and both sweeps plain (plain_sweeps == 3)
    run8(defaults(4, 0.2), [](int t, const StepPlan &p) {
        CHECK(p.uv.fused_uv && p.mont.fused && p.leith && !p.launch_visc && !p.stress_fold, "headline, step %d", t);
        if (t <= 3) CHECK(p.gene == 0.0 && !p.uv.hm && p.needs_arrays && p.rebuild, "headline, step %d", t);
        else CHECK(p.gene == 1.0 && p.uv.hm && !p.needs_arrays && !p.rebuild && p.uv.plain && p.mont.plain, "headline, step %d", t);
    });
    // the wind-driven frame folds its stress from step 4 (steps 2 and 3 reuse step 1's launch), and a folded step stays on
    // the arrays with the general Montgomery sweep's plain form only
    run8(windy(2), [](int t, const StepPlan &p) {
        CHECK(p.stress_fold == (t >= 4) && p.launch_stress == (t == 1), "wind, step %d", t);
        CHECK(!p.uv.hm && !p.uv.plain && p.needs_arrays, "wind, step %d", t);
        CHECK(p.mont.fused == (t >= 4) && p.launch_visc == (t <= 3), "wind (dvis = 0), step %d", t);
        if (t >= 4) CHECK(p.uv.zv && p.mont.zero_visc && p.mont.lean_d2h, "wind, step %d", t);
    });
    // keep_diag = 1 clears lean_d2h, zero_visc, the Montgomery sweep's plain form and the fold; the u+v sweep stores no
    // diagnostic and keeps its plain form (test_gpu_plain_sweeps.py: keep_diag flips the Montgomery bit only)
    for (StepFacts f : {defaults(2, 0.0), defaults(4, 0.2), windy(2)}) {
        f.keep_diag = true;
        run8(f, [&](int t, const StepPlan &p) {
            CHECK(!p.mont.lean_d2h && !p.mont.zero_visc && !p.uv.zv && !p.mont.plain && !p.stress_fold, "keep_diag, step %d", t);
            CHECK(p.uv.plain == (!f.has_stress && p.uv.prod), "keep_diag, step %d", t);
        });
    }
    // fold_stress = 0 with wind keeps the launch and lets the form run (test_gpu_mont_history.py: stommel_wind_drag)
    StepFacts f = windy(2);
    f.fold_stress = false;
    run8(f, [](int t, const StepPlan &p) {
        CHECK(!p.stress_fold && p.launch_stress == (t == 1 || t >= 4) && p.uv.hm == (t >= 4) && !p.uv.plain, "fold_stress = 0, step %d", t);
    });
    // a lid handle (fuse = fuse_uv = 0, no kept levels) never takes the form and runs with gene = 0
    f = defaults(2, 0.0);
    f.lid = true; f.fuse = f.fuse_uv = false; f.mont_keep = false; f.ocrp = 1.0;
    run8(f, [](int t, const StepPlan &p) {
        CHECK(p.gene == 0.0 && !p.uv.hm && !p.uv.fused_uv && !p.mont.fused && !p.uv.prod && !p.uv.plain && !p.mont.plain, "lid, step %d", t);
    });
    // the table of forms: twelve, and the header's predicate names the same twelve
    int n = 0;
    for (int c = 0; c < 32; ++c) {
        const bool sf = c & 1, prod = c & 2, zv = c & 4, hm = c & 8, plain = c & 16;
        CHECK(beom_plan::uv_form_exists(sf, prod, zv, hm, plain) == is_form(sf, prod, zv, hm, plain), "form %d", c);
        n += is_form(sf, prod, zv, hm, plain);
    }
    CHECK(n == 12, "%d forms", n);
    // the scalars of integrate_time: the ramp is set once for steps 1-3, then follows ctim; n_3d = 2 refreshes on even steps
    const StepPlan a = plan_step(defaults(2, 0.2), 2, 1.0, 0.5, 4.0, 0.0, 2), b = plan_step(defaults(2, 0.2), 5, 1.0, 0.5, 4.0, 0.0, 2);
    CHECK(a.ctim == 2.0 && a.ramp == 1.5 / 4.0 && a.upst && a.leith && a.mont.keep_visc, "step 2 of n_3d = 2");
    CHECK(b.ctim == 3.5 && b.ramp == 3.5 / 4.0 && !b.upst && !b.leith && !b.mont.keep_visc && !b.launch_stress, "step 5 of n_3d = 2");
    CHECK(plan_step(defaults(2, 0.2), 5, 1.0, 0.5, 4.0, 1.0, 2).ramp == 1.0, "a restart has no ramp");
}

}  // namespace

int main(int argc, char **argv) {
    rows();
    enumerate(argc > 1 && !std::strcmp(argv[1], "full"));
    std::printf("%lld checks held\n", g_checks);
    return 0;
}
