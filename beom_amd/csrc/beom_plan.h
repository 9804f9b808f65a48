// beom_plan.h — which form does step `tstp` of a handle run?  The one place that decides it: plan_step() takes the facts
// of the handle and the step's arguments and returns a StepPlan; beom_engine.hip executes the plan and decides nothing
// (apply_plan, step_front, launch_mont_visc, launch_uv_fused).  Host only, no HIP header: tests/step_plan_check.cpp
// enumerates it without a GPU.  The scalars are those of integrate_time (private_mod.f95:1858-1901).
#pragma once

namespace beom_plan {

// What the decisions read, and nothing else (facts_of in beom_engine.hip fills it from the handle).
struct StepFacts {
    // the handle
    // lid: rgld > 0.5, the engine's own test.  The two plain gates read !(rgld >= 0.5), the kernels' test, before they moved
    // here; rgld is a switch of 0 or 1, so !lid is the same gate for every value a caller passes (it differs at 0.5 alone).
    bool dense; int nlay; bool lid;
    double svis, dvis, bvis, g_fb, ocrp;
    bool has_nudg, has_tide, has_stress, has_bodf, has_hto;      // DevView's flags (has_stress: uploaded stresses count)
    bool wind, bot, top, up_tt, up_tb, up_tu;   // distribute_stress's three terms | a non-zero tt3d / tb3d / tu3d was uploaded
    bool fold_static_ok, visc_all_zero, mont_keep;
    // options (beom_set_option)
    bool fuse, fuse_uv, fold_stress, lean_d2h, lean_visc, mont_history, plain_sweeps, keep_diag;
    // moving state
    int mont_levels_valid;
};

struct StepPlan {
    int tstp, n_3d;
    double ctim, ramp, gene;
    // stress_fold:   distribute_stress inside the fused momentum sweep (k_uv_fused_sf; beom_info "stress_folded")
    // launch_stress: ... or as its own launch in front of the step
    // rebuild:       steps 1-3 rebuild the transports (:2166-2177; a lid: centred instead of upstream)
    // leith:         this step refreshes the Leith viscosity (:2188, :2268)
    // launch_visc:   update_viscosity as its own sweep
    // needs_arrays:  the step works on the history arrays dmx, dmy: hist_sync runs first
    bool first3, upst, stress_fold, launch_stress, rebuild, leith, launch_visc, needs_arrays;
    // The Montgomery sweep.
    // fused:     Montgomery + Leith in one sweep (k_mont_visc); else update_mont, then launch_visc
    // keep_visc: a refreshed viscosity has to stand for later steps (n_3d > 1)
    // lean_d2h:  d2hx, d2hy stored only where the fused u+v sweep reads them
    // zero_visc: v_cc = v_ll = +0 and never refreshed: the viscous products are +-0
    // plain:     the instantiation with the optional forcing compiled out (beom_info "plain_sweeps" bit 1)
    struct Mont { bool fused, keep_visc, lean_d2h, zero_visc, plain; } mont;
    // The momentum sweep.
    // fused_uv: update_u + update_v in one sweep (k_uv_fused); else two launches of k_update_uv
    // first_x:  update_u first (even tstp, :2193-2199,2276-2282)
    // prod:     the Montgomery sweep staged the viscous products pcd, qlr
    // zv:       ... and they are +-0: the sweep skips the term
    // hm:       the history-from-Montgomery form (beom_info "mont_history")
    // plain:    the instantiation with the optional forcing compiled out (beom_info "plain_sweeps" bit 0)
    struct Uv { bool fused_uv, first_x, prod, zv, hm, plain; } uv;
};

// update_u + update_v in one sweep: a fact of the handle, the same for every step (beom_step_phase's -20 rests on it)
// (svis > 0: the v_cc / v_ll form, uu4 and vv4 read through L2)
inline bool fuses_uv(const StepFacts &f) { return f.dense && f.fuse_uv; }

inline bool can_fuse(const StepFacts &f, bool first3) {
    // either every step refreshes the viscosity (dvis > 1e-3 and n_3d = 1, :2268) — Montgomery + Leith
    // in one sweep — or no step after the third ever does (dvis <= 1e-3, svis = 0): v_cc, v_ll stand
    // and the sweep forms their products with this step's dive, rvor
    if (!(f.dense && f.fuse && f.nlay <= 8) || f.svis > 0.0) return false;
    if (f.dvis > 1.e-3) return true;              // refresh steps: Leith in the sweep; others: standing v_cc, v_ll
    return !first3;                               // steps 1-3 call update_viscosity unconditionally (:2188)
}

inline StepPlan plan_step(const StepFacts &f, int tstp, double tres, double dtd8, double dt_r, double rsta, int n_3d) {
    StepPlan p{};
    p.tstp = tstp;
    p.ctim = tres + dtd8 * (double)tstp;                           // :1862,1887
    p.first3 = tstp <= 3;
    p.ramp = 1.0;
    bool stress;
    if (p.first3) {
        const double c1 = tres + dtd8 * 1.0;                       // ramp is set once, at tstp = 1 (:1864-1866)
        if (rsta < 0.5 && c1 < dt_r) p.ramp = c1 / dt_r;
        p.upst = true;                                             // update_viscosity is unconditional (:2188)
        stress = tstp == 1;                                        // :1863
    } else {
        if (rsta < 0.5 && p.ctim < dt_r) p.ramp = p.ctim / dt_r;   // :1898-1901
        p.upst = (tstp % n_3d) == 0;                               // :1889-1892
        stress = p.upst;                                           // :1894-1896
    }
    p.gene = (p.first3 || (f.lid && f.g_fb > 0.5)) ? 0.0 : f.g_fb;      // :1859,1877; :1880-1884: no multistep with a lid
    p.n_3d = n_3d;
    p.rebuild = p.first3;
    p.mont.fused = can_fuse(f, p.first3);
    p.uv.fused_uv = fuses_uv(f);
    p.uv.first_x = tstp % 2 == 0;
    // distribute_stress of this step inside its fused momentum sweep (uv_core): the fractions are constants (ocrp = 0), every
    // step refreshes the stress (so tt3d, tb3d, tu3d are never read back; steps 2 and 3 reuse step 1's, :1863), and an array
    // the engine does not refresh holds nothing but zeros.  The three arrays then keep their values of step 3 ("keep_diag" = 1
    // keeps them current).
    p.stress_fold = f.fold_stress && f.fold_static_ok && p.uv.fused_uv && stress && !p.first3 && p.n_3d == 1 && !f.keep_diag &&
                    (f.wind || !f.up_tt) && (f.bot || !f.up_tb) && (f.top || !f.up_tu);
    p.launch_stress = stress && !p.stress_fold;
    p.leith = f.dvis > 1.e-3 && p.upst;
    // The Montgomery sweep.  :2187-2188, 2266-2269 in one sweep: can_fuse has excluded the columns k_mont_visc has no
    // instantiation for (nlay > 8), so the products are staged whenever the sweep is fused
    p.uv.prod = p.mont.fused;
    if (p.mont.fused) {
        const bool uv_fused_follows = p.uv.fused_uv;
        p.mont.lean_d2h = uv_fused_follows && f.lean_d2h && !f.keep_diag;
        p.mont.keep_visc = p.leith && p.n_3d > 1;
        p.mont.zero_visc = !p.leith && uv_fused_follows && f.lean_visc && f.visc_all_zero && f.dvis == 0.0 && f.bvis == 0.0 &&
                           !f.keep_diag;
        // plain: nothing of what PLAIN compiles out of body_mont_visc is asked for by this launch
        p.mont.plain = f.plain_sweeps && f.ocrp == 0.0 && !f.lid && !f.has_hto && !f.keep_diag && !p.mont.keep_visc;
    }
    p.launch_visc = !p.uv.prod && (p.first3 || p.leith || f.svis > 0.0);     // :2188,2268
    if (p.uv.fused_uv) {
        p.uv.zv = p.uv.prod && p.mont.zero_visc;
        // plain: a staged sweep (not the _sf kernel) of a handle with nothing of what PLAIN compiles out of uv_core
        p.uv.plain = f.plain_sweeps && p.uv.prod && !p.stress_fold && !f.has_nudg && !f.has_tide && !f.has_stress && !f.has_bodf &&
                     !f.lid && f.svis == 0.0;
    }
    // The history-from-Montgomery form of the fused u+v sweep: the option is on; the handle keeps the levels (a whole dense
    // frame, no lid); the step takes the fused u+v sweep with the products staged (k_mont_visc runs for every nlay <= 8,
    // which mont_keep implies) and the multistep term live; its stress does not fold (k_uv_fused_sf stays on the arrays);
    // and the buffers hold the three steps before this one.
    p.uv.hm = f.mont_history && f.mont_keep && p.mont.fused && p.uv.fused_uv && p.gene != 0.0 && !p.stress_fold &&
              f.mont_levels_valid >= 3;
    p.needs_arrays = !p.uv.hm;
    return p;
}

// The twelve instantiations of the fused u+v sweep per tile geometry and u/v order, as (prod, zv, hm, plain) with sf =
// stress_fold: k_uv_fused_sf and the general k_uv_fused take (prod, zv) in {11, 10, 00}; hm and plain are forms of the
// staged k_uv_fused only (4 plain: zv x hm; 2 hm: zv).  raw_uv_fused compiles exactly these.
constexpr bool uv_form_exists(bool sf, bool prod, bool zv, bool hm, bool plain) { return !((zv || hm || plain) && !prod) && !(sf && (hm || plain)); }

}  // namespace beom_plan
