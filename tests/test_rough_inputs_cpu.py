"""The rough inputs of rough_inputs.py, judged on the CPU before the GPU tests rely on them: on the inputs and on the
oracle's result only, never on a handle's.

Rough: every roughened array differs from its copy shifted by one cell in x, one cell in y, one layer and one level at 80 %
or more of the places.  Straddling: with ocrp = 1, at least 10 % of the wet cell-layers lie below 2 hsal and at least 10 %
above, in every layer.  Bounded: after step plan A (steps 1-5) and B (steps 7-12) the oracle's fields are finite, wet
thicknesses positive and max |u|, |v| <= 20 U, so that no blow-up swamps the small terms.  Liveness: re-seeding one input
alone changes the oracle's state after plan B, unless the configuration's parameters switch that term off
(rough_inputs.switched_off says which, and the test holds it to that list in both directions).

Three more conditions for the configurations that exist for one kernel family each: the private_mod3d epilogue's threshold
is straddled inside its sponge and changes the result; the rough lid states drive every pressure solve to its cap of 1000
sweeps; and two lid runs from rest give the counts of sweeps that reach the other paths of the engine's batched solve."""
import numpy as np
import pytest

import oracle_lib
import rough_inputs as RI
import tracers_ref as T
from helpers import same, same_bits

PLANS = {"A": (1, 5), "B": (7, 6)}
MUST_BE_LIVE = ("h_to", "taus:0", "taus:1", "bodf", "rs_h:0", "rs_h:1", "dmdx:0", "dmdx:1", "dmdx:2", "dmdy:0", "dmdy:1", "dmdy:2",
                "v_cc", "v_ll", "tt3d", "tb3d", "tu3d", "hdot", "tide", "nudg", "fnud", "fcor", "h_th", "hlay", "u", "v", "h_u", "h_v",
                "pi_s")
LIDS = ("lid_wind_drag_2l", "lid_coast_3l")
_DEAD = {}


def _oracle_after(g, plan, variant=0):
    o = oracle_lib.Oracle(g, variant=variant)
    o.step(*PLANS[plan])
    return o.state()


def _sweeps_per_step(g, first, nsteps):
    """The oracle's Gauss-Seidel sweeps of every step's solve, one step per call."""
    o = oracle_lib.Oracle(g)
    out = []
    for t in range(first, first + nsteps):
        before = o.lid_sweeps()
        o.step(t, 1)
        after = o.lid_sweeps()
        assert after["solves"] == before["solves"] + 1 and after["sweeps"] == before["sweeps"] + after["last"]
        out.append(after["last"])
    return out


@pytest.mark.parametrize("frame", ["130x18", "321x50"])
@pytest.mark.parametrize("config", list(RI.CONFIGS))
def test_rough_straddling_bounded(config, frame):
    f = RI.base_fields(config, frame)
    lid = float(f.p.rgld) > 0.5
    assert ("pi_s" in RI.present(f)) == lid
    before = {k: np.array(getattr(f, k), copy=True) for k in RI.present(f)}
    g = RI.rough_fields(f, 1)
    for k in RI.present(f):
        assert same_bits(getattr(f, k), before[k]), (k, "the shared object was written")
    assert ("pi_s" in g.rough_support) == lid
    if lid:
        assert float(f.p.g_fb) == 0.0
        w = g.mk_n > 0.5
        assert np.all(g.pi_s[w] != 0.0) and np.all(np.abs(g.pi_s) <= 10.0) and np.all(g.pi_s[~w] == 0.0)
        fr = RI.shifted_fractions(g, "pi_s")
        assert "x" in fr and "y" in fr, (config, fr)
    for k in g.rough_support:
        for shift, frac in RI.shifted_fractions(g, k).items():
            assert frac >= 0.8, (config, frame, k, shift, frac)
    for k in ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy", "fcor", "h_to", "h_th"):
        fr = RI.shifted_fractions(g, k)
        assert "x" in fr and "y" in fr, (config, k, fr)
        assert ("layer" in fr) == (RI.AXES[k][1] is not None and f.p.nlay > 1) and ("level" in fr) == (RI.AXES[k][2] is not None), (config, k, fr)
    assert len(set(g.bodf.ravel())) == g.bodf.size and np.all(g.bodf != 0.0)
    wet = g.mk_n > 0.5
    assert np.all(g.h_to[wet] != 0.0)
    open_u = np.broadcast_to((g.mk_u > 0.5)[None], g.u.shape)
    zero = g.u[open_u] == 0.0
    neg = zero & np.signbit(g.u[open_u])
    assert 0.03 <= neg.mean() <= 0.07 and 0.03 <= (zero & ~neg).mean() <= 0.07, (neg.mean(), zero.mean())
    assert np.array_equal(g.nudg == 0.0, f.nudg == 0.0)                  # exact 0 outside the sponge: the ng == 0 shortcuts
    if float(f.p.ocrp) > 0.5:
        for k, (below, above) in enumerate(RI.straddling(g)):
            assert below >= 0.10 and above >= 0.10, (config, frame, k, below, above)
    for plan in PLANS:
        growth = RI.bounded(g, _oracle_after(g, plan, RI.variant_of(config)))
        print("%s %s plan %s: growth %.2f" % (config, frame, plan, growth))


@pytest.mark.parametrize("config", list(RI.CONFIGS))
def test_liveness(config):
    f = RI.base_fields(config, "130x18")
    variant = RI.variant_of(config)
    ref = {k: v.copy() for k, v in _oracle_after(RI.rough_fields(f, 1), "B", variant).items()}
    dead = set()
    for x in RI.INPUTS:
        st = _oracle_after(RI.rough_fields(f, 1, reseed=(x,)), "B", variant)
        if all(same_bits(st[k], ref[k]) for k in ("hlay", "u", "v", "h_u", "h_v")):
            dead.add(x)
    _DEAD[config] = dead
    assert dead == RI.switched_off(f.p, f), (config, sorted(dead), sorted(RI.switched_off(f.p, f)))


def test_every_term_is_live_somewhere():
    for config in RI.CONFIGS:
        if config not in _DEAD:
            test_liveness(config)
    for x in MUST_BE_LIVE:
        assert any(x not in _DEAD[c] for c in RI.CONFIGS), (x, "dead in every configuration")
    for c in LIDS:
        assert "pi_s" not in _DEAD[c], (c, "the starting pressure is dead")
    assert "taus:0" not in _DEAD["sill_ocrp_stress_3l"]


def test_variant_epilogue_straddles_its_threshold_and_changes_the_result():
    """variant3d_sponge_3l: inside the eastern sponge layer 3 lies on both sides of 20 hsal (the branches of
    private_mod3d.f95:1636-1683), and the oracle with variant = 1 differs from variant = 0 after plan B."""
    for frame in ("130x18", "321x50"):
        f = RI.base_fields("variant3d_sponge_3l", frame)
        g = RI.rough_fields(f, 1)
        p = f.p
        assert RI.variant_of("variant3d_sponge_3l") == 1 and p.nlay == 3
        east = (g.mk_n > 0.5) & (g.subc[0] > p.lm // 2) & (g.nudg[0] != 0.0)
        assert east.sum() >= 12 * p.mm // 2
        h3, thr = g.hlay[2][east], 20.0 * float(p.hsal)
        below, above = float(np.mean(h3 < thr)), float(np.mean(h3 > thr))
        print("variant3d_sponge_3l %s: layer 3 below / above 20 hsal in the eastern sponge %.2f / %.2f" % (frame, below, above))
        assert below >= 0.25 and above >= 0.25, (frame, below, above)
        assert np.any((g.mk_n > 0.5) & (g.subc[0] < p.lm // 2) & (g.nudg[0] != 0.0))      # and the western half is nudged too
        a, b = _oracle_after(g, "B", 1)["hlay"].copy(), _oracle_after(g, "B", 0)["hlay"]
        share = float(np.mean(a[:, g.mk_n > 0.5] != b[:, g.mk_n > 0.5]))
        print("variant3d_sponge_3l %s: variant 1 differs from variant 0 in %.3f of the cell-layers" % (frame, share))
        assert share > 0.0, frame


@pytest.mark.parametrize("config,frame", [(c, fr) for c in LIDS for fr in ("130x18", "321x50", "130x99")])
def test_rough_lid_solves_stop_at_the_cap(config, frame):
    """On the rough state no solve of plans A and B converges: every one stops at surf_pressure's 1000 sweeps, from the
    rough starting pressure and from a zero one."""
    g = RI.rough_fields(RI.base_fields(config, frame), 1)
    for start in ("rough", "zero"):
        if start == "zero":
            g.pi_s = np.zeros_like(g.pi_s)
        for first, n in PLANS.values():
            counts = _sweeps_per_step(g, first, n)
            assert counts == [1000] * n, (config, frame, start, first, counts)


def test_lid_from_rest_reaches_the_other_batch_paths():
    """What the two from-rest runs of the GPU suite are for, held on the oracle's own counts: a solve of 1000 sweeps
    directly followed by one of at most 16 (a first batch sized from a solve at the cap, the chosen sweep at its start),
    and a solve of 257...999 sweeps (the ring of 257 copies wraps, the chosen sweep lies in a later batch)."""
    strong = _sweeps_per_step(RI.lid_from_rest(RI.LID_REST_WINDS["strong"]), 1, 8)
    print("lid from rest, strong wind: sweeps per step", strong)
    assert any(a == 1000 and b <= 16 for a, b in zip(strong, strong[1:])), strong
    mild = _sweeps_per_step(RI.lid_from_rest(RI.LID_REST_WINDS["mild"]), 1, 8)
    print("lid from rest, mild wind: sweeps per step", mild)
    assert any(257 <= c <= 999 for c in mild) and all(c < 1000 for c in mild), mild


def test_reseeding_changes_one_input_alone():
    f = RI.base_fields("closed_dt3d_forced_3l", "130x18")
    a, b = RI.rough_fields(f, 1), RI.rough_fields(f, 1, reseed=("dmdx:1",))
    for k in RI.present(f):
        if k != "dmdx":
            assert same_bits(getattr(a, k), getattr(b, k)), k
    assert same_bits(a.dmdx[:, :, 0], b.dmdx[:, :, 0]) and same_bits(a.dmdx[:, :, 2], b.dmdx[:, :, 2])
    assert not same(a.dmdx[:, :, 1], b.dmdx[:, :, 1])
    assert same_bits(a.bodf, b.bodf)


@pytest.mark.parametrize("frame", ["130x18", "4200x9"])
def test_tracer_of_concentration_one_is_the_thickness_with_dry_cells(frame):
    """Empty cells away from coasts, with transports beside them: tracers_ref.update on a tracer of concentration 1 and
    relaxation concentration 1 equals the oracle's update_h, three sweeps in a row (the no-gradient rule at an empty upwind
    cell takes the other side's concentration: 1)."""
    config = "closed_leith_3l" if frame == "130x18" else "zero_visc_2l"
    f = RI.base_fields(config, frame)
    g = RI.dry_cell_state(f, 3)
    wet = g.mk_n > 0.5
    share = g.dry[:, wet].mean()
    assert 0.08 <= share <= 0.12 and np.all(g.hlay[g.dry] == 0.0) and not np.signbit(g.hlay[g.dry]).any(), share
    W, S = g.neig[:, 4], g.neig[:, 6]
    interior = g.dry & (g.mk_u > 0.5)[None] & (g.mk_v > 0.5)[None] & (g.mk_u[g.neig[:, 0]] > 0.5)[None] & (g.mk_v[g.neig[:, 2]] > 0.5)[None]
    assert interior.sum() > 0.05 * wet.sum() * f.p.nlay                 # away from coasts
    assert np.all(g.h_u[interior] != 0.0) and np.all(g.h_v[interior] != 0.0)
    assert not (g.dry & g.dry[:, W]).any() and not (g.dry & g.dry[:, S]).any()
    o = oracle_lib.Oracle(g)
    q = np.array(g.hlay, copy=True)[None]
    rq = np.array(g.rs_h, copy=True)[None]
    ctrg = np.ones_like(q)
    for tstp in (7, 8, 9):
        gene, ramp, ctim = T.step_scalars(f.p, tstp)
        h = o.a["hlay"].copy()
        q, rq = T.update(g, h, g.h_u, g.h_v, q, rq, ctrg, gene, ramp, ctim)
        o.update_h(gene, ramp, ctim)
        assert np.isfinite(q).all()
        assert same(q[0], o.a["hlay"]), (frame, tstp, float(np.max(np.abs(q[0] - o.a["hlay"]))))
        assert same(rq[0], o.a["rs_h"]), (frame, tstp)
    assert not same(o.a["hlay"], g.hlay)
