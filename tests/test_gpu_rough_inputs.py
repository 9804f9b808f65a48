"""Every sweep on rough inputs (rough_inputs.py: no field constant, smooth or zero; test_rough_inputs_cpu holds the inputs
to "rough", "straddling" and "bounded") against oracle_lib.Oracle built from the same rough Fields: helpers.same_bits over
the keys the handle's form keeps (test_gpu_parity._live / _fuses), the one tidal configuration to the project's COS_TOL.

Plan A: create from the rough fields, step(1, 5) — steps 1-3 rebuild the transports from rough u and hlay, then steps 4-5.
Plan B: step(7, ...) in calls of 2, 1 and 3 with a download after each — three steps on the uploaded history, viscosity and
stress arrays, then (on eligible handles) the history-from-Montgomery form.  The oracle's results are computed once per
configuration and frame and shared by both tile geometries.

The two rigid-lid configurations have a test of their own (test_rigid_lid_on_rough_states): the same plans, with the lid
pressure and the handle's counts of Gauss-Seidel sweeps and solves held to the oracle's after every call."""
import copy
import os

import numpy as np
import pytest

import integrals_ref as R
import oracle_lib
import rough_inputs as RI
import tracers_ref as T
from beom_amd import capi
from helpers import SCRATCH, STATE, maxrel, same, same_bits, tile_geometry
from test_gpu_parity import COS_TOL, MODES, PROGNOSTIC, _fuses, _live

pytestmark = pytest.mark.gpu
CALLS_B = (2, 1, 3)

LIDS = ("lid_wind_drag_2l", "lid_coast_3l")      # (their own test further down: the pressure and the counts of sweeps)
# name: (configuration, arguments of rough_fields, dense_hint, stress folded from step 4 on?)
VARIANTS = {c: (c, {}, 1, False) for c in RI.CONFIGS if c not in LIDS}
VARIANTS.update({
    # the fold needs every uploaded stress array to have its forcing: no top drag here, so tu3d stays +0
    "stommel_wind_drag": ("stommel_wind_drag", {"zero": ("tu3d",)}, 1, True),
    "stommel_wind_drag_unfolded": ("stommel_wind_drag_unfolded", {"zero": ("tu3d",)}, 1, False),
    "island_ragged_3l_table": ("island_ragged_3l", {}, 0, False),
    "zero_visc_2l_pos0": ("zero_visc_2l", {"visc": "zero"}, 1, False),
    "zero_visc_2l_neg0": ("zero_visc_2l", {"visc": "neg0"}, 1, False),
})
_ROUGH, _ORACLE = {}, {}


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _rough(variant, frame):
    key = (variant, frame)
    if key not in _ROUGH:
        config, kw = VARIANTS[variant][:2] if variant in VARIANTS else (variant, {})      # (a lid: the configuration itself)
        _ROUGH[key] = RI.rough_fields(RI.base_fields(config, frame), 1, **kw)
    return _ROUGH[key]


def _snap(o):
    return {k: np.array(v, copy=True) for k, v in o.state().items()}


def _oracle(variant, frame):
    """{"A": state after steps 1-5, "B": [(state, scratch of the last layer) after each call of plan B]}, computed once."""
    key = (variant, frame)
    if key not in _ORACLE:
        g = _rough(variant, frame)
        ev = RI.variant_of(VARIANTS[variant][0])
        o = oracle_lib.Oracle(g, variant=ev)
        o.step(1, 5)
        res = {"A": _snap(o), "B": []}
        o = oracle_lib.Oracle(g, variant=ev)
        t = 7
        for n in CALLS_B:
            o.step(t, n)
            t += n
            res["B"].append((_snap(o), {k: o.a[k].copy() for k in SCRATCH}))
        RI.bounded(g, res["A"]); RI.bounded(g, res["B"][-1][0])
        _ORACLE[key] = res
    return _ORACLE[key]


def _engine(g, variant, rows=None, **kw):
    config, _, dense_hint, _ = VARIANTS[variant]
    opts = dict(RI.CONFIGS, **RI.GATE_CONFIGS)[config][1]
    kw = dict(kw, variant=RI.variant_of(config))
    if rows is None:
        e = capi.Engine(g, dense_hint=dense_hint, **kw)
    else:
        with tile_geometry(rows):
            e = capi.Engine(g, dense_hint=dense_hint, **kw)
        assert e.info("tile_rows") == (rows if e.is_dense else 0)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def _keys(e, p):
    return _live(e, PROGNOSTIC if _fuses(p) else STATE)


def _exact(g):
    return not (g.has.get("tide", False) and np.any(g.tide != 0.0))


def _assert_state(st, ref, keys, exact, what):
    for k in keys:
        if exact:
            assert same_bits(st[k], ref[k]), what + (k, float(np.nanmax(np.abs(st[k] - ref[k]))))
        else:
            assert maxrel(st[k], ref[k]) <= COS_TOL, what + (k, maxrel(st[k], ref[k]))


def _eligible(e, p):
    """The handle can run the history-from-Montgomery form: a whole dense frame, fusable, with the multistep term."""
    return bool(e.is_dense) and p.nlay <= 8 and not float(p.svis) > 0.0 and float(p.g_fb) != 0.0 and float(p.rgld) < 0.5


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("frame", ["130x18", "321x50"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_plans_a_and_b_against_the_oracle(variant, frame, rows):
    config, _, dense_hint, folded = VARIANTS[variant]
    g = _rough(variant, frame)
    p = g.p
    ref = _oracle(variant, frame)
    exact = _exact(g)
    what = (variant, frame, rows)
    # plan A
    e = _engine(g, variant, rows)
    assert bool(e.is_dense) == bool(dense_hint) and bool(e.is_embedded) == (bool(dense_hint) and RI.CONFIGS[config][2])
    e.step(1, 5)
    assert e.info("stress_folded") == int(folded), what
    _assert_state(e.download(), ref["A"], _keys(e, p), exact, what + ("plan A",))
    e.close()
    # plan B
    e = _engine(g, variant, rows)
    t, seen = 7, []
    for n, (want, scr) in zip(CALLS_B, ref["B"]):
        e.step(t, n)
        t += n
        seen.append(e.info("mont_history"))
        assert e.info("stress_folded") == int(folded), what + (t,)
        st = e.download()
        _assert_state(st, want, _keys(e, p), exact, what + ("plan B", t - 1))
        if _eligible(e, p) and not folded and exact:
            assert same_bits(e.download_scratch()["mont"][p.nlay - 1], scr["mont"]), what + ("mont", t - 1)
    assert seen == ([0, 0, 1] if _eligible(e, p) and not folded else [0, 0, 0]), what + (seen,)
    assert np.isfinite(st["hlay"]).all()
    e.close()


@pytest.mark.parametrize("mode", [m for m in MODES if m != "dense_fused"])
@pytest.mark.parametrize("config", ["closed_leith_3l", "sill_ocrp_sponge_3l", "zero_visc_2l", "closed_dt3d_forced_3l",
                                    "sill_ocrp_stress_3l", "variant3d_sponge_3l"])
def test_other_engine_modes_on_plan_b(config, mode):
    """The table path, the separate sweeps, one fused sweep without the other, and the fused pair that keeps its diagnostics:
    the forms the production default does not launch read the same rough arrays through other kernels."""
    g = _rough(config, "130x18")
    p = g.p
    dh, fmv, fuv, keep = MODES[mode]
    e = capi.Engine(g, dense_hint=dh, variant=RI.variant_of(config))
    for k, v in (("fuse_mont_visc", fmv), ("fuse_uv", fuv), ("keep_diag", keep)):
        e.set_option(k, v)
    t = 7
    for n, (want, scr) in zip(CALLS_B, _oracle(config, "130x18")["B"]):
        e.step(t, n)
        t += n
        st = e.download()
        lossy = mode == "dense_fuse_mv_only" and _fuses(p)
        _assert_state(st, want, _live(e, PROGNOSTIC), True, (config, mode, t - 1))
        sc = e.download_scratch()
        if not lossy:
            for k in ("v_cc", "v_ll"):
                assert same(st[k], want[k]), (config, mode, t - 1, k)
        for k in (SCRATCH if not lossy else ("mont", "pvor", "d2hx", "d2hy")):
            assert same(sc[k][p.nlay - 1], scr[k]), (config, mode, t - 1, k, maxrel(sc[k][p.nlay - 1], scr[k]))
    e.close()


# ---- the rigid lid ------------------------------------------------------------------------------------------------------------
_LID_ORACLE = {}


def _lid_counts(x):
    """(sweeps, solves) so far: of a handle, or of the oracle library."""
    if isinstance(x, oracle_lib.Oracle):
        c = x.lid_sweeps()
        return c["sweeps"], c["solves"]
    return x.info("lid_sweeps"), x.info("lid_solves")


def _lid_oracle_call(o, t, n):
    """Steps t..t+n-1 on the oracle: (state, pressure, sweeps, solves of this call)."""
    s0, n0 = _lid_counts(o)
    o.step(t, n)
    s1, n1 = _lid_counts(o)
    return _snap(o), o.rgld["pi_s"].copy(), s1 - s0, n1 - n0


def _lid_oracle(config, frame):
    """{"A": [result of step(1, 5)], "B": [results of the calls of plan B]} on the rough state, computed once."""
    key = (config, frame)
    if key not in _LID_ORACLE:
        g = _rough(config, frame)
        res = {"A": [_lid_oracle_call(oracle_lib.Oracle(g), 1, 5)], "B": []}
        o = oracle_lib.Oracle(g)
        t = 7
        for n in CALLS_B:
            res["B"].append(_lid_oracle_call(o, t, n))
            t += n
        RI.bounded(g, res["A"][-1][0]); RI.bounded(g, res["B"][-1][0])
        _LID_ORACLE[key] = res
    return _LID_ORACLE[key]


def _lid_engine_call(e, t, n, want, what):
    """Steps t..t+n-1 on the handle against the oracle's result of the same call: the fields that carry on and the pressure
    bit for bit, the other arrays as numbers, and the sweeps and solves the handle counts."""
    state, pi_s, sweeps, solves = want
    s0, n0 = _lid_counts(e)
    e.step(t, n)
    s1, n1 = _lid_counts(e)
    assert e.info("stress_folded") == 0, what
    st = e.download()
    for k in ("hlay", "u", "v", "h_u", "h_v"):
        assert same_bits(st[k], state[k]), what + (k, float(np.nanmax(np.abs(st[k] - state[k]))))
    got = e.download_pressure()
    assert same_bits(got, pi_s), what + ("pi_s", float(np.nanmax(np.abs(got - pi_s))))
    for k in PROGNOSTIC:
        assert same(st[k], state[k]), what + (k, maxrel(st[k], state[k]))
    assert (s1 - s0, n1 - n0) == (sweeps, solves) and solves == n, what + ("sweeps, solves", (s1 - s0, n1 - n0), (sweeps, solves))


@pytest.mark.parametrize("frame", ["130x18", "321x50"])
@pytest.mark.parametrize("config,dense_hint", [("lid_wind_drag_2l", 1), ("lid_coast_3l", 1), ("lid_coast_3l", 0)])
def test_rigid_lid_on_rough_states(config, dense_hint, frame):
    """rgld = 1 from a rough state and a rough starting pressure that is no solve's result: every solve runs into
    surf_pressure's 1000 sweeps (test_rough_inputs_cpu holds the oracle to that), the last batch of the pipeline is a short
    one and the ring of pressure copies wraps three times per solve.  Plan A creates the handle with the rough pressure,
    plan B uploads it afterwards, and scatters state and pressure once more between its second and third call."""
    g = _rough(config, frame)
    ref = _lid_oracle(config, frame)
    what = (config, dense_hint, frame)
    e = capi.Engine(g, dense_hint=dense_hint)
    assert bool(e.is_dense) == bool(dense_hint) and bool(e.is_embedded) == (bool(dense_hint) and RI.CONFIGS[config][2])
    _lid_engine_call(e, 1, 5, ref["A"][0], what + ("plan A",))
    assert ref["A"][0][2] == 5 * 1000, what
    e.close()
    own = copy.copy(g)
    own.pi_s = RI.base_fields(config, frame).pi_s              # the case's own starting pressure at creation
    assert not same(own.pi_s, g.pi_s)
    e = capi.Engine(own, dense_hint=dense_hint)
    e.upload_pressure(g.pi_s)
    assert same_bits(e.download_pressure(), g.pi_s), what
    t = 7
    for i, (n, want) in enumerate(zip(CALLS_B, ref["B"])):
        if i == 2:
            e.upload(**e.download()); e.upload_pressure(e.download_pressure())
        _lid_engine_call(e, t, n, want, what + ("plan B", t + n - 1))
        assert want[2] == n * 1000, what
        t += n
    e.close()


@pytest.mark.parametrize("wind", list(RI.LID_REST_WINDS))
def test_rigid_lid_from_rest_sweep_counts_per_step(wind):
    """The lid started from rest, one step per call, the handle's count of sweeps against the oracle's on every step.
    strong: solves at the cap followed by one that converges within the first batch, which the solve before sized at its
    largest.  mild: solves that converge in a later batch, after the ring of 257 copies has wrapped."""
    g = RI.lid_from_rest(RI.LID_REST_WINDS[wind])
    e, o = capi.Engine(g), oracle_lib.Oracle(g)
    assert e.is_dense and not e.is_embedded
    counts = []
    for t in range(1, 9):
        want = _lid_oracle_call(o, t, 1)
        _lid_engine_call(e, t, 1, want, ("from rest", wind, t))
        counts.append(want[2])
    print("lid from rest, %s wind: sweeps per step %s" % (wind, counts))
    if wind == "strong":
        assert any(a == 1000 and b <= 16 for a, b in zip(counts, counts[1:])), counts
    else:
        assert any(257 <= c <= 999 for c in counts) and all(c < 1000 for c in counts), counts
    e.close()


# ---- the gates of the folded stress -------------------------------------------------------------------------------------------
GATES = {   # configuration: the stress arrays whose forcing it lacks
    "stommel_wind_drag": ("tu3d",),
    "closed_wind_only_2l": ("tb3d", "tu3d"),
    "closed_drag_only_2l": ("tt3d", "tu3d"),
}


def _gate_run(g, folded, what):
    e, o = capi.Engine(g), oracle_lib.Oracle(g)
    e.step(7, 6); o.step(7, 6)
    assert e.info("stress_folded") == folded, what
    _assert_state(e.download(), o.state(), _live(e, PROGNOSTIC), True, what)
    RI.bounded(g, o.state())
    e.close()


@pytest.mark.parametrize("config", list(GATES))
def test_uploaded_stress_without_its_forcing_keeps_the_fold_off(config):
    lacking = GATES[config]
    f = RI.base_fields(config, "130x18")
    _gate_run(RI.rough_fields(f, 1, zero=lacking), 1, (config, "control: the arrays without forcing are +0, the stress folds"))
    for arr in lacking:
        g = RI.rough_fields(f, 1, zero=tuple(k for k in lacking if k != arr))
        assert np.any(getattr(g, arr) != 0.0)
        _gate_run(g, 0, (config, arr, "uploaded without its forcing"))


def test_body_force_of_minus_zero_keeps_the_fold_off():
    f = RI.base_fields("stommel_wind_drag", "130x18")
    g = RI.rough_fields(f, 1, zero=("tu3d",))
    _gate_run(g, 1, ("bodf", "control: no -0"))
    g = copy.copy(g)
    g.bodf = np.array(g.bodf, copy=True)
    g.bodf[1, 0] = -0.0
    _gate_run(g, 0, ("bodf", "one entry of -0"))


# ---- bands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,nband", [("closed_leith_3l", 2), ("closed_leith_3l", 3), ("jet_xyper_2l", 2),
                                          ("island_ragged_3l", 2), ("sill_ocrp_stress_3l", 2)])
def test_bands_against_the_oracle(config, nband):
    g = _rough(config, "130x99")
    p = g.p
    ref = _oracle(config, "130x99")
    many = capi.MultiEngine(g, devices=[0] * nband)
    assert many.count == nband and many.describe()["ring"] == int(float(p.yper) > 0.5)
    many.step(1, 5)
    _assert_state(many.download(), ref["A"], PROGNOSTIC, True, (config, nband, "plan A"))
    s = many.stats()
    assert s["split"] + s["plain"] == 5 * nband and s["split"] >= 2 * nband, s
    many.close()
    many = capi.MultiEngine(g, devices=[0] * nband)
    t = 7
    for n, (want, _) in zip(CALLS_B, ref["B"]):
        many.step(t, n)
        t += n
        _assert_state(many.download(), want, PROGNOSTIC, True, (config, nband, "plan B", t - 1))
    s = many.stats()
    assert s["split"] + s["plain"] == 6 * nband and s["split"] >= 3 * nband, s
    assert many.info("mont_history") == 0
    many.close()


# ---- tracers --------------------------------------------------------------------------------------------------------------
def _finite_same(a, b):
    return bool(np.isfinite(a).all()) and same(a, b)


@pytest.mark.parametrize("kind,frame", [("dense", "130x18"), ("embedded", "130x18"), ("table", "130x18"),
                                        ("dense", "4200x9"), ("embedded", "4200x9"), ("table", "4200x9"),
                                        ("dense", "321x50"), ("embedded", "321x50"), ("table", "321x50")])
def test_tracer_sweep_on_its_own_with_dry_cells(kind, frame):
    """beom_update_tracers in front of beom_update_h, no dynamics: 8 tracers on a state with empty cells away from coasts
    and transports beside them, three sweeps against tracers_ref.update fed with the handle's own thicknesses.  321 x 50 is
    the frame with interior waves; scheme 2 on these states: test_gpu_tracers_limited_rough."""
    config = "island_ragged_3l" if kind == "embedded" else ("zero_visc_2l" if frame == "4200x9" else "closed_leith_3l")
    f = RI.base_fields(config, frame)
    g = RI.dry_cell_state(f, 3)
    e = capi.Engine(g, dense_hint=0 if kind == "table" else 1)
    assert bool(e.is_dense) == (kind != "table") and bool(e.is_embedded) == (kind == "embedded")
    q, rq, ctrg = RI.rough_tracers(g, g.hlay, 8, 5)
    e.set_tracers(8)
    e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    for tstp in (7, 8, 9):
        gene, ramp, ctim = T.step_scalars(f.p, tstp)
        st = e.download(("hlay", "h_u", "h_v"))
        assert same_bits(st["h_u"], g.h_u) and same_bits(st["h_v"], g.h_v)
        q, rq = T.update(g, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, gene, ramp, ctim)
        e.update_tracers(gene, ramp, ctim)
        e.update_h(gene, ramp, ctim)
        e.sync()
        got = e.download_tracers()
        assert _finite_same(got["q"], q), (kind, frame, tstp, "q", maxrel(got["q"], q))
        assert _finite_same(got["rq"], rq), (kind, frame, tstp, "rq", maxrel(got["rq"], rq))
        h = e.download(("hlay",))["hlay"]
        assert _finite_same(got["q"][0][:, 1:], h[:, 1:]), (kind, frame, tstp, "q of the uniform tracer vs hlay")
    assert not same(got["q"][1], RI.rough_tracers(g, g.hlay, 8, 5)[0][1])
    e.close()


@pytest.mark.parametrize("config,ntrc", [("sill_ocrp_sponge_3l", 1), ("jet_xyper_2l", 3), ("closed_12l_hdot", 8)])
def test_plan_b_with_tracers_against_the_restatement(config, ntrc):
    g = _rough(config, "130x18")
    e = _engine(g, config)
    q, rq, ctrg = RI.rough_tracers(g, g.hlay, ntrc, 7)
    e.set_tracers(ntrc)
    assert e.info("tracers") == ntrc
    e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    for tstp in range(7, 13):
        st = e.download(("hlay", "h_u", "h_v"))
        gene, ramp, ctim = T.step_scalars(g.p, tstp)
        q, rq = T.update(g, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, gene, ramp, ctim)
        e.step(tstp, 1)
        got = e.download_tracers()
        assert _finite_same(got["q"], q), (config, tstp, "q", maxrel(got["q"], q))
        assert _finite_same(got["rq"], rq), (config, tstp, "rq", maxrel(got["rq"], rq))
    _assert_state(e.download(), _oracle(config, "130x18")["B"][-1][0], _keys(e, g.p), True, (config, "the state under the tracers"))
    e.close()


def test_two_bands_with_eight_tracers_against_the_single_handle():
    g = _rough("closed_leith_3l", "130x99")
    q, rq, ctrg = RI.rough_tracers(g, g.hlay, 8, 9)
    got = []
    for x in (capi.Engine(g), capi.MultiEngine(g, devices=[0, 0])):
        x.set_tracers(8)
        x.upload_tracers(q=q, rq=rq, ctrg=ctrg)
        t = 7
        for n in CALLS_B:
            x.step(t, n)
            t += n
        got.append(x.download_tracers())
        x.close()
    assert np.isfinite(got[0]["q"]).all() and not same(got[0]["q"], q)
    assert same_bits(got[0]["q"], got[1]["q"]) and same_bits(got[0]["rq"], got[1]["rq"])


# ---- integrals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "table", "embedded", "two_bands"])
def test_integrals_of_a_rough_state(kind):
    config = "island_ragged_3l" if kind == "embedded" else "closed_leith_3l"
    g = _rough(config, "130x99")
    want = R.integrals(g, {k: getattr(g, k) for k in ("hlay", "u", "v")})
    assert np.isfinite(want).all()
    if kind == "two_bands":
        x = capi.MultiEngine(g, devices=[0, 0])
    else:
        x = capi.Engine(g, dense_hint=0 if kind == "table" else 1)
        assert bool(x.is_dense) == (kind != "table") and bool(x.is_embedded) == (kind == "embedded")
    got = x.integrals()["raw"]
    assert same_bits(got, want), (kind, got, want)
    x.close()
