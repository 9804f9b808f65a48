"""Forcing in time on the GPU (beom_set_forcing, include/beom_hip.h): the launch alone against tests/forcing_ref.py, and
K-step calls against the oracle stepped one step at a time with the array replaced on the host before each step, bit for
bit.  tests/test_forcing_cpu.py holds the inputs used here to their conditions on the oracle."""
from __future__ import annotations

import copy as _copy

import numpy as np
import pytest

import forcing_cases as FC
import forcing_ref as FR
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import Golden, same_bits, tile_geometry
from test_gpu_parity import _fields

pytestmark = pytest.mark.gpu
NSTEPS = FC.NSTEPS


def _golden(name):
    g = Golden(name)
    return g, _fields(g)


def _rc(fn):
    try:
        fn()
    except capi.BeomError as e:
        return str(e)
    return ""


def _sets(f, fields, period_steps=None, special=False):
    out = {}
    for k, field in enumerate(fields):
        fr = FC.make_frames(f, field, seed=5 + k)
        if special:
            fr = FC.with_special_entries(fr)
        times = FC.frame_times(f)
        out[field] = (times, fr, 0.0 if period_steps is None else period_steps * float(f.p.dtd8))
    return out


def _give(e, sets):
    for field, (times, frames, period) in sets.items():
        e.set_forcing(field, times, frames, period)


def _stepped(e, calls):
    t = 1
    for n in calls:
        e.step(t, n)
        t += n
    return e.download()


def _same_state(got, want, what, keys=FC.PROGNOSTIC):
    for k in keys:
        assert same_bits(got[k], want[k]), (what, k, int(np.sum(np.asarray(got[k]) != np.asarray(want[k]))))


# ---- 1. the launch alone ----------------------------------------------------------------------------------------------------------
LAUNCH_HANDLES = [("stommel_24x16", 4, 1), ("stommel_24x16", 8, 1), ("island_3l_forced", None, 1), ("random_coast_2l_xper", None, 0),
                  ("island_10l_deep", None, 1), ("rigid_lid_closed_3l_wind", None, 1)]


@pytest.mark.parametrize("name,rows,dense_hint", LAUNCH_HANDLES)
def test_the_launch_alone_equals_the_reference(name, rows, dense_hint):
    """Dense 64 x 4 and 64 x 8, embedded, the table path (n1 = ndeg + 1: the alignment changes from slice to slice), ten
    layers of hdot, and a sentinel that holds a wind of its own (rigid_lid_closed_3l_wind).  Frames with exact +0, -0 and
    entries equal between consecutive frames; every launch is counted, a repeated weight launches nothing."""
    g, f = _golden(name)
    if rows:
        with tile_geometry(rows):
            e = capi.Engine(f, variant=g.variant, dense_hint=dense_hint)
        assert e.info("tile_rows") == rows
    else:
        e = capi.Engine(f, variant=g.variant, dense_hint=dense_hint)
    if name == "random_coast_2l_xper":
        assert not e.is_dense
    if name == "island_3l_forced":
        assert e.is_embedded
    assert e.info("forcing_launches") == 0
    created = e.download_forcing()
    assert same_bits(created["taus"], f.taus) and same_bits(created["hdot"], f.hdot if f.has.get("hdot", True) else np.zeros_like(f.hdot))
    launches = 0
    for field in ("taus", "hdot"):
        other = "hdot" if field == "taus" else "taus"
        for period_steps in (None, 8.0):
            times, frames, period = _sets(f, (field,), period_steps, special=True)[field]
            e.set_forcing(field, times, frames, period)
            launches += 1
            assert e.info("forcing_%s_frames" % field) == 3 and e.info("forcing_launches") == launches
            assert same_bits(e.download_forcing()[field], frames[0]), (name, field, "the first frame is not in the buffer")
            last = (0, 0, 0.0)
            table = FC.time_table(f, times, period)
            for ctim in table + table[-1:]:                  # (the last time twice: the same weight again)
                e.apply_forcing(ctim)
                w = FR.weight(times, period, ctim)
                if w != last:
                    launches += 1
                last = w
                got = e.download_forcing()
                assert same_bits(got[field], FR.field(frames, times, period, ctim)), (name, field, period, ctim, w)
                assert same_bits(got[other], created[other]), (name, field, "the other field moved")
                assert e.info("forcing_launches") == launches, (name, field, ctim, w)
        e.set_forcing(field, None)
        assert e.info("forcing_%s_frames" % field) == 0
        assert same_bits(e.download_forcing()[field], created[field])
    e.close()


# ---- 2. steps against the oracle ----------------------------------------------------------------------------------------------------
def _against_oracle(name, fields, period_steps=None, nsteps=NSTEPS, calls=((NSTEPS,), (5, 7), (1,) * NSTEPS), expect=None, **kw):
    g, f = _golden(name)
    sets = _sets(f, fields, period_steps)
    want = FC.oracle_run(f, g.variant, sets, nsteps).state()
    for c in calls:
        assert sum(c) == nsteps
        e = capi.Engine(f, variant=g.variant, **kw)
        _give(e, sets)
        got = _stepped(e, c)
        _same_state(got, want, (name, fields, c))
        if expect:
            expect(e)
        e.close()
    return want


@pytest.mark.parametrize("name,dense_hint", [("stommel_24x16", 1), ("island_3l_forced", 1), ("random_coast_2l_xper", 0),
                                             ("island_10l_deep", 1), ("biharm_island_2l", 1)])
def test_taus_frames_step_as_the_oracle_with_the_array_replaced(name, dense_hint):
    _against_oracle(name, ("taus",), dense_hint=dense_hint)


@pytest.mark.parametrize("name", ["island_3l_forced", "topdrag_topo_2l"])
def test_hdot_frames_step_as_the_oracle_with_the_array_replaced(name):
    """(n_3d = 2: the stress is refreshed every other step.)"""
    _against_oracle(name, ("hdot",))


def test_a_handle_created_without_hdot_gains_it():
    g, f = _golden("stommel_24x16")
    assert not f.has["hdot"]
    _against_oracle("stommel_24x16", ("hdot",))


def test_a_handle_created_without_wind_gains_it():
    g, f = _golden("jet_2l_xyper")
    assert not np.any(f.taus)
    _against_oracle("jet_2l_xyper", ("taus",))


def test_both_fields_at_once():
    _against_oracle("island_3l_forced", ("taus", "hdot"))


def test_a_cyclic_set_whose_period_is_seven_steps():
    """The frames span 6.75 steps: steps 10 to 12 are the second cycle, step 9.25 + ... the wrap interval."""
    want = _against_oracle("stommel_24x16", ("taus",), period_steps=7.0)
    other = _against_oracle("stommel_24x16", ("taus",), calls=((NSTEPS,),))
    assert not same_bits(want["u"], other["u"]), "the period changed nothing"


def test_a_negative_hdot_on_dry_cells_of_a_nudged_frame_keeps_the_oracles_zeros():
    """Steps 1-3 (gene = 0) on the sill with sponges: its dry margin cells start with a thickness of -0.0 north of row 125,
    and the frames bring a negative hdot to about half of them, so rs_3 = (hdot)*mk_n is -0.0 there.  The reference adds
    (..)*dt*0 = +0.0 to rs_3*dt before the thickness: the nudged form of update_h keeps +0.0 as the oracle does."""
    import addons_kit as K
    f = K.frame("sill_sponges")
    kit = K.Kit(f, seed=2)
    sets = {"hdot": kit.hdot}
    h0, dry = np.asarray(f.hlay), np.asarray(f.mk_n)[None, :] < 0.5
    hit = dry & (h0 == 0.0) & np.signbit(h0) & (kit.hdot[1][0] < 0.0)
    hit[:, 0] = False
    assert hit.sum() >= 20 and np.any(f.nudg[0] != 0.0), "no dry cell with a -0 thickness under a negative hdot: nothing tested"
    e = capi.Engine(f)
    _give(e, sets)
    for first, k in ((1, 1), (2, 1), (3, 1), (4, NSTEPS - 3)):
        e.step(first, k)
        want = FC.oracle_run(f, 0, sets, first + k - 1).state()
        assert not np.signbit(want["hlay"][hit]).any()
        _same_state(e.download(), want, ("sill_sponges", first + k - 1), keys=("hlay", "h_u", "h_v", "rs_h"))      # what update_h writes, and the transports built on it
    e.close()


# ---- 3. the folded stress -----------------------------------------------------------------------------------------------------------
def test_the_stress_stays_folded_while_the_frames_vary():
    g, f = _golden("stommel_24x16")
    sets = _sets(f, ("taus",))
    folded, apart = capi.Engine(f, variant=g.variant), capi.Engine(f, variant=g.variant)
    apart.set_option("fold_stress", 0)
    for e in (folded, apart):
        _give(e, sets)
        e.step(1, 3)
    assert folded.info("stress_folded") == 0
    for t in range(4, NSTEPS + 1):
        for e in (folded, apart):
            e.step(t, 1)
        assert folded.info("stress_folded") == 1 and apart.info("stress_folded") == 0, t
    _same_state(folded.download(), apart.download(), "folded against fold_stress = 0")
    # the folded sweep's copy is zero at the sentinel and in every slot that is no cell, or the coast would feel a wind: the
    # oracle's run says so
    _same_state(folded.download(), FC.oracle_run(f, g.variant, sets).state(), "folded against the oracle")
    folded.close(); apart.close()


# ---- 4. equal frames and clearing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stommel_24x16", "island_3l_forced"])
def test_equal_frames_and_clearing(name):
    g, f = _golden(name)
    times = FC.frame_times(f)
    plain = capi.Engine(f, variant=g.variant)
    _, counts = plain.profile_steps(1, NSTEPS)
    want = plain.download()
    assert plain.info("forcing_launches") == 0
    # a set of equal frames, -0 entries among them, steps as a handle created with that array
    f2 = _fields(g)
    f2.taus = np.array(f.taus, dtype=np.float64)
    f2.taus[:, 3::11] = -0.0
    made = capi.Engine(f2, variant=g.variant)
    given = capi.Engine(f, variant=g.variant)
    given.set_forcing("taus", times, np.stack([f2.taus] * 3))
    if f.has["hdot"]:
        given.set_forcing("hdot", times, np.stack([f.hdot] * 3))
    a, b = _stepped(made, (NSTEPS,)), _stepped(given, (5, 7))
    _same_state(b, a, (name, "equal frames"), keys=FC.PROGNOSTIC + ("tt3d",) if not given.info("stress_folded") else FC.PROGNOSTIC)
    for what in ("stress_folded", "plain_sweeps", "uv_fused", "mont_history"):
        assert made.info(what) == given.info(what), (name, what)
    made.close(); given.close()
    # after clearing, the handle steps as the untouched one, launch for launch
    cleared = capi.Engine(f, variant=g.variant)
    _give(cleared, _sets(f, ("taus", "hdot")))
    cleared.set_forcing("taus", None); cleared.set_forcing("hdot", None)
    n0 = cleared.info("forcing_launches")
    _, counts2 = cleared.profile_steps(1, NSTEPS)
    assert counts2 == counts and cleared.info("forcing_launches") == n0
    _same_state(cleared.download(), want, (name, "cleared"), keys=FC.PROGNOSTIC + ("tt3d", "tb3d", "tu3d"))
    plain.close(); cleared.close()


def test_clearing_a_gained_wind_leaves_nothing_behind():
    """jet_2l_xyper has no stress at all: after frames have run and are cleared, it must again."""
    g, f = _golden("jet_2l_xyper")
    plain, e = capi.Engine(f, variant=g.variant), capi.Engine(f, variant=g.variant)
    _give(e, _sets(f, ("taus",)))
    e.step(1, 4)
    e.set_forcing("taus", None)
    e.upload(**{k: getattr(f, k) for k in capi.STATE_NAMES if k not in ("tt3d", "tb3d", "tu3d")})
    a, b = _stepped(e, (NSTEPS,)), _stepped(plain, (NSTEPS,))
    _same_state(a, b, "a cleared wind", keys=FC.PROGNOSTIC + ("tt3d",))
    assert e.info("plain_sweeps") == plain.info("plain_sweeps")
    plain.close(); e.close()


# ---- 5. tracers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["upstream", "limited"])
def test_the_unit_tracer_is_still_hlay_under_hdot_frames(scheme):
    g, f = _golden("island_3l_forced")
    sets = _sets(f, ("hdot",))
    e = capi.Engine(f, variant=g.variant)
    _give(e, sets)
    e.set_tracers(1)
    e.set_tracer_scheme(scheme)
    e.upload_tracers(q=np.array(f.hlay, dtype=np.float64)[None], ctrg=np.ones((1,) + f.hlay.shape))
    e.step(1, 5); e.step(6, 7)
    q, h = e.download_tracers()["q"][0], e.download(("hlay",))["hlay"]
    assert same_bits(q[:, 1:], h[:, 1:]), scheme
    assert same_bits(h, FC.oracle_run(f, g.variant, sets).state()["hlay"])
    e.close()


# ---- 6. bands ---------------------------------------------------------------------------------------------------------------------------
def _bands_against_single(f, variant, fields, what, cut=None, steady_wind=False):
    sets = _sets(f, fields)
    fs = f
    if steady_wind:                    # the steady MultiEngine the cut is compared with blows the first frame
        fs = _copy.copy(f)
        fs.taus = np.array(sets["taus"][1][0])
    e = capi.Engine(f, variant=variant)
    _give(e, sets)
    want = _stepped(e, (5, 7))
    want_forcing = e.download_forcing()
    e.close()
    for nb in (2, 3):
        for overlap in (0, 1):
            many, steady = (capi.MultiEngine(x, devices=[0] * nb, variant=variant) for x in (f, fs))
            assert many.count == nb
            for m in (many, steady):
                m.set_option("overlap", overlap)
            _give(many, sets)
            got = _stepped(many, (5, 7))
            _same_state(got, want, (what, nb, overlap))
            gf = many.download_forcing()
            for k in ("taus", "hdot"):
                assert same_bits(gf[k], want_forcing[k]), (what, nb, overlap, k)
            steady.step(1, 5); steady.step(6, 7)
            s = many.stats()
            assert s == steady.stats(), (what, nb, overlap, "frames changed how the bands' steps are cut")
            if cut:
                assert (s["split"] >= nb * (NSTEPS - 3)) if overlap else (s["split"] == 0), (what, nb, overlap, s)
            assert many.info("forcing_launches") > 0
            many.close(); steady.close()


def test_a_chain_of_bands_with_land():
    g, f = _golden("island_3l_forced")
    _bands_against_single(f, g.variant, ("taus", "hdot"), "island_3l_forced")


def test_a_ring_of_bands():
    g, f = _golden("jet_2l_xyper")
    _bands_against_single(f, g.variant, ("taus",), "jet_2l_xyper")


def test_cut_steps_of_bands_stay_cut():
    """A closed frame of 49 x 101 cells whose bands' steps are cut, as those of a steady MultiEngine with wind are."""
    p, files = I.case_headline(48, 100, 2)
    f = read_input_data(p, files=files)
    assert not np.any(f.taus)          # (the case has no wind of its own: the frames bring it, the steady handle is given one)
    _bands_against_single(f, 0, ("taus",), "closed_2l", cut=True, steady_wind=True)


# ---- 7. rigid lid -----------------------------------------------------------------------------------------------------------------------
def test_the_rigid_lid_with_taus_frames():
    """ocrp = 1: the stress fractions follow the thicknesses; the sentinel holds a wind of its own."""
    g, f = _golden("rigid_lid_closed_3l_wind")
    assert np.all(f.taus[:, 0] != 0.0)
    sets = {"taus": (FC.frame_times(f, (0.5, 2.0, 3.5)), FC.make_frames(f, "taus"), 0.0)}
    want = FC.oracle_run(f, g.variant, sets, 4)
    for calls in ((4,), (1, 1, 1, 1)):
        e = capi.Engine(f, variant=g.variant)
        _give(e, sets)
        got = _stepped(e, calls)
        _same_state(got, want.state(), ("rigid lid", calls), keys=FC.PROGNOSTIC + ("tt3d",))
        assert same_bits(e.download_pressure(), want.rgld["pi_s"])
        assert same_bits(e.download_forcing()["taus"], want.a["taus"])
        e.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    g, f = _golden("island_3l_forced")
    sets = _sets(f, ("taus", "hdot"))
    e, ref = capi.Engine(f, variant=g.variant), capi.Engine(f, variant=g.variant)
    for x in (e, ref):
        _give(x, sets)
        x.step(1, 4)
    times, frames, _ = sets["taus"]
    nan, inf = float("nan"), float("inf")
    bad_frames = [np.array(frames), np.array(frames)]
    bad_frames[0][1, 1, 7] = nan
    bad_frames[1][2, 0, 0] = -inf
    n0 = e.info("forcing_launches")
    bad = [("taus", times[::-1], frames, 0.0), ("taus", [times[0], times[0], times[2]], frames, 0.0), ("hdot", [times[0], nan, times[2]], sets["hdot"][1], 0.0),
           ("taus", times, frames, float(times[2] - times[0])), ("taus", times, frames, -1.0), ("hdot", times, sets["hdot"][1], inf),
           ("taus", times, bad_frames[0], 0.0), ("taus", times, bad_frames[1], 0.0)]
    for field, t, fr, period in bad:
        msg = _rc(lambda: e.set_forcing(field, t, fr, period))
        assert "error -3: beom_set_forcing:" in msg and len(msg.split("beom_set_forcing:")[1].strip()) > 15, (field, period, msg)
    err = capi.C.create_string_buffer(capi.ERRLEN + 1)
    assert e.lib.beom_set_forcing(e.h, 3, 3, capi._dp(np.array(times)), 0.0, capi._dp(frames), err, capi.ERRLEN) == -3 and b"field" in err.value
    assert "field" in _rc(lambda: e.set_forcing("fnud", times, frames))
    assert (e.info("forcing_taus_frames"), e.info("forcing_hdot_frames"), e.info("forcing_launches")) == (3, 3, n0)
    # ... and the handle steps as before
    e.step(5, 8); ref.step(5, 8)
    _same_state(e.download(), ref.download(), "after refused sets")
    e.close(); ref.close()
    # the same through a frame's bands: checked on the global arrays, before any band is touched
    many = capi.MultiEngine(f, devices=[0, 0], variant=g.variant)
    msg = _rc(lambda: many.set_forcing("taus", times, bad_frames[0]))
    assert "error -3: beom_multi_set_forcing:" in msg, msg
    assert many.info("forcing_taus_frames") == 0
    many.close()
    # a handle that holds one band's window
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    fr = np.zeros((2, 2, fw.p.ndeg + 1))
    msg = _rc(lambda: band.set_forcing("taus", [1.0, 2.0], fr))
    assert "error -6:" in msg and len(msg.split("error -6:")[1].strip()) > 20, msg
    msg = _rc(band.download_forcing)
    assert "error -6:" in msg, msg
    band.close()
