"""Every add-on that rides on the time step on ONE handle (addons_kit: forcing in time, tracers of either scheme with lateral
and vertical mixing, moments, tracer moments, harmonics, the five recorders, floats with their track), against the handles
that keep each add-on alone, against the numpy restatements on the downloaded state, on 2 and 3 bands against the single
handle, through a lifecycle in mid-run and in every class of set-up order.  Every comparison is helpers.same_bits (through
addons_kit.differences): no tolerance anywhere.  Every case runs 12 steps, so the rebuild of steps 1-3 and both u/v orders are
inside.  test_addons_kit_cpu holds the kit's inputs to their conditions without a GPU."""
import numpy as np
import pytest

import addons_kit as K
import column_series_ref as CS
import forcing_ref as FO
import maps_ref as MR
import series_ref as S
import tracer_column_series_ref as TCS
import tracer_series_ref as TS
from beom_amd import capi
from helpers import STATE, same_bits

pytestmark = pytest.mark.gpu
NSTEPS = K.NSTEPS
PROGNOSTIC = ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy")      # everything that determines the future of a run
TRACER_PARTS = ("tracer_moments", "tracer_series", "tracer_column_series", "maps")


def _h0r4(f):
    return np.ascontiguousarray(np.asarray(f.h_0)[:, 1:].astype(np.float32))


def _run(e, kit, parts, calls, first=1, between=None):
    """Steps the handle and collects every download of the parts, the launch counters and the infos of the last step."""
    K.step_calls(e, calls, first, between)
    out = kit.collect(e, parts)
    out["launches"] = kit.launches(e, parts)
    out["infos"] = {k: e.info(k) for k in K.STEP_INFOS}
    return out


def _same(a, b, keys, what):
    for k in keys:
        d = K.differences(a[k], b[k], k)
        assert d == [], (what, d)


def _no_stress(st):
    """The state without tt3d, tb3d, tu3d.  Under a folded stress they are not kept current, and an uploaded stress array is
    the caller's: it stays in force once the wind that would rewrite it is gone (set_forcing("taus", None) zeroes only a
    tt3d the handle wrote itself).  A caller who puts a state back and then clears the wind leaves them out."""
    return {k: v for k, v in st.items() if k not in ("tt3d", "tb3d", "tu3d")}


def _from_step(rec, first, last=NSTEPS):
    """The records of a recorder's download taken at steps first..last."""
    keep = (np.asarray(rec["tstp"]) >= first) & (np.asarray(rec["tstp"]) <= last)
    return {k: (np.asarray(v)[keep] if (isinstance(v, np.ndarray) and v.shape[:1] == keep.shape) else v)
            for k, v in rec.items() if k != "count"}


# ---- a. one handle, each kind -------------------------------------------------------------------------------------------------
KINDS = {"embedded": ("island_ragged_3l", 1), "table": ("island_ragged_3l", 0), "twelve_layers": ("closed_12l", 1)}
_SINGLE = {}


def _single_runs(kind, scheme):
    """Once per (kind, scheme): `all` (the full kit in calls of 5 and 7 steps, with integrals(), the output and diag records
    and a download between them), `base`, `bare` (no part at all) and one handle `base + X` per diagnostic X in one call."""
    key = (kind, scheme)
    if key not in _SINGLE:
        name, dense_hint = KINDS[kind]
        f = K.frame(name)
        kit = K.Kit(f, seed=1, scheme=scheme)
        h0r4 = _h0r4(f)
        seen = {}

        def between(e, k):
            seen["integrals"] = e.integrals()["raw"]
            seen["outputs"] = e.download_outputs(h0r4)
            seen["diag"] = e.download_diag()
            seen["state"] = e.download()

        def handle(parts, calls, between=None):
            e = capi.Engine(f, dense_hint=dense_hint)
            assert bool(e.is_dense) == bool(dense_hint) and e.is_embedded == (kind == "embedded"), kind
            kit.apply(e, parts)
            out = _run(e, kit, parts, calls, between=between)
            e.close()
            return out

        runs = {"all": handle(kit.keeps("single"), (5, 7), between), "base": handle(K.BASE, (NSTEPS,)), "bare": handle((), (NSTEPS,))}
        for x in K.DIAGNOSTICS:
            runs[x] = handle(K.BASE + (x,) + (("float_track",) if x == "floats" else ()), (NSTEPS,))
        assert np.isfinite(seen["integrals"]).all() and np.isfinite(seen["state"]["hlay"]).all()
        _SINGLE[key] = (f, kit, runs)
    return _SINGLE[key]


@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("kind", list(KINDS))
def test_everything_on_one_handle_gives_the_bits_of_each_alone(kind, scheme):
    f, kit, runs = _single_runs(kind, scheme)
    every, base = runs["all"], runs["base"]
    _same(every, base, ("state", "tracers", "forcing"), (kind, scheme, "all vs base"))
    assert every["infos"] == base["infos"], (kind, scheme, every["infos"], base["infos"])
    for name, n in base["launches"].items():
        assert every["launches"][name] == n, (kind, scheme, name)
    assert base["launches"]["tracer_mix_launches"] == NSTEPS and base["launches"]["tracer_vmix_launches"] == NSTEPS
    assert base["launches"]["forcing_launches"] > 2
    for x in K.DIAGNOSTICS:
        alone = runs[x]
        keys = (x, "float_track") if x == "floats" else (x,)
        _same(every, alone, keys, (kind, scheme, "all vs base + " + x))
        _same(alone, base, ("state", "tracers", "forcing"), (kind, scheme, "base + %s vs base" % x))
        assert alone["infos"] == base["infos"], (kind, scheme, x)
        for name, n in alone["launches"].items():      # (the floats launch once more per call: stage 1 alone in front of it)
            want = n + 1 if name == "float_launches" else n
            assert every["launches"][name] == want, (kind, scheme, x, name, every["launches"][name], want)
    # what the accumulators say of themselves
    for x in K.ACCUMULATORS:
        t = K.samples(K.STRIDES[x], 1, NSTEPS)
        assert (every[x]["count"], every[x]["tstp_first"], every[x]["tstp_last"]) == (len(t), t[0], t[-1]), x
    for x in K.RECORDERS + ("float_track",):
        assert list(every[x]["tstp"]) == K.samples(K.STRIDES[x], 1, NSTEPS), x
    assert every["launches"]["moment_launches"] == 6 and every["launches"]["tracer_moment_launches"] > 0
    assert every["launches"]["harmonic_launches"] == 5 * NSTEPS and every["launches"]["map_launches"] == 4
    # the forcing moves the step, the tracers are passive
    assert not same_bits(base["state"]["u"], runs["bare"]["state"]["u"]), "the frames change nothing: nothing tested"
    assert not same_bits(base["state"]["hlay"], runs["bare"]["state"]["hlay"]), "hdot changes nothing: nothing tested"


# ---- b. anchors outside the engine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("kind", list(KINDS))
def test_everything_on_one_handle_equals_the_restatements(kind, scheme):
    f, kit, runs = _single_runs(kind, scheme)
    every = runs["all"]
    p, nl, ntrc = f.p, f.p.nlay, kit.ntrc
    st, q = every["state"], every["tracers"]["q"]
    assert all(np.isfinite(st[k]).all() for k in STATE) and np.isfinite(q).all() and np.isfinite(every["tracers"]["rq"]).all()
    hq = (st["hlay"], st["h_u"], st["h_v"], q)
    win = kit.windows
    # the last record of each recorder is the restatement on the downloaded state and tracers
    ser, tser, cser, tcser, maps = (every[k] for k in K.RECORDERS)
    for rec in (ser, tser, cser, tcser, maps):
        assert rec["tstp"][-1] == NSTEPS
    assert same_bits(ser["rows"][-1], S.row_record(f, st, 2)), "series"
    assert same_bits(tser["rows"][-1], TS.row_record(f, *hq, 3)), "tracer series"
    assert same_bits(cser["cols"][-1], CS.column_record(f, st, 2, rows=win["column_series"])), "column series"
    assert same_bits(tcser["cols"][-1], TCS.column_record(f, *hq, 3, rows=win["tracer_column_series"])), "tracer column series"
    assert same_bits(maps["raw"][-1], MR.record(f, st, 3, K.MAPS_BLOCK, q)), "maps"
    assert maps["block"] == K.MAPS_BLOCK
    # ... and each of them is live: nothing moves, nothing tested
    assert ser["ke"][-1].any() and ser["tu"][-1].any() and ser["tv"][-1].any(), "no transport anywhere: nothing tested"
    assert tser["fu"][-1].any() and tser["fv"][-1].any() and np.all(tser["inv"][-1].any(axis=0))
    wet_rows = np.isfinite(tser["cmin"][-1][:, 1:])
    assert wet_rows.any() and np.any(tser["cmin"][-1][:, 1:][wet_rows] < tser["cmax"][-1][:, 1:][wet_rows])
    assert cser["tu"][-1].any() and cser["tv"][-1].any() and tcser["fu"][-1].any() and tcser["fv"][-1].any()
    assert not same_bits(cser["cols"][-1], CS.column_record(f, st, 2)), "the row window cuts nothing off: nothing tested"
    assert not same_bits(tcser["cols"][-1], TCS.column_record(f, *hq, 3)), "the row window cuts nothing off: nothing tested"
    assert not same_bits(tcser["cols"][-1], TCS.column_record(f, *hq, 3, rows=win["column_series"])), "one window for both"
    assert maps["hu"][-1].any() and maps["hv"][-1].any() and np.all(maps["q"][-1].reshape(ntrc * nl, -1).any(axis=1))
    for rec, key in ((ser, "rows"), (tser, "rows"), (cser, "cols"), (tcser, "cols"), (maps, "raw")):
        assert not same_bits(rec[key][-1], rec[key][0]), "a record that does not change: nothing tested"
    # the unit tracer is the thickness, with every mixing, both frame sets and every diagnostic on
    assert same_bits(q[0][:, 1:], st["hlay"][:, 1:]), "the unit tracer left the thickness"
    assert not same_bits(st["hlay"], f.hlay), "the thickness did not move: nothing tested"
    for t in range(1, ntrc):
        assert not same_bits(q[t], kit.q[t]) and not same_bits(q[t][:, 1:], st["hlay"][:, 1:]), (t, "a rough tracer did not move")
    assert same_bits(tser["fu"][-1][:, 0], ser["tu"][-1]) and same_bits(tser["fv"][-1][:, 0], ser["tv"][-1]), "the unit tracer's fluxes"
    # the frames in the buffers are those of step 12
    for field, (times, frames, period) in (("taus", kit.taus), ("hdot", kit.hdot)):
        want = FO.field(frames, times, period, kit.ctim(NSTEPS))
        assert same_bits(every["forcing"][field], want) and want.any(), field
    assert not same_bits(every["forcing"]["taus"], kit.taus[1][0]) and not same_bits(every["forcing"]["taus"], kit.taus[1][2])
    # the harmonics' normal matrix is the host sum of the weights over the sampled steps
    har = every["harmonics"]
    gram = np.zeros((5, 5))
    for t in K.samples(K.STRIDES["harmonics"], 1, NSTEPS):
        w = np.array([1.0] + [x for om in kit.omega for x in capi.harmonic_weights(om, kit.ctim(t))])
        gram = gram + np.outer(w, w)
    assert same_bits(har["gram"], gram) and list(har["omega"]) == list(kit.omega)
    assert har["sum"].shape == (5, 5, nl, p.ndeg + 1) and all(har["sum"][i, m][:, 1:].any() for i in range(5) for m in range(5))
    assert "amp" in har and np.isfinite(har["amp"]).all(), "twelve samples determine five coefficients"
    # moments and tracer moments are live at their top level
    mo, tm = every["moments"], every["tracer_moments"]
    assert mo["sum"].shape[0] == 5 and mo["sq"].shape[0] == 5 and all(mo["sq"][k][:, 1:].any() for k in range(5))
    assert tm["sum"].shape[:2] == (4, ntrc) and all(tm["sum"][m, t][:, 1:].any() for m in range(4) for t in range(1, ntrc))
    assert all(tm["sq"][t][:, 1:].any() for t in range(1, ntrc))
    # the float track's last record is where the floats are
    fl, tr = every["floats"], every["float_track"]
    assert tr["tstp"][-1] == NSTEPS and tr["x"].shape == (NSTEPS // 2, K.NFLOATS)
    assert same_bits(tr["x"][-1], fl["x"]) and same_bits(tr["y"][-1], fl["y"])
    assert not same_bits(fl["x"], kit.floats[0]) and not same_bits(fl["y"], kit.floats[1]), "the floats did not move: nothing tested"
    assert not same_bits(tr["x"][-1], tr["x"][0]) and tr["h"][-1].all()


# ---- c. bands keep the single handle's bits -------------------------------------------------------------------------------------
BAND_FRAMES = {"closed_3l": 1, "closed_3l_island": 2, "sill_sponges": 1, "jet_ring": 2}      # frame: tracer scheme (rings carry none)
CUT = ("closed_3l", "closed_3l_island")               # closed frames: every band's step is cut from step 4 on
_ONE = {}


@pytest.fixture(scope="module")
def band_frames():
    """The frames of the banded cases, built once in front of them (the sill's rest state is an iteration in numpy that takes
    seconds on the host: set-up that the cases share, not part of any of them)."""
    return {name: K.frame(name) for name in BAND_FRAMES}


def _band_kit(name):
    f = K.frame(name)
    kit = K.Kit(f, seed=2, scheme=BAND_FRAMES[name])
    return f, kit, kit.keeps("ring" if name == "jet_ring" else "bands")


def _one(name):
    """The single handle with the kit the frame's bands keep, in one call of 12 steps; once per frame."""
    if name not in _ONE:
        f, kit, parts = _band_kit(name)
        e = kit.apply(capi.Engine(f), parts)
        _ONE[name] = _run(e, kit, parts, (NSTEPS,))
        e.close()
    return _ONE[name]


def _same_floats(got, want, what):
    assert same_bits(got["x"], want["x"]), (what, "x", float(np.max(np.abs(got["x"] - want["x"]))))
    assert same_bits(got["y"], want["y"]), (what, "y", float(np.max(np.abs(got["y"] - want["y"]))))
    assert np.array_equal(got["layer"], want["layer"]) and np.array_equal(got["rejected"], want["rejected"]), (what, "rejected")


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("nband", [2, 3])
@pytest.mark.parametrize("name", list(BAND_FRAMES))
def test_bands_keep_the_single_handles_bits(band_frames, name, nband, overlap):
    """(sill_sponges on 3 bands is the case that found update_h's shortcut for gene = 0: the middle band has no sponge row and
    runs the unforced form, the single handle the nudged one, which kept a -0.0 thickness in dry cells under a negative
    hdot where the reference gives +0.0; the moments' first sample, behind step 2, showed it.)"""
    f, kit, parts = _band_kit(name)
    ring = name == "jet_ring"
    base = tuple(k for k in K.BASE if k in parts)
    assert ("tracers" in parts) != ring and "floats" in parts and "harmonics" in parts and "series" in parts
    one = _one(name)

    def banded(parts, calls):
        m = capi.MultiEngine(f, devices=[0] * nband)
        assert m.count == nband and m.describe()["ring"] == int(ring)
        m.set_option("overlap", overlap)
        kit.apply(m, parts)
        out = _run(m, kit, parts, calls)
        out["stats"] = m.stats()
        m.close()
        return out

    many, plain = banded(parts, (5, 7)), banded(base, (5, 7))
    what = (name, nband, overlap)
    # the add-ons leave the bands' step as it was, and the bands step as the single handle does
    _same(many, plain, ("state",) + base, what + ("many vs plain",))
    for k in PROGNOSTIC:
        assert same_bits(many["state"][k], one["state"][k]), what + ("many vs one", k)
    _same(many, one, tuple(k for k in parts if k != "floats"), what + ("many vs one",))
    _same_floats(many["floats"], one["floats"], what)
    for k, n in one["launches"].items():               # (the floats launch once more per call: stage 1 alone in front of it)
        assert many["launches"][k] == (n + 1 if k == "float_launches" else n), (what, k, many["launches"][k], n)
    assert many["stats"] == plain["stats"], (what, many["stats"], plain["stats"], "the add-ons changed how the bands' steps are cut")
    if not overlap:
        assert many["stats"]["split"] == 0, (what, many["stats"])
    elif name in CUT:
        assert many["stats"]["split"] >= nband * (NSTEPS - 3), (what, many["stats"], "the bands' steps were not cut")
    # live: the single handle's downloads are the ones held to the restatements in (b); here they must move at all
    assert not same_bits(one["floats"]["x"], kit.floats[0]) and one["series"]["tu"][-1].any() and one["harmonics"]["count"] == NSTEPS
    assert all(one["moments"]["sq"][k][:, 1:].any() for k in range(5))
    if not ring:
        assert same_bits(one["tracers"]["q"][0][:, 1:], one["state"]["hlay"][:, 1:]), "the unit tracer left the thickness"
        assert not same_bits(one["tracers"]["q"][1], kit.q[1]) and one["tracer_series"]["fv"][-1].any()
        assert one["tracer_moments"]["count"] == 4
    if name == "closed_3l":                            # another division of the same run gives the same bits again
        again = banded(parts, (1,) * NSTEPS)
        _same(again, many, ("state",) + tuple(k for k in parts if k != "floats"), what + ("calls of one step",))
        _same_floats(again["floats"], many["floats"], what + ("calls of one step",))
        assert again["stats"] == many["stats"]


# ---- d. lifecycle in mid-run ----------------------------------------------------------------------------------------------------
def _make(kind, f):
    if kind == "single":
        return capi.Engine(f)
    m = capi.MultiEngine(f, devices=[0, 0, 0])
    assert m.count == 3
    return m


@pytest.mark.parametrize("kind", ["single", "bands"])
def test_lifecycle_in_mid_run(kind):
    """Five steps under the full kit; harmonics, series and floats freed, the moments reset, state and tracers taken down and
    put back, the taus set cleared, set_tracers with the same count; four steps; set_tracers(2) and a two-tracer kit; three
    steps.  A second handle, built fresh at each change from the first one's downloads with what is alive in the segment,
    reproduces each segment."""
    f = K.frame("closed_3l")
    kit = K.Kit(f, seed=3, scheme=2)
    parts = kit.keeps(kind)
    single = kind == "single"
    on_tracers = tuple(k for k in TRACER_PARTS if k in parts)
    e = kit.apply(_make(kind, f), parts)
    e.step(1, 5)

    # ---- the first change
    e.set_harmonics(())
    e.set_series(0)
    e.set_floats([], [], 1)
    assert (e.info("harmonics"), e.info("series"), e.info("floats")) == (0, 0, 0)
    e.reset_moments()
    st5, tr5 = e.download(), e.download_tracers()
    e.upload(**_no_stress(st5))
    e.set_forcing("taus", None)
    e.set_tracers(kit.ntrc)                            # the same count: everything that hangs on the tracers stays
    assert (e.info("tracers"), e.info("tracer_mixing"), e.info("tracer_vmixing"), e.info("tracer_scheme")) == (3, 1, 1, 2)
    assert (e.info("tracer_moments"), e.info("tracer_moment_samples")) == (3, 1)
    assert e.info("tracer_series") == 3
    if single:
        assert e.info("tracer_series_records") == 2
        assert (e.info("tracer_column_series"), e.info("tracer_column_series_records")) == (3, 1)
        assert (e.info("maps"), e.info("maps_block"), e.info("maps_records")) == (3, K.MAPS_BLOCK, 1)
        assert (e.info("column_series"), e.info("column_series_records")) == (2, 2)
    assert (e.info("moments"), e.info("moment_samples")) == (3, 0)
    e.upload_tracers(q=tr5["q"], rq=tr5["rq"], ctrg=kit.ctrg)
    e.step(6, 4)
    alive2 = tuple(k for k in parts if k not in ("harmonics", "series", "floats", "float_track"))
    first2 = kit.collect(e, tuple(k for k in alive2 if k in ("tracers", "forcing") + on_tracers))      # (the moments and the column series go on)
    assert (first2["tracer_moments"]["count"], first2["tracer_moments"]["tstp_first"], first2["tracer_moments"]["tstp_last"]) == (3, 3, 9)
    assert list(first2["tracer_series"]["tstp"]) == [2, 4, 6, 8]

    twin = kit.apply(_make(kind, f), alive2)
    twin.upload(**_no_stress(st5))
    twin.set_forcing("taus", None)
    twin.upload_tracers(q=tr5["q"], rq=tr5["rq"], ctrg=kit.ctrg)
    twin.step(6, 4)
    second2 = kit.collect(twin, alive2)
    for k in PROGNOSTIC:
        assert same_bits(first2["state"][k], second2["state"][k]), (kind, "steps 6-9", k)
    _same(first2, second2, ("tracers", "forcing"), (kind, "steps 6-9"))
    for k in on_tracers:
        if k != "tracer_moments":                      # (the first handle's tracer moments began at step 3)
            d = K.differences(_from_step(first2[k], 6), _from_step(second2[k], 6), k)
            assert d == [] and list(second2[k]["tstp"]) == K.samples(K.STRIDES[k], 6, 9), (kind, "steps 6-9", d)
    twin.close()

    # ---- the second change: another tracer count
    mom9 = e.download_moments()
    _same({"moments": mom9}, second2, ("moments",), (kind, "the moments since their reset"))
    assert (mom9["count"], mom9["tstp_first"], mom9["tstp_last"]) == (2, 6, 8)
    e.set_tracers(2)
    assert (e.info("tracers"), e.info("tracer_mixing"), e.info("tracer_vmixing"), e.info("tracer_scheme")) == (2, 0, 0, 2)
    assert (e.info("tracer_moments"), e.info("tracer_series"), e.info("tracer_series_records")) == (0, 0, 0)
    if single:
        assert (e.info("tracer_column_series"), e.info("maps"), e.info("maps_block")) == (0, 0, 0)
        assert (e.info("column_series"), e.info("column_series_records")) == (2, 4), "the column series was touched"
    for call in (e.download_tracer_moments, e.download_tracer_series):
        with pytest.raises(capi.BeomError):
            call()
    assert (e.info("moments"), e.info("moment_samples")) == (3, 2)
    _same({"moments": e.download_moments()}, {"moments": mom9}, ("moments",), (kind, "the moments were touched"))
    st9 = first2["state"]
    kit2 = K.Kit(f, seed=4, scheme=2, ntrc=2, state=st9)
    rearmed = tuple(k for k in parts if k in ("tracers", "harmonics", "series", "floats", "float_track") + on_tracers)
    kit2.apply(e, rearmed)
    e.step(10, 3)
    first3 = kit2.collect(e, rearmed)
    first3["moments"] = e.download_moments()
    if single:
        first3["column_series"] = e.download_column_series()

    carried = tuple(k for k in ("forcing", "moments", "column_series") if k in parts)
    twin = kit.apply(_make(kind, f), carried)
    twin.upload(**_no_stress(st9))
    twin.set_forcing("taus", None)
    kit2.apply(twin, rearmed)
    twin.step(10, 3)
    second3 = kit2.collect(twin, rearmed)
    for k in PROGNOSTIC:
        assert same_bits(first3["state"][k], second3["state"][k]), (kind, "steps 10-12", k)
    _same(first3, second3, rearmed, (kind, "steps 10-12"))
    if single:
        assert list(first3["column_series"]["tstp"]) == [2, 4, 6, 8, 10, 12]
        d = K.differences(_from_step(first3["column_series"], 10), _from_step(twin.download_column_series(), 10), "column_series")
        d += K.differences(_from_step(first3["column_series"], 6, 9), _from_step(second2["column_series"], 6, 9), "column_series")
        assert d == [], (kind, "steps 6-12", d)
    twin.close()
    # the counts are what the documented rules say: the moments count from their reset, the others from their set
    mo = first3["moments"]
    assert (mo["count"], mo["tstp_first"], mo["tstp_last"]) == (4, 6, 12)
    tm, ha = first3["tracer_moments"], first3["harmonics"]
    assert (tm["count"], tm["tstp_first"], tm["tstp_last"]) == (1, 12, 12) and tm["ref"].shape[1] == 2
    assert (ha["count"], ha["tstp_first"], ha["tstp_last"]) == (3, 10, 12)
    assert list(first3["series"]["tstp"]) == [10, 11, 12] and list(first3["tracer_series"]["tstp"]) == [10, 12]
    q = first3["tracers"]["q"]
    assert q.shape[0] == 2 and same_bits(q[0][:, 1:], first3["state"]["hlay"][:, 1:]), "the unit tracer left the thickness"
    assert not same_bits(q[1], kit2.q[1]) and not same_bits(first3["floats"]["x"], kit2.floats[0]), "nothing moves: nothing tested"
    assert not same_bits(first3["state"]["u"], st9["u"]) and not same_bits(st9["u"], st5["u"])
    # a handle with the base alone, never taken down and put back, ends in the same state; on bands the lifecycle leaves
    # the cut of the steps as it is
    plain = kit.apply(_make(kind, f), K.BASE)
    plain.step(1, 5)
    plain.set_forcing("taus", None)
    plain.step(6, 4)
    plain.set_tracers(2)
    kit2.apply(plain, ("tracers",))
    plain.step(10, 3)
    last = plain.download(PROGNOSTIC)
    for k in PROGNOSTIC:
        assert same_bits(last[k], first3["state"][k]), (kind, "plain", k)
    assert same_bits(plain.download_tracers()["q"], q), (kind, "plain", "q")
    if not single:
        assert e.stats() == plain.stats() and plain.stats()["split"] >= 3 * (NSTEPS - 3), (e.stats(), plain.stats())
    plain.close()
    e.close()


# ---- e. every permutation class of set-up order -----------------------------------------------------------------------------------
def _legal(order):
    """The order with everything that needs the tracers directly behind them (in the order it came), the track flag last."""
    needy = [k for k in order if k in TRACER_PARTS]
    out = []
    for k in order:
        if k in TRACER_PARTS or k == "float_track":
            continue
        out.append(k)
        if k == "tracers":
            out += needy
    return tuple(out) + ("float_track",)


def _orders():
    acc, rec, flo = K.ACCUMULATORS, K.RECORDERS, ("floats",)
    forward = K.BASE + acc + rec + flo
    return {"forward": forward, "reverse": forward[::-1], "recorders_first": rec + acc + flo + K.BASE,
            "accumulators_first": acc + flo + rec + K.BASE[::-1], "forcing_last": tuple(k for k in forward if k != "forcing") + ("forcing",),
            "tracers_last": tuple(k for k in forward[::-1] if k != "tracers") + ("tracers",)}


def test_every_set_up_order_gives_the_same_bits():
    f = K.frame("island_ragged_129x33_2l")
    kit = K.Kit(f, seed=5, scheme=2, nsteps=6)
    orders = {k: _legal(v) for k, v in _orders().items()}
    assert len(set(orders.values())) == 6 and all(sorted(o) == sorted(K.EVERYTHING) for o in orders.values()), orders
    for o in orders.values():
        assert all(o.index(k) > o.index("tracers") for k in TRACER_PARTS)
    runs = {}
    for name, order in orders.items():
        e = capi.Engine(f)
        assert e.is_embedded
        kit.apply(e, order)
        runs[name] = _run(e, kit, K.EVERYTHING, (6,))
        e.close()
    want = runs["forward"]
    for name, got in runs.items():
        _same(got, want, ("state",) + K.EVERYTHING, (name, "vs forward"))
        assert got["launches"] == want["launches"] and got["infos"] == want["infos"], name
    assert want["moments"]["count"] == 3 and want["tracer_moments"]["count"] == 2 and want["harmonics"]["count"] == 6
    assert list(want["maps"]["tstp"]) == [3, 6] and want["maps"]["q"][-1].any() and want["series"]["tu"][-1].any()
    assert not same_bits(want["floats"]["x"], kit.floats[0]) and not same_bits(want["tracers"]["q"][1], kit.q[1])
