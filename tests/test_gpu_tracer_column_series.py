"""The tracer column series on the device (beom_set_tracer_column_series, include/beom_hip.h) against the numpy restatement
(tracer_column_series_ref, tied to column_series_ref and tracer_series_ref by test_tracer_column_series_cpu) applied to the
state and tracers downloaded at the record's step.  Every comparison with the restatement is helpers.same_bits: the order of
summation (the pairwise tree over the aligned global row index) is the contract and the bounds see no signed zero, so a dense
handle, an embedded one and the table path give the same bits, whatever the division into calls, the row window's place or
the batches of column chunks.  The only tolerance is the cross-check against the tracer series' total, which adds in another
order."""
import numpy as np
import pytest

import tracer_column_series_ref as TC
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, same_bits
from test_gpu_biharm_tiled import CASES
from test_gpu_column_series import _case
from test_gpu_series import _refusal
from test_gpu_tracer_series import _with_tracers
from test_tracer_series_cpu import rough_case

pytestmark = pytest.mark.gpu
HQ = ("hlay", "h_u", "h_v")

BAD_ARGS = "beom_set_tracer_column_series: level %d, stride %d, %d records (level 0..3, stride >= 1, records >= 1)"
BAD_ROWS = "beom_set_tracer_column_series: rows %d..%d outside 1..%d"
OVERFLOW = ("beom_step: steps %d..%d would write %d records of the tracer column series (stride %d) but the recorder holds %d of %d: "
            "empty it with beom_download_tracer_column_series, or take fewer steps per call")
NONE = "beom_download_tracer_column_series: the handle keeps no tracer column series (beom_set_tracer_column_series)"
NO_TRACER = "beom_set_tracer_column_series: the handle carries no tracer (beom_set_tracers comes first)"
SAMPLE = "beom_sample_tracer_column_series (tracer column series set? recorder full?)"
ON_BANDS = ("%s: a handle on bands keeps no tracer column series (a column's tree over the global rows crosses the bands, "
            "and nothing combines the bands' tree nodes yet); use a single handle (beom_set_tracer_column_series)")
ON_A_BAND = "beom_set_tracer_column_series: a handle on a band of rows keeps no tracer column series (a column's tree crosses the bands)"


def _series_of(e, calls, level, stride=1, records=16, rows=None):
    e.set_tracer_column_series(level, stride, records, rows)
    t = 1
    for n in calls:
        e.step(t, n)
        t += n
    return e.download_tracer_column_series()


def _restated(f, e, level, rows=None):
    st = e.download(HQ)
    return TC.column_record(f, st["hlay"], st["h_u"], st["h_v"], e.download_tracers()["q"], level, rows)


def _same_views(got, want, ntrc, nl, level, p, what):
    v = TC.views(want, ntrc, nl, level)
    for k in TC.NAMES[:2 * level]:
        assert same_bits(got[k], v[k]), (what, k)
    for k in TC.NAMES[2 * level:] + ("transport",) * (level < 2):
        assert k not in got, (what, k)
    assert same_bits(got["total"], TC.total(want, ntrc, nl, level)), (what, "total")
    if level >= 2:
        assert same_bits(got["transport"], float(p.dl) * v["fu"]), (what, "transport")


# ---- 1. every level on each handle kind ---------------------------------------------------------------------------------------
_TWIN = {}


def _twin_records(name, ntrc, nsteps):
    """The restatement at level 3 of a twin handle's state and tracers behind each of its first steps, formed once per frame
    and tracer count and left unchanged (the lower levels are its prefixes: test_tracer_column_series_cpu)."""
    key = (name, ntrc)
    if key not in _TWIN:
        f = _case(name)
        twin = _with_tracers(capi.Engine(f), f, ntrc)
        out = []
        for t in range(1, nsteps + 1):
            twin.step(t, 1)
            out.append(_restated(f, twin, 3))
        twin.close()
        _TWIN[key] = (f, np.stack(out))
    return _TWIN[key]


def _records_on_each_handle_kind(name, level, ntrc):
    calls = (1,) if name == "wide_67_chunks" else (4, 2)         # (4201 columns: one record only)
    n = sum(calls)
    f, want3 = _twin_records(name, ntrc, n)
    nl, L = f.p.nlay, f.p.lm + 1
    want = np.ascontiguousarray(want3.reshape(n, L, ntrc, nl, 6)[..., :2 * level]).reshape(n, L, -1)
    e, tab = _with_tracers(capi.Engine(f), f, ntrc), _with_tracers(capi.Engine(f, dense_hint=0), f, ntrc)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    a, b = _series_of(e, calls, level), _series_of(tab, calls, level)
    cnt = TC.count(ntrc, nl, level)
    assert cnt == e.lib.beom_tracer_series_count(ntrc, nl, level)
    for got in (a, b):
        assert got["count"] == n and list(got["tstp"]) == list(range(1, n + 1)) and got["cols"].shape == (n, L, cnt)
    assert same_bits(a["cols"], b["cols"]), (name, level, ntrc, "dense vs table path")
    assert not np.isnan(want).any()
    for k in range(n):
        assert same_bits(a["cols"][k], want[k]), (name, level, ntrc, k + 1)
    _same_views(a, want, ntrc, nl, level, f.p, (name, level, ntrc))
    _same_views(b, want, ntrc, nl, level, f.p, (name, level, ntrc, "table path"))
    assert np.all(a["inv"][-1].any(axis=0)) and np.all(a["var"][-1].any(axis=0)), (name, "an empty tracer-layer: nothing tested")
    if level >= 2:
        assert a["fu"][-1].any() and a["fv"][-1].any(), (name, "no flux anywhere: nothing tested")
    if level >= 3:
        wet = np.isfinite(a["cmin"][-1])
        assert wet.any() and np.all(a["cmin"][-1][wet] <= a["cmax"][-1][wet])
        if name == "island_ragged_3l":
            assert (~wet).any(), (name, "no column without a wet cell")
            assert np.all(a["cmin"][-1][~wet] == np.inf) and np.all(a["cmax"][-1][~wet] == -np.inf)
    e.close(); tab.close()


@pytest.mark.parametrize("ntrc", [1, 3])
@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("name", ["jet_xyper_2l", "island_ragged_3l", "closed_12l", "soliton_xper", "tall_4201_rows",
                                  "wide_67_chunks"])
def test_records_on_each_handle_kind(name, level, ntrc):
    _records_on_each_handle_kind(name, level, ntrc)


# ---- 2. the widest instantiation ----------------------------------------------------------------------------------------------
def test_eight_tracers_at_level_3():
    _records_on_each_handle_kind("island_ragged_3l", 3, 8)


# ---- 3. rough contents by hand: negative and -0 concentrations, dry cells -----------------------------------------------------
@pytest.mark.parametrize("config", ["island_ragged_3l", "jet_xyper_2l"])
def test_rough_contents_by_hand(config):
    """The rough state and tracers of test_tracer_series_cpu.rough_case as uploaded (no step): concentrations below zero and of
    -0, dry cell-layers with a stranded content.  Level 3, dense and table path; h_u and h_v are told apart; a concentration
    of -0 shows as +0 in the bounds (no bound is a negative zero)."""
    g, st, q = rough_case(config)
    nl, ntrc = g.p.nlay, q.shape[0]
    want = TC.column_record(g, st["hlay"], st["h_u"], st["h_v"], q, 3)
    swapped = TC.views(TC.column_record(g, st["hlay"], st["h_v"], st["h_u"], q, 3), ntrc, nl, 3)
    for dense_hint in (1, 0):
        e = capi.Engine(g, dense_hint=dense_hint)
        e.set_tracers(ntrc)
        e.upload(**st)
        e.upload_tracers(q=q)
        e.set_tracer_column_series(3, 1, 1)
        e.sample_tracer_column_series()
        got = e.download_tracer_column_series()
        assert list(got["tstp"]) == [0]
        assert same_bits(got["cols"][0], want), (config, dense_hint)
        _same_views(got, want[None], ntrc, nl, 3, g.p, (config, dense_hint))
        assert not same_bits(got["fu"][0], swapped["fu"]) and not same_bits(got["fv"][0], swapped["fv"])
        assert got["fu"].any() and got["fv"].any()
        for k in ("cmin", "cmax"):
            zero = got[k][0] == 0.0
            assert not np.signbit(got[k][0][zero]).any(), (config, k, "a bound of -0")
        e.close()
    # the -0 concentrations are there, and one of them is a column's bound in the restatement: what the device matched
    c = np.where(st["hlay"][None] > 0.0, q / np.where(st["hlay"][None] > 0.0, st["hlay"][None], 1.0), 0.0)
    assert np.any((c == 0.0) & np.signbit(c) & (st["hlay"][None] > 0.0))


# ---- 4. frames of very few rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm,yper", [(1, False), (1, True), (2, False), (2, True)])
def test_frames_of_very_few_rows(mm, yper):
    """mm = 1: columns of two rows, the tree is padded to 2 and every row past it inside the block of 32 holds -0.0; periodic
    in y (the jet's frame, periodic in x too) the last row is the duplicate and a column of mm = 1 is one live cell.  mm = 2:
    three rows, padded to 4.  Ten columns, so 54 lanes of the one column chunk are idle.  Built as test_frames_narrower_than_four_columns builds its frames,
    with the axes exchanged; by hand on uploaded contents, no step."""
    p, files = I.case_unstable_jet(lm=9, mm=mm, nlay=2, dt_s=1.5) if yper else I.case_headline(9, mm, 2)
    f = read_input_data(p, files=files)
    assert f.p.mm + 1 == mm + 1 < 4 and (float(f.p.yper) > 0.5) == yper
    r = np.random.default_rng([mm, int(yper), 78])
    h = np.asarray(f.hlay, dtype=np.float64)
    st = {"hlay": h, "h_u": r.uniform(-1.0, 1.0, h.shape), "h_v": r.uniform(-1.0, 1.0, h.shape)}
    st["h_u"][:, 0] = 0.0; st["h_v"][:, 0] = 0.0
    q = np.ascontiguousarray(r.uniform(-0.4, 1.2, (2,) + h.shape) * h[None])
    for dense_hint in (1, 0):
        e = capi.Engine(f, dense_hint=dense_hint)
        e.set_tracers(2)
        e.upload(**st)
        e.upload_tracers(q=q)
        for level in (1, 2, 3):
            e.set_tracer_column_series(level, 1, 1)
            e.sample_tracer_column_series()
            got = e.download_tracer_column_series()
            want = TC.column_record(f, h, st["h_u"], st["h_v"], q, level)
            assert same_bits(got["cols"][0], want), (mm, yper, dense_hint, level)
        assert got["inv"].any() and got["fu"].any()
        e.close()


# ---- 5. both schemes, with lateral and vertical mixing ------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [1, 2])
def test_both_schemes_with_mixing(scheme):
    """The record reads the final arrays only: whatever advected and mixed the tracers, it equals the restatement on the
    downloads.  Under scheme 2 the faces are still the upstream ones."""
    f = _case("island_ragged_3l")
    p, ntrc = f.p, 3
    e = _with_tracers(capi.Engine(f), f, ntrc)
    e.set_tracer_scheme(scheme)
    e.set_tracer_mixing(kappa=0.2 * float(p.dl) ** 2 / float(p.dt), decay=0.02 / float(p.dt))
    e.set_tracer_vertical_mixing(1.0e-3)
    e.set_tracer_column_series(3, 1, 4)
    want = []
    for t in range(1, 5):
        e.step(t, 1)
        want.append(_restated(f, e, 3))
    got = e.download_tracer_column_series()
    assert e.info("tracer_scheme") == scheme and e.info("tracer_mix_launches") == 4 and e.info("tracer_vmix_launches") == 4
    assert list(got["tstp"]) == [1, 2, 3, 4]
    for k in range(4):
        assert same_bits(got["cols"][k], want[k]), (scheme, k + 1)
    assert not same_bits(got["cols"][3], got["cols"][0])
    e.close()


# ---- 6. the unit tracer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jet_xyper_2l", "island_ragged_3l"])
def test_the_unit_tracer_carries_the_column_series_transports(name):
    """Concentration 1 (and the thickness' own history, relaxation concentration 1): q stays hlay bit for bit, so fu, fv are
    the column series' tu, tv at every step, from the same handle keeping both recorders; inv = var, and the bounds are 1.0
    on every column with a wet cell."""
    f = _case(name)
    e = capi.Engine(f)
    e.set_tracers(1)
    q = e.set_concentration(1.0)
    e.upload_tracers(rq=np.ascontiguousarray(np.asarray(f.rs_h, dtype=np.float64)[None]), ctrg=np.ones_like(q))
    e.set_column_series(2, 1, 8)
    e.set_tracer_column_series(3, 1, 8)
    e.step(1, 4); e.step(5, 2)
    ser, trc = e.download_column_series(), e.download_tracer_column_series()
    assert list(ser["tstp"]) == list(trc["tstp"]) == [1, 2, 3, 4, 5, 6]
    assert same_bits(e.download_tracers()["q"][0][:, 1:], e.download(("hlay",))["hlay"][:, 1:]), name
    assert same_bits(trc["fu"][:, :, 0], ser["tu"]) and same_bits(trc["fv"][:, :, 0], ser["tv"]), name
    assert ser["tu"][-1].any() and ser["tv"][-1].any(), (name, "no transport anywhere: nothing tested")
    assert same_bits(trc["inv"], trc["var"]), name
    wet = np.isfinite(trc["cmin"])
    assert wet.any() and np.all(trc["cmin"][wet] == 1.0) and np.all(trc["cmax"][wet] == 1.0), name
    assert np.all(trc["cmin"][~wet] == np.inf) and np.all(trc["cmax"][~wet] == -np.inf)
    assert np.all(trc["inv"][wet] > 0.0) and not trc["inv"][~wet].any()
    e.close()


# ---- 7. division into calls, stride, the entry by hand ------------------------------------------------------------------------
def test_division_into_calls_and_stride():
    f = _case("jet_xyper_2l")
    nl, ntrc, L = f.p.nlay, 3, f.p.lm + 1
    runs = []
    for calls in ((12,), (5, 7), (1,) * 12):
        e = _with_tracers(capi.Engine(f), f, ntrc)
        runs.append(_series_of(e, calls, 3))
        e.close()
    for r in runs:
        assert list(r["tstp"]) == list(range(1, 13))
        assert same_bits(r["cols"], runs[0]["cols"])
    e = _with_tracers(capi.Engine(f), f, ntrc)
    r3 = _series_of(e, (5, 7), 3, stride=3)
    assert list(r3["tstp"]) == [3, 6, 9, 12]
    assert same_bits(r3["cols"], runs[0]["cols"][2::3])
    assert same_bits(r3["cols"][-1], _restated(f, e, 3))
    # the download has emptied the recorder
    assert e.info("tracer_column_series") == 3 and e.info("tracer_column_series_records") == 0
    again = e.download_tracer_column_series()
    assert again["count"] == 0 and again["cols"].shape[0] == 0 and again["tstp"].size == 0
    # one record by hand, under the last step's number, whatever the stride; uploads leave it where it is
    e.sample_tracer_column_series()
    assert e.info("tracer_column_series_records") == 1
    e.upload(**e.download())
    tr = e.download_tracers()
    e.upload_tracers(q=tr["q"], rq=tr["rq"])
    assert e.info("tracer_column_series_records") == 1
    got = e.download_tracer_column_series()
    assert got["count"] == 1 and list(got["tstp"]) == [12]
    assert same_bits(got["cols"][0], runs[0]["cols"][11])
    # other arguments reallocate and empty; the same tracer count keeps the recorder, another one frees it; level 0 frees
    e.sample_tracer_column_series()
    e.set_tracer_column_series(1, 2, 3)
    assert e.info("tracer_column_series") == 1 and e.info("tracer_column_series_records") == 0
    e.step(13, 4)
    assert list(e.download_tracer_column_series()["tstp"]) == [14, 16]
    e.set_tracers(ntrc)
    assert e.info("tracer_column_series") == 1
    e.set_tracers(2)
    assert e.info("tracer_column_series") == 0 and e.info("tracer_column_series_records") == 0
    assert _refusal(e.download_tracer_column_series, -3) == NONE
    e.set_tracer_column_series(2, 1, 2)
    assert e.download_tracer_column_series()["cols"].shape == (0, L, TC.count(2, nl, 2))
    e.set_tracer_column_series(0)
    assert e.info("tracer_column_series") == 0
    assert _refusal(e.download_tracer_column_series, -3) == NONE
    e.close()


# ---- 8. the row window --------------------------------------------------------------------------------------------------------
def test_row_window():
    f = _case("island_ragged_3l")
    M, nl, ntrc = f.p.mm + 1, f.p.nlay, 2
    assert M == 71
    e = _with_tracers(capi.Engine(f), f, ntrc)
    e.step(1, 3)
    st, tr = e.download(), e.download_tracers()
    recs = {}
    for rows in (None, (1, M), (20, 41), (71, 71)):
        want = TC.column_record(f, st["hlay"], st["h_u"], st["h_v"], tr["q"], 3, rows)
        for dense_hint in (1, 0):
            x = capi.Engine(f, dense_hint=dense_hint)
            x.set_tracers(ntrc)
            x.upload(**st)
            x.upload_tracers(q=tr["q"])
            x.set_tracer_column_series(3, 1, 1, rows)
            x.sample_tracer_column_series()
            got = x.download_tracer_column_series()["cols"][0]
            assert same_bits(got, want), (rows, dense_hint)
            recs[rows] = got
            x.close()
    assert same_bits(recs[(1, M)], recs[None])
    assert not same_bits(recs[(20, 41)], recs[None])
    whole, part = TC.views(recs[None], ntrc, nl, 3), TC.views(recs[(20, 41)], ntrc, nl, 3)
    assert part["inv"].any() and part["fu"].any()
    # bounds outside the window do not count: somewhere the window's bounds are strictly inside the column's
    assert np.all(part["cmin"] >= whole["cmin"]) and np.all(part["cmax"] <= whole["cmax"])
    assert np.any(part["cmin"] > whole["cmin"]) and np.any(part["cmax"] < whole["cmax"])
    e.close()


# ---- 9. batches ---------------------------------------------------------------------------------------------------------------
def test_batches_of_one_chunk_give_the_same_bits():
    f = _case("wide_67_chunks")
    a, b = _with_tracers(capi.Engine(f), f, 2), _with_tracers(capi.Engine(f), f, 2)
    b.set_option("tracer_column_series_batch", 1)
    ra, rb = _series_of(a, (1,), 3), _series_of(b, (1,), 3)
    assert ra["cols"].shape[1] == 4201 and ra["fu"].any()
    assert same_bits(ra["cols"], rb["cols"])
    a.close(); b.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    f = _case("island_ragged_3l")
    M = f.p.mm + 1
    e = capi.Engine(f)
    assert _refusal(lambda: e.set_tracer_column_series(1), -3) == NO_TRACER
    assert _refusal(e.download_tracer_column_series, -3) == NONE
    assert _refusal(e.sample_tracer_column_series, -3) == SAMPLE
    _with_tracers(e, f, 2)
    assert _refusal(e.download_tracer_column_series, -3) == NONE       # no recorder yet
    assert _refusal(e.sample_tracer_column_series, -3) == SAMPLE
    for args in ((4, 1, 4), (-1, 1, 4), (1, 0, 4), (2, 1, 0)):
        assert _refusal(lambda: e.set_tracer_column_series(*args), -3) == BAD_ARGS % args, args
    for rows in ((0, 5), (5, 4), (1, M + 1), (M + 1, M + 1)):
        assert _refusal(lambda: e.set_tracer_column_series(2, 1, 4, rows), -3) == BAD_ROWS % (rows + (M,)), rows
    assert e.info("tracer_column_series") == 0
    e.step(1, 3)
    e.set_tracer_column_series(3, 1, 4)
    before, qb = e.download(STATE), e.download_tracers()
    assert _refusal(lambda: e.step(4, 5), -3) == OVERFLOW % (4, 8, 5, 1, 0, 4)
    after, qa = e.download(STATE), e.download_tracers()
    for k in before:
        assert same_bits(before[k], after[k]), k
    assert same_bits(qb["q"], qa["q"]) and same_bits(qb["rq"], qa["rq"])
    assert e.info("tracer_column_series_records") == 0
    e.step(4, 4)
    assert e.info("tracer_column_series_records") == 4
    assert _refusal(e.sample_tracer_column_series, -3) == SAMPLE       # a full recorder
    assert _refusal(lambda: e.step(8, 1), -3) == OVERFLOW % (8, 8, 1, 1, 4, 4)
    assert e.info("tracer_column_series_records") == 4
    assert list(e.download_tracer_column_series()["tstp"]) == [4, 5, 6, 7]
    e.step(8, 1)                                                # the same step is taken once the recorder is empty
    assert list(e.download_tracer_column_series()["tstp"]) == [8]
    e.close()


def test_handles_on_bands_refuse():
    from beom_amd import slab
    f = _case("closed_12l")
    many = _with_tracers(capi.MultiEngine(f, devices=[0, 0]), f, 1)
    assert _refusal(lambda: many.set_tracer_column_series(2), -6) == ON_BANDS % "beom_multi_set_tracer_column_series"
    assert _refusal(many.download_tracer_column_series, -6) == ON_BANDS % "beom_multi_download_tracer_column_series"
    many.close()
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    assert _refusal(lambda: band.set_tracer_column_series(2), -6) == ON_BANDS % "beom_multi_set_tracer_column_series"
    assert _refusal(band.download_tracer_column_series, -6) == ON_BANDS % "beom_multi_download_tracer_column_series"
    band.close()
    # a single handle that is a band of rows
    geo = slab.decompose(f.p.mm, f.p.lm, 2)[0]
    e = capi.Engine(slab.slice_fields(f, geo), slab_row0=geo.row0, slab_mm=f.p.mm)
    e.set_tracers(1)
    assert _refusal(lambda: e.set_tracer_column_series(2), -6) == ON_A_BAND
    e.close()


# ---- 11. the recorders together -----------------------------------------------------------------------------------------------
def test_recorders_together_and_the_state():
    """One handle with the series, the column series, the tracer series, the tracer column series and integrals() between the
    steps: each recorder's records are those of a handle that keeps it alone, and the state and q are those of a handle with
    no recorder."""
    f = _case("island_ragged_3l")
    names = ("all", "series", "column", "tracer", "tracer_column", "plain")
    h = {k: _with_tracers(capi.Engine(f), f, 2) for k in names}
    for k in ("all", "series"):
        h[k].set_series(2, 1, 8)
    for k in ("all", "column"):
        h[k].set_column_series(2, 1, 8)
    for k in ("all", "tracer"):
        h[k].set_tracer_series(3, 1, 8)
    for k in ("all", "tracer_column"):
        h[k].set_tracer_column_series(3, 1, 8)
    for calls in ((1, 3), (4, 4)):
        for e in h.values():
            e.step(*calls)
        h["all"].integrals()
    a = h["all"]
    for what in ("mont_history", "plain_sweeps", "uv_fused"):
        assert a.info(what) == h["plain"].info(what), what
    got = a.download_tracer_column_series()
    assert got["count"] == 7 and same_bits(got["cols"], h["tracer_column"].download_tracer_column_series()["cols"])
    assert same_bits(got["cols"][-1], _restated(f, a, 3))
    assert same_bits(a.download_column_series()["cols"], h["column"].download_column_series()["cols"])
    assert same_bits(a.download_series()["rows"], h["series"].download_series()["rows"])
    assert same_bits(a.download_tracer_series()["rows"], h["tracer"].download_tracer_series()["rows"])
    sa, sp = a.download(), h["plain"].download()
    for k in sa:
        assert same_bits(sa[k], sp[k]), k
    ta, tp = a.download_tracers(), h["plain"].download_tracers()
    assert same_bits(ta["q"], tp["q"]) and same_bits(ta["rq"], tp["rq"])
    for e in h.values():
        e.close()


# ---- 12. the cross-check with the tracer series -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["island_ragged_3l", "jet_xyper_2l"])
def test_total_is_within_the_bound_of_the_tracer_series(name):
    """total adds along columns first, the tracer series' along rows first: two pairwise trees over the same terms x_q, each
    entry within 2 * gamma_D * sum |x_q| (tracer_column_series_ref.gamma_bound)."""
    f = _case(name)
    e = _with_tracers(capi.Engine(f), f, 3)
    e.set_tracer_series(1, 5, 1)
    got = _series_of(e, (5,), 1, stride=5)
    rows = e.download_tracer_series()
    assert list(got["tstp"]) == list(rows["tstp"]) == [5]
    st = e.download(HQ)
    bound = TC.gamma_bound(f, st["hlay"], st["h_u"], st["h_v"], e.download_tracers()["q"])
    diff = np.abs(got["total"][0] - rows["total"][0])
    print("total vs the tracer series: |diff| / bound =", diff / np.where(bound > 0, bound, 1.0))
    assert np.all(bound > 0.0) and np.all(diff <= bound), (diff, bound)
    e.close()
