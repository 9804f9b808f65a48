"""The column series on the device (beom_set_column_series, include/beom_hip.h) against the numpy restatement
(column_series_ref.column_record) applied to the state downloaded at the record's step.  Every comparison with the restatement
is helpers.same_bits: the order of summation (the pairwise tree over the aligned global row index) is the contract, so a dense
handle, an embedded one and the table path give the same bits, whatever the division into calls, the row window's place or
the batches of column chunks.  The only tolerance is the cross-check against integrals(), which adds in another order."""
import numpy as np
import pytest

import column_series_ref as CS
import rough_inputs as RI
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import Golden, same_bits
from test_gpu_biharm_tiled import CASES
from test_gpu_integrals import _case as _integrals_case, _fields
from test_gpu_series import _refusal
from test_gpu_tracer_series import _with_tracers

pytestmark = pytest.mark.gpu
FIELDS = ("hlay", "u", "v", "h_u", "h_v")

BAD_ARGS = "beom_set_column_series: level %d, stride %d, %d records (level 0..2, stride >= 1, records >= 1)"
BAD_ROWS = "beom_set_column_series: rows %d..%d outside 1..%d"
OVERFLOW = ("beom_step: steps %d..%d would write %d records of the column series (stride %d) but the recorder holds %d of %d: "
            "empty it with beom_download_column_series, or take fewer steps per call")
NONE = "beom_download_column_series: the handle keeps no column series (beom_set_column_series)"
SAMPLE = "beom_sample_column_series (column series set? recorder full?)"
ON_BANDS = ("%s: a handle on bands keeps no column series (a column's tree over the global rows crosses the bands, "
            "and nothing combines the bands' tree nodes yet); use a single handle (beom_set_column_series)")


def _case(name):
    if name == "tall_4201_rows":                        # 10 columns x 4201 rows: the tree padded to 8192, 54 idle lanes
        p, files = I.case_headline(9, 4200, 2)
        return read_input_data(p.replace(svis="0."), files=files)
    return _integrals_case(name)


def _series_of(e, calls, level, stride=1, records=16, rows=None):
    e.set_column_series(level, stride, records, rows)
    t = 1
    for n in calls:
        e.step(t, n)
        t += n
    return e.download_column_series()


# ---- 1. level 1 and 2 on each handle kind -------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ["jet_xyper_2l", "island_ragged_3l", "closed_12l", "wide_67_chunks", "tall_4201_rows",
                                  "soliton_xper"])
def test_records_on_each_handle_kind(name, level):
    f = _case(name)
    nl, L = f.p.nlay, f.p.lm + 1
    calls = (1,) if name == "wide_67_chunks" else (4, 2)
    e, tab, twin = capi.Engine(f), capi.Engine(f, dense_hint=0), capi.Engine(f)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    a, b = _series_of(e, calls, level), _series_of(tab, calls, level)
    n = sum(calls)
    cnt = CS.count(nl, level)
    assert cnt == e.lib.beom_series_count(nl, level)
    for got in (a, b):
        assert got["count"] == n and list(got["tstp"]) == list(range(1, n + 1)) and got["cols"].shape == (n, L, cnt)
    assert same_bits(a["cols"], b["cols"]), (name, level, "dense vs table path")
    for k in range(n):
        twin.step(k + 1, 1)
        want = CS.column_record(f, twin.download(FIELDS), level)
        assert np.isfinite(want).all()
        assert same_bits(a["cols"][k], want), (name, level, k + 1)
        assert same_bits(a["total"][k], CS.total(want, nl)), (name, level, k + 1)
        assert same_bits(a["vol"][k], want[:, 0:4 * nl:4]) and same_bits(a["ke"][k], want[:, 1:4 * nl:4])
        assert same_bits(a["ens"][k], want[:, 2:4 * nl:4]) and same_bits(a["circ"][k], want[:, 3:4 * nl:4])
        assert same_bits(a["eta2"][k], want[:, 4 * nl])
        if level == 2:
            assert same_bits(a["tu"][k], want[:, 4 * nl + 1:5 * nl + 1]) and same_bits(a["tv"][k], want[:, 5 * nl + 1:])
            assert same_bits(a["phi"][k], CS.phi(want, f.p))
    if level == 2:
        assert a["tu"][-1].any() and a["tv"][-1].any(), (name, "no transport anywhere: nothing tested")
    else:
        assert "tu" not in a and "phi" not in a
    assert a["vol"][-1].any() and a["ke"][-1].any()
    e.close(); tab.close(); twin.close()


# ---- 2. the reference's own configurations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rigid_lid_sill_2l", "variant3d_3l", "biharm_island_2l", "obc_mcbc0_2l"])
def test_goldens_level_2(name):
    g = Golden(name)
    f = _fields(g)
    e = capi.Engine(f, variant=g.variant)
    e.set_column_series(2, 1, 5)
    want = []
    for t in range(1, 6):
        e.step(t, 1)
        want.append(CS.column_record(f, e.download(FIELDS), 2))
    got = e.download_column_series()
    assert got["count"] == 5 and list(got["tstp"]) == [1, 2, 3, 4, 5]
    assert np.isfinite(got["cols"]).all()
    for k in range(5):
        assert same_bits(got["cols"][k], want[k]), (name, k + 1)
    assert got["tv"].any() and got["tu"].any(), (name, "no transport anywhere: nothing tested")
    e.close()


# ---- 3. division into calls, stride, the entry by hand ------------------------------------------------------------------------
def test_division_into_calls_and_stride():
    f = _case("jet_xyper_2l")
    runs = []
    for calls in ((12,), (5, 7), (1,) * 12):
        e = capi.Engine(f)
        runs.append(_series_of(e, calls, 2))
        e.close()
    for r in runs:
        assert list(r["tstp"]) == list(range(1, 13))
        assert same_bits(r["cols"], runs[0]["cols"])
    e = capi.Engine(f)
    r3 = _series_of(e, (5, 7), 2, stride=3)
    assert list(r3["tstp"]) == [3, 6, 9, 12]
    assert same_bits(r3["cols"], runs[0]["cols"][2::3])
    # the download has emptied the recorder
    assert e.info("column_series") == 2 and e.info("column_series_records") == 0
    again = e.download_column_series()
    assert again["count"] == 0 and again["cols"].shape[0] == 0 and again["tstp"].size == 0
    # one record by hand, under the last step's number, whatever the stride; an upload leaves it where it is
    e.sample_column_series()
    assert e.info("column_series_records") == 1
    e.upload(**e.download())
    assert e.info("column_series_records") == 1
    got = e.download_column_series()
    assert got["count"] == 1 and list(got["tstp"]) == [12]
    assert same_bits(got["cols"][0], runs[0]["cols"][11])
    # other arguments reallocate and empty; level 0 frees
    e.sample_column_series()
    e.set_column_series(1, 2, 3)
    assert e.info("column_series") == 1 and e.info("column_series_records") == 0
    e.step(13, 4)
    got = e.download_column_series()
    assert list(got["tstp"]) == [14, 16] and got["cols"].shape[2] == CS.count(f.p.nlay, 1)
    e.set_column_series(0)
    assert e.info("column_series") == 0
    assert _refusal(e.download_column_series, -3) == NONE
    e.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    f = _case("island_ragged_3l")
    M = f.p.mm + 1
    e = capi.Engine(f)
    assert _refusal(e.download_column_series, -3) == NONE
    assert _refusal(e.sample_column_series, -3) == SAMPLE
    for args in ((3, 1, 4), (-1, 1, 4), (1, 0, 4), (2, 1, 0)):
        assert _refusal(lambda: e.set_column_series(*args), -3) == BAD_ARGS % args, args
    for rows in ((0, 5), (5, 4), (1, M + 1), (M + 1, M + 1)):
        assert _refusal(lambda: e.set_column_series(2, 1, 4, rows), -3) == BAD_ROWS % (rows + (M,)), rows
    assert e.info("column_series") == 0
    e.step(1, 3)
    e.set_column_series(2, 1, 4)
    before = e.download(("hlay", "u", "v"))
    assert _refusal(lambda: e.step(4, 5), -3) == OVERFLOW % (4, 8, 5, 1, 0, 4)
    after = e.download(("hlay", "u", "v"))
    for k in before:
        assert same_bits(before[k], after[k]), k
    assert e.info("column_series_records") == 0
    e.step(4, 4)
    assert e.info("column_series_records") == 4
    assert _refusal(e.sample_column_series, -3) == SAMPLE       # a full recorder
    assert _refusal(lambda: e.step(8, 1), -3) == OVERFLOW % (8, 8, 1, 1, 4, 4)
    assert e.info("column_series_records") == 4
    got = e.download_column_series()
    assert list(got["tstp"]) == [4, 5, 6, 7]
    e.step(8, 1)                                                # the same step is taken once the recorder is empty
    assert list(e.download_column_series()["tstp"]) == [8]
    e.close()


def test_handles_on_bands_refuse():
    from beom_amd import slab
    f = _case("closed_12l")
    many = capi.MultiEngine(f, devices=[0, 0])
    assert _refusal(lambda: many.set_column_series(2), -6) == ON_BANDS % "beom_multi_set_column_series"
    assert _refusal(many.download_column_series, -6) == ON_BANDS % "beom_multi_download_column_series"
    many.close()
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    assert _refusal(lambda: band.set_column_series(2), -6) == ON_BANDS % "beom_multi_set_column_series"
    band.close()


# ---- 5. the recorders together ------------------------------------------------------------------------------------------------
def test_recorders_together_and_the_state():
    """One handle with the series, the column series, the tracer series and integrals() between the steps: each recorder's
    records are those of a handle that keeps it alone, and the state is that of a handle with no recorder."""
    f = _case("island_ragged_3l")
    names = ("all", "series", "column", "tracer", "plain")
    h = {k: _with_tracers(capi.Engine(f), f, 2) for k in names}
    for k in ("all", "series"):
        h[k].set_series(2, 1, 8)
    for k in ("all", "column"):
        h[k].set_column_series(2, 1, 8)
    for k in ("all", "tracer"):
        h[k].set_tracer_series(2, 1, 8)
    for calls in ((1, 3), (4, 4)):
        for e in h.values():
            e.step(*calls)
        h["all"].integrals()
    a = h["all"]
    got = a.download_column_series()
    assert got["count"] == 7 and same_bits(got["cols"], h["column"].download_column_series()["cols"])
    assert same_bits(got["cols"][-1], CS.column_record(f, a.download(FIELDS), 2))
    assert same_bits(a.download_series()["rows"], h["series"].download_series()["rows"])
    assert same_bits(a.download_tracer_series()["rows"], h["tracer"].download_tracer_series()["rows"])
    sa, sp = a.download(), h["plain"].download()
    for k in sa:
        assert same_bits(sa[k], sp[k]), k
    assert same_bits(a.download_tracers()["q"], h["plain"].download_tracers()["q"])
    for e in h.values():
        e.close()


# ---- 6. the row window --------------------------------------------------------------------------------------------------------
def test_row_window():
    f = _case("island_ragged_3l")
    M = f.p.mm + 1
    assert M == 71
    e = capi.Engine(f)
    e.step(1, 3)
    st = e.download(FIELDS)
    recs = {}
    for rows in (None, (1, M), (20, 41), (71, 71)):
        for dense_hint in (1, 0):
            x = capi.Engine(f, dense_hint=dense_hint)
            x.upload(**e.download())
            x.set_column_series(2, 1, 1, rows)
            x.sample_column_series()
            got = x.download_column_series()["cols"][0]
            assert same_bits(got, CS.column_record(f, st, 2, rows)), (rows, dense_hint)
            recs[rows] = got
            x.close()
    assert same_bits(recs[(1, M)], recs[None])
    assert not same_bits(recs[(20, 41)], recs[None]) and recs[(20, 41)].any()
    e.close()


# ---- 7. batches ---------------------------------------------------------------------------------------------------------------
def test_batches_of_one_chunk_give_the_same_bits():
    f = _case("wide_67_chunks")
    a, b = capi.Engine(f), capi.Engine(f)
    b.set_option("column_series_batch", 1)
    ra, rb = _series_of(a, (1,), 2), _series_of(b, (1,), 2)
    assert ra["cols"].shape[1] == 4201 and ra["tu"].any()
    assert same_bits(ra["cols"], rb["cols"])
    a.close(); b.close()


# ---- 8. liveness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["island_ragged_3l", "jet_xyper_2l"])
def test_rough_transports_are_live(config):
    """The rough h_u, h_v as uploaded (no step): the record equals the restatement and differs from one with h_u and h_v
    swapped.  jet_xyper_2l: every interior column's tu, tv is non-zero and differs from its neighbour's, and values put into
    the duplicated column and row (the steps leave +0 there) contribute +0.0."""
    g = RI.rough_fields(RI.base_fields(config, "130x18"), 1)
    p, nl = g.p, g.p.nlay
    if config == "jet_xyper_2l":
        dup = (g.subc[0] == p.lm + 1) | (g.subc[1] == p.mm + 1)
        dup[0] = False
        g.h_u = np.where(dup[None, :], 1.5, g.h_u)
        g.h_v = np.where(dup[None, :], -2.5, g.h_v)
    for dense_hint in (1, 0):
        e = capi.Engine(g, dense_hint=dense_hint)
        e.set_column_series(2, 1, 1)
        e.sample_column_series()
        got = e.download_column_series()
        st = e.download(FIELDS)
        assert same_bits(st["h_u"], g.h_u) and same_bits(st["h_v"], g.h_v)
        assert list(got["tstp"]) == [0]
        assert same_bits(got["cols"][0], CS.column_record(g, st, 2)), (config, dense_hint)
        assert not same_bits(got["cols"][0], CS.column_record(g, dict(st, h_u=st["h_v"], h_v=st["h_u"]), 2))
        assert got["tu"][0].any() and got["tv"][0].any()
        if config == "jet_xyper_2l":                            # (no land, no wall: every interior column carries transport)
            for t in (got["tu"][0], got["tv"][0]):
                assert np.all(t[1:p.lm] != 0.0)
                assert np.all(t[2:p.lm] != t[1:p.lm - 1])
            assert not got["cols"][0][p.lm].any() and not np.signbit(got["cols"][0][p.lm]).any()
            clean = dict(st, h_u=np.where(dup[None, :], 0.0, st["h_u"]), h_v=np.where(dup[None, :], 0.0, st["h_v"]))
            assert same_bits(got["cols"][0], CS.column_record(g, clean, 2))
        e.close()


# ---- 9. the cross-check with the integrals ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["island_ragged_3l", "jet_xyper_2l"])
def test_total_is_within_the_bound_of_the_integrals(name):
    """total adds along columns first, integrals() along rows first: two pairwise trees over the same terms, each entry within
    2 * gamma_D * sum |T_k| (column_series_ref.gamma_bound)."""
    f = _case(name)
    e = capi.Engine(f)
    got = _series_of(e, (5,), 1, stride=5)
    raw = e.integrals()["raw"]
    bound = CS.gamma_bound(f, e.download(FIELDS))
    diff = np.abs(got["total"][0] - raw)
    print("total vs integrals: |diff| / bound =", diff / np.where(bound > 0, bound, 1.0))
    assert np.all(diff <= bound), (diff, bound)
    e.close()
