"""The series of row sums on the device (beom_set_series, include/beom_hip.h) against the numpy restatement
(series_ref.row_record) applied to the state downloaded at the record's step.  Every comparison is helpers.same_bits: the
order of summation is the integrals' contract, so a dense handle, an embedded one, the table path and a frame cut into bands
(chain, chain with land, ring) give the same bits, whatever the division into calls.  No tolerance anywhere."""
import numpy as np
import pytest

import rough_inputs as RI
import series_ref as S
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import Golden, same_bits
from test_gpu_biharm_tiled import CASES
from test_gpu_integrals import _band_case, _case, _fields

pytestmark = pytest.mark.gpu
FIELDS = ("hlay", "u", "v", "h_u", "h_v")
_SINGLE = {}


def _rc(call):
    with pytest.raises(capi.BeomError) as ei:
        call()
    return str(ei.value)


def _refusal(call, code):
    """The whole message behind the `error <code>:` tag."""
    msg = _rc(call)
    tag = "beom_hip error %d: " % code
    assert msg.startswith(tag), msg
    return msg[len(tag):]


BAD_ARGS = "%s: level %d, stride %d, %d records (level 0..2, stride >= 1, records >= 1)"
OVERFLOW = ("%s: steps %d..%d would write %d records of the series (stride %d) but the recorder holds %d of %d: "
            "empty it with %s, or take fewer steps per call")
SAMPLE = "beom_sample_series (series set? recorder full?)"


def _series_of(e, calls, level, stride=1, records=16):
    e.set_series(level, stride, records)
    t = 1
    for n in calls:
        e.step(t, n)
        t += n
    return e.download_series()


# ---- 1. level 1 and 2 on each handle kind -------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ["jet_xyper_2l", "island_ragged_3l", "closed_12l", "wide_67_chunks"])
def test_records_on_each_handle_kind(name, level):
    f = _case(name)
    nl, M = f.p.nlay, f.p.mm + 1
    calls = (1,) if name == "wide_67_chunks" else (4, 2)         # (4201 columns: one record only)
    e, tab, twin = capi.Engine(f), capi.Engine(f, dense_hint=0), capi.Engine(f)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    a, b = _series_of(e, calls, level), _series_of(tab, calls, level)
    n = sum(calls)
    cnt = S.count(nl, level)
    assert cnt == e.lib.beom_series_count(nl, level)
    for got in (a, b):
        assert got["count"] == n and list(got["tstp"]) == list(range(1, n + 1)) and got["rows"].shape == (n, M, cnt)
    assert same_bits(a["rows"], b["rows"]), (name, level, "dense vs table path")
    for k in range(n):
        twin.step(k + 1, 1)
        want = S.row_record(f, twin.download(FIELDS), level)
        assert np.isfinite(want).all()
        assert same_bits(a["rows"][k], want), (name, level, k + 1)
        assert same_bits(a["raw"][k], twin.integrals()["raw"]), (name, level, k + 1)
        assert same_bits(a["rows"][k][:, :4 * nl + 1], twin.integral_rows(1, M)), (name, level, k + 1)
        assert same_bits(a["vol"][k], want[:, 0:4 * nl:4]) and same_bits(a["eta2"][k], want[:, 4 * nl])
        if level == 2:
            assert same_bits(a["tv"][k], want[:, 5 * nl + 1:]) and same_bits(a["psi"][k], S.psi(want, f.p))
    if level == 2:
        assert a["tu"][-1].any() and a["tv"][-1].any(), (name, "no transport anywhere: nothing tested")
    else:
        assert "tu" not in a and "psi" not in a
    e.close(); tab.close(); twin.close()


# ---- 2. the reference's own configurations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rigid_lid_sill_2l", "variant3d_3l", "biharm_island_2l", "obc_mcbc0_2l"])
def test_goldens_level_2(name):
    g = Golden(name)
    f = _fields(g)
    e = capi.Engine(f, variant=g.variant)
    e.set_series(2, 1, 5)
    want = []
    for t in range(1, 6):
        e.step(t, 1)
        want.append(S.row_record(f, e.download(FIELDS), 2))
    got = e.download_series()
    assert got["count"] == 5 and list(got["tstp"]) == [1, 2, 3, 4, 5]
    assert np.isfinite(got["rows"]).all()
    for k in range(5):
        assert same_bits(got["rows"][k], want[k]), (name, k + 1)
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
        assert same_bits(r["rows"], runs[0]["rows"])
    e = capi.Engine(f)
    r3 = _series_of(e, (5, 7), 2, stride=3)
    assert list(r3["tstp"]) == [3, 6, 9, 12]
    assert same_bits(r3["rows"], runs[0]["rows"][2::3])
    # the download has emptied the recorder
    assert e.info("series") == 2 and e.info("series_records") == 0
    again = e.download_series()
    assert again["count"] == 0 and again["rows"].shape[0] == 0 and again["tstp"].size == 0
    # one record by hand, under the last step's number, whatever the stride; an upload leaves it where it is
    e.sample_series()
    assert e.info("series_records") == 1
    e.upload(**e.download())
    assert e.info("series_records") == 1
    got = e.download_series()
    assert got["count"] == 1 and list(got["tstp"]) == [12]
    assert same_bits(got["rows"][0], runs[0]["rows"][11])
    # other arguments reallocate and empty; level 0 frees
    e.sample_series()
    e.set_series(1, 2, 3)
    assert e.info("series") == 1 and e.info("series_records") == 0
    e.step(13, 4)
    got = e.download_series()
    assert list(got["tstp"]) == [14, 16] and got["rows"].shape[2] == S.count(f.p.nlay, 1)
    e.set_series(0)
    assert e.info("series") == 0
    e.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    f = _case("island_ragged_3l")
    e = capi.Engine(f)
    assert _refusal(e.download_series, -3) == "beom_download_series: the handle keeps no series (beom_set_series)"
    assert _refusal(e.sample_series, -3) == SAMPLE
    for args in ((3, 1, 4), (-1, 1, 4), (1, 0, 4), (2, 1, 0)):
        assert _refusal(lambda: e.set_series(*args), -3) == BAD_ARGS % (("beom_set_series",) + args), args
    assert e.info("series") == 0
    e.step(1, 3)
    e.set_series(2, 1, 4)
    before = e.download(("hlay", "u", "v"))
    assert _refusal(lambda: e.step(4, 5), -3) == OVERFLOW % ("beom_step", 4, 8, 5, 1, 0, 4, "beom_download_series")
    after = e.download(("hlay", "u", "v"))
    for k in before:
        assert same_bits(before[k], after[k]), k
    assert e.info("series_records") == 0
    e.step(4, 4)
    assert e.info("series_records") == 4
    assert _refusal(e.sample_series, -3) == SAMPLE              # a full recorder
    assert _refusal(lambda: e.step(8, 1), -3) == OVERFLOW % ("beom_step", 8, 8, 1, 1, 4, 4, "beom_download_series")
    assert e.info("series_records") == 4
    got = e.download_series()
    assert list(got["tstp"]) == [4, 5, 6, 7]
    e.step(8, 1)                                                # the same step is taken once the recorder is empty
    assert list(e.download_series()["tstp"]) == [8]
    e.close()


def test_a_handle_that_holds_one_bands_window_refuses():
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    assert _refusal(lambda: band.set_series(2), -6) == (
        "beom_multi_set_series: a handle that holds one band's window keeps no series (its rows are nowhere assembled); "
        "use a handle created from the global arrays")
    band.close()


# ---- 5. a series changes nothing else -----------------------------------------------------------------------------------------
def test_a_series_leaves_the_state_as_it_was():
    f = _case("island_ragged_3l")
    plain, withs = capi.Engine(f), capi.Engine(f)
    withs.set_series(2, 1, 10)
    for x in (plain, withs):
        x.step(1, 4); x.step(5, 6)
    a, b = plain.download(), withs.download()
    for k in a:
        assert same_bits(a[k], b[k]), k
    assert withs.download_series()["count"] == 10
    plain.close(); withs.close()


# ---- 6. bands -----------------------------------------------------------------------------------------------------------------
def _band_fields(case):
    if case == "island_ragged_3l":                               # a frame with land: the bands' rows differ in length
        return _case(case)
    p, files = _band_case(case)
    return read_input_data(p, files=files)


def _single_handle_series(case):
    """The single handle's records of the banded cases (7 + 6 steps, stride 2, level 2), formed once."""
    if case not in _SINGLE:
        f = _band_fields(case)
        one = capi.Engine(f)
        got = _series_of(one, (7, 6), 2, stride=2, records=8)
        want = S.row_record(f, one.download(FIELDS), 2)          # (step 13 carries no record: the state is one step on)
        one.sample_series()
        assert same_bits(one.download_series()["rows"][0], want), case
        one.close()
        _SINGLE[case] = (f, got)
    return _SINGLE[case]


@pytest.mark.parametrize("nband", [2, 3])
@pytest.mark.parametrize("case", ["closed_12l", "sill_sponges", "jet_ring", "island_ragged_3l"])
def test_bands_give_the_single_handles_records(case, nband):
    f, want = _single_handle_series(case)
    assert list(want["tstp"]) == [2, 4, 6, 8, 10, 12] and np.isfinite(want["rows"]).all()
    many, plain = capi.MultiEngine(f, devices=[0] * nband), capi.MultiEngine(f, devices=[0] * nband)
    ring = int(float(f.p.yper) > 0.5)
    assert many.count == nband and many.describe()["ring"] == ring == int(case == "jet_ring")
    got = _series_of(many, (7, 6), 2, stride=2, records=8)
    plain.step(1, 7); plain.step(8, 6)
    assert list(got["tstp"]) == list(want["tstp"])
    assert same_bits(got["rows"], want["rows"]), (case, nband)
    assert same_bits(got["raw"], want["raw"])
    if ring:
        last = got["rows"][:, f.p.mm]
        assert not last.any() and not np.signbit(last).any()
    assert many.stats() == plain.stats(), (case, nband, many.stats(), plain.stats())
    a, b = many.download(FIELDS), plain.download(FIELDS)
    for k in a:
        assert same_bits(a[k], b[k]), (case, nband, k)
    # the recorder is empty again, and a call that would overflow it is refused before anything is launched
    assert many.download_series()["count"] == 0
    many.set_series(2, 1, 3)
    assert _refusal(lambda: many.step(14, 4), -3) == OVERFLOW % ("beom_multi_step", 14, 17, 4, 1, 0, 3, "beom_multi_download_series")
    many.step(14, 3)
    assert list(many.download_series()["tstp"]) == [14, 15, 16]
    # a handle without a series says so, and bad arguments are refused in the bands' own words
    assert _refusal(plain.download_series, -3) == "beom_multi_download_series: the handle keeps no series (beom_multi_set_series)"
    assert _refusal(lambda: plain.set_series(3, 1, 4), -3) == BAD_ARGS % ("beom_multi_set_series", 3, 1, 4)
    many.close(); plain.close()


# ---- 7. liveness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["island_ragged_3l", "jet_xyper_2l"])
def test_rough_transports_are_live(config):
    """The rough h_u, h_v as uploaded (no step): every layer's tu, tv is non-zero and differs between neighbouring rows, and a
    restatement that swaps h_u and h_v fails the comparison.  jet_xyper_2l: values put into the duplicated column and row
    (the steps leave +0 there) contribute +0.0."""
    g = RI.rough_fields(RI.base_fields(config, "130x18"), 1)
    p, nl = g.p, g.p.nlay
    if config == "jet_xyper_2l":
        dup = (g.subc[0] == p.lm + 1) | (g.subc[1] == p.mm + 1)
        dup[0] = False
        g.h_u = np.where(dup[None, :], 1.5, g.h_u)
        g.h_v = np.where(dup[None, :], -2.5, g.h_v)
    for dense_hint in (1, 0):
        e = capi.Engine(g, dense_hint=dense_hint)
        e.set_series(2, 1, 1)
        e.sample_series()
        got = e.download_series()
        st = e.download(FIELDS)
        assert same_bits(st["h_u"], g.h_u) and same_bits(st["h_v"], g.h_v)
        assert list(got["tstp"]) == [0]
        assert same_bits(got["rows"][0], S.row_record(g, st, 2)), (config, dense_hint)
        assert not same_bits(got["rows"][0], S.row_record(g, dict(st, h_u=st["h_v"], h_v=st["h_u"]), 2))
        for t in (got["tu"][0], got["tv"][0]):
            assert np.all(t[1:p.mm] != 0.0)
            assert np.all(t[2:p.mm] != t[1:p.mm - 1])
        if config == "jet_xyper_2l":
            assert not got["rows"][0][p.mm].any() and not np.signbit(got["rows"][0][p.mm]).any()
        e.close()
