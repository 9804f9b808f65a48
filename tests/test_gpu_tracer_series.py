"""The tracer series on the device (beom_set_tracer_series, include/beom_hip.h) against the numpy restatement
(tracer_series_ref, tied to series_ref and integrals_ref by test_tracer_series_cpu) applied to the state and tracers downloaded
at the record's step.  Every comparison is helpers.same_bits: the order of summation is the integrals' contract and the bounds
see no signed zero, so a dense handle, an embedded one, the table path and a frame cut into bands give the same bits, whatever
the division into calls or into launches.  No tolerance anywhere."""
import numpy as np
import pytest

import tracer_series_ref as TS
import tracers_ref as T
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, same_bits
from test_gpu_biharm_tiled import CASES
from test_gpu_integrals import _case
from test_gpu_tracer_moments import _band_frame
from test_tracer_series_cpu import rough_case

pytestmark = pytest.mark.gpu
HQ = ("hlay", "h_u", "h_v")
FIELDS = ("hlay", "u", "v", "h_u", "h_v")


def _rc(call):
    with pytest.raises(capi.BeomError) as ei:
        call()
    return str(ei.value)


def _refused(call, code, what):
    msg = _rc(call)
    tag = "error %d:" % code
    assert tag in msg and len(msg.split(tag)[1].strip()) > 20, (what, msg)


def _refusal(call, code):
    """The whole message behind the `error <code>:` tag."""
    msg = _rc(call)
    tag = "beom_hip error %d: " % code
    assert msg.startswith(tag), msg
    return msg[len(tag):]


BAD_ARGS = "%s: level %d, stride %d, %d records (level 0..3, stride >= 1, records >= 1)"
OVERFLOW = ("%s: steps %d..%d would write %d records of the tracer series (stride %d) but the recorder holds %d of %d: "
            "empty it with %s, or take fewer steps per call")
SAMPLE = "beom_sample_tracer_series (tracer series set? recorder full?)"
NONE = "beom_download_tracer_series: the handle keeps no tracer series (beom_set_tracer_series)"
NO_TRACER = "beom_set_tracer_series: the handle carries no tracer (beom_set_tracers comes first)"
RING = "%s: bands of a frame periodic in y do not carry tracers (the ring's companion frame has no q); use a single handle"
WINDOW = "%s: a handle that holds one band's window does not carry tracers (its exchange is sized at creation)"


def _contents(f, ntrc):
    """q, rq, ctrg of ntrc tracers on the frame's own thicknesses: patches of 5 x 4 cells with other values per tracer, the
    lower one negative for every second tracer; a relaxation concentration that varies from cell to cell."""
    p = f.p
    h = np.asarray(f.hlay, dtype=np.float64)
    c = np.stack([T.patchy(f, low=(-0.3 if t % 2 else 0.2) + 0.05 * t, high=1.0 + 0.15 * t) for t in range(ntrc)])
    i, j = f.subc[0].astype(np.float64), f.subc[1].astype(np.float64)
    ctrg = np.stack([np.broadcast_to(0.4 + 0.3 * np.sin(0.37 * i + 0.1 * t) * np.cos(0.23 * j), h.shape) for t in range(ntrc)])
    q = c * h[None]
    return np.ascontiguousarray(q), np.zeros(q.shape + (2,)), np.ascontiguousarray(ctrg)


def _with_tracers(e, f, ntrc):
    q, rq, ctrg = _contents(f, ntrc)
    e.set_tracers(ntrc)
    e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    return e


def _series_of(e, calls, level, stride=1, records=16):
    e.set_tracer_series(level, stride, records)
    t = 1
    for n in calls:
        e.step(t, n)
        t += n
    return e.download_tracer_series()


def _restated(f, e, level):
    st = e.download(HQ)
    return TS.row_record(f, st["hlay"], st["h_u"], st["h_v"], e.download_tracers()["q"], level)


def _same_views(got, want, ntrc, nl, level, p, what):
    v = TS.views(want, ntrc, nl, level)
    for k in TS.NAMES[:2 * level]:
        assert same_bits(got[k], v[k]), (what, k)
    for k in TS.NAMES[2 * level:] + ("transport",) * (level < 2):
        assert k not in got, (what, k)
    assert same_bits(got["total"], TS.total(want, ntrc, nl, level)), (what, "total")
    if level >= 2:
        assert same_bits(got["transport"], float(p.dl) * v["fv"]), (what, "transport")


# ---- 1. every level on each handle kind ---------------------------------------------------------------------------------------
_TWIN = {}


def _twin_states(name, ntrc, nsteps):
    """hlay, h_u, h_v and q of a twin handle behind each of its first steps, downloaded once per frame and tracer count."""
    key = (name, ntrc)
    if key not in _TWIN:
        f = _case(name)
        twin = _with_tracers(capi.Engine(f), f, ntrc)
        out = []
        for t in range(1, nsteps + 1):
            twin.step(t, 1)
            out.append((twin.download(HQ), twin.download_tracers()["q"]))
        twin.close()
        _TWIN[key] = (f, out)
    return _TWIN[key]


def _records_on_each_handle_kind(name, level, ntrc):
    calls = (1,) if name == "wide_67_chunks" else (4, 2)         # (4201 columns: one record only)
    n = sum(calls)
    f, states = _twin_states(name, ntrc, n)
    nl, M = f.p.nlay, f.p.mm + 1
    e, tab = _with_tracers(capi.Engine(f), f, ntrc), _with_tracers(capi.Engine(f, dense_hint=0), f, ntrc)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    a, b = _series_of(e, calls, level), _series_of(tab, calls, level)
    cnt = TS.count(ntrc, nl, level)
    assert cnt == e.lib.beom_tracer_series_count(ntrc, nl, level)
    for got in (a, b):
        assert got["count"] == n and list(got["tstp"]) == list(range(1, n + 1)) and got["rows"].shape == (n, M, cnt)
    assert same_bits(a["rows"], b["rows"]), (name, level, ntrc, "dense vs table path")
    for k, (st, q) in enumerate(states):
        want = TS.row_record(f, st["hlay"], st["h_u"], st["h_v"], q, level)
        assert not np.isnan(want).any()
        assert same_bits(a["rows"][k], want), (name, level, ntrc, k + 1)
    want = np.stack([TS.row_record(f, st["hlay"], st["h_u"], st["h_v"], q, level) for st, q in states])
    _same_views(a, want, ntrc, nl, level, f.p, (name, level, ntrc))
    assert np.all(a["inv"][-1].any(axis=0)) and np.all(a["var"][-1].any(axis=0)), (name, "an empty tracer-layer: nothing tested")
    if level >= 2:
        assert a["fu"][-1].any() and a["fv"][-1].any(), (name, "no flux anywhere: nothing tested")
    if level >= 3:
        wet_rows = np.isfinite(a["cmin"][-1])
        assert wet_rows.any() and np.all(a["cmin"][-1][wet_rows] <= a["cmax"][-1][wet_rows])
        assert np.any(a["cmin"][-1][wet_rows] < a["cmax"][-1][wet_rows])
    e.close(); tab.close()


@pytest.mark.parametrize("ntrc", [1, 3])
@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("name", ["jet_xyper_2l", "island_ragged_3l", "closed_12l", "wide_67_chunks"])
def test_records_on_each_handle_kind(name, level, ntrc):
    _records_on_each_handle_kind(name, level, ntrc)


def test_eight_tracers_at_level_3():
    _records_on_each_handle_kind("jet_xyper_2l", 3, 8)


# ---- 2. rough contents by hand: negative and -0 concentrations, dry cells, rows of launches ---------------------------------------
@pytest.mark.parametrize("config", ["island_ragged_3l", "jet_xyper_2l"])
def test_rough_contents_by_hand(config):
    """The rough state and tracers of test_tracer_series_cpu.rough_case as uploaded (no step): concentrations below zero and of
    -0, dry cell-layers with a stranded content, a row whose maximum is a zero.  Every level, dense and table path; and the
    same record taken four rows per launch (option "tracer_series_batch")."""
    g, st, q = rough_case(config)
    p, nl, ntrc = g.p, g.p.nlay, q.shape[0]
    want = {level: TS.row_record(g, st["hlay"], st["h_u"], st["h_v"], q, level) for level in (1, 2, 3)}
    for dense_hint in (1, 0):
        e = capi.Engine(g, dense_hint=dense_hint)
        e.set_tracers(ntrc)
        e.upload(**st)
        e.upload_tracers(q=q)
        for batch in (0, 4):
            e.set_option("tracer_series_batch", batch)
            for level in (1, 2, 3):
                e.set_tracer_series(level, 1, 1)
                e.sample_tracer_series()
                got = e.download_tracer_series()
                assert list(got["tstp"]) == [0]
                assert same_bits(got["rows"][0], want[level]), (config, dense_hint, batch, level)
        top = got["cmax"][0, 4, 0, 0]                             # row 5, tracer 0, layer 1: the maximum is +0
        assert top == 0.0 and not np.signbit(top)
        swapped = TS.row_record(g, st["hlay"], st["h_v"], st["h_u"], q, 3)
        assert not same_bits(got["fu"][0], TS.views(swapped, ntrc, nl, 3)["fu"])
        e.close()


@pytest.mark.parametrize("lm,xper", [(1, False), (1, True), (2, False)])
def test_frames_narrower_than_four_columns(lm, xper):
    """lm = 1: rows of two columns, the tree's width is 2, so the four sums of a tracer-layer go through integral_wave_tree one
    by one (width < 4) and a level-1 pair through integral_wave_tree2; periodic in x the second column is the duplicate and a
    row is one live cell.  lm = 2: three columns, width 4.  By hand on uploaded contents, no step."""
    p, files = I.case_unstable_jet(lm=lm, mm=9, nlay=2, dt_s=1.5) if xper else I.case_headline(lm, 9, 2)
    f = read_input_data(p, files=files)
    assert f.p.lm + 1 == lm + 1 < 4 and (float(f.p.xper) > 0.5) == xper
    r = np.random.default_rng([lm, int(xper), 77])
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
            e.set_tracer_series(level, 1, 1)
            e.sample_tracer_series()
            got = e.download_tracer_series()
            want = TS.row_record(f, h, st["h_u"], st["h_v"], q, level)
            assert same_bits(got["rows"][0], want), (lm, xper, dense_hint, level)
        assert got["inv"].any() and got["fv"].any()
        e.close()


# ---- 3. both schemes, with lateral and vertical mixing ------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [1, 2])
def test_both_schemes_with_mixing(scheme):
    """The record reads the final arrays only: whatever advected and mixed the tracers, it equals the restatement on the
    downloads.  Under scheme 2 the faces are still the upstream ones."""
    f = _case("island_ragged_3l")
    p, nl, ntrc = f.p, f.p.nlay, 3
    e = _with_tracers(capi.Engine(f), f, ntrc)
    e.set_tracer_scheme(scheme)
    e.set_tracer_mixing(kappa=0.2 * float(p.dl) ** 2 / float(p.dt), decay=0.02 / float(p.dt))
    e.set_tracer_vertical_mixing(1.0e-3)
    e.set_tracer_series(3, 1, 4)
    want = []
    for t in range(1, 5):
        e.step(t, 1)
        want.append(_restated(f, e, 3))
    got = e.download_tracer_series()
    assert e.info("tracer_scheme") == scheme and e.info("tracer_mix_launches") == 4 and e.info("tracer_vmix_launches") == 4
    assert list(got["tstp"]) == [1, 2, 3, 4]
    for k in range(4):
        assert same_bits(got["rows"][k], want[k]), (scheme, k + 1)
    assert not same_bits(got["rows"][3], got["rows"][0])
    e.close()


@pytest.mark.parametrize("name", ["biharm_island_2l", "obc_mcbc0_2l", "tc_wave_sponge"])
def test_goldens_level_3(name):
    """The reference's own configurations that carry tracers: svis > 0, an open boundary whose transports enter from outside
    the frame (the upwind cell of those faces is the sentinel, which is dry), sponges."""
    from helpers import Golden
    from test_gpu_integrals import _fields
    g = Golden(name)
    f = _fields(g)
    e = _with_tracers(capi.Engine(f, variant=g.variant), f, 2)
    e.set_tracer_series(3, 1, 5)
    want = []
    for t in range(1, 6):
        e.step(t, 1)
        want.append(_restated(f, e, 3))
    got = e.download_tracer_series()
    assert got["count"] == 5 and list(got["tstp"]) == [1, 2, 3, 4, 5]
    for k in range(5):
        assert same_bits(got["rows"][k], want[k]), (name, k + 1)
    assert got["fu"].any() and got["fv"].any(), (name, "no flux anywhere: nothing tested")
    e.close()


# ---- 4. the unit tracer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jet_xyper_2l", "island_ragged_3l"])
def test_the_unit_tracer_carries_the_series_transports(name):
    """Concentration 1 (and the thickness' own history, relaxation concentration 1): q stays hlay bit for bit, so fu, fv are
    the series' tu, tv at every step, inv = var, and the bounds are 1.0 on every row with a wet cell."""
    f = _case(name)
    nl = f.p.nlay
    e = capi.Engine(f)
    e.set_tracers(1)
    q = e.set_concentration(1.0)
    e.upload_tracers(rq=np.ascontiguousarray(np.asarray(f.rs_h, dtype=np.float64)[None]), ctrg=np.ones_like(q))
    e.set_series(2, 1, 8)
    e.set_tracer_series(3, 1, 8)
    e.step(1, 4); e.step(5, 2)
    ser, trc = e.download_series(), e.download_tracer_series()
    assert list(ser["tstp"]) == list(trc["tstp"]) == [1, 2, 3, 4, 5, 6]
    assert same_bits(e.download_tracers()["q"][0][:, 1:], e.download(("hlay",))["hlay"][:, 1:]), name
    assert same_bits(trc["fu"][:, :, 0], ser["tu"]) and same_bits(trc["fv"][:, :, 0], ser["tv"]), name
    assert ser["tu"][-1].any() and ser["tv"][-1].any(), (name, "no transport anywhere: nothing tested")
    assert same_bits(trc["inv"], trc["var"]), name
    wet_rows = np.isfinite(trc["cmin"])
    assert wet_rows.any() and np.all(trc["cmin"][wet_rows] == 1.0) and np.all(trc["cmax"][wet_rows] == 1.0), name
    assert np.all(trc["cmin"][~wet_rows] == np.inf) and np.all(trc["cmax"][~wet_rows] == -np.inf)
    assert np.all(trc["inv"][wet_rows] > 0.0) and not trc["inv"][~wet_rows].any()
    e.close()


# ---- 5. division into calls, stride, the entry by hand ------------------------------------------------------------------------
def test_division_into_calls_and_stride():
    f = _case("jet_xyper_2l")
    nl, ntrc = f.p.nlay, 3
    runs = []
    for calls in ((12,), (5, 7), (1,) * 12):
        e = _with_tracers(capi.Engine(f), f, ntrc)
        runs.append(_series_of(e, calls, 3))
        e.close()
    for r in runs:
        assert list(r["tstp"]) == list(range(1, 13))
        assert same_bits(r["rows"], runs[0]["rows"])
    e = _with_tracers(capi.Engine(f), f, ntrc)
    r3 = _series_of(e, (5, 7), 3, stride=3)
    assert list(r3["tstp"]) == [3, 6, 9, 12]
    assert same_bits(r3["rows"], runs[0]["rows"][2::3])
    # the download has emptied the recorder
    assert e.info("tracer_series") == 3 and e.info("tracer_series_records") == 0
    again = e.download_tracer_series()
    assert again["count"] == 0 and again["rows"].shape[0] == 0 and again["tstp"].size == 0
    # one record by hand, under the last step's number, whatever the stride; uploads leave it where it is
    e.sample_tracer_series()
    assert e.info("tracer_series_records") == 1
    e.upload(**e.download())
    tr = e.download_tracers()
    e.upload_tracers(q=tr["q"], rq=tr["rq"])
    assert e.info("tracer_series_records") == 1
    got = e.download_tracer_series()
    assert got["count"] == 1 and list(got["tstp"]) == [12]
    assert same_bits(got["rows"][0], runs[0]["rows"][11])
    # other arguments reallocate and empty; the same tracer count keeps the recorder, another one frees it; level 0 frees
    e.sample_tracer_series()
    e.set_tracer_series(1, 2, 3)
    assert e.info("tracer_series") == 1 and e.info("tracer_series_records") == 0
    e.step(13, 4)
    e.set_tracers(ntrc)
    assert e.info("tracer_series") == 1
    e.set_tracers(2)
    assert e.info("tracer_series") == 0 and e.info("tracer_series_records") == 0
    assert "-3" in _rc(e.download_tracer_series)
    e.set_tracer_series(2, 1, 2)
    assert e.download_tracer_series()["rows"].shape == (0, f.p.mm + 1, TS.count(2, nl, 2))
    e.set_tracer_series(0)
    assert e.info("tracer_series") == 0
    e.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    f = _case("island_ragged_3l")
    e = capi.Engine(f)
    assert _refusal(lambda: e.set_tracer_series(1), -3) == NO_TRACER
    assert _refusal(e.download_tracer_series, -3) == NONE and _refusal(e.sample_tracer_series, -3) == SAMPLE
    _with_tracers(e, f, 2)
    assert _refusal(e.download_tracer_series, -3) == NONE       # no tracer series yet
    assert _refusal(e.sample_tracer_series, -3) == SAMPLE
    for args in ((4, 1, 4), (-1, 1, 4), (1, 0, 4), (2, 1, 0)):
        assert _refusal(lambda: e.set_tracer_series(*args), -3) == BAD_ARGS % (("beom_set_tracer_series",) + args), args
    assert e.info("tracer_series") == 0
    e.step(1, 3)
    e.set_tracer_series(3, 1, 4)
    before, qb = e.download(STATE), e.download_tracers()
    assert _refusal(lambda: e.step(4, 5), -3) == OVERFLOW % ("beom_step", 4, 8, 5, 1, 0, 4, "beom_download_tracer_series")
    after, qa = e.download(STATE), e.download_tracers()
    for k in before:
        assert same_bits(before[k], after[k]), k
    assert same_bits(qb["q"], qa["q"]) and same_bits(qb["rq"], qa["rq"])
    assert e.info("tracer_series_records") == 0
    e.step(4, 4)
    assert e.info("tracer_series_records") == 4
    assert _refusal(e.sample_tracer_series, -3) == SAMPLE       # a full recorder
    assert _refusal(lambda: e.step(8, 1), -3) == OVERFLOW % ("beom_step", 8, 8, 1, 1, 4, 4, "beom_download_tracer_series")
    assert e.info("tracer_series_records") == 4
    assert list(e.download_tracer_series()["tstp"]) == [4, 5, 6, 7]
    e.step(8, 1)                                                # the same step is taken once the recorder is empty
    assert list(e.download_tracer_series()["tstp"]) == [8]
    e.close()


def test_handles_that_carry_no_tracers_refuse():
    # bands of a frame periodic in y, and a handle that holds one band's window: neither carries tracers
    ring = capi.MultiEngine(_band_frame("jet_xyper_2l"), devices=(0, 0))
    assert ring.describe()["ring"] == 1
    assert _refusal(lambda: ring.set_tracer_series(1), -6) == RING % "beom_multi_set_tracer_series"
    assert _refusal(ring.download_tracer_series, -6) == RING % "beom_multi_download_tracer_series"
    ring.close()
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    assert _refusal(lambda: band.set_tracer_series(1), -6) == WINDOW % "beom_multi_set_tracer_series"
    band.close()
    many = capi.MultiEngine(_band_frame("closed_2l"), devices=(0, 0))
    assert _refusal(lambda: many.set_tracer_series(1), -3) == NO_TRACER.replace("beom_", "beom_multi_")
    assert _refusal(many.download_tracer_series, -3) == NONE.replace("beom_", "beom_multi_")
    many.close()
    # variant = 1 and the rigid lid refuse tracers, as before
    from helpers import Golden
    from test_gpu_integrals import _fields
    for name in ("variant3d_3l", "rigid_lid_sill_2l"):
        g = Golden(name)
        e = capi.Engine(_fields(g), variant=g.variant)
        _refused(lambda: e.set_tracers(1), -6, name)
        assert _refusal(lambda: e.set_tracer_series(1), -3) == NO_TRACER, name
        e.close()


# ---- 7. a tracer series changes nothing else ------------------------------------------------------------------------------------
def test_a_tracer_series_leaves_everything_else_as_it_was():
    f = _case("island_ragged_3l")
    plain, withs = _with_tracers(capi.Engine(f), f, 2), _with_tracers(capi.Engine(f), f, 2)
    for x in (plain, withs):
        x.set_series(2, 1, 10)
        x.set_tracer_moments(3, 2)
    withs.set_tracer_series(3, 1, 10)
    for x in (plain, withs):
        x.step(1, 4); x.step(5, 6)
    for what in ("mont_history", "plain_sweeps", "uv_fused", "tracer_moment_launches", "series_records"):
        assert plain.info(what) == withs.info(what), what
    assert plain.info("tracer_series") == 0 and withs.info("tracer_series") == 3 and withs.info("tracer_series_records") == 10
    a, b = plain.download(STATE), withs.download(STATE)
    for k in a:
        assert same_bits(a[k], b[k]), k
    ta, tb = plain.download_tracers(), withs.download_tracers()
    assert same_bits(ta["q"], tb["q"]) and same_bits(ta["rq"], tb["rq"])
    ma, mb = plain.download_tracer_moments(), withs.download_tracer_moments()
    assert ma["count"] == mb["count"] == 5
    for k in ("ref", "sum", "sq"):
        assert same_bits(ma[k], mb[k]), ("tracer moments", k)
    sa, sb = plain.download_series(), withs.download_series()
    assert list(sa["tstp"]) == list(sb["tstp"]) and same_bits(sa["rows"], sb["rows"])
    assert withs.download_tracer_series()["count"] == 10
    plain.close(); withs.close()


# ---- 8. bands -----------------------------------------------------------------------------------------------------------------
_SINGLE = {}


def _band_fields(case):
    if case == "closed_2l":
        return _band_frame("closed_2l")
    # the frame with land of test_gpu_tracer_moments: an island across every seam
    p, files = I.case_headline(48, 100, 2)
    files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
    x = np.arange(p.lm + 2)[:, None]; y = np.arange(p.mm + 2)[None, :]
    land = ((x - 0.4 * p.lm) / (0.2 * p.lm)) ** 2 + ((y - 0.5 * p.mm) / (0.3 * p.mm)) ** 2 < 1.0
    files["h_bo"][land] = 0.0
    files["init"][land] = 0.0
    p = p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"]))
    return read_input_data(p, files=files)


def _single_handle_records(case):
    """The single handle's records of the banded cases (5 + 7 steps, stride 2, level 3), formed once and checked against the
    restatement at the last step."""
    if case not in _SINGLE:
        f = _band_fields(case)
        one = _with_tracers(capi.Engine(f), f, 2)
        assert one.is_embedded == (case == "closed_2l_island")
        got = _series_of(one, (5, 7), 3, stride=2, records=8)
        assert same_bits(got["rows"][-1], _restated(f, one, 3)), case
        one.close()
        _SINGLE[case] = (f, got)
    return _SINGLE[case]


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("nband", [2, 3])
@pytest.mark.parametrize("case", ["closed_2l", "closed_2l_island"])
def test_bands_give_the_single_handles_records(case, nband, overlap):
    f, want = _single_handle_records(case)
    assert list(want["tstp"]) == [2, 4, 6, 8, 10, 12] and not np.isnan(want["rows"]).any()
    assert want["fu"].any() and want["fv"].any()
    many, plain = (_with_tracers(capi.MultiEngine(f, devices=[0] * nband), f, 2) for _ in range(2))
    assert many.count == nband
    for x in (many, plain):
        x.set_option("overlap", overlap)
    got = _series_of(many, (5, 7), 3, stride=2, records=8)
    plain.step(1, 5); plain.step(6, 7)
    assert list(got["tstp"]) == list(want["tstp"])
    assert same_bits(got["rows"], want["rows"]), (case, nband, overlap)
    assert same_bits(got["total"], want["total"]) and same_bits(got["transport"], want["transport"])
    s = many.stats()
    assert s == plain.stats(), (case, nband, overlap, s, plain.stats())
    if overlap:
        assert s["split"] >= nband * 9, (nband, s, "the bands' steps were not cut")
    else:
        assert s["split"] == 0, (nband, s)
    a, b = many.download(FIELDS), plain.download(FIELDS)
    for k in a:
        assert same_bits(a[k], b[k]), (case, nband, k)
    assert same_bits(many.download_tracers()["q"], plain.download_tracers()["q"])
    # the recorder is empty again, and a call that would overflow it is refused before anything is launched
    assert many.download_tracer_series()["count"] == 0
    many.set_tracer_series(3, 1, 3)
    assert _refusal(lambda: many.step(13, 4), -3) == OVERFLOW % ("beom_multi_step", 13, 16, 4, 1, 0, 3, "beom_multi_download_tracer_series")
    many.step(13, 3)
    assert list(many.download_tracer_series()["tstp"]) == [13, 14, 15]
    # a handle without a tracer series says so, and bad arguments are refused in the bands' own words
    assert _refusal(plain.download_tracer_series, -3) == NONE.replace("beom_", "beom_multi_")
    assert _refusal(lambda: plain.set_tracer_series(4, 1, 4), -3) == BAD_ARGS % ("beom_multi_set_tracer_series", 4, 1, 4)
    many.close(); plain.close()
