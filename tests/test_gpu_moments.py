"""Moments on the device (beom_set_moments ..., include/beom_hip.h) against the numpy restatement (moments_ref, held to
two-pass values by test_moments_cpu): the per-sweep entry on rough fields, real steps fed with the state downloaded from the
same handle, one call of K steps against K calls, every handle kind and 2 / 3 bands (cut steps, whole steps, a ring), a
handle with moments steps as one without, moments beside tracers and floats, refusals.  Every comparison is
helpers.same_bits."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import floats_ref as FR
import moments_ref as MR
import rough_inputs as RI
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, Golden, same_bits, tile_geometry
from test_gpu_parity import _fields, _live

pytestmark = pytest.mark.gpu
NSTEPS = 12
MODES = {"dense_64x4": (1, 4), "dense_64x8": (1, 8), "table": (0, 8)}      # name: (dense_hint, tile rows)
NEVER_DENSE = ("random_coast_2l_xper",)           # (wraps row by row: stays on the table path whatever the hint)
# the small golden frames give an elementwise kernel what it can get wrong: element counts that are no multiple of the pair
# or the block, the 15-element alignment offset, the layer stride, padding slots that the download leaves out
PER_SWEEP = [("jet_2l_xyper", "dense_64x4"), ("jet_2l_xyper", "dense_64x8"), ("island_3l_forced", "dense_64x4"),
             ("random_coast_2l_xper", "table")]
REAL = ("jet_2l_xyper", "island_3l_forced", "sill_4l_ocrp", "variant3d_3l", "rigid_lid_sill_2l", "biharm_island_2l", "obc_mcbc0_2l")


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _engine(g, mode="dense_64x4"):
    dense_hint, rows = MODES[mode]
    with tile_geometry(rows):
        e = capi.Engine(_fields(g), variant=g.variant, dense_hint=dense_hint)
    assert e.is_dense == (bool(dense_hint) and g.name not in NEVER_DENSE), (g.name, mode)
    return e


def _same_moments(got, ref, what):
    """ref, sum, sq and count of a download against the restatement."""
    assert got["count"] == ref.count, (what, got["count"], ref.count)
    assert same_bits(got["ref"], ref.ref), (what, "ref")
    assert same_bits(got["sum"], ref.sum), (what, "sum", float(np.max(np.abs(got["sum"] - ref.sum))))
    if ref.level >= 3:
        assert same_bits(got["sq"], ref.sq), (what, "sq", float(np.max(np.abs(got["sq"] - ref.sq))))
        assert same_bits(got["var"], ref.var), (what, "var")
    else:
        assert "sq" not in got and "var" not in got
    assert same_bits(got["mean"], ref.mean), (what, "mean")


def _same_downloads(a, b, what):
    assert (a["count"], a["tstp_first"], a["tstp_last"]) == (b["count"], b["tstp_first"], b["tstp_last"]), what
    for k in ("ref", "sum", "sq"):
        assert (k in a) == (k in b)
        if k in a:
            assert same_bits(a[k], b[k]), (what, k)


# ---- the per-sweep entry on rough fields ------------------------------------------------------------------------------------
_ROUGH = {}


def _rough_states(name, f):
    """Six rough states of the fixture (rough_inputs amplitudes, exact +-0 in the velocities), built once."""
    if name not in _ROUGH:
        _ROUGH[name] = [{k: np.ascontiguousarray(getattr(g, k), dtype=np.float64) for k in MR.FIELDS}
                        for g in (RI.rough_fields(f, seed) for seed in range(1, 7))]
    return _ROUGH[name]


@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("name,mode", PER_SWEEP)
def test_per_sweep_entry_equals_the_restatement(name, mode, level):
    g = Golden(name)
    e = _engine(g, mode)
    if name == "island_3l_forced":
        assert e.is_embedded
    ref = MR.Moments(level)
    e.set_moments(level, stride=7)                   # (the per-sweep entry samples whatever the stride)
    assert e.info("moments") == level and e.info("moment_samples") == 0
    for k, st in enumerate(_rough_states(name, e.f), 1):
        e.upload(**st)
        e.sample_moments()
        ref.sample(st)
        _same_moments(e.download_moments(), ref, (name, mode, level, k))
    assert e.info("moment_samples") == 6 and e.info("moment_launches") == 6
    assert np.any(ref.sum[:, :, 1:] != 0.0)
    # reset: the next sample is a first sample again, on arrays that held another average
    e.reset_moments()
    zero = e.download_moments()
    assert zero["count"] == 0 and not zero["ref"].any() and not zero["sum"].any()
    ref.reset()
    for st in _rough_states(name, e.f)[3:]:
        e.upload(**st)
        e.sample_moments()
        ref.sample(st)
    _same_moments(e.download_moments(), ref, (name, mode, level, "after reset"))
    e.close()


# ---- real steps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense_64x4", "table"])
@pytest.mark.parametrize("name", REAL)
def test_real_steps_equal_the_restatement(name, mode):
    """12 steps one at a time with stride 1: the restatement fed download() of the same handle after every step."""
    g = Golden(name)
    e = _engine(g, mode)
    ref = MR.Moments(3)
    e.set_moments(3)
    for t in range(1, NSTEPS + 1):
        e.step(t, 1)
        if name == "jet_2l_xyper" and mode != "table" and t >= 8:
            # the partner buffers and the stale history are what is being sampled
            assert e.info("mont_history") == 1, (name, mode, t)
        ref.sample(e.download(MR.FIELDS))
        got = e.download_moments()
        _same_moments(got, ref, (name, mode, t))
        assert (got["tstp_first"], got["tstp_last"]) == (1, t)
    assert np.isfinite(ref.sum).all() and np.isfinite(ref.sq).all()
    assert np.any(ref.sum[0][:, 1:] != 0.0) and np.any(ref.sq[:, :, 1:] != 0.0), (name, "nothing moved: nothing tested")
    assert e.info("moment_launches") == NSTEPS
    e.close()


@pytest.mark.parametrize("name", ["jet_2l_xyper", "rigid_lid_sill_2l"])
def test_one_call_of_12_steps_stride_3_against_12_calls(name):
    g = Golden(name)
    one, many = _engine(g), _engine(g)
    for e in (one, many):
        e.set_moments(3, stride=3)
    one.step(1, NSTEPS)
    for t in range(1, NSTEPS + 1):
        many.step(t, 1)
    a, b = one.download_moments(), many.download_moments()
    _same_downloads(a, b, name)
    assert (a["count"], a["tstp_first"], a["tstp_last"]) == (4, 3, 12)
    assert one.info("moment_launches") == 4 and many.info("moment_launches") == 4 and one.info("moment_samples") == 4
    # a restart continues the average: beom_upload_state does not reset
    st = one.download()
    one.upload(**st)
    one.step(NSTEPS + 1, 3); many.step(NSTEPS + 1, 3)
    a, b = one.download_moments(), many.download_moments()
    _same_downloads(a, b, (name, "continued"))
    assert (a["count"], a["tstp_first"], a["tstp_last"]) == (5, 3, 15)
    one.close(); many.close()


# ---- handle kinds -----------------------------------------------------------------------------------------------------------
def _stepped(x, level=3, stride=1, calls=(5, 7)):
    x.set_moments(level, stride)
    t = 1
    for n in calls:
        x.step(t, n)
        t += n
    assert t - 1 == NSTEPS
    return x.download_moments()


@pytest.mark.parametrize("name", ["jet_2l_xyper", "island_3l_forced"])
def test_handle_kinds_give_the_same_bits(name):
    g = Golden(name)
    got = {}
    for mode in MODES:
        e = _engine(g, mode)
        got[mode] = _stepped(e)
        e.close()
    assert got["table"]["count"] == NSTEPS and np.any(got["table"]["sq"] != 0.0)
    for mode in ("dense_64x4", "dense_64x8"):
        _same_downloads(got[mode], got["table"], (name, mode))


def _band_frame(name):
    """Frames of a few thousand cells whose bands are tall enough (32 rows) for a cut step."""
    p, files = I.case_headline(48, 100, 2) if name == "closed_2l" else I.case_unstable_jet(lm=40, mm=96, nlay=2, dt_s=1.5)
    return read_input_data(p, files=files)


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("level", [2, 3])
def test_bands_give_the_single_handles_bits(level, overlap):
    """2 and 3 bands in one process, stepping cut (overlap = 1) and whole (overlap = 0), stride 2 over calls of 5 and 7."""
    f = _band_frame("closed_2l")
    e = capi.Engine(f)
    want = _stepped(e, level, 2)
    e.close()
    assert (want["count"], want["tstp_first"], want["tstp_last"]) == (6, 2, 12) and np.any(want["sum"][:, :, 1:] != 0.0)
    for nb in (2, 3):
        many = capi.MultiEngine(f, devices=[0] * nb)
        assert many.count == nb
        many.set_option("overlap", overlap)
        got = _stepped(many, level, 2)
        s = many.stats()
        if overlap:
            assert s["split"] >= nb * (NSTEPS - 3), (nb, s, "the bands' steps were not cut")
        else:
            assert s["split"] == 0, (nb, s)
        _same_downloads(got, want, ("closed_2l", level, overlap, nb))
        assert many.info("moment_launches") == 6
        many.reset_moments()
        assert many.download_moments()["count"] == 0
        many.close()


def test_bands_of_a_frame_with_land_give_the_single_handles_bits():
    """Moments on 2 and 3 bands of a frame WITH land: the bands' rows differ in length, the global arrays take each band's
    packed row ranges.  The island is an ellipse (half-axes 0.2 lm and 0.3 mm around (0.4 lm, 0.5 mm)): a disc of radius
    0.2 lm would lie between the two seams of 3 bands, which fall near rows mm/3 and 2 mm/3."""
    p, files = I.case_headline(48, 100, 2)
    files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
    x = np.arange(p.lm + 2)[:, None]; y = np.arange(p.mm + 2)[None, :]
    land = ((x - 0.4 * p.lm) / (0.2 * p.lm)) ** 2 + ((y - 0.5 * p.mm) / (0.3 * p.mm)) ** 2 < 1.0
    files["h_bo"][land] = 0.0
    files["init"][land] = 0.0
    p = p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"]))
    f = read_input_data(p, files=files)
    e = capi.Engine(f)
    assert e.is_embedded
    want = _stepped(e, 3, 2)
    e.close()
    assert (want["count"], want["tstp_first"], want["tstp_last"]) == (6, 2, 12) and np.any(want["sum"][:, :, 1:] != 0.0)
    row_len = np.bincount(f.subc[1, 1:], minlength=p.mm + 2)
    for nb in (2, 3):
        many = capi.MultiEngine(f, devices=[0] * nb)
        assert many.count == nb
        bands = [many.band(k) for k in range(nb)]
        for k in range(nb - 1):                   # the island crosses every seam: the rows on both sides are short
            assert bands[k + 1]["own0"] == bands[k]["own1"] + 1
            assert row_len[bands[k]["own1"]] < p.lm + 1 and row_len[bands[k + 1]["own0"]] < p.lm + 1, (nb, k, bands)
        got = _stepped(many, 3, 2)
        _same_downloads(got, want, ("closed_2l with an island", nb))
        many.close()


def test_a_ring_of_bands_gives_the_single_handles_bits():
    """A frame periodic in y on 2 bands: the orphan row mm+1 comes from the companion frame's own moments."""
    f = copy.copy(_band_frame("jet_xyper_2l"))
    orphan = 1 + f.p.mm * (f.p.lm + 1)             # row mm+1 is masked out (it duplicates row 1) and would hold +0 only:
    f.hlay = np.array(f.hlay, dtype=np.float64)    # give it a thickness of its own, which no step changes
    f.hlay[:, orphan:] = 7.0 + np.arange(f.hlay.shape[1] - orphan)[None]
    e = capi.Engine(f)
    want = _stepped(e, 3, 2)
    e.close()
    ring = capi.MultiEngine(f, devices=(0, 0))
    assert ring.describe()["ring"] == 1
    got = _stepped(ring, 3, 2)
    _same_downloads(got, want, "ring")
    assert same_bits(want["ref"][0][:, orphan:], f.hlay[:, orphan:]), "the orphan row did not keep its own thickness: nothing tested"
    assert np.any(want["sum"][:, :, 1:orphan] != 0.0)
    ring.close()


# ---- a handle with moments steps as one without ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jet_2l_xyper", "island_3l_forced", "rigid_lid_sill_2l"])
def test_moments_leave_the_step_as_it_was(name):
    g = Golden(name)
    plain, mom = _engine(g), _engine(g)
    mom.set_moments(3)
    plain.step(1, 10); mom.step(1, 10)
    for what in ("mont_history", "plain_sweeps", "uv_fused", "stress_folded"):
        assert plain.info(what) == mom.info(what), (name, what)
    a, b = plain.download(), mom.download()
    for key in STATE:
        assert same_bits(a[key], b[key]), (name, key)
    assert plain.info("moments") == 0 and plain.info("moment_launches") == 0 and mom.info("moment_launches") == 10
    mom.set_moments(0)                                              # freed: back to a handle without moments
    assert mom.info("moments") == 0 and mom.info("moment_samples") == 0
    with pytest.raises(capi.BeomError):
        mom.download_moments()
    plain.step(11, 2); mom.step(11, 2)
    assert mom.info("moment_launches") == 10
    a, b = plain.download(), mom.download()
    for key in _live(plain, STATE):
        assert same_bits(a[key], b[key]), (name, key, "after the moments were freed")
    plain.close(); mom.close()


# ---- beside tracers and floats ----------------------------------------------------------------------------------------------
def test_with_tracers_and_floats_together():
    """All three features on one handle give the bits each gives alone."""
    g = Golden("island_3l_forced")
    f = _fields(g)
    x, y, layer = FR.seed_floats(f, 500, 3)
    q = np.ascontiguousarray(np.stack([np.asarray(f.hlay, dtype=np.float64), 0.5 * np.asarray(f.hlay, dtype=np.float64)]))

    def run(tracers, floats, moments):
        e = _engine(g)
        if tracers:
            e.set_tracers(2)
            e.upload_tracers(q=q)
        if floats:
            e.set_floats(x, y, layer)
        if moments:
            e.set_moments(3, 2)
        e.step(1, 5); e.step(6, 7)
        out = (e.download_tracers() if tracers else None, e.download_floats() if floats else None,
               e.download_moments() if moments else None, e.download())
        e.close()
        return out

    tr, fl, mo, st = run(True, True, True)
    tr1, fl1, mo1 = run(True, False, False)[0], run(False, True, False)[1], run(False, False, True)[2]
    assert same_bits(tr["q"], tr1["q"]) and same_bits(tr["rq"], tr1["rq"])
    assert same_bits(fl["x"], fl1["x"]) and same_bits(fl["y"], fl1["y"]) and np.array_equal(fl["rejected"], fl1["rejected"])
    _same_downloads(mo, mo1, "moments beside tracers and floats")
    assert mo["count"] == 6


# ---- refusals and errors ------------------------------------------------------------------------------------------------------
def _rc(call):
    with pytest.raises(capi.BeomError) as ei:
        call()
    return str(ei.value)


def test_refusals_and_errors():
    g = Golden("island_3l_forced")
    e = _engine(g)
    for what, call in {"download": e.download_moments, "sample": e.sample_moments, "reset": e.reset_moments}.items():
        assert "error -3" in _rc(call), (what, "without set_moments")
    for level, stride in ((-1, 1), (4, 1), (1, 0), (3, -2)):
        msg = _rc(lambda: e.set_moments(level, stride))
        assert "error -3:" in msg and len(msg.split("error -3:")[1].strip()) > 20, (level, stride, msg)
        assert e.info("moments") == 0
    n = (5, e.p.nlay, e.p.ndeg + 1)
    for level in (1, 2):
        e.set_moments(level)
        sq, count = np.zeros(n), C.c_longlong(-1)
        rc = e.lib.beom_download_moments(e.h, None, None, capi._dp(sq), C.byref(count), None, None, e._err, capi.ERRLEN)
        assert rc == -3 and len(e._err.value.decode().strip()) > 20, (level, rc)
        # count = 0 downloads zeros, and only the fields the level keeps
        nf = 3 if level == 1 else 5
        ref, sm = np.full(n, 7.0), np.full(n, 7.0)
        t0, t1 = C.c_int(-1), C.c_int(-1)
        rc = e.lib.beom_download_moments(e.h, capi._dp(ref), capi._dp(sm), None, C.byref(count), C.byref(t0), C.byref(t1),
                                         e._err, capi.ERRLEN)
        assert rc == 0 and (count.value, t0.value, t1.value) == (0, 0, 0)
        assert not ref[:nf].any() and not sm[:nf].any() and (ref[nf:] == 7.0).all() and (sm[nf:] == 7.0).all()
        got = e.download_moments()
        assert got["count"] == 0 and got["ref"].shape[0] == nf and not got["sum"].any()
    e.step(1, 2)
    assert e.download_moments()["count"] == 2
    e.close()
    # a handle that holds one band's window
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    msg = _rc(lambda: band.set_moments(1))
    assert "error -6:" in msg and len(msg.split("error -6:")[1].strip()) > 20, msg
    band.close()
