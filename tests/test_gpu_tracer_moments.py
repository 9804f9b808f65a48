"""Tracer moments on the device (beom_set_tracer_moments ..., include/beom_hip.h) against the numpy restatement
(tracer_moments_ref, tied to the field moments and to two-pass values by test_tracer_moments_cpu): the per-sweep entry on rough
fields with negative concentrations and dry neighbours, real steps fed with the downloads of the same handle under both tracer
schemes, one call of K steps against K calls and a restart, every handle kind, 2 and 3 bands (cut steps, whole steps, an
island across the seams), a handle with tracer moments steps as one without, the identity with the field moments on one
handle, refusals.  Every comparison is helpers.same_bits."""
import ctypes as C
import os

import numpy as np
import pytest

import floats_ref as FR
import rough_inputs as RI
import tracer_moments_ref as TM
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, Golden, same_bits, tile_geometry
from test_gpu_parity import _fields, _live
from test_gpu_tracers import _tracers

pytestmark = pytest.mark.gpu
NSTEPS = 12
MODES = {"dense_64x4": (1, 4), "dense_64x8": (1, 8), "table": (0, 8)}      # name: (dense_hint, tile rows)
NEVER_DENSE = ("random_coast_2l_xper",)           # (wraps row by row: stays on the table path whatever the hint)
# golden frames of a few hundred cells: their rows are shorter than a wave, so a dense handle runs the edge form of the kernel
# only; its interior waves (the shuffles) are reached in test_handle_kinds_on_a_frame_wider_than_a_wave
PER_SWEEP = [("jet_2l_xyper", "dense_64x4"), ("jet_2l_xyper", "dense_64x8"), ("island_3l_forced", "dense_64x4"),
             ("random_coast_2l_xper", "table")]
REAL = ("jet_2l_xyper", "island_3l_forced", "sill_4l_ocrp", "tc_wave_sponge")


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _engine(g, mode="dense_64x4", tracers=True):
    dense_hint, rows = MODES[mode]
    f = _fields(g)
    with tile_geometry(rows):
        e = capi.Engine(f, variant=g.variant, dense_hint=dense_hint)
    assert e.is_dense == (bool(dense_hint) and g.name not in NEVER_DENSE), (g.name, mode)
    if tracers:
        q, rq, ctrg = _tracers(f)
        e.set_tracers(2)
        e.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    return e


def _same_moments(got, ref, what):
    """ref, sum, sq and count of a download against the restatement."""
    assert got["count"] == ref.count, (what, got["count"], ref.count)
    assert got["ref"].shape == ref.ref.shape, (what, got["ref"].shape, ref.ref.shape)
    for k in range(ref.nq):
        assert same_bits(got["ref"][k], ref.ref[k]), (what, "ref", TM.QUANTITIES[k], float(np.max(np.abs(got["ref"][k] - ref.ref[k]))))
        assert same_bits(got["sum"][k], ref.sum[k]), (what, "sum", TM.QUANTITIES[k], float(np.max(np.abs(got["sum"][k] - ref.sum[k]))))
    if ref.level >= 3:
        assert same_bits(got["sq"], ref.sq), (what, "sq", float(np.max(np.abs(got["sq"] - ref.sq))))
        assert same_bits(got["var_c"], ref.var_c), (what, "var_c")
    else:
        assert "sq" not in got and "var_c" not in got
    assert same_bits(got["mean"], ref.mean), (what, "mean")
    assert not got["ref"][..., 0].any() and not got["sum"][..., 0].any()


def _same_downloads(a, b, what):
    assert (a["count"], a["tstp_first"], a["tstp_last"]) == (b["count"], b["tstp_first"], b["tstp_last"]), what
    for k in ("ref", "sum", "sq"):
        assert (k in a) == (k in b)
        if k in a:
            assert same_bits(a[k], b[k]), (what, k)


# ---- the per-sweep entry on rough fields ------------------------------------------------------------------------------------
_ROUGH = {}


def _rough_states(name, f):
    """Six rough states of the fixture (rough_inputs amplitudes) with one cell-layer in twenty dried up (hlay = +0 exactly, so
    wet cells have dry neighbours on every side), and per state a rough content of two tracers: concentrations in
    [-0.4, 1.2], and a content stranded in the dry cell-layers, which reads as concentration +0.  Built once."""
    if name not in _ROUGH:
        out = []
        for seed in range(1, 7):
            g = RI.rough_fields(f, seed)
            r = np.random.default_rng([seed, 977])
            h = np.array(g.hlay, dtype=np.float64)
            dry = r.uniform(0.0, 1.0, h.shape) < 0.05
            h[dry] = 0.0
            c = r.uniform(-0.4, 1.2, (2,) + h.shape)
            q = np.where(dry[None], r.uniform(-0.01, 0.01, c.shape), c * h[None])
            q[..., 0] = 0.0
            st = {"hlay": h, "h_u": np.ascontiguousarray(g.h_u, dtype=np.float64), "h_v": np.ascontiguousarray(g.h_v, dtype=np.float64)}
            out.append((st, np.ascontiguousarray(q)))
        _ROUGH[name] = out
    return _ROUGH[name]


def test_rough_states_are_rough():
    f = _fields(Golden("island_3l_forced"))
    W, S = f.neig[:, 4].astype(np.int64), f.neig[:, 6].astype(np.int64)
    st, q = _rough_states("island_3l_forced", f)[0]
    wet = st["hlay"] > 0
    assert np.any(q[:, wet] < 0.0), "no negative concentration"
    assert np.any(wet[:, 1:] & ~wet[:, W][:, 1:] & (st["h_u"][:, 1:] > 0)), "no face whose upwind W cell is dry"
    assert np.any(wet[:, 1:] & ~wet[:, S][:, 1:] & (st["h_v"][:, 1:] > 0)), "no face whose upwind S cell is dry"
    assert np.any(~wet[:, 1:] & wet[:, W][:, 1:] & (st["h_u"][:, 1:] < 0)), "no dry cell upwind of its W face"
    for k in ("h_u", "h_v"):
        assert np.any(st[k] > 0) and np.any(st[k] < 0), k


@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("name,mode", PER_SWEEP)
def test_per_sweep_entry_equals_the_restatement(name, mode, level):
    g = Golden(name)
    e = _engine(g, mode)
    if name == "island_3l_forced":
        assert e.is_embedded
    ref = TM.TracerMoments(e.f, level)
    e.set_tracer_moments(level, stride=7)            # (the per-sweep entry samples whatever the stride)
    assert e.info("tracer_moments") == level and e.info("tracer_moment_samples") == 0
    states = _rough_states(name, e.f)
    for k, (st, q) in enumerate(states, 1):
        e.upload(**st)
        e.upload_tracers(q=q)
        e.sample_tracer_moments()
        ref.sample(st["hlay"], st["h_u"], st["h_v"], q)
        _same_moments(e.download_tracer_moments(), ref, (name, mode, level, k))
    assert e.info("tracer_moment_samples") == 6 and e.info("tracer_moment_launches") == 6
    for k in range(ref.nq):
        assert np.any(ref.sum[k][..., 1:] != 0.0), TM.QUANTITIES[k]
    # reset: the next sample is a first sample again, on arrays that held another average
    e.reset_tracer_moments()
    zero = e.download_tracer_moments()
    assert zero["count"] == 0 and not zero["ref"].any() and not zero["sum"].any()
    ref.reset()
    for st, q in states[3:]:
        e.upload(**st)
        e.upload_tracers(q=q)
        e.sample_tracer_moments()
        ref.sample(st["hlay"], st["h_u"], st["h_v"], q)
    _same_moments(e.download_tracer_moments(), ref, (name, mode, level, "after reset"))
    e.close()


# ---- real steps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("name", REAL)
def test_real_steps_equal_the_restatement(name, scheme):
    """12 steps one at a time with stride 1: the restatement fed the downloads of the same handle after every step.  Under
    scheme 2 the sampled faces are still the upstream ones."""
    g = Golden(name)
    e = _engine(g)
    e.set_tracer_scheme(scheme)
    ref = TM.TracerMoments(e.f, 3)
    e.set_tracer_moments(3)
    for t in range(1, NSTEPS + 1):
        e.step(t, 1)
        st = e.download(("hlay", "h_u", "h_v"))
        ref.sample(st["hlay"], st["h_u"], st["h_v"], e.download_tracers()["q"])
        got = e.download_tracer_moments()
        _same_moments(got, ref, (name, scheme, t))
        assert (got["tstp_first"], got["tstp_last"]) == (1, t)
    assert np.isfinite(ref.sum).all() and np.isfinite(ref.sq).all()
    for k in range(4):
        assert np.any(ref.sum[k, 1][:, 1:] != 0.0), (name, TM.QUANTITIES[k], "nothing moved: nothing tested")
    assert np.any(ref.sq[1][:, 1:] != 0.0)
    assert e.info("tracer_moment_launches") == NSTEPS and e.info("tracer_scheme") == scheme
    e.close()


def test_one_call_of_12_steps_stride_3_against_12_calls_and_a_restart():
    g = Golden("jet_2l_xyper")
    one, many = _engine(g), _engine(g)
    for e in (one, many):
        e.set_tracer_moments(3, stride=3)
    one.step(1, NSTEPS)
    for t in range(1, NSTEPS + 1):
        many.step(t, 1)
    a, b = one.download_tracer_moments(), many.download_tracer_moments()
    _same_downloads(a, b, "one call against twelve")
    assert (a["count"], a["tstp_first"], a["tstp_last"]) == (4, 3, 12) and np.any(a["sq"] != 0.0)
    assert one.info("tracer_moment_launches") == 4 and many.info("tracer_moment_launches") == 4
    assert one.info("tracer_moment_samples") == 4
    # a restart continues the average: neither beom_upload_state nor beom_upload_tracers resets
    st, tr = one.download(), one.download_tracers()
    one.upload(**st)
    one.upload_tracers(q=tr["q"], rq=tr["rq"])
    one.step(NSTEPS + 1, 3); many.step(NSTEPS + 1, 3)
    a, b = one.download_tracer_moments(), many.download_tracer_moments()
    _same_downloads(a, b, "continued")
    assert (a["count"], a["tstp_first"], a["tstp_last"]) == (5, 3, 15)
    # beom_set_tracers with another count frees them; with the same count it does not
    many.set_tracers(2)
    assert many.info("tracer_moments") == 3
    many.set_tracers(1)
    assert many.info("tracer_moments") == 0 and many.info("tracer_moment_samples") == 0
    one.close(); many.close()


# ---- handle kinds -----------------------------------------------------------------------------------------------------------
def _stepped(x, level=3, stride=1, calls=(5, 7)):
    x.set_tracer_moments(level, stride)
    t = 1
    for n in calls:
        x.step(t, n)
        t += n
    assert t - 1 == NSTEPS
    return x.download_tracer_moments()


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


def _with_tracers(x, f):
    q, rq, ctrg = _tracers(f)
    x.set_tracers(2)
    x.upload_tracers(q=q, rq=rq, ctrg=ctrg)
    return x


def test_handle_kinds_on_a_frame_wider_than_a_wave():
    """150 x 131 x 3: rows of more than 64 cells, so the dense handle has interior waves (W thickness and concentration by
    shuffle, lane 0 loading its own) next to edge waves, and the table path has both of its forms too; all against the
    restatement fed this handle's downloads, and against each other."""
    p, files = I.case_headline(150, 131, 3)
    f = read_input_data(p, files=files)
    e, tab = _with_tracers(capi.Engine(f), f), _with_tracers(capi.Engine(f, dense_hint=0), f)
    assert e.is_dense and not tab.is_dense
    ref = TM.TracerMoments(f, 3)
    for x in (e, tab):
        x.set_tracer_moments(3, 2)
    for t in (1, 3):
        e.step(t, 2); tab.step(t, 2)
        st = e.download(("hlay", "h_u", "h_v"))
        ref.sample(st["hlay"], st["h_u"], st["h_v"], e.download_tracers()["q"])
    a, b = e.download_tracer_moments(), tab.download_tracer_moments()
    _same_moments(a, ref, "150 x 131 x 3, dense")
    _same_downloads(a, b, "dense against the table path")
    assert np.any(ref.sum[2:, 1][..., 1:] != 0.0) and (a["tstp_first"], a["tstp_last"]) == (2, 4)
    e.close(); tab.close()


# ---- bands ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("level", [2, 3])
def test_bands_give_the_single_handles_bits(level, overlap):
    """2 and 3 bands in one process, stepping cut (overlap = 1) and whole (overlap = 0), stride 2 over calls of 5 and 7."""
    f = _band_frame("closed_2l")
    e = _with_tracers(capi.Engine(f), f)
    want = _stepped(e, level, 2)
    e.close()
    assert (want["count"], want["tstp_first"], want["tstp_last"]) == (6, 2, 12)
    for k in range(4):
        assert np.any(want["sum"][k, 1][:, 1:] != 0.0), TM.QUANTITIES[k]
    for nb in (2, 3):
        many = _with_tracers(capi.MultiEngine(f, devices=[0] * nb), f)
        assert many.count == nb
        many.set_option("overlap", overlap)
        got = _stepped(many, level, 2)
        s = many.stats()
        if overlap:
            assert s["split"] >= nb * (NSTEPS - 3), (nb, s, "the bands' steps were not cut")
        else:
            assert s["split"] == 0, (nb, s)
        _same_downloads(got, want, ("closed_2l", level, overlap, nb))
        assert many.info("tracer_moment_launches") == 6 and many.info("tracer_moments") == level
        many.reset_tracer_moments()
        assert many.download_tracer_moments()["count"] == 0
        many.close()


def test_bands_of_a_frame_with_land_give_the_single_handles_bits():
    """2 and 3 bands of a frame WITH land: the island (an ellipse, half-axes 0.2 lm and 0.3 mm around (0.4 lm, 0.5 mm)) lies
    across every seam, so the rows on both sides of a seam are short and the S neighbour of a band's first owned row is land
    for some cells and a ghost cell for others."""
    p, files = I.case_headline(48, 100, 2)
    files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
    x = np.arange(p.lm + 2)[:, None]; y = np.arange(p.mm + 2)[None, :]
    land = ((x - 0.4 * p.lm) / (0.2 * p.lm)) ** 2 + ((y - 0.5 * p.mm) / (0.3 * p.mm)) ** 2 < 1.0
    files["h_bo"][land] = 0.0
    files["init"][land] = 0.0
    p = p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"]))
    f = read_input_data(p, files=files)
    e = _with_tracers(capi.Engine(f), f)
    assert e.is_embedded
    want = _stepped(e, 3, 2)
    e.close()
    assert (want["count"], want["tstp_first"], want["tstp_last"]) == (6, 2, 12) and np.any(want["sum"][2:, 1][..., 1:] != 0.0)
    row_len = np.bincount(f.subc[1, 1:], minlength=p.mm + 2)
    for nb in (2, 3):
        many = _with_tracers(capi.MultiEngine(f, devices=[0] * nb), f)
        assert many.count == nb
        bands = [many.band(k) for k in range(nb)]
        for k in range(nb - 1):
            assert bands[k + 1]["own0"] == bands[k]["own1"] + 1
            assert row_len[bands[k]["own1"]] < p.lm + 1 and row_len[bands[k + 1]["own0"]] < p.lm + 1, (nb, k, bands)
        got = _stepped(many, 3, 2)
        _same_downloads(got, want, ("closed_2l with an island", nb))
        many.close()


# ---- nothing else moves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jet_2l_xyper", "island_3l_forced"])
def test_tracer_moments_leave_everything_else_as_it_was(name):
    g = Golden(name)
    x, y, layer = FR.seed_floats(_fields(g), 300, 3)
    plain, mom = _engine(g), _engine(g)
    for e in (plain, mom):
        e.set_floats(x, y, layer)
        e.set_moments(3, 2)
    mom.set_tracer_moments(3)
    plain.step(1, 4); mom.step(1, 4)
    plain.step(5, 6); mom.step(5, 6)
    for what in ("mont_history", "plain_sweeps", "uv_fused"):
        assert plain.info(what) == mom.info(what), (name, what)
    a, b = plain.download(), mom.download()
    for key in _live(plain, STATE):
        assert same_bits(a[key], b[key]), (name, key)
    ta, tb = plain.download_tracers(), mom.download_tracers()
    assert same_bits(ta["q"], tb["q"]) and same_bits(ta["rq"], tb["rq"]), name
    fa, fb = plain.download_floats(), mom.download_floats()
    assert same_bits(fa["x"], fb["x"]) and same_bits(fa["y"], fb["y"]) and np.array_equal(fa["rejected"], fb["rejected"])
    ma, mb = plain.download_moments(), mom.download_moments()
    assert ma["count"] == mb["count"] == 5
    for k in ("ref", "sum", "sq"):
        assert same_bits(ma[k], mb[k]), (name, "field moments", k)
    assert plain.info("tracer_moments") == 0 and plain.info("tracer_moment_launches") == 0
    assert mom.info("tracer_moment_launches") == 10 and mom.info("moment_launches") == 5
    mom.set_tracer_moments(0)                                       # freed: the launch count stops growing
    assert mom.info("tracer_moments") == 0 and mom.info("tracer_moment_samples") == 0
    with pytest.raises(capi.BeomError):
        mom.download_tracer_moments()
    plain.step(11, 2); mom.step(11, 2)
    assert mom.info("tracer_moment_launches") == 10
    a, b = plain.download(), mom.download()
    for key in _live(plain, STATE):
        assert same_bits(a[key], b[key]), (name, key, "after the tracer moments were freed")
    assert same_bits(plain.download_tracers()["q"], mom.download_tracers()["q"])
    plain.close(); mom.close()


# ---- the identity on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jet_2l_xyper", "island_3l_forced", "obc_mcbc0_2l"])
def test_a_tracer_equal_to_hlay_has_the_field_moments_of_the_same_handle(name):
    """The q = hlay, ctrg = 1 tracer next to set_moments(2): its sums of q, fu, fv are those of hlay, h_u, h_v, at faces with a
    wet cell on either side in every sample."""
    g = Golden(name)
    e = _engine(g)
    f = e.f
    W, S = f.neig[:, 4].astype(np.int64), f.neig[:, 6].astype(np.int64)
    e.set_moments(2)
    e.set_tracer_moments(2)
    n1 = f.p.ndeg + 1
    face_u, face_v = np.ones((f.p.nlay, n1), bool), np.ones((f.p.nlay, n1), bool)
    for t in range(1, NSTEPS + 1):
        e.step(t, 1)
        wet = e.download(("hlay",))["hlay"] > 0
        face_u &= wet | wet[:, W]
        face_v &= wet | wet[:, S]
    fm, tm = e.download_moments(), e.download_tracer_moments()
    assert fm["count"] == tm["count"] == NSTEPS
    face_u[:, 0] = face_v[:, 0] = False
    for what in ("ref", "sum"):
        assert same_bits(tm[what][0, 0][:, 1:], fm[what][0][:, 1:]), (name, what, "q against hlay")
        assert same_bits(tm[what][2, 0][face_u], fm[what][3][face_u]), (name, what, "fu against h_u")
        assert same_bits(tm[what][3, 0][face_v], fm[what][4][face_v]), (name, what, "fv against h_v")
    assert np.any(fm["sum"][0][:, 1:] != 0.0) and np.any(fm["sum"][3][face_u] != 0.0) and np.any(fm["sum"][4][face_v] != 0.0)
    e.close()


# ---- refusals and errors ------------------------------------------------------------------------------------------------------
def _rc(call):
    with pytest.raises(capi.BeomError) as ei:
        call()
    return str(ei.value)


def _refused(call, code, what):
    msg = _rc(call)
    tag = "error %d:" % code
    assert tag in msg and len(msg.split(tag)[1].strip()) > 20, (what, msg)


def test_refusals_and_errors():
    g = Golden("island_3l_forced")
    e = _engine(g, tracers=False)
    _refused(lambda: e.set_tracer_moments(1), -3, "no tracers on the handle")
    assert e.info("tracer_moments") == 0
    e.close()
    e = _engine(g)
    _refused(e.download_tracer_moments, -3, "a download before set")
    for what, call in {"sample": e.sample_tracer_moments, "reset": e.reset_tracer_moments}.items():
        assert "error -3" in _rc(call), (what, "without set_tracer_moments")
    for level, stride in ((-1, 1), (4, 1), (1, 0), (3, -2)):
        _refused(lambda: e.set_tracer_moments(level, stride), -3, (level, stride))
        assert e.info("tracer_moments") == 0
    n = (2, e.p.nlay, e.p.ndeg + 1)
    for level in (1, 2):
        e.set_tracer_moments(level)
        sq, count = np.zeros(n), C.c_longlong(-1)
        rc = e.lib.beom_download_tracer_moments(e.h, None, None, capi._dp(sq), C.byref(count), None, None, e._err, capi.ERRLEN)
        assert rc == -3 and len(e._err.value.decode().strip()) > 20, (level, rc)
        got = e.download_tracer_moments()              # count = 0 downloads zeros, and only the quantities the level keeps
        assert got["count"] == 0 and got["ref"].shape[0] == (2 if level == 1 else 4) and not got["sum"].any()
    e.step(1, 2)
    assert e.download_tracer_moments()["count"] == 2
    e.close()
    # bands of a frame periodic in y, and a handle that holds one band's window: neither carries tracers
    ring = capi.MultiEngine(_band_frame("jet_xyper_2l"), devices=(0, 0))
    assert ring.describe()["ring"] == 1
    _refused(lambda: ring.set_tracer_moments(1), -6, "a ring")
    _refused(ring.download_tracer_moments, -6, "a ring's download")
    ring.close()
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    _refused(lambda: band.set_tracer_moments(1), -6, "a handle that holds one band's window")
    band.close()
    many = capi.MultiEngine(_band_frame("closed_2l"), devices=(0, 0))
    _refused(lambda: many.set_tracer_moments(1), -3, "bands without tracers")
    _refused(many.download_tracer_moments, -3, "bands: a download before set")
    many.close()
