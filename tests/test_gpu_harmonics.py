"""Harmonics on the device (beom_set_harmonics ..., include/beom_hip.h) against the numpy restatement (harmonics_ref, held to
the truth by test_harmonics_cpu): the per-sweep entry on rough fields, real tidal steps fed with the state downloaded from
the same handle, one call of K steps against K calls, the other handle kinds, 2 / 3 bands (a ring, chains, cut and whole
steps), a handle with harmonics steps as one without and beside the other add-ons, a fit of uploaded tones, refusals.
Every comparison of raw arrays is helpers.same_bits."""
import ctypes as C
import os

import numpy as np
import pytest

import floats_ref as FR
import harmonics_ref as HR
import rough_inputs as RI
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import STATE, Golden, same_bits, tile_geometry
from test_gpu_parity import _fields, _live
from test_harmonics_cpu import _longdouble_fit

pytestmark = pytest.mark.gpu
NSTEPS = 12
MODES = {"dense_64x4": (1, 4), "dense_64x8": (1, 8), "table": (0, 8)}      # name: (dense_hint, tile rows)
NEVER_DENSE = ("random_coast_2l_xper",)           # (wraps row by row: stays on the table path whatever the hint)
# the small golden frames give an elementwise kernel what it can get wrong: element counts that are no multiple of the pair
# or the block, the 15-element alignment offset, the layer stride, padding slots that the download leaves out
PER_SWEEP = [("jet_2l_xyper", "dense_64x4"), ("jet_2l_xyper", "dense_64x8"), ("island_3l_forced", "dense_64x4"),
             ("random_coast_2l_xper", "table")]
OMEGAS = {1: (11.7,), 2: (12.14, 24.28), 4: (0.9, 12.14, 13.3, 40.1)}      # rad/day, nothing special about them


@pytest.fixture(autouse=True)
def _no_geometry_leak():
    before = os.environ.get("BEOM_TILE4")
    yield
    assert os.environ.get("BEOM_TILE4") == before


def _engine(g, mode="dense_64x4", check_path=False):
    dense_hint, rows = MODES[mode]
    with tile_geometry(rows):
        e = capi.Engine(_fields(g), variant=g.variant, dense_hint=dense_hint)
    if check_path:
        assert e.is_dense == (bool(dense_hint) and g.name not in NEVER_DENSE), (g.name, mode)
    return e


def _ctim(e, tstp):
    """The time of the sample behind step tstp: plan_step's expression."""
    return float(getattr(e.f, "tres", 0.0)) + float(e.p.dtd8) * float(tstp)


def _same_harmonics(got, ref, what):
    """ref, sum, gram, count and omega of a download against the restatement."""
    assert got["count"] == ref.count, (what, got["count"], ref.count)
    assert list(got["omega"]) == ref.omega, what
    assert same_bits(got["gram"], ref.gram), (what, "gram")
    assert same_bits(got["ref"], ref.ref), (what, "ref")
    assert got["sum"].shape == ref.sum.shape, (what, got["sum"].shape, ref.sum.shape)
    assert same_bits(got["sum"], ref.sum), (what, "sum", float(np.max(np.abs(got["sum"] - ref.sum))))


def _same_downloads(a, b, what):
    assert (a["count"], a["tstp_first"], a["tstp_last"]) == (b["count"], b["tstp_first"], b["tstp_last"]), what
    for k in ("omega", "gram", "ref", "sum"):
        assert same_bits(a[k], b[k]), (what, k)


# ---- 1. the per-sweep entry on rough fields -----------------------------------------------------------------------------------
_ROUGH = {}


def _rough_states(name, f):
    """Six rough states of the fixture (rough_inputs amplitudes, exact +-0 in the velocities), built once."""
    if name not in _ROUGH:
        _ROUGH[name] = [{k: np.ascontiguousarray(getattr(g, k), dtype=np.float64) for k in HR.FIELDS}
                        for g in (RI.rough_fields(f, seed) for seed in range(1, 7))]
    return _ROUGH[name]


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("name,mode", PER_SWEEP)
def test_per_sweep_entry_equals_the_restatement(name, mode, K, level):
    g = Golden(name)
    e = _engine(g, mode, check_path=True)
    if name == "island_3l_forced":
        assert e.is_embedded
    ref = HR.Harmonics(OMEGAS[K], level)
    e.set_harmonics(OMEGAS[K], level, stride=7)      # (the per-sweep entry samples whatever the stride)
    assert (e.info("harmonics"), e.info("harmonic_level"), e.info("harmonic_samples")) == (K, level, 0)
    states = _rough_states(name, e.f)
    ctim = 0.0
    for k, st in enumerate(states, 1):
        ctim += 0.013 * k                            # a time that grows from sample to sample, unevenly
        e.upload(**st)
        e.sample_harmonics(ctim)
        ref.sample(st, ctim)
        _same_harmonics(e.download_harmonics(), ref, (name, mode, K, level, k))
    assert e.info("harmonic_samples") == 6 and e.info("harmonic_launches") == 6 * ref.nf
    assert np.any(ref.sum[:, :, :, 1:] != 0.0) and all(np.any(ref.sum[f, m] != 0.0) for f in range(ref.nf) for m in range(ref.nw))
    # reset: the next sample is a first sample again, on arrays that held another analysis
    e.reset_harmonics()
    zero = e.download_harmonics()
    assert zero["count"] == 0 and not zero["ref"].any() and not zero["sum"].any() and not zero["gram"].any()
    assert "amp" not in zero
    ref.reset()
    for st in states[3:]:
        ctim += 0.2
        e.upload(**st)
        e.sample_harmonics(ctim)
        ref.sample(st, ctim)
    _same_harmonics(e.download_harmonics(), ref, (name, mode, K, level, "after reset"))
    e.close()


# ---- 2. real steps ------------------------------------------------------------------------------------------------------------
def _stepped_one_by_one(e, ref, stride, what, nsteps=NSTEPS):
    """nsteps calls of one step; the restatement is fed download() of the same handle after every sampled step."""
    for t in range(1, nsteps + 1):
        e.step(t, 1)
        if t % stride == 0:
            ref.sample(e.download(HR.FIELDS), _ctim(e, t))
            got = e.download_harmonics()
            _same_harmonics(got, ref, (what, t))
            assert (got["tstp_first"], got["tstp_last"]) == (stride, t)
    assert np.isfinite(ref.sum).all() and np.any(ref.sum[0][:, :, 1:] != 0.0), (what, "nothing moved: nothing tested")


@pytest.mark.parametrize("name", ["tide_sponge", "tc_tide_ridge_3l_noocrp"])
def test_real_tidal_steps_equal_the_restatement(name):
    g = Golden(name)
    many, one = _engine(g), _engine(g)
    w = float(many.f.w_ti[0])
    assert w > 0.0
    ref = HR.Harmonics((w, 2.0 * w), 2)
    for e in (many, one):
        e.set_harmonics((w, 2.0 * w), level=2, stride=3)
    _stepped_one_by_one(many, ref, 3, name)
    one.step(1, NSTEPS)
    a, b = one.download_harmonics(), many.download_harmonics()
    _same_downloads(a, b, name)
    assert (a["count"], a["tstp_first"], a["tstp_last"]) == (4, 3, 12)
    assert one.info("harmonic_launches") == many.info("harmonic_launches") == 4 * 5
    # omega = None is the handle's w_ti
    one.set_harmonics()
    assert one.info("harmonics") == 1 and list(one.download_harmonics()["omega"]) == [w]
    # a restart continues the analysis: beom_upload_state does not reset
    st = many.download()
    many.upload(**st)
    many.step(NSTEPS + 1, 3)
    ref.sample(many.download(HR.FIELDS), _ctim(many, 15))
    got = many.download_harmonics()
    _same_harmonics(got, ref, (name, "continued"))
    assert (got["count"], got["tstp_last"]) == (5, 15)
    many.close(); one.close()


# ---- 3. the other handle kinds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["variant3d_3l", "rigid_lid_sill_2l", "biharm_island_2l", "obc_mcbc0_2l"])
def test_other_handle_kinds_equal_the_restatement(name):
    g = Golden(name)
    many, one = _engine(g), _engine(g)
    om = 2.0 * np.pi / (6.0 * float(many.p.dtd8))      # six steps to a period, so that the weights are of every size and sign
    ref = HR.Harmonics(om, 2)
    for e in (many, one):
        e.set_harmonics(om, level=2, stride=3)
    _stepped_one_by_one(many, ref, 3, name)
    one.step(1, 5); one.step(6, 7)
    _same_downloads(one.download_harmonics(), many.download_harmonics(), name)
    many.close(); one.close()


# ---- 4. bands -------------------------------------------------------------------------------------------------------------------
def _stepped(x, omega, level=2, stride=2, calls=(5, 7)):
    x.set_harmonics(omega, level, stride)
    t = 1
    for n in calls:
        x.step(t, n)
        t += n
    assert t - 1 == NSTEPS
    return x.download_harmonics()


def _bands_against_single(f, variant, nbands, omega, what, cut=None):
    e = capi.Engine(f, variant=variant)
    want = _stepped(e, omega)
    e.close()
    assert (want["count"], want["tstp_first"], want["tstp_last"]) == (6, 2, 12) and np.any(want["sum"][:, :, :, 1:] != 0.0)
    for nb in nbands:
        for overlap in (1, 0):
            many, plain = (capi.MultiEngine(f, devices=[0] * nb, variant=variant) for _ in range(2))
            assert many.count == nb
            for m in (many, plain):
                m.set_option("overlap", overlap)
            got = _stepped(many, omega)
            plain.step(1, 5); plain.step(6, 7)
            s = many.stats()
            assert s == plain.stats(), (what, nb, overlap, "harmonics changed how the bands' steps are cut")
            if cut is not None:
                assert (s["split"] >= nb * (NSTEPS - 3)) if (cut and overlap) else (s["split"] == 0), (what, nb, overlap, s)
            _same_downloads(got, want, (what, nb, overlap))
            assert many.info("harmonic_launches") == 6 * 5
            a, b = many.download(), plain.download()
            for key in ("hlay", "u", "v", "h_u", "h_v"):
                assert same_bits(a[key], b[key]), (what, nb, overlap, key)
            many.reset_harmonics()
            zero = many.download_harmonics()
            assert zero["count"] == 0 and not zero["gram"].any() and not zero["sum"].any()
            many.close(); plain.close()
    return want


def test_a_ring_of_bands_gives_the_single_handles_bits():
    """jet_2l_xyper on 2 and 3 bands: the orphan row mm+1 comes from the companion frame's own harmonics."""
    g = Golden("jet_2l_xyper")
    f = _fields(g)
    orphan = 1 + f.p.mm * (f.p.lm + 1)             # row mm+1 is masked out (it duplicates row 1) and would hold +0 only:
    f.hlay = np.array(f.hlay, dtype=np.float64)    # give it a thickness of its own, which no step changes
    f.hlay[:, orphan:] = 7.0 + np.arange(f.hlay.shape[1] - orphan)[None]
    om = 2.0 * np.pi / (5.0 * float(f.p.dtd8))
    want = _bands_against_single(f, g.variant, (2, 3), (om, 1.7 * om), "ring")
    assert same_bits(want["ref"][0][:, orphan:], f.hlay[:, orphan:]), "the orphan row did not keep its own thickness: nothing tested"


@pytest.mark.parametrize("name,nbands", [("island_3l_forced", (2, 3)), ("tide_sponge", (2,))])
def test_a_chain_of_bands_gives_the_single_handles_bits(name, nbands):
    """(tide_sponge has 10 rows: two bands of 5 are all that beom_multi_create accepts, three are refused.)"""
    g = Golden(name)
    f = _fields(g)
    w = float(f.w_ti[0])
    om = (w, 2.0 * w) if w > 0.0 else (2.0 * np.pi / (5.0 * float(f.p.dtd8)),)
    _bands_against_single(f, g.variant, nbands, om, name)


def test_cut_steps_of_bands_stay_cut():
    """The golden frames' bands are too short for a cut step (fewer than 32 rows): a closed frame of 49 x 101 cells whose
    bands are cut, with and without harmonics alike."""
    p, files = I.case_headline(48, 100, 2)
    f = read_input_data(p, files=files)
    om = 2.0 * np.pi / (5.0 * float(f.p.dtd8))
    _bands_against_single(f, 0, (2, 3), (om, 2.0 * om), "closed_2l", cut=True)


# ---- 5. no side effect ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tide_sponge", "island_3l_forced", "rigid_lid_sill_2l"])
def test_harmonics_leave_the_step_as_it_was(name):
    g = Golden(name)
    plain, har = _engine(g), _engine(g)
    har.set_harmonics((12.14,), level=2)
    plain.step(1, NSTEPS); har.step(1, NSTEPS)
    for what in ("mont_history", "plain_sweeps", "uv_fused", "stress_folded"):
        assert plain.info(what) == har.info(what), (name, what)
    a, b = plain.download(), har.download()
    for key in STATE:
        assert same_bits(a[key], b[key]), (name, key)
    assert plain.info("harmonics") == 0 and plain.info("harmonic_launches") == 0
    assert har.info("harmonic_samples") == NSTEPS and har.info("harmonic_launches") == 5 * NSTEPS      # one launch per field
    har.set_harmonics(())                                              # freed: back to a handle without harmonics
    assert har.info("harmonics") == 0 and har.info("harmonic_level") == 0 and har.info("harmonic_samples") == 0
    with pytest.raises(capi.BeomError):
        har.download_harmonics()
    plain.step(NSTEPS + 1, 2); har.step(NSTEPS + 1, 2)
    assert har.info("harmonic_launches") == 5 * NSTEPS
    a, b = plain.download(), har.download()
    for key in _live(plain, STATE):
        assert same_bits(a[key], b[key]), (name, key, "after the harmonics were freed")
    plain.close(); har.close()


def test_beside_moments_tracers_and_floats():
    """All four add-ons on one handle give the bits each gives alone."""
    g = Golden("island_3l_forced")
    f = _fields(g)
    x, y, layer = FR.seed_floats(f, 500, 3)
    q = np.ascontiguousarray(np.stack([np.asarray(f.hlay, dtype=np.float64), 0.5 * np.asarray(f.hlay, dtype=np.float64)]))
    om = 2.0 * np.pi / (5.0 * float(f.p.dtd8))

    def run(tracers, floats, moments, harmonics):
        e = _engine(g)
        if tracers:
            e.set_tracers(2)
            e.upload_tracers(q=q)
        if floats:
            e.set_floats(x, y, layer)
        if moments:
            e.set_moments(3, 3)
        if harmonics:
            e.set_harmonics((om, 3.0 * om), 1, 2)
        e.step(1, 5); e.step(6, 7)
        out = (e.download_tracers() if tracers else None, e.download_floats() if floats else None,
               e.download_moments() if moments else None, e.download_harmonics() if harmonics else None)
        if harmonics:
            assert e.info("harmonic_launches") == 3 * 6 and (e.info("moment_launches") == 4) == bool(moments)
        e.close()
        return out

    tr, fl, mo, ha = run(True, True, True, True)
    tr1, fl1, mo1, ha1 = run(True, False, False, False)[0], run(False, True, False, False)[1], run(False, False, True, False)[2], \
        run(False, False, False, True)[3]
    assert same_bits(tr["q"], tr1["q"]) and same_bits(tr["rq"], tr1["rq"])
    assert same_bits(fl["x"], fl1["x"]) and same_bits(fl["y"], fl1["y"]) and np.array_equal(fl["rejected"], fl1["rejected"])
    for k in ("ref", "sum", "sq"):
        assert same_bits(mo[k], mo1[k]), k
    assert (mo["count"], mo1["count"]) == (4, 4)
    _same_downloads(ha, ha1, "harmonics beside moments, tracers and floats")
    assert ha["count"] == 6 and np.any(ha["sum"][:, :, :, 1:] != 0.0)


def test_moments_by_caller_governs_the_samples():
    g = Golden("tide_sponge")
    e = _engine(g)
    e.set_harmonics()
    e.set_option("moments_by_caller", 1)
    e.step(1, 4)
    assert e.info("harmonic_samples") == 0 and e.info("harmonic_launches") == 0
    e.sample_harmonics(_ctim(e, 4))
    got = e.download_harmonics()
    assert (got["count"], got["tstp_first"], got["tstp_last"]) == (1, 4, 4) and same_bits(got["ref"][0], e.download(("hlay",))["hlay"])
    e.close()


# ---- 6. a fit on the device -----------------------------------------------------------------------------------------------------
def test_fit_of_uploaded_tones():
    """40 states over 1.5 periods of M2: hlay = its rest value + 0.01 cos(omega t - phi(cell)), u and v the tone alone.
    u and v carry no rounding of their own and are held to the TRUE amplitude and phase; a sample of hlay is rounded to
    half an ulp of the layer's thickness before it is taken, so hlay and the surface elevation are held to the least-squares
    fit of the very samples in long double (test_harmonics_cpu.test_short_record... has the reasoning and the figures).
    The bound is the contract's, 8 N 2^-53 max|d| / amp."""
    g = Golden("jet_2l_xyper")
    e = _engine(g)
    f = e.f
    N, om, amp0 = 40, HR.M2, 0.01
    t = np.arange(N) * (1.5 * 2.0 * np.pi / om / N)
    base = {k: np.array(getattr(f, k), dtype=np.float64) for k in STATE}
    rng = np.random.default_rng(5)
    phi = np.broadcast_to(rng.uniform(-np.pi, np.pi, base["hlay"].shape[1])[None], base["hlay"].shape)      # phi(cell)
    e.set_harmonics((om,), level=1, stride=1)
    ref = HR.Harmonics(om, 1)
    hs = []
    for n, tn in enumerate(t):
        tone = amp0 * np.cos(om * tn - phi)
        tone[:, 0] = 0.0                              # (the sentinel keeps its constants)
        st = dict(base, hlay=base["hlay"] + tone, u=tone.copy(), v=tone.copy())
        e.upload(**st)
        e.sample_harmonics(tn)
        ref.sample(st, tn)
        hs.append(st["hlay"])
        if n == 1:
            two = e.download_harmonics()
            assert two["count"] == 2 and "amp" not in two and "mean" not in two and "eta_amp" not in two
    got = e.download_harmonics()
    _same_harmonics(got, ref, "tones")
    assert got["amp"].shape == (3, 1) + phi.shape and got["eta_amp"].shape == (1,) + phi.shape
    hs = np.stack(hs)                                 # [N, nlay, n1]
    live = np.s_[:, 1:]
    # u, v against the truth
    dmax = 2.0 * amp0
    b = HR.bound(N, dmax, amp0)
    for fi in (1, 2):
        ea = np.abs(got["amp"][fi, 0] - amp0)[live] / amp0
        ep = np.abs(HR.phase_diff(got["phase"][fi, 0], phi))[live]
        print("field", fi, "amp err", ea.max(), "phase err", ep.max(), "bound", b)
        assert ea.max() <= b and ep.max() <= b, (fi, ea.max(), ep.max(), b)
    # hlay against the long-double fit of what was uploaded
    shape = phi.shape
    want = _longdouble_fit(ref, t, hs.reshape(N, -1)).reshape((3,) + shape)
    amp_w, ph_w = np.hypot(want[1], want[2]), np.arctan2(want[2], want[1]).astype(np.float64)
    dm = np.max(np.abs(hs - hs[0][None]), axis=0)
    bh = HR.bound(N, dm[live], amp0)
    ea = np.abs((got["amp"][0, 0][live] - amp_w[live]) / amp_w[live]).astype(np.float64)
    ep = np.abs(HR.phase_diff(got["phase"][0, 0], ph_w))[live]
    print("hlay amp err", ea.max(), "phase err", ep.max(), "bound", bh.min())
    assert np.all(ea <= bh) and np.all(ep <= bh)
    assert np.all(np.abs(amp_w.astype(np.float64)[live] - amp0) <= N * 2.0 ** -53 * 2.0 * np.abs(hs).max())
    # the surface elevation: the layer sums, formed exactly
    es = hs.astype(np.longdouble).sum(axis=1)         # [N, n1]
    a = _longdouble_fit(ref, t, es)
    amp_e = np.hypot(a[1], a[2]).astype(np.float64)[1:]
    dme = np.max(np.abs(es - es[0][None]), axis=0).astype(np.float64)[1:]
    be = HR.bound(N, dme, amp_e)
    ee = np.abs(got["eta_amp"][0, 0][1:] - amp_e) / amp_e
    print("eta amp err", ee.max(), "bound", be.min(), "amp", amp_e.min(), amp_e.max())
    assert np.all(amp_e > 0.0199) and np.all(ee <= be)
    e.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def _rc(call):
    with pytest.raises(capi.BeomError) as ei:
        call()
    return str(ei.value)


def test_refusals_and_errors():
    g = Golden("island_3l_forced")
    e = _engine(g)
    for what, call in {"download": e.download_harmonics, "sample": lambda: e.sample_harmonics(0.5), "reset": e.reset_harmonics}.items():
        assert "error -3" in _rc(call), (what, "without set_harmonics")
    assert "w_ti" in _rc(e.set_harmonics), "a golden without tide: omega = None has nothing to stand for"
    e.set_harmonics((3.0, 5.0), level=2, stride=4)
    e.step(1, 4)
    before = e.download_harmonics()
    assert before["count"] == 1
    nan, inf = float("nan"), float("inf")
    bad = [((1.0, 2.0, 3.0, 4.0, 5.0), 1, 1), ((3.0,), 0, 1), ((3.0,), 3, 1), ((3.0,), 1, 0), ((nan,), 1, 1), ((3.0, inf), 1, 1),
           ((0.0,), 1, 1), ((3.0, -1.0), 1, 1), ((3.0, 5.0, 3.0), 1, 1)]
    for omega, level, stride in bad:
        msg = _rc(lambda: e.set_harmonics(omega, level, stride))
        assert "error -3:" in msg and len(msg.split("error -3:")[1].strip()) > 20, (omega, level, stride, msg)
        assert (e.info("harmonics"), e.info("harmonic_level"), e.info("harmonic_samples")) == (2, 2, 1), (omega, level, stride)
    _same_downloads(e.download_harmonics(), before, "a refused set_harmonics touched the handle's harmonics")
    # any pointer may be NULL; count = 0 downloads zeros
    e.reset_harmonics()
    n = (5, 5, e.p.nlay, e.p.ndeg + 1)
    sm, count = np.full(n, 7.0), C.c_longlong(-1)
    rc = e.lib.beom_download_harmonics(e.h, None, capi._dp(sm), None, None, C.byref(count), None, None, e._err, capi.ERRLEN)
    assert rc == 0 and count.value == 0 and not sm.any()
    assert e.lib.beom_download_harmonics(e.h, None, None, None, None, None, None, None, e._err, capi.ERRLEN) == 0
    e.close()
    # a handle that holds one band's window
    from beom_amd import slab
    recipe = I.recipe_headline(150, 131, 3)
    fw, _, orphan = slab.build_band(recipe, 1, 0)
    band = capi.BandEngine(fw, recipe.p, 1, 0, device=0, rccl_id=None, orphan=orphan)
    msg = _rc(lambda: band.set_harmonics((3.0,)))
    assert "error -6:" in msg and len(msg.split("error -6:")[1].strip()) > 20, msg
    band.close()
