"""The output records (eta_, u___, v___), the scans (min/max, thin-layer flag) and the diag records (pvor, mont, v_cc) formed
on the device — k_out_convert, k_out_scan, k_diag_w12, k_diag_records, beom_download_outputs / beom_download_diag and their
beom_multi_ forms — against outputs_ref, the numpy restatement test_outputs_cpu pins to the real reference's files.

The restatement's input is always the handle's OWN download() (other tests hold that to the oracle), so every comparison is
exact: records as uint32, scans with ==, the flag as an integer.

A. rough states (rough_inputs) straight after creation and after step(1, 5), every handle kind, padded pitches, 1-12 layers;
B. scans of doctored states: extremes placed at the ends of the cell range, on both sides of a workgroup boundary of the
   scan, in its last workgroup, and where they must be ignored; thin cells per layer and workgroup;
C. the same on bands and on a ring of bands: extremes, and thin cells paired with a thin cell of another layer in another
   band, in the first and last owned row of every band (the rows on both sides of every seam; rows 1 and mm of the ring),
   in every band's middle row and in the orphan row mm + 1;
D. downloads between the steps of every step form disturb nothing: two handles, one of which downloads after every call."""
import ctypes as C

import numpy as np
import pytest

import outputs_cases as K
import outputs_ref as O
from beom_amd import capi
from helpers import STATE, same_bits

pytestmark = pytest.mark.gpu
CALLS_B = (2, 1, 3)
HLUV = ("hlay", "u", "v")


def _lid(x):
    return float(x.p.rgld) > 0.5


def _check_records(x, f, h0, what, diag=True):
    """Every record and scan of handle x == the restatement of its own state.  Returns the state."""
    st = x.download(HLUV)
    pi_s = x.download_pressure() if _lid(x) else None
    eta, u4, v4, mm, thin = x.download_outputs(h0)
    want = O.records(f, st["hlay"], st["u"], st["v"], h0, pi_s)
    for nm, a, b in zip(("eta", "u", "v"), (eta, u4, v4), want):
        assert np.isfinite(b).all(), what + (nm,)
        assert O.same_r4(a, b), what + (nm, int(np.sum(a.view(np.uint32) != b.view(np.uint32))))
    wmm, wthin = O.scans(f, st["hlay"], st["u"], st["v"])
    assert np.array_equal(mm, wmm), what + ("minmax", mm, wmm)
    assert int(thin) == wthin, what + ("thin", thin, wthin)
    if diag:
        for nm, a, b in zip(("pvor", "mont", "v_cc"), x.download_diag(), O.diag(f, st["hlay"], st["u"], st["v"])):
            assert np.isfinite(b).all(), what + (nm,)
            assert O.same_r4(a, b), what + (nm, int(np.sum(a.view(np.uint32) != b.view(np.uint32))))
    return st


def _engine(g, kind):
    e = capi.Engine(g, dense_hint=0 if kind == "table" else 1)
    assert bool(e.is_dense) == (kind != "table") and bool(e.is_embedded) == (kind == "embedded"), kind
    return e


# ---- A ----------------------------------------------------------------------------------------------------------------------
A_CASES = ([("dense", "closed_leith_3l", fr) for fr in ("63x7", "130x18", "192x30", "4200x9")]
           + [("dense", "jet_xyper_2l", "130x18"), ("dense", "jet_xyper_2l", "192x30"), ("dense", "soliton_xper_1l", "130x18"),
              ("dense", "closed_12l_hdot", "192x30"), ("dense", "sill_ocrp_sponge_3l", "130x18"),
              ("embedded", "island_ragged_3l", "130x18"), ("embedded", "island_ragged_3l", "192x30"),
              ("table", "island_ragged_3l", "130x18"), ("table", "closed_leith_3l", "130x18"),
              ("dense", "sponge_obc_mcbc0_2l", "130x18")])


@pytest.mark.parametrize("kind,config,frame", A_CASES)
def test_records_of_rough_states_after_creation_and_after_plan_a(kind, config, frame):
    assert (config, frame) in K.ROUGH_CASES                             # test_outputs_cpu holds this state to "rough"
    g = K.rough_state(config, frame)
    h0 = K.h0_rough(g)
    e = _engine(g, kind)
    st = _check_records(e, g, h0, (kind, config, frame, "after creation"))
    for k in HLUV:
        assert same_bits(st[k], getattr(g, k)), (kind, config, frame, k)
    first, second = e.download_outputs(h0), e.download_outputs(None)      # a second call, without h_0: the same five results
    for nm, a, b in zip(("eta", "u", "v"), first[:3], second[:3]):
        assert O.same_r4(a, b), (kind, config, frame, nm, "second call")
    assert np.array_equal(first[3], second[3]) and first[4] == second[4] == 0, (kind, config, frame, "scans of the second call")
    e.step(1, 5)
    st2 = _check_records(e, g, h0, (kind, config, frame, "after plan A"))
    assert np.isfinite(st2["hlay"]).all() and not same_bits(st2["u"], st["u"])
    e.close()


def _raw_outputs(e, h0, eta=False, u=False, v=False, scans=False, thin_only=False):
    n = (e.p.nlay, e.p.ndeg)
    bufs = [np.full(n, np.float32(7.0)) if on else None for on in (eta, u, v)]
    mm = np.full((e.p.nlay, 6), 7.0) if scans else None
    thin = C.c_int(-7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    e._check(e.lib.beom_download_outputs(e.h, ptr(h0), *[ptr(b) for b in bufs],
                                         mm.ctypes.data_as(C.POINTER(C.c_double)) if scans else None,
                                         C.byref(thin) if (scans or thin_only) else None, e._err, capi.ERRLEN))
    return bufs, mm, thin.value


@pytest.mark.parametrize("kind,config,frame", [("dense", "closed_leith_3l", "192x30"), ("embedded", "island_ragged_3l", "192x30"),
                                               ("table", "island_ragged_3l", "130x18")])
def test_argument_forms_of_the_raw_library(kind, config, frame):
    """eta alone, one velocity alone, the scans alone, the flag alone; pvor alone (k_diag_w12 is skipped), v_cc alone, mont alone."""
    g = K.rough_state(config, frame)
    h0 = K.h0_rough(g)
    e = _engine(g, kind)
    e.step(1, 5)
    st = _check_records(e, g, h0, (kind, "all arguments"))
    want = O.records(g, st["hlay"], st["u"], st["v"], h0)
    wmm, wthin = O.scans(g, st["hlay"], st["u"], st["v"])
    for q in range(3):
        on = [q == 0, q == 1, q == 2]
        bufs, mm, thin = _raw_outputs(e, None, *on)
        assert O.same_r4(bufs[q], want[q]) and all(b is None for i, b in enumerate(bufs) if i != q) and thin == -7, (kind, q)
    bufs, mm, thin = _raw_outputs(e, h0, scans=True)
    assert np.array_equal(mm, wmm) and thin == wthin == 0
    assert _raw_outputs(e, None, thin_only=True)[2] == 0
    n = (g.p.nlay, g.p.ndeg)
    e.step(6, 1)                                                        # the work arrays hold the step's own values again
    st = e.download(HLUV)
    wd = O.diag(g, st["hlay"], st["u"], st["v"])
    for q in (0, 2, 1):                                                 # pvor first: no k_diag_w12 has run since the step
        out = [np.full(n, np.float32(7.0)) if i == q else None for i in range(3)]
        e._check(e.lib.beom_download_diag(e.h, *[a.ctypes.data_as(C.c_void_p) if a is not None else None for a in out],
                                          e._err, capi.ERRLEN))
        assert O.same_r4(out[q], wd[q]), (kind, ("pvor", "mont", "v_cc")[q], "alone")
    e.close()


# ---- B ----------------------------------------------------------------------------------------------------------------------
def _scan_of(x, h0):
    """doctored state -> minmax of the handle after uploading it (the upload is read back and must hold the placed bits)."""
    def scan(doc, flag=None):
        x.upload(**doc)
        st = x.download(HLUV)
        for k in HLUV:
            assert same_bits(st[k], doc[k]), k
        _, _, _, mm, thin = x.download_outputs(h0)
        if flag is not None:
            assert int(thin) == flag, (thin, flag)
        return mm
    return scan


@pytest.mark.parametrize("kind,config,frame", K.SCAN_HANDLES)
def test_scans_find_placed_extremes_and_thin_cells(kind, config, frame):
    g = K.rough_state(config, frame)
    st = {k: getattr(g, k) for k in HLUV}
    h0 = K.h0_rough(g)
    e = _engine(g, kind)
    if kind != "table":
        ptr, layer_stride, pitch, row0 = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
        e._check(e.lib.beom_device_field(e.h, b"hlay", C.byref(ptr), C.byref(layer_stride), C.byref(pitch), C.byref(row0)))
        assert pitch.value == (g.p.lm + 1 + 15) // 16 * 16 != g.p.lm + 1      # the slots outputs_ref.slots assumes
    scan = _scan_of(e, h0)
    for rank, (cls, cell) in enumerate(K.scan_cells(g, kind).items()):
        for lay_min, lay_max in K.layer_pairs(g.p.nlay):
            doc, want = K.place_extremes(g, st, cell, rank, lay_min, lay_max)
            got = scan(doc, 0)
            assert np.array_equal(got, want), (kind, cls, cell, lay_min, lay_max, got, want)
    doc, want = K.place_ignored(g, st)
    got = scan(doc, 0)
    assert np.array_equal(got, want), (kind, "closed faces and a dry cell", got, want)
    for nm, (where, flag) in K.thin_cases(g, kind).items():
        doc = K.place_thin(g, st, where)
        e.upload(**doc)
        _check_records(e, g, h0, (kind, "thin", nm), diag=False)
        assert e.download_outputs(None)[4] == flag, (kind, nm)
    e.close()


# ---- C ----------------------------------------------------------------------------------------------------------------------
BANDS = [("closed_leith_3l", 2), ("closed_leith_3l", 3), ("island_ragged_3l", 2), ("jet_xyper_2l", 2)]


@pytest.mark.parametrize("config,nband", BANDS)
def test_records_of_bands_after_creation_and_after_plan_a(config, nband):
    g = K.rough_state(config, K.BAND_FRAME)
    h0 = K.h0_rough(g)
    many = capi.MultiEngine(g, devices=[0] * nband)
    assert many.count == nband and many.describe()["ring"] == int(float(g.p.yper) > 0.5)
    _check_records(many, g, h0, (config, nband, "after creation"))
    many.step(1, 5)
    _check_records(many, g, h0, (config, nband, "after plan A"))
    many.close()


@pytest.mark.parametrize("config,nband", BANDS)
def test_scans_of_bands_find_placed_extremes_and_thin_cells(config, nband):
    g = K.rough_state(config, K.BAND_FRAME)
    st = {k: getattr(g, k) for k in HLUV}
    h0 = K.h0_rough(g)
    mm, nl = int(g.p.mm), int(g.p.nlay)
    ring = float(g.p.yper) > 0.5
    many = capi.MultiEngine(g, devices=[0] * nband)
    bands = [many.band(k) for k in range(nband)]
    assert bands[0]["own0"] == 1 and all(bands[k + 1]["own0"] == bands[k]["own1"] + 1 for k in range(nband - 1))
    assert bands[-1]["own1"] == (mm if ring else mm + 1)
    rows = sorted({r for b in bands for r in (b["own0"], b["own1"])} | ({1, mm, mm + 1} if ring else set()))
    scan = _scan_of(many, h0)
    counted = K.check_row_placements(g, st, rows, scan=lambda doc: scan(doc, 0))
    assert counted >= 6 * 2 * (len(rows) - 2), (rows, counted)
    # thin cells: every band's edge rows and middle row against another band's middle row, in different layers
    own = [(b["own0"], b["own1"]) for b in bands]
    mid = [(a + b) // 2 for a, b in own]
    if not ring:                                                      # a middle row is no other band's ghost row: the merge decides
        for k, r in enumerate(mid):
            assert all(not (b["win0"] <= r <= b["win1"]) for i, b in enumerate(bands) if i != k), (k, r, bands)
    cases = K.band_thin_cases(g, own)
    assert len(cases) >= 6 * nband
    for nm, (where, flag) in cases.items():
        doc = K.place_thin(g, st, where)
        assert O.scans(g, doc["hlay"], doc["u"], doc["v"])[1] == flag, (config, nm)
        many.upload(**doc)
        _check_records(many, g, h0, (config, nband, "thin", nm), diag=False)
        assert many.download_outputs(h0)[4] == flag, (config, nband, nm)
    many.close()


# ---- D ----------------------------------------------------------------------------------------------------------------------
LIVE_SCRATCH = ("mont", "rvor", "pvor", "dive")        # d2hx, d2hy are the work arrays of the diag records (dead between steps)
# name: (configuration, handle: a kind of single handle or ("bands", n), options)
FORMS = {
    "closed_leith_3l": ("closed_leith_3l", "dense", {}),
    "closed_leith_3l_keep_diag": ("closed_leith_3l", "dense", {"keep_diag": 1}),
    "closed_svis_3l": ("closed_svis_3l", "dense", {}),
    "closed_dt3d_forced_3l": ("closed_dt3d_forced_3l", "dense", {}),
    "stommel_wind_drag": ("stommel_wind_drag", "dense", {}),
    "closed_12l_hdot": ("closed_12l_hdot", "dense", {}),
    "island_ragged_3l": ("island_ragged_3l", "embedded", {}),
    "island_ragged_3l_table": ("island_ragged_3l", "table", {}),
    "two_bands": ("closed_leith_3l", ("bands", 2), {}),
    "ring": ("jet_xyper_2l", ("bands", 2), {}),             # periodic in y: its bands form a ring
}


def _same_handles(a, b, what, lid=False):
    """STATE, and on a single handle the live scratch (and the lid pressure), hold the same bits on both handles.  A frame cut
    into bands compares STATE only: the library has no download of the bands' scratch arrays."""
    sa, sb = a.download(), b.download()
    for k in STATE:
        assert same_bits(sa[k], sb[k]), what + (k,)
    if isinstance(a, capi.Engine):
        ca, cb = a.download_scratch(), b.download_scratch()
        for k in LIVE_SCRATCH + (("d2hx", "d2hy") if lid else ()):
            assert same_bits(ca[k], cb[k]), what + ("scratch", k)
    if lid:
        assert same_bits(a.download_pressure(), b.download_pressure()), what + ("pi_s",)


@pytest.mark.parametrize("form", list(FORMS))
def test_downloads_between_steps_disturb_nothing(form):
    """Plan B (steps 7-12 in calls of 2, 1, 3) and two steps more on two handles of the same rough state; one forms every
    record after every call.  After each call both hold the same bits (_same_handles: bands compare STATE only), so no step
    read what a download wrote, and the records equal the restatement of that state."""
    config, handle, opts = FORMS[form]
    banded = isinstance(handle, tuple)
    frame = K.BAND_FRAME if banded else "130x18"
    g = K.rough_state(config, frame)
    assert (config, frame) in K.ROUGH_CASES                              # test_outputs_cpu holds this very state to "rough"
    h0 = K.h0_rough(g)
    make = (lambda: capi.MultiEngine(g, devices=[0] * handle[1])) if banded else (lambda: _engine(g, handle))
    a, b = make(), make()
    for x in (a, b):
        for k, v in opts.items():
            x.set_option(k, v)
    t, seen, cc = 7, [], []
    for n in CALLS_B + (2,):
        a.step(t, n); b.step(t, n)
        t += n
        st = _check_records(a, g, h0, (form, t - 1))
        assert np.isfinite(st["hlay"]).all()
        _same_handles(a, b, (form, t - 1))
        seen.append((a.info("mont_history"), b.info("mont_history")))
        cc.append(a.download(("v_cc",))["v_cc"])
    if form == "closed_leith_3l":
        assert seen[2] == (1, 1) and seen[3] == (1, 1), seen          # the downloads ran between steps of the history-from-Montgomery form
        assert same_bits(cc[0], g.v_cc) and same_bits(cc[3], g.v_cc)  # the fused pair does not keep its viscosity
    if form == "closed_leith_3l_keep_diag":                           # ... and with keep_diag = 1 it does, anew in every call
        assert not same_bits(cc[0], g.v_cc) and not same_bits(cc[1], cc[0]) and not same_bits(cc[3], cc[2])
    if form == "closed_dt3d_forced_3l":                               # viscosity and stress every third step only: steps 9 and 12
        assert g.p.n_3d == 3
        assert not same_bits(cc[1], cc[0]) and not same_bits(cc[2], cc[1]) and same_bits(cc[3], cc[2])
    if form == "stommel_wind_drag":
        assert a.info("stress_folded") == 1
    if form == "closed_svis_3l":
        assert a.info("biharm_tiled") == 1
    if form == "ring":
        assert a.describe()["ring"] == 1
    if banded:
        assert a.count == handle[1]
    a.close(); b.close()


def test_downloads_between_steps_of_a_rigid_lid_handle():
    """The lid's diag records work in pcd / qlr (its next step reads the stored curvatures d2hx, d2hy of the last layer)."""
    from beom_amd import inputs as I
    from beom_amd.grid import read_input_data
    p, files = I.case_sill_exchange3d(lm=133, mm=41, nlay=3, dt_s=0.01, npts=5, sill_halfwidth=6.0)
    f = read_input_data(p.replace(rgld="1."), files=files)
    h0 = np.ascontiguousarray(f.h_0[:, 1:], dtype=np.float32)
    a, b = capi.Engine(f), capi.Engine(f)
    t = 1
    for n in (3, 4, 3):
        a.step(t, n); b.step(t, n)
        t += n
        _check_records(a, f, h0, ("lid", t - 1))
        eta = a.download_outputs(None)[0]
        assert O.same_r4(eta[0], a.download_pressure()[1:].astype(np.float32)) and np.any(eta[0] != 0), ("lid", t - 1, "eta[0] is pi_s")
        _same_handles(a, b, ("lid", t - 1), lid=True)
    a.close(); b.close()
