"""One description of "everything on": the inputs of every add-on that rides on the time step, how they are applied to an
Engine or a MultiEngine, and how every download is collected into one dict.  Helper module of test_addons_kit_cpu, which holds
these inputs to their conditions without a GPU, and of test_gpu_addons_together; not a conftest, and nothing here touches a
device at import.  The generators are the suite's own: rough_inputs.rough_tracers, floats_ref.seed_floats,
forcing_cases.make_frames / with_special_entries; mix_coefficients and kappa_v_table were test_gpu_tracer_mix._coefficients
and test_gpu_tracer_vmix._kappa_v, which import them back.

Parts (Kit.apply(e, parts), Kit.collect(e, parts)):
  base          "forcing"  taus: 3 frames with special entries, cyclic with a period of 7 steps; hdot: 2 frames, not cyclic
                "tracers"  the scheme, ntrc tracers (tracer 0: q = hlay, ctrg = 1, the thickness' own history; the others
                           rough), lateral mixing (kappa, decay, source) and vertical mixing (kappa_v > 0 on every interface)
  accumulators  "moments" level 3 stride 2, "tracer_moments" level 3 stride 3, "harmonics" K = 2 level 2 stride 1
  recorders     "series" level 2 stride 1, "tracer_series" level 3 stride 2, "column_series" level 2 stride 2 on a row
                window, "tracer_column_series" level 3 stride 3 on another window, "maps" level 3 B = 8 stride 3
  floats        "floats" about 300 over all layers; "float_track" gives them a track recorder of stride 2
Every recorder holds exactly the records of steps 1..nsteps: the longest call just fits."""
import copy

import numpy as np

import floats_ref as FR
import forcing_cases as FC
import rough_inputs as RI
import tracer_mix_ref as TM
from beom_amd import inputs as I
from beom_amd.grid import read_input_data
from helpers import same_bits

NSTEPS = 12
BASE = ("forcing", "tracers")
ACCUMULATORS = ("moments", "tracer_moments", "harmonics")
RECORDERS = ("series", "tracer_series", "column_series", "tracer_column_series", "maps")
FLOATS = ("floats", "float_track")
DIAGNOSTICS = ACCUMULATORS + RECORDERS + ("floats",)            # what test (a) adds to the base one at a time
EVERYTHING = BASE + ACCUMULATORS + RECORDERS + FLOATS
NEEDS_TRACERS = ("tracers", "tracer_moments", "tracer_series", "tracer_column_series")      # (and the maps at level 3)
# what a handle kind refuses: bands keep no column series, tracer column series, maps or float track; rings nothing of tracers
REFUSED = {"single": (), "bands": ("column_series", "tracer_column_series", "maps", "float_track"),
           "ring": ("column_series", "tracer_column_series", "maps", "float_track") + NEEDS_TRACERS}
STRIDES = {"moments": 2, "tracer_moments": 3, "harmonics": 1, "series": 1, "tracer_series": 2, "column_series": 2,
           "tracer_column_series": 3, "maps": 3, "float_track": 2}
LEVELS = {"moments": 3, "tracer_moments": 3, "harmonics": 2, "series": 2, "tracer_series": 3, "column_series": 2,
          "tracer_column_series": 3, "maps": 3}
MAPS_BLOCK = 8
NFLOATS = 300
TAUS_FACTORS, TAUS_PERIOD_STEPS = (2.5, 6.0, 8.25), 7.0        # frame times in steps; steps 2 and 9 lie in the wrap interval
HDOT_FACTORS = (3.0, 8.5)
# the counters of beom_info each part moves (the recorders but the maps have none)
LAUNCHES = {"forcing": ("forcing_launches",), "tracers": ("tracer_mix_launches", "tracer_vmix_launches"),
            "moments": ("moment_launches",), "tracer_moments": ("tracer_moment_launches",),
            "harmonics": ("harmonic_launches",), "maps": ("map_launches",), "floats": ("float_launches",)}
STEP_INFOS = ("stress_folded", "plain_sweeps", "uv_fused", "mont_history")


def _ellipse(pf):
    """An elliptical island across every seam of 2 and of 3 bands (the recipe of test_gpu_tracer_series._band_fields)."""
    p, files = pf
    files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
    x = np.arange(p.lm + 2)[:, None]; y = np.arange(p.mm + 2)[None, :]
    land = ((x - 0.4 * p.lm) / (0.2 * p.lm)) ** 2 + ((y - 0.5 * p.mm) / (0.3 * p.mm)) ** 2 < 1.0
    files["h_bo"][land] = 0.0
    files["init"][land] = 0.0
    return p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"])), files


def _no_svis(pf):
    return pf[0].replace(svis="0."), pf[1]


# name: (recipe, the handle kinds the tests put it on)
FRAMES = {
    "island_ragged_3l": (lambda: _no_svis(RI._with_land(I.case_headline(200, 70, 3))), ("single",)),         # 201 x 71 x 3, embedded
    "closed_12l": (lambda: _no_svis(I.case_headline(150, 37, 12)), ("single",)),                             # per-layer launches
    "island_ragged_129x33_2l": (lambda: _no_svis(RI._with_land(I.case_headline(129, 33, 2))), ("single",)),  # the small embedded frame
    "closed_3l": (lambda: I.case_headline(150, 131, 3), ("single", "bands")),         # rows wider than a wave, 3 bands are cut
    "closed_3l_island": (lambda: _ellipse(I.case_headline(150, 131, 3)), ("single", "bands")),
    "sill_sponges": (lambda: I.case_sill_exchange3d(lm=133, mm=199, nlay=4, dt_s=0.01, npts=5, sill_halfwidth=20.0), ("single", "bands")),
    "jet_ring": (lambda: I.case_unstable_jet(lm=40, mm=96, nlay=2, dt_s=1.5), ("single", "ring")),
}
BANDED = tuple(k for k, (_, kinds) in FRAMES.items() if len(kinds) > 1)
_FIELDS = {}


def frame(name):
    """The Fields of a frame of FRAMES, built once; callers get a shallow copy and set attributes only."""
    if name not in _FIELDS:
        p, files = FRAMES[name][0]()
        _FIELDS[name] = read_input_data(p, files=files)
    return copy.copy(_FIELDS[name])


def mix_coefficients(p, ntrc=3):
    """kappa, decay, source [ntrc, nlay]: the uniform tracer diffuses at the cap; the second one with another kappa in every
    layer, a decay in layer 1 and a source in the others; the third with decay and source alone."""
    cap, dt, nl = TM.kappa_cap(p), float(p.dt), p.nlay
    kappa, decay, source = np.zeros((ntrc, nl)), np.zeros((ntrc, nl)), np.zeros((ntrc, nl))
    kappa[0] = cap
    if ntrc > 1:
        kappa[1] = cap * (0.9 - 0.6 * np.arange(nl) / max(nl - 1, 1))
        decay[1, 0] = 0.05 / dt
        source[1, 1:] = 0.02 / dt
    if ntrc > 2:
        decay[2] = 0.03 / dt
        source[2] = 0.01 / dt
    return kappa, decay, source


def kappa_v_table(p, ntrc=3):
    """[ntrc, nlay-1] in m2/s: another value for every tracer and interface, from 1e-5 (explicit would do) to dt kappa_v /
    hbar^2 far beyond any explicit limit; tracer 0 (the uniform one) gets the largest; the last tracer's row has a zero."""
    nk = p.nlay - 1
    kv = 10.0 ** (-5.0 + 6.0 * ((np.arange(ntrc)[:, None] * 5 + np.arange(nk)[None] * 3) % 7) / 6.0)
    kv[0] = 25.0 * (1.0 + np.arange(nk))
    kv[ntrc - 1, nk // 2] = 0.0
    return kv


def kind_of(e):
    """"single", "bands" or "ring" of a handle (an Engine, or a MultiEngine on a chain or on a frame periodic in y)."""
    if not e._multi:
        return "single"
    return "ring" if float(e.p.yper) > 0.5 else "bands"


def samples(stride, first, last):
    """The steps first..last a stride samples."""
    return [t for t in range(first, last + 1) if t % stride == 0]


class Kit:
    """The inputs of the full kit for the Fields f.  state: the arrays the tracers and their history are built on (hlay, rs_h;
    default: the frame's own)."""

    def __init__(self, f, seed=1, scheme=1, ntrc=3, nsteps=NSTEPS, state=None):
        self.f, self.p, self.seed, self.scheme, self.ntrc, self.nsteps = f, f.p, int(seed), int(scheme), int(ntrc), int(nsteps)
        p = f.p
        d = float(p.dtd8)
        # ---- forcing in time
        self.taus = (FC.frame_times(f, TAUS_FACTORS), FC.with_special_entries(FC.make_frames(f, "taus", seed=5 + self.seed, nfr=3)),
                     TAUS_PERIOD_STEPS * d)
        self.hdot = (FC.frame_times(f, HDOT_FACTORS), FC.make_frames(f, "hdot", seed=11 + self.seed, nfr=2), 0.0)
        # ---- tracers, on the thicknesses and the thickness history they start from
        h = np.asarray(f.hlay if state is None else state["hlay"], dtype=np.float64)
        self.q, self.rq, self.ctrg = RI.rough_tracers(f, h, self.ntrc, self.seed)
        if state is not None:
            self.rq[0] = state["rs_h"]
        self.kappa, self.decay, self.source = mix_coefficients(p, self.ntrc)
        kv = kappa_v_table(p, self.ntrc)
        self.kappa_v = np.where(kv > 0.0, kv, 3.0e-4)                # open on every interface
        # ---- accumulators
        om = 2.0 * np.pi / (5.0 * d)                                 # five steps to a period: weights of every size and sign
        self.omega = (om, 1.7 * om)
        # ---- recorders: windows strictly inside the frame
        M = p.mm + 1
        self.windows = {"column_series": (2 + M // 5, M - M // 4), "tracer_column_series": (2, 1 + M // 2)}
        self.records = {k: len(samples(STRIDES[k], 1, self.nsteps)) for k in RECORDERS + ("float_track",)}
        # ---- floats
        self.floats = FR.seed_floats(f, NFLOATS, 3 + self.seed)

    def keeps(self, kind):
        """The parts a handle kind keeps ("single", "bands", "ring"), in the forward order."""
        return tuple(k for k in EVERYTHING if k not in REFUSED[kind])

    def ctim(self, tstp):
        return FC.ctim_of(self.f, tstp)

    # ---- applying
    def apply(self, e, parts=None):
        """Applies the parts in the order given (default: all the handle keeps, forward).  "float_track" is a property of
        "floats", wherever it stands."""
        parts = self.keeps(kind_of(e)) if parts is None else tuple(parts)
        for k in parts:
            if k != "float_track":
                getattr(self, "_set_" + k)(e, parts)
        return e

    def _set_forcing(self, e, parts):
        e.set_forcing("taus", *self.taus[:2], period=self.taus[2])
        e.set_forcing("hdot", *self.hdot[:2], period=self.hdot[2])

    def _set_tracers(self, e, parts):
        e.set_tracer_scheme(self.scheme)
        e.set_tracers(self.ntrc)
        e.upload_tracers(q=self.q, rq=self.rq, ctrg=self.ctrg)
        e.set_tracer_mixing(kappa=self.kappa, decay=self.decay, source=self.source)
        e.set_tracer_vertical_mixing(self.kappa_v)

    def _set_moments(self, e, parts):
        e.set_moments(LEVELS["moments"], STRIDES["moments"])

    def _set_tracer_moments(self, e, parts):
        e.set_tracer_moments(LEVELS["tracer_moments"], STRIDES["tracer_moments"])

    def _set_harmonics(self, e, parts):
        e.set_harmonics(self.omega, LEVELS["harmonics"], STRIDES["harmonics"])

    def _set_series(self, e, parts):
        e.set_series(LEVELS["series"], STRIDES["series"], self.records["series"])

    def _set_tracer_series(self, e, parts):
        e.set_tracer_series(LEVELS["tracer_series"], STRIDES["tracer_series"], self.records["tracer_series"])

    def _set_column_series(self, e, parts):
        e.set_column_series(LEVELS["column_series"], STRIDES["column_series"], self.records["column_series"],
                            rows=self.windows["column_series"])

    def _set_tracer_column_series(self, e, parts):
        e.set_tracer_column_series(LEVELS["tracer_column_series"], STRIDES["tracer_column_series"],
                                   self.records["tracer_column_series"], rows=self.windows["tracer_column_series"])

    def _set_maps(self, e, parts):
        e.set_maps(LEVELS["maps"], MAPS_BLOCK, STRIDES["maps"], self.records["maps"])

    def _set_floats(self, e, parts):
        x, y, layer = self.floats
        if "float_track" in parts:
            e.set_floats(x, y, layer, records=self.records["float_track"], stride=STRIDES["float_track"])
        else:
            e.set_floats(x, y, layer)

    # ---- collecting
    def collect(self, e, parts=None):
        """{part: its download} and "state": every download of the parts, the state among them always."""
        parts = self.keeps(kind_of(e)) if parts is None else tuple(parts)
        out = {"state": e.download()}
        for k in parts:
            if k == "forcing":
                out[k] = e.download_forcing()
            elif k == "float_track":
                out[k] = e.download_float_track()
            else:
                out[k] = getattr(e, "download_" + k)()
        return out

    def launches(self, e, parts):
        """{counter: value} of the launch counters the parts move."""
        return {name: e.info(name) for k in parts for name in LAUNCHES.get(k, ())}


def step_calls(e, calls, first=1, between=None):
    """Steps the handle in calls of these lengths from step `first`; between(e, k) runs behind call k but the last."""
    t = first
    for k, n in enumerate(calls):
        e.step(t, n)
        t += n
        if between is not None and k + 1 < len(calls):
            between(e, k)
    return t - 1


def differences(a, b, path=""):
    """The places where two downloads differ: every float array bit for bit (helpers.same_bits), every other value and
    array by equality, dicts key by key.  [] = the same bits."""
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)) or set(a) != set(b):
            return [path + ": keys"]
        out = []
        for k in sorted(a):
            out += differences(a[k], b[k], "%s/%s" % (path, k))
        return out
    if isinstance(a, (tuple, list)):
        if not isinstance(b, (tuple, list)) or len(a) != len(b):
            return [path + ": length"]
        out = []
        for k, (x, y) in enumerate(zip(a, b)):
            out += differences(x, y, "%s[%d]" % (path, k))
        return out
    x, y = np.asarray(a), np.asarray(b)
    if x.dtype.kind == "f" and y.dtype.kind == "f" and x.dtype == y.dtype == np.float64:
        return [] if same_bits(x, y) else [path]
    if x.dtype.kind == "f" and y.dtype.kind == "f":                  # the real*4 records: bit for bit in their own width
        return [] if (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()) else [path]
    return [] if (x.shape == y.shape and bool(np.array_equal(x, y))) else [path]
