"""The flux-limited tracer scheme (scheme 2) without a GPU: its numpy restatement (tracers_limited_ref) pinned to the reference
through the oracle — a tracer of uniform concentration 1 IS the layer thickness, bit for bit —, its conservation, what it buys
(sharpness) and what it keeps (bounds) on a uniform flow, the mix of limiter outcomes that the GPU test's input produces, and
the ctypes prototypes of the new calls against the header."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import tracers_limited_ref as TL
import tracers_ref as T
from beom_amd import capi
from helpers import Golden, same_bits
from test_tracers_cpu import _CTYPE, PIN, _fields, _prototypes

NSTEPS = 40
GPU_GOLDENS = ("stommel_24x16", "soliton_31x15_xper", "jet_2l_xyper", "island_3l_forced", "random_coast_2l_xper", "sill_4l_ocrp",
               "tc_wave_sponge", "obc_mcbc0_2l", "biharm_island_2l", "tide_sponge")
OPEN_EVERYWHERE = ("jet_2l_xyper", "tc_wave_sponge")       # no land, no closed edge: the fallback never happens


def _drive(f, o, q, rq, ctrg, nsteps, after):
    """nsteps of the oracle with the scheme-2 tracer update in front of each step's update_h; after(t, q, rq) once per step."""
    for t in range(1, nsteps + 1):
        if t <= 3:
            o.rebuild_fluxes()
        gene, ramp, ctim = T.step_scalars(f.p, t, float(getattr(f, "tres", 0.0)))
        st = o.state()
        q, rq = TL.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, gene, ramp, ctim, scheme=2)
        o.step(t, 1)
        after(t, q, rq)
    return q, rq


@pytest.mark.parametrize("name", PIN)
def test_uniform_tracer_is_the_oracles_layer_thickness(name):
    g = Golden(name)
    assert not g.uses_cos(), name
    f = _fields(g)
    o = oracle_lib.Oracle(f, variant=g.variant)
    q = np.array(f.hlay, dtype=np.float64)[None].copy()
    rq = np.array(f.rs_h, dtype=np.float64)[None].copy()
    ctrg = np.ones_like(q)

    def after(t, q, rq):
        assert same_bits(q[0][:, 1:], o.state()["hlay"][:, 1:]), (name, t)

    _drive(f, o, q, rq, ctrg, NSTEPS, after)


@pytest.mark.parametrize("name", ["stommel_24x16", "jet_2l_xyper", "tc_conservation_xyper_stdfb"])
def test_wavy_tracer_keeps_its_content(name):
    g = Golden(name)
    f = _fields(g)
    assert not np.any(f.nudg) and not (f.has.get("hdot", False) and np.any(f.hdot)), name
    o = oracle_lib.Oracle(f, variant=g.variant)
    q = (TL.wavy(f) * f.hlay)[None].copy()
    rq = np.zeros(q.shape + (2,))
    total0 = np.sum(f.mk_n * q[0], axis=1)
    assert (total0 > 0).all()
    worst = [0.0]

    def after(t, q, rq):
        total = np.sum(f.mk_n * q[0], axis=1)
        worst[0] = max(worst[0], float(np.max(np.abs(total - total0) / total0)))

    _drive(f, o, q, rq, None, NSTEPS, after)
    print("%s: max relative drift of sum(mk_n * q) over %d steps = %.3g" % (name, NSTEPS, worst[0]))
    assert worst[0] <= 1e-13, (name, worst[0])


# ---- a uniform flow over the frame of jet_2l_xyper: sharpness and bounds -------------------------------------------------------
def _uniform_flow(sign):
    f = _fields(Golden("jet_2l_xyper"))
    assert not np.any(f.nudg) and not (f.has.get("hdot", False) and np.any(f.hdot)) and not (f.has.get("tide", False) and np.any(f.tide))
    p = f.p
    wet = np.arange(p.ndeg + 1) > 0
    hlay = np.tile(np.where(wet, 100.0, 0.0), (p.nlay, 1))
    u0, v0 = sign * 0.1 * float(p.dl) / float(p.dt), sign * 0.05 * float(p.dl) / float(p.dt)
    h_u = np.tile(100.0 * u0 * f.mk_u, (p.nlay, 1))
    h_v = np.tile(100.0 * v0 * f.mk_v, (p.nlay, 1))
    return f, hlay, h_u, h_v


def _shapes(f):
    i, j = f.subc[0].astype(np.float64), f.subc[1].astype(np.float64)
    box = np.where((np.abs(i - 8) <= 3) & (np.abs(j - 8) <= 3), 1.0, 0.0)
    gauss = np.exp(-((i - 8) ** 2 + (j - 8) ** 2) / 8.0)
    box[0] = gauss[0] = 0.0
    return {"box": box, "gaussian": gauss}


def _advect(f, hlay, h_u, h_v, c0, scheme, nsteps=100):
    q = (c0[None] * hlay)[None].copy()
    rq = np.zeros(q.shape + (2,))
    lo, hi = np.inf, -np.inf
    for t in range(1, nsteps + 1):
        gene = 0.0 if t <= 3 else float(f.p.g_fb)
        q, rq = TL.update(f, hlay, h_u, h_v, q, rq, None, gene, 1.0, 0.0, scheme=scheme)
        c = q[0][:, 1:] / hlay[:, 1:]
        lo, hi = min(lo, float(c.min())), max(hi, float(c.max()))
    c = q[0][:, 1:] / hlay[:, 1:]
    kept = float(np.sum(f.mk_n[1:] * c * c) / np.sum(f.mk_n[1:] * c0[None, 1:] ** 2 * np.ones_like(c)))
    return lo, hi, kept, float(c.max())


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("shape", ["box", "gaussian"])
def test_limited_scheme_is_sharper_and_keeps_bounds(shape, sign):
    f, hlay, h_u, h_v = _uniform_flow(sign)
    c0 = _shapes(f)[shape]
    lo2, hi2, kept2, max2 = _advect(f, hlay, h_u, h_v, c0, 2)
    _, _, kept1, max1 = _advect(f, hlay, h_u, h_v, c0, 1)
    print("%s sign %+.0f: scheme 1 max c %.3f variance kept %.3f | scheme 2 max c %.3f variance kept %.3f, min c %.3g, max c - 1 %.3g"
          % (shape, sign, max1, kept1, max2, kept2, lo2, hi2 - 1.0))
    assert lo2 >= -1e-12 and hi2 <= 1.0 + 1e-12, (shape, sign, lo2, hi2)
    assert kept2 >= 1.5 * kept1, (shape, sign, kept1, kept2)


# ---- what the GPU test feeds the kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPU_GOLDENS)
def test_wavy_input_reaches_every_outcome_of_the_limiter(name):
    g = Golden(name)
    f = _fields(g)
    o = oracle_lib.Oracle(f, variant=g.variant)
    o.step(1, 6)
    st = o.state()
    n = TL.outcomes(f, st["hlay"], st["h_u"], st["h_v"], TL.wavy(f) * st["hlay"])
    faces = sum(n.values())
    share = {k: n[k] / faces for k in TL.OUTCOMES}
    print(name, faces, " ".join("%s %.1f%%" % (k, 100 * share[k]) for k in TL.OUTCOMES))
    for k in TL.OUTCOMES[1:]:
        assert share[k] >= 0.04, (name, k, share)
    if name in OPEN_EVERYWHERE:
        assert n["fallback"] == 0, (name, share)
    else:
        assert share["fallback"] >= 0.03, (name, share)


# ---- the binding --------------------------------------------------------------------------------------------------------------
NEW = ("beom_set_tracer_scheme", "beom_multi_set_tracer_scheme")


def test_ctypes_prototypes_match_the_header():
    protos = _prototypes()
    lib = capi.load()
    for name in NEW:
        assert name in protos and name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == [_CTYPE[t] for t in protos[name]], (name, protos[name], fn.argtypes)
    assert protos["beom_set_tracer_scheme"] == ["beom_handle", "int", "char *", "int"]
    assert protos["beom_multi_set_tracer_scheme"] == ["beom_multi_handle", "int", "char *", "int"]


def test_null_handle_is_refused():
    lib = capi.load()
    err = C.create_string_buffer(200)
    assert lib.beom_set_tracer_scheme(None, 2, err, 199) == -1
    assert lib.beom_multi_set_tracer_scheme(None, 2, err, 199) == -1
    assert lib.beom_set_tracer_scheme(None, 1, err, 199) == -1


def test_unknown_scheme_is_refused():
    """The scheme is looked at before the handle, so this needs no device."""
    lib = capi.load()
    err = C.create_string_buffer(200)
    for scheme in (0, 3):
        assert lib.beom_set_tracer_scheme(None, scheme, err, 199) == -3
        assert b"scheme" in err.value
        assert lib.beom_multi_set_tracer_scheme(None, scheme, err, 199) == -3
