"""Passive tracers without a GPU: the numpy restatement of the scheme (tracers_ref) pinned to the reference through the
oracle — a tracer of uniform concentration 1 IS the layer thickness, bit for bit — its conservation, and the ctypes
prototypes of the new calls against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib
import tracers_ref as T
from beom_amd import capi
from helpers import Golden, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEPS = 40
PIN = ("jet_2l_xyper", "soliton_31x15_xper", "tc_conservation_xyper_stdfb", "stommel_24x16", "island_3l_forced", "sill_2l_ocrp",
       "random_coast_2l_xper", "tc_wave_sponge", "obc_mcbc0_2l", "tc_outcrop_seamount_5l", "carrier_beach", "tc_lock_exchange",
       "biharm_island_2l")


def _fields(g):
    f = g.fields()
    f.invf = float(g.static("invf"))
    return f


def _drive(f, o, q, rq, ctrg, nsteps, after):
    """nsteps of the oracle with the tracer update in front of each step's update_h; after(t, q, rq) once per step."""
    for t in range(1, nsteps + 1):
        if t <= 3:
            o.rebuild_fluxes()                      # what the step is about to do itself (:2166-2177): the same values
        gene, ramp, ctim = T.step_scalars(f.p, t, float(getattr(f, "tres", 0.0)))
        st = o.state()
        q, rq = T.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, ctrg, gene, ramp, ctim)
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
def test_patchy_tracer_keeps_its_content(name):
    g = Golden(name)
    f = _fields(g)
    assert not np.any(f.nudg) and not (f.has.get("hdot", False) and np.any(f.hdot)), name
    o = oracle_lib.Oracle(f, variant=g.variant)
    q = (T.patchy(f) * f.hlay)[None].copy()
    rq = np.zeros(q.shape + (2,))
    total0 = np.sum(f.mk_n * q[0], axis=1)
    assert (total0 > 0).all()
    worst = [0.0]

    def after(t, q, rq):
        total = np.sum(f.mk_n * q[0], axis=1)
        rel = float(np.max(np.abs(total - total0) / total0))
        worst[0] = max(worst[0], rel)

    _drive(f, o, q, rq, None, NSTEPS, after)
    print("%s: max relative drift of sum(mk_n * q) over %d steps = %.3g" % (name, NSTEPS, worst[0]))
    assert worst[0] <= 1e-13, (name, worst[0])


# ---- the binding --------------------------------------------------------------------------------------------------------------
NEW = ("beom_set_tracers", "beom_upload_tracers", "beom_download_tracers", "beom_update_tracers",
       "beom_multi_set_tracers", "beom_multi_upload_tracers", "beom_multi_download_tracers")
_CTYPE = {"beom_handle": C.c_void_p, "beom_multi_handle": C.c_void_p, "int": C.c_int, "double": C.c_double,
          "const double *": C.POINTER(C.c_double), "double *": C.POINTER(C.c_double), "char *": C.c_char_p}


def _prototypes():
    txt = open(os.path.join(ROOT, "include", "beom_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(beom_\w+)\s*\(([^)]*)\)\s*;", txt):
        types = []
        for a in args.split(","):
            m = re.match(r"^\s*(.*?)(\w+)\s*$", " ".join(a.split()))
            types.append(" ".join(m.group(1).split()))
        out[name] = types
    return out


def test_ctypes_prototypes_match_the_header():
    protos = _prototypes()
    lib = capi.load()
    for name in NEW:
        assert name in protos and name in capi.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == [_CTYPE[t] for t in protos[name]], (name, protos[name], fn.argtypes)
    txt = open(os.path.join(ROOT, "include", "beom_hip.h")).read()
    assert re.search(r"#define\s+BEOM_MAX_TRACERS\s+8\b", txt) and capi.BEOM_MAX_TRACERS == 8
    assert re.search(r"#define\s+BEOM_ABI_VERSION\s+2\b", txt)


def test_null_handle_is_refused():
    lib = capi.load()
    err = C.create_string_buffer(200)
    assert lib.beom_set_tracers(None, 1, err, 199) == -1
    assert lib.beom_upload_tracers(None, None, None, None, err, 199) == -1
    assert lib.beom_download_tracers(None, None, None, err, 199) == -1
    assert lib.beom_update_tracers(None, 0.0, 1.0, 0.0) == -1
    assert lib.beom_multi_set_tracers(None, 1, err, 199) == -1
    assert lib.beom_multi_upload_tracers(None, None, None, None, err, 199) == -1
    assert lib.beom_multi_download_tracers(None, None, None, err, 199) == -1
