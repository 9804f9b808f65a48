"""The tracer series' contract on the CPU (include/beom_hip.h, "Tracer series"): the numpy restatement (tracer_series_ref) tied
to things already pinned, not to itself.

  identity      with q = hlay the restatement's fu, fv ARE series_ref's tu, tv, inv = var = the row sums of hlay, and the
                bounds are 1.0: on the reference's own states of two goldens.
  liveness      what the rough tracer field has to show before any device comparison means something.
  count         beom_tracer_series_count of the library against the restatement's.
  conservation  total (the tree over the rows of inv) of a patchy tracer stays constant to rounding in a closed frame.

rough_case() is also what test_gpu_tracer_series uploads.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import integrals_ref as R
import oracle_lib
import rough_inputs as RI
import series_ref as S
import tracer_series_ref as TS
import tracers_ref as T
from beom_amd import capi
from helpers import Golden, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(g):
    f = g.fields()
    f.invf = float(g.static("invf"))
    return f


# ---- (a) the identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 10])
@pytest.mark.parametrize("name", ["jet_2l_xyper", "island_3l_forced"])
def test_a_tracer_equal_to_hlay_has_the_series_transports(name, step):
    """q = hlay on the reference's own state: c is exactly 1 in every wet cell, so every face with a wet cell on either side
    carries h_u * 1 = h_u.  The identity rests on every live water cell (mk_n = 1) having hlay > 0 and on every live face that
    carries a transport having a wet cell on one side: both checked first.  (Every live cell having hlay > 0 does not hold on
    island_3l_forced: the rim cells of a closed frame are packed cells with mk_n = 0 and hlay = +0, and the reference stores a
    transport at 24 resp. 27 of them in layers 1 and 3 — through a face whose other side is a wet cell, so cf is still 1.)"""
    g = Golden(name)
    f = _fields(g)
    st = {k: np.ascontiguousarray(g.step(step, k), dtype=np.float64) for k in ("hlay", "h_u", "h_v")}
    nl, M = f.p.nlay, f.p.mm + 1
    live = TS.live_mask(f)
    wet = st["hlay"] > 0.0
    water = np.asarray(f.mk_n) > 0.5
    assert np.all(wet[:, live & water]), (name, "a live water cell without thickness")
    W_, S_ = f.neig[:, 4].astype(np.int64), f.neig[:, 6].astype(np.int64)
    for key, back in (("h_u", W_), ("h_v", S_)):
        stranded = (st[key] != 0.0) & ~(wet | wet[:, back]) & live[None]
        assert not stranded.any(), (name, key, "a live face that carries a transport between two dry cells")
    q = st["hlay"][None].copy()
    rec = TS.row_record(f, st["hlay"], st["h_u"], st["h_v"], q, 3)
    assert rec.shape == (M, TS.count(1, nl, 3))
    v = TS.views(rec, 1, nl, 3)
    tutv = R.row_sums(f, S.transport_terms(f, st))                       # [M, 2*nlay]: tu per layer, then tv
    assert same_bits(v["fu"][:, 0], tutv[:, :nl]), (name, "fu against tu")
    assert same_bits(v["fv"][:, 0], tutv[:, nl:]), (name, "fv against tv")
    assert np.any(tutv[:, :nl] != 0.0) and np.any(tutv[:, nl:] != 0.0), (name, "no transport anywhere: nothing tested")
    assert same_bits(v["inv"], v["var"]), name
    hsum = R.row_sums(f, np.where(live[None], st["hlay"], 0.0))
    assert same_bits(v["inv"][:, 0], hsum), (name, "inv against the row sums of hlay")
    jrow = f.subc[1] - 1
    for l in range(nl):
        has_wet = np.bincount(jrow[1:][(wet[l] & live)[1:]], minlength=M) > 0
        assert has_wet.any()
        assert np.all(v["cmin"][has_wet, 0, l] == 1.0) and np.all(v["cmax"][has_wet, 0, l] == 1.0), (name, l)
        assert np.all(v["cmin"][~has_wet, 0, l] == np.inf) and np.all(v["cmax"][~has_wet, 0, l] == -np.inf), (name, l)
    # the levels are prefixes of each other, entry by entry
    for level in (1, 2):
        lo = TS.row_record(f, st["hlay"], st["h_u"], st["h_v"], q, level)
        assert same_bits(lo.reshape(M, 1, nl, 2 * level), rec.reshape(M, 1, nl, 6)[..., :2 * level]), (name, level)


# ---- (b) the rough tracer field ---------------------------------------------------------------------------------------------
_ROUGH = {}


def rough_case(config="island_ragged_3l", frame="130x18", ntrc=3, seed=1):
    """(g, st, q): a rough state of rough_inputs on the configuration's frame with one cell-layer in twenty dried up (hlay = +0
    exactly), and ntrc rough tracers: concentrations in [-0.4, 1.2], a content stranded in the dry cell-layers (it reads as
    concentration +0), a few contents of exactly -0 in wet cells (concentration -0: the bounds see +0), and in row 5, layer 1,
    tracer 0 nothing above zero, so that the row's maximum is one of those zeros.  Built once per argument set."""
    key = (config, frame, ntrc, seed)
    if key not in _ROUGH:
        g = RI.rough_fields(RI.base_fields(config, frame), seed)
        r = np.random.default_rng([seed, 4217])
        h = np.array(g.hlay, dtype=np.float64)
        dry = r.uniform(0.0, 1.0, h.shape) < 0.05
        h[dry] = 0.0
        c = r.uniform(-0.4, 1.2, (ntrc,) + h.shape)
        row5 = g.subc[1] == 5
        c[0, 0, row5] = -np.abs(c[0, 0, row5])
        q = np.where(dry[None], r.uniform(-0.01, 0.01, c.shape), c * h[None])
        q = np.where((r.uniform(0.0, 1.0, c.shape) < 0.02) & ~dry[None], -0.0, q)
        q[0, 0] = np.where(row5 & (g.subc[0] % 7 == 3) & ~dry[0], -0.0, q[0, 0])
        q[..., 0] = 0.0
        st = {"hlay": h, "h_u": np.ascontiguousarray(g.h_u, dtype=np.float64), "h_v": np.ascontiguousarray(g.h_v, dtype=np.float64)}
        _ROUGH[key] = (g, st, np.ascontiguousarray(q))
    return _ROUGH[key]


@pytest.mark.parametrize("config", ["island_ragged_3l", "jet_xyper_2l"])
def test_the_rough_record_is_rough(config):
    g, st, q = rough_case(config)
    p, nl, ntrc = g.p, g.p.nlay, q.shape[0]
    rec = TS.row_record(g, st["hlay"], st["h_u"], st["h_v"], q, 3)
    v = TS.views(rec, ntrc, nl, 3)
    inner = rec[1:p.mm]                                                    # (rows 2..mm: the first and last may be rim or duplicate)
    differs = np.mean(inner[1:] != inner[:-1])
    print("%s: rows differ from their southern neighbour at %.1f %% of the places" % (config, 100.0 * differs))
    assert differs >= 0.8, (config, differs)
    for k in ("fu", "fv", "inv", "var"):
        assert np.all(v[k][1:p.mm] != 0.0), (config, k, "a row sum that is zero")
    assert np.mean(v["cmin"][1:p.mm] < v["cmax"][1:p.mm]) > 0.9, config
    x, xb, wet = TS.cell_terms(g, st["hlay"], st["h_u"], st["h_v"], q)
    c = T.concentration(st["hlay"][None], q)[0]
    assert np.any(c[:, wet] < 0.0), "no negative concentration in a live wet cell"
    neg0 = (c == 0.0) & np.signbit(c) & wet[None]
    assert neg0.any(), "no concentration of -0 in a live wet cell"
    assert not np.any(np.signbit(xb[neg0])), "c + 0.0 kept a -0"
    assert np.any(~wet[:, 1:] & TS.live_mask(g)[None, 1:]), "no live dry cell: the wet rule is not exercised"
    # row 5, layer 1, tracer 0: nothing above zero, a -0 among the concentrations, and the maximum is +0
    sel = wet[0] & (g.subc[1] == 5)
    assert sel.any() and np.all(c[0, 0, sel] <= 0.0) and neg0[0, 0, sel].any(), config
    top = v["cmax"][4, 0, 0]
    assert top == 0.0 and not np.signbit(top), (config, top)


# ---- (c) the count ----------------------------------------------------------------------------------------------------------
def test_the_librarys_count_is_the_restatements():
    lib = capi.load()
    for ntrc in (1, 3, 8):
        for nlay in (1, 4, 12):
            for level in (1, 2, 3):
                assert lib.beom_tracer_series_count(ntrc, nlay, level) == TS.count(ntrc, nlay, level) == ntrc * nlay * 2 * level


# ---- (d) conservation -------------------------------------------------------------------------------------------------------
NSTEPS = 10
DRIFT_BOUND = 6.1e-16


def test_total_stays_constant_in_a_closed_frame():
    """stommel_24x16: closed, no sponge, no hdot, no mixing, no decay.  A patchy tracer stepped by tracers_ref in front of every
    oracle step; total[t, l] = the tree over the rows of inv of the record behind each step.  The flux form telescopes, so
    the total moves by rounding only: every step rounds each of the 425 contents once (2^-53 relative) and the tree rounds
    log2 of as many partial sums.  Measured on the CPU with this restatement over these 10 steps: max |total - total0| / total0
    = 1.51e-16 (one ulp of the total).  The bound is four times that, 6.1e-16: room for a few more of the same roundings, none
    for a lost cell (one cell of 425 is 2e-3 of the total)."""
    g = Golden("stommel_24x16")
    f = _fields(g)
    assert float(f.p.xper) < 0.5 and float(f.p.yper) < 0.5
    assert not np.any(f.nudg) and not (f.has.get("hdot", False) and np.any(f.hdot))
    o = oracle_lib.Oracle(f, variant=g.variant)
    nl = f.p.nlay
    q = (T.patchy(f) * f.hlay)[None].copy()
    rq = np.zeros(q.shape + (2,))
    st = o.state()
    total0 = TS.total(TS.row_record(f, st["hlay"], st["h_u"], st["h_v"], q, 1), 1, nl, 1)
    assert total0.shape == (1, nl) and np.all(total0 > 0.0)
    worst, moved = 0.0, False
    for t in range(1, NSTEPS + 1):
        if t <= 3:
            o.rebuild_fluxes()
        gene, ramp, ctim = T.step_scalars(f.p, t, float(getattr(f, "tres", 0.0)))
        st = o.state()
        qn, rq = T.update(f, st["hlay"], st["h_u"], st["h_v"], q, rq, None, gene, ramp, ctim)
        moved = moved or bool(np.any(qn != q))
        q = qn
        o.step(t, 1)
        st = o.state()
        rec = TS.row_record(f, st["hlay"], st["h_u"], st["h_v"], q, 2)
        total = TS.total(rec, 1, nl, 2)
        worst = max(worst, float(np.max(np.abs(total - total0) / total0)))
    print("stommel_24x16: max |total - total0| / total0 over %d steps = %.3g (bound %.3g)" % (NSTEPS, worst, DRIFT_BOUND))
    assert moved, "the tracer never moved: nothing tested"
    assert worst <= DRIFT_BOUND, worst


# ---- the header and the binding ---------------------------------------------------------------------------------------------
_CTYPE = {"beom_handle": C.c_void_p, "beom_multi_handle": C.c_void_p, "int": C.c_int, "double *": C.POINTER(C.c_double),
          "int *": C.POINTER(C.c_int), "char *": C.c_char_p}


def test_header_states_the_contract_and_the_binding_matches_it():
    want = {"beom_tracer_series_count", "beom_set_tracer_series", "beom_sample_tracer_series", "beom_download_tracer_series",
            "beom_band_set_tracer_series", "beom_multi_set_tracer_series", "beom_multi_download_tracer_series"}
    assert set(capi.TRACER_SERIES_EXPORTS) == want and want <= set(capi.EXPORTS)
    txt = open(os.path.join(ROOT, "include", "beom_hip.h")).read()
    for word in ("trc_conc", "trc_face", "x_b  = c + 0.0", "+inf", "beom_download_tracer_series", "tracer_series_records"):
        assert word in txt, word
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint\s+(beom_\w+)\s*\(([^)]*)\)\s*;", code):
        protos[name] = [" ".join(re.match(r"^\s*(.*?)(\w+)\s*$", " ".join(a.split())).group(1).split()) for a in args.split(",")]
    lib = capi.load()
    for name in want:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert list(fn.argtypes) == [_CTYPE[t] for t in protos[name]], (name, protos[name], fn.argtypes)
    for cls in (capi.Engine, capi.MultiEngine):
        for meth in ("set_tracer_series", "download_tracer_series"):
            assert callable(getattr(cls, meth)), (cls.__name__, meth)
    assert callable(capi.Engine.sample_tracer_series)


def test_null_handle_is_refused():
    lib = capi.load()
    err = C.create_string_buffer(200)
    assert lib.beom_set_tracer_series(None, 1, 1, 1, err, 199) == -1
    assert lib.beom_band_set_tracer_series(None, 1, 1, 1, 1, 1, err, 199) == -1
    assert lib.beom_sample_tracer_series(None) == -1
    assert lib.beom_download_tracer_series(None, None, None, None, err, 199) == -1
    assert lib.beom_multi_set_tracer_series(None, 1, 1, 1, err, 199) == -1
    assert lib.beom_multi_download_tracer_series(None, None, None, None, err, 199) == -1
