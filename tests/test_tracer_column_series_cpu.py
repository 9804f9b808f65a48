"""The tracer column series' contract on the CPU (include/beom_hip.h, "Tracer column series"): the numpy restatement
(tracer_column_series_ref) tied to things already pinned, not to itself.

  identity      with q = hlay the restatement's fu, fv ARE column_series_ref's tu, tv, inv = var = its vol, and the bounds are
                1.0 (or +inf, -inf where a column has no wet cell): on the reference's own states of two goldens.
  liveness      what the rough tracer field has to show before any device comparison means something.
  cross-check   the tree over the columns of inv against the tracer series' total, within the bound of two pairwise trees.
  presence      the library exports the new symbols and the binding has the methods.

No GPU."""
import ctypes as C

import numpy as np
import pytest

import column_series_ref as CS
import integrals_ref as R
import tracer_column_series_ref as TC
import tracer_series_ref as TS
from beom_amd import capi
from helpers import Golden, same_bits
from test_tracer_series_cpu import _fields, rough_case


# ---- (a) the identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 10])
@pytest.mark.parametrize("name", ["jet_2l_xyper", "island_3l_forced"])
def test_a_tracer_equal_to_hlay_has_the_column_series_transports(name, step):
    """q = hlay on the reference's own state: c is exactly 1 in every wet cell, so every face with a wet cell on either side
    carries h_u * 1 = h_u.  The preconditions are test_tracer_series_cpu's: every live water cell has hlay > 0, and every live
    face that carries a transport has a wet cell on one side.  vol = the column sums of mk_n * hlay, inv those of hlay over the
    live cells: equal because a live cell with mk_n = 0 has hlay = +0 (checked)."""
    g = Golden(name)
    f = _fields(g)
    st = {k: np.ascontiguousarray(g.step(step, k), dtype=np.float64) for k in ("hlay", "u", "v", "h_u", "h_v")}
    nl, L, M = f.p.nlay, f.p.lm + 1, f.p.mm + 1
    live = TS.live_mask(f)
    wet = st["hlay"] > 0.0
    water = np.asarray(f.mk_n) > 0.5
    assert np.all(wet[:, live & water]), (name, "a live water cell without thickness")
    assert not np.any(st["hlay"][:, live & ~water]), (name, "a live cell with mk_n = 0 that has thickness")
    W_, S_ = f.neig[:, 4].astype(np.int64), f.neig[:, 6].astype(np.int64)
    for key, back in (("h_u", W_), ("h_v", S_)):
        stranded = (st[key] != 0.0) & ~(wet | wet[:, back]) & live[None]
        assert not stranded.any(), (name, key, "a live face that carries a transport between two dry cells")
    q = st["hlay"][None].copy()
    rec = TC.column_record(f, st["hlay"], st["h_u"], st["h_v"], q, 3)
    assert rec.shape == (L, TC.count(1, nl, 3))
    v = TC.views(rec, 1, nl, 3)
    cs = CS.column_record(f, st, 2)
    tu, tv, vol = cs[:, 4 * nl + 1:5 * nl + 1], cs[:, 5 * nl + 1:], cs[:, 0:4 * nl:4]
    assert same_bits(v["fu"][:, 0], tu), (name, "fu against tu")
    assert same_bits(v["fv"][:, 0], tv), (name, "fv against tv")
    # (the jet's first step carries no transport in y yet)
    assert (tu.any() and tv.any()) if step == 10 else (tu.any() or tv.any()), (name, "no transport anywhere: nothing tested")
    assert same_bits(v["inv"], v["var"]), name
    assert same_bits(v["inv"][:, 0], vol), (name, "inv against vol")
    icol = f.subc[0] - 1
    for l in range(nl):
        has_wet = np.bincount(icol[1:][(wet[l] & live)[1:]], minlength=L) > 0
        assert has_wet.any()
        assert np.all(v["cmin"][has_wet, 0, l] == 1.0) and np.all(v["cmax"][has_wet, 0, l] == 1.0), (name, l)
        assert np.all(v["cmin"][~has_wet, 0, l] == np.inf) and np.all(v["cmax"][~has_wet, 0, l] == -np.inf), (name, l)
    # the levels are prefixes of each other, entry by entry
    for level in (1, 2):
        lo = TC.column_record(f, st["hlay"], st["h_u"], st["h_v"], q, level)
        assert same_bits(lo.reshape(L, 1, nl, 2 * level), rec.reshape(L, 1, nl, 6)[..., :2 * level]), (name, level)


# ---- (b) the rough tracer field ---------------------------------------------------------------------------------------------
def test_the_rough_record_is_rough():
    g, st, q = rough_case()
    nl, ntrc = g.p.nlay, q.shape[0]
    rec = TC.column_record(g, st["hlay"], st["h_u"], st["h_v"], q, 3)
    v = TC.views(rec, ntrc, nl, 3)
    assert np.isfinite(rec.reshape(-1, 6)[:, :4]).all()
    for k in TC.NAMES:
        differs = np.mean(v[k][1:] != v[k][:-1])
        print("%s: columns differ from their western neighbour at %.1f %% of the places" % (k, 100.0 * differs))
        assert differs >= 0.8, (k, differs)
    assert np.isfinite(v["cmin"]).any() and np.any(v["cmin"] == np.inf), "the bounds are all finite or all infinite"
    assert np.isfinite(v["cmax"]).any() and np.any(v["cmax"] == -np.inf)
    # a row window changes the record and leaves sums that are not zero
    w = TC.column_record(g, st["hlay"], st["h_u"], st["h_v"], q, 3, (5, 11))
    assert not same_bits(w, rec)
    vw = TC.views(w, ntrc, nl, 3)
    for k in ("inv", "var", "fu", "fv"):
        assert vw[k].any() and not same_bits(vw[k], v[k]), k
    # h_u and h_v are told apart
    s = TC.views(TC.column_record(g, st["hlay"], st["h_v"], st["h_u"], q, 3), ntrc, nl, 3)
    assert not same_bits(s["fu"], v["fu"]) and not same_bits(s["fv"], v["fv"])
    assert same_bits(s["inv"], v["inv"]) and same_bits(s["cmax"], v["cmax"])


# ---- (c) the cross-check with the tracer series -----------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["island_ragged_3l", "jet_xyper_2l"])
def test_total_is_within_the_bound_of_the_tracer_series(config):
    """total adds along columns first, the tracer series' along rows first: two pairwise trees over the same terms x_q, each
    entry within 2 * gamma_D * sum |x_q| (tracer_column_series_ref.gamma_bound)."""
    g, st, q = rough_case(config)
    nl, ntrc = g.p.nlay, q.shape[0]
    args = (g, st["hlay"], st["h_u"], st["h_v"], q)
    a = TC.total(TC.column_record(*args, 1), ntrc, nl, 1)
    b = TS.total(TS.row_record(*args, 1), ntrc, nl, 1)
    bound = TC.gamma_bound(*args)
    assert a.shape == b.shape == bound.shape == (ntrc, nl) and np.all(bound > 0.0)
    print("%s: |columns first - rows first| / bound =" % config, np.abs(a - b) / bound)
    assert np.all(np.abs(a - b) <= bound)
    assert same_bits(a, R.tree(np.moveaxis(TC.views(TC.column_record(*args, 3), ntrc, nl, 3)["inv"], 0, -1)))


# ---- (d) presence -----------------------------------------------------------------------------------------------------------
def test_library_and_binding_have_the_tracer_column_series():
    want = {"beom_set_tracer_column_series", "beom_sample_tracer_column_series", "beom_download_tracer_column_series",
            "beom_multi_set_tracer_column_series", "beom_multi_download_tracer_column_series"}
    assert set(capi.TRACER_COLUMN_SERIES_EXPORTS) == want and want <= set(capi.EXPORTS)
    lib = capi.load()
    for name in want:
        assert getattr(lib, name).restype is C.c_int, name
    for meth in ("set_tracer_column_series", "sample_tracer_column_series", "download_tracer_column_series"):
        assert callable(getattr(capi.Engine, meth)), meth
    for cls in (capi.MultiEngine, capi.BandEngine):
        for meth in ("set_tracer_column_series", "download_tracer_column_series"):
            assert callable(getattr(cls, meth)), (cls.__name__, meth)


def test_null_handle_is_refused():
    lib = capi.load()
    err = C.create_string_buffer(200)
    assert lib.beom_set_tracer_column_series(None, 1, 1, 1, 1, 1, err, 199) == -1
    assert lib.beom_sample_tracer_column_series(None) == -1
    assert lib.beom_download_tracer_column_series(None, None, None, None, err, 199) == -1
    assert lib.beom_multi_set_tracer_column_series(None, 1, 1, 1, 1, 1, err, 199) == -1
    assert lib.beom_multi_download_tracer_column_series(None, None, None, None, err, 199) == -1
