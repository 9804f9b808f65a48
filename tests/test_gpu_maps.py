"""The maps on the device (beom_set_maps, include/beom_hip.h) against the numpy restatement (maps_ref.record) applied to the
state downloaded at the record's step.  Every comparison with the restatement is helpers.same_bits: the order of summation
(inside an aligned block the rows of each column, then the columns, both by the pairwise tree) is the contract, so a dense
handle, an embedded one and the table path give the same bits, whatever the division into calls."""
import numpy as np
import pytest

import maps_ref as MR
import rough_inputs as RI
from beom_amd import capi, inputs as I
from beom_amd.grid import read_input_data
from helpers import Golden, same_bits
from test_gpu_biharm_tiled import CASES
from test_gpu_integrals import _case as _integrals_case, _fields
from test_gpu_series import _refusal
from test_gpu_tracer_series import _with_tracers

pytestmark = pytest.mark.gpu
FIELDS = ("hlay", "u", "v", "h_u", "h_v")

BAD_ARGS = ("beom_set_maps: level %d, block %d, stride %d, %d records (level 0..3, block a power of two in 2..64, "
            "stride >= 1, records >= 1)")
OVERFLOW = ("beom_step: steps %d..%d would write %d records of the maps (stride %d) but the recorder holds %d of %d: "
            "empty it with beom_download_maps, or take fewer steps per call")
NONE = "beom_download_maps: the handle keeps no maps (beom_set_maps)"
SAMPLE = "beom_sample_maps (maps set? recorder full?)"
NO_TRACER = "beom_set_maps: the handle carries no tracer (beom_set_tracers comes first)"
ON_BANDS = ("%s: a handle on bands keeps no maps (a block's tree must not cross a seam between bands, and nothing "
            "aligns the seams to the block edge yet); use a single handle (beom_set_maps)")


def _case(name):
    if name == "smaller_than_a_block":                  # 20 x 9 cells: one partial block of 64 x 64
        p, files = I.case_headline(19, 8, 2)
        return read_input_data(p.replace(svis="0."), files=files)
    return _integrals_case(name)


_TWINS = {}


def _twin_states(name, n):
    """(fields, [the state after step 1..n]) of a handle without maps, stepped once per case and kept."""
    if name not in _TWINS:
        f = _case(name)
        twin = capi.Engine(f)
        states = []
        for t in range(1, n + 1):
            twin.step(t, 1)
            states.append(twin.download(FIELDS))
        twin.close()
        _TWINS[name] = (f, states)
    f, states = _TWINS[name]
    assert len(states) >= n
    return f, states


def _maps_of(e, calls, level, block, stride=1, records=16):
    e.set_maps(level, block, stride, records)
    t = 1
    for n in calls:
        e.step(t, n)
        t += n
    return e.download_maps()


def _same_views(got, k, want, ntrc, nl, level, what):
    v = MR.views(want, ntrc, nl, level)
    for name, a in v.items():
        assert same_bits(got[name][k], a), (what, name)
    assert set(got) == set(v) | {"count", "tstp", "block", "raw"}


# ---- 1. levels 1 and 2 on each handle kind ------------------------------------------------------------------------------------
# (the block edge is a run-time argument that drives both the tree over a block's rows and the cross-lane steps over its
# columns: one frame meets every edge)
RECORD_CASES = [(name, B) for name in ("jet_xyper_2l", "island_ragged_3l", "closed_12l", "soliton_xper", "wide_67_chunks")
                for B in (2, 8, 64)] + [("smaller_than_a_block", 64)] + [("island_ragged_3l", B) for B in (4, 16, 32)]


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name,B", RECORD_CASES)
def test_records_on_each_handle_kind(name, B, level):
    calls = (4, 2)
    n = sum(calls)
    f, states = _twin_states(name, n)
    p, nl = f.p, f.p.nlay
    Lc, Mc = -(-(p.lm + 1) // B), -(-(p.mm + 1) // B)
    e, tab = capi.Engine(f), capi.Engine(f, dense_hint=0)
    assert e.is_dense and not tab.is_dense
    if name in CASES:
        assert e.is_embedded == CASES[name][1]
    a, b = _maps_of(e, calls, level, B), _maps_of(tab, calls, level, B)
    cnt = MR.count(0, nl, level)
    assert cnt == e.lib.beom_maps_count(0, nl, level)
    for got in (a, b):
        assert got["count"] == n and list(got["tstp"]) == list(range(1, n + 1)) and got["block"] == B
        assert got["raw"].shape == (n, cnt, Mc, Lc)
    assert same_bits(a["raw"], b["raw"]), (name, B, level, "dense vs table path")
    for k in range(n):
        want = MR.record(f, states[k], level, B)
        assert np.isfinite(want).all()
        assert same_bits(a["raw"][k], want), (name, B, level, k + 1)
        _same_views(a, k, want, 0, nl, level, (name, B, level, k + 1))
    assert a["h"][-1].any() and a["u"][-1].any() and a["v"][-1].any(), (name, "no velocity anywhere: nothing tested")
    if level == 2:
        assert a["ke"][-1].any() and a["hu"][-1].any() and a["hv"][-1].any(), (name, "no transport anywhere: nothing tested")
    else:
        assert "ke" not in a and "hu" not in a
    if name == "island_ragged_3l" and B == 2:
        assert (a["n"][-1] == 0.0).any(), "no block lies wholly on land"
    if name == "smaller_than_a_block":
        assert (Mc, Lc) == (1, 1)
    assert e.info("map_launches") == n
    e.close(); tab.close()


# ---- 2. the reference's own configurations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rigid_lid_sill_2l", "variant3d_3l", "biharm_island_2l", "obc_mcbc0_2l"])
def test_goldens_level_2(name):
    g = Golden(name)
    f = _fields(g)
    e = capi.Engine(f, variant=g.variant)
    e.set_maps(2, 8, 1, 5)
    want = []
    for t in range(1, 6):
        e.step(t, 1)
        want.append(MR.record(f, e.download(FIELDS), 2, 8))
    got = e.download_maps()
    assert got["count"] == 5 and list(got["tstp"]) == [1, 2, 3, 4, 5]
    assert np.isfinite(got["raw"]).all()
    for k in range(5):
        assert same_bits(got["raw"][k], want[k]), (name, k + 1)
    assert got["hu"].any() and got["hv"].any() and got["u"].any() and got["v"].any(), (name, "nothing moves: nothing tested")
    e.close()


# ---- 3. level 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [1, 2])
@pytest.mark.parametrize("ntrc", [1, 3])
def test_level_3(ntrc, scheme):
    f = _case("island_ragged_3l")
    nl = f.p.nlay
    for dense_hint, B in ((1, 8), (0, 2), (1, 64)):
        e = _with_tracers(capi.Engine(f, dense_hint=dense_hint), f, ntrc)
        e.set_tracer_scheme(scheme)
        e.set_maps(3, B, 1, 4)
        assert e.info("maps") == 3 and e.info("maps_block") == B
        want = []
        for t in range(1, 4):
            e.step(t, 1)
            want.append(MR.record(f, e.download(FIELDS), 3, B, e.download_tracers()["q"]))
        got = e.download_maps()
        assert got["count"] == 3 and got["raw"].shape[1] == MR.count(ntrc, nl, 3) == e.lib.beom_maps_count(ntrc, nl, 3)
        for k in range(3):
            assert same_bits(got["raw"][k], want[k]), (ntrc, scheme, dense_hint, B, k + 1)
            _same_views(got, k, want[k], ntrc, nl, 3, (ntrc, scheme, dense_hint, B, k + 1))
        assert got["q"][-1].any() and got["q"].shape[1:3] == (ntrc, nl)
        # a tracer whose content is the thickness: q == h bit for bit in the blocks whose live cells all have mk_n = 1
        st = e.download(FIELDS)
        trc = e.download_tracers()
        q = trc["q"].copy()
        q[0] = st["hlay"]
        e.upload_tracers(q=q, rq=trc["rq"])
        e.sample_maps()
        got = e.download_maps()
        assert list(got["tstp"]) == [3]
        assert same_bits(got["raw"][0], MR.record(f, st, 3, B, q))
        dry = MR.block_sums(MR.rectangle(f, np.where(MR.duplicates(f) | (f.mk_n > 0.5), 0.0, 1.0)[None]), B)[0]
        wet = (dry == 0.0) & (got["n"][0] > 0.0)
        assert (wet.any() or B == 64) and np.all(got["h"][0][:, wet] != 0.0)      # (every 64 x 64 block of this frame touches its rim)
        assert same_bits(got["q"][0, 0][:, wet], got["h"][0][:, wet])
        e.close()


def test_level_3_needs_tracers_and_follows_their_count():
    f = _case("island_ragged_3l")
    e = capi.Engine(f)
    assert _refusal(lambda: e.set_maps(3, 8), -3) == NO_TRACER
    assert e.info("maps") == 0
    _with_tracers(e, f, 2)
    e.set_maps(3, 8, 1, 4)
    e.step(1, 2)
    assert e.info("maps") == 3 and e.info("maps_records") == 2
    _with_tracers(e, f, 2)                              # the same count: the recorder stays
    assert e.info("maps") == 3 and e.info("maps_records") == 2
    _with_tracers(e, f, 3)                              # another count frees it
    assert e.info("maps") == 0 and e.info("maps_block") == 0
    assert _refusal(e.download_maps, -3) == NONE
    e.set_maps(2, 8, 1, 4)                              # levels 1 and 2 do not look at the tracers
    e.set_tracers(1)
    assert e.info("maps") == 2
    e.close()


# ---- 4. division into calls, stride, the entry by hand ------------------------------------------------------------------------
def test_division_into_calls_and_stride():
    f = _case("jet_xyper_2l")
    runs = []
    for calls in ((12,), (5, 7), (1,) * 12):
        e = capi.Engine(f)
        runs.append(_maps_of(e, calls, 2, 8))
        e.close()
    for r in runs:
        assert list(r["tstp"]) == list(range(1, 13))
        assert same_bits(r["raw"], runs[0]["raw"])
    e = capi.Engine(f)
    r3 = _maps_of(e, (5, 7), 2, 8, stride=3)
    assert list(r3["tstp"]) == [3, 6, 9, 12]
    assert same_bits(r3["raw"], runs[0]["raw"][2::3])
    # the download has emptied the recorder
    assert e.info("maps") == 2 and e.info("maps_block") == 8 and e.info("maps_records") == 0
    again = e.download_maps()
    assert again["count"] == 0 and again["raw"].shape[0] == 0 and again["tstp"].size == 0
    # one record by hand, under the last step's number, whatever the stride; an upload leaves it where it is
    e.sample_maps()
    assert e.info("maps_records") == 1
    e.upload(**e.download())
    assert e.info("maps_records") == 1
    got = e.download_maps()
    assert got["count"] == 1 and list(got["tstp"]) == [12]
    assert same_bits(got["raw"][0], runs[0]["raw"][11])
    # other arguments reallocate and empty; level 0 frees
    e.sample_maps()
    e.set_maps(1, 2, 2, 3)
    assert e.info("maps") == 1 and e.info("maps_block") == 2 and e.info("maps_records") == 0
    e.step(13, 4)
    got = e.download_maps()
    assert list(got["tstp"]) == [14, 16] and got["raw"].shape[1] == MR.count(0, f.p.nlay, 1) and got["block"] == 2
    assert same_bits(got["raw"][1], MR.record(f, e.download(FIELDS), 1, 2))
    e.set_maps(0)
    assert e.info("maps") == 0 and e.info("maps_block") == 0
    assert _refusal(e.download_maps, -3) == NONE
    e.close()


@pytest.mark.parametrize("config", ["jet_xyper_2l", "island_ragged_3l"])
def test_rough_state_by_hand_at_every_block_edge(config):
    """The rough state of rough_inputs as uploaded (no step) on frame 321 x 50, where interior waves exist: every block edge
    2..64 at level 2 on the dense or embedded handle and on the table path equals the restatement and differs from the
    record with h_u and h_v swapped.  jet_xyper_2l: values put into the duplicated column and row (the steps leave +0 there)
    contribute +0.0."""
    g = RI.rough_fields(RI.base_fields(config, "321x50"), 1)
    p, nl = g.p, g.p.nlay
    dup = MR.duplicates(g)
    dup[0] = False
    assert dup.any() == (config == "jet_xyper_2l")
    for k, val in (("u", 0.75), ("v", -1.25), ("h_u", 1.5), ("h_v", -2.5)):
        setattr(g, k, np.where(dup[None, :], val, getattr(g, k)))
    for dense_hint in (1, 0):
        e = capi.Engine(g, dense_hint=dense_hint)
        assert bool(e.is_dense) == bool(dense_hint) and e.is_embedded == (config == "island_ragged_3l" and dense_hint == 1)
        st = e.download(FIELDS)
        for k in FIELDS:
            assert same_bits(st[k], getattr(g, k)), k
        for B in (2, 4, 8, 16, 32, 64):
            e.set_maps(2, B, 1, 1)
            e.sample_maps()
            got = e.download_maps()
            assert list(got["tstp"]) == [0] and got["block"] == B
            want = MR.record(g, st, 2, B)
            assert np.isfinite(want).all()
            assert same_bits(got["raw"][0], want), (config, dense_hint, B)
            assert not same_bits(got["raw"][0], MR.record(g, dict(st, h_u=st["h_v"], h_v=st["h_u"]), 2, B)), (config, dense_hint, B)
            _same_views(got, 0, want, 0, nl, 2, (config, dense_hint, B))
            assert got["u"][0].any() and got["v"][0].any() and got["hu"][0].any() and got["hv"][0].any() and got["ke"][0].any()
            if config == "jet_xyper_2l" and B <= 8:           # (no land, no wall: every block of an interior wave carries transport)
                inner = got["hu"][0][:, :(p.mm // B), :(p.lm // B)]
                assert np.all(inner != 0.0) and np.all(inner[:, :, 1:] != inner[:, :, :-1])
        e.close()


# ---- 5. overflow and bad arguments --------------------------------------------------------------------------------------------
def test_refusals():
    f = _case("island_ragged_3l")
    e = capi.Engine(f)
    assert _refusal(e.download_maps, -3) == NONE
    assert _refusal(e.sample_maps, -3) == SAMPLE
    for args in ((4, 8, 1, 4), (-1, 8, 1, 4), (1, 0, 1, 4), (1, 3, 1, 4), (2, 128, 1, 4), (2, 1, 1, 4), (1, 8, 0, 4), (2, 8, 1, 0)):
        assert _refusal(lambda: e.set_maps(*args), -3) == BAD_ARGS % args, args
    assert e.info("maps") == 0
    e.step(1, 3)
    e.set_maps(2, 8, 1, 4)
    before = e.download(("hlay", "u", "v"))
    assert _refusal(lambda: e.step(4, 5), -3) == OVERFLOW % (4, 8, 5, 1, 0, 4)
    after = e.download(("hlay", "u", "v"))
    for k in before:
        assert same_bits(before[k], after[k]), k
    assert e.info("maps_records") == 0
    e.step(4, 4)                                                # the next smaller call runs
    assert e.info("maps_records") == 4
    assert _refusal(e.sample_maps, -3) == SAMPLE                # a full recorder
    assert _refusal(lambda: e.step(8, 1), -3) == OVERFLOW % (8, 8, 1, 1, 4, 4)
    assert e.info("maps_records") == 4
    got = e.download_maps()
    assert list(got["tstp"]) == [4, 5, 6, 7]
    e.step(8, 1)                                                # the same step is taken once the recorder is empty
    assert list(e.download_maps()["tstp"]) == [8]
    e.close()


# ---- 6. bands refuse ----------------------------------------------------------------------------------------------------------
def test_handles_on_bands_refuse():
    f = _case("closed_12l")
    many = capi.MultiEngine(f, devices=[0, 0])
    assert _refusal(lambda: many.set_maps(2), -6) == ON_BANDS % "beom_multi_set_maps"
    assert _refusal(many.download_maps, -6) == ON_BANDS % "beom_multi_download_maps"
    many.close()


# ---- 7. nothing changes without it --------------------------------------------------------------------------------------------
def test_state_does_not_depend_on_the_maps():
    f = _case("island_ragged_3l")
    never, freed, kept = capi.Engine(f), capi.Engine(f), capi.Engine(f)
    freed.set_maps(2, 8, 1, 4)
    freed.step(1, 2)
    freed.set_maps(0)
    never.step(1, 2)
    kept.set_maps(2, 8, 2, 4)
    kept.step(1, 2)
    for e in (never, freed, kept):
        e.step(3, 4)
    assert never.info("map_launches") == 0 and freed.info("map_launches") == 2 and kept.info("map_launches") == 3
    a = never.download()
    for e in (freed, kept):
        b = e.download()
        for k in a:
            assert same_bits(a[k], b[k]), k
    assert list(kept.download_maps()["tstp"]) == [2, 4, 6]
    for e in (never, freed, kept):
        e.close()
