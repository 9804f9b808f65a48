"""Conservation integrals, the part that needs no GPU: the numpy restatement (integrals_ref) is pinned to the reference's
arithmetic through the oracle, the host-only row tree of the library (beom_integral_combine) equals the restatement's bit for
bit, and the definitions behave on the reference's own dumps."""
import numpy as np
import pytest

import integrals_ref as R
import oracle_lib
from beom_amd import capi
from helpers import Golden, golden_names, same_bits


def _fields(g):
    f = g.fields()
    f.invf = float(g.static("invf"))
    return f


def _state(g, t):
    return {k: np.ascontiguousarray(g.step(t, k), dtype=np.float64) for k in ("hlay", "u", "v")}


@pytest.mark.parametrize("name", ["jet_2l_xyper", "island_3l_forced", "random_coast_2l_xper", "sill_4l_ocrp"])
def test_restated_vorticity_equals_oracle(name):
    """rvor, pvor of the restatement against oracle_lib.Oracle.update_mont on the golden state of step 10, bit for bit."""
    g = Golden(name)
    f = _fields(g)
    st = _state(g, 10)
    o = oracle_lib.Oracle(f, variant=g.variant)
    for k in st:
        o.a[k][...] = st[k]
    for l in range(g.p.nlay):
        o.update_mont(l + 1)
        rv, pv, _, _ = R.vorticity(f, st, l)
        assert same_bits(rv[1:], o.a["rvor"][1:]), (name, l, "rvor")
        assert same_bits(pv[1:], o.a["pvor"][1:]), (name, l, "pvor")


@pytest.mark.parametrize("nrows", [1, 2, 3, 17, 64, 65, 4097])
def test_library_row_tree_equals_restatement(nrows):
    """beom_integral_combine (host only) against the restatement's tree: mixed signs, -0.0, denormals."""
    rng = np.random.default_rng(1000 + nrows)
    count = 9
    rows = rng.standard_normal((nrows, count)) * 10.0 ** rng.integers(-12, 12, size=(nrows, count))
    rows[:, 1] = -0.0                                            # a sum of -0.0 alone ...
    rows[::2, 2] = -0.0; rows[1::2, 2] = 0.0                     # ... and mixed with +0.0
    rows[:, 3] = rng.integers(-3, 4, size=nrows) * 4.9406564584124654e-324      # denormals
    rows[:, 4] = np.where(rng.random(nrows) < 0.5, -0.0, rows[:, 4])
    rows[:, 5] = rng.standard_normal(nrows) * 2.2250738585072014e-308 * 0.25
    got = capi.combine_integral_rows(rows)
    want = R.combine(rows)
    assert same_bits(got, want), (nrows, got, want)
    if nrows & (nrows - 1) == 0:
        assert np.signbit(got[1])                                # no padding: -0.0 + -0.0 stays -0.0
    else:
        assert not np.signbit(got[1])                            # a +0.0 pad joins the sum


@pytest.mark.parametrize("name", ["tc_conservation_xyper_stdfb", "tc_conservation_outcrop_3l_closed"])
def test_layer_volume_is_conserved_on_reference_dumps(name):
    """Σ mk_n*h per layer over steps 1..10 of the REFERENCE's dumps.  Measured with the restatement: layer 1 goes
    44105.028991445863 -> 44105.02899144587 (xyper_stdfb) and 29154.456707548488 -> 29154.456707548485 (outcrop_3l_closed),
    one unit in the last place; bound 8 * 2**-52 relative (the observed 1-2 ulp with head-room for the other layers, steps)."""
    g = Golden(name)
    f = _fields(g)
    steps = [t for t in range(1, 11) if "step%d_hlay" % t in g.z.files]
    assert steps[0] == 1 and steps[-1] == 10
    vol = np.array([R.integrals(f, _state(g, t))[0:4 * g.p.nlay:4] for t in steps])
    for l in range(g.p.nlay):
        rel = np.max(np.abs(vol[:, l] - vol[0, l])) / abs(vol[0, l])
        print(name, "layer", l + 1, "vol %.17g -> %.17g" % (vol[0, l], vol[-1, l]), "max relative change %.3g" % rel)
        assert rel <= 8 * 2.0 ** -52, (name, l, rel)


@pytest.mark.parametrize("name", golden_names())
def test_energy_and_enstrophy_are_finite_and_non_negative(name):
    g = Golden(name)
    f = _fields(g)
    for t in (1, 10):
        st = _state(g, t)
        s = R.integrals(f, st)
        nl = g.p.nlay
        assert np.isfinite(s).all(), (name, t, s)
        assert (s[1:4 * nl:4] >= 0).all() and (s[2:4 * nl:4] >= 0).all() and s[4 * nl] >= 0, (name, t, s)
        for l in range(nl):                                      # no cell where pvor is defined has nm = 0 or have <= 0
            _, _, have, nm = R.vorticity(f, st, l)
            bad = (f.mkpi > 0.5) & ((nm == 0) | (have <= 0))
            assert not bad[1:].any(), (name, t, l, int(bad[1:].sum()))


def test_duplicated_row_and_column_contribute_nothing():
    """jet_2l_xyper: the sums equal those over the cells with i <= lm, j <= mm, masked plainly before the tree; and without
    the rule the enstrophy would count the seam twice."""
    g = Golden("jet_2l_xyper")
    f = _fields(g)
    p = g.p
    st = _state(g, 10)
    t = R.terms(f, st, mask_duplicates=False)
    keep = (f.subc[0] <= p.lm) & (f.subc[1] <= p.mm)
    plain = R.combine(R.row_sums(f, np.where(keep[None, :], t, 0.0)))
    got = R.integrals(f, st)
    assert same_bits(got, plain)
    unmasked = R.combine(R.row_sums(f, t))
    assert (unmasked[2:4 * p.nlay:4] > got[2:4 * p.nlay:4]).all()
    for q in (0, 1, 3):                                          # mk_n, mk_u, mkpe are 0 there already
        assert same_bits(unmasked[q:4 * p.nlay:4], got[q:4 * p.nlay:4]), q
