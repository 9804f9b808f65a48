"""The maps (beom_set_maps), the part that needs no GPU: the numpy restatement (maps_ref) pinned to the yardsticks that already
exist — the column series' restatement where one block covers the frame, the integrals' restatement through the tree over
all blocks, a cell count, a unit tracer and a scalar loop with explicit recursion — on rough states (tests/rough_inputs.py),
a frame periodic both ways and a frame with land among them."""
import numpy as np
import pytest

import column_series_ref as CS
import integrals_ref as R
import maps_ref as MR
import rough_inputs as RI
from helpers import same_bits

FIELDS = ("hlay", "u", "v", "h_u", "h_v")
CONFIGS = ["island_ragged_3l", "jet_xyper_2l"]                 # (land; both periodic seams with their duplicates)


def _rough(config, frame):
    g = RI.rough_fields(RI.base_fields(config, frame), 1)
    return g, {k: getattr(g, k) for k in FIELDS}


# ---- 1. one block over the frame is the column series' total ------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
def test_one_block_over_the_frame_is_the_column_series_total(config):
    """B = 64 on a 64 x 8 frame: the same terms in the same order, rows then columns; the extra +0.0 padding changes no bit
    of a non-zero sum."""
    g, st = _rough(config, "63x7")
    p, nl = g.p, g.p.nlay
    assert p.lm + 1 <= 64 and p.mm + 1 <= 64
    rec = MR.record(g, st, 2, 64)
    assert rec.shape == (MR.count(0, nl, 2), 1, 1)
    v = MR.views(rec, 0, nl, 2)
    cols = CS.column_record(g, st, 2)
    tot = CS.total(cols, nl)
    tu, tv = R.tree(cols[:, 4 * nl + 1:5 * nl + 1].T), R.tree(cols[:, 5 * nl + 1:].T)
    for want in (tot[0:4 * nl:4], tot[1:4 * nl:4], tu, tv):
        assert np.all(want != 0.0)
    assert same_bits(v["h"][:, 0, 0], tot[0:4 * nl:4]) and same_bits(v["ke"][:, 0, 0], tot[1:4 * nl:4])
    assert same_bits(v["hu"][:, 0, 0], tu) and same_bits(v["hv"][:, 0, 0], tv)


# ---- 2. the tree over all blocks against the integrals ------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 8])
@pytest.mark.parametrize("config", CONFIGS)
def test_tree_over_the_blocks_is_within_the_bound_of_the_integrals(config, B):
    """Two pairwise summations of the same terms in different orders: within 2 * ceil(log2(L*M)) * 2^-53 * sum |terms|."""
    g, st = _rough(config, "130x18")
    p, nl = g.p, g.p.nlay
    v = MR.views(MR.record(g, st, 2, B), 0, nl, 2)
    want = R.integrals(g, st)
    t = np.abs(R.terms(g, st)).sum(axis=1)
    D = int(np.ceil(np.log2((p.lm + 1) * (p.mm + 1))))
    for name, k in (("h", 0), ("ke", 1)):
        got = R.tree(R.tree(v[name]))                          # blocks of a block row, then the block rows
        bound = 2.0 * D * 2.0 ** -53 * t[k:4 * nl:4]
        diff = np.abs(got - want[k:4 * nl:4])
        print(config, B, name, "|diff| =", diff, "bound =", bound)
        assert np.all(want[k:4 * nl:4] != 0.0) and np.all(diff <= bound), (name, diff, bound)


# ---- 3. n is the live-cell count ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 8, 64])
@pytest.mark.parametrize("config", CONFIGS)
def test_n_is_the_count_of_live_cells(config, B):
    g, st = _rough(config, "130x18")
    p = g.p
    n = MR.record(g, st, 1, B)[0]
    live = ~MR.duplicates(g)
    I, J = (g.subc[0] - 1) // B, (g.subc[1] - 1) // B
    want = np.zeros_like(n)
    for ipnt in np.nonzero(live)[0]:
        want[J[ipnt], I[ipnt]] += 1.0
    assert same_bits(n, want)
    assert n.sum() == p.ndeg - (MR.duplicates(g).sum() - 1)    # packed cells minus duplicates (the sentinel is no cell)
    if config == "island_ragged_3l" and B == 2:
        assert (n == 0.0).any(), "no block lies wholly on land: nothing tested"
        assert not np.signbit(n).any()
    if config == "jet_xyper_2l":                               # the duplicated column and row count nothing
        assert n.sum() == p.lm * p.mm


# ---- 4. a unit tracer's content is the thickness ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 8])
@pytest.mark.parametrize("config", CONFIGS)
def test_unit_tracer_is_the_thickness(config, B):
    """q = hlay: level 3's q equals h bit for bit in every block whose live cells all have mk_n = 1 (h's term is mk_n * hlay)."""
    g, st = _rough(config, "130x18")
    nl = g.p.nlay
    q = np.asarray(st["hlay"], dtype=np.float64)[None]
    rec = MR.record(g, st, 3, B, q)
    assert rec.shape[0] == MR.count(1, nl, 3)
    v = MR.views(rec, 1, nl, 3)
    dry = MR.block_sums(MR.rectangle(g, np.where(MR.duplicates(g) | (g.mk_n > 0.5), 0.0, 1.0)[None]), B)[0]
    ok = dry == 0.0
    wet = ok & (v["n"] > 0.0)
    assert wet.any() and np.all(v["h"][:, wet] != 0.0) and not v["h"][:, ok & ~wet].any()
    assert same_bits(v["q"][0][:, ok], v["h"][:, ok])
    assert same_bits(rec[:1 + 6 * nl], MR.record(g, st, 2, B))


# ---- 5. the array form is a scalar loop with explicit recursion ---------------------------------------------------------------
def _tree_rec(vals):
    if len(vals) == 1:
        return float(vals[0])
    h = len(vals) // 2
    return _tree_rec(vals[:h]) + _tree_rec(vals[h:])


@pytest.mark.parametrize("B", [2, 8])
@pytest.mark.parametrize("config", CONFIGS)
def test_array_form_is_a_scalar_loop(config, B):
    g, st = _rough(config, "130x18")
    p = g.p
    t = MR.terms(g, st, 2)
    rec = MR.record(g, st, 2, B)
    cell = {(int(g.subc[0, ip]), int(g.subc[1, ip])): ip for ip in range(1, p.ndeg + 1)}
    Mc, Lc = rec.shape[1:]
    blocks = [(0, 0), (Mc - 1, Lc - 1), (Mc // 2, Lc // 2), (Mc - 1, 0), (1, Lc - 1)]      # corners (partial blocks) and the middle
    for J, I in blocks:
        for k in range(t.shape[0]):
            cols = []
            for a in range(B):
                i = I * B + a + 1
                col = []
                for b in range(B):
                    ip = cell.get((i, J * B + b + 1), 0)
                    col.append(float(t[k, ip]) if ip else 0.0)
                cols.append(_tree_rec(col))
            want = _tree_rec(cols)
            assert same_bits(np.float64(rec[k, J, I]), np.float64(want)), (J, I, k)
    assert rec[1:].any()
