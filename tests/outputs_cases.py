"""The states test_outputs_cpu and test_gpu_outputs feed the output kernels with (helper module, not a conftest): the rough
states by name, a rough h_0, where the scan tests place extremes and thin cells — by device slot on a single handle, by rows
of the frame on bands — and what the scans must then return, worked out from the masks alone.  Reads the init mirror's
Fields through rough_inputs; the arithmetic of the records is outputs_ref's."""
import numpy as np

import rough_inputs as RI
from outputs_ref import F4, F8, scan_masks, scans

BLOCK = 256                     # threads per workgroup of the scan: one partial result per BLOCK device slots


def h0_rough(f, seed=11):
    """h_0 in real*4 plus noise of +-1 m per cell and layer (so that no eta is a round number or a copy of its neighbour)."""
    r = np.random.default_rng([seed, 4321])
    h0 = np.asarray(f.h_0, dtype=F8)[:, 1:]
    return np.ascontiguousarray((h0 + r.uniform(-1.0, 1.0, h0.shape)).astype(F4))


def slots(f, kind):
    """(device slot of every packed cell 0..ndeg, last slot): kind "table" keeps the packed order; "dense" / "embedded" handles
    keep cell (i, j) at i + (j - 1) * P with the row pitch P = lm + 1 rounded up to 16."""
    p = f.p
    n1 = int(p.ndeg) + 1
    if kind == "table":
        return np.arange(n1, dtype=np.int64), int(p.ndeg)
    L = int(p.lm) + 1
    P = (L + 15) // 16 * 16
    s = np.asarray(f.subc[0], dtype=np.int64) + (np.asarray(f.subc[1], dtype=np.int64) - 1) * P
    s[0] = 0
    return s, P * (int(p.mm) + 1)


def scan_cells(f, kind):
    """{class: packed cell} where the scan tests place values, whatever the masks there (the restatement says what counts):
    cells 1 and ndeg; the last lane of a workgroup of the scan and the first lane of the next, both wet with open faces;
    the first cell of the last, partly filled workgroup that holds a cell at all; and per mask (n, u, v) its first and last
    cell (a value there always counts)."""
    p = f.p
    nd = int(p.ndeg)
    s, last = slots(f, kind)
    wet, mu, mv = scan_masks(f)
    allm = (np.asarray(f.mk_n) > 0.5) & (np.asarray(f.mk_u) > 0.5) & (np.asarray(f.mk_v) > 0.5)
    of_slot = {int(x): c for c, x in enumerate(s)}
    cells = {"cell1": 1, "ndeg": nd}
    pairs = [(of_slot[x], of_slot[x + 1]) for x in range(BLOCK - 1, last, BLOCK)
             if x in of_slot and x + 1 in of_slot and allm[of_slot[x]] and allm[of_slot[x + 1]]]
    assert pairs, "no workgroup boundary between two open wet cells"
    cells["lane255"], cells["lane0"] = pairs[len(pairs) // 2]
    nblk = last // BLOCK + 1
    assert (last + 1) % BLOCK != 0, "the last workgroup is full"
    tail = [c for c in range(1, nd + 1) if s[c] >= (nblk - 1) * BLOCK]
    assert tail, "no cell in the last workgroup"
    cells["lastblock"] = tail[0]
    for nm, m in (("n", wet), ("u", mu), ("v", mv)):
        idx = np.nonzero(m)[0]
        idx = idx[idx > 0] if idx.max() > 0 else idx
        cells["first_" + nm], cells["last_" + nm] = int(idx[0]), int(idx[-1])
    return cells


def row_cells(f, rows):
    """{"row<j>": packed cell} for rows j of the frame: a cell of the row that is wet with open faces where the row has one,
    else its middle cell (a value there is ignored by the scans)."""
    j = np.asarray(f.subc[1], dtype=np.int64)
    allm = (np.asarray(f.mk_n) > 0.5) & (np.asarray(f.mk_u) > 0.5) & (np.asarray(f.mk_v) > 0.5)
    out = {}
    for r in rows:
        inrow = np.nonzero(j == r)[0]
        inrow = inrow[inrow > 0]
        ok = inrow[allm[inrow]]
        out["row%d" % r] = int(ok[len(ok) // 3]) if ok.size else int(inrow[inrow.size // 2])
    return out


def placed_value(base_mm, q, layer, rank):
    """A value beyond the rough range for extreme q (0..5 = min h, max h, min u, ...) of a layer: distinct per layer and rank
    (the place's number), exactly representable steps of 1/64."""
    sign = -1.0 if q % 2 == 0 else 1.0
    step = (1 + layer) + (1 + rank) / 64.0
    if q == 0:
        return float(base_mm[layer, 0]) * (0.75 - step / 64.0)        # thinner than every cell, far above hmin / 2
    if q == 1:
        return float(base_mm[layer, 1]) + step
    return sign * (1.0 + step)


def place_extremes(f, state, cell, rank, lay_min, lay_max):
    """A doctored copy of state (hlay, u, v): the three minima placed in layer lay_min and the three maxima in layer lay_max of
    one cell.  Returns (state, expected minmax): the placed value where the cell counts for that field, the rough state's own
    extreme elsewhere."""
    base, thin = scans(f, state["hlay"], state["u"], state["v"])
    assert thin == 0
    masks = scan_masks(f)
    out = {k: np.array(state[k], dtype=F8, copy=True) for k in ("hlay", "u", "v")}
    want = base.copy()
    for q in range(6):
        k = lay_min if q % 2 == 0 else lay_max
        val = placed_value(base, q, k, rank)
        out[("hlay", "u", "v")[q // 2]][k, cell] = val
        if masks[q // 2][cell]:
            want[k, q] = val
    return out, want


def ignored_cells(f):
    """{"u": a wet cell whose W face is closed, "v": one whose S face is closed, "h": a dry cell (inside the land where the
    frame has any: a cell whose eight neighbours are dry too, else a margin cell)}."""
    wet = np.asarray(f.mk_n) > 0.5
    mu, mv = np.asarray(f.mk_u) > 0.5, np.asarray(f.mk_v) > 0.5
    nb = np.asarray(f.neig).astype(np.int64)
    cu = np.nonzero(wet & ~mu)[0]
    cv = np.nonzero(wet & ~mv)[0]
    dry = ~wet & (np.arange(wet.size) > 0)
    deep = dry & np.all(dry[nb] & (nb > 0), axis=1)
    ch = np.nonzero(deep)[0] if deep.any() else np.nonzero(dry)[0]
    return {"u": int(cu[cu.size // 2]), "v": int(cv[cv.size // 2]), "h": int(ch[ch.size // 2])}


def place_ignored(f, state):
    """Values far beyond the range at a closed u face, a closed v face and in a dry cell, every layer: the scans stay the
    rough state's own."""
    base, _ = scans(f, state["hlay"], state["u"], state["v"])
    c = ignored_cells(f)
    out = {k: np.array(state[k], dtype=F8, copy=True) for k in ("hlay", "u", "v")}
    for k in range(int(f.p.nlay)):
        sgn = -1.0 if k % 2 else 1.0
        out["u"][k, c["u"]] = sgn * (50.0 + k)
        out["v"][k, c["v"]] = -sgn * (60.0 + k)
        out["hlay"][k, c["h"]] = 1.0e5 + k if k % 2 else 1.0e-3 * float(f.p.hmin)       # (thin too: a dry cell is no thin layer)
    return out, base


def place_thin(f, state, where):
    """where: [(layer (0-based), packed cell)]; the thickness there becomes hmin / 4."""
    out = {k: np.array(state[k], dtype=F8, copy=True) for k in ("hlay", "u", "v")}
    for k, c in where:
        out["hlay"][k, c] = 0.25 * float(f.p.hmin)
    return out


def thin_cases(f, kind):
    """{name: ([(layer, cell)], expected flag)} of a single handle.  Cell ndeg is a margin cell in every frame this project
    builds (row mm + 1 is dry), so "cell ndeg of the last layer" is the last WET cell of the last layer, and cell ndeg itself
    is one of the dry cells that must report 0."""
    nl, nd = int(f.p.nlay), int(f.p.ndeg)
    s, last = slots(f, kind)
    wet = np.asarray(f.mk_n) > 0.5
    w = np.nonzero(wet)[0]
    blk = s[w] // BLOCK
    early, late = int(w[0]), int(w[-1])
    assert blk[0] != blk[-1]
    dry = ignored_cells(f)["h"]
    assert not wet[nd] and not wet[dry]
    out = {"layer2_only": ([(1, int(w[w.size // 2]))], 2),
           "last_wet_cell_last_layer": ([(nl - 1, late)], nl),
           "dry_cells_only": ([(0, dry), (nl - 1, nd)], 0)}
    if nl >= 3:
        out["layers_3_and_2_in_different_blocks"] = ([(2, early), (1, late)], 2)
        out["layers_2_and_3_in_different_blocks"] = ([(1, early), (2, late)], 2)
    return out


# (configuration, frame) of every rough state the GPU tests use; the thresholds of test_outputs_cpu hold for each
ROUGH_CASES = [("closed_leith_3l", "63x7"), ("closed_leith_3l", "130x18"), ("closed_leith_3l", "192x30"), ("closed_leith_3l", "4200x9"),
               ("jet_xyper_2l", "130x18"), ("jet_xyper_2l", "192x30"), ("soliton_xper_1l", "130x18"), ("closed_12l_hdot", "192x30"),
               ("sill_ocrp_sponge_3l", "130x18"), ("island_ragged_3l", "130x18"), ("island_ragged_3l", "192x30"),
               ("sponge_obc_mcbc0_2l", "130x18"), ("closed_svis_3l", "130x18"), ("closed_dt3d_forced_3l", "130x18"),
               ("stommel_wind_drag", "130x18"), ("closed_12l_hdot", "130x18"),
               ("closed_leith_3l", "130x99"), ("island_ragged_3l", "130x99"), ("jet_xyper_2l", "130x99")]
CONSTANT_V_CC = ("soliton_xper_1l", "stommel_wind_drag")         # dvis = 0: their v_cc record is bvis everywhere
# handle kind, configuration, frame of the scan tests with placed values
SCAN_HANDLES = [("dense", "closed_leith_3l", "192x30"), ("embedded", "island_ragged_3l", "192x30"), ("table", "island_ragged_3l", "130x18")]
BAND_CONFIGS = ("closed_leith_3l", "island_ragged_3l", "jet_xyper_2l")
BAND_FRAME = "130x99"
# arguments of rough_fields per (configuration, frame): the stress folds only if the array without forcing stays +0
ROUGH_KW = {("stommel_wind_drag", "130x18"): {"zero": ("tu3d",)}}
_STATES = {}


def rough_state(config, frame):
    """rough_inputs.rough_fields(base_fields(config, frame), 1, **ROUGH_KW), built once per session: the one state of that
    name, for the CPU conditions and the GPU tests alike; callers never write its arrays."""
    key = (config, frame)
    if key not in _STATES:
        _STATES[key] = RI.rough_fields(RI.base_fields(config, frame), 1, **ROUGH_KW.get(key, {}))
    return _STATES[key]


def layer_pairs(nlay):
    """(layer of the minima, layer of the maxima): every layer gets both in turn, two layers at least."""
    return [(k, (k + 1) % nlay) for k in range(nlay)] if nlay > 1 else [(0, 0)]


def check_row_placements(f, state, rows, scan=None):
    """Places the six extremes in a cell of every row of `rows`, two layer pairs each, and compares scan(doctored state) —
    the restatement itself when scan is None — with the expected minmax.  Returns how many placed values counted."""
    masks = scan_masks(f)
    counted = 0
    for rank, (nm, cell) in enumerate(row_cells(f, rows).items()):
        for lay_min, lay_max in layer_pairs(int(f.p.nlay))[:2]:
            doc, want = place_extremes(f, state, cell, rank, lay_min, lay_max)
            got = scans(f, doc["hlay"], doc["u"], doc["v"])[0] if scan is None else scan(doc)
            assert np.array_equal(got, want), (nm, lay_min, lay_max, got, want)
            counted += sum(bool(masks[q // 2][cell]) for q in range(6))
    return counted


def guessed_bands(f, nband):
    """[(first owned row, last owned row)] of nband bands dealt by rows (a ring owns rows 1..mm, the orphan row mm + 1 is
    nobody's): for the CPU test, which has no handle to ask; the GPU test takes the rows the handle dealt."""
    mm = int(f.p.mm)
    top = mm if float(f.p.yper) > 0.5 else mm + 1
    cut = [1 + (top * k) // nband for k in range(nband + 1)]
    return [(cut[k], cut[k + 1] - 1) for k in range(nband)]


def band_thin_cases(f, bands):
    """{name: ([(layer, cell)], expected flag)} on a frame cut into `bands` [(own0, own1)], nlay >= 2.  For every band and each
    of its edge rows (its first and last owned row: the rows on both sides of every seam, rows 1 and mm of a ring, the dry
    margin row of a closed frame) a thin cell in that row, paired with a thin cell of another layer in the middle row of the
    NEXT band — once with the upper layer in the edge row (that band's flag must win the merge), once with the lower one
    (the other band's must).  Then every band's middle row against the next band's, the middle band included, and on a ring
    the orphan row alone.  The expected flag comes from the masks: the lowest-numbered layer among the cells that are wet."""
    nl, mm = int(f.p.nlay), int(f.p.mm)
    wet = np.asarray(f.mk_n) > 0.5
    la, lb = nl - 1, nl - 2
    nb = len(bands)
    mid = [(a + b) // 2 for a, b in bands]
    rows = sorted({r for ab in bands for r in ab} | set(mid) | {mm + 1})
    cell = row_cells(f, rows)
    def case(where):
        hit = [k + 1 for k, c in where if wet[c]]
        return where, (min(hit) if hit else 0)
    out = {}
    for k, (own0, own1) in enumerate(bands):
        other = cell["row%d" % mid[(k + 1) % nb]]
        for r in (own0, own1):
            c = cell["row%d" % r]
            out["band %d row %d upper layer, band %d lower" % (k, r, (k + 1) % nb)] = case([(lb, c), (la, other)])
            out["band %d row %d lower layer, band %d upper" % (k, r, (k + 1) % nb)] = case([(la, c), (lb, other)])
        out["band %d middle row upper layer, band %d lower" % (k, (k + 1) % nb)] = case([(lb, cell["row%d" % mid[k]]), (la, other)])
        out["band %d middle row alone" % k] = case([(la, cell["row%d" % mid[k]])])
    if float(f.p.yper) > 0.5:
        out["orphan row alone"] = case([(0, cell["row%d" % (mm + 1)])])
    return out
