"""The flux-limited tracer scheme (scheme 2) on rough states with dry cells, without a GPU.

1. The numpy restatement (tracers_limited_ref) against a second, independently written form (tracers_limited_scalar: plain
   loops over Python floats, one cell at a time, following neig) on dry-cell states: every limited face with dry cells and
   transports of either sign, bit for bit.
2. Conditions on what test_gpu_tracers_limited_rough feeds the device, computed from the inputs alone with the kernel's
   interior-tile condition restated here (interior_tiles): the frame has interior tiles in both geometries, dry cell-layers
   lie inside them, every outcome of the limiter has a share, and in every layer each of the four reads of the staged form's
   outer ring (column c+2 from the east column, c-2 from lane 0, row r+2 from the top row, r-2 from the bottom row) happens
   both with a non-zero limiter and with the cell read being the only dry one of its stencil.  Conditions, not
   measurements: if a change of seed breaks one, the seed changes, not the condition.
3. The flux form closes on dry-cell states: |sum(mk_n r3)| / sum(|mk_n r3|) of scheme 2 within four times what the scheme-1
   restatement (pinned to the oracle by test_tracers_cpu) shows on the same inputs — the margin this project has used before.
   Measured here (321 x 50, 8 tracers, steps 7-9): scheme 1 1.6e-18 .. 3.0e-18, scheme 2 1.8e-18 .. 2.6e-18."""
import math

import numpy as np
import pytest

import rough_inputs as RI
import tracers_limited_ref as TL
import tracers_limited_scalar as TS
import tracers_ref as T
from helpers import same_bits

SEED_STATE, SEED_TRACERS = 3, 5
TX = 64


# ---- the interior-tile condition of k_tracers_lim, restated ----------------------------------------------------------------
def regular_tiles(f, win=None):
    """reg4 of an embedded handle restated: {(tx, t4)} of the 64 x 4 tiles whose every cell, and every cell within 3 of it, is
    a packed cell with all five masks 1.  win = (win0, win1): a band's window of global rows (local row j = global j - win0 + 1;
    what lies outside the window is no cell)."""
    L, Mg = f.p.lm + 1, f.p.mm + 1
    win0, win1 = win if win is not None else (1, Mg)
    M = win1 - win0 + 1
    good = np.zeros((L + 2, M + 2), bool)
    i, j = f.subc[0, 1:].astype(np.int64), f.subc[1, 1:].astype(np.int64) - (win0 - 1)
    ok = np.ones(f.p.ndeg, bool)
    for k in ("mk_n", "mk_u", "mk_v", "mkpe", "mkpi"):
        ok &= np.asarray(getattr(f, k))[1:] == 1.0
    ok &= (j >= 1) & (j <= M)
    good[i[ok], j[ok]] = True
    out = set()
    for t4 in range((M + 3) // 4):
        for tx in range((L + 63) // 64):
            x0, y0 = tx * 64 + 1, t4 * 4 + 1
            if x0 - 3 < 0 or y0 - 3 < 0 or x0 + 66 > L + 1 or y0 + 6 > M + 1:
                continue
            if good[x0 - 3:x0 + 67, y0 - 3:y0 + 7].all():
                out.add((tx, t4))
    return out


def interior_tiles(L, M, rows, joff=0, Mg=None, regular=None):
    """[(x0, y0)] of the 64 x rows tiles of an L x M frame (a band's window: local rows, joff, Mg of the whole frame) that
    take the staged body: the tile and its ring of two lie in 2..L-2 x 2..M-2, in global rows too, and on an embedded
    handle (regular = regular_tiles(...)) every 64 x 4 tile under it is regular."""
    Mg = M if Mg is None else Mg
    out = []
    for ty in range((M + rows - 1) // rows):
        for ch in range((L + TX - 1) // TX):
            x0, y0 = ch * TX + 1, ty * rows + 1
            inside = (x0 - 2 >= 2 and x0 + TX + 1 <= L - 2 and y0 - 2 >= 2 and y0 + rows + 1 <= M - 2
                      and y0 - 2 + joff >= 2 and y0 + rows + 1 + joff <= Mg - 2)
            if inside and regular is not None:
                t4 = (y0 - 1) >> 2
                inside = all((ch, t4 + k) in regular and (t4 + k) * 4 < M for k in range(rows >> 2))
            if inside:
                out.append((x0, y0))
    return out


def _case(config, frame, ntrc):
    g = RI.dry_cell_state(RI.base_fields(config, frame), SEED_STATE)
    q, rq, ctrg = RI.rough_tracers(g, g.hlay, ntrc, SEED_TRACERS)
    return g, q, rq, ctrg


# ---- 1. the scalar reference against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["closed_leith_3l", "island_ragged_3l", "jet_xyper_2l", "closed_12l_hdot", "sill_ocrp_sponge_3l"])
def test_restatement_equals_the_scalar_reference(config):
    g, q, rq, ctrg = _case(config, "130x18", 3)
    assert g.dry.any() and (np.asarray(g.hlay)[g.dry] == 0.0).all()
    if config == "closed_12l_hdot":
        assert np.any(g.hdot > 0.0) and np.any(g.hdot < 0.0)
    if config == "sill_ocrp_sponge_3l":
        assert np.any(g.nudg[0] != 0.0)
    for tstp in (7, 8):
        gene, ramp, ctim = T.step_scalars(g.p, tstp)
        assert gene != 0.0
        a = TL.update(g, g.hlay, g.h_u, g.h_v, q, rq, ctrg, gene, ramp, ctim, scheme=2)
        b = TS.update(g, g.hlay, g.h_u, g.h_v, q, rq, ctrg, gene)
        for k, (x, y) in enumerate(zip(a, b)):
            if not same_bits(x, y):
                bad = np.argwhere(~((x == y) & (np.signbit(x) == np.signbit(y))))[0]
                raise AssertionError((config, tstp, "q rq".split()[k], "first difference at (tracer, layer, cell[, level])",
                                      tuple(int(v) for v in bad), float(x[tuple(bad)]), float(y[tuple(bad)])))
        q, rq = a
    assert np.isfinite(q).all() and np.isfinite(rq).all()


# ---- 2. conditions on the inputs of the GPU test ----------------------------------------------------------------------------
GPU_FRAME = "321x50"
RING_READS = ("east column, h_u(E) <= 0: c+2", "west column, h_u > 0: c-2", "top row, h_v(N) <= 0: r+2", "bottom row, h_v > 0: r-2")


def _ring_reads(g, q1, tiles, rows):
    """Per layer and per read of RING_READS: (faces with a fully wet stencil and a non-zero limiter, faces with U and D wet
    and UU the only dry one), over the cells of the interior tiles `tiles`."""
    p = g.p
    E, N, W, S = (g.neig[:, k].astype(np.int64) for k in (0, 2, 4, 6))
    i, j = g.subc[0].astype(np.int64), g.subc[1].astype(np.int64)
    here = np.arange(p.ndeg + 1)
    col = {"e": np.zeros(p.ndeg + 1, bool), "w": np.zeros(p.ndeg + 1, bool), "t": np.zeros(p.ndeg + 1, bool), "b": np.zeros(p.ndeg + 1, bool)}
    for x0, y0 in tiles:
        inside = (i >= x0) & (i < x0 + TX) & (j >= y0) & (j < y0 + rows) & (here > 0)
        col["e"] |= inside & (i == x0 + TX - 1); col["w"] |= inside & (i == x0)
        col["t"] |= inside & (j == y0 + rows - 1); col["b"] |= inside & (j == y0)
    out = []
    for l in range(p.nlay):
        c, wet = T.concentration(g.hlay[l], q1[l])
        per = []
        # (cells whose face is meant, the face's own cell, its transport, back and forward links, sign wanted)
        for cells, at, flux, back, fwd, positive in ((col["e"], E, g.h_u[l], W, E, False), (col["w"], here, g.h_u[l], W, E, True),
                                                     (col["t"], N, g.h_v[l], S, N, False), (col["b"], here, g.h_v[l], S, N, True)):
            x = at[cells]                                    # the cell that stores the face's transport
            F = flux[x]
            pick = (F > 0.0) if positive else ~(F > 0.0)
            x, F = x[pick], F[pick]
            U = back[x] if positive else x
            D = x if positive else back[x]
            UU = back[back[x]] if positive else fwd[x]
            du, dd = c[U] - c[UU], c[D] - c[U]
            lim = np.where(du * dd > 0.0, np.minimum(np.minimum(2.0 * np.abs(du), 2.0 * np.abs(dd)), np.abs((du + 2.0 * dd) * TL.T3)), 0.0)
            per.append((int(np.sum(wet[U] & wet[D] & wet[UU] & (lim != 0.0))), int(np.sum(wet[U] & wet[D] & ~wet[UU]))))
        out.append(per)
    return out


@pytest.mark.parametrize("rows", [4, 8])
@pytest.mark.parametrize("config", ["closed_leith_3l", "jet_xyper_2l", "closed_12l_hdot", "sill_ocrp_sponge_3l", "tide_sponge_2l"])
def test_gpu_inputs_reach_the_staged_body(config, rows):
    g, q, rq, ctrg = _case(config, GPU_FRAME, 8)
    p = g.p
    L, M = p.lm + 1, p.mm + 1
    assert (L, M) == (322, 51)
    tiles = interior_tiles(L, M, rows)
    assert len(tiles) == {4: 30, 8: 12}[rows]
    i, j = g.subc[0].astype(np.int64), g.subc[1].astype(np.int64)
    inside = np.zeros(p.ndeg + 1, bool)
    for x0, y0 in tiles:
        inside |= (i >= x0) & (i < x0 + TX) & (j >= y0) & (j < y0 + rows)
    inside[0] = False
    ndry = int(np.sum(g.dry & inside[None]))
    n = TL.outcomes(g, g.hlay, g.h_u, g.h_v, q[1])
    faces = sum(n.values())
    share = {k: n[k] / faces for k in TL.OUTCOMES}
    reads = _ring_reads(g, q[1], tiles, rows)
    print("%s 64x%d: %d interior tiles, %d dry cell-layers inside, shares %s, weakest ring read: limited %d, UU alone dry %d"
          % (config, rows, len(tiles), ndry, " ".join("%s %.3f" % (k, share[k]) for k in TL.OUTCOMES),
             min(a for per in reads for a, _ in per), min(b for per in reads for _, b in per)))
    assert ndry >= 1, (config, rows)
    for k in TL.OUTCOMES:
        assert share[k] >= 0.03, (config, k, share)
    for l, per in enumerate(reads):
        for name, (limited, uu_dry) in zip(RING_READS, per):
            assert limited >= 1, (config, rows, "layer", l + 1, name, "never with a fully wet stencil and a non-zero limiter")
            assert uu_dry >= 1, (config, rows, "layer", l + 1, name, "never with UU the only dry cell")


def nudged_inside(g, rows):
    """(cells of interior tiles with a relaxation rate on the thickness, cells of interior tiles)."""
    i, j = g.subc[0].astype(np.int64), g.subc[1].astype(np.int64)
    inside = np.zeros(g.p.ndeg + 1, bool)
    for x0, y0 in interior_tiles(g.p.lm + 1, g.p.mm + 1, rows):
        inside |= (i >= x0) & (i < x0 + TX) & (j >= y0) & (j < y0 + rows)
    inside[0] = False
    return int(np.sum(inside & (g.nudg[0] != 0.0))), int(inside.sum())


@pytest.mark.parametrize("frame,rows", [("321x50", 4), ("321x51", 4), ("321x51", 8)])
def test_sill_sponge_reaches_interior_tiles(frame, rows):
    """The one-tracer plan B cases of the GPU test are there for nudging inside the staged body: some cell of an interior
    tile has a relaxation rate, and some has none (the ng == 0 shortcut beside the nudged expression).  The sill's sponges are
    rows 1-5 and the last six: on 321 x 50 the 64 x 4 tiles reach row 5, the 64 x 8 tiles reach neither (their first interior
    tile row starts at 9, their last ends at row 40 of 51), so 321 x 51 is there, where a 64 x 8 tile row ends at row 48."""
    g = RI.rough_fields(RI.base_fields("sill_ocrp_sponge_3l", frame), 1)
    nudged, cells = nudged_inside(g, rows)
    print("sill_ocrp_sponge_3l %s 64x%d: %d nudged cells inside interior tiles, %d without a rate" % (frame, rows, nudged, cells - nudged))
    assert 1 <= nudged < cells


# ---- 3. the flux form closes on dry-cell states -----------------------------------------------------------------------------
def _closure(g, r3):
    """max over tracers and layers of |fsum(mk_n r3)| / fsum(|mk_n r3|)."""
    worst = 0.0
    for t in range(r3.shape[0]):
        for l in range(r3.shape[1]):
            x = (np.asarray(g.mk_n) * r3[t, l]).tolist()
            worst = max(worst, abs(math.fsum(x)) / math.fsum(abs(v) for v in x))
    return worst


@pytest.mark.parametrize("config", ["closed_leith_3l", "jet_xyper_2l", "island_ragged_3l"])
def test_flux_form_closes_on_dry_cell_states(config):
    g, q0, rq0, ctrg = _case(config, GPU_FRAME, 8)
    assert not np.any(g.nudg != 0.0) and not (g.has.get("hdot", False) and np.any(g.hdot != 0.0))
    worst = {}
    for scheme in (1, 2):
        q, rq = q0, rq0
        worst[scheme] = 0.0
        for tstp in (7, 8, 9):
            gene, ramp, ctim = T.step_scalars(g.p, tstp)
            q, rq = TL.update(g, g.hlay, g.h_u, g.h_v, q, rq, ctrg, gene, ramp, ctim, scheme=scheme)
            worst[scheme] = max(worst[scheme], _closure(g, rq[..., 1]))
        assert np.isfinite(q).all()
    print("%s: flux-form closure, scheme 1 %.3g, scheme 2 %.3g" % (config, worst[1], worst[2]))
    assert worst[1] > 0.0
    assert worst[2] <= 4.0 * worst[1], (config, worst)
