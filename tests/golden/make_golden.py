#!/usr/bin/env python3
"""Generates tests/golden/*.npz from the REAL reference (this container only).

For every case: build the reference with oracle/ref_build.py (flang -O2
-ffp-contract=off, patches P0-P4 described there), run it on the case's inputs in a
scratch directory, and keep
  * the parameter block (JSON) and the real*4 input arrays,
  * the static module state after read_input_data (connectivity, masks, forcings),
  * the FP64 module state after time steps 1,2,3,4,5,10 (+ per-step scalars),
  * the reference's own real*4 output records (eta_, u___, v___, grid.bin, h_0.bin).
Fixtures are data only (inputs and expected outputs); no reference text is stored.

Usage:  python tests/golden/make_golden.py [case ...]
"""
from __future__ import annotations

import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from beom_amd import inputs as I          # noqa: E402
from beom_amd.params import make_params   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = (1, 2, 3, 4, 5, 10)


def basin_with_island(lm=22, mm=17):
    """Closed basin with an island, a bay and a one-cell channel: exercises every land
    mask combination of index_grid_points (private_mod.f95:692-730)."""
    h = np.zeros((lm + 2, mm + 2))
    h[1:-1, 1:-1] = 500.0
    x = np.arange(lm + 2)[:, None]; y = np.arange(mm + 2)[None, :]
    h[1:-1, 1:-1] -= 150.0 * np.exp(-((x - 6.0) ** 2 + (y - 5.0) ** 2) / 20.0)[1:-1, 1:-1]
    h[9:13, 7:10] = 0.0           # island
    h[1:5, mm - 3:mm + 1] = 0.0   # land in NW corner -> bay
    h[16, 1:8] = 0.0              # peninsula
    h[16, 4] = 450.0              # one-cell channel through it
    h[lm - 2:lm + 1, mm] = 0.0
    return h


def case_island(nlay=3):
    lm, mm = 22, 17
    h_bo = basin_with_island(lm, mm)
    ndeg = I.get_nbr_deg_freedom(h_bo)
    x = (np.arange(lm + 2) - 0.5 * (lm + 1))[:, None]; y = (np.arange(mm + 2) - 0.5 * (mm + 1))[None, :]
    mound = 0.8 * np.exp(-(x ** 2 + y ** 2) / 16.0)
    topl = [0.0, 0.25, 0.5][:nlay]
    n = np.zeros((lm + 2, mm + 2, nlay)); u = np.zeros_like(n); v = np.zeros_like(n)
    for k in range(nlay):
        n[:, :, k] = mound * (1.0 - topl[k]) * (1.0 if k == 0 else -3.0)
    u[:, :, 0] = 0.05 * np.sin(0.4 * y) * np.ones_like(x)
    v[:, :, nlay - 1] = -0.03 * np.cos(0.3 * x) * np.ones_like(y)
    init = np.stack([n, u, v], axis=3)
    taus = np.zeros((lm + 2, mm + 2, 2))
    taus[:, :, 0] = 0.1 * np.cos(np.pi * y / mm) * np.ones_like(x)
    taus[:, :, 1] = 0.02 * np.sin(np.pi * x / lm) * np.ones_like(y)
    hdot = np.zeros((lm + 2, mm + 2, nlay))
    hdot[:, :, 0] = 1.0e-6 * np.exp(-((x - 3) ** 2 + (y + 2) ** 2) / 9.0)
    hdot[:, :, nlay - 1] = -hdot[:, :, 0]
    bodf = np.zeros((nlay, 2)); bodf[0, 0] = 1.0e-7; bodf[nlay - 1, 1] = -2.0e-7
    fcor = 1.0e-4 + 2.0e-11 * 5.0e3 * y * np.ones_like(x)
    dl = 5.0e3
    cext = np.sqrt(9.8 * h_bo.max())
    dt = 0.5 * dl / cext
    p = make_params(lm, mm, nlay, ndeg, dl, cext, 1.0e-4, [1026.0, 1027.0, 1028.0][:nlay], topl,
                    12 * dt / 86400.0, 4 * dt / 86400.0, 6.4 * dt / 86400.0, 2.2 * dt / 86400.0, 5.0, 0.3, 2.5e-3,
                    1.0, 10.0, 10.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0,
                    desc="golden: island, wind, quadratic drag, hdot, bodf, ramp, dt3d")
    return p, {"h_bo": h_bo, "init": init, "taus": taus, "hdot": hdot, "bodf": bodf, "fcor": fcor}


def case_island_deep(nlay=10):
    """Closed island basin with a column of more layers than the fused sweeps take (nlay > 8: per-layer Montgomery and
    viscosity launches next to the fused u+v sweep); topl spread over the whole column, wind, drag and Leith viscosity."""
    lm, mm = 14, 11
    h_bo = np.zeros((lm + 2, mm + 2))
    h_bo[1:-1, 1:-1] = 500.0
    x = np.arange(lm + 2)[:, None]; y = np.arange(mm + 2)[None, :]
    h_bo[1:-1, 1:-1] -= 120.0 * np.exp(-((x - 4.0) ** 2 + (y - 3.0) ** 2) / 12.0)[1:-1, 1:-1]
    h_bo[6:9, 5:8] = 0.0          # island
    h_bo[1:4, mm - 2:mm + 1] = 0.0    # land in the NW corner -> bay
    h_bo[11, 1:5] = 0.0           # peninsula
    ndeg = I.get_nbr_deg_freedom(h_bo)
    xc = (x - 0.5 * (lm + 1)) * np.ones((1, mm + 2)); yc = (y - 0.5 * (mm + 1)) * np.ones((lm + 2, 1))
    mound = 0.8 * np.exp(-(xc ** 2 + yc ** 2) / 10.0)
    topl = list(np.linspace(0.0, 0.7, nlay))
    n = np.zeros((lm + 2, mm + 2, nlay)); u = np.zeros_like(n); v = np.zeros_like(n)
    for k in range(nlay):
        n[:, :, k] = mound * (1.0 - topl[k]) * (1.0 if k == 0 else -2.0)
    u[:, :, 0] = 0.05 * np.sin(0.5 * yc)
    v[:, :, nlay - 1] = -0.03 * np.cos(0.4 * xc)
    u[:, :, nlay // 2] = 0.02 * np.cos(0.3 * yc)
    init = np.stack([n, u, v], axis=3)
    init[h_bo == 0.0] = 0.0
    taus = np.zeros((lm + 2, mm + 2, 2))
    taus[:, :, 0] = 0.1 * np.cos(np.pi * yc / mm)
    taus[:, :, 1] = 0.02 * np.sin(np.pi * xc / lm)
    fcor = 1.0e-4 + 2.0e-11 * 5.0e3 * yc
    dl = 5.0e3
    cext = np.sqrt(9.8 * h_bo.max())
    dt = 0.5 * dl / cext
    p = make_params(lm, mm, nlay, ndeg, dl, cext, 1.0e-4, list(np.linspace(1026.0, 1028.0, nlay)), topl,
                    12 * dt / 86400.0, 4 * dt / 86400.0, 6.4 * dt / 86400.0, 0.0, 5.0, 0.3, 2.5e-3,
                    1.0, 10.0, 10.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0,
                    desc="golden: island, %d layers, wind, quadratic drag, Leith" % nlay)
    return p, {"h_bo": h_bo, "init": init, "taus": taus, "fcor": fcor}


def case_sill_deep(nlay=16):
    """Outcropping sill with nudged northern and southern sponges and a column of 16 layers (BEOM_MAX_LAYERS): the
    interfaces spread over the upper 60 % of the deepest water column, so the deep ones outcrop on the sill."""
    from beom_amd.params import format_like_print_params
    p, f = I.case_sill_exchange3d(lm=5, mm=17, nlay=nlay, dt_s=0.01, npts=3, sill_halfwidth=3.0)
    topl = format_like_print_params("topl", np.linspace(0.0, 0.6, nlay))[2:-2].split(",")
    return p.replace(topl=topl), f


def case_tide(lm=20, mm=9):
    """Nudged western boundary with a tidal constituent in eta and u (cos path,
    private_mod.f95:1453-1454,1538-1539,1632-1634)."""
    nlay = 2
    h_bo = np.zeros((lm + 2, mm + 2)); h_bo[1:-1, 1:-1] = 80.0
    ndeg = I.get_nbr_deg_freedom(h_bo)
    nudg = np.zeros((lm + 2, mm + 2, 3))
    for i in range(0, 7):     # i = 0 too: index_boundary_points (:1106-1132) wants the dry margin nudged
        nudg[i, :, 0:2] = 0.4 * (7 - i) / 7.0
    tide = np.zeros((2, 1, lm + 2, mm + 2, 3))
    tide[0, 0, :, :, 0] = 0.3; tide[1, 0, :, :, 0] = 0.5
    tide[0, 0, :, :, 1] = 0.05; tide[1, 0, :, :, 1] = 1.1
    tide[0, 0, 0, 0, 0] = 12.14             # omega (rad/day) lives at (1,k,0,0,1)
    init = np.zeros((lm + 2, mm + 2, nlay, 3))
    cext = np.sqrt(9.8 * 80.0); dl = 2.0e3; dt = 0.5 * dl / cext
    p = make_params(lm, mm, nlay, ndeg, dl, cext, 0.5e-4, [1025.0, 1027.0], [0.0, 0.4],
                    12 * dt / 86400.0, 1.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.5, 10.0, 10.0, 1.0, 1.0,
                    0.0, 0.0, 0.0, 0.0, 0.0, 0.0, desc="golden: tide + sponge")
    return p, {"h_bo": h_bo, "nudg": nudg, "tide": tide, "init": init}


def case_3d_variant(lm=24, mm=11):
    """private_mod3d.f95 epilogue (:1635-1683): 3 layers, eta nudging on both halves."""
    nlay = 3
    h_bo = np.zeros((lm + 2, mm + 2)); h_bo[1:-1, 1:-1] = 900.0
    ndeg = I.get_nbr_deg_freedom(h_bo)
    nudg = np.zeros((lm + 2, mm + 2, 3))
    for i in range(1, 6):
        nudg[i, :, 0] = 0.05 * (6 - i)
        nudg[lm + 1 - i, :, 0] = 0.04 * (6 - i)
    nudg[0:3, :, 1] = 0.02       # a nudged western segment must exist (:1226-1231)
    init = np.zeros((lm + 2, mm + 2, nlay, 3))
    x = (np.arange(lm + 2) - lm // 2)[:, None] * np.ones((1, mm + 2))
    init[:, :, 1, 0] = 20.0 * np.tanh(x / 4.0)
    init[:, :, 2, 0] = -150.0 * (x > 3)          # makes hlay(:,3) straddle 20*hsal on the east side
    cext = np.sqrt(9.8 * 900.0); dl = 1.0e3; dt = 0.5 * dl / cext
    p = make_params(lm, mm, nlay, ndeg, dl, cext, 1.0e-4, [1026.0, 1027.0, 1028.0], [0.0, 0.3, 0.8],
                    12 * dt / 86400.0, 1.0, 0.0, 0.0, 0.0, 0.2, 0.0, 1.0, 10.0, 10.0, 1.0, 1.0,
                    0.0, 0.0, 0.0, 0.0, 0.0, 0.0, desc="golden: private_mod3d update_h epilogue")
    return p, {"h_bo": h_bo, "nudg": nudg, "init": init}


def case_obc():
    """Nudged OPEN boundaries with the original BEOM treatment (mcbc = 0): no_gradient_obc
    (private_mod.f95:2613-2679) on a western (u-normal) and a northern (v-normal) boundary."""
    lm, mm, nlay = 30, 14, 2
    h_bo = np.zeros((lm + 2, mm + 2)); h_bo[1:-1, 1:-1] = 120.0
    ndeg = I.get_nbr_deg_freedom(h_bo)
    nudg = np.zeros((lm + 2, mm + 2, 3))
    for i in range(0, 7):                       # western sponge: eta and u (normal), margin included
        nudg[i, :, 0] = np.maximum(nudg[i, :, 0], 0.35 * (7 - i) / 7.0)
        nudg[i, :, 1] = np.maximum(nudg[i, :, 1], 0.35 * (7 - i) / 7.0)
    for j in range(mm + 1, mm - 5, -1):         # northern sponge: eta and v (normal)
        w = 0.3 * (j - (mm - 5)) / 7.0
        nudg[:, j, 0] = np.maximum(nudg[:, j, 0], w)
        nudg[:, j, 2] = np.maximum(nudg[:, j, 2], w)
    x = (np.arange(lm + 2) - 18.0)[:, None]; y = (np.arange(mm + 2) - 6.0)[None, :]
    init = np.zeros((lm + 2, mm + 2, nlay, 3))
    init[:, :, 0, 0] = 0.5 * np.exp(-(x ** 2 + y ** 2) / 9.0)
    init[:, :, 1, 0] = -2.0 * np.exp(-(x ** 2 + y ** 2) / 9.0)
    init[:, :, 0, 1] = 0.02
    cext = np.sqrt(9.8 * 120.0); dl = 3.0e3; dt = 0.5 * dl / cext
    p = make_params(lm, mm, nlay, ndeg, dl, cext, 0.8e-4, [1025.0, 1027.5], [0.0, 0.35],
                    12 * dt / 86400.0, 4 * dt / 86400.0, 0.0, 0.0, 0.0, 0.15, 0.0, 1.0, 10.0, 10.0, 1.0, 1.0,
                    0.0, 0.0, 0.0, 0.0, 0.0, 0.0, desc="golden: open boundaries, mcbc = 0", mcbc="0.")
    return p, {"h_bo": h_bo, "nudg": nudg, "init": init}


def case_obc_yper():
    """no_gradient_obc (mcbc = 0) on a channel periodic in y: a nudged western and a nudged eastern open boundary whose
    segments run through the periodic seam and the orphan row mm+1 (:642-668, :1060-1240, :2613-2679)."""
    lm, mm, nlay = 30, 27, 2
    h_bo = np.zeros((lm + 2, mm + 2)); h_bo[1:-1, :] = 120.0
    ndeg = I.get_nbr_deg_freedom(h_bo)
    nudg = np.zeros((lm + 2, mm + 2, 3))
    for i in range(0, 7):                       # western sponge: eta and u (normal), margin included
        nudg[i, :, 0] = 0.35 * (7 - i) / 7.0
        nudg[i, :, 1] = 0.35 * (7 - i) / 7.0
    for i in range(lm + 1, lm - 5, -1):         # eastern sponge
        w = 0.3 * (i - (lm - 5)) / 7.0
        nudg[i, :, 0] = np.maximum(nudg[i, :, 0], w)
        nudg[i, :, 1] = np.maximum(nudg[i, :, 1], w)
    x = (np.arange(lm + 2) - 14.0)[:, None]; y = (np.arange(mm + 2) - 9.0)[None, :]
    init = np.zeros((lm + 2, mm + 2, nlay, 3))
    init[:, :, 0, 0] = 0.5 * np.exp(-(x ** 2 + y ** 2) / 9.0)
    init[:, :, 1, 0] = -2.0 * np.exp(-(x ** 2 + y ** 2) / 9.0)
    init[:, :, 0, 1] = 0.02
    init[:, :, 1, 2] = 0.01 * np.sin(2 * np.pi * np.arange(mm + 2) / mm)[None, :]
    for a_ in (init,):                          # periodic margins in y
        a_[:, 0] = a_[:, mm]; a_[:, mm + 1] = a_[:, 1]
    cext = np.sqrt(9.8 * 120.0); dl = 3.0e3; dt = 0.5 * dl / cext
    p = make_params(lm, mm, nlay, ndeg, dl, cext, 0.8e-4, [1025.0, 1027.5], [0.0, 0.35],
                    12 * dt / 86400.0, 4 * dt / 86400.0, 0.0, 0.0, 0.0, 0.15, 0.0, 1.0, 10.0, 10.0, 1.0, 1.0,
                    0.0, 0.0, 0.0, 0.0, 1.0, 0.0, desc="golden: open boundaries mcbc = 0, periodic in y", mcbc="0.")
    return p, {"h_bo": h_bo, "nudg": nudg, "init": init}


def case_biharm():
    """Biharmonic viscosity svis > 0 (private_mod.f95:2508-2599, 1471-1473, 1555-1557) on the
    island basin: every land-mask combination meets the masked Laplacians."""
    p, f = case_island(2)
    return p.replace(svis="2.e10", dt3d="0."), f


def case_topdrag():
    """The fork's top drag (tdrg > 0, distribute_stress :2006, :2075-2112) under a surface
    topography file (topt = 1: h_2d = h_bo - h_to in real*4, :809-832), island basin."""
    p, f = case_island(2)
    lm, mm = p.lm, p.mm
    x = np.arange(lm + 2)[:, None]; y = np.arange(mm + 2)[None, :]
    # with topt = 1 the reference reads h_to into an unallocated buffer when it meets bodf.bin
    # (:809-814): no body force in this case
    f = {k: v for k, v in f.items() if k != "bodf"}
    f["h_to"] = (40.0 * np.exp(-((x - 15.0) ** 2 + (y - 11.0) ** 2) / 30.0)).astype(np.float32)
    return p.replace(tdrg="2.e-3", topt="1."), f


def case_topdrag_ocrp():
    """Top drag together with outcropping (ocrp = 1 branch of the stress fractions, :1991)."""
    p, f = I.case_sill_exchange3d(lm=15, mm=41, nlay=2, dt_s=0.01, npts=5, sill_halfwidth=6.0)
    return p.replace(tdrg="1.e-3"), f


def case_random_coast():
    """x-periodic channel with seeded random land: blobs, one-cell islands, one-cell straits and
    diagonal contacts — every neighbour/mask combination of index_grid_points (:588-764) that the
    hand-made island basin may have missed.  Wind, linear drag, 2 layers."""
    rng = np.random.RandomState(20261004)
    lm, mm, nlay = 26, 19, 2
    h = np.zeros((lm + 2, mm + 2))
    h[1:-1, 1:-1] = 300.0 + 100.0 * rng.rand(lm, mm)
    land = rng.rand(lm + 2, mm + 2) < 0.14
    for _ in range(3):                                  # a few larger blobs
        cx, cy, r = rng.randint(3, lm - 2), rng.randint(3, mm - 2), rng.randint(2, 4)
        x = np.arange(lm + 2)[:, None]; y = np.arange(mm + 2)[None, :]
        land |= ((x - cx) ** 2 + (y - cy) ** 2) <= r * r
    h[land] = 0.0
    h[:, 0] = 0.0; h[:, -1] = 0.0
    h[0, :] = h[lm, :]; h[lm + 1, :] = h[1, :]          # periodic margins, as the channel recipes do
    ndeg = I.get_nbr_deg_freedom(h)
    x = (np.arange(lm + 2) - 0.5 * (lm + 1))[:, None]; y = (np.arange(mm + 2) - 0.5 * (mm + 1))[None, :]
    n = np.zeros((lm + 2, mm + 2, nlay)); u = np.zeros_like(n); v = np.zeros_like(n)
    n[:, :, 0] = 0.5 * np.exp(-(x ** 2 + y ** 2) / 30.0)
    n[:, :, 1] = -1.5 * np.exp(-((x - 4) ** 2 + (y + 3) ** 2) / 20.0)
    u[:, :, 0] = 0.04 * np.cos(0.5 * y) * np.ones_like(x)
    v[:, :, 1] = 0.02 * np.sin(0.7 * x) * np.ones_like(y)
    init = np.stack([n, u, v], axis=3)
    taus = np.zeros((lm + 2, mm + 2, 2))
    taus[:, :, 0] = 0.08 * np.sin(np.pi * (y / mm)) * np.ones_like(x)
    dl = 4.0e3
    cext = np.sqrt(9.8 * h.max())
    dt = 0.5 * dl / cext
    p = make_params(lm, mm, nlay, ndeg, dl, cext, 8.0e-5, [1026.0, 1028.0], [0.0, 0.4],
                    12 * dt / 86400.0, 4 * dt / 86400.0, 0.0, 0.0, 5.0, 0.25, 3.0e-4,
                    1.0, 10.0, 10.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0,
                    desc="golden: random coastline, x-periodic")
    return p, {"h_bo": h, "init": init, "taus": taus}


def _short(pf, nsteps=12, nout=4, **lits):
    """Same recipe, a dozen time steps (fixtures hold steps 1..10)."""
    p, f = pf
    dt = float(p.dt)
    return p.replace(dt_s="%.9f" % ((nsteps + 0.2) * dt / 86400.0), dt_o="%.9f" % ((nout + 0.01) * dt / 86400.0), **lits), f


def _with_dt3d(pf, nsteps3d=3):
    """Viscosity and stresses refreshed every nsteps3d steps only (dt3d > 0, :1889-1896)."""
    p, f = pf
    return p.replace(dt3d="%.9f" % ((nsteps3d + 0.2) * float(p.dt) / 86400.0)), f


def _std_fb(pf):
    p, f = pf
    return p.replace(g_fb="0."), f


CASES = {
    # name: (builder, reference engine file)
    "stommel_24x16": (lambda: I.case_stommel(lm=24, mm=16, dl=100.0e3, dt_s=0.2), "private_mod.f95"),
    "soliton_31x15_xper": (lambda: I.case_soliton(lm=31, mm=15, dt_s=5.0), "private_mod.f95"),
    "jet_2l_xyper": (lambda: I.case_unstable_jet(lm=21, mm=27, nlay=2, dt_s=1.5, dt_o=0.45), "private_mod.f95"),
    "jet_1l_xyper_stdfb": (lambda: _std_fb(I.case_unstable_jet(lm=21, mm=27, nlay=1, dt_s=1.5)), "private_mod.f95"),
    "sill_2l_ocrp": (lambda: I.case_sill_exchange3d(lm=15, mm=41, nlay=2, dt_s=0.01, npts=5,
                                                    sill_halfwidth=6.0), "private_mod.f95"),
    "sill_4l_ocrp": (lambda: I.case_sill_exchange3d(lm=15, mm=41, nlay=4, dt_s=0.01, npts=5,
                                                    sill_halfwidth=6.0), "private_mod.f95"),
    "carrier_beach": (lambda: I.case_carrier_beach(lm=120, mm=3, dt_s=0.002), "private_mod.f95"),
    "island_3l_forced": (lambda: case_island(3), "private_mod.f95"),
    "tide_sponge": (case_tide, "private_mod.f95"),
    "variant3d_3l": (case_3d_variant, "private_mod3d.f95"),
    "obc_mcbc0_2l": (case_obc, "private_mod.f95"),
    "biharm_island_2l": (case_biharm, "private_mod.f95"),
    "obc_mcbc0_yper_2l": (case_obc_yper, "private_mod.f95"),
    "jet_2l_xyper_dt3d": (lambda: _with_dt3d(I.case_unstable_jet(lm=21, mm=27, nlay=2, dt_s=1.5, dt_o=0.45)), "private_mod.f95"),
    "stommel_24x16_dt3d": (lambda: _with_dt3d(I.case_stommel(lm=24, mm=16, dl=100.0e3, dt_s=0.2), 2), "private_mod.f95"),
    "random_coast_2l_xper": (case_random_coast, "private_mod.f95"),
    # reduced-size runs of further testcases/*.m recipes (beom_amd/inputs.py)
    "tc_upwelling_wind_yper": (lambda: _short(I.case_upwelling_seaward_wind(lm=40, mm=1), dt_r="0.002"), "private_mod.f95"),
    "tc_lock_exchange": (lambda: _short(I.case_lock_exchange(lx=16.0e3)), "private_mod.f95"),
    "tc_morel_upwelling_xper": (lambda: _short(I.case_morel_upwelling(ly_in_rext=0.2)), "private_mod.f95"),
    "tc_outcrop_seamount_5l": (lambda: _short(I.case_outcrop_seamount(lx=200.0e3)), "private_mod.f95"),
    "tc_wave_sponge": (lambda: _short(I.case_wave_sponge(lx=100.0e3, ly=80.0e3, npts=5)), "private_mod.f95"),
    "tc_tide_ridge_7l": (lambda: _short(I.case_tide_ridge(lm=60, npts=5, ridge_halfwidth=10.0), dt_r="0.002"), "private_mod.f95"),
    "tc_tide_ridge_3l_noocrp": (lambda: _short(I.case_tide_ridge(lm=60, ocrp=0, npts=5, ridge_halfwidth=10.0), dt_r="0.002"), "private_mod.f95"),
    "tc_baines_ridge_yper": (lambda: _short(I.case_baines_ridge(domain_in_lros=14.0, npts=5)), "private_mod.f95"),
    "tc_mixed_open_bc": (lambda: _short(I.case_mixed_open_bc(lm=30, mm=24, npts=5), dt_r="0.002"), "private_mod.f95"),
    "tc_conservation_xyper_stdfb": (lambda: _short(I.case_conservation(lx=200.0e3)), "private_mod.f95"),
    "tc_conservation_outcrop_3l_closed": (lambda: _short(I.case_conservation(lx=200.0e3, nlay=3, outc=1, xper=0, yper=0)), "private_mod.f95"),
    "tc_sill_exchange2d": (lambda: _short(I.case_sill_exchange2d(lx=6.0e3, npts=8, sill_halfwidth=10.0)), "private_mod.f95"),
    "tc_sill_exchange2d_tides": (lambda: _short(I.case_sill_exchange2d(lx=6.0e3, npts=5, tides=True, sill_halfwidth=10.0)), "private_mod.f95"),
    "tc_outcrop_seamount_3d_3l": (lambda: _short(I.case_outcrop_seamount(lx=100.0e3, nlay=3, three_d=True)), "private_mod.f95"),
    "topdrag_topo_2l": (case_topdrag, "private_mod.f95"),
    "topdrag_sill_ocrp_2l": (case_topdrag_ocrp, "private_mod.f95"),
    # the fork's rigid lid (rgld = 1: Poisson equation for the lid pressure by Gauss-Seidel sweeps, :1705-1838; needs
    # ocrp = 1, since the operators are set up inside get_equilibrium_thickness_h_0, :505-563; g_fb = 1 is overridden, :1880)
    "rigid_lid_sill_2l": (lambda: (lambda pf: (pf[0].replace(rgld="1."), pf[1]))(
        I.case_sill_exchange3d(lm=24, mm=31, nlay=2, dt_s=0.01, npts=5, sill_halfwidth=6.0)), "private_mod.f95"),
    # columns of more than 8 layers (up to BEOM_MAX_LAYERS = 16)
    "island_10l_deep": (case_island_deep, "private_mod.f95"),
    "sill_16l_ocrp": (case_sill_deep, "private_mod.f95"),
    "rigid_lid_closed_3l_wind": (lambda: (lambda pf: (pf[0].replace(rgld="1.", ocrp="1.", bdrg="2.e-4", tauw=["0.05", "0.02"], g_fb="0."), pf[1]))(
        _short(I.case_conservation(lx=200.0e3, nlay=3, outc=1, xper=0, yper=0))), "private_mod.f95"),
}


# Restarted runs (rsta = 1, private_mod.f95:238, 1299-1420, 1862-1866, 1887, 1898-1901): the case is first run from rest
# with outputs; then the reference is built again with rsta = 1 and run in the SAME directory — it continues from the last
# complete record (real*4 eta_, u___, v___; tres = the last entry of time.txt) with three plain forward-backward steps, no
# wind ramp, and ctim = tres + dtd8*tstp.  The fixture holds the first run's files (pre_file_*: what the restart found in
# odir), the FP64 state of the restarted run and the files after it.
RESTART_CASES = {
    "restart_island_3l_forced": (lambda: case_island(3), "private_mod.f95"),     # wind ramp (dt_r) switched off by rsta
    "restart_tide_sponge": (lambda: (lambda pf: (pf[0].replace(dt_o="%.9f" % (5.01 * float(pf[0].dt) / 86400.0)), pf[1]))(case_tide()),
                            "private_mod.f95"),                                   # tidal phase w_ti*ctim continues at tres
}
OUTPUT_FILES = ("grid.bin", "h_0.bin", "eta_.bin", "u___.bin", "v___.bin", "pvor.bin", "mont.bin", "v_cc.bin")


def _collect_files(work, prefix, out):
    for fn in OUTPUT_FILES:
        if os.path.exists(os.path.join(work, fn)):
            out[prefix + fn.replace(".", "_")] = np.fromfile(os.path.join(work, fn), dtype=np.uint8)
    for fn in ("time.txt", "param_basin.txt"):
        with open(os.path.join(work, fn)) as fh:
            out[prefix + fn.replace(".", "_")] = np.array(fh.read())


def generate(name):
    import ref_build
    import refdump
    restart = name in RESTART_CASES
    builder, engine = (RESTART_CASES if restart else CASES)[name]
    p, files = builder()
    work = os.path.join("/tmp", "beom_golden", name)
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    I.write_inputs(work, files)
    pre = {}
    if restart:
        exe0 = ref_build.build(p, os.path.join(ROOT, "oracle", "_ref", "golden_" + name + "_first"), engine)
        ref_build.run(exe0, work)
        _collect_files(work, "pre_file_", pre)
        p = p.replace(rsta="1.")
    exe = ref_build.build(p, os.path.join(ROOT, "oracle", "_ref", "golden_" + name), engine)
    ref_build.run(exe, work, dump_upto=max(STEPS))
    out = {"params_json": np.array(json.dumps(p.to_json())), "engine": np.array(engine)}
    out.update(pre)
    for k, a in files.items():
        out["in_" + k] = np.asarray(a).astype(np.float32)
    st = refdump.read_static(os.path.join(work, "oracle_static.bin"))
    for k, a in st.items():
        out["static_" + k] = np.asarray(a)
    for t in STEPS:
        d = refdump.read_step(os.path.join(work, "oracle_step_%06d.bin" % t), p.nlay, p.ndeg)
        for k, a in d.items():
            out["step%d_%s" % (t, k)] = np.asarray(a)
    _collect_files(work, "file_", out)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-24s lm=%d mm=%d nlay=%d ndeg=%d  %.1f KiB" % (name, p.lm, p.mm, p.nlay, p.ndeg,
                                                           os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    for nm in (sys.argv[1:] or list(CASES) + list(RESTART_CASES)):
        generate(nm)
