"""Rough inputs for the sweeps: no field constant, smooth or zero (helper module of test_rough_inputs_cpu and
test_gpu_rough_inputs; not a conftest, imports nothing from the code under test but the init mirror).

rough_fields(f, seed) returns a shallow copy of a Fields object whose statics and state are replaced by arrays that vary from
cell to cell, layer to layer and level to level without symmetry, with exact +0 / -0 sprinkled into the velocities and, with
ocrp = 1, thicknesses on both sides of the outcropping thresholds.  The shared object's arrays are never written; masks,
neig and subc stay the case's own.  Every array draws from a generator of its own (seed, name), so `reseed=("h_to",)`
changes that one input alone: the liveness tests use it.

Tracers: dry_cell_state and rough_tracers feed the tracer sweep of both schemes.  Scheme 1 meets them in
test_gpu_rough_inputs; scheme 2 (the flux-limited faces) in test_tracers_limited_rough_cpu, which holds the inputs to what
the staged form needs (dry cells inside interior tiles, every outer-ring read), and in test_gpu_tracers_limited_rough on
frame 321 x 50, the first with interior tiles, 321 x 83 for the bands of the island and 321 x 51 for the sill's sponge.

Amplitudes (all configurations; dt, dl, hsal the case's own):
  u, v          uniform in +-U at open faces, U = 0.05 m/s, 5 % exact +0 and 5 % exact -0
  h_u, h_v      velocity x face thickness x a factor in [0.8, 1.2] per cell (not what update_u would have stored)
  rs_h          +-0.01 m / dt per level, wet cells
  dmdx, dmdy    +-0.02 U / dt per level, open faces
  v_cc, v_ll    (0, 0.02 dl^2 / dt] per cell
  tt3d ...      +-0.005 U / dt x rho0 x the layer's own thickness, per cell and component (a bounded acceleration in thin
                layers; tt3d at most 0.5 U / invf where a sponge relaxes towards its Ekman velocity)
  hlay          internal interfaces moved by +-10 % of the thinner neighbour layer (column total kept), then +-min(eta, 2 % of
                the column) on the top layer; ocrp = 1: 0.9 / nlay (at most 0.3) of the wet cells of each layer at 1-3 hsal,
                the difference put into the layer below (above, for the last layer)
  fcor          x [0.5, 1.5] per cell;  h_to  +-(0.25-2.5) eta, never 0 in a wet cell;  h_th  +-eta, where
                eta = min(2 cm, 0.2 U cext / g): a surface step accelerates its faces by less than 0.1 U per step
  taus          +-max|taus| in both components per cell, where the case has wind
  nudg          x [0.5, 1] inside the sponge (exact 0 kept elsewhere);  fnud  thickness +-2 cm, velocities +-U there
  hdot          +-max|hdot| per cell and layer where the case has it;  tide  amplitude x [0.5, 1.5], phase +-1 rad
  bodf          +-(0.5-1) x 0.02 U / dt, distinct per layer and direction
  pi_s          with a rigid lid only: uniform in +-10 at wet cells, 0 elsewhere (the oracle's pressure on these states
                reaches 30-50 after its 1000 sweeps): a starting pressure that is no earlier solve's result

Growth: max(|u|, |v|) / U of the oracle after step plan B (steps 7-12 from the rough state), frame 130 x 18, seed 1 —
measured on the CPU oracle; the bound of the tests is 20:
  closed_leith_3l 1.8   jet_xyper_2l 13.6   soliton_xper_1l 2.7   sill_ocrp_sponge_3l 10.7   stommel_wind_drag 1.4
  island_ragged_3l 1.7   closed_svis_3l 1.4   closed_dt3d_forced_3l 1.7   sponge_obc_mcbc0_2l 1.8   tide_sponge_2l 1.8
  closed_12l_hdot 1.6   zero_visc_2l 1.6
(the jet's random divergence on a 5 m column radiates gravity waves of several U within a step; the sill's comes from the
cell-layers placed at 1-3 hsal).
The lid, outcropping-stress and private_mod3d configurations, plan A / plan B on 130 x 18, then on 321 x 50:
  lid_wind_drag_2l 8.5 / 9.8, 9.5 / 11.2   lid_coast_3l 8.2 / 10.2, 9.1 / 11.9   sill_ocrp_stress_3l 8.3 / 8.4, 8.8 / 8.9
  variant3d_sponge_3l 6.7 / 8.7, 7.0 / 8.6
(on the rough lid states every solve of both plans stops at surf_pressure's cap of 1000 sweeps, from the rough and from a
zero starting pressure; variant3d_sponge_3l: layer 3 of the eastern sponge's cells lies below / above 20 hsal in 54 / 46 %
at 130 x 18 and 50 / 50 % at 321 x 50, and variant 1 differs from variant 0 in 15 % and 6 % of the cell-layers after plan B).
"""
import copy
import zlib

import numpy as np

from beom_amd import inputs as I
from beom_amd.grid import read_input_data
from beom_amd.params import make_params
from helpers import land_mask

U0 = 0.05
STATIC_INPUTS = ("fcor", "h_to", "h_th", "taus:0", "taus:1", "nudg", "fnud", "hdot", "tide", "bodf")
STATE_INPUTS = ("hlay", "u", "v", "h_u", "h_v", "rs_h:0", "rs_h:1", "dmdx:0", "dmdx:1", "dmdx:2", "dmdy:0", "dmdy:1", "dmdy:2",
                "v_cc", "v_ll", "tt3d", "tb3d", "tu3d", "pi_s")
INPUTS = STATIC_INPUTS + STATE_INPUTS
# array name: (axis of the packed cells, axis of the layers, axis of the levels / components); None = no such axis
AXES = {"fcor": (0, None, None), "h_to": (0, None, None), "h_th": (0, None, None), "taus": (1, None, 0), "nudg": (1, None, 0),
        "fnud": (2, 1, 0), "hdot": (1, 0, None), "tide": (1, None, 0), "hlay": (1, 0, None), "u": (1, 0, None),
        "v": (1, 0, None), "h_u": (1, 0, None), "h_v": (1, 0, None), "rs_h": (1, 0, 2), "dmdx": (1, 0, 2), "dmdy": (1, 0, 2),
        "v_cc": (1, 0, None), "v_ll": (1, 0, None), "tt3d": (2, 0, 1), "tb3d": (2, 0, 1), "tu3d": (2, 0, 1),
        "pi_s": (0, None, None)}                       # (None on a case without a lid: present() leaves it out)


def present(f):
    """The arrays of AXES the Fields object f has (pi_s: with a rigid lid only)."""
    return [k for k in AXES if getattr(f, k, None) is not None]


def _rng(seed, reseed, name):
    return np.random.default_rng([int(seed) + (7919 if name in reseed else 0), zlib.crc32(name.encode())])


def _pm(r, shape):
    return r.uniform(-1.0, 1.0, shape)


def _velocity(r, open_, nlay, U):
    """Uniform in +-U at open faces, about 5 % exact +0 and 5 % exact -0; the case's 0 elsewhere."""
    a = _pm(r, (nlay, open_.size)) * U
    z = r.uniform(0.0, 1.0, a.shape)
    a = np.where(z < 0.05, 0.0, np.where(z < 0.10, -0.0, a))
    return np.where(open_[None, :], a, 0.0)


def rough_fields(f, seed, U=U0, reseed=(), visc="rough", zero=()):
    """visc: "rough" (v_cc, v_ll in (0, 0.02 dl^2/dt]), "zero" (all +0) or "neg0" (all +0 but one -0 in v_ll).
    zero: state arrays left +0 everywhere (a stress array whose forcing the handle lacks keeps the stress from folding)."""
    p = f.p
    g = copy.copy(f)
    g.has = dict(f.has)
    nlay, n1 = p.nlay, p.ndeg + 1
    dt, dl, hsal = float(p.dt), float(p.dl), float(p.hsal)
    R = lambda name: _rng(seed, reseed, name)
    wet = np.asarray(f.mk_n) > 0.5
    opu, opv = np.asarray(f.mk_u) > 0.5, np.asarray(f.mk_v) > 0.5
    cell = np.arange(n1) > 0
    W, S = f.neig[:, 4].astype(np.int64), f.neig[:, 6].astype(np.int64)
    sup = {}
    # a surface step of eta between neighbours accelerates them by about eta / 2 x sqrt(g / H) per step: kept below 0.1 U
    eta = min(0.02, 0.2 * U * float(p.cext) / float(p.grav))

    # ---- statics
    base = np.where(f.fcor != 0.0, f.fcor, 1.0e-5)
    g.fcor = np.where(cell, base * R("fcor").uniform(0.5, 1.5, n1), f.fcor)
    sup["fcor"] = cell.copy()
    r = R("h_to")
    g.h_to = np.where(wet, np.where(r.uniform(0, 1, n1) < 0.5, -1.0, 1.0) * r.uniform(0.25, 2.5, n1) * eta, 0.0)
    sup["h_to"] = wet.copy()
    g.h_th = f.h_th + np.where(wet, _pm(R("h_th"), n1) * eta, 0.0)
    sup["h_th"] = wet.copy()
    wind = bool(np.any(np.abs(f.taus) > 1.0e-7))
    g.taus = np.array(f.taus, dtype=np.float64)
    sup["taus"] = np.zeros(g.taus.shape, bool)
    if wind:
        amp = float(np.max(np.abs(f.taus)))
        for c in (0, 1):
            g.taus[c] = np.where(cell, _pm(R("taus:%d" % c), n1) * amp, 0.0)
            sup["taus"][c] = cell
    sponge = np.asarray(f.nudg) != 0.0                              # [3, n1]
    g.nudg = np.where(sponge, f.nudg * R("nudg").uniform(0.5, 1.0, f.nudg.shape), f.nudg)
    sup["nudg"] = sponge.copy()
    r = R("fnud")
    g.fnud = np.array(f.fnud, dtype=np.float64)
    g.fnud[0] = np.where(sponge[0][None] & wet[None], f.fnud[0] + _pm(r, (nlay, n1)) * 0.02, f.fnud[0])
    g.fnud[1] = np.where(sponge[1][None] & opu[None], _pm(r, (nlay, n1)) * U, f.fnud[1])
    g.fnud[2] = np.where(sponge[2][None] & opv[None], _pm(r, (nlay, n1)) * U, f.fnud[2])
    sup["fnud"] = np.stack([np.broadcast_to(m[None], (nlay, n1)) for m in (sponge[0] & wet, sponge[1] & opu, sponge[2] & opv)])
    g.hdot = np.array(f.hdot, dtype=np.float64)
    sup["hdot"] = np.zeros(g.hdot.shape, bool)
    if f.has.get("hdot", False) and np.any(f.hdot != 0.0):
        g.hdot = np.where(wet[None], _pm(R("hdot"), (nlay, n1)) * float(np.max(np.abs(f.hdot))), 0.0)
        sup["hdot"] = np.broadcast_to(wet[None], g.hdot.shape).copy()
    g.tide = np.array(f.tide, dtype=np.float64)
    sup["tide"] = np.zeros(g.tide.shape, bool)
    if f.has.get("tide", False) and np.any(f.tide != 0.0):
        r = R("tide")
        on = f.tide[:, :, 0, 0] != 0.0                               # where the constituent has an amplitude
        g.tide[:, :, 0, 0] = np.where(on, f.tide[:, :, 0, 0] * r.uniform(0.5, 1.5, on.shape), 0.0)
        g.tide[:, :, 0, 1] = np.where(on, f.tide[:, :, 0, 1] + _pm(r, on.shape), f.tide[:, :, 0, 1])
        sup["tide"][:, :, 0, 0] = on; sup["tide"][:, :, 0, 1] = on
    r = R("bodf")
    g.bodf = np.where(r.uniform(0, 1, (2, nlay)) < 0.5, -1.0, 1.0) * r.uniform(0.5, 1.0, (2, nlay)) * (0.02 * U / dt)
    g.has["bodf"] = True

    # ---- state: thicknesses first (the transports and the stresses scale with them)
    r = R("hlay")
    h = np.array(f.hlay, dtype=np.float64)
    for k in range(nlay - 1):                                        # internal interfaces: the column total is kept
        d = _pm(r, n1) * 0.1 * np.minimum(h[k], h[k + 1])
        d = np.where(wet, d, 0.0)
        h[k] = h[k] + d; h[k + 1] = h[k + 1] - d
    if float(p.ocrp) > 0.5 and nlay > 1:                             # a share of cell-layers at 1-3 hsal
        share = min(0.3, 0.9 / nlay)
        pick = r.uniform(0.0, 1.0, n1)
        thin = r.uniform(1.0, 3.0, (nlay, n1)) * hsal
        for k in range(nlay):
            to = k + 1 if k < nlay - 1 else k - 1
            move = h[k] - thin[k]
            ok = wet & (pick >= k * share) & (pick < (k + 1) * share) & (h[to] + move > 3.0 * hsal) & (h[to] > 3.0 * hsal)
            h[to] = np.where(ok, h[to] + move, h[to])
            h[k] = np.where(ok, thin[k], h[k])
    col = h.sum(axis=0)
    h[0] = h[0] + np.where(wet, _pm(r, n1) * np.minimum(eta, 0.02 * col), 0.0)
    g.hlay = h
    sup["hlay"] = np.broadcast_to(wet[None], h.shape).copy()
    g.u = _velocity(R("u"), opu, nlay, U)
    g.v = _velocity(R("v"), opv, nlay, U)
    hcu = (h + h[:, W]) / (1.0 + np.asarray(f.mk_u))[None]
    hcv = (h + h[:, S]) / (1.0 + np.asarray(f.mk_v))[None]
    g.h_u = g.u * hcu * R("h_u").uniform(0.8, 1.2, (nlay, n1))
    g.h_v = g.v * hcv * R("h_v").uniform(0.8, 1.2, (nlay, n1))
    for k, m in (("u", opu), ("h_u", opu), ("v", opv), ("h_v", opv)):
        sup[k] = np.broadcast_to(m[None], (nlay, n1)).copy()
    g.rs_h = np.zeros((nlay, n1, 2))
    for lev in (0, 1):
        g.rs_h[:, :, lev] = np.where(wet[None], _pm(R("rs_h:%d" % lev), (nlay, n1)) * (0.01 / dt), 0.0)
    sup["rs_h"] = np.broadcast_to(wet[None, :, None], g.rs_h.shape).copy()
    for k, m in (("dmdx", opu), ("dmdy", opv)):
        a = np.zeros((nlay, n1, 3))
        for lev in range(3):
            a[:, :, lev] = np.where(m[None], _pm(R("%s:%d" % (k, lev)), (nlay, n1)) * (0.02 * U / dt), 0.0)
        setattr(g, k, a)
        sup[k] = np.broadcast_to(m[None, :, None], a.shape).copy()
    for k in ("v_cc", "v_ll"):
        a = np.zeros((nlay, n1))
        if visc == "rough":
            a = np.where(cell[None], (1.0 - R(k).uniform(0.0, 1.0, (nlay, n1))) * (0.02 * dl * dl / dt), 0.0)
        elif visc == "neg0" and k == "v_ll":
            a[nlay - 1, n1 // 2] = -0.0
        else:
            assert visc in ("zero", "neg0"), visc
        setattr(g, k, a)
        sup[k] = np.broadcast_to(cell[None], a.shape).copy() if visc == "rough" else np.zeros(a.shape, bool)
    for k, m in (("tt3d", None), ("tb3d", None), ("tu3d", None)):
        r = R(k)
        a = np.zeros((nlay, 2, n1))
        acc = 0.005 * U / dt
        if k == "tt3d" and sponge[1:].any() and float(f.invf) != 0.0:
            acc = min(acc, 0.5 * U / abs(float(f.invf)))            # (a sponge relaxes towards tt3d x invf / (rho h): below U / 2)
        amp = acc * float(p.rho0)
        a[:, 0] = np.where(opu[None], _pm(r, (nlay, n1)) * amp * hcu, 0.0)
        a[:, 1] = np.where(opv[None], _pm(r, (nlay, n1)) * amp * hcv, 0.0)
        setattr(g, k, a)
        sup[k] = np.stack([np.broadcast_to(opu[None], (nlay, n1)), np.broadcast_to(opv[None], (nlay, n1))], axis=1)
    if float(p.rgld) > 0.5:                                          # a starting pressure that is no solve's result
        g.pi_s = np.where(wet, _pm(R("pi_s"), n1) * 10.0, 0.0)
        sup["pi_s"] = wet.copy()
    for k in zero:
        setattr(g, k, np.zeros_like(getattr(g, k)))
        sup[k] = np.zeros(sup[k].shape, bool)
    g.rough_support = sup
    return g


def dry_cell_state(f, seed, U=U0, share=0.13):
    """A rough state for the h and tracer sweeps alone: exact +0 thickness in about 10 % of the wet cell-layers, no two of them
    neighbours in x or y (a face between two empty cells carries no tracer, whatever its transport: the identity "a tracer
    of concentration 1 is the thickness" would not hold there), and non-zero transports at every open face."""
    g = rough_fields(f, seed, U)
    p = f.p
    nlay, n1 = p.nlay, p.ndeg + 1
    r = _rng(seed, (), "dry")
    wet = np.asarray(f.mk_n) > 0.5
    E, N = f.neig[:, 0].astype(np.int64), f.neig[:, 2].astype(np.int64)
    cand = (r.uniform(0.0, 1.0, (nlay, n1)) < share) & wet[None]
    dry = cand & ~cand[:, E] & ~cand[:, N]
    g.hlay = np.where(dry, 0.0, g.hlay)
    hmean = np.array([g.hlay[k][wet].mean() for k in range(nlay)])[:, None]
    for k, m in (("h_u", f.mk_u), ("h_v", f.mk_v)):
        s = np.where(r.uniform(0.0, 1.0, (nlay, n1)) < 0.5, -1.0, 1.0)
        setattr(g, k, np.where((np.asarray(m) > 0.5)[None], s * r.uniform(0.2, 1.0, (nlay, n1)) * U * hmean, 0.0))
    g.dry = dry
    return g


def rough_tracers(f, h, ntrc, seed):
    """q, rq, ctrg of ntrc tracers on thicknesses h: tracer 0 has concentration 1 and relaxation concentration 1 and the
    thickness' own history (its content is the thickness); the others are rough in every cell, layer and level."""
    p = f.p
    n = (ntrc, p.nlay, p.ndeg + 1)
    r = _rng(seed, (), "tracers")
    c = r.uniform(0.1, 1.0, n)
    ctrg = r.uniform(0.1, 1.0, n)
    c[0] = 1.0; ctrg[0] = 1.0
    c[:, :, 0] = 0.0
    q = np.ascontiguousarray(c * np.asarray(h, dtype=np.float64)[None])
    rq = _pm(r, n + (2,)) * (0.01 / float(p.dt)) * (np.asarray(f.mk_n) > 0.5)[None, None, :, None]
    rq[0] = f.rs_h
    return q, np.ascontiguousarray(rq), np.ascontiguousarray(ctrg)


# ---- the three input conditions ------------------------------------------------------------------------------------------
def shifted_fractions(g, name):
    """{shift: fraction of places where the roughened array `name` of g differs from its copy shifted by one cell in x, one
    cell in y, one layer, one level}; places = where the array and its shifted copy are both roughened.  Shifts the array
    does not have, or has no place for, are left out."""
    a, sup = np.asarray(getattr(g, name)), g.rough_support[name]
    ca, la, va = AXES[name]
    out = {}
    for shift, nb in (("x", g.neig[:, 4]), ("y", g.neig[:, 6])):
        b, sb = np.take(a, nb.astype(np.int64), axis=ca), np.take(sup, nb.astype(np.int64), axis=ca)
        ok = sup & sb
        if ok.any():
            out[shift] = float(np.mean(a[ok] != b[ok]))
    for shift, ax in (("layer", la), ("level", va)):
        if ax is None or a.shape[ax] < 2:
            continue
        lo = [slice(None)] * a.ndim; hi = [slice(None)] * a.ndim
        lo[ax] = slice(0, -1); hi[ax] = slice(1, None)
        ok = sup[tuple(lo)] & sup[tuple(hi)]
        if ok.any():
            out[shift] = float(np.mean(a[tuple(lo)][ok] != a[tuple(hi)][ok]))
    return out


def straddling(g):
    """Per layer: (share of wet cell-layers below 2 hsal, share above)."""
    wet = np.asarray(g.mk_n) > 0.5
    two = 2.0 * float(g.p.hsal)
    return [(float(np.mean(g.hlay[k][wet] < two)), float(np.mean(g.hlay[k][wet] > two))) for k in range(g.p.nlay)]


def bounded(g, state, U=U0):
    """The oracle's result is finite, wet thicknesses are positive and max |u|, |v| <= 20 U.  Returns the growth factor."""
    wet = np.asarray(g.mk_n) > 0.5
    for k, a in state.items():
        assert np.isfinite(a).all(), k
    assert (state["hlay"][:, wet] > 0.0).all()
    growth = max(float(np.max(np.abs(state["u"]))), float(np.max(np.abs(state["v"])))) / U
    assert growth <= 20.0, growth
    return growth


# ---- configurations ------------------------------------------------------------------------------------------------------
def _with_land(pf):
    p, files = pf
    files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
    land = land_mask(p, True)
    files["h_bo"][land] = 0.0
    if "init" in files:
        files["init"][land] = 0.0
    return p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"])), files


def _sponges(p, width=9):
    """Western and eastern sponges on eta and u, the dry margin columns included (so that, with mcbc = 0, the boundary cells
    are found as segments of no_gradient_obc)."""
    nudg = np.zeros((p.lm + 2, p.mm + 2, 3))
    for i in range(0, width):
        nudg[i, :, 0:2] = 0.3 * (width - i) / width
    for i in range(p.lm + 1, p.lm + 1 - width, -1):
        w = 0.25 * (i - (p.lm + 1 - width)) / width
        nudg[i, :, 0] = np.maximum(nudg[i, :, 0], w); nudg[i, :, 1] = np.maximum(nudg[i, :, 1], w)
    return nudg


def _sponge_obc(lm, mm):
    p, files = I.case_headline(lm, mm, 2)
    return p.replace(mcbc="0."), dict(files, nudg=_sponges(p))


def _tide_sponge(lm, mm):
    p, files = I.case_headline(lm, mm, 2)
    tide = np.zeros((2, 1, lm + 2, mm + 2, 3))
    tide[0, 0, :, :, 0] = 0.02; tide[0, 0, :, :, 1] = 0.01; tide[0, 0, :, :, 2] = 0.01       # amplitudes of eta, u, v
    tide[1, 0, :, :, 1] = np.pi / 2.0; tide[1, 0, :, :, 2] = np.pi / 3.0                   # phases
    tide[0, 0, 0, 0, 0] = 2.0 * np.pi / (12.4206012 / 24.0)                                # M2, rad/day, in the first element
    return p, dict(files, nudg=_sponges(p), tide=tide)


def _dt3d_forced(lm, mm):
    p, files = I.case_headline(lm, mm, 3)
    return p.replace(dt3d="%.9f" % (3.2 * float(p.dt) / 86400.0), bdrg="1.e-3", tdrg="5.e-4", qdrg="0.5",
                     tauw=["0.05", "0.02"]), files


def _lid(nlay, coast=False, tauw=("0.05", "0.02")):
    """The rigid lid (rgld = 1; its operators need ocrp = 1) on the headline basin with wind and bottom drag, no multistep
    term.  coast: land north of row 0.8 mm — a straight coast (at a cell with four dry faces, as a ragged coast has them,
    the reference's operators are 1/0 and the oracle gives NaN from step 1)."""
    def make(lm, mm):
        p, files = I.case_headline(lm, mm, nlay)
        p = p.replace(rgld="1.", ocrp="1.", g_fb="0.", bdrg="2.e-4", tauw=list(tauw))
        if coast:
            files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
            files["h_bo"][:, int(0.8 * p.mm) + 1:] = 0.0
            p = p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"]))
        return p, files
    return make


LID_REST_WINDS = {"strong": ("5.", "2."), "mild": ("0.5", "0.2")}


def lid_from_rest(tauw, frame="130x18"):
    """Fields of the 2-layer lid case started from rest under the wind tauw (two literals): the solves converge, in a
    number of sweeps that depends on the wind."""
    p, files = _lid(2, tauw=tauw)(*FRAMES[frame])
    return read_input_data(p, files=files)


def _sill_stress(lm, mm):
    p, files = CONFIGS["sill_ocrp_sponge_3l"][0](lm, mm)
    return p.replace(bdrg="1.e-3", tdrg="5.e-4", qdrg="0.5", tauw=["0.05", "0.02"]), files


def _variant3d_sponge(lm, mm):
    """case_3d_variant of tests/golden/make_golden.py (the update_h epilogue of private_mod3d.f95, :1635-1683) on any frame,
    with layer 3 at 200 m = 20 hsal in the east before roughening, and sponges on eta 12 columns wide at both ends at a
    tenth of the golden's rates (with the golden's own the oracle's growth on the rough state is 22-37 U)."""
    nlay = 3
    h_bo = np.zeros((lm + 2, mm + 2)); h_bo[1:-1, 1:-1] = 900.0
    nudg = np.zeros((lm + 2, mm + 2, 3))
    for i in range(1, 13):
        nudg[i, :, 0] = 0.1 * 0.25 * (13 - i) / 12.0
        nudg[lm + 1 - i, :, 0] = 0.1 * 0.20 * (13 - i) / 12.0
    nudg[0:3, :, 1] = 0.02                           # a nudged western segment must exist (:1226-1231)
    init = np.zeros((lm + 2, mm + 2, nlay, 3))
    x = (np.arange(lm + 2) - lm // 2)[:, None] * np.ones((1, mm + 2))
    init[:, :, 1, 0] = 20.0 * np.tanh(x / 4.0)
    init[:, :, 2, 0] = 20.0 * (x > 3)
    cext = np.sqrt(9.8 * 900.0); dl = 1.0e3; dt = 0.5 * dl / cext
    p = make_params(lm, mm, nlay, I.get_nbr_deg_freedom(h_bo), dl, cext, 1.0e-4, [1026.0, 1027.0, 1028.0], [0.0, 0.3, 0.8],
                    12 * dt / 86400.0, 1.0, 0.0, 0.0, 0.0, 0.2, 0.0, 1.0, 10.0, 10.0, 1.0, 1.0,
                    0.0, 0.0, 0.0, 0.0, 0.0, 0.0, desc="rough inputs: private_mod3d update_h epilogue")
    return p, {"h_bo": h_bo, "nudg": nudg, "init": init}


def _closed_12l(lm, mm):
    p, files = I.case_headline(lm, mm, 12)
    hdot = np.zeros((lm + 2, mm + 2, 12))
    hdot[1:-1, 1:-1, :] = 1.0e-5
    return p, dict(files, hdot=hdot)


# name: ((lm, mm) -> (params, files), options set on the handle, embedded handle?)
CONFIGS = {
    "closed_leith_3l": (lambda lm, mm: I.case_headline(lm, mm, 3), {}, False),
    "jet_xyper_2l": (lambda lm, mm: I.case_unstable_jet(lm=lm, mm=mm, nlay=2, dt_s=1.5), {}, False),
    "soliton_xper_1l": (lambda lm, mm: I.case_soliton(lm=lm, mm=mm, dt_s=5.0), {}, False),
    "sill_ocrp_sponge_3l": (lambda lm, mm: I.case_sill_exchange3d(lm=lm, mm=mm, nlay=3, dt_s=0.01, npts=5,
                                                                   sill_halfwidth=max(3.0, mm / 6.0)), {}, False),
    "stommel_wind_drag": (lambda lm, mm: I.case_stommel(lm=lm, mm=mm, dl=50.0e3, dt_s=0.2), {}, False),
    "stommel_wind_drag_unfolded": (lambda lm, mm: I.case_stommel(lm=lm, mm=mm, dl=50.0e3, dt_s=0.2), {"fold_stress": 0}, False),
    "island_ragged_3l": (lambda lm, mm: _with_land(I.case_headline(lm, mm, 3)), {}, True),
    "closed_svis_3l": (lambda lm, mm: (lambda pf: (pf[0].replace(svis="1.e9"), pf[1]))(I.case_headline(lm, mm, 3)), {}, False),
    "closed_dt3d_forced_3l": (_dt3d_forced, {}, False),
    "sponge_obc_mcbc0_2l": (_sponge_obc, {}, False),
    "tide_sponge_2l": (_tide_sponge, {}, False),
    "closed_12l_hdot": (_closed_12l, {}, False),
    "zero_visc_2l": (lambda lm, mm: I.case_headline(lm, mm, 2, dvis=0.0), {}, False),
    "lid_wind_drag_2l": (_lid(2), {}, False),
    "lid_coast_3l": (_lid(3, coast=True), {}, True),
    "sill_ocrp_stress_3l": (_sill_stress, {}, False),
    "variant3d_sponge_3l": (_variant3d_sponge, {}, False),
}
# the `variant` of the oracle and of the engine (1: the update_h epilogue of private_mod3d.f95); 0 where not listed
ENGINE_VARIANT = {"variant3d_sponge_3l": 1}


def variant_of(config):
    return ENGINE_VARIANT.get(config, 0)


# handles with one forcing only, for the gates of the folded stress (not part of the sweep over CONFIGS)
GATE_CONFIGS = {
    "closed_wind_only_2l": (lambda lm, mm: (lambda pf: (pf[0].replace(tauw=["0.05", "0.02"]), pf[1]))(I.case_headline(lm, mm, 2)), {}, False),
    "closed_drag_only_2l": (lambda lm, mm: (lambda pf: (pf[0].replace(bdrg="1.e-3"), pf[1]))(I.case_headline(lm, mm, 2)), {}, False),
}
FRAMES = {"130x18": (130, 18), "321x50": (321, 50), "130x99": (130, 99), "4200x9": (4200, 9),
          # for the output records: one tile, 512 cell slots in three workgroups of the scan (the last holds cell ndeg alone);
          # lm + 1 = 193 = 1 mod 64, a row pitch padded by 15
          "63x7": (63, 7), "192x30": (192, 30),
          # for the bands under tracer scheme 2: on island_ragged_3l every window of 2 and of 3 bands holds an interior tile of
          # both geometries (on 321 x 50 the ragged corner leaves band 0 of 3 without one)
          "321x83": (321, 83),
          # the sill's northern sponge (the last six rows) inside an interior 64 x 8 tile of the flux-limited tracer sweep: a
          # tile row ends at row 48 of 52 (on 321 x 50 the last interior one ends at row 40 of 51)
          "321x51": (321, 51)}
_BASE = {}


def base_fields(config, frame):
    """The case's own Fields, built once per (config, frame); callers get a shallow copy and set attributes only."""
    key = (config, frame)
    if key not in _BASE:
        p, files = dict(CONFIGS, **GATE_CONFIGS)[config][0](*FRAMES[frame])
        if float(p.g_fb) == 0.0 and float(p.rgld) < 0.5:
            p = p.replace(g_fb="1.")                   # (the multistep terms are what the history levels are for; a lid has none)
        _BASE[key] = read_input_data(p, files=files)
    return copy.copy(_BASE[key])


def switched_off(p, f):
    """The inputs of INPUTS a configuration does not read in step plan B, from its parameters: what the liveness test
    expects to be dead, so that nothing is silently untested."""
    off = set()
    n3 = p.n_3d
    if float(p.svis) > 0.0 or (float(p.dvis) > 1.0e-3 and n3 == 1):
        off |= {"v_cc", "v_ll"}                        # biharmonic form, or Leith refreshed on every step
    wind = bool(np.any(np.abs(f.taus) > 1.0e-7))
    if not wind:
        off |= {"taus:0", "taus:1"}
    if n3 == 1:                                        # a forcing that is on rewrites its array on every step
        if wind: off.add("tt3d")
        if float(p.bdrg) > 1.0e-7: off.add("tb3d")
        if float(p.tdrg) > 1.0e-7: off.add("tu3d")
    if not np.any(f.nudg != 0.0):
        off |= {"nudg", "fnud"}
    if not (f.has.get("hdot", False) and np.any(f.hdot != 0.0)):
        off.add("hdot")
    if not (f.has.get("tide", False) and np.any(f.tide != 0.0)):
        off.add("tide")
    if float(p.rgld) > 0.5:
        # no multistep with a lid (gene = 0 on every step, private_mod.f95:1880-1884): the history levels of update_h and of
        # update_u / update_v are multiplied by 0; and from step 4 on the transports are rebuilt from u and hlay before
        # update_h reads them (:2237-2257), so the uploaded ones are never read
        off |= {"rs_h:0", "rs_h:1", "dmdx:0", "dmdx:1", "dmdx:2", "dmdy:0", "dmdy:1", "dmdy:2", "h_u", "h_v"}
    else:
        off.add("pi_s")
    return off
