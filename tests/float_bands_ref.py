"""Inputs and the restatement's trajectories for floats on bands: helper module of test_float_bands_cpu and
test_gpu_float_bands, not a conftest; imports nothing from the code under test but the input builders.

The frames are the ones the moments tests cut into bands; the floats are half floats_ref.seed_floats and half seeded in wet
cells within a strip around every seam between bands (on a ring the seam y = 0 = mm too), so that hand-overs are the rule and
not the exception.  `owner_changes` reads a trajectory of the restatement alone: who owns a float is a matter of its home
row floor(y) + 1 and the bands' rows, nothing a device has computed."""
import numpy as np

import floats_ref as R
from beom_amd import inputs as I
from beom_amd.grid import read_input_data

NSTEPS, CDT, SEED = 12, 0.9, 1
COUNTS = (3, 1000, 4096)                  # fewer than a wave, not a multiple of the block, several blocks
STRIP = 2                                 # rows on either side of a seam that take the seam floats
# 2 bands of the island frame: the seam y = 51 meets the ellipse where its coast runs straight north-south (u is masked to zero
# there and hardly a step is rejected: 6 in 12 steps of 4096 floats); 20 rows reach the staircase (28 rejected, 180 owner changes)
STRIPS = {("island", 2): 20}

# the rows each band owns, fixed by hand (own0, own1): 101 and 96 rows dealt evenly, remainders first; the island frame's
# bands hold equal numbers of packed cells.  test_gpu_float_bands checks them against MultiEngine.band.
CUTS = {("closed", 2): ((1, 51), (52, 101)), ("closed", 3): ((1, 34), (35, 68), (69, 101)),
        ("island", 2): ((1, 51), (52, 101)), ("island", 3): ((1, 30), (31, 72), (73, 101)),
        ("ring", 2): ((1, 48), (49, 96)), ("ring", 1): ((1, 96),)}
CASES = tuple(CUTS)

_FRAMES = {}


def frame(name):
    """closed: 48 x 100 x 2; island: the same with the elliptic island of test_gpu_moments; ring: the jet 40 x 96 x 2, periodic in x and y"""
    if name not in _FRAMES:
        if name == "ring":
            p, files = I.case_unstable_jet(lm=40, mm=96, nlay=2, dt_s=1.5)
        else:
            p, files = I.case_headline(48, 100, 2)
            if name == "island":
                files = {k: np.array(v, dtype=np.float64) for k, v in files.items()}
                x = np.arange(p.lm + 2)[:, None]; y = np.arange(p.mm + 2)[None, :]
                land = ((x - 0.4 * p.lm) / (0.2 * p.lm)) ** 2 + ((y - 0.5 * p.mm) / (0.3 * p.mm)) ** 2 < 1.0
                files["h_bo"][land] = 0.0
                files["init"][land] = 0.0
                p = p.replace(ndeg=I.get_nbr_deg_freedom(files["h_bo"]))
        _FRAMES[name] = read_input_data(p, files=files)
    return _FRAMES[name]


_REAL_FRAMES = {}


def real_frame(name):
    """The frame whose real steps carry floats across the seams.  The jet of the ring is antisymmetric about its axis y = mm / 2
    and at rest in y: after 12 steps |v| is 3e-18 on the face y = 48 and 2e-36 on y = 0 — the two seams of 2 bands — so no
    float within reach of a seam ever crosses it.  The ring therefore starts with a meridional flow added to its state,
    v + A sin(2 pi x / lm) on the open v faces, A = 0.3 rows / (NSTEPS cdt): northward in one half of the frame and southward in
    the other, at every seam.  The other frames start as they are."""
    if name != "ring":
        return frame(name)
    if name not in _REAL_FRAMES:
        import copy
        f0 = frame(name)
        fr = R.Frame(f0)
        f = copy.copy(f0)
        a = 0.3 / (NSTEPS * cdt_of(f0))
        f.v = np.ascontiguousarray(np.asarray(f0.v, dtype=np.float64)
                                   + a * np.sin(2.0 * np.pi * (fr.i - 0.5) / fr.lm)[None, :] * np.asarray(f0.mk_v, dtype=np.float64)[None, :])
        _REAL_FRAMES[name] = f
    return _REAL_FRAMES[name]


def cdt_of(f):
    """dt * i_dl as the engine forms it: i_dl = 1.0 / dl first."""
    return float(f.p.dt) * (1.0 / float(f.p.dl))


def seams(name, cuts):
    """y of every seam between two bands: own1 of each band but the last of a chain; on a ring also 0 = mm (the last band's north)"""
    s = [float(c[1]) for c in cuts[:-1]]
    if name == "ring":
        s.append(0.0)
    return s


def _near(fr, r, n, seam, reach, decades=0):
    """n floats in wet cells within `reach` of y = seam (both sides; a ring wraps): the distance is reach * uniform, or with
    `decades` reach * 10^(-decades * uniform) — real velocities near a seam may be orders of magnitude below the frame's
    largest, and floats at every scale of distance make sure some cross.  In a row with a coast, the wet cells next to land
    are taken eight times as often as the others (the landing rule's other branches)."""
    u = r.uniform(0.0, 1.0, n)
    y = seam + reach * (10.0 ** (-decades * u) if decades else u) * np.where(r.integers(0, 2, n) == 1, 1.0, -1.0)
    if fr.yper:
        y = np.where(y < 0.0, y + fr.mm, y)
        y = np.where(y >= fr.mm, y - fr.mm, y)
    x = np.zeros(n)
    j = np.floor(y).astype(np.int64) + 1
    for row in np.unique(j):
        cells = fr.cmap[1:fr.lm + 1, row]
        wet = fr.wetc[cells]
        assert wet.any(), "no wet cell in row %d" % row
        coast = wet & (~np.roll(wet, 1) | ~np.roll(wet, -1) | ~fr.wetc[fr.cmap[1:fr.lm + 1, row + 1]] | ~fr.wetc[fr.cmap[1:fr.lm + 1, row - 1]])
        if not fr.xper:
            coast[[0, -1]] = False                               # (the frame's own walls are no island)
        w = np.where(wet, 1.0, 0.0) + 7.0 * coast
        t = np.flatnonzero(j == row)
        i = r.choice(fr.lm, size=t.size, p=w / w.sum())         # 0-based column: the cell spans [i, i + 1)
        x[t] = np.minimum(i + r.uniform(0.0, 1.0, t.size), np.nextafter(i + 1.0, 0.0))
    return x, y


def seed(f, name, cuts, n, reach=float(STRIP), decades=0, seed_=SEED):
    """n floats: the first half anywhere in the water (floats_ref.seed_floats), the rest dealt to the seams"""
    fr = R.Frame(f)
    nh = n - n // 2
    x, y, layer = R.seed_floats(f, n, seed_)
    r = np.random.default_rng([int(seed_), 77, n])
    ss = seams(name, cuts)
    for k, t in enumerate(np.array_split(np.arange(nh, n), max(len(ss), 1))):
        if ss and t.size:
            x[t], y[t] = _near(fr, r, t.size, ss[k], reach, decades)
    assert fr.wet(x, y).all()
    return x, y, layer


def owner(cuts, y):
    """index of the band whose rows hold floor(y) + 1 (-1: none)"""
    j = np.floor(y).astype(np.int64) + 1
    o = np.full(j.shape, -1, dtype=np.int64)
    for k, (a, b) in enumerate(cuts):
        o[(j >= a) & (j <= b)] = k
    return o


class Changes:
    """Owner changes along a trajectory ys[0..T] (positions after each step; ys[0] the seeds), per seam and direction."""

    def __init__(self, name, cuts, ys, mm):
        ss = seams(name, cuts)
        self.total = 0
        self.north = {s: 0 for s in ss}          # crossings towards larger y (on a ring: ... -> mm -> 0 -> ...)
        self.south = {s: 0 for s in ss}
        self.per_step = []
        seq = [owner(cuts, y) for y in ys]
        assert all((o >= 0).all() for o in seq)
        for t in range(1, len(ys)):
            ch = seq[t] != seq[t - 1]
            self.per_step.append(int(ch.sum()))
            self.total += int(ch.sum())
            dy = ys[t] - ys[t - 1]
            wrapped = np.abs(dy) > 0.5 * mm                    # through y = 0 = mm
            up = np.where(wrapped, dy < 0.0, dy > 0.0)
            for s in ss:
                if s == 0.0:
                    at = ch & wrapped
                else:
                    lo, hi = np.minimum(ys[t], ys[t - 1]), np.maximum(ys[t], ys[t - 1])
                    at = ch & ~wrapped & (lo < s) & (hi >= s)
                self.north[s] += int(np.sum(at & up)); self.south[s] += int(np.sum(at & ~up))
        o = np.stack(seq)                                       # [T+1, n]
        away = np.cumsum(o != o[0], axis=0) > 0                 # the float has been with another band by step t
        self.came_back = int(np.sum(np.any(away[:-1] & (o[1:] == o[0]), axis=0)))      # floats handed over that came home again
        self.seam_wraps_north = sum(int(np.sum((np.abs(ys[t] - ys[t - 1]) > 0.5 * mm) & (ys[t] < ys[t - 1]))) for t in range(1, len(ys)))
        self.seam_wraps_south = sum(int(np.sum((np.abs(ys[t] - ys[t - 1]) > 0.5 * mm) & (ys[t] > ys[t - 1]))) for t in range(1, len(ys)))


_ROUGH = {}


def rough_reference(name, nb, n, vmax_cdt=CDT):
    """The restatement on rough velocities scaled to cdt * max|u| = vmax_cdt: (x0, y0, layer, steps), steps[t-1] =
    (before, after, x, y, rejected) — computed once per case and count, shared by the tests, never changed."""
    key = (name, nb, n, vmax_cdt)
    if key not in _ROUGH:
        f = frame(name)
        fr, cdt = R.Frame(f), cdt_of(f)
        amp = vmax_cdt / cdt
        x0, y0, layer = seed(f, name, CUTS[(name, nb)], n, reach=float(STRIPS.get((name, nb), STRIP)))
        x, y, rej, steps = x0, y0, np.zeros(n, dtype=np.int32), []
        for t in range(1, NSTEPS + 1):
            before, after = R.rough_velocities(f, SEED, 2 * t - 1, amp), R.rough_velocities(f, SEED, 2 * t, amp)
            x, y, branch = R.step(fr, before, after, x, y, layer, cdt)
            rej = rej + (branch != 0).astype(np.int32)
            steps.append((before, after, x, y, rej))
        _ROUGH[key] = (x0, y0, layer, steps)
    return _ROUGH[key]


def rough_changes(name, nb, n):
    x0, y0, layer, steps = rough_reference(name, nb, n)
    return Changes(name, CUTS[(name, nb)], [y0] + [s[3] for s in steps], int(frame(name).p.mm))
