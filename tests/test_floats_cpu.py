"""The numpy restatement of the float scheme (floats_ref) held to conditions on inputs of its own, before any device comparison
means anything: the rough inputs move floats across cells, seams and coasts in every way the scheme distinguishes, and an
analytic yardstick pins the interpolation and Heun's factor.  No GPU."""
import numpy as np
import pytest

import floats_ref as R
from helpers import Golden

FIXTURES = ("random_coast_2l_xper", "jet_2l_xyper", "soliton_31x15_xper", "island_3l_forced")
LAND = ("random_coast_2l_xper", "island_3l_forced")
NFLOATS, NSTEPS, CDT, SEED = 4096, 12, 0.9, 1


def rough_run(f, n=NFLOATS, nsteps=NSTEPS, cdt=CDT, amp=1.0, seed=SEED):
    """The run the CPU conditions and the device comparison share: velocities redrawn for every stage.  Yields
    (step, before, after, x, y, branch) with x, y the positions after the step."""
    fr = R.Frame(f)
    x, y, layer = R.seed_floats(f, n, seed)
    yield 0, None, None, x, y, layer
    for t in range(1, nsteps + 1):
        before, after = R.rough_velocities(f, seed, 2 * t - 1, amp), R.rough_velocities(f, seed, 2 * t, amp)
        x, y, branch = R.step(fr, before, after, x, y, layer, cdt)
        yield t, before, after, x, y, branch


@pytest.mark.parametrize("name", FIXTURES)
def test_rough_inputs_exercise_the_scheme(name):
    f = Golden(name).fields()
    fr = R.Frame(f)
    run = rough_run(f)
    _, _, _, x, y, layer = next(run)
    assert layer.min() == 1 and layer.max() == f.p.nlay
    moved = wraps_x = wraps_y = rejected = 0
    branches = np.zeros(4, dtype=np.int64)
    for t, before, after, xn, yn, branch in run:
        assert fr.wet(xn, yn).all(), (name, t, "a float left the water")
        moved += int(np.sum(fr.cell(xn, yn) != fr.cell(x, y)))
        wraps_x += int(np.sum(np.abs(xn - x) > 0.5 * fr.lm))
        wraps_y += int(np.sum(np.abs(yn - y) > 0.5 * fr.mm))
        rejected += int(np.sum(branch != 0))
        branches += np.bincount(branch, minlength=4)
        x, y = xn, yn
    total = NFLOATS * NSTEPS
    print("%s: cell changes %.1f %%, wraps x %d y %d, rejected %d of %d (%.2f %%), branches %s"
          % (name, 100.0 * moved / total, wraps_x, wraps_y, rejected, total, 100.0 * rejected / total, branches.tolist()))
    assert moved >= 0.2 * total, (name, moved, total)
    assert fr.xper == (float(f.p.xper) > 0.5) and fr.yper == (float(f.p.yper) > 0.5)
    if fr.xper:
        assert wraps_x >= 10, (name, wraps_x)
    else:
        assert wraps_x == 0
    if fr.yper:
        assert wraps_y >= 10, (name, wraps_y)
    else:
        assert wraps_y == 0
    if name in LAND:
        assert rejected >= 20, (name, rejected)
        assert rejected <= 0.05 * total, (name, rejected)
        assert (branches[:3] > 0).all(), (name, branches)


def test_every_landing_branch_is_taken():
    """The random floats of the land fixtures take the first three candidates; hand-placed floats at coast corners of the
    random coast take each of the four (floats_ref.corner_floats says why the last needs velocities without the masks)."""
    f = Golden("random_coast_2l_xper").fields()
    fr = R.Frame(f)
    x, y, layer, uv, cdt, want = R.corner_floats(f)
    assert fr.wet(x, y).all()
    xn, yn, branch = R.step(fr, uv, uv, x, y, layer, cdt)
    assert branch.tolist() == want.tolist() and sorted(branch.tolist()) == [0, 1, 2, 3]
    assert fr.wet(xn, yn).all()
    assert xn[0] == x[0] and yn[0] == y[0]                          # it stayed
    assert xn[1] == x[1] and yn[1] != y[1]                          # (x, yn)
    assert xn[2] != x[2] and yn[2] == y[2]                          # (xn, y)
    assert xn[3] != x[3] and yn[3] != y[3]


class _Closed:
    """A closed lm x mm basin without land, built by hand: packed cells (i, j), i = 1..lm+1, j = 1..mm+1, row by row."""

    def __init__(self, lm, mm, nlay=1):
        L, M = lm + 1, mm + 1
        ndeg = L * M

        class P:
            pass
        self.p = P()
        self.p.lm, self.p.mm, self.p.nlay, self.p.ndeg = lm, mm, nlay, ndeg
        jj, ii = np.meshgrid(np.arange(1, M + 1), np.arange(1, L + 1), indexing="ij")
        ii, jj = ii.ravel(), jj.ravel()
        self.subc = np.zeros((2, ndeg + 1), dtype=np.int32)
        self.subc[0, 1:] = ii; self.subc[1, 1:] = jj
        idx = lambda i, j: np.where((i >= 1) & (i <= L) & (j >= 1) & (j <= M), i + (j - 1) * L, 0)
        self.neig = np.zeros((ndeg + 1, 8), dtype=np.int32)
        for k, (di, dj) in enumerate(((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))):
            self.neig[1:, k] = idx(ii + di, jj + dj)
        self.mk_n = np.zeros(ndeg + 1)
        self.mk_n[1:] = ((ii <= lm) & (jj <= mm)).astype(np.float64)


def test_linear_field_follows_heuns_factor():
    """u = s (x - 16), v = -s (y - 12) on the faces of a closed 32 x 24 frame: the interpolation reproduces a field linear
    along its own axis exactly up to rounding, so Heun's method multiplies x - 16 by 1 + c + c^2/2 and y - 12 by
    1 - c + c^2/2 per step, c = s cdt = 0.02.  Bound: a few roundings of size eps lm per step, 50 steps: ~2e-13 <= 1e-12 lm."""
    lm, mm, n, c = 32, 24, 50, 0.02
    f = _Closed(lm, mm)
    fr = R.Frame(f)
    assert not fr.xper and not fr.yper
    cdt = 0.5
    s = c / cdt
    i, j = fr.i.astype(np.float64), fr.j.astype(np.float64)
    u = (s * ((i - 1.0) - 16.0))[None].copy()
    v = (-s * ((j - 1.0) - 12.0))[None].copy()
    r = np.random.default_rng(5)
    x0, y0 = 16.0 + r.uniform(-3.0, 3.0, 200), 12.0 + r.uniform(-3.0, 3.0, 200)
    layer = np.ones(200, dtype=np.int32)
    x, y = x0.copy(), y0.copy()
    for _ in range(n):
        x, y, branch = R.step(fr, (u, v), (u, v), x, y, layer, cdt)
        assert (branch == 0).all()
    gx, gy = (1.0 + c + 0.5 * c * c) ** n, (1.0 - c + 0.5 * c * c) ** n
    ex, ey = np.abs(x - 16.0 - (x0 - 16.0) * gx), np.abs(y - 12.0 - (y0 - 12.0) * gy)
    print("linear field: max error x %.3g y %.3g (bound %.3g)" % (ex.max(), ey.max(), 1e-12 * lm))
    assert np.abs(x - x0).max() > 1.0                                 # the floats went somewhere
    assert ex.max() <= 1e-12 * lm and ey.max() <= 1e-12 * lm
