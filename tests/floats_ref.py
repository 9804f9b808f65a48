"""Numpy restatement of the float scheme (include/beom_hip.h "Lagrangian floats", beom_amd/csrc/beom_floats.h): helper module of
test_floats_cpu and test_gpu_floats, not a conftest; imports nothing from the code under test.

Arrays as the engine's callers hold them: u, v [nlay, ndeg+1] with index 0 the land sentinel; x, y float64 [n] in grid units;
layer int [n], 1-based.  Every statement is the header's, in its order; numpy never contracts a multiply-add."""
import zlib

import numpy as np


class Frame:
    """What the scheme needs of a Fields object: the (i, j) -> packed cell map, E and N links, the wet mask, the wraps."""

    def __init__(self, f):
        p = f.p
        self.lm, self.mm, self.nlay, self.n1 = int(p.lm), int(p.mm), int(p.nlay), int(p.ndeg) + 1
        neig = np.asarray(f.neig).astype(np.int64)
        i, j = np.asarray(f.subc[0]).astype(np.int64), np.asarray(f.subc[1]).astype(np.int64)
        self.i, self.j = i, j
        self.E, self.N = neig[:, 0], neig[:, 2]
        self.cmap = np.zeros((self.lm + 2, self.mm + 2), dtype=np.int64)        # [i, j], 0 = no packed cell
        self.cmap[i[1:], j[1:]] = np.arange(1, self.n1)
        self.wetc = np.asarray(f.mk_n) > 0.5
        self.wetc[0] = False
        self.xper = bool(np.any(neig[1:, 4][i[1:] == 1] != 0))                  # a cell of column 1 with a W neighbour
        self.yper = bool(np.any(neig[1:, 6][j[1:] == 1] != 0))

    def cell(self, x, y):
        fx, fy = np.floor(x), np.floor(y)
        with np.errstate(invalid="ignore"):
            ok = (fx >= 0.0) & (fx < self.lm + 1.0) & (fy >= 0.0) & (fy < self.mm + 1.0)
        i = np.where(ok, fx, 0.0).astype(np.int64) + 1
        j = np.where(ok, fy, 0.0).astype(np.int64) + 1
        return np.where(ok, self.cmap[i, j], 0)

    def wet(self, x, y):
        return self.wetc[self.cell(x, y)]

    def velocity(self, u, v, x, y, layer):
        fx, fy = np.floor(x), np.floor(y)
        a, b = x - fx, y - fy
        p = self.cell(x, y)
        l = np.asarray(layer).astype(np.int64) - 1
        U = (1.0 - a) * u[l, p] + a * u[l, self.E[p]]
        V = (1.0 - b) * v[l, p] + b * v[l, self.N[p]]
        return U, V

    def wrapx(self, z):
        return _wrap(z, float(self.lm), self.xper)

    def wrapy(self, z):
        return _wrap(z, float(self.mm), self.yper)


def _wrap(z, n, per):
    if per:
        z = np.where(z < 0.0, z + n, z)
        z = np.where(z >= n, z - n, z)
    return z


def stage1(fr, u, v, x, y, layer, cdt):
    """-> k1x, k1y, xs, ys"""
    U, V = fr.velocity(u, v, x, y, layer)
    k1x, k1y = U * cdt, V * cdt
    xs, ys = fr.wrapx(x + k1x), fr.wrapy(y + k1y)
    dry = ~fr.wet(xs, ys)
    return k1x, k1y, np.where(dry, x, xs), np.where(dry, y, ys)


def stage2(fr, u, v, x, y, layer, cdt, k1x, k1y, xs, ys):
    """-> x, y, branch: which candidate of the landing rule each float took (0 = the first ... 3 = it stayed)"""
    U, V = fr.velocity(u, v, xs, ys, layer)
    k2x, k2y = U * cdt, V * cdt
    xn, yn = fr.wrapx(x + 0.5 * (k1x + k2x)), fr.wrapy(y + 0.5 * (k1y + k2y))
    w0, w1, w2 = fr.wet(xn, yn), fr.wet(xn, y), fr.wet(x, yn)
    branch = np.where(w0, 0, np.where(w1, 1, np.where(w2, 2, 3)))
    xo = np.where(branch <= 1, xn, x)
    yo = np.where((branch == 0) | (branch == 2), yn, y)
    return xo, yo, branch


def step(fr, before, after, x, y, layer, cdt):
    """One step of Heun's method: before = (u, v) as the step begins, after = (u, v) as it leaves them."""
    k1x, k1y, xs, ys = stage1(fr, before[0], before[1], x, y, layer, cdt)
    return stage2(fr, after[0], after[1], x, y, layer, cdt, k1x, k1y, xs, ys)


# ---- inputs of the tests (in the spirit of rough_inputs: nothing constant, smooth or zero) ---------------------------------------
def _rng(seed, name):
    return np.random.default_rng([int(seed), zlib.crc32(name.encode())])


def rough_velocities(f, seed, stage, amp=1.0):
    """u, v uniform in +-amp at open faces (times mk_u / mk_v), drawn anew for every (seed, stage)."""
    nlay, n1 = int(f.p.nlay), int(f.p.ndeg) + 1
    r = _rng(seed, "uv%d" % stage)
    u = r.uniform(-1.0, 1.0, (nlay, n1)) * amp * np.asarray(f.mk_u, dtype=np.float64)[None]
    v = r.uniform(-1.0, 1.0, (nlay, n1)) * amp * np.asarray(f.mk_v, dtype=np.float64)[None]
    return np.ascontiguousarray(u), np.ascontiguousarray(v)


def seed_floats(f, n, seed):
    """n floats at random places inside wet cells, random layers."""
    fr = Frame(f)
    r = _rng(seed, "floats")
    cells = np.flatnonzero(fr.wetc)
    c = cells[r.integers(0, cells.size, n)]
    x = (fr.i[c] - 1).astype(np.float64) + r.uniform(0.0, 1.0, n)
    y = (fr.j[c] - 1).astype(np.float64) + r.uniform(0.0, 1.0, n)
    x, y = np.minimum(x, np.nextafter(fr.i[c].astype(np.float64), 0.0)), np.minimum(y, np.nextafter(fr.j[c].astype(np.float64), 0.0))
    layer = r.integers(1, int(f.p.nlay) + 1, n).astype(np.int32)
    assert fr.wet(x, y).all()
    return x, y, layer


def corner_floats(f):
    """Hand-placed floats, one for each branch of the landing rule, with the velocity field that takes them there.  The last
    branch (the float stays) is out of reach of velocities that carry the masks: the wall-normal component falls linearly to
    the stored zero at a coast face, so a float crosses a wall only with a stage 2 evaluated in ANOTHER cell, which stage 1
    reaches through a wet face; from there the float is too far from a second wall of its own cell to cross that too (the
    random floats of test_floats_cpu take the first three branches and never the last).  The restatement and the kernel
    take any u, v, so this field is a plain constant, NOT masked: (u, v) = (1, 1) before and after the step.
      float 0: a wet cell whose E, N and NE cells are all dry  -> (xn, yn), (xn, y), (x, yn) dry: it stays      (branch 3)
      float 1: a wet cell whose E and NE cells are dry, N wet  -> (xn, yn), (xn, y) dry, (x, yn) wet            (branch 2)
      float 2: a wet cell whose N and NE cells are dry, E wet  -> (xn, yn) dry, (xn, y) wet                     (branch 1)
      float 3: a wet cell with wet E, N and NE                 -> the first candidate                           (branch 0)
    Returns x, y, layer, (u, v), cdt and the expected branches; cdt = 0.9, floats at (0.8, 0.8) of their cell."""
    fr = Frame(f)
    w = fr.wetc
    E, N = fr.E, fr.N
    NE = np.asarray(f.neig).astype(np.int64)[:, 1]
    cells = np.arange(fr.n1)
    inside = w & (fr.i < fr.lm) & (fr.j < fr.mm) & (cells > 0)
    # "dry" includes cells that do not exist (link 0): wetc[0] is False
    want = ((~w[E] & ~w[N] & ~w[NE]), (~w[E] & w[N] & ~w[NE]), (w[E] & ~w[N] & ~w[NE]), (w[E] & w[N] & w[NE]))
    picks = []
    for k, m in enumerate(want):
        c = np.flatnonzero(inside & m)
        assert c.size, "no wet cell of kind %d on this frame" % k
        picks.append(int(c[0]))
    c = np.array(picks)
    x, y = (fr.i[c] - 1) + 0.8, (fr.j[c] - 1) + 0.8
    layer = np.ones(4, dtype=np.int32)
    u = np.ones((fr.nlay, fr.n1)); v = np.ones((fr.nlay, fr.n1))
    return x.astype(np.float64), y.astype(np.float64), layer, (u, v), 0.9, np.array([3, 2, 1, 0])
