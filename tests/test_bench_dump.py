"""bench.py --dump-outputs without a GPU: the cells it writes (fixed, within the byte budget) and the assembly of the
bands of an N-rank run into one array per field (a stand-in engine serves windows cut from known global arrays)."""
import os
import types

import numpy as np
import pytest

import bench
from beom_amd import slab

LEVELS = {"rs_h": (2,), "dmdx": (3,), "dmdy": (3,)}          # time levels the state keeps (grid.Fields)


def _params(lm, mm, nlay):
    return types.SimpleNamespace(lm=lm, mm=mm, nlay=nlay, ndeg=(lm + 1) * (mm + 1))


def test_dump_cells_fixed_and_within_budget():
    p = _params(4096, 4096, 4)
    levels = sum(int(np.prod(LEVELS.get(k, ()))) for k in bench.DUMP_FIELDS)
    c = bench.dump_cells(p, levels)
    assert np.array_equal(c, bench.dump_cells(p, levels))
    assert c.size * 8 * p.nlay * levels <= bench.DUMP_BYTES <= 64e6 - 4096
    assert c[0] >= 1 and c[-1] <= p.ndeg and np.all(np.diff(c) > 0)
    small = _params(63, 40, 3)
    assert np.array_equal(bench.dump_cells(small, levels), np.arange(1, small.ndeg + 1))


@pytest.mark.parametrize("world,yper,budget", [(3, False, None), (3, True, None), (1, True, None),
                                               (2, False, 8 * 3 * 13 * 1000), (4, True, 8 * 3 * 13 * 1000)])
def test_dump_outputs_assembles_bands(tmp_path, monkeypatch, world, yper, budget):
    if budget:
        monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    lm, mm, nlay = 63, 80, 3
    p, L = _params(lm, mm, nlay), lm + 1
    rng = np.random.default_rng(1)
    full = {k: rng.standard_normal((nlay, p.ndeg + 1) + LEVELS.get(k, ())) for k in bench.DUMP_FIELDS}
    shapes = types.SimpleNamespace(**{k: np.zeros((nlay, 2) + LEVELS.get(k, ())) for k in bench.DUMP_FIELDS})

    class Band:                      # BandEngine.download: window rows (south ghosts, owned, north ghosts); orphan row mm+1
        def __init__(self, g):
            self.g, self.f = g, shapes

        def download(self, names, orphan=False):
            rows = self.g.global_rows()
            out = {k: np.full((nlay, 1 + len(rows) * L) + full[k].shape[2:], np.nan) for k in names}
            for r, gr in enumerate(rows):
                for k in names:
                    out[k][:, 1 + r * L:1 + (r + 1) * L] = full[k][:, 1 + (gr - 1) * L:1 + gr * L]
            oo = None
            if yper and self.g.rank == 0:
                oo = {k: np.concatenate([np.full((nlay, 1) + full[k].shape[2:], np.nan), full[k][:, 1 + mm * L:]], axis=1)
                      for k in names}
            return out, oo

    sent = {}

    class Dist:                      # gather_object of the ranks, called in turn, rank 0 last
        def __init__(self, rank):
            self.rank = rank

        def gather_object(self, obj, lst, dst=0):
            sent[self.rank] = obj
            if lst is not None:
                lst[:] = [sent[r] for r in range(world)]

    geoms = slab.decompose(mm, lm, world, yper=yper)
    for rank in list(range(1, world)) + [0]:
        bench.dump_outputs(str(tmp_path), Band(geoms[rank]), p, geoms[rank], world, rank, Dist(rank))
    cells = bench.dump_cells(p, 13)
    assert (cells.size < p.ndeg) == bool(budget)
    for k in bench.DUMP_FIELDS:
        got = np.load(os.path.join(str(tmp_path), k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, full[k][:, cells]), k
