"""Frame sets for the forcing-in-time tests, and the oracle stepped one step at a time with the array replaced on the host
before each step (the oracle reads its statics through pointers, so writing Oracle.a[...] in place is enough).  Shared by
tests/test_forcing_cpu.py, which holds these inputs to their conditions, and tests/test_gpu_forcing.py."""
from __future__ import annotations

import copy

import numpy as np

import forcing_ref as FR
import oracle_lib

NSTEPS = 12
TIME_FACTORS = (2.5, 6.0, 9.25)        # frame times in steps: tres + factor*dtd8
PROGNOSTIC = ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy")      # everything that determines the future of a run


def tres_of(f) -> float:
    return float(getattr(f, "tres", 0.0))


def ctim_of(f, tstp: int) -> float:
    return tres_of(f) + float(f.p.dtd8) * float(tstp)          # plan_step's own expression


def frame_times(f, factors=TIME_FACTORS) -> np.ndarray:
    return np.array([tres_of(f) + x * float(f.p.dtd8) for x in factors])


def base_of(f, field: str) -> np.ndarray:
    """The array the frames grow from: the handle's own, or, where that is all zero (a golden without wind or without hdot),
    a smooth pattern over the real cells of a size the run tolerates: 0.05 N/m2 of wind; a thickness source that moves
    1e-5 of the thinnest layer's mean thickness per step (the noise on it raises gravity waves: on stommel_24x16 that adds a
    tenth to the steady run's max |u|, |v|; ten times more doubles them)."""
    a = np.array(getattr(f, field), dtype=np.float64)
    if a.any():
        return a
    n = a.shape[1]
    x = np.arange(n, dtype=np.float64)
    amp = 0.05 if field == "taus" else 1.e-5 * float(np.min(np.mean(np.asarray(f.hlay)[:, 1:], axis=1))) / float(f.p.dt)
    for o in range(a.shape[0]):
        a[o, 1:] = amp * np.sin(0.37 * x[1:] + 1.3 * o)
    return a


def make_frames(f, field: str, seed: int = 5, nfr: int = 3) -> np.ndarray:
    """F_k = base*(1 + 0.5k) + 0.3*max|base|*N(0,1) on the non-zero entries of base; frames[nfr, outer, ndeg+1]."""
    base = base_of(f, field)
    rng = np.random.default_rng(seed)
    live = base != 0.0
    out = np.zeros((nfr,) + base.shape)
    for k in range(nfr):
        out[k] = base * (1.0 + 0.5 * k)
        out[k][live] += 0.3 * float(np.max(np.abs(base))) * rng.standard_normal(int(live.sum()))
    return out


def with_special_entries(frames: np.ndarray) -> np.ndarray:
    """The same frames with exact +0 and -0 entries (in every frame, and -0 in one frame only) and entries equal between
    consecutive frames, among them a -0 pair, spread over every outer slice: what the select of the rule is there for."""
    fr = np.array(frames, dtype=np.float64)
    n = fr.shape[2]
    for o in range(fr.shape[1]):
        idx = np.arange(1 + o % 3, n, 7)
        fr[:, o, idx[0::4]] = 0.0
        fr[:, o, idx[1::4]] = -0.0
        fr[1:, o, idx[2::4]] = fr[:-1, o, idx[2::4]]          # equal between consecutive frames
        fr[1, o, idx[3::4]] = -0.0                            # -0 next to a value
    return fr


def time_table(f, times, period=0.0):
    """Times before the first frame, exactly at each, between frames, after the last; with a period, several periods ahead
    and behind, and in the wrap interval."""
    d = float(f.p.dtd8)
    t = [times[0] - 3.0 * d, times[0] - 0.25 * d] + [float(x) for x in times]
    t += [0.5 * (a + b) for a, b in zip(times[:-1], times[1:])] + [times[0] + 0.37 * (times[1] - times[0])]
    t += [times[-1] + 0.5 * d, times[-1] + 40.0 * d]
    if period > 0.0:
        t += [times[0] + 3.0 * period + 0.3 * d, times[0] - 4.0 * period + 1.7 * d, times[-1] + 0.5 * (times[0] + period - times[-1]),
              times[-1] - 2.0 * period + 0.25 * (times[0] + period - times[-1])]
    return t


def oracle_of(f, variant: int, fields):
    """An oracle with its OWN copies of taus and hdot (Oracle does not copy statics: two built from one Fields share them),
    hdot switched on where the frames bring it."""
    f2 = copy.copy(f)
    f2.taus = np.array(f.taus, dtype=np.float64, order="C", copy=True)
    f2.hdot = np.array(f.hdot, dtype=np.float64, order="C", copy=True)
    f2.has = dict(f.has)
    if "hdot" in fields:
        f2.has["hdot"] = True
    o = oracle_lib.Oracle(f2, variant=variant)
    assert o.a["taus"] is f2.taus and o.a["hdot"] is f2.hdot
    return o


def oracle_run(f, variant: int, sets: dict, nsteps: int = NSTEPS, watch=None):
    """sets: {field: (times, frames, period)}.  The oracle stepped one by one, each field replaced by forcing_ref.field at the
    step's ctim before the step.  watch(tstp, field, array) sees every replaced array.  Returns the oracle."""
    o = oracle_of(f, variant, sets)
    for t in range(1, nsteps + 1):
        for field, (times, frames, period) in sets.items():
            x = FR.field(frames, times, period, ctim_of(f, t))
            o.a[field][...] = x
            if watch is not None:
                watch(t, field, x)
        o.step(t, 1)
    return o


def steady_run(f, variant: int, sets: dict, nsteps: int = NSTEPS):
    """The oracle under the steady first frame of every set."""
    o = oracle_of(f, variant, sets)
    for field, (times, frames, period) in sets.items():
        o.a[field][...] = frames[0]
    o.step(1, nsteps)
    return o
