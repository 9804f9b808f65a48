"""The rule of forcing in time (include/beom_hip.h, "Forcing in time") in numpy / Python floats: the executable form the
engine's host function and launch are compared with, bit for bit.  Python floats and numpy float64 round every operation
once and never contract."""
from __future__ import annotations

import math

import numpy as np


def weight(times, period, ctim):
    """(k0, k1, a): the two frames and the weight of time ctim."""
    t_ = [float(x) for x in np.atleast_1d(times)]
    nfr = len(t_)
    period, ctim = float(period), float(ctim)
    if nfr == 1:
        return 0, 0, 0.0
    last = nfr - 1
    t = ctim
    if period > 0.0:
        r = math.fmod(ctim - t_[0], period)
        if r < 0.0:
            r += period
        t = t_[0] + r
        if t >= t_[last]:
            return last, 0, (t - t_[last]) / ((t_[0] + period) - t_[last])
    if t < t_[0]:
        return 0, 0, 0.0
    if t >= t_[last]:
        return last, last, 0.0
    k0 = max(k for k in range(nfr) if t_[k] <= t)
    return k0, k0 + 1, (t - t_[k0]) / (t_[k0 + 1] - t_[k0])


def lerp(A, B, a):
    """Per element: d = B - A; x = (a == 0 || d == 0) ? A : A + a*d."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    d = B - A
    if a == 0.0:
        return A.copy()
    return np.where(d == 0.0, A, A + np.float64(a) * d)


def field(frames, times, period, ctim):
    """The field at time ctim of the frame set frames[nfr, ...]."""
    k0, k1, a = weight(times, period, ctim)
    return lerp(frames[k0], frames[k1], a)


def convex(A, B, a):
    """The plain form (1-a)*A + a*B, which does NOT return equal frames bit for bit (tests/test_forcing_cpu.py)."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    return (1.0 - np.float64(a)) * A + np.float64(a) * B
