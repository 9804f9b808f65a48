"""numpy restatement of the tracer moments (include/beom_hip.h, "Tracer moments"): the four sampled quantities from the tracer
restatement's own concentration and upstream face (tracers_ref.concentration, tracers_ref._face), fed to the shifted sums of
the contract taken literally, one x - ref, S + d, d*d, Q + p per sample, as whole-array FP64 operations.  Helper module of
test_tracer_moments_cpu and test_gpu_tracer_moments; imports nothing from the code under test (f is the init mirror's Fields).

Shapes: hlay, h_u, h_v [nlay, ndeg+1]; q [ntrc, nlay, ndeg+1]; ref, sum [2 or 4, ntrc, nlay, ndeg+1]; sq [ntrc, nlay, ndeg+1].
Index 0 (the sentinel) is no real cell: it feeds its neighbours' faces and is itself kept at +0.0, as a download returns it."""
import numpy as np

import tracers_ref as T

QUANTITIES = ("q", "c", "fu", "fv")


def quantities(f, hlay, h_u, h_v, q):
    """x[4, ntrc, nlay, ndeg+1]: x_q = q, x_c = c(p), x_fu = h_u * cf between W and p, x_fv = h_v * cf between S and p; +0.0
    at index 0."""
    q = np.asarray(q, dtype=np.float64)
    W, S = f.neig[:, 4].astype(np.int64), f.neig[:, 6].astype(np.int64)
    here = np.arange(f.p.ndeg + 1)
    x = np.zeros((4,) + q.shape)
    for t in range(q.shape[0]):
        for l in range(f.p.nlay):
            c, wet = T.concentration(np.asarray(hlay[l], dtype=np.float64), q[t, l])
            x[0, t, l] = q[t, l]
            x[1, t, l] = c
            x[2, t, l] = T._face(np.asarray(h_u[l], dtype=np.float64), c, wet, W, here)
            x[3, t, l] = T._face(np.asarray(h_v[l], dtype=np.float64), c, wet, S, here)
    x[..., 0] = 0.0
    return x


class TracerMoments:
    """level 1: ref, S of q and c; 2: and of fu, fv; 3: and Q of (c, c).  sample(hlay, h_u, h_v, q) takes the arrays as they
    stand at the end of a step; sample_x(x) takes the four quantities themselves."""

    def __init__(self, f, level=3):
        assert level in (1, 2, 3), level
        self.f = f
        self.level = level
        self.nq = 4 if level >= 2 else 2
        self.reset()

    def reset(self):
        """count = 0: the next sample is a first sample (the arrays are left as they are until then)."""
        self.count = 0

    def sample(self, hlay, h_u, h_v, q):
        self.sample_x(quantities(self.f, hlay, h_u, h_v, q))

    def sample_x(self, x):
        x = np.array(x[:self.nq], dtype=np.float64)
        if self.count == 0:
            self.ref = x
            self.sum = np.zeros_like(x)                              # +0.0
            self.sq = np.zeros(x.shape[1:]) if self.level >= 3 else None
            self.count = 1
            return
        d = x - self.ref
        self.sum = self.sum + d
        if self.level >= 3:
            p = d[1] * d[1]                                          # rounded, then added
            self.sq = self.sq + p
        self.count += 1

    @property
    def mean(self):
        return self.ref + self.sum / float(self.count)

    @property
    def var_c(self):
        assert self.level >= 3
        n = float(self.count)
        return self.sq / n - (self.sum[1] / n) * (self.sum[1] / n)
