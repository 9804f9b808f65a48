"""numpy restatement of the moments (include/beom_hip.h, "Moments"): the statements of the contract taken literally, one
x - ref, S + d, d*d, Q + p per sample, as whole-array FP64 operations.  Helper module of test_moments_cpu and
test_gpu_moments; imports nothing from the code under test."""
import numpy as np

FIELDS = ("hlay", "u", "v", "h_u", "h_v")
PAIRS = ((0, 0), (1, 1), (2, 2), (1, 3), (2, 4))        # (h,h) (u,u) (v,v) (u,h_u) (v,h_v)


class Moments:
    """level 1: ref, S of hlay, u, v; 2: and of h_u, h_v; 3: and the five Q.  sample(fields) takes the five arrays (a dict by
    name or a sequence in the order of FIELDS), all of one shape."""

    def __init__(self, level=3):
        assert level in (1, 2, 3), level
        self.level = level
        self.nf = 5 if level >= 2 else 3
        self.reset()

    def reset(self):
        """count = 0: the next sample is a first sample (the arrays are left as they are until then)."""
        self.count = 0

    def sample(self, fields):
        x = [np.array(fields[k] if isinstance(fields, dict) else fields[i], dtype=np.float64) for i, k in enumerate(FIELDS)]
        if self.count == 0:
            self.ref = np.stack(x[:self.nf])
            self.sum = np.zeros_like(self.ref)                       # +0.0
            self.sq = np.zeros((5,) + x[0].shape) if self.level >= 3 else None
            self.count = 1
            return
        d = [x[f] - self.ref[f] for f in range(self.nf)]
        for f in range(self.nf):
            self.sum[f] = self.sum[f] + d[f]
        if self.level >= 3:
            for m, (a, b) in enumerate(PAIRS):
                p = d[a] * d[b]                                      # rounded, then added
                self.sq[m] = self.sq[m] + p
        self.count += 1

    @property
    def mean(self):
        return self.ref + self.sum / float(self.count)

    @property
    def var(self):
        """var[0..2]: the variances of hlay, u, v; var[3..4]: the covariances of (u, h_u), (v, h_v)."""
        assert self.level >= 3
        n = float(self.count)
        return np.stack([self.sq[m] / n - (self.sum[a] / n) * (self.sum[b] / n) for m, (a, b) in enumerate(PAIRS)])
