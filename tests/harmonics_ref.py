"""numpy restatement of the harmonics (include/beom_hip.h, "Harmonics"): the statements of the contract taken literally, one
x - ref, S0 + d, d*cw, C + p, d*sw, S + p per sample and frequency, as whole-array FP64 operations, and the normal matrix
G + w_i*w_j.  The weights are the engine's own, capi.harmonic_weights (the contract hands exactly them to the restatement;
test_harmonics_cpu holds them to math.cos / math.sin); nothing else comes from the code under test.  Helper module of
test_harmonics_cpu and test_gpu_harmonics."""
import numpy as np

from beom_amd import capi

FIELDS = ("hlay", "u", "v", "h_u", "h_v")
M2 = 2.0 * np.pi / (12.4206012 / 24.0)            # rad/day


class Harmonics:
    """level 1: hlay, u, v; 2: and h_u, h_v.  sample(fields, ctim) takes the arrays (a dict by name or a sequence in the
    order of FIELDS), all of one shape."""

    def __init__(self, omega, level=1):
        self.omega = [float(w) for w in np.atleast_1d(omega)]
        assert 1 <= len(self.omega) <= 4 and level in (1, 2)
        self.level, self.K, self.nw = level, len(self.omega), 1 + 2 * len(self.omega)
        self.nf = 5 if level >= 2 else 3
        self.reset()

    def reset(self):
        """count = 0 and G = 0: the next sample is a first sample."""
        self.count = 0
        self.gram = np.zeros((self.nw, self.nw))

    def weights(self, ctim):
        w = [1.0]
        for om in self.omega:
            w.extend(capi.harmonic_weights(om, ctim))
        return np.array(w)

    def sample(self, fields, ctim):
        x = [np.array(fields[k] if isinstance(fields, dict) else fields[i], dtype=np.float64) for i, k in enumerate(FIELDS[:self.nf])]
        w = self.weights(ctim)
        for i in range(self.nw):
            for j in range(self.nw):
                self.gram[i, j] = self.gram[i, j] + w[i] * w[j]
        if self.count == 0:
            self.ref = np.stack(x)
            self.sum = np.zeros((self.nf, self.nw) + x[0].shape)      # +0.0
            self.count = 1
            return
        for f in range(self.nf):
            d = x[f] - self.ref[f]
            self.sum[f, 0] = self.sum[f, 0] + d
            for k in range(self.K):
                p = d * w[1 + 2 * k]                                  # rounded, then added
                self.sum[f, 1 + 2 * k] = self.sum[f, 1 + 2 * k] + p
                p = d * w[2 + 2 * k]
                self.sum[f, 2 + 2 * k] = self.sum[f, 2 + 2 * k] + p
        self.count += 1

    def solve(self):
        """a [1+2K, F, *shape]: G a = (S0, C_1, S_1, ...) per element."""
        b = np.moveaxis(self.sum, 1, 0)
        return np.linalg.solve(self.gram, b.reshape(self.nw, -1)).reshape(b.shape)

    def fit(self):
        """mean [F, *shape], amp and phase [F, K, *shape]."""
        a = self.solve()
        amp = np.stack([np.hypot(a[1 + 2 * k], a[2 + 2 * k]) for k in range(self.K)], axis=1)
        phase = np.stack([np.arctan2(a[2 + 2 * k], a[1 + 2 * k]) for k in range(self.K)], axis=1)
        return self.ref + a[0], amp, phase


def phase_diff(a, b):
    """a - b wrapped into (-pi, pi]."""
    return np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b))))


def bound(nsamples, dmax, amp):
    """The fit's error bound of the contract, relative to amp (and in radians for the phase): two roundings per sample and
    sum, divided by the ~N/2 diagonal of G, times its condition number ~2: 8*N*2^-53*max|d|/amp."""
    return 8.0 * nsamples * 2.0 ** -53 * dmax / amp
