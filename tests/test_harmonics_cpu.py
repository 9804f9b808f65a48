"""The harmonics' contract on the CPU (include/beom_hip.h, "Harmonics"): the host-only weights against math.cos / math.sin;
the numpy restatement (harmonics_ref) recovering amplitudes, phases and means of tidal signals on a deep layer within the
rounding bound of the contract, on a long record and on one of 1.3 periods; identities; the interface elevations by
linearity (capi.derive_harmonics).  No GPU.

The bound (harmonics_ref.bound): a sum takes two roundings per sample (the product, the addition), each at most 2^-53 of a
partial sum that stays below N*max|d|; the error of a sum, at most 2*N*2^-53*N*max|d|, is divided by the ~N/2 diagonal of
the normal matrix and multiplied by its condition number ~2: 8*N*2^-53*max|d| absolute, /amp_k relative, and as much in
radians for the phase."""
import math

import numpy as np

import harmonics_ref as HR
from beom_amd import capi

NCELL = 16
EPS = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_weights_are_libm_of_the_fp64_product():
    rng = np.random.default_rng(7)
    omega = rng.uniform(0.1, 60.0, 10000)
    ctim = np.concatenate([rng.uniform(0.0, 40.0, 5000), rng.uniform(0.0, 40000.0, 5000)])
    for om, t in zip(omega.tolist(), ctim.tolist()):
        th = om * t
        cw, sw = capi.harmonic_weights(om, t)
        assert (cw, sw) == (math.cos(th), math.sin(th)), (om, t)
    assert capi.harmonic_weights(12.0, 0.0) == (1.0, 0.0)


# ---- recovery -----------------------------------------------------------------------------------------------------------------
def _signal(amps, nsamples, dt, base=4000.0, seed=1, omega=HR.M2):
    """x_n [nsamples, NCELL] = base + u + sum_k amps[k] cos((k+1) omega t_n - phi_k), t_n = n*dt; u and phi_k per cell."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1.0, 1.0, NCELL)
    phi = np.stack([rng.uniform(-np.pi, np.pi, NCELL) for _ in amps])
    t = np.arange(nsamples) * dt
    x = np.full((nsamples, NCELL), base) + u[None]
    for k, a in enumerate(amps):
        x = x + a * np.cos((k + 1) * omega * t[:, None] - phi[k][None])
    return t, x, base + u, phi


def _fed(omega, t, x, level=1):
    h = HR.Harmonics(omega, level)
    for tn, xn in zip(t, x):
        h.sample([xn] * h.nf, tn)
    return h


def _check_fit(h, x, amps, phi, mu, what):
    mean, amp, phase = h.fit()
    dmax = np.max(np.abs(x - x[0][None]), axis=0)
    for k, a in enumerate(amps):
        b = HR.bound(len(x), dmax, a)
        ea, ep = np.abs(amp[0, k] - a) / a, np.abs(HR.phase_diff(phase[0, k], phi[k]))
        print(what, "k", k, "amp err", ea.max(), "phase err", ep.max(), "bound", b.min())
        assert np.all(ea <= b), (what, k, ea.max(), b.min())
        assert np.all(ep <= b), (what, k, ep.max(), b.min())
    # the mean: a_0 against mu - ref (exact in FP64: both lie within a factor of two), the key `mean` one rounding further
    babs = 8.0 * len(x) * EPS * dmax
    e0 = np.abs(h.solve()[0][0] - (mu - h.ref[0]))
    print(what, "a_0 err", e0.max(), "bound", babs.min())
    assert np.all(e0 <= babs), (what, e0.max(), babs.min())
    assert np.all(np.abs(mean[0] - mu) <= babs + 0.5 * np.spacing(np.abs(mu))), what
    for f in range(1, h.nf):
        assert np.array_equal(_bits(amp[f]), _bits(amp[0])) and np.array_equal(_bits(mean[f]), _bits(mean[0]))


def test_recovery_of_m2_and_m4_on_a_deep_layer():
    """0.01 m of M2 and 0.005 m of M4 on 4000 m, 3000 samples 0.0104 days apart, K = 2, against the true amplitudes, phases
    and mean.  Measured here: amplitudes 7.3e-13 and 2.2e-12 relative, phases 1.3e-12 and 1.7e-12 rad, against bounds from
    3.8e-12 and 7.6e-12; the header's 2.2e-12 is the larger amplitude figure."""
    amps = (0.01, 0.005)
    t, x, mu, phi = _signal(amps, 3000, 0.0104)
    h = _fed((HR.M2, 2.0 * HR.M2), t, x)
    assert h.count == 3000
    _check_fit(h, x, amps, phi, mu, "M2+M4")


def test_why_the_sums_are_shifted():
    """The same record through sums of x itself (ref = 0): the deep layer's 4000 m take the digits that the shift keeps."""
    amps = (0.01, 0.005)
    t, x, _, _ = _signal(amps, 3000, 0.0104)
    om = (HR.M2, 2.0 * HR.M2)
    h = _fed(om, t, x)
    plain = HR.Harmonics(om, 1)
    plain.sample([np.zeros(NCELL)] * 3, t[0])        # a first sample that sets ref = 0 ...
    plain.gram[:] = 0.0                               # ... and is not part of the record
    plain.count = 1
    for tn, xn in zip(t, x):
        plain.sample([xn] * 3, tn)
    assert not plain.ref.any() and np.array_equal(plain.gram, h.gram)
    err = {}
    for what, a in (("shifted", h.fit()[1]), ("plain", plain.fit()[1])):
        err[what] = max(float(np.max(np.abs(a[0, k] - amps[k]) / amps[k])) for k in range(2))
    print("amplitude error, shifted", err["shifted"], "plain", err["plain"])
    assert err["shifted"] < 4e-12 and err["plain"] > 3.0 * err["shifted"]


def _longdouble_fit(h, t, x):
    """Least squares of the very samples x [N, cells] in long double, with the restatement's weights: a [1+2K, cells] by
    elimination."""
    L = np.longdouble
    W = np.stack([h.weights(tn) for tn in t]).astype(L)               # [N, nw]
    d = x.astype(L) - x[0].astype(L)[None]                            # exact
    G, b = W.T @ W, W.T @ d
    n = G.shape[0]
    for i in range(n):
        for j in range(i + 1, n):
            m = G[j, i] / G[i, i]
            G[j] = G[j] - m * G[i]
            b[j] = b[j] - m * b[i]
    a = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        a[i] = (b[i] - G[i, i + 1:] @ a[i + 1:]) / G[i, i]
    return a


def test_short_record_needs_no_whole_number_of_periods():
    """One tone, K = 1, 67 samples over 1.3 periods.  Two references, one bound (the contract's):
    - samples that carry no rounding of their own (the tone around a mean below 1) against the TRUE amplitude, phase and mean;
    - the tone on 4000 m against the least-squares fit of the very samples in long double.  There each sample is rounded to
      half an ulp of 4000, 2.3e-13, which 67 samples average down to some 3e-14 in the fit (measured against the truth:
      2.7e-12 relative in amplitude); the contract's bound is on the accumulation's roundings (1.2e-13 relative here), not
      on what the samples lost before they were taken, so the truth of that case is the exact fit of what was sampled."""
    period = 2.0 * np.pi / HR.M2
    dt = 1.3 * period / 67
    t, x, mu, phi = _signal((0.01,), 67, dt, base=0.0)
    _check_fit(_fed(HR.M2, t, x), x, (0.01,), phi, mu, "67 samples around 0")
    t, x, mu, phi = _signal((0.01,), 67, dt)
    h = _fed(HR.M2, t, x)
    a, want = h.solve()[:, 0], _longdouble_fit(h, t, x)
    dmax = np.max(np.abs(x - x[0][None]), axis=0)
    amp, amp_w = np.hypot(a[1], a[2]), np.hypot(want[1], want[2])
    b = HR.bound(67, dmax, 0.01)
    ea = np.abs((amp - amp_w) / amp_w).astype(np.float64)
    ep = np.abs(HR.phase_diff(np.arctan2(a[2], a[1]), np.arctan2(want[2], want[1]).astype(np.float64)))
    e0 = np.abs(a[0] - want[0]).astype(np.float64)
    print("67 samples on 4000 m: amp", ea.max(), "phase", ep.max(), "a_0", e0.max(), "bound", b.min())
    assert np.all(ea <= b) and np.all(ep <= b) and np.all(e0 <= b * 0.01)
    # and the long-double fit itself finds the tone as well as the samples allow: 67 roundings of 2^-53 * 4096 at most
    assert np.all(np.abs(amp_w - 0.01) <= 67 * EPS * 4096.0)


# ---- identities ---------------------------------------------------------------------------------------------------------------
def test_identities():
    rng = np.random.default_rng(3)
    const = [rng.uniform(1.0, 4000.0, (3, NCELL)) for _ in range(5)]
    const[1][0, :4] = -0.0
    h = HR.Harmonics((HR.M2, 1.9 * HR.M2, 3.0), 2)
    for n in range(9):
        h.sample(const, 0.37 * n)
    assert h.count == 9 and h.sum.shape == (5, 7, 3, NCELL)
    assert not h.sum.any() and not np.signbit(h.sum).any(), "a constant field: every sum is +0.0"
    mean, amp, _ = h.fit()
    assert np.array_equal(_bits(mean), _bits(h.ref)) or np.array_equal(mean, h.ref)
    assert np.array_equal(mean, np.stack(const)) and not amp.any()
    assert np.array_equal(h.gram, h.gram.T) and h.gram[0, 0] == 9.0
    assert abs(np.trace(h.gram) - (9.0 + 3 * 9.0)) < 1e-12          # cw^2 + sw^2 = 1 per frequency and sample
    # reset starts over: the same samples after a reset give the same bits as a fresh analysis
    t, x, _, _ = _signal((0.01,), 20, 0.03)
    a = _fed((HR.M2, 3.0), t, x)
    b = HR.Harmonics((HR.M2, 3.0), 1)
    for n in range(5):
        b.sample([x[n] + 1.0] * 3, 7.0 + n)
    b.reset()
    assert b.count == 0 and not b.gram.any()
    for tn, xn in zip(t, x):
        b.sample([xn] * 3, tn)
    assert b.count == a.count == 20
    for k in ("ref", "sum", "gram"):
        assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k
    assert a.gram[0, 0] == 20.0


# ---- the interface elevations by linearity -----------------------------------------------------------------------------------
def test_eta_by_linearity():
    """Three layers (500, 1500, 2000 m), each with its own M2 and M4 amplitude and phase: the harmonics of the interface
    elevations as capi.derive_harmonics forms them from the layers' coefficients, and those of the cumulative layer sum
    analysed as a field of its own, each against the true amplitude and phase of that interface (the layers' phasors
    summed), within the bound formed with the interface's own max|d| and amplitude."""
    rng = np.random.default_rng(11)
    nlay, N, dt = 3, 3000, 0.0104
    base = np.array([500.0, 1500.0, 2000.0])[:, None] + rng.uniform(-1.0, 1.0, (nlay, NCELL))
    amps = np.stack([rng.uniform(0.002, 0.01, (nlay, NCELL)), rng.uniform(0.001, 0.005, (nlay, NCELL))])    # [K, nlay, NCELL]
    phi = np.stack([0.8 + rng.uniform(-0.6, 0.6, (nlay, NCELL)), -2.0 + rng.uniform(-0.6, 0.6, (nlay, NCELL))])
    om = (HR.M2, 2.0 * HR.M2)
    t = np.arange(N) * dt
    layers, sums = HR.Harmonics(om, 1), HR.Harmonics(om, 1)
    dmax, e0 = np.zeros((nlay, NCELL)), None
    for tn in t:
        x = base + sum(amps[k] * np.cos(om[k] * tn - phi[k]) for k in range(2))
        eta = np.cumsum(x[::-1], axis=0)[::-1]                      # interface ilay: the layers from ilay down to the bottom
        e0 = eta if e0 is None else e0
        dmax = np.maximum(dmax, np.abs(eta - e0))
        layers.sample([x] * 3, tn)
        sums.sample([eta] * 3, tn)
    got = capi.derive_harmonics({"count": layers.count, "ref": layers.ref, "sum": layers.sum, "gram": layers.gram})
    assert got["eta_amp"].shape == (2, nlay, NCELL) and got["amp"].shape == (3, 2, nlay, NCELL)
    _, amp_l, phase_l = layers.fit()
    assert np.array_equal(got["amp"], amp_l) and np.array_equal(got["phase"], phase_l)
    _, amp_s, phase_s = sums.fit()
    z = np.cumsum((amps * np.exp(1j * phi))[:, ::-1], axis=1)[:, ::-1]      # the true phasors of the interfaces
    for k in range(2):
        b = HR.bound(N, dmax, np.abs(z[k]))
        for what, a, p in (("derived", got["eta_amp"][k], got["eta_phase"][k]), ("of the sum", amp_s[0, k], phase_s[0, k])):
            ea, ep = np.abs(a - np.abs(z[k])) / np.abs(z[k]), np.abs(HR.phase_diff(p, np.angle(z[k])))
            print("eta", what, "k", k, "amp err", ea.max(), "phase err", ep.max(), "bound", b.min())
            assert np.all(ea <= b) and np.all(ep <= b), (what, k, ea.max(), ep.max(), b.min())
    # too few samples, or a singular normal matrix: the derived keys are absent
    few = _fed(HR.M2, t[:2], np.full((2, NCELL), 3.0))
    out = capi.derive_harmonics({"count": 2, "ref": few.ref, "sum": few.sum, "gram": few.gram})
    assert "amp" not in out and "mean" not in out and "eta_amp" not in out
