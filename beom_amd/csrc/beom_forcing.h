// beom_forcing.h — forcing in time: the wind stress taus(0:ndeg, 2) and the thickness source hdot(0:ndeg, nlay) interpolated
// between frames at the top of every time step (no reference routine; DESIGN.md §4 "Forcing in time").
//
// The rule (include/beom_hip.h states it in full; tests/forcing_ref.py is its executable form).  A frame set has nfr >= 1
// frames at strictly increasing times (days, the clock of ctim) and a period (0 = none).  The WEIGHT of a step is formed on
// the host in FP64, forcing_weight below: the two frames k0, k1 and a in [0, 1).  The FIELD is formed per element on the
// device, A and B the values of frames k0 and k1, no contraction:
//     d = B - A;   x = (a == 0 || d == 0) ? A : A + a*d
// The select makes equal frames (and a = 0) return the frame bit for bit, a -0 included; (1-a)*A + a*B does not.
//
// The first part of this file is plain C++ (beom_multi.hip uses it without the kernel); the kernel follows where
// beom_dev.h has been included.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace beom_forcing {

// the frames k0, k1 and the weight a of time ctim; every operation rounded once, written as in include/beom_hip.h
inline void forcing_weight(int nfr, const double *times, double period, double ctim, int *k0, int *k1, double *a) {
    *k0 = 0; *k1 = 0; *a = 0.0;
    if (nfr <= 1) return;
    const int last = nfr - 1;
    double t = ctim;
    if (period > 0.0) {
        double r = std::fmod(ctim - times[0], period);
        if (r < 0.0) r += period;
        t = times[0] + r;
        if (t >= times[last]) {
            *k0 = last; *k1 = 0;
            *a = (t - times[last]) / ((times[0] + period) - times[last]);
            return;
        }
    }
    if (t < times[0]) return;
    if (t >= times[last]) { *k0 = last; *k1 = last; return; }
    int k = 0;
    while (k + 1 < nfr && times[k + 1] <= t) ++k;
    *k0 = k; *k1 = k + 1;
    *a = (t - times[k]) / (times[k + 1] - times[k]);
}

// 0, or -3 with the fault named in msg: what beom_set_forcing refuses before it touches anything.  count = the elements of
// one frame in the caller's storage.
inline int check_set(const char *who, int field, int nfr, const double *times, double period, const double *frames, size_t count,
                     char *msg, size_t len) {
    auto say = [&](const char *fmt, auto... v) { if (msg && len) std::snprintf(msg, len, fmt, who, v...); return -3; };
    if (field != 1 && field != 2) return say("%s: unknown field %d (BEOM_FORCING_TAUS = 1, BEOM_FORCING_HDOT = 2)", field);
    if (nfr < 0) return say("%s: nfr = %d", nfr);
    if (nfr == 0) return 0;
    if (!times || !frames) return say("%s: null times or frames with nfr = %d", nfr);
    for (int k = 0; k < nfr; ++k) {
        if (!std::isfinite(times[k])) return say("%s: times[%d] is not finite", k);
        if (k > 0 && !(times[k] > times[k - 1])) return say("%s: times are not strictly increasing at times[%d]", k);
    }
    if (!std::isfinite(period) || period < 0.0) return say("%s: period %g (0, or longer than the span of the times)", period);
    if (period > 0.0 && !(period > times[nfr - 1] - times[0]))
        return say("%s: period %g is too short for times that span %g", period, times[nfr - 1] - times[0]);
    for (size_t i = 0; i < (size_t)nfr * count; ++i)
        if (!std::isfinite(frames[i])) return say("%s: frame %d holds a value that is not finite (element %lld)", (int)(i / count), (long long)(i % count));
    return 0;
}

}  // namespace beom_forcing

#ifdef BEOM_BLOCK
// ---- the launch.  Purely elementwise: no cell context, no DevView.  Frames and destinations are arrays [outer][n1] in the
// device layout (padded pitch, embedded slots), all allocated alike (element 1 on a 128-byte boundary).  blockIdx.y is the
// outer slice (direction | layer); within a slice element 0 is the sentinel's slot, taken singly, the rest goes as 16-byte
// pairs from the first aligned element on (n1 is odd on the table path, so the parity changes from slice to slice), with a
// single element in front and behind where needed.  PAIRS = false (arrays not aligned alike): one element per thread.
// TWO: taus has a second destination, the cells-only copy the folded momentum sweep reads; it keeps +0 at the sentinel, so
// element 0 is not written there (the frames hold +0 in every other slot that is no cell).
// Compulsory words per element: read 2, write 1 (hdot) | 2 (taus).
struct ForcingView {
    long long n1;                                  // elements of one slice
    const double *A, *B;                           // frames k0, k1
    double *x, *xc;                                // the interpolated field | its cells-only copy (TWO)
};

__device__ __forceinline__ double frc_lerp(double A, double B, double a) {
    const double d = B - A;
    return (a == 0.0 || d == 0.0) ? A : A + a * d;
}
__device__ __forceinline__ double2 frc_lerp(double2 A, double2 B, double a) { return make_double2(frc_lerp(A.x, B.x, a), frc_lerp(A.y, B.y, a)); }

template <bool TWO, class T>
__device__ __forceinline__ void forcing_at(const ForcingView &v, double a, long long e, bool cells = true) {
    const T A = *reinterpret_cast<const T *>(v.A + e), B = *reinterpret_cast<const T *>(v.B + e);
    const T x = frc_lerp(A, B, a);
    *reinterpret_cast<T *>(v.x + e) = x;
    if (TWO && cells) *reinterpret_cast<T *>(v.xc + e) = x;
}

template <bool TWO, bool PAIRS>
__global__ void __launch_bounds__(BEOM_BLOCK) k_forcing_lerp(const ForcingView v, const double a) {
    const long long base = (long long)blockIdx.y * v.n1;
    const long long t0 = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x, step = (long long)gridDim.x * BEOM_BLOCK;
    if (t0 == 0) forcing_at<TWO, double>(v, a, base, false);
    if (!PAIRS) {
        for (long long i = 1 + t0; i < v.n1; i += step) forcing_at<TWO, double>(v, a, base + i);
        return;
    }
    const long long first = 1 + (long long)((reinterpret_cast<uintptr_t>(v.A + base + 1) >> 3) & 1);   // first 16-byte aligned element
    const long long pairs = v.n1 > first ? (v.n1 - first) / 2 : 0;
    for (long long i = t0; i < pairs; i += step) forcing_at<TWO, double2>(v, a, base + first + 2 * i);
    if (t0 == 1 && first == 2 && v.n1 > 1) forcing_at<TWO, double>(v, a, base + 1);
    if (t0 == 2 && first + 2 * pairs < v.n1) forcing_at<TWO, double>(v, a, base + v.n1 - 1);
}
#endif
