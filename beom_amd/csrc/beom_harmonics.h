// beom_harmonics.h — least-squares harmonic analysis of the layer fields (no reference routine; DESIGN.md f-N14).
// Include after beom_moments.h (mom_sub, mom_add, mom_zero).
//
// Per field x (hlay, u, v; at level 2 also h_u, h_v) and K <= BEOM_MAX_HARMONICS frequencies the device keeps a reference
// and 1 + 2K sums shifted by it.  The weights cw_k = cos(omega_k*ctim), sw_k = sin(omega_k*ctim) of a sample are formed on
// the host (beom_harmonic_weights) and arrive as scalars; all FP64, no contraction, in this order, at every element:
//     first sample:   ref = x;  S0 = +0.0;  C_k = S_k = +0.0
//     later samples:  d = x - ref;  S0 = S0 + d;  C_k = C_k + d*cw_k;  S_k = S_k + d*sw_k      (the product rounded, then added)
// k ascending.  The normal matrix of the fit is the host's (include/beom_hip.h); the solve is the caller's.
//
// Elementwise as k_moments: the whole storage [0, nlay*n1) of a state array, sentinels and padding slots included (they hold
// constants and accumulate +0.0), 16-byte pairs from element 1 on, element 0 and an odd tail singly.  One launch per field:
// it reads x and ref and read-modify-writes 1 + 2K sums, at most 2 + 9 arrays, 4 + 4K words per element; FIRST only writes.
// The arrays and weights are named members chosen at compile time, never indexed.
#pragma once

struct HarmView {
    long long n;                                   // elements of every array: nlay * n1
    const double *x;                               // the field as the step leaves it
    double *r, *a0;                                // its reference and S0
    double *c1, *s1, *c2, *s2, *c3, *s3, *c4, *s4; // C_k, S_k (null beyond K)
    double cw1, sw1, cw2, sw2, cw3, sw3, cw4, sw4; // this sample's weights
};

__device__ __forceinline__ double harm_mul(double d, double w) { return d * w; }
__device__ __forceinline__ double2 harm_mul(double2 d, double w) { return make_double2(d.x * w, d.y * w); }

// one sample at elements [e, e + sizeof(T)/8): every load of the iteration stands in front of the first store
template <int K, bool FIRST, class T>
__device__ __forceinline__ void harmonics_at(const HarmView &h, long long e) {
    auto ld = [e](const double *p) { return *reinterpret_cast<const T *>(p + e); };
    auto st = [e](double *p, T v) { *reinterpret_cast<T *>(p + e) = v; };
    const T z = mom_zero<T>();
    const T x = ld(h.x);
    if constexpr (FIRST) {
        st(h.r, x); st(h.a0, z);
        st(h.c1, z); st(h.s1, z);
        if constexpr (K >= 2) { st(h.c2, z); st(h.s2, z); }
        if constexpr (K >= 3) { st(h.c3, z); st(h.s3, z); }
        if constexpr (K >= 4) { st(h.c4, z); st(h.s4, z); }
    } else {
        const T r = ld(h.r), a0 = ld(h.a0), c1 = ld(h.c1), s1 = ld(h.s1);
        T c2 = z, s2 = z, c3 = z, s3 = z, c4 = z, s4 = z;
        if constexpr (K >= 2) { c2 = ld(h.c2); s2 = ld(h.s2); }
        if constexpr (K >= 3) { c3 = ld(h.c3); s3 = ld(h.s3); }
        if constexpr (K >= 4) { c4 = ld(h.c4); s4 = ld(h.s4); }
        const T d = mom_sub(x, r);
        st(h.a0, mom_add(a0, d));
        st(h.c1, mom_add(c1, harm_mul(d, h.cw1))); st(h.s1, mom_add(s1, harm_mul(d, h.sw1)));
        if constexpr (K >= 2) { st(h.c2, mom_add(c2, harm_mul(d, h.cw2))); st(h.s2, mom_add(s2, harm_mul(d, h.sw2))); }
        if constexpr (K >= 3) { st(h.c3, mom_add(c3, harm_mul(d, h.cw3))); st(h.s3, mom_add(s3, harm_mul(d, h.sw3))); }
        if constexpr (K >= 4) { st(h.c4, mom_add(c4, harm_mul(d, h.cw4))); st(h.s4, mom_add(s4, harm_mul(d, h.sw4))); }
    }
}

// grid-stride over the pairs (1,2), (3,4), ...; the first two threads of the grid take the single elements
template <int K, bool FIRST>
__global__ void __launch_bounds__(BEOM_BLOCK) k_harmonics(const HarmView h) {
    const long long pairs = (h.n - 1) / 2;
    const long long t0 = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x, step = (long long)gridDim.x * BEOM_BLOCK;
    for (long long i = t0; i < pairs; i += step) harmonics_at<K, FIRST, double2>(h, 1 + 2 * i);
    if (t0 == 0) harmonics_at<K, FIRST, double>(h, 0);
    if (t0 == 1 && 1 + 2 * pairs < h.n) harmonics_at<K, FIRST, double>(h, h.n - 1);
}
