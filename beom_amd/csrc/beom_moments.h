// beom_moments.h — time means and second moments of the layer fields (no reference routine; DESIGN.md f-N8).
// Include after beom_kernels.h.
//
// The five fields f = 0..4 are hlay, u, v, h_u, h_v.  The sums are shifted by a reference that the first sample sets; all
// FP64, no contraction, in this order, at every element:
//     first sample:   ref_f = x_f;  S_f = +0.0;  Q_m = +0.0
//     later samples:  d_f = x_f - ref_f;  S_f = S_f + d_f;  Q_m = Q_m + d_a*d_b          (the product rounded, then added)
//     m = 0..4:       (a, b) = (h,h) (u,u) (v,v) (u,h_u) (v,h_v)
// mean = ref + S/count and (co)variance = Q/count - (S_a/count)*(S_b/count) are the caller's.  A plain sum of x and x*x
// loses a deep layer's signal: on h = 4000 + 0.01*sin(..) + noise the plain variance is off by 7.2e-3 relative after
// 100 000 samples, the shifted one by 5.8e-14 (include/beom_hip.h).
// LEVEL 1 keeps ref, S of hlay, u, v; LEVEL 2 adds those of h_u, h_v; LEVEL 3 adds the five Q.  Nothing else is touched.
//
// Purely elementwise: no cell context, no DevView.  The kernel runs over the whole storage [0, nlay*n1) of the state
// arrays, sentinels and padding slots included (they hold constants and accumulate +0.0); references and sums live in
// arrays of the same shape and alignment (element 1 on a 128-byte boundary, as dev_alloc leaves it).  So every array is
// read and written as 16-byte pairs starting at element 1; element 0 and, when nlay*n1 is even, the last element are
// taken singly.  The arrays travel as named pointers of a kernel argument of their own, never indexed.  FIRST writes only;
// later samples read the fields and references and read-modify-write the sums: 12 / 20 / 30 words per element.
#pragma once

struct MomentView {
    long long n;                                   // elements of every array: nlay * n1
    const double *x0, *x1, *x2, *x3, *x4;          // hlay, u, v, h_u, h_v as the step leaves them
    double *r0, *r1, *r2, *r3, *r4;                // the references
    double *s0, *s1, *s2, *s3, *s4;                // the shifted sums
    double *q0, *q1, *q2, *q3, *q4;                // the shifted second moments (level 3)
};

__device__ __forceinline__ double mom_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double mom_add(double a, double b) { return a + b; }
__device__ __forceinline__ double mom_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double2 mom_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 mom_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 mom_mul(double2 a, double2 b) { return make_double2(a.x * b.x, a.y * b.y); }
template <class T> __device__ __forceinline__ T mom_zero();
template <> __device__ __forceinline__ double mom_zero<double>() { return 0.0; }
template <> __device__ __forceinline__ double2 mom_zero<double2>() { return make_double2(0.0, 0.0); }

// one sample at elements [e, e + sizeof(T)/8): every load of the iteration stands in front of the first use
template <int LEVEL, bool FIRST, class T>
__device__ __forceinline__ void moments_at(const MomentView &m, long long e) {
    auto ld = [e](const double *p) { return *reinterpret_cast<const T *>(p + e); };
    auto st = [e](double *p, T v) { *reinterpret_cast<T *>(p + e) = v; };
    const T z = mom_zero<T>();
    const T x0 = ld(m.x0), x1 = ld(m.x1), x2 = ld(m.x2);
    const T x3 = LEVEL >= 2 ? ld(m.x3) : z, x4 = LEVEL >= 2 ? ld(m.x4) : z;
    if (FIRST) {
        st(m.r0, x0); st(m.r1, x1); st(m.r2, x2);
        st(m.s0, z); st(m.s1, z); st(m.s2, z);
        if (LEVEL >= 2) { st(m.r3, x3); st(m.r4, x4); st(m.s3, z); st(m.s4, z); }
        if (LEVEL >= 3) { st(m.q0, z); st(m.q1, z); st(m.q2, z); st(m.q3, z); st(m.q4, z); }
        return;
    }
    const T r0 = ld(m.r0), r1 = ld(m.r1), r2 = ld(m.r2);
    const T s0 = ld(m.s0), s1 = ld(m.s1), s2 = ld(m.s2);
    const T r3 = LEVEL >= 2 ? ld(m.r3) : z, r4 = LEVEL >= 2 ? ld(m.r4) : z;
    const T s3 = LEVEL >= 2 ? ld(m.s3) : z, s4 = LEVEL >= 2 ? ld(m.s4) : z;
    const T q0 = LEVEL >= 3 ? ld(m.q0) : z, q1 = LEVEL >= 3 ? ld(m.q1) : z, q2 = LEVEL >= 3 ? ld(m.q2) : z;
    const T q3 = LEVEL >= 3 ? ld(m.q3) : z, q4 = LEVEL >= 3 ? ld(m.q4) : z;
    const T d0 = mom_sub(x0, r0), d1 = mom_sub(x1, r1), d2 = mom_sub(x2, r2);
    st(m.s0, mom_add(s0, d0)); st(m.s1, mom_add(s1, d1)); st(m.s2, mom_add(s2, d2));
    if (LEVEL >= 2) {
        const T d3 = mom_sub(x3, r3), d4 = mom_sub(x4, r4);
        st(m.s3, mom_add(s3, d3)); st(m.s4, mom_add(s4, d4));
        if (LEVEL >= 3) {
            st(m.q0, mom_add(q0, mom_mul(d0, d0))); st(m.q1, mom_add(q1, mom_mul(d1, d1))); st(m.q2, mom_add(q2, mom_mul(d2, d2)));
            st(m.q3, mom_add(q3, mom_mul(d1, d3))); st(m.q4, mom_add(q4, mom_mul(d2, d4)));
        }
    }
}

// grid-stride over the pairs (1,2), (3,4), ...; the first two threads of the grid take the single elements
template <int LEVEL, bool FIRST>
__global__ void __launch_bounds__(BEOM_BLOCK) k_moments(const MomentView m) {
    const long long pairs = (m.n - 1) / 2;
    const long long t0 = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x, step = (long long)gridDim.x * BEOM_BLOCK;
    for (long long i = t0; i < pairs; i += step) moments_at<LEVEL, FIRST, double2>(m, 1 + 2 * i);
    if (t0 == 0) moments_at<LEVEL, FIRST, double>(m, 0);
    if (t0 == 1 && 1 + 2 * pairs < m.n) moments_at<LEVEL, FIRST, double>(m, m.n - 1);
}
