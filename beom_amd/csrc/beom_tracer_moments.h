// beom_tracer_moments.h — time means of the tracers' content, concentration and face fluxes, and the concentration's second
// moment (no reference routine; DESIGN.md f-N9).  Include after beom_tracers.h: trc_conc and trc_face are the sweep's own.
//
// Per tracer t, layer l and real cell p (W, S = neig(5|7, p)) four quantities are sampled, k = 0..3:
//     x_q  = q(p,l,t)
//     x_c  = trc_conc(q(p,l,t), hlay(p,l))
//     x_fu = trc_face(h_u(p,l), c(W), hlay(W,l), c(p), hlay(p,l))          the upstream face between W and p
//     x_fv = trc_face(h_v(p,l), c(S), hlay(S,l), c(p), hlay(p,l))          the upstream face between S and p
// and fed to the moments' shifted sums (beom_moments.h), all FP64, no contraction, in this order:
//     first sample:   ref_k = x_k;  S_k = +0.0;  Q = +0.0
//     later samples:  d_k = x_k - ref_k;  S_k = S_k + d_k;  Q = Q + d_c*d_c            (the product rounded, then added)
// LEVEL 1 keeps ref, S of q and c; LEVEL 2 adds those of fu, fv; LEVEL 3 adds Q.  A sample stands at the very end of a step,
// where q, hlay, h_u, h_v are what the next step's tracer sweep reads: under scheme 1 x_fu, x_fv are that sweep's Fu(p),
// Fv(p) bit for bit.  Under scheme 2 they are still the upstream faces (Koren's face is not restated here).
//
// One thread per cell-layer, a loop over the tracers; hlay at p, W, S and h_u, h_v at p are read once per cell-layer.  Where
// the lanes of a wave are row neighbours (interior waves) the W thickness and the W concentration come by wavefront shuffle
// and lane 0 loads its own.  Per tracer every load of ref, S and Q stands in front of the first store.  The accumulators are
// [ntrc][nlay][n1] arrays of the state's padded layout and travel as named pointers of a kernel argument of their own; slots
// that are no real cell (sentinel, padding, land slots of the rectangle) are never written and keep the +0.0 they were
// allocated with.  Compulsory words per cell-layer: hlay(p), h_u(p), h_v(p) once (hlay(W), hlay(S), q(W), q(S) are other
// threads' own words), then per tracer q(p), four ref read, four S and Q read and written: 3 + (1 + 4 + 8 + 2) ntrc =
// 3 + 15 ntrc at level 3; a FIRST sample reads q(p) and writes four ref, four S and Q: 3 + 10 ntrc.  No atomics, no LDS.
#pragma once

struct TrcMomentView {
    int ntrc;
    const double *q;                               // [ntrc][nlay][n1], as the step leaves it
    double *r_q, *r_c, *r_fu, *r_fv;               // the references
    double *s_q, *s_c, *s_fu, *s_fv;               // the shifted sums
    double *sq_c;                                  // the shifted second moment of the concentration (level 3)
};

template <int LEVEL, bool FIRST, class C>
__device__ __forceinline__ void body_tracer_moments(const C &c, const DevView &d, const TrcMomentView &m) {
    constexpr bool ROW = C::kLanesAreRowNeighbours;
    constexpr bool FACES = LEVEL >= 2;
    const int ipnt = c.ipnt, ilay = (int)blockIdx.y + 1;
    const int lane = (int)threadIdx.x & 63;
    const int c5 = FACES ? c.template nb<5>() : 0, c7 = FACES ? c.template nb<7>() : 0;
    // thicknesses and transports of the stencil: once per cell-layer, for every tracer
    const double hP = LL(d.hlay, ipnt, ilay);
    double hW = 0.0, hS = 0.0, huP = 0.0, hvP = 0.0;
    if (FACES) {
        hS = LL(d.hlay, c7, ilay); huP = LL(d.h_u, ipnt, ilay); hvP = LL(d.h_v, ipnt, ilay);
        if (ROW) {
            hW = __shfl_up(hP, 1, 64);
            if (lane == 0) hW = LL(d.hlay, c5, ilay);
        } else {
            hW = LL(d.hlay, c5, ilay);
        }
    }
    for (int t = 0; t < m.ntrc; ++t) {
        const double xq = TQ(m.q, ipnt, ilay, t);
        const double xc = trc_conc(xq, hP);
        double xfu = 0.0, xfv = 0.0;
        if (FACES) {
            const double cS = trc_conc(TQ(m.q, c7, ilay, t), hS);
            double cW;
            if (ROW) {
                cW = __shfl_up(xc, 1, 64);
                if (lane == 0) cW = trc_conc(TQ(m.q, c5, ilay, t), hW);      // its W neighbour belongs to another wave
            } else {
                cW = trc_conc(TQ(m.q, c5, ilay, t), hW);
            }
            xfu = trc_face(huP, cW, hW, xc, hP);
            xfv = trc_face(hvP, cS, hS, xc, hP);
        }
        if (FIRST) {
            TQ(m.r_q, ipnt, ilay, t) = xq; TQ(m.r_c, ipnt, ilay, t) = xc;
            TQ(m.s_q, ipnt, ilay, t) = 0.0; TQ(m.s_c, ipnt, ilay, t) = 0.0;
            if (FACES) {
                TQ(m.r_fu, ipnt, ilay, t) = xfu; TQ(m.r_fv, ipnt, ilay, t) = xfv;
                TQ(m.s_fu, ipnt, ilay, t) = 0.0; TQ(m.s_fv, ipnt, ilay, t) = 0.0;
            }
            if (LEVEL >= 3) TQ(m.sq_c, ipnt, ilay, t) = 0.0;
            continue;
        }
        const double rq = TQ(m.r_q, ipnt, ilay, t), rc = TQ(m.r_c, ipnt, ilay, t);
        const double sq = TQ(m.s_q, ipnt, ilay, t), sc = TQ(m.s_c, ipnt, ilay, t);
        const double rfu = FACES ? TQ(m.r_fu, ipnt, ilay, t) : 0.0, rfv = FACES ? TQ(m.r_fv, ipnt, ilay, t) : 0.0;
        const double sfu = FACES ? TQ(m.s_fu, ipnt, ilay, t) : 0.0, sfv = FACES ? TQ(m.s_fv, ipnt, ilay, t) : 0.0;
        const double qc = LEVEL >= 3 ? TQ(m.sq_c, ipnt, ilay, t) : 0.0;
        const double dq = xq - rq, dc = xc - rc;
        TQ(m.s_q, ipnt, ilay, t) = sq + dq; TQ(m.s_c, ipnt, ilay, t) = sc + dc;
        if (FACES) {
            const double dfu = xfu - rfu, dfv = xfv - rfv;
            TQ(m.s_fu, ipnt, ilay, t) = sfu + dfu; TQ(m.s_fv, ipnt, ilay, t) = sfv + dfv;
        }
        if (LEVEL >= 3) {
            const double pc = dc * dc;
            TQ(m.sq_c, ipnt, ilay, t) = qc + pc;
        }
    }
}

template <class CTX, int LEVEL, bool FIRST>
__global__ __launch_bounds__(BEOM_BLOCK) void k_tracer_moments(DevView d, TrcMomentView m) {
    CTX c;
    if (!c.init(d)) return;
    if (c.wave_is_interior()) body_tracer_moments<LEVEL, FIRST>(c.as_interior(), d, m);
    else body_tracer_moments<LEVEL, FIRST>(c, d, m);
}
