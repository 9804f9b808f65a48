// beom_tracer_mix.h — lateral diffusion, decay and sources of the passive tracers (no reference routine; DESIGN.md f-N11).
// Include after beom_tracers.h: trc_conc, trc_back_links and TQ are the sweep's own.
//
// An operator-split forward-Euler update of the layer CONTENT q in a launch of its own, in front of the tracer sweep of either
// scheme, while q and hlay still belong to the same time level.  Per tracer t, layer l and cell p (E, N, W, S =
// neig(1|3|5|7, p)), all FP64, no contraction, in this order:
//     c(x)     = hlay(x,l) > 0 ? q(x,l) / hlay(x,l) : +0.0                       (trc_conc itself)
//     kd       = kappa(t,l) * i_dl
//     G(b, x)  = hf > 0 ? (kd * hf) * (c(b) - c(x)) : +0.0,   hf = fmin(hlay(b,l), hlay(x,l))
//     Gu(p) = G(W(p), p)    Gu(E) = G(W(E), E)    Gv(p) = G(S(p), p)    Gv(N) = G(S(N), N)
//     div      = ((Gu(p) - Gu(E)) + (Gv(p) - Gv(N))) * i_dl
//     r        = ((div + source(t,l) * hlay(p,l)) - decay(t,l) * q(p,l)) * mk_n(p)
//     q_mix    = hlay(p,l) > 0 ? q(p,l) + dt * r : q(p,l)
// W(E), S(N) are cell E's and N's own back links by the rule of trc_back_links (the sentinel's links are 0, a rectangle slot
// that is no cell stands for the sentinel, the table path reads neig).  G(b, x) is the diffusive flux of content into x through
// the face it shares with b, div(kappa h grad c) in flux form; the face is as thick as the thinner of its two cells, so a face
// next to land, a dry cell, the frame's edge or an open boundary carries nothing (hlay(0) = 0), every weight hf / hlay(p) is
// at most 1 and kappa dt / dl^2 <= 1/4 makes the new concentration a convex combination of the five old ones.  decay is a
// rate in 1/s, source adds concentration per second.  dt is the handle's dt in steps 1-3 too; rq is not touched.  With
// q = hlay and decay = source = +0 every c is exactly 1, every G is +0 and q_mix = q: the identity of beom_tracers.h survives.
//
// One launch for all tracers; hlay at p, E, N, W, S is read once per cell-layer and reused for every tracer.  q is written out
// of place (q -> q_alt, swapped by the host: neighbours read q); only cells are written.  Where the lanes of a wave are row
// neighbours (interior waves) the E / W thicknesses and concentrations come by wavefront shuffle and Gu(E) is the neighbour
// lane's Gu(p) — the same expression, hence the same bits; the wave's end lanes fetch their outer neighbour themselves: three
// divisions per cell and tracer (own, N, S) plus one for the end lanes.  The coefficients are one device array
// [3][ntrc][nlay] (kappa, decay, source) read at wave-uniform addresses, never an indexed kernel argument.  A tracer-layer
// whose three coefficients are +0 goes through the same arithmetic (the swap is per array, so its q has to reach the partner).
// A thread asks for the next tracer's q (own, N, S, and an end lane's outer neighbour) before it divides the current one's.
// Compulsory words per cell-layer: hlay(p) once, then per tracer q(p) read and q_alt(p) written: 1 + 2 ntrc.  No LDS.
#pragma once

struct TrcMixView {
    int ntrc;
    const double *q;              // [ntrc][nlay][n1], read
    double *q_out;                // the partner q_mix is written to
    const double *coef;           // [3][ntrc][nlay]: kappa, decay, source
};

// the diffusive flux of content into `here` through the face it shares with `back`
__device__ __forceinline__ double trc_mix_face(double kd, double c_back, double h_back, double c_here, double h_here) {
    const double hf = fmin(h_back, h_here);
    return hf > 0.0 ? (kd * hf) * (c_back - c_here) : 0.0;
}

template <class C>
__device__ __forceinline__ void body_tracer_mix(const C &c, const DevView &d, const TrcMixView &m) {
    constexpr bool ROW = C::kLanesAreRowNeighbours;
    const int ipnt = c.ipnt, ilay = (int)blockIdx.y + 1;
    const int lane = (int)threadIdx.x & 63;
    const int c1 = c.template nb<1>(), c3 = c.template nb<3>(), c5 = c.template nb<5>(), c7 = c.template nb<7>();
    int wE, sN;
    trc_back_links(c, d, c1, c3, wE, sN);
    const double i_dl = d.i_dl, dt = d.dt, mkn = c.mk_n();
    const double *__restrict__ q = m.q;
    double *__restrict__ q_out = m.q_out;
    // thicknesses of the stencil: once per cell-layer, for every tracer; the first tracer's contents are asked for with them
    const double hP = LL(d.hlay, ipnt, ilay), hN = LL(d.hlay, c3, ilay), hS = LL(d.hlay, c7, ilay);
    double qP = TQ(q, ipnt, ilay, 0), qN = TQ(q, c3, ilay, 0), qS = TQ(q, c7, ilay, 0);
    // the wave's end lanes: their outer neighbour (W of lane 0, E of lane 63) belongs to another wave
    const bool end = ROW && (lane == 0 || lane == 63);
    const int cX = lane == 0 ? c5 : c1;
    double qX = 0.0;
    double hE, hW, hWE = hP, hSN = hP;
    if (ROW) {
        double hX = 0.0;
        if (end) { hX = LL(d.hlay, cX, ilay); qX = TQ(q, cX, ilay, 0); }
        hE = __shfl_down(hP, 1, 64); hW = __shfl_up(hP, 1, 64);
        if (lane == 63) hE = hX;
        if (lane == 0) hW = hX;
    } else {
        hE = LL(d.hlay, c1, ilay); hW = LL(d.hlay, c5, ilay);
        if (wE != ipnt) hWE = LL(d.hlay, wE, ilay);
        if (sN != ipnt) hSN = LL(d.hlay, sN, ilay);
    }
    const int nco = m.ntrc * d.nlay;
    for (int t = 0; t < m.ntrc; ++t) {
        const double *co = m.coef + (t * d.nlay + (ilay - 1));      // wave-uniform
        const double kd = co[0] * i_dl, decay = co[nco], source = co[2 * nco];
        // the next tracer's contents are in flight while this one's divisions run (q_out is another array: __restrict__)
        double nP = 0.0, nN = 0.0, nS = 0.0, nX = 0.0;
        if (t + 1 < m.ntrc) {
            nP = TQ(q, ipnt, ilay, t + 1); nN = TQ(q, c3, ilay, t + 1); nS = TQ(q, c7, ilay, t + 1);
            if (end) nX = TQ(q, cX, ilay, t + 1);
        }
        const double cP = trc_conc(qP, hP), cN = trc_conc(qN, hN), cS = trc_conc(qS, hS);
        double Gu, GuE;
        if (ROW) {
            double cW = __shfl_up(cP, 1, 64), cx = 0.0;
            if (end) cx = trc_conc(qX, lane == 0 ? hW : hE);                 // one more division for the two end lanes
            if (lane == 0) cW = cx;
            Gu = trc_mix_face(kd, cW, hW, cP, hP);
            GuE = __shfl_down(Gu, 1, 64);                                    // the E lane's own Gu(p)
            if (lane == 63) GuE = trc_mix_face(kd, cP, hP, cx, hE);
        } else {
            const double cE = trc_conc(TQ(q, c1, ilay, t), hE), cW = trc_conc(TQ(q, c5, ilay, t), hW);
            const double cWE = wE != ipnt ? trc_conc(TQ(q, wE, ilay, t), hWE) : cP;
            Gu = trc_mix_face(kd, cW, hW, cP, hP);
            GuE = trc_mix_face(kd, cWE, hWE, cE, hE);
        }
        const double cSN = (ROW || sN == ipnt) ? cP : trc_conc(TQ(q, sN, ilay, t), hSN);
        const double Gv = trc_mix_face(kd, cS, hS, cP, hP), GvN = trc_mix_face(kd, cSN, hSN, cN, hN);
        const double div = ((Gu - GuE) + (Gv - GvN)) * i_dl;
        double r = (div + source * hP) - decay * qP;
        r = r * mkn;
        TQ(q_out, ipnt, ilay, t) = hP > 0.0 ? qP + dt * r : qP;
        qP = nP; qN = nN; qS = nS; qX = nX;
    }
}

template <class CTX>
__global__ __launch_bounds__(BEOM_BLOCK) void k_tracer_mix(DevView d, TrcMixView m) {
    CTX c;
    if (!c.init(d)) return;
    if (c.wave_is_interior()) body_tracer_mix(c.as_interior(), d, m);
    else body_tracer_mix(c, d, m);
}
