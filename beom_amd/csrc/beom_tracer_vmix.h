// beom_tracer_vmix.h — vertical (diapycnal) diffusion of the passive tracers between the layers of a water column (no
// reference routine; DESIGN.md f-N12).  Include after beom_tracers.h: trc_conc and TQ are the sweep's own.
//
// An operator-split backward-Euler update of the layer CONTENT q in a launch of its own, behind the lateral mixing and in
// front of the tracer sweep of either scheme, while q and hlay still belong to the same time level.  The unknowns are the
// FLUXES G_k through the interfaces k = 1..nlay-1 (between layers k and k+1, 1 = top), not the concentrations.  Per cell p
// and tracer t, all FP64, no contraction, in this order:
//     m_l   = hlay(p,l) > 0
//     c_l   = trc_conc(q_l, h_l)                    (m_l ? q_l / h_l : +0.0)
//     b_l   = m_l ? 1.0 / h_l : +0.0                (once per cell, for every tracer)
//     rk(t,k) = 1.0 / (dt * kappa_v(t,k))           formed on the HOST (product first, then reciprocal); +0.0 where
//                                                   kappa_v(t,k) == 0
//     open(k) = mk_n(p) > 0.5 && m_k && m_{k+1} && rk(t,k) > 0
//     forward, k = 1 .. nlay-1, with s_0 = 1.0, y_0 = +0.0:
//         R   = (0.5 * (h_k + h_{k+1})) * rk(t,k)
//         pp  = R + b_k * s_{k-1}
//         den = pp + b_{k+1}
//         inv = 1.0 / den
//         num = (c_k - c_{k+1}) + b_k * y_{k-1}
//         open(k):  g_k = b_{k+1} * inv;  y_k = num * inv;  s_k = pp * inv
//         else:     g_k = +0.0;           y_k = +0.0;       s_k = 1.0
//     back:  G_{nlay-1} = y_{nlay-1};   G_k = y_k + g_k * G_{k+1};   G_0 = G_nlay = +0.0
//     q'_l = m_l ? (q_l + G_{l-1}) - G_l : q_l
// G_k is the content moved from layer k into layer k+1 during the step: it solves
//     G_k (R_k + b_k + b_{k+1}) - b_k G_{k-1} - b_{k+1} G_{k+1} = c_k - c_{k+1},
// which is G = (dt kappa / hbar)(c'_k - c'_{k+1}) with c' = q'/h and hbar the mean of the two thicknesses.  The elimination
// carries s_k = 1 - g_k as pp/den, so nothing nearly equal and positive is ever subtracted.  The matrix's row sum is
// R_k >= 0: stable for every kappa_v, and kappa_v -> infinity gives the thickness-weighted column mean.  Every G_k enters two
// layers with opposite sign: the column sum of q changes by rounding only.  With q = hlay every c is exactly 1, every num, y
// and G is +0 and q' = q: the identity of beom_tracers.h survives.  A dry layer, a land cell, the sentinel or
// kappa_v(t,k) = 0 closes an interface and the column falls into independent pieces; a thin wet layer conducts (its
// resistance is its thickness).  The error is rounding of the content, a few units of 2^-52 (|q_l| + |G_{l-1}| + |G_l|): a
// massless layer's CONCENTRATION is accurate only to the rounding of the content that passes through it, as in any
// conservative form.  dt is the handle's dt in steps 1-3 too; rq is not touched.
//
// One thread per cell walks the layers (nz = 1, as k_update_h does where one thread takes the column); NL = nlay is a
// template argument, every layer loop unrolls and the column lives in registers: h and b once per cell, q, g and y per
// tracer.  A column reads its own cell only, so q is updated IN PLACE (no partner array, no swap); only cells are written.
// Every layer's load and store is lane-contiguous.  The next tracer's q column is asked for before the current one's
// elimination.  rk is one device array [ntrc][nlay-1] read at wave-uniform addresses, never an indexed kernel argument.
// No LDS, no atomics, no cross-lane traffic.  Compulsory words per cell-layer: hlay once, then per tracer q read and
// written: 1 + 2 ntrc.  Divisions per cell: nlay + ntrc (2 nlay - 1).
#pragma once

struct TrcVmixView {
    int ntrc;
    double *q;                    // [ntrc][nlay][n1], updated in place
    const double *rk;             // [ntrc][nlay-1]: 1 / (dt * kappa_v), +0 = closed
};

template <int NL, class C>
__device__ __forceinline__ void body_tracer_vmix(const C &c, const DevView &d, const TrcVmixView &m) {
    const int ipnt = c.ipnt;
    const bool wet_cell = c.mk_n() > 0.5;
    double *__restrict__ q = m.q;
    // thicknesses of the column, once per cell for every tracer; the first tracer's contents are asked for with them
    double h[NL], b[NL], qn[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) h[l] = LL(d.hlay, ipnt, l + 1);
#pragma unroll
    for (int l = 0; l < NL; ++l) qn[l] = TQ(q, ipnt, l + 1, 0);
#pragma unroll
    for (int l = 0; l < NL; ++l) b[l] = h[l] > 0.0 ? 1.0 / h[l] : 0.0;
    for (int t = 0; t < m.ntrc; ++t) {
        const double *rk = m.rk + t * (NL - 1);                     // wave-uniform
        double qq[NL], g[NL - 1], y[NL - 1];
        // (an empty statement that hands h back unchanged: what depends on h alone - the wet and open predicates, a lane
        // mask in two scalar registers each, and the mean thicknesses - is then formed where a tracer uses it and not kept
        // for all tracers, which at 12 layers and more cost more scalar registers than a wave has)
#pragma unroll
        for (int l = 0; l < NL; ++l) asm volatile("" : "+v"(h[l]));
        // (and the layer stride likewise at 12 layers and more: the layers' offsets are then lane arithmetic where they
        // are used, not 2 NL scalar registers held through the loop)
        long long n1 = d.n1;
        if constexpr (NL >= 12) asm volatile("" : "+v"(n1));
        double *qt = q + ((long long)ipnt + n1 * ((long long)NL * t));      // TQ(q, ipnt, 1, t); d.nlay is NL
#pragma unroll
        for (int l = 0; l < NL; ++l) qq[l] = qn[l];
        // the next tracer's column is in flight while this one's divisions run (a column is its own cell's: no aliasing)
        if (t + 1 < m.ntrc) {
#pragma unroll
            for (int l = 0; l < NL; ++l) qn[l] = qt[n1 * (NL + l)];
        }
        double s = 1.0, yp = 0.0, ck = trc_conc(qq[0], h[0]);
#pragma unroll
        for (int k = 0; k < NL - 1; ++k) {
            const double cn = trc_conc(qq[k + 1], h[k + 1]);
            const double r = rk[k];
            const double R = (0.5 * (h[k] + h[k + 1])) * r;
            const double pp = R + b[k] * s;
            const double den = pp + b[k + 1];
            const double inv = 1.0 / den;
            const double num = (ck - cn) + b[k] * yp;
            const bool open = wet_cell && h[k] > 0.0 && h[k + 1] > 0.0 && r > 0.0;
            g[k] = open ? b[k + 1] * inv : 0.0;
            yp = open ? num * inv : 0.0;
            s = open ? pp * inv : 1.0;
            y[k] = yp;
            ck = cn;
        }
        // back substitution from the bottom; a layer is stored as soon as both of its fluxes are known
        double Gb = 0.0;                                             // G_l of the layer in hand (G_nlay = +0)
#pragma unroll
        for (int l = NL - 1; l >= 0; --l) {
            double Ga = 0.0;                                         // G_{l-1} (G_0 = +0)
            if (l > 0) Ga = l == NL - 1 ? y[l - 1] : y[l - 1] + g[l - 1] * Gb;
            double hl = h[l];
            asm volatile("" : "+v"(hl));                              // (likewise: m_l is compared again, not kept from the way down)
            qt[n1 * l] = hl > 0.0 ? (qq[l] + Ga) - Gb : qq[l];
            Gb = Ga;
        }
    }
}

template <class CTX, int NL>
__global__ __launch_bounds__(BEOM_BLOCK) void k_tracer_vmix(DevView d, TrcVmixView m) {
    CTX c;
    if (!c.init(d)) return;
    body_tracer_vmix<NL>(c, d, m);
}
