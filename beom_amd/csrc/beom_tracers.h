// beom_tracers.h — passive tracers carried by the layer transports (no reference routine; DESIGN.md f-N6).
// Include after beom_kernels.h.
//
// Per tracer the engine holds the layer CONTENT q = thickness x concentration and two history levels of its tendency, and
// advances q with the face transports h_u, h_v update_h is about to use and with update_h's own time scheme, so a tracer of
// concentration 1 IS the layer thickness, bit for bit.  Per layer l and cell p (E, N, W, S = neig(1|3|5|7, p)), all FP64,
// no contraction, in this order:
//     c(x)   = hlay(x,l) > 0 ? q(x,l) / hlay(x,l) : +0.0            wet(x) = hlay(x,l) > 0
//     Fu(p)  = h_u(p,l) * cf,  (a,b) = h_u(p,l) > 0 ? (W,p) : (p,W),  cf = wet(a) ? c(a) : c(b)
//     Fv(p)  = h_v(p,l) * cf,  (a,b) = h_v(p,l) > 0 ? (S,p) : (p,S),  cf = wet(a) ? c(a) : c(b)
//     src    = hdot present ? hdot(p,l) * (hdot(p,l) > 0 ? ctrg(p,l) : c(p)) : +0.0
//     r3     = ((Fu(p) - Fu(E)) * i_dl + (Fv(p) - Fv(N)) * i_dl + src) * mk_n(p)
//     rhsi   = ((1.5+beta)*r3 - (0.5+2*beta)*rq(2) + beta*rq(1)) * dt * gene + r3 * dt * (1-gene)
//     qh     = q + rhsi
//     hfor   = fnud(p,l,1) + (tide present ? ramp*tide(1,p,1)*vecl*cos(tide(2,p,1) - w_ti*ctim) : 0.0)
//     q_new  = (ctrg(p,l) * hfor) * nudg(p,1) + (1 - nudg(p,1)) * qh
//     rq(1) <- rq(2);  rq(2) <- r3
// Fu(E), Fv(N) are the same face expressions at cell E (N) with THAT cell's own W (S) link.  The no-gradient rule (an empty
// upwind cell hands over the other side's concentration) is what keeps the identity above where the reference's transports
// enter from land or from outside the frame.  First-order upstream: conservative, keeps a constant constant, NOT monotone.
//
// One launch per step for all tracers; the thickness / transport stencil of a cell-layer is read once and reused for
// every tracer.  q is written out of place (q -> q_alt, swapped by the host: neighbours read q); the tendency goes where the
// older level was (rq rotates by pointer).  Where the lanes of a wave are row neighbours (interior waves) the E / W
// concentrations, thicknesses and the E transport come by wavefront shuffle: three divisions per cell and tracer (own, N, S)
// plus one for the wave's two end lanes, instead of five.
#pragma once

struct TrcView {
    int ntrc, has_ctrg;
    const double *q;              // [ntrc][nlay][n1], read
    double *q_out;                // the partner q is written to
    double *rq0, *rq1;            // rq0 = rq(1,..) older (overwritten with the new tendency), rq1 = rq(2,..) newer
    const double *ctrg;           // relaxation concentration; null until uploaded (= +0.0)
};

#define TQ(a, ip, il, t) (a)[(long long)(ip) + d.n1 * ((long long)((il) - 1) + (long long)d.nlay * (long long)(t))]

__device__ __forceinline__ double trc_conc(double q, double h) { return h > 0.0 ? q / h : 0.0; }
// flux * cf for the face between `back` (W or S) and `here`
__device__ __forceinline__ double trc_face(double flux, double c_back, double h_back, double c_here, double h_here) {
    const double cf = flux > 0.0 ? (h_back > 0.0 ? c_back : c_here) : (h_here > 0.0 ? c_here : c_back);
    return flux * cf;
}

// the W link of E and the S link of N: the cell itself wherever links are plain offsets; on the rectangle a link into a
// slot that is no cell stands for the sentinel, whose own links are all 0; the table path reads the caller's table
__device__ __forceinline__ void trc_back_links(const CellPackedInt &c, const DevView &, int, int, int &wE, int &sN) { wE = c.ipnt; sN = c.ipnt; }
template <bool INT>
__device__ __forceinline__ void trc_back_links(const CellDenseT<INT> &c, const DevView &d, int c1, int c3, int &wE, int &sN) {
    if (INT) { wE = c.ipnt; sN = c.ipnt; return; }
    wE = (c1 != 0 && slot_is_cell(d, c1)) ? c.ipnt : 0;
    sN = (c3 != 0 && slot_is_cell(d, c3)) ? c.ipnt : 0;
}
__device__ __forceinline__ void trc_back_links(const CellGather &c, const DevView &d, int c1, int c3, int &wE, int &sN) {
    (void)c;
    wE = d.neig[8ll * c1 + 4];
    sN = d.neig[8ll * c3 + 6];
}

// FORCE as in k_update_h: 0 = no nudging anywhere, 1 = nudging, 2 = nudging + tidal constituent
template <int FORCE, class C>
__device__ __forceinline__ void body_tracers(const C &c, const DevView &d, const TrcView &tv, double gene, double ramp, double ctim) {
    constexpr bool FORCED = FORCE > 0;
    constexpr bool ROW = C::kLanesAreRowNeighbours;
    const int ipnt = c.ipnt, ilay = (int)blockIdx.y + 1;
    const int lane = (int)threadIdx.x & 63;
    const int c1 = c.template nb<1>(), c3 = c.template nb<3>(), c5 = c.template nb<5>(), c7 = c.template nb<7>();
    int wE, sN;
    trc_back_links(c, d, c1, c3, wE, sN);
    const double i_dl = d.i_dl, mkn = c.mk_n();
    const double ng = FORCED ? nudg_rate<1>(c, d) : 0.0;
    // thicknesses and transports of the stencil: once per cell-layer, for every tracer
    const double hP = LL(d.hlay, ipnt, ilay), hN = LL(d.hlay, c3, ilay), hS = LL(d.hlay, c7, ilay);
    const double huP = LL(d.h_u, ipnt, ilay), hvP = LL(d.h_v, ipnt, ilay), hvN = LL(d.h_v, c3, ilay);
    double hE, hW, huE, hWE = hP, hSN = hP;
    if (ROW) {
        hE = __shfl_down(hP, 1, 64); hW = __shfl_up(hP, 1, 64); huE = __shfl_down(huP, 1, 64);
        if (lane == 63) { hE = LL(d.hlay, c1, ilay); huE = LL(d.h_u, c1, ilay); }
        if (lane == 0) hW = LL(d.hlay, c5, ilay);
    } else {
        hE = LL(d.hlay, c1, ilay); hW = LL(d.hlay, c5, ilay); huE = LL(d.h_u, c1, ilay);
        hWE = LL(d.hlay, wE, ilay); hSN = LL(d.hlay, sN, ilay);
    }
    const double hd = d.has_hdot ? LL(d.hdot, ipnt, ilay) : 0.0;
    const bool want_ctrg = tv.has_ctrg && (FORCED || d.has_hdot);
    for (int t = 0; t < tv.ntrc; ++t) {
        const double qP = TQ(tv.q, ipnt, ilay, t);
        const double r1 = TQ(tv.rq0, ipnt, ilay, t), r2 = TQ(tv.rq1, ipnt, ilay, t);
        const double cP = trc_conc(qP, hP);
        const double cN = trc_conc(TQ(tv.q, c3, ilay, t), hN), cS = trc_conc(TQ(tv.q, c7, ilay, t), hS);
        double cE, cW, cWE = cP, cSN = cP;
        if (ROW) {
            cE = __shfl_down(cP, 1, 64); cW = __shfl_up(cP, 1, 64);
            if (lane == 0 || lane == 63) {          // the wave's end lanes: their outer neighbour belongs to another wave
                const double cx = trc_conc(TQ(tv.q, lane == 0 ? c5 : c1, ilay, t), lane == 0 ? hW : hE);
                if (lane == 0) cW = cx; else cE = cx;
            }
        } else {
            cE = trc_conc(TQ(tv.q, c1, ilay, t), hE); cW = trc_conc(TQ(tv.q, c5, ilay, t), hW);
            cWE = trc_conc(TQ(tv.q, wE, ilay, t), hWE); cSN = trc_conc(TQ(tv.q, sN, ilay, t), hSN);
        }
        const double Fu = trc_face(huP, cW, hW, cP, hP), FuE = trc_face(huE, cWE, hWE, cE, hE);
        const double Fv = trc_face(hvP, cS, hS, cP, hP), FvN = trc_face(hvN, cSN, hSN, cN, hN);
        const double ct = want_ctrg ? TQ(tv.ctrg, ipnt, ilay, t) : 0.0;
        const double src = d.has_hdot ? hd * (hd > 0.0 ? ct : cP) : 0.0;
        double r3 = (Fu - FuE) * i_dl + (Fv - FvN) * i_dl + src;
        r3 = r3 * mkn;
        const double rhsi = ((1.5 + d.beta) * r3 - (0.5 + 2.0 * d.beta) * r2 + d.beta * r1) * d.dt * gene + r3 * d.dt * (1.0 - gene);
        const double qh = qP + rhsi;
        // unforced: (ctrg*hfor)*0 + (1-0)*qh = (+-0) + qh; as update_h, written (+0) + qh
        double qnew = 0.0 + qh;
        if (FORCED) {
            if (ng == 0.0 && qh != 0.0) {
                qnew = qh;                        // (+-0) + qh for a non-zero qh: away from the sponges nothing more is fetched
            } else {
                double hfor = FNUD_(ipnt, ilay, 1);
                if (FORCE > 1) {
                    const double vecl = (ilay == 1) ? 1.0 : 0.0;
                    hfor = hfor + ramp * TIDE_(1, ipnt, 1) * vecl * cos(TIDE_(2, ipnt, 1) - d.w_ti * ctim);
                }
                qnew = (ct * hfor) * ng + (1.0 - ng) * qh;
            }
        }
        TQ(tv.q_out, ipnt, ilay, t) = qnew;
        TQ(tv.rq0, ipnt, ilay, t) = r3;           // host swaps rq0 <-> rq1 afterwards
    }
}

template <class CTX, int FORCE>
__global__ __launch_bounds__(BEOM_BLOCK) void k_tracers(DevView d, TrcView tv, double gene, double ramp, double ctim) {
    CTX c;
    if (!c.init(d)) return;
    if (c.wave_is_interior()) body_tracers<FORCE>(c.as_interior(), d, tv, gene, ramp, ctim);
    else body_tracers<FORCE>(c, d, tv, gene, ramp, ctim);
}

// ghost-row exchange: rows [jlo, jlo+nrows) of q <-> the part of the buffer behind k_rows_copy's five fields,
// [tracer][layer][row][column]; blockIdx.y = 1: the second group of rows <-> the second buffer
template <bool PACK>
__global__ __launch_bounds__(BEOM_BLOCK) void k_rows_copy_q(DevView d, double *q, int ntrc, int jlo, int nrows, double *buf, int jlo2, double *buf2) {
    if (blockIdx.y == 1) { jlo = jlo2; buf = buf2; }
    const long long per_lay = (long long)nrows * d.L;
    const long long total = (long long)ntrc * d.nlay * per_lay;
    const long long t = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x;
    if (t >= total) return;
    const long long lay = t / per_lay;           // tracer * nlay + layer
    const long long c = t - lay * per_lay;
    const long long row = c / d.L;
    const long long ip = 1 + (long long)(jlo - 1 + row) * (d.P ? d.P : d.L) + (c - row * d.L) + d.n1 * lay;
    if (PACK) buf[t] = q[ip];
    else q[ip] = buf[t];
}
