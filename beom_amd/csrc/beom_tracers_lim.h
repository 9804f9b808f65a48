// beom_tracers_lim.h — the flux-limited tracer scheme (beom_set_tracer_scheme, scheme 2; DESIGN.md f-N6).
// Include after beom_tracers.h.
//
// Everything of beom_tracers.h stays except the face concentration cf.  For the face of cell x towards its back neighbour B
// (B = W(x) for Fu, B = S(x) for Fv), with F = the stored transport at x, all FP64, no contraction, in this order:
//     (U, D, UU) = F > 0 ? (B, x, back(B)) : (x, B, fwd(x))     back = W|S link, fwd = E|N link, each of the cell named
//     first      = wet(U) ? c(U) : c(D)                          (scheme 1's cf, no-gradient rule included)
//     if !(wet(U) && wet(D) && wet(UU))   cf = first
//     else  du = c(U) - c(UU);  dd = c(D) - c(U)
//           if (du*dd > 0.0)  m   = fmin(fmin(2.0*fabs(du), 2.0*fabs(dd)), fabs((du + 2.0*dd) * T3)),   T3 = 1.0/3.0 (FP64)
//                             lim = copysign(m, dd)
//           else              lim = +0.0
//           cf = c(U) + 0.5*lim
//     flux = F * cf
// Koren's limiter: the kappa = 1/3 third-order upwind-biased face value where the field is smooth, clipped to stay between
// the upwind and the downwind cell.  The links of the sentinel are all 0 and hlay(0) = 0, so next to land, a dry cell or the
// frame's edge the face falls back to scheme 1's value; with every concentration equal du = dd = 0, lim = +0.0 and
// cf = c(U) exactly, which keeps the identity with hlay.  A method-of-lines limiter under the thickness equation's
// three-level time scheme: bounds were kept in the runs measured at |u|dt/dl = 0.1 with |v|dt/dl = 0.05 and at 0.15 with
// 0.075; it goes unstable at 0.25 + 0.125 (upstream itself at 0.4 + 0.2).  Nothing of that is asserted here.
//
// Two forms, one arithmetic:
//  * by links (the table path, and on the rectangle every tile that touches land, the frame's rim, a periodic seam or a
//    band's edge): a thread follows the links of its cell twice — the caller's table, or the closed form of CellDenseT with
//    a slot that is no cell standing for the sentinel — and divides for every cell of its four faces' stencils;
//  * tiled (interior tiles of dense and embedded handles, 64 x 8 and 64 x 4): the thickness and, per tracer, the
//    concentration of the tile plus a ring of two are staged in LDS — one division per staged cell, (64+4)(R+4)/(64 R) =
//    1.6 per cell at R = 8 —, and every face value comes from LDS with plain offsets and no mask.
//    LDS: two images of (R+4) x 68 doubles, 13 KB at R = 8 (8.7 KB at R = 4); rows are read and written 64 consecutive
//    doubles at a time, so the pitch needs no padding.
#pragma once

template <int Q> struct TrcTiled {};                 // the CTX of k_tracers_lim on the rectangle: tiles of 64 x 4Q cells

template <int Q>
struct TrcLimGeom {
    using G = TileGeom<Q>;
    static constexpr int SR = G::TY + 4, SC = G::TX + 4;       // tile + ring of two
    static constexpr int NS = SR * SC, NSI = (NS + G::BLOCK - 1) / G::BLOCK;
};

__device__ __forceinline__ double trc_lim_cf(double cU, bool wU, double cD, bool wD, double cUU, bool wUU) {
    if (!(wU && wD && wUU)) return wU ? cU : cD;
    constexpr double T3 = 1.0 / 3.0;
    const double du = cU - cUU, dd = cD - cU;
    double lim = 0.0;
    if (du * dd > 0.0) {
        const double m = fmin(fmin(2.0 * fabs(du), 2.0 * fabs(dd)), fabs((du + 2.0 * dd) * T3));
        lim = copysign(m, dd);
    }
    return cU + 0.5 * lim;
}

// ---- links ---------------------------------------------------------------------------------------------------------------
// a cell as the link walkers see it: its index, and on the rectangle its local coordinates (a = 0: the sentinel)
struct TrcPos { int t, a, b; };
struct TrcLinkTable {                                // the caller's neig (row 0, the sentinel's, is all 0)
    template <int K> static __device__ __forceinline__ TrcPos step(const DevView &d, const TrcPos &p) {
        return TrcPos{d.neig[8ll * p.t + (K - 1)], 0, 0};
    }
};
struct TrcLinkDense {                                // CellDenseT<false>::at, with a slot that is no cell = the sentinel
    template <int K> static __device__ __forceinline__ TrcPos step(const DevView &d, const TrcPos &p) {
        if (p.a == 0) return TrcPos{0, 0, 0};
        int a = p.a + NbOff<K>::di, b = p.b + NbOff<K>::dj;
        if (!halo_target<false>(d, a, b)) return TrcPos{0, 0, 0};
        const int t = a + (b - 1) * d.P;
        if (!slot_is_cell(d, t)) return TrcPos{0, 0, 0};
        return TrcPos{t, a, b};
    }
};
// (U, D, UU) of the face of cell x towards its back neighbour, F = the transport stored at x
template <class LK, bool XDIR>
__device__ __forceinline__ void trc_lim_stencil(const DevView &d, const TrcPos &x, double F, int (&s)[3]) {
    constexpr int BACK = XDIR ? 5 : 7, FWD = XDIR ? 1 : 3;
    const TrcPos B = LK::template step<BACK>(d, x);
    if (F > 0.0) { s[0] = B.t; s[1] = x.t; s[2] = LK::template step<BACK>(d, B).t; }
    else { s[0] = x.t; s[1] = B.t; s[2] = LK::template step<FWD>(d, x).t; }
}

// ---- from the fluxes to q_new: the statements of body_tracers -------------------------------------------------------------
template <int FORCE>
__device__ __forceinline__ void trc_lim_finish(const DevView &d, const TrcView &tv, int ipnt, int ilay, int t, double qP, double cP,
                                               double Fu, double FuE, double Fv, double FvN, double hd, bool want_ctrg,
                                               double mkn, double ng, double gene, double ramp, double ctim) {
    constexpr bool FORCED = FORCE > 0;
    const double r1 = TQ(tv.rq0, ipnt, ilay, t), r2 = TQ(tv.rq1, ipnt, ilay, t);
    const double ct = want_ctrg ? TQ(tv.ctrg, ipnt, ilay, t) : 0.0;
    const double src = d.has_hdot ? hd * (hd > 0.0 ? ct : cP) : 0.0;
    double r3 = (Fu - FuE) * d.i_dl + (Fv - FvN) * d.i_dl + src;
    r3 = r3 * mkn;
    const double rhsi = ((1.5 + d.beta) * r3 - (0.5 + 2.0 * d.beta) * r2 + d.beta * r1) * d.dt * gene + r3 * d.dt * (1.0 - gene);
    const double qh = qP + rhsi;
    double qnew = 0.0 + qh;                           // unforced: (+-0) + qh, written (+0) + qh as update_h does
    if (FORCED) {
        if (ng == 0.0 && qh != 0.0) {
            qnew = qh;
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
    TQ(tv.rq0, ipnt, ilay, t) = r3;                   // host swaps rq0 <-> rq1 afterwards
}

// ---- one cell by its links ------------------------------------------------------------------------------------------------
template <int FORCE, class LK>
__device__ __forceinline__ void body_tracers_lim_links(const DevView &d, const TrcView &tv, const TrcPos &p, int ilay, double mkn, double ng,
                                                       double gene, double ramp, double ctim) {
    const int ipnt = p.t;
    const TrcPos E = LK::template step<1>(d, p), N = LK::template step<3>(d, p);
    // the four faces: Fu(p), Fu(E), Fv(p), Fv(N); their transports, stencils and thicknesses once for every tracer
    double F[4];
    F[0] = LL(d.h_u, ipnt, ilay); F[1] = LL(d.h_u, E.t, ilay); F[2] = LL(d.h_v, ipnt, ilay); F[3] = LL(d.h_v, N.t, ilay);
    int s[4][3];
    trc_lim_stencil<LK, true>(d, p, F[0], s[0]);
    trc_lim_stencil<LK, true>(d, E, F[1], s[1]);
    trc_lim_stencil<LK, false>(d, p, F[2], s[2]);
    trc_lim_stencil<LK, false>(d, N, F[3], s[3]);
    double h[4][3];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int k = 0; k < 3; ++k) h[f][k] = LL(d.hlay, s[f][k], ilay);
    const double hP = LL(d.hlay, ipnt, ilay);
    const double hd = d.has_hdot ? LL(d.hdot, ipnt, ilay) : 0.0;
    const bool want_ctrg = tv.has_ctrg && (FORCE > 0 || d.has_hdot);
    for (int t = 0; t < tv.ntrc; ++t) {
        const double qP = TQ(tv.q, ipnt, ilay, t);
        const double cP = trc_conc(qP, hP);
        double fl[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const double cU = trc_conc(TQ(tv.q, s[f][0], ilay, t), h[f][0]), cD = trc_conc(TQ(tv.q, s[f][1], ilay, t), h[f][1]);
            const double cUU = trc_conc(TQ(tv.q, s[f][2], ilay, t), h[f][2]);
            fl[f] = F[f] * trc_lim_cf(cU, h[f][0] > 0.0, cD, h[f][1] > 0.0, cUU, h[f][2] > 0.0);
        }
        trc_lim_finish<FORCE>(d, tv, ipnt, ilay, t, qP, cP, fl[0], fl[1], fl[2], fl[3], hd, want_ctrg, mkn, ng, gene, ramp, ctim);
    }
}

// ---- an interior tile: every cell of the tile and of its ring of two is a wet-or-dry cell of the frame with plain links ------
template <int Q, int FORCE>
__device__ __forceinline__ void body_tracers_lim_int(const DevView &d, const TrcView &tv, int x0, int y0, int ilay, double gene,
                                                     double ramp, double ctim, double (*s_h)[TrcLimGeom<Q>::SC],
                                                     double (*s_c)[TrcLimGeom<Q>::SC]) {
    using G = TileGeom<Q>;
    using B = TrcLimGeom<Q>;
    const int tid = threadIdx.x;
    const int lx = tid & 63, wy = tid >> 6;
    const long long lay = d.n1 * (long long)(ilay - 1);
    // ---- the thicknesses of the stage, and what a thread keeps of its own cells for every tracer
    double hh[B::NSI];
    int sr[B::NSI], sc[B::NSI];
    long long sg[B::NSI];
#pragma unroll
    for (int k = 0; k < B::NSI; ++k) {
        const int idx = tid + k * G::BLOCK;
        const int idc = idx < B::NS ? idx : tid;         // clamped: the load is harmless, the store is skipped
        sr[k] = idc / B::SC; sc[k] = idc - sr[k] * B::SC;
        sg[k] = (long long)(x0 - 2 + sc[k]) + (long long)(y0 - 3 + sr[k]) * d.P + lay;
        hh[k] = d.hlay[sg[k]];
    }
    double hu[Q], huE[Q], hv[Q], hvN[Q], hd[Q], ng[Q];
    bool sel[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = y0 + wy + G::WAVES * q;
        sel[q] = row_selected(d, j);
        const long long ip = (long long)(x0 + lx) + (long long)(j - 1) * d.P + lay;
        hu[q] = d.h_u[ip]; huE[q] = d.h_u[ip + 1]; hv[q] = d.h_v[ip]; hvN[q] = d.h_v[ip + d.P];
        hd[q] = d.has_hdot ? d.hdot[ip] : 0.0;
        ng[q] = 0.0;
        if (FORCE > 0) {
            CellDenseT<true> cc;
            cc.set_cell(d, x0 + lx, j);
            ng[q] = nudg_rate<1>(cc, d);
        }
    }
#pragma unroll
    for (int k = 0; k < B::NSI; ++k)
        if (tid + k * G::BLOCK < B::NS) s_h[sr[k]][sc[k]] = hh[k];
    __syncthreads();
    // wet flags of a cell's stencil: bit 0..4 = columns c-2..c+2 of its row, bit 5..8 = rows r-2, r-1, r+1, r+2 of its column
    unsigned wet[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int r = wy + G::WAVES * q + 2, c = lx + 2;
        unsigned w = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) w |= (s_h[r][c - 2 + k] > 0.0 ? 1u : 0u) << k;
        w |= (s_h[r - 2][c] > 0.0 ? 1u : 0u) << 5; w |= (s_h[r - 1][c] > 0.0 ? 1u : 0u) << 6;
        w |= (s_h[r + 1][c] > 0.0 ? 1u : 0u) << 7; w |= (s_h[r + 2][c] > 0.0 ? 1u : 0u) << 8;
        wet[q] = w;
    }
    const bool want_ctrg = tv.has_ctrg && (FORCE > 0 || d.has_hdot);
    const long long per_trc = d.n1 * (long long)d.nlay;
    for (int t = 0; t < tv.ntrc; ++t) {
        double cc[B::NSI];
#pragma unroll
        for (int k = 0; k < B::NSI; ++k) cc[k] = trc_conc(tv.q[sg[k] + per_trc * t], hh[k]);
        if (t > 0) __syncthreads();                      // the faces of the tracer before have been read
#pragma unroll
        for (int k = 0; k < B::NSI; ++k)
            if (tid + k * G::BLOCK < B::NS) s_c[sr[k]][sc[k]] = cc[k];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (!sel[q]) continue;
            const int rr = wy + G::WAVES * q, r = rr + 2, c = lx + 2;
            const unsigned w = wet[q];
            const double xm2 = s_c[r][c - 2], xm1 = s_c[r][c - 1], c0 = s_c[r][c], xp1 = s_c[r][c + 1], xp2 = s_c[r][c + 2];
            const double ym2 = s_c[r - 2][c], ym1 = s_c[r - 1][c], yp1 = s_c[r + 1][c], yp2 = s_c[r + 2][c];
            const bool wxm2 = w & 1u, wxm1 = w & 2u, w0 = w & 4u, wxp1 = w & 8u, wxp2 = w & 16u;
            const bool wym2 = w & 32u, wym1 = w & 64u, wyp1 = w & 128u, wyp2 = w & 256u;
            const double Fu = hu[q] * (hu[q] > 0.0 ? trc_lim_cf(xm1, wxm1, c0, w0, xm2, wxm2) : trc_lim_cf(c0, w0, xm1, wxm1, xp1, wxp1));
            const double FuE = huE[q] * (huE[q] > 0.0 ? trc_lim_cf(c0, w0, xp1, wxp1, xm1, wxm1) : trc_lim_cf(xp1, wxp1, c0, w0, xp2, wxp2));
            const double Fv = hv[q] * (hv[q] > 0.0 ? trc_lim_cf(ym1, wym1, c0, w0, ym2, wym2) : trc_lim_cf(c0, w0, ym1, wym1, yp1, wyp1));
            const double FvN = hvN[q] * (hvN[q] > 0.0 ? trc_lim_cf(c0, w0, yp1, wyp1, ym1, wym1) : trc_lim_cf(yp1, wyp1, c0, w0, yp2, wyp2));
            const int ipnt = (x0 + lx) + (y0 + rr - 1) * d.P;
            const double qP = TQ(tv.q, ipnt, ilay, t);
            trc_lim_finish<FORCE>(d, tv, ipnt, ilay, t, qP, c0, Fu, FuE, Fv, FvN, hd[q], want_ctrg, 1.0, ng[q], gene, ramp, ctim);
        }
    }
}

// ---- a tile by links ---------------------------------------------------------------------------------------------------------
template <int Q, int FORCE>
__device__ __forceinline__ void body_tracers_lim_edge(const DevView &d, const TrcView &tv, int x0, int y0, int ilay, double gene,
                                                      double ramp, double ctim) {
    using G = TileGeom<Q>;
    const int lx = (int)threadIdx.x & 63, wy = (int)threadIdx.x >> 6;
    const int i = x0 + lx;
    for (int q = 0; q < Q; ++q) {
        const int j = y0 + wy + G::WAVES * q;
        if (!(i <= d.L && j <= d.M && row_selected(d, j))) continue;
        CellDenseT<false> cc;
        cc.set_cell(d, i, j);
        if (!slot_is_cell(d, cc.ipnt)) continue;         // embedded: land slots keep the sentinel's values
        const double ng = FORCE > 0 ? nudg_rate<1>(cc, d) : 0.0;
        body_tracers_lim_links<FORCE, TrcLinkDense>(d, tv, TrcPos{cc.ipnt, i, j}, ilay, cc.mk_n(), ng, gene, ramp, ctim);
    }
}

template <int FORCE>
__device__ __forceinline__ void tracers_lim_workgroup(CellGather c, const DevView &d, const TrcView &tv, double gene, double ramp, double ctim) {
    if (!c.init(d)) return;
    const double ng = FORCE > 0 ? nudg_rate<1>(c, d) : 0.0;
    body_tracers_lim_links<FORCE, TrcLinkTable>(d, tv, TrcPos{c.ipnt, 0, 0}, (int)blockIdx.y + 1, c.mk_n(), ng, gene, ramp, ctim);
}
template <int FORCE, int Q>
__device__ __forceinline__ void tracers_lim_workgroup(TrcTiled<Q>, const DevView &d, const TrcView &tv, double gene, double ramp, double ctim) {
    using G = TileGeom<Q>;
    using B = TrcLimGeom<Q>;
    __shared__ double s_h[B::SR][B::SC];
    __shared__ double s_c[B::SR][B::SC];
    const TileMap tm(d, G::TX, G::TY);
    int ty, ch;
    if (!tm.locate(blockIdx.x, ty, ch)) return;               // whole block: no barrier is skipped by part of it
    const int x0 = ch * G::TX + 1, y0 = ty * G::TY + 1;
    const int ilay = blockIdx.y + 1;
    // block-uniform: the tile and its ring of two lie in 2..L-2 x 2..M-2 (global rows too), no land within 3 cells
    const bool interior = x0 - 2 >= 2 && x0 + G::TX + 1 <= d.L - 2 && y0 - 2 >= 2 && y0 + G::TY + 1 <= d.M - 2
                          && y0 - 2 + d.joff >= 2 && y0 + G::TY + 1 + d.joff <= d.Mg - 2 && tile_regular(d, x0, y0, G::TY);
    if (interior) body_tracers_lim_int<Q, FORCE>(d, tv, x0, y0, ilay, gene, ramp, ctim, s_h, s_c);
    else body_tracers_lim_edge<Q, FORCE>(d, tv, x0, y0, ilay, gene, ramp, ctim);
}

// CTX = CellGather (table path) or TrcTiled<Q> (dense and embedded handles); FORCE as in k_tracers
template <class CTX, int FORCE>
__global__ __launch_bounds__(BEOM_BLOCK) void k_tracers_lim(DevView d, TrcView tv, double gene, double ramp, double ctim) {
    tracers_lim_workgroup<FORCE>(CTX{}, d, tv, gene, ramp, ctim);
}
template <int Q>
static inline dim3 tracers_lim_grid(const DevView &d) {
    return dim3(TileMap(d, TileGeom<Q>::TX, TileGeom<Q>::TY).blocks(), (unsigned)d.nlay, 1);
}
