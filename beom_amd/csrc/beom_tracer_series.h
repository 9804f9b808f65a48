// beom_tracer_series.h — a record of the tracers' row inventories, variance, face fluxes and bounds per sampled step, kept on
// the device (no reference routine; DESIGN.md §4 "Tracer series").  Include after beom_tracer_moments.h and beom_series.h:
// trc_conc and trc_face are the sweep's own, the trees are the integrals'.
//
// Per tracer t, layer l and packed cell p (W, S = neig(5|7, p)), all FP64, no contraction, of the arrays as the step leaves
// them (where the tracer-moment sample stands):
//     x_q  = q(p,l,t)
//     c    = trc_conc(q(p,l,t), hlay(p,l))
//     x_v  = x_q * c                                                        (rounded, then summed: the row sum is sum h c^2)
//     x_fu = trc_face(h_u(p,l), c(W), hlay(W,l), c, hlay(p,l))
//     x_fv = trc_face(h_v(p,l), c(S), hlay(S,l), c, hlay(p,l))
//     x_b  = c + 0.0                                                        (a -0 becomes +0)
// One record is rec[(j-1)*cnt + ((t*nlay + (l-1))*nq + m)] for the recorder's rows j, nq = 2 * LEVEL, cnt = ntrc*nlay*nq:
//     m = 0 inv = sum x_q, 1 var = sum x_v (level 1);  2 fu = sum x_fu, 3 fv = sum x_fv (level 2);  4 cmin, 5 cmax (level 3).
// The sums follow the integrals' live rule (+0.0 where there is no packed cell and on the duplicated column / row of a
// periodic frame) and order of summation (the pairwise tree over the aligned column index, beom_integrals.h).  The bounds
// are the minimum and maximum of x_b over the live positions with hlay(p,l) > 0, +inf and -inf where there is none; no
// signed zero enters, so any order of comparison gives the same bits.
//
// k_integral_rows' geometry: a wavefront = 64 aligned columns of one row, a workgroup = BEOM_TILE_Y consecutive rows of one
// chunk; a lane walks the layers of its cell and, inside a layer, the tracers.  hlay at p, W, S and h_u, h_v at p are read
// once per cell-layer for all tracers; in interior waves the W thickness and the W concentration come by wavefront shuffle
// and lane 0 loads its own (as body_tracer_moments): two divisions per cell and tracer at level >= 2, one at level 1.
// Compulsory words per cell-layer: hlay(p), h_u(p), h_v(p), then q(p) per tracer: 3 + ntrc (1 + ntrc at level 1).  Chunk
// partials go to part[(r * nch + chunk) * cnt + k]; k_tracer_series_chunks finishes every row straight into the record's
// slot.  No atomics, no workgroup waits for another, nothing comes back to the host.
#pragma once

// the minimum of a and the maximum of b over the wave in 6 exchanges instead of 12: the odd lane of a pair carries -max
// (negation is exact, and max = -min of the negated values), from there on every lane carries one minimum.  Padding lanes
// hold +inf and -inf.  Result: the minimum in lane 0, MINUS the maximum in lane 1.
__device__ __forceinline__ double tracer_series_wave_bounds(double mn, double mx, int lane) {
    const bool odd = lane & 1;
    const double nmx = -mx;
    double v = fmin(odd ? nmx : mn, __shfl_xor(odd ? mn : nmx, 1, 64));
#pragma unroll
    for (int s = 2; s < 64; s <<= 1) v = fmin(v, __shfl_xor(v, s, 64));
    return v;
}

// one wavefront = 64 consecutive columns of one row.  live = false: the lane's position holds +0.0 in the sums and the
// identities in the bounds (no cell there, or the duplicated column / row); its context is that of some valid slot.
template <int LEVEL, class C>
__device__ __forceinline__ void body_tracer_series(const C &c, const DevView &d, const double *q, int ntrc, bool live, int width,
                                                   double *out) {
    constexpr bool ROW = C::kLanesAreRowNeighbours;
    constexpr bool FACES = LEVEL >= 2;
    constexpr int NQ = 2 * LEVEL;
    const int ipnt = c.ipnt;
    const int lane = (int)threadIdx.x & 63;
    const int c5 = FACES ? c.template nb<5>() : 0, c7 = FACES ? c.template nb<7>() : 0;
    for (int ilay = 1; ilay <= d.nlay; ++ilay) {
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
        const bool wet = live && hP > 0.0;
        for (int t = 0; t < ntrc; ++t) {
            const double xq = TQ(q, ipnt, ilay, t);
            const double xc = trc_conc(xq, hP);
            const double xv = xq * xc;
            double *o2 = out + ((long long)t * d.nlay + (ilay - 1)) * NQ;
            const double s_q = live ? xq : 0.0, s_v = live ? xv : 0.0;
            if (!FACES) {
                if (width >= 2) {
                    const double s = integral_wave_tree2(s_q, s_v, width, lane);
                    if (lane < 2) o2[lane] = s;
                } else if (lane == 0) {
                    o2[0] = s_q; o2[1] = s_v;
                }
                continue;
            }
            const double cS = trc_conc(TQ(q, c7, ilay, t), hS);
            double cW;
            if (ROW) {
                cW = __shfl_up(xc, 1, 64);
                if (lane == 0) cW = trc_conc(TQ(q, c5, ilay, t), hW);        // its W neighbour belongs to another wave
            } else {
                cW = trc_conc(TQ(q, c5, ilay, t), hW);
            }
            const double xfu = trc_face(huP, cW, hW, xc, hP), xfv = trc_face(hvP, cS, hS, xc, hP);
            double s_fu = live ? xfu : 0.0, s_fv = live ? xfv : 0.0;
            if (width >= 4) {
                const double s = integral_wave_tree4(s_q, s_v, s_fu, s_fv, width, lane);
                if (lane < 4) o2[((lane & 1) << 1) | (lane >> 1)] = s;       // lanes 0, 1, 2, 3 hold inv, fu, var, fv
            } else {
                const double a = integral_wave_tree(s_q, width), b = integral_wave_tree(s_v, width);
                s_fu = integral_wave_tree(s_fu, width); s_fv = integral_wave_tree(s_fv, width);
                if (lane == 0) { o2[0] = a; o2[1] = b; o2[2] = s_fu; o2[3] = s_fv; }
            }
            if (LEVEL >= 3) {
                const double xb = xc + 0.0;
                const double s = tracer_series_wave_bounds(wet ? xb : HUGE_VAL, wet ? xb : -HUGE_VAL, lane);
                if (lane < 2) o2[4 + lane] = lane ? -s : s;
            }
        }
    }
}

// k_integral_rows' geometry and arguments, and the tracers' contents and count; part[(r * nch + chunk) * cnt + k] with
// cnt = ntrc * nlay * 2 * LEVEL
template <bool DENSE, int LEVEL>
__global__ __launch_bounds__(BEOM_BLOCK) void k_tracer_series_rows(DevView d, const double *q, int ntrc, int jlo, int nrows, int width,
                                                                   int xdup, int ydup, const int32_t *cellmap, double *part) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.y * BEOM_TILE_Y + wave;
    if (r >= nrows) return;
    const int j = jlo + r, chunk = (int)blockIdx.x, i = chunk * 64 + lane + 1;
    const bool in = i <= d.L;
    const bool dup = (xdup && i == d.L) || (ydup && j + d.joff == d.Mg);
    double *out = part + ((long long)r * (int)gridDim.x + chunk) * ((long long)ntrc * d.nlay * (2 * LEVEL));
    if constexpr (DENSE) {
        CellDense c;
        c.set_cell(d, in ? i : d.L, j);
        const bool live = in && !dup && slot_is_cell(d, c.ipnt);
        if (c.wave_is_interior()) body_tracer_series<LEVEL>(c.as_interior(), d, q, ntrc, live, width, out);
        else body_tracer_series<LEVEL>(c, d, q, ntrc, live, width, out);
    } else {
        CellGather c;
        c.ipnt = in ? cellmap[(long long)(j - 1) * d.L + (i - 1)] : 0;
        c.row = d.neig + 8ll * c.ipnt;
        c.dv = &d;
        body_tracer_series<LEVEL>(c, d, q, ntrc, c.ipnt != 0 && !dup, width, out);
    }
}

// The chunks of a row -> the row's entries, straight into the record: one wavefront per row and tracer-layer, a lane per
// chunk.  Entries m < 4 are summed by k_integral_chunks' tree (+0.0 past the row's last chunk); m = 4, 5 take the minimum
// resp. maximum (+inf, -inf past the last chunk).  Rows of more than 64 chunks go group by group of 64 aligned chunks and
// lane 0 finishes over the groups in LDS (ngroups a power of two, <= kIntegralMaxGroups).
__global__ __launch_bounds__(64) void k_tracer_series_chunks(const double *part, double *rows, int cnt, int nq, int nch, int nchp2) {
    __shared__ double grp[kIntegralMaxGroups];
    const int lane = (int)threadIdx.x;
    const long long r = blockIdx.x;
    const double *p = part + r * nch * cnt;
    const int width = nchp2 < 64 ? nchp2 : 64, ngroups = nchp2 < 64 ? 1 : nchp2 / 64;
    for (int m = 0; m < nq; ++m) {
        const int k = (int)blockIdx.y * nq + m;
        const double pad = m < 4 ? 0.0 : (m == 4 ? HUGE_VAL : -HUGE_VAL);
        double v = pad;
        for (int g = 0; g < ngroups; ++g) {
            const int c = g * 64 + lane;
            v = c < nch ? p[(long long)c * cnt + k] : pad;
            if (m < 4) {
                v = integral_wave_tree(v, width);
            } else {
#pragma unroll
                for (int s = 1; s < 64; s <<= 1) {
                    const double w = __shfl_xor(v, s, 64);
                    v = m == 4 ? fmin(v, w) : fmax(v, w);
                }
            }
            if (ngroups > 1 && lane == 0) grp[g] = v;
        }
        if (lane == 0) {
            if (ngroups > 1) {
                for (int n = ngroups; n > 1; n >>= 1)
                    for (int i = 0; i < n / 2; ++i)
                        grp[i] = m < 4 ? grp[2 * i] + grp[2 * i + 1] : (m == 4 ? fmin(grp[2 * i], grp[2 * i + 1]) : fmax(grp[2 * i], grp[2 * i + 1]));
                v = grp[0];
            }
            rows[r * cnt + k] = v;
        }
    }
}
