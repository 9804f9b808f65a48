// beom_maps.h — a record of sums over aligned B x B blocks of cells per sampled step, kept on the device (no reference routine;
// DESIGN.md §4 "Maps").  Include after beom_tracer_column_series.h, behind every other kernel header (the kernels before it
// keep their place in the code object): ColumnTree and the ColumnRows* contexts are the column series'.
//
// B = 2^logb (2..64), Lc = ceil(L/B), Mc = ceil(M/B); block (I, J) covers i = (I-1)B+1 .. IB, j = (J-1)B+1 .. JB on the global
// indices.  One record is rec[(k*Mc + (J-1))*Lc + (I-1)], an image per entry k:
//     k = 0                          n, the sum of 1.0 over the block's live cells
//     k = 1 + (l-1)*E + m            per layer l; E = 3 at level 1, 6 at level 2 and above
//         m = 0 h   mk_n * hlay      m = 1 u   the cell's own u        m = 2 v   the cell's own v
//         m = 3 ke  mk_u*((u*u)*hcu) + mk_v*((v*v)*hcv) (body_integral's statement, beom_integrals.h)
//         m = 4 hu  the stored h_u   m = 5 hv  the stored h_v
//     k = 1 + 6*nlay + t*nlay + (l-1)   level 3: the content q of tracer t
// Live rule: the integrals' (+0.0 past L or M, where there is no packed cell, at the sentinel and on the duplicated column / row
// of a periodic frame).  Order of summation: inside a block each column's B rows go through the pairwise tree over the row
// offset, then the B column sums through the pairwise tree over the column offset: a complete binary tree, its only padding
// the +0.0 of the positions that are not live.
//
// k_map_blocks: a wavefront owns 64 consecutive columns (a lane per column: every own-cell load is coalesced) and the B rows
// of one block row; a lane pushes its rows through the streaming tree in registers, then the 64/B groups of B lanes combine in
// logb cross-lane steps (lane ^ 2^s at step s: both partners form a + b, which IEEE addition commutes, so every lane of a group
// ends with the group's bits) and the group's first lane stores.  The layer loop is outermost, the tracers of a layer follow
// its fields one at a time: the tree holds 6 * kMapMaxLog doubles at most.  A block is finished inside one wavefront: no
// scratch, no LDS, no barrier, no atomics, and the four waves of a workgroup are independent (four chunks of columns).
// logb is a run-time, wave-uniform kernel argument, not a template parameter: the tree's levels are static registers either
// way and the row loop is rolled, so six block edges x three levels x two layouts would be 36 kernels for no shorter code.
#pragma once

constexpr int kMapMaxLog = 6;                  // B <= 64: a block's columns fit a wavefront
constexpr int kMapWaves = BEOM_BLOCK / 64;

// the sum over each aligned group of 2^logb lanes, in tree order over the lane offset; every lane of the wave must be active
__device__ __forceinline__ double map_group(double v, int logb) {
#pragma unroll
    for (int s = 0; s < kMapMaxLog; ++s)
        if (s < logb) v = v + __shfl_xor(v, 1 << s, 64);
    return v;
}

// The terms of one cell and layer.  first: the block's first row loads hS; every later row takes it from the row below, which
// this lane has just finished (p_h0: its h0 — the same array element, hence the same bits), as column_terms does.
template <int LEVEL, class C>
__device__ __forceinline__ void map_terms(const C &c, const DevView &d, bool live, int ilay, bool first, double &p_h0,
                                          double (&t)[LEVEL >= 2 ? 6 : 3]) {
    const int ipnt = c.ipnt;
    const double h0 = LL(d.hlay, ipnt, ilay), u0 = LL(d.u, ipnt, ilay), v0 = LL(d.v, ipnt, ilay);
    t[0] = live ? c.mk_n() * h0 : 0.0;
    t[1] = live ? u0 : 0.0;
    t[2] = live ? v0 : 0.0;
    if constexpr (LEVEL >= 2) {
        const double mku = c.mk_u(), mkv = c.mk_v();
        const double hW = LL(d.hlay, c.template nb<5>(), ilay);
        double hS = p_h0;
        if (first) hS = LL(d.hlay, c.template nb<7>(), ilay);
        const double hcu = (hW + h0) / (1.0 + mku);
        const double hcv = (h0 + hS) / (1.0 + mkv);
        const double hu = LL(d.h_u, ipnt, ilay), hv = LL(d.h_v, ipnt, ilay);
        t[3] = live ? mku * ((u0 * u0) * hcu) + mkv * ((v0 * v0) * hcv) : 0.0;
        t[4] = live ? hu : 0.0;
        t[5] = live ? hv : 0.0;
    }
    p_h0 = h0;
}

// A wavefront's block row in one form of rows (beom_column_series.h): all layers and, at LEVEL 3, their tracers.  out: the
// lane's block in image 0; img = Mc * Lc; store: the lane is the first of a group whose block exists.  OPAQUE: the layer (and
// tracer) index goes through a vector register, so that its offset is added per load, not kept as a scalar base per array
// (the general forms have no registers for those, as column_layer says).
template <int LEVEL, bool OPAQUE, class ROWS>
__device__ __forceinline__ void map_wave(const ROWS &rows, const DevView &d, const double *q, int ntrc, int logb, double *out,
                                         long long img, bool store) {
    constexpr int E = LEVEL >= 2 ? 6 : 3;
    const int B = 1 << logb;
    for (int ilay = 1; ilay <= d.nlay; ++ilay) {
        ColumnTree<E, kMapMaxLog> tree;
        double sum[E], nlive = 0.0, p_h0 = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) sum[e] = 0.0;
#pragma unroll 1
        for (int r = 0; r < B; ++r) {
            const auto c = rows.cell(r);
            const bool live = rows.live(r, c);
            int il = ilay;
            if constexpr (OPAQUE) asm volatile("" : "+v"(il));
            double t[E];
            map_terms<LEVEL>(c, d, live, il, r == 0, p_h0, t);
            nlive = nlive + (live ? 1.0 : 0.0);
            tree.push(r, t, sum, logb);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double s = map_group(sum[e], logb);
            if (store) out[(1 + (long long)(ilay - 1) * E + e) * img] = s;
        }
        if (ilay == 1) {                       // (the live positions are every layer's)
            const double n = map_group(nlive, logb);
            if (store) out[0] = n;
        }
        if constexpr (LEVEL >= 3) {
            for (int t = 0; t < ntrc; ++t) {
                ColumnTree<1, kMapMaxLog> qtree;
                double qsum[1] = {0.0};
#pragma unroll 1
                for (int r = 0; r < B; ++r) {
                    const auto c = rows.cell(r);
                    const bool live = rows.live(r, c);
                    int il = ilay, tt = t;
                    if constexpr (OPAQUE) asm volatile("" : "+v"(il), "+v"(tt));
                    const double xq = TQ(q, c.ipnt, il, tt);
                    const double x[1] = {live ? xq : 0.0};
                    qtree.push(r, x, qsum, logb);
                }
                const double s = map_group(qsum[0], logb);
                if (store) out[(1 + 6ll * d.nlay + (long long)t * d.nlay + (ilay - 1)) * img] = s;
            }
        }
    }
}

// Grid (chunks of 64 columns / kMapWaves, block rows); a wave per chunk.  xdup, ydup: the frame wraps (its column lm+1 resp.
// row mm+1 is a duplicate); cellmap: the table path's packed cell of every (i, j); rec: the record's slot, [cnt][Mc][Lc].
template <bool DENSE, int LEVEL>
__global__ __launch_bounds__(BEOM_BLOCK) void k_map_blocks(DevView d, const double *q, int ntrc, int logb, int xdup, int ydup,
                                                           const int32_t *cellmap, double *rec, int Lc, int Mc) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int chunk = (int)blockIdx.x * kMapWaves + wave;
    if (chunk * 64 >= d.L) return;             // (wave-uniform: the waves of a workgroup do not meet again)
    const int B = 1 << logb, J = (int)blockIdx.y;
    const int i = chunk * 64 + lane + 1, j0 = J * B + 1;
    const int I = (i - 1) >> logb;
    const bool store = (lane & (B - 1)) == 0 && I < Lc && J < Mc;
    const long long img = (long long)Mc * Lc;
    double *out = rec + ((long long)J * Lc + (store ? I : 0));
    constexpr int kNoWindow = 0x7fffffff;      // (no row window, no -0.0 padding: the maps' padding is +0.0 throughout)
    if constexpr (DENSE) {
        const int i0 = __builtin_amdgcn_readfirstlane(i - lane);
        // (no band keeps maps: local rows are global rows)
        bool interior = i0 >= 2 && i0 + 63 <= d.L - 2 && j0 >= 2 && j0 + B - 1 <= d.M - 2;
        if (interior && d.embedded)            // (every 64 x 4 tile of reg4 the block row touches)
            for (int t4 = (j0 - 1) >> 2; t4 <= (j0 + B - 2) >> 2; ++t4)
                interior = interior && d.reg4[(long long)t4 * d.reg_nx + ((i0 - 1) >> 6)] != 0;
        if (interior) map_wave<LEVEL, false>(ColumnRowsInterior{&d, i, j0}, d, q, ntrc, logb, out, img, store);
        else map_wave<LEVEL, true>(ColumnRowsDense{&d, i, j0, 1, d.M, kNoWindow, xdup, ydup}, d, q, ntrc, logb, out, img, store);
    } else {
        map_wave<LEVEL, true>(ColumnRowsGather{&d, cellmap, i, j0, 1, d.M, kNoWindow, xdup, ydup}, d, q, ntrc, logb, out, img, store);
    }
}
