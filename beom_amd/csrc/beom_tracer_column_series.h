// beom_tracer_column_series.h — a record of the tracers' column inventories, variance, face fluxes and bounds per sampled step,
// kept on the device (no reference routine; DESIGN.md §4 "Tracer column series").  Include after beom_column_series.h, behind
// every other kernel header (the kernels before it keep their place in the code object): ColumnTree, the ColumnRows* contexts
// and column_combine are the column series', trc_conc and trc_face the tracer sweep's own.
//
// Per tracer t, layer l and packed cell p the quantities are the tracer series' (beom_tracer_series.h), word for word:
//     x_q = q(p,l,t),  c = trc_conc(x_q, hlay(p,l)),  x_v = x_q * c (rounded, then summed),
//     x_fu = trc_face(h_u(p,l), c(W), hlay(W,l), c, hlay(p,l)),  x_fv = trc_face(h_v(p,l), c(S), hlay(S,l), c, hlay(p,l)),
//     x_b = c + 0.0.
// One record is cols[(i-1)*cnt + ((t*nlay + (l-1))*nq + m)] for the columns i = 1..L, nq = 2 * LEVEL, cnt = ntrc*nlay*nq:
//     m = 0 inv, 1 var (level 1);  2 fu, 3 fv (level 2);  4 cmin, 5 cmax (level 3).
// Live rule: the integrals' and the tracer series' (+0.0 where there is no packed cell and on the duplicated column / row of
// a periodic frame) and, outside the row window wlo..whi, +0.0.  Order of summation: the column series' — the pairwise tree
// over the aligned global row index r = j-1, the column padded with +0.0 to M2; rows past M2 inside a block hold -0.0
// (beom_column_series.h).  cmin, cmax: the minimum and maximum of x_b over the live positions of the column inside the window
// with hlay > 0, +inf and -inf where there is none; no signed zero enters, so any order of comparison gives the same bits.
//
// Stage 1, k_tracer_column_blocks: k_column_blocks' geometry (a wavefront = 64 columns, a lane per column, kColRows aligned
// rows; four waves make a block of kColBlockRows rows through LDS in tree order).  Layers outer, tracers in the middle, the
// rows innermost: one tracer's tree is live at a time.  The S thickness and S concentration of a row are the row below's own
// hlay and c (the same array elements through the same function, hence the same bits); in interior waves the W thickness and
// W concentration come by wavefront shuffle and lane 0 loads and divides its own: one division per cell and tracer plus the
// first row's S and lane 0's W.  Compulsory words per cell-layer: hlay, h_u, h_v, then q per tracer: 3 + ntrc (1 + ntrc at
// level 1).  Partials: part[(block * cnt + k) * colpad + column].  Stage 2, k_tracer_column_finish: a thread per (column,
// entry); sums walk the block partials in tree order as k_column_finish does, bounds take fmin resp. fmax over the blocks.
// No atomics, no workgroup waits for another, nothing comes back to the host.
#pragma once

// The four waves' values of one entry -> the block's: levels kColLog, kColLog + 1 of the tree for a sum (m < 4), the
// minimum (m = 4) resp. maximum (m = 5) for a bound.
__device__ __forceinline__ double tracer_column_combine(int m, double a, double b, double c, double e) {
    if (m < 4) return column_combine(a, b, c, e);
    return m == 4 ? fmin(fmin(a, b), fmin(c, e)) : fmax(fmax(a, b), fmax(c, e));
}

// A wave's values of one tracer-layer (sum[], and at LEVEL 3 its bounds) -> LDS -> the block's partials.  One barrier per
// call; the buffer alternates with `it`, so a buffer is written again only behind the barrier that follows its readers.
template <int LEVEL>
__device__ __forceinline__ void tracer_column_out(const double (&sum)[LEVEL >= 2 ? 4 : 2], double mn, double mx,
                                                  double (*lds)[kColWaves][2 * LEVEL][64], int it, int k0, int wave, int lane,
                                                  double *out, int colpad) {
    constexpr int NS = LEVEL >= 2 ? 4 : 2, NQ = 2 * LEVEL;
    double (*buf)[NQ][64] = lds[it & 1];
#pragma unroll
    for (int e = 0; e < NS; ++e) buf[wave][e][lane] = sum[e];
    if constexpr (LEVEL >= 3) { buf[wave][4][lane] = mn; buf[wave][5][lane] = mx; }
    __syncthreads();
    for (int e = wave; e < NQ; e += kColWaves)
        out[(long long)(k0 + e) * colpad] = tracer_column_combine(e, buf[0][e][lane], buf[1][e][lane], buf[2][e][lane], buf[3][e][lane]);
}

// The interior form: every cell of the sub-block is wet interior inside the window (wave-uniform), the rows fully unrolled.
// hlay, h_u, h_v of the 8 rows are loaded once per layer and kept across the tracer loop.  Lane 0's W neighbours belong to
// another wave: lanes 0..7 load the W cell of lane 0's column in row `lane` and divide once for all 8 rows (the same array
// elements through trc_conc, hence the same bits as that cell's own c); row r reads lane r's value.
template <int LEVEL>
__device__ __forceinline__ void tracer_column_wave_interior(const ColumnRowsInterior &rows, const DevView &d, const double *q, int ntrc,
                                                            double (*lds)[kColWaves][2 * LEVEL][64], int wave, int lane, double *out, int colpad) {
    constexpr bool FACES = LEVEL >= 2;
    constexpr int NS = FACES ? 4 : 2, NQ = 2 * LEVEL;
    // The rows' places in vector registers, opaque: a row's offset is then added per load.  Folded into scalar bases per array
    // and row they are 64 scalar registers, more than there are.
    int ip[kColRows];
#pragma unroll
    for (int r = 0; r < kColRows; ++r) {
        ip[r] = rows.cell(r).ipnt;
        asm volatile("" : "+v"(ip[r]));
    }
    const int ipS = rows.cell(0).template nb<7>();                    // the row below the sub-block
    const int ipW = rows.cell(lane & (kColRows - 1)).template nb<5>() - lane;     // lane 0's W neighbour in row lane % 8
    int it = 0;
    for (int ilay = 1; ilay <= d.nlay; ++ilay) {
        double hP[kColRows], hW[kColRows], hu[kColRows], hv[kColRows], hS0 = 0.0, hWl = 0.0;
        if constexpr (FACES) { hS0 = LL(d.hlay, ipS, ilay); hWl = LL(d.hlay, ipW, ilay); }
#pragma unroll
        for (int r = 0; r < kColRows; ++r) {
            hP[r] = LL(d.hlay, ip[r], ilay);
            hW[r] = 0.0; hu[r] = 0.0; hv[r] = 0.0;
            if constexpr (FACES) {
                hu[r] = LL(d.h_u, ip[r], ilay); hv[r] = LL(d.h_v, ip[r], ilay);
                const double w0 = __shfl(hWl, r, 64);
                hW[r] = __shfl_up(hP[r], 1, 64);
                if (lane == 0) hW[r] = w0;
            }
        }
        for (int t = 0; t < ntrc; ++t, ++it) {
            ColumnTree<NS> tree;
            double sum[NS], mn = HUGE_VAL, mx = -HUGE_VAL;
            double hS = hS0, cS = 0.0, cWl = 0.0;
            if constexpr (FACES) { cS = trc_conc(TQ(q, ipS, ilay, t), hS0); cWl = trc_conc(TQ(q, ipW, ilay, t), hWl); }
#pragma unroll
            for (int r = 0; r < kColRows; ++r) {
                // (opaque per tracer: the comparisons on them are then formed where they are used.  Hoisted out of the
                // tracer loop they are four masks per row, two scalar registers each, more than there are.)
                asm volatile("" : "+v"(hP[r]));
                if constexpr (FACES) asm volatile("" : "+v"(hW[r]), "+v"(hu[r]), "+v"(hv[r]));
                const double xq = TQ(q, ip[r], ilay, t);
                const double xc = trc_conc(xq, hP[r]);
                double x[NS];
                x[0] = xq; x[1] = xq * xc;
                if constexpr (FACES) {
                    const double w0 = __shfl(cWl, r, 64);
                    double cW = __shfl_up(xc, 1, 64);
                    if (lane == 0) cW = w0;
                    x[2] = trc_face(hu[r], cW, hW[r], xc, hP[r]);
                    x[3] = trc_face(hv[r], cS, hS, xc, hP[r]);
                    hS = hP[r]; cS = xc;           // the next row's S: this row's own
                }
                if constexpr (LEVEL >= 3) {
                    const bool wet = hP[r] > 0.0;
                    const double xb = xc + 0.0;
                    mn = fmin(mn, wet ? xb : HUGE_VAL); mx = fmax(mx, wet ? xb : -HUGE_VAL);
                }
                tree.push(r, x, sum);
            }
            tracer_column_out<LEVEL>(sum, mn, mx, lds, it, (t * d.nlay + (ilay - 1)) * NQ, wave, lane, out, colpad);
        }
    }
}

// The general form (rim, land, the table path, sub-blocks the window cuts, embedded tiles that touch land): the row loop stays
// rolled, W and S are loaded directly, as in k_column_blocks and for the reasons written there.
template <int LEVEL, class ROWS>
__device__ __forceinline__ void tracer_column_wave_general(const ROWS &rows, const DevView &d, const double *q, int ntrc,
                                                           double (*lds)[kColWaves][2 * LEVEL][64], int wave, int lane, double *out, int colpad) {
    constexpr bool FACES = LEVEL >= 2;
    constexpr int NS = FACES ? 4 : 2, NQ = 2 * LEVEL;
    int it = 0;
    for (int ilay = 1; ilay <= d.nlay; ++ilay) {
        for (int t = 0; t < ntrc; ++t, ++it) {
            ColumnTree<NS> tree;
            double sum[NS], mn = HUGE_VAL, mx = -HUGE_VAL;
#pragma unroll 1
            for (int r = 0; r < kColRows; ++r) {
                const auto c = rows.cell(r);
                const bool live = rows.live(r, c);
                const double pad = rows.pad(r);
                int il = ilay, tt = t;               // (in vector registers: the offsets are then added per load, not kept as
                asm volatile("" : "+v"(il), "+v"(tt));      // scalar bases per array, as in column_layer)
                const int ipnt = c.ipnt;
                const double hP = LL(d.hlay, ipnt, il);
                const double xq = TQ(q, ipnt, il, tt);
                const double xc = trc_conc(xq, hP);
                double x[NS];
                x[0] = live ? xq : pad; x[1] = live ? xq * xc : pad;
                if constexpr (FACES) {
                    const int c5 = c.template nb<5>(), c7 = c.template nb<7>();
                    const double hW = LL(d.hlay, c5, il), hS = LL(d.hlay, c7, il);
                    const double huP = LL(d.h_u, ipnt, il), hvP = LL(d.h_v, ipnt, il);
                    const double cW = trc_conc(TQ(q, c5, il, tt), hW), cS = trc_conc(TQ(q, c7, il, tt), hS);
                    const double xfu = trc_face(huP, cW, hW, xc, hP), xfv = trc_face(hvP, cS, hS, xc, hP);
                    x[2] = live ? xfu : pad; x[3] = live ? xfv : pad;
                }
                if constexpr (LEVEL >= 3) {
                    const bool wet = live && hP > 0.0;
                    const double xb = xc + 0.0;
                    mn = fmin(mn, wet ? xb : HUGE_VAL); mx = fmax(mx, wet ? xb : -HUGE_VAL);
                }
                tree.push(r, x, sum);
            }
            tracer_column_out<LEVEL>(sum, mn, mx, lds, it, (t * d.nlay + (ilay - 1)) * NQ, wave, lane, out, colpad);
        }
    }
}

// k_column_blocks' grid and arguments, and the tracers' contents and count: grid (chunks of the batch, blocks of kColBlockRows
// rows); chunk0: the batch's first 64-column chunk; colpad = 64 * the chunks part[] is laid out for.  Every wave of a
// workgroup meets nlay * ntrc barriers, whatever its form.
template <bool DENSE, int LEVEL>
__global__ __launch_bounds__(BEOM_BLOCK) void k_tracer_column_blocks(DevView d, const double *q, int ntrc, int chunk0, int wlo, int whi,
                                                                     int M2, int xdup, int ydup, const int32_t *cellmap, double *part,
                                                                     int colpad) {
    constexpr int NQ = 2 * LEVEL;
    __shared__ double lds[2][kColWaves][NQ][64];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int blk = (int)blockIdx.y;
    const int i = (chunk0 + (int)blockIdx.x) * 64 + lane + 1;
    const int j0 = (blk * kColWaves + wave) * kColRows + 1;
    const long long cnt = (long long)ntrc * d.nlay * NQ;
    double *out = part + (long long)blk * cnt * colpad + ((int)blockIdx.x * 64 + lane);
    if constexpr (DENSE) {
        const int i0 = __builtin_amdgcn_readfirstlane(i - lane);
        // (no band keeps a tracer column series: local rows are global rows.  A sub-block the window cuts takes the general form.)
        bool interior = i0 >= 2 && i0 + 63 <= d.L - 2 && j0 >= 2 && j0 + kColRows - 1 <= d.M - 2 && j0 >= wlo && j0 + kColRows - 1 <= whi;
        if (interior && d.embedded) {          // (a sub-block = two 64 x 4 tiles of reg4, one above the other)
            const long long t4 = (long long)((j0 - 1) >> 2) * d.reg_nx + ((i0 - 1) >> 6);
            interior = d.reg4[t4] != 0 && d.reg4[t4 + d.reg_nx] != 0;
        }
        if (interior) tracer_column_wave_interior<LEVEL>(ColumnRowsInterior{&d, i, j0}, d, q, ntrc, lds, wave, lane, out, colpad);
        else tracer_column_wave_general<LEVEL>(ColumnRowsDense{&d, i, j0, wlo, whi, M2, xdup, ydup}, d, q, ntrc, lds, wave, lane, out, colpad);
    } else {
        tracer_column_wave_general<LEVEL>(ColumnRowsGather{&d, cellmap, i, j0, wlo, whi, M2, xdup, ydup}, d, q, ntrc, lds, wave, lane, out, colpad);
    }
}

// The block partials of a column and entry -> the record's slot.  Entries m < 4 (k % nq): the upper levels of the column's
// tree, walked exactly as k_column_finish walks them (nblkp2 = M2 / kColBlockRows, at least 1; blocks past nblk are the tree's
// padding, +0.0; groups of kColFinishGroup blocks where there are as many).  m = 4, 5: the minimum resp. maximum over the
// blocks (a block without a live wet cell holds +inf, -inf).  Grid (columns of the batch / 256, cnt).
template <int LEVELS>
__global__ __launch_bounds__(BEOM_BLOCK) void k_tracer_column_finish(const double *part, double *rec, int cnt, int nq, int colpad,
                                                                     int ncols, int nblk, int nblkp2) {
    const int col = (int)blockIdx.x * BEOM_BLOCK + (int)threadIdx.x, k = (int)blockIdx.y;
    if (col >= ncols) return;
    const double *p = part + (long long)k * colpad + col;
    const long long stride = (long long)cnt * colpad;
    const int m = k % nq;
    double v = 0.0;
    if (m >= 4) {
        v = m == 4 ? HUGE_VAL : -HUGE_VAL;
#pragma unroll 4
        for (int b = 0; b < nblk; ++b) {
            const double w = p[b * stride];
            v = m == 4 ? fmin(v, w) : fmax(v, w);
        }
        rec[(long long)col * cnt + k] = v;
        return;
    }
    double s[LEVELS];
    if (nblkp2 >= kColFinishGroup) {
        for (int g = 0; g < nblkp2 / kColFinishGroup; ++g) {
            double w[kColFinishGroup];
#pragma unroll
            for (int n = 0; n < kColFinishGroup; ++n) {
                const int b = g * kColFinishGroup + n;
                w[n] = b < nblk ? p[b * stride] : 0.0;
            }
#pragma unroll
            for (int n = kColFinishGroup; n > 1; n >>= 1)
#pragma unroll
                for (int a = 0; a < n / 2; ++a) w[a] = w[2 * a] + w[2 * a + 1];
            v = w[0];
            bool placed = false;
#pragma unroll
            for (int l = 0; l < LEVELS - kColFinishGroupLog; ++l) {
                if (placed) continue;
                if ((g >> l) & 1) v = s[l] + v;
                else { s[l] = v; placed = true; }
            }
        }
    } else {
        for (int b = 0; b < nblkp2; ++b) {
            v = b < nblk ? p[b * stride] : 0.0;
            bool placed = false;
#pragma unroll
            for (int l = 0; l < kColFinishGroupLog; ++l) {
                if (placed) continue;
                if ((b >> l) & 1) v = s[l] + v;
                else { s[l] = v; placed = true; }
            }
        }
    }
    rec[(long long)col * cnt + k] = v;      // (the last block closes every level: v is the root)
}
