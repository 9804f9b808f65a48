// beom_column_series.h — a record of column sums per sampled step, kept on the device (no reference routine).  Include after
// every other kernel header (the kernels before it keep their place in the code object).
//
// One record is cols[(i-1)*cnt + k] for the columns i = 1..L: the series' entries (beom_series.h: vol, ke, ens, circ per layer,
// eta2, at level 2 the stored transports h_u, h_v per layer) summed along the column instead of along the row, with the
// integrals' live rule and, outside the row window wlo..whi, +0.0.  Order of summation: the pairwise tree over the aligned
// global row index r = j-1, the column padded with +0.0 to M2 = the next power of two of M; the tree has log2(M2) levels and
// no more.  Where a block of rows reaches past M2 (a frame of fewer rows than a block), the rows past M2 hold -0.0, the
// identity of IEEE addition (x + -0.0 = x bit for bit, for -0.0 too): the block's further levels then change nothing.
//
// Stage 1, k_column_blocks: a wavefront owns 64 consecutive columns (a lane per column: every own-cell load is coalesced) and
// kColRows consecutive rows starting at a multiple of kColRows; a lane adds its terms in a streaming pairwise tree kept in
// registers (no cross-lane exchange), the waves of a workgroup combine through LDS in tree order, and one partial comes out per
// aligned block of kColBlockRows rows, entry and column: part[(block * cnt + k) * colpad + column].  Stage 2, k_column_finish:
// a thread per (column, entry) walks the block partials in tree order and writes the record's slot.  No atomics, no workgroup
// waits for another, nothing comes back to the host.
#pragma once

constexpr int kColLog = 3;                                 // a wavefront's sub-block: 2^3 rows
constexpr int kColRows = 1 << kColLog;
constexpr int kColWaves = BEOM_BLOCK / 64;                 // (four: two more levels of the tree in LDS)
constexpr int kColBlockRows = kColRows * kColWaves;

// The streaming pairwise tree of E sums over kColRows elements pushed in order: s[e][k] waits as the left operand of level k.
// Every index is static: where r is a constant of an unrolled row loop the conditions fold away, where the row loop is rolled
// they are wave-uniform.  LOG: the levels there are registers for; `levels` <= LOG: those in use (the maps' block edge is a
// run-time value, beom_maps.h), a constant LOG in the column series, where its test folds away.
template <int E, int LOG = kColLog>
struct ColumnTree {
    double s[E][LOG];
    // once the sub-block is complete (r = 2^levels - 1), sum[] holds its sums
    __device__ __forceinline__ void push(int r, const double (&t)[E], double (&sum)[E], int levels = LOG) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double v = t[e];
            bool placed = false, root = false;             // root: v has passed every level in use (stored once, below)
#pragma unroll
            for (int k = 0; k < LOG; ++k) {
                if (placed) continue;
                if (k >= levels) { root = true; placed = true; }
                else if ((r >> k) & 1) v = s[e][k] + v;
                else { s[e][k] = v; placed = true; }
            }
            if (root || !placed) sum[e] = v;
        }
    }
};

// The terms of one cell and layer: body_integral's statements (beom_integrals.h) and, at LEVEL 2, body_series' (beom_series.h),
// restated.  first: the sub-block's first row loads hS, hSW, uS; every later row takes them from the row below, which this
// lane has just finished (p_h0, p_hW, p_u0: its h0, hW, u0 — the same array elements, hence the same bits).  pad: what a
// position that is not live holds (+0.0; -0.0 in the rows past M2).  -> h0
template <int LEVEL, class C>
__device__ __forceinline__ double column_terms(const C &c, const DevView &d, bool live, double pad, double mkpi, int ilay, bool first,
                                               double &p_h0, double &p_hW, double &p_u0, double (&t)[LEVEL >= 2 ? 6 : 4]) {
    const int ipnt = c.ipnt;
    const int c5 = c.template nb<5>(), c6 = c.template nb<6>(), c7 = c.template nb<7>();
    const double mkn = c.mk_n(), mku = c.mk_u(), mkv = c.mk_v(), mkpe = c.mkpe();
    const double mk5 = c.template mk_n_nb<5>(c5), mk6 = c.template mk_n_nb<6>(c6), mk7 = c.template mk_n_nb<7>(c7);
    const double nm = mkn + mk5 + mk6 + mk7;
    const bool pv_on = live && mkpi > 0.5 && nm > 0.0;
    const double h0 = LL(d.hlay, ipnt, ilay), hW = LL(d.hlay, c5, ilay);
    const double u0 = LL(d.u, ipnt, ilay);
    const double v0 = LL(d.v, ipnt, ilay), vW = LL(d.v, c5, ilay);
    double hSW = p_hW, hS = p_h0, uS = p_u0;
    if (first) { hSW = LL(d.hlay, c6, ilay); hS = LL(d.hlay, c7, ilay); uS = LL(d.u, c7, ilay); }
    p_h0 = h0; p_hW = hW; p_u0 = u0;
    const double hcu = (hW + h0) / (1.0 + mku);
    const double hcv = (h0 + hS) / (1.0 + mkv);
    const double rv = (v0 - vW - u0 + uS) * d.i_dl * mkpe;
    const double have = h0 + hW + hSW + hS;
    const double pv = (d.fcor[ipnt] + rv * d.uadv) * mkpi * nm / have;
    t[0] = live ? mkn * h0 : pad;
    t[1] = live ? mku * ((u0 * u0) * hcu) + mkv * ((v0 * v0) * hcv) : pad;
    t[2] = pv_on ? 0.5 * (pv * pv) * (have / nm) : pad;
    t[3] = live ? rv : pad;
    if constexpr (LEVEL >= 2) {
        const double hu = LL(d.h_u, ipnt, ilay), hv = LL(d.h_v, ipnt, ilay);
        t[4] = live ? hu : pad;
        t[5] = live ? hv : pad;
    }
    return h0;
}

// A wavefront's sub-block of rows j0 .. j0 + kColRows - 1 in one of three forms.  cell(r): the context of row j0 + r (that of
// some valid slot where the row is past M or the lane past L), live(r, c): whether its term counts, pad(r), mkpi(c).
struct ColumnRowsInterior {        // every cell of the sub-block is wet interior with unit masks, inside the window (wave-uniform)
    const DevView *dv;
    int i, j0;
    __device__ __forceinline__ CellDenseT<true> cell(int r) const {
        CellDense c;
        c.set_cell(*dv, i, j0 + r);
        return c.as_interior();
    }
    __device__ __forceinline__ bool live(int, const CellDenseT<true> &) const { return true; }
    __device__ __forceinline__ double pad(int) const { return 0.0; }
    __device__ __forceinline__ double mkpi(const CellDenseT<true> &) const { return 1.0; }
};
struct ColumnRowsDense {           // dense and embedded handles: neighbours by offset, the masks of k_series_rows
    const DevView *dv;
    int i, j0, wlo, whi, M2, xdup, ydup;
    __device__ __forceinline__ CellDense cell(int r) const {
        // The cell's place is made opaque per row, in vector registers: its wraps and mask predicates are then formed where
        // they are used.  Hoisted out of the row and layer loops they are a dozen masks, two scalar registers each, more
        // than there are.
        int a = i <= dv->L ? i : dv->L;
        int b = j0 + r <= dv->M ? j0 + r : dv->M;
        asm volatile("" : "+v"(a), "+v"(b));
        CellDense c;
        c.set_cell(*dv, a, b);
        return c;
    }
    __device__ __forceinline__ bool live(int r, const CellDense &c) const {
        const int j = j0 + r;
        int a = i;
        asm volatile("" : "+v"(a));          // (as in cell)
        const bool dup = (xdup && a == dv->L) || (ydup && j == dv->M);
        return a <= dv->L && j <= dv->M && j >= wlo && j <= whi && !dup && slot_is_cell(*dv, c.ipnt);
    }
    __device__ __forceinline__ double pad(int r) const { return j0 + r > M2 ? -0.0 : 0.0; }
    __device__ __forceinline__ double mkpi(const CellDense &c) const { return dv->embedded ? dv->mkpi[c.ipnt] : 1.0; }
};
struct ColumnRowsGather {          // the table path: the packed cell of (i, j) from the cell map
    const DevView *dv;
    const int32_t *cellmap;
    int i, j0, wlo, whi, M2, xdup, ydup;
    __device__ __forceinline__ CellGather cell(int r) const {
        CellGather c;
        c.ipnt = i <= dv->L && j0 + r <= dv->M ? cellmap[(long long)(j0 + r - 1) * dv->L + (i - 1)] : 0;
        c.row = dv->neig + 8ll * c.ipnt;
        c.dv = dv;
        return c;
    }
    __device__ __forceinline__ bool live(int r, const CellGather &c) const {
        const int j = j0 + r;
        const bool dup = (xdup && i == dv->L) || (ydup && j == dv->M);
        return c.ipnt != 0 && j >= wlo && j <= whi && !dup;
    }
    __device__ __forceinline__ double pad(int r) const { return j0 + r > M2 ? -0.0 : 0.0; }
    __device__ __forceinline__ double mkpi(const CellGather &c) const { return c.mkpi(); }
};

// One layer of a sub-block -> its sums.  UNROLLED: the rows fully unrolled, every index a constant, hcol[r] carried from layer
// to layer by the caller (the interior form, the hot one).  Otherwise the row loop stays rolled, so that the rows' set-up
// (wraps, masks, table look-ups) is not kept in registers for all rows across the layer loop; r is then wave-uniform and
// hcol is left alone (column_eta2 adds the thicknesses again, in the same order).
template <int LEVEL, bool UNROLLED, class ROWS>
__device__ __forceinline__ void column_layer(const ROWS &rows, const DevView &d, int ilay, double (&hcol)[kColRows],
                                             double (&sum)[LEVEL >= 2 ? 6 : 4]) {
    constexpr int E = LEVEL >= 2 ? 6 : 4;
    ColumnTree<E> tree;
    double p_h0 = 0.0, p_hW = 0.0, p_u0 = 0.0;
    if constexpr (UNROLLED) {
#pragma unroll
        for (int r = 0; r < kColRows; ++r) {
            const auto c = rows.cell(r);
            double t[E];
            hcol[r] = hcol[r] + column_terms<LEVEL>(c, d, rows.live(r, c), rows.pad(r), rows.mkpi(c), ilay, r == 0, p_h0, p_hW, p_u0, t);
            tree.push(r, t, sum);
        }
    } else {
#pragma unroll 1
        for (int r = 0; r < kColRows; ++r) {
            const auto c = rows.cell(r);
            double t[E];
            int il = ilay;                       // (in a vector register: the layer's offset is then added per load, not kept
            asm volatile("" : "+v"(il));         // as a scalar base per array, which this form has no registers for)
            column_terms<LEVEL>(c, d, rows.live(r, c), rows.pad(r), rows.mkpi(c), il, r == 0, p_h0, p_hW, p_u0, t);
            tree.push(r, t, sum);
        }
    }
}
// the eta2 terms of a sub-block through the same tree
template <bool UNROLLED, class ROWS>
__device__ __forceinline__ double column_eta2(const ROWS &rows, const DevView &d, const double (&hcol)[kColRows]) {
    ColumnTree<1> tree;
    double sum[1] = {0.0};
    if constexpr (UNROLLED) {
#pragma unroll
        for (int r = 0; r < kColRows; ++r) {
            const auto c = rows.cell(r);
            const double eta = hcol[r] - d.h_th[c.ipnt];
            const double t[1] = {rows.live(r, c) ? c.mk_n() * (eta * eta) : rows.pad(r)};
            tree.push(r, t, sum);
        }
    } else {
#pragma unroll 1
        for (int r = 0; r < kColRows; ++r) {
            const auto c = rows.cell(r);
            double hc = 0.0;
            for (int ilay = 1; ilay <= d.nlay; ++ilay) hc = hc + LL(d.hlay, c.ipnt, ilay);
            const double eta = hc - d.h_th[c.ipnt];
            const double t[1] = {rows.live(r, c) ? c.mk_n() * (eta * eta) : rows.pad(r)};
            tree.push(r, t, sum);
        }
    }
    return sum[0];
}

// levels kColLog and kColLog + 1 of the tree: the four waves' sums of one entry, in row order
__device__ __forceinline__ double column_combine(double a, double b, double c, double e) { return (a + b) + (c + e); }

// A wavefront's part of k_column_blocks in one form of rows: all layers, then eta2.  Every wave of a workgroup runs all layers
// (rows past M count +0.0, rows past M2 -0.0): there is one barrier per layer and one for eta2, the LDS buffer alternating, so a
// buffer is written again only behind the barrier that follows its readers.  The waves of a workgroup may run different forms:
// each meets the same number of barriers.  (One layer loop per form, not one loop with the choice inside: the forms' loop
// invariants would otherwise all be live at once, more scalar registers than there are.)
template <int LEVEL, bool UNROLLED, class ROWS>
__device__ __forceinline__ void column_wave(const ROWS &rows, const DevView &d, double (*lds)[kColWaves][LEVEL >= 2 ? 6 : 4][64],
                                            int wave, int lane, double *out, int colpad) {
    constexpr int E = LEVEL >= 2 ? 6 : 4;
    double hcol[kColRows];
#pragma unroll
    for (int r = 0; r < kColRows; ++r) hcol[r] = 0.0;
    for (int ilay = 1; ilay <= d.nlay; ++ilay) {
        double sum[E];
        column_layer<LEVEL, UNROLLED>(rows, d, ilay, hcol, sum);
        double (*buf)[E][64] = lds[ilay & 1];
#pragma unroll
        for (int e = 0; e < E; ++e) buf[wave][e][lane] = sum[e];
        __syncthreads();
        for (int e = wave; e < E; e += kColWaves) {
            const int k = e < 4 ? 4 * (ilay - 1) + e : e * d.nlay + 1 + (ilay - 1);      // (e = 4: tu at 4*nlay + 1, e = 5: tv)
            out[(long long)k * colpad] = column_combine(buf[0][e][lane], buf[1][e][lane], buf[2][e][lane], buf[3][e][lane]);
        }
    }
    const double eta2 = column_eta2<UNROLLED>(rows, d, hcol);
    double (*buf)[E][64] = lds[(d.nlay + 1) & 1];
    buf[wave][0][lane] = eta2;
    __syncthreads();
    if (wave == 0) out[(long long)(4 * d.nlay) * colpad] = column_combine(buf[0][0][lane], buf[1][0][lane], buf[2][0][lane], buf[3][0][lane]);
}

// Grid (chunks of the batch, blocks of kColBlockRows rows); chunk0: the batch's first 64-column chunk; colpad = 64 * the
// chunks part[] is laid out for.
template <bool DENSE, int LEVEL>
__global__ __launch_bounds__(BEOM_BLOCK) void k_column_blocks(DevView d, int chunk0, int wlo, int whi, int M2, int xdup, int ydup,
                                                              const int32_t *cellmap, double *part, int colpad) {
    constexpr int E = LEVEL >= 2 ? 6 : 4;
    __shared__ double lds[2][kColWaves][E][64];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int blk = (int)blockIdx.y;
    const int i = (chunk0 + (int)blockIdx.x) * 64 + lane + 1;
    const int j0 = (blk * kColWaves + wave) * kColRows + 1;
    const int cnt = (LEVEL >= 2 ? 6 : 4) * d.nlay + 1;
    double *out = part + (long long)blk * cnt * colpad + ((int)blockIdx.x * 64 + lane);
    if constexpr (DENSE) {
        const int i0 = __builtin_amdgcn_readfirstlane(i - lane);
        // (no band keeps a column series: local rows are global rows.  A sub-block the window cuts takes the general form.)
        bool interior = i0 >= 2 && i0 + 63 <= d.L - 2 && j0 >= 2 && j0 + kColRows - 1 <= d.M - 2 && j0 >= wlo && j0 + kColRows - 1 <= whi;
        if (interior && d.embedded) {          // (a sub-block = two 64 x 4 tiles of reg4, one above the other)
            const long long t4 = (long long)((j0 - 1) >> 2) * d.reg_nx + ((i0 - 1) >> 6);
            interior = d.reg4[t4] != 0 && d.reg4[t4 + d.reg_nx] != 0;
        }
        if (interior) column_wave<LEVEL, true>(ColumnRowsInterior{&d, i, j0}, d, lds, wave, lane, out, colpad);
        else column_wave<LEVEL, false>(ColumnRowsDense{&d, i, j0, wlo, whi, M2, xdup, ydup}, d, lds, wave, lane, out, colpad);
    } else {
        column_wave<LEVEL, false>(ColumnRowsGather{&d, cellmap, i, j0, wlo, whi, M2, xdup, ydup}, d, lds, wave, lane, out, colpad);
    }
}

// The block partials of a column and entry -> the record's slot: the upper levels of the column's tree, walked in order with a
// streaming tree of static registers (nblkp2 = M2 / kColBlockRows, at least 1: every addition here is one of the column's own
// tree; blocks past nblk are its padding, +0.0).  Grid (columns of the batch / 256, cnt); the loads are coalesced over columns.
// Where there are at least kColFinishGroup blocks they are taken a group at a time: its loads are issued together (one by one,
// each waiting for the last, a column of 128 blocks took 0.25 ms), its aligned sub-tree is added in registers, and the
// streaming tree continues above it.  (A template only to be emitted behind the kernels that were there before it.)
constexpr int kColFinishLevels = 24, kColFinishGroupLog = 4, kColFinishGroup = 1 << kColFinishGroupLog;
template <int LEVELS>
__global__ __launch_bounds__(BEOM_BLOCK) void k_column_finish(const double *part, double *rec, int cnt, int colpad, int ncols,
                                                              int nblk, int nblkp2) {
    const int col = (int)blockIdx.x * BEOM_BLOCK + (int)threadIdx.x, k = (int)blockIdx.y;
    if (col >= ncols) return;
    const double *p = part + (long long)k * colpad + col;
    const long long stride = (long long)cnt * colpad;
    double s[LEVELS];
    double v = 0.0;
    if (nblkp2 >= kColFinishGroup) {
        for (int g = 0; g < nblkp2 / kColFinishGroup; ++g) {
            double w[kColFinishGroup];
#pragma unroll
            for (int q = 0; q < kColFinishGroup; ++q) {
                const int b = g * kColFinishGroup + q;
                w[q] = b < nblk ? p[b * stride] : 0.0;
            }
#pragma unroll
            for (int n = kColFinishGroup; n > 1; n >>= 1)
#pragma unroll
                for (int m = 0; m < n / 2; ++m) w[m] = w[2 * m] + w[2 * m + 1];
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
