// beom_integrals.h — conservation integrals of the state between two steps (no reference routine: the reference's one
// quantitative test case reads the output files back, testcases/conservation.m:116-211).  Include after beom_kernels.h.
//
// Per layer l the sums of        vol  = mk_n * h
//                                ke   = mk_u * ((u*u) * hcu) + mk_v * ((v*v) * hcv)     hcu, hcv: private_mod.f95:1438, 1521
//                                ens  = 0.5 * (pvor*pvor) * (have / nm)  where mkpi > 0.5 and nm > 0, else +0   (:2421-2433)
//                                circ = rvor                                                                   (:2388-2389)
// and per column                 eta2 = mk_n * (eta*eta),  eta = hcol - h_th                                    (:2367-2373)
// rvor, pvor are what update_mont_rvor_pvor_dive_kine would store for THIS state (body_update_mont's statements).
//
// Order of summation (the contract): the terms sit on the rectangle c = i-1, r = j-1, +0.0 where there is no packed cell and
// on the duplicated column / row of a periodic frame; a row is summed by the pairwise tree over the aligned column index
// (level k+1 adds elements 2m and 2m+1 of level k; the row padded with +0.0 to the next power of two), the row sums by the
// same tree over rows (beom_integral_combine, on the host).  A wavefront's butterfly (__shfl_xor by 1, 2, ..., 32) over 64
// consecutive columns starting at a multiple of 64 IS the bottom six levels of that tree, and the 64-column chunks of a row
// combine by the same rule (k_integral_chunks) — so the bits do not depend on the handle kind, nor on who owns a row.
#pragma once

// bottom levels of the tree inside a wavefront; width = min(64, row padded to a power of two) (wave-uniform)
__device__ __forceinline__ double integral_wave_tree(double v, int width) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1)
        if (s < width) v = v + __shfl_xor(v, s, 64);
    return v;
}

// The same tree for the four sums of a layer at once (width >= 4), in 7 exchanges instead of 24: a sum of two lanes is
// needed in one of them only, so at level 0 the even lane of a pair keeps (a, b) and the odd one (c, d), at level 1 the lower
// pair of lanes keeps the first of its two, and from there on every lane carries one sum.  Every addition has the operands
// of integral_wave_tree's (IEEE addition commutes).  Result: a in lane 0, c in lane 1, b in lane 2, d in lane 3.
__device__ __forceinline__ double integral_wave_tree4(double a, double b, double c, double d, int width, int lane) {
    const bool odd = lane & 1, up = lane & 2;
    double k0 = odd ? c : a, k1 = odd ? d : b;
    k0 = k0 + __shfl_xor(odd ? a : c, 1, 64);
    k1 = k1 + __shfl_xor(odd ? b : d, 1, 64);
    double v = (up ? k1 : k0) + __shfl_xor(up ? k0 : k1, 2, 64);
#pragma unroll
    for (int s = 4; s < 64; s <<= 1)
        if (s < width) v = v + __shfl_xor(v, s, 64);
    return v;
}

// one wavefront = 64 consecutive columns of one row; every lane walks the layers of its cell.  live = false: the lane's
// position holds +0.0 (no cell there, or the duplicated column / row); its context is that of some valid slot.
template <class C>
__device__ __forceinline__ void body_integral(const C &c, const DevView &d, bool live, double mkpi, int width, double *out) {
    const int ipnt = c.ipnt;
    const int c5 = c.template nb<5>(), c6 = c.template nb<6>(), c7 = c.template nb<7>();
    const double mkn = c.mk_n(), mku = c.mk_u(), mkv = c.mk_v(), mkpe = c.mkpe();
    const double mk5 = c.template mk_n_nb<5>(c5), mk6 = c.template mk_n_nb<6>(c6), mk7 = c.template mk_n_nb<7>(c7);
    const double fcor = d.fcor[ipnt], h_th = d.h_th[ipnt];
    const double nm = mkn + mk5 + mk6 + mk7;
    const bool pv_on = live && mkpi > 0.5 && nm > 0.0;
    const int lane = (int)threadIdx.x & 63;
    const bool lane0 = lane == 0;
    double hcol = 0.0;
    for (int ilay = 1; ilay <= d.nlay; ++ilay) {
        const double h0 = LL(d.hlay, ipnt, ilay), hW = LL(d.hlay, c5, ilay), hSW = LL(d.hlay, c6, ilay), hS = LL(d.hlay, c7, ilay);
        const double u0 = LL(d.u, ipnt, ilay), uS = LL(d.u, c7, ilay);
        const double v0 = LL(d.v, ipnt, ilay), vW = LL(d.v, c5, ilay);
        hcol = hcol + h0;
        const double hcu = (hW + h0) / (1.0 + mku);
        const double hcv = (h0 + hS) / (1.0 + mkv);
        const double rv = (v0 - vW - u0 + uS) * d.i_dl * mkpe;
        const double have = h0 + hW + hSW + hS;
        const double pv = (fcor + rv * d.uadv) * mkpi * nm / have;
        double t_vol = mkn * h0;
        double t_ke = mku * ((u0 * u0) * hcu) + mkv * ((v0 * v0) * hcv);
        double t_ens = pv_on ? 0.5 * (pv * pv) * (have / nm) : 0.0;
        double t_circ = rv;
        if (!live) { t_vol = 0.0; t_ke = 0.0; t_circ = 0.0; }
        double *o = out + 4 * (ilay - 1);
        if (width >= 4) {
            const double t = integral_wave_tree4(t_vol, t_ke, t_ens, t_circ, width, lane);
            if (lane < 4) o[((lane & 1) << 1) | (lane >> 1)] = t;      // lanes 0, 1, 2, 3 hold vol, ens, ke, circ
        } else {
            t_vol = integral_wave_tree(t_vol, width);
            t_ke = integral_wave_tree(t_ke, width);
            t_ens = integral_wave_tree(t_ens, width);
            t_circ = integral_wave_tree(t_circ, width);
            if (lane0) { o[0] = t_vol; o[1] = t_ke; o[2] = t_ens; o[3] = t_circ; }
        }
    }
    const double eta = hcol - h_th;
    double t_eta2 = live ? mkn * (eta * eta) : 0.0;
    t_eta2 = integral_wave_tree(t_eta2, width);
    if (lane0) out[4 * d.nlay] = t_eta2;
}

// Chunk sums of local rows jlo .. jlo+nrows-1: part[(r * nch + chunk) * count + k], count = 4*nlay + 1, nch = gridDim.x.
// A workgroup = the same chunk of four consecutive rows (the S rows a wave reads were just touched by its sibling).
// DENSE: dense and embedded handles, neighbours by offset (CellDense).  Otherwise the packed cell of (i, j) comes from
// cellmap[(j-1)*L + (i-1)] (0 = no cell there) and its neighbours and masks from the caller's tables (CellGather), so a
// cell's term lands on its own column whatever gaps the row has.
template <bool DENSE>
__global__ __launch_bounds__(BEOM_BLOCK) void k_integral_rows(DevView d, int jlo, int nrows, int width, int xdup, int ydup,
                                                              const int32_t *cellmap, double *part) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.y * BEOM_TILE_Y + wave;
    if (r >= nrows) return;
    const int j = jlo + r, chunk = (int)blockIdx.x, i = chunk * 64 + lane + 1;
    const bool in = i <= d.L;
    const bool dup = (xdup && i == d.L) || (ydup && j + d.joff == d.Mg);
    double *out = part + ((long long)r * (int)gridDim.x + chunk) * (4 * d.nlay + 1);
    if constexpr (DENSE) {
        CellDense c;
        c.set_cell(d, in ? i : d.L, j);
        const bool live = in && !dup && slot_is_cell(d, c.ipnt);
        if (c.wave_is_interior()) body_integral(c.as_interior(), d, live, 1.0, width, out);
        else body_integral(c, d, live, d.embedded ? d.mkpi[c.ipnt] : 1.0, width, out);
    } else {
        CellGather c;
        c.ipnt = in ? cellmap[(long long)(j - 1) * d.L + (i - 1)] : 0;
        c.row = d.neig + 8ll * c.ipnt;
        c.dv = &d;
        body_integral(c, d, c.ipnt != 0 && !dup, c.mkpi(), width, out);
    }
}

// The chunks of a row -> its row sum, the upper levels of the row's tree: one wavefront per row, a lane per chunk (+0.0
// past the row's last chunk: the padding), the butterfly again; rows of more than 64 chunks go group by group of 64 aligned
// chunks and lane 0 finishes the tree over the groups in LDS (ngroups a power of two, <= kIntegralMaxGroups).
constexpr int kIntegralMaxGroups = 256;
__global__ __launch_bounds__(64) void k_integral_chunks(const double *part, double *rows, int count, int nch, int nchp2) {
    __shared__ double grp[kIntegralMaxGroups];
    const int lane = (int)threadIdx.x;
    const long long r = blockIdx.x;
    const double *p = part + r * nch * count;
    const int width = nchp2 < 64 ? nchp2 : 64, ngroups = nchp2 < 64 ? 1 : nchp2 / 64;
    for (int k = 0; k < count; ++k) {
        double v = 0.0;
        for (int g = 0; g < ngroups; ++g) {
            const int c = g * 64 + lane;
            v = c < nch ? p[(long long)c * count + k] : 0.0;
            v = integral_wave_tree(v, width);
            if (ngroups > 1 && lane == 0) grp[g] = v;
        }
        if (lane == 0) {
            if (ngroups > 1) {
                for (int n = ngroups; n > 1; n >>= 1)
                    for (int m = 0; m < n / 2; ++m) grp[m] = grp[2 * m] + grp[2 * m + 1];
                v = grp[0];
            }
            rows[r * count + k] = v;
        }
    }
}

// Table-path handles: where on the rectangle each packed cell sits (subc; a slab's rows are global rows joff+1 ...), and
// whether the frame wraps (encoded only in neig, private_mod.f95:614-685: a cell of column 1 with a W neighbour, a cell of
// global row 1 with an S neighbour).  flags[0] = periodic in x, flags[1] = periodic in y (plain stores of the same value).
__global__ __launch_bounds__(BEOM_BLOCK) void k_integral_cellmap(DevView d, int32_t *cellmap, int32_t *flags) {
    const long long ipnt = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x + 1;
    if (ipnt > d.ndeg) return;
    const int i = d.subc[ipnt], jg = d.subc[ipnt + d.n1], j = jg - d.joff;
    if (i >= 1 && i <= d.L && j >= 1 && j <= d.M) cellmap[(long long)(j - 1) * d.L + (i - 1)] = (int32_t)ipnt;
    if (i == 1 && d.neig[8 * ipnt + 4] != 0) flags[0] = 1;
    if (jg == 1 && d.neig[8 * ipnt + 6] != 0) flags[1] = 1;
}
