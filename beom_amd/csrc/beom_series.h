// beom_series.h — a record of row sums per sampled step, kept on the device (no reference routine).  Include after
// beom_integrals.h.
//
// One record is rec[(j-1)*cnt + k] for the handle's rows j: the 4*nlay + 1 sums of beom_integral_rows in its layout and, at
// level 2 (cnt = 6*nlay + 1), per layer l the row sums of the stored transports
//                                tu[l] = sum_i h_u(i, j, l)   at 4*nlay + 1 + (l-1)
//                                tv[l] = sum_i h_v(i, j, l)   at 5*nlay + 1 + (l-1)
// with the integrals' live rule (+0.0 where there is no packed cell and on the duplicated column / row of a periodic frame)
// and the integrals' order of summation: the pairwise tree over the aligned column index.  Level 1 launches k_integral_rows
// itself; level 2 launches k_series_rows, whose first 4*nlay + 1 sums ARE body_integral's; k_integral_chunks finishes the rows
// of either straight into the record's slot.  No atomics, no workgroup waits for another, nothing comes back to the host.
#pragma once

// The tree for two sums at once (width >= 2), in 6 exchanges instead of 12: at level 0 the even lane of a pair keeps a and
// the odd one b, from there on every lane carries one sum.  Every addition has the operands of integral_wave_tree's (IEEE
// addition commutes).  Result: a in lane 0, b in lane 1.
__device__ __forceinline__ double integral_wave_tree2(double a, double b, int width, int lane) {
    const bool odd = lane & 1;
    double v = (odd ? b : a) + __shfl_xor(odd ? a : b, 1, 64);
#pragma unroll
    for (int s = 2; s < 64; s <<= 1)
        if (s < width) v = v + __shfl_xor(v, s, 64);
    return v;
}

// body_integral's sums, then the two transport sums of every layer: own-cell loads only (coalesced along the row)
template <class C>
__device__ __forceinline__ void body_series(const C &c, const DevView &d, bool live, double mkpi, int width, double *out) {
    body_integral(c, d, live, mkpi, width, out);
    const int ipnt = c.ipnt;
    const int lane = (int)threadIdx.x & 63;
    double *tu = out + 4 * d.nlay + 1, *tv = tu + d.nlay;
    for (int ilay = 1; ilay <= d.nlay; ++ilay) {
        const double hu = LL(d.h_u, ipnt, ilay), hv = LL(d.h_v, ipnt, ilay);
        const double t_u = live ? hu : 0.0, t_v = live ? hv : 0.0;
        if (width >= 2) {
            const double t = integral_wave_tree2(t_u, t_v, width, lane);
            if (lane < 2) (lane ? tv : tu)[ilay - 1] = t;
        } else if (lane == 0) {
            tu[ilay - 1] = t_u; tv[ilay - 1] = t_v;
        }
    }
}

// k_integral_rows' geometry and arguments; part[(r * nch + chunk) * count + k] with count = 6*nlay + 1
template <bool DENSE>
__global__ __launch_bounds__(BEOM_BLOCK) void k_series_rows(DevView d, int jlo, int nrows, int width, int xdup, int ydup,
                                                            const int32_t *cellmap, double *part) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.y * BEOM_TILE_Y + wave;
    if (r >= nrows) return;
    const int j = jlo + r, chunk = (int)blockIdx.x, i = chunk * 64 + lane + 1;
    const bool in = i <= d.L;
    const bool dup = (xdup && i == d.L) || (ydup && j + d.joff == d.Mg);
    double *out = part + ((long long)r * (int)gridDim.x + chunk) * (6 * d.nlay + 1);
    if constexpr (DENSE) {
        CellDense c;
        c.set_cell(d, in ? i : d.L, j);
        const bool live = in && !dup && slot_is_cell(d, c.ipnt);
        if (c.wave_is_interior()) body_series(c.as_interior(), d, live, 1.0, width, out);
        else body_series(c, d, live, d.embedded ? d.mkpi[c.ipnt] : 1.0, width, out);
    } else {
        CellGather c;
        c.ipnt = in ? cellmap[(long long)(j - 1) * d.L + (i - 1)] : 0;
        c.row = d.neig + 8ll * c.ipnt;
        c.dv = &d;
        body_series(c, d, c.ipnt != 0 && !dup, c.mkpi(), width, out);
    }
}
