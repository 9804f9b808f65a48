// beom_dense_host.h — host-side closed forms of the dense frame: the
// connectivity table and the five masks index_grid_points builds (private_mod.f95:567-764) for a
// frame whose interior is entirely wet, generalised to a window of rows of a taller frame
// (a j-slab).  Used to VERIFY a caller's tables (beom_create) and to GENERATE the tables of the
// row bands the multi-GPU driver cuts (beom_multi.hip).
// Further down: the host-only plans that beom_create and beom_set_rigid_lid upload (device layout,
// wave table, nudging tiles, the lid's Gauss-Seidel schedule).  They make no HIP call.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/beom_hip.h"

namespace beom_dense {

struct HostNb {   // host twin of CellDenseT::at (beom_dev.h): wraps act on the TARGET coordinate
    int L, M, xper, ywrap;
    int at(int a, int b) const {
        if (xper) { if (a == 0) a = L - 1; else if (a == L) a = 1; }
        if (ywrap) { if (b == 0) b = M - 1; else if (b == M) b = 1; }
        return (a >= 1 && a <= L && b >= 1 && b <= M) ? (a + (b - 1) * L) : 0;
    }
};

// slots 1..8 = E NE N NW W SW S SE (private_mod.f95:28-30)
static const int kDi[8] = {1, 1, 0, -1, -1, -1, 0, 1};
static const int kDj[8] = {0, 1, 1, 1, 0, -1, -1, -1};

// mask predicates of private_mod.f95:701-714 (+ :621,627,649,655,676 when periodic) at column i
// of global row jg in a frame of Mg rows
struct Masks { double n, u, v, pe, pi; };
inline Masks masks_at(int i, int jg, int L, int Mg, int xper, int yper) {
    const bool in = i <= L - 1 && jg <= Mg - 1;
    Masks m;
    m.n = in ? 1.0 : 0.0;
    m.u = (in && (i >= 2 || xper)) ? 1.0 : 0.0;
    m.v = (in && (jg >= 2 || yper)) ? 1.0 : 0.0;
    m.pe = (in && (i >= 2 || xper) && (jg >= 2 || yper)) ? 1.0 : 0.0;
    m.pi = 1.0;
    return m;
}

// Local rows 1..M are global rows joff+1..joff+M of an Mg-row frame.  Neighbours are local
// indices (0 outside the window); masks and subc(:,2) are those of the global frame.  A slab
// never wraps in y by itself (a y-periodic frame cut into bands gets its wrap from the exchange).
inline bool verify(int L, int M, int joff, int Mg, int slab, int xper, int yper, long long ndeg,
                   const int32_t *neig, const int32_t *subc, const double *mk_u, const double *mk_v,
                   const double *mk_n, const double *mkpe, const double *mkpi) {
    if (ndeg != (long long)L * M) return false;
    const HostNb nb{L, M, xper, (yper && !slab) ? 1 : 0};
    const long long n1 = ndeg + 1;
    for (int j = 1; j <= M; ++j) {
        const int jg = j + joff;
        for (int i = 1; i <= L; ++i) {
            const long long ip = i + (long long)(j - 1) * L;
            if (subc[ip] != i || subc[ip + n1] != jg) return false;
            for (int k = 0; k < 8; ++k)
                if (neig[k + 8 * ip] != nb.at(i + kDi[k], j + kDj[k])) return false;
            const Masks m = masks_at(i, jg, L, Mg, xper, yper);
            if (mk_n[ip] != m.n || mk_u[ip] != m.u || mk_v[ip] != m.v || mkpe[ip] != m.pe || mkpi[ip] != m.pi) return false;
        }
    }
    return true;
}

struct Tables {
    std::vector<int32_t> neig, subc;
    std::vector<double> mk_u, mk_v, mk_n, mkpe, mkpi;
};
// the tables verify() accepts, sentinel entries (index 0) zero
inline Tables generate(int L, int M, int joff, int Mg, int slab, int xper, int yper) {
    Tables t;
    const size_t n1 = (size_t)L * M + 1;
    t.neig.assign(8 * n1, 0); t.subc.assign(2 * n1, 0);
    t.mk_u.assign(n1, 0.0); t.mk_v.assign(n1, 0.0); t.mk_n.assign(n1, 0.0); t.mkpe.assign(n1, 0.0); t.mkpi.assign(n1, 0.0);
    const HostNb nb{L, M, xper, (yper && !slab) ? 1 : 0};
    for (int j = 1; j <= M; ++j) {
        const int jg = j + joff;
        for (int i = 1; i <= L; ++i) {
            const size_t ip = (size_t)i + (size_t)(j - 1) * L;
            t.subc[ip] = i; t.subc[ip + n1] = jg;
            for (int k = 0; k < 8; ++k) t.neig[k + 8 * ip] = nb.at(i + kDi[k], j + kDj[k]);
            const Masks m = masks_at(i, jg, L, Mg, xper, yper);
            t.mk_n[ip] = m.n; t.mk_u[ip] = m.u; t.mk_v[ip] = m.v; t.mkpe[ip] = m.pe; t.mkpi[ip] = m.pi;
        }
    }
    return t;
}

// ---- plans of beom_create and beom_set_rigid_lid ------------------------------------------

// the caller's connectivity and masks, as beom_create receives them
struct Grid { const int32_t *neig, *subc; const double *mk_u, *mk_v, *mk_n, *mkpe, *mkpi; };

inline int padded_pitch(int L) { return (L + 15) / 16 * 16; }

// Where the packed cells live on the device.  Dense handles (the closed form above, or the same rectangle with land on it:
// "embedded") keep a padded row pitch P (DevView::P); every other handle keeps the caller's packed layout (P = 0).
struct Layout {
    bool dense = false, embedded = false;      // (embedded handles are dense handles too)
    int xper = 0, yper = 0;                    // periodicity, encoded only in neig (private_mod.f95:614-685)
    int P = 0;
    std::vector<int32_t> slot_of, pk_of;       // embedded: packed index -> slot, slot -> packed index (0 = not a packed cell)
    std::vector<unsigned char> reg4;           // embedded: per 64 x 4 tile, 1 = every cell within 3 of it is wet interior with unit masks
    int reg_nx = 0;                            // tiles per row of reg4
    std::vector<int32_t> dev_index;            // packed index -> device index, for tables uploaded later (empty if none will be)
};

// Frames with land: the same rectangle, every packed cell in the slot of its (i, j) (subc), if the caller's
// connectivity is what offsets on the rectangle give — wraps as for a dense frame, and wherever the table says 0 the
// offset lands outside the rectangle or on a slot that is no packed cell (it then holds the sentinel's values).
inline bool embed(Layout &lay, int L, int M, int slab, long long ndeg, const Grid &g) {
    const size_t n1h = (size_t)ndeg + 1;
    const int P = padded_pitch(L);
    lay.slot_of.assign(n1h, 0); lay.pk_of.assign((size_t)P * M + 1, 0);
    for (size_t p = 1; p < n1h; ++p) {
        const int i = g.subc[p], j = g.subc[p + n1h];
        if (i < 1 || i > L || j < 1 || j > M) return false;
        const int32_t sl = (int32_t)(i + (long long)(j - 1) * P);
        if (lay.pk_of[sl]) return false;
        lay.slot_of[p] = sl; lay.pk_of[sl] = (int32_t)p;
    }
    for (int xp = 0; xp < 2; ++xp)
        for (int yp = 0; yp < 2; ++yp) {
            if (slab && yp) continue;
            const HostNb nb{L, M, xp, yp};
            bool match = true;
            for (size_t p = 1; p < n1h && match; ++p) {
                const int i = g.subc[p], j = g.subc[p + n1h];
                for (int k = 0; k < 8 && match; ++k) {
                    const int q = nb.at(i + kDi[k], j + kDj[k]);      // packed-pitch index on the L x M rectangle, or 0
                    const int32_t want = g.neig[k + 8 * p];
                    const int32_t got = q ? lay.pk_of[(size_t)((q - 1) % L + 1) + (size_t)((q - 1) / L) * P] : 0;
                    match = want == got;
                }
            }
            if (match) { lay.xper = xp; lay.yper = yp; return true; }
        }
    return false;
}

// 64 x 4 tiles whose every cell, and every cell within 3 of it, is wet interior with unit masks (reg4)
inline std::vector<unsigned char> regular_tiles(int L, int M, long long ndeg, const Grid &g) {
    const size_t n1h = (size_t)ndeg + 1;
    const int ntx = (L + 63) / 64, nty = (M + 3) / 4;
    std::vector<unsigned char> good((size_t)(L + 2) * (M + 2), 0);       // (i, j) in 0..L+1 x 0..M+1
    for (size_t p = 1; p < n1h; ++p)
        if (g.mk_n[p] == 1.0 && g.mk_u[p] == 1.0 && g.mk_v[p] == 1.0 && g.mkpe[p] == 1.0 && g.mkpi[p] == 1.0)
            good[(size_t)g.subc[p] + (size_t)g.subc[p + n1h] * (L + 2)] = 1;
    // 2-D prefix sums of "not good" -> any bad cell in a window
    std::vector<int32_t> bad((size_t)(L + 3) * (M + 3), 0);
    for (int j = 0; j <= M + 1; ++j)
        for (int i = 0; i <= L + 1; ++i)
            bad[(size_t)(i + 1) + (size_t)(j + 1) * (L + 3)] = (good[(size_t)i + (size_t)j * (L + 2)] ? 0 : 1)
                + bad[(size_t)i + (size_t)(j + 1) * (L + 3)] + bad[(size_t)(i + 1) + (size_t)j * (L + 3)] - bad[(size_t)i + (size_t)j * (L + 3)];
    auto any_bad = [&](int i0, int i1, int j0, int j1) {          // inclusive window, clipped to 0..L+1 x 0..M+1 (the margin is bad)
        if (i0 < 0 || j0 < 0 || i1 > L + 1 || j1 > M + 1) return true;
        return bad[(size_t)(i1 + 1) + (size_t)(j1 + 1) * (L + 3)] - bad[(size_t)i0 + (size_t)(j1 + 1) * (L + 3)]
               - bad[(size_t)(i1 + 1) + (size_t)j0 * (L + 3)] + bad[(size_t)i0 + (size_t)j0 * (L + 3)] != 0;
    };
    std::vector<unsigned char> reg4((size_t)ntx * nty, 0);
    for (int ty = 0; ty < nty; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            const int x0 = tx * 64 + 1, y0 = ty * 4 + 1;
            reg4[(size_t)ty * ntx + tx] = any_bad(x0 - 3, x0 + 63 + 3, y0 - 3, y0 + 3 + 3) ? 0 : 1;
        }
    return reg4;
}

// The layout of a handle whose local rows 1..M are global rows joff+1..joff+M of an Mg-row frame (slab: a band)
inline Layout plan_layout(const beom_params &prm, int L, int M, int joff, int Mg, int slab, const Grid &g) {
    Layout lay;
    if (prm.dense_hint && (long long)prm.ndeg == (long long)L * M)
        for (int xp = 0; xp < 2 && !lay.dense; ++xp)
            for (int yp = 0; yp < 2 && !lay.dense; ++yp) {
                if (slab && yp) continue;      // a slab of a y-periodic frame gets its wrap from the exchange, not from neig
                if (verify(L, M, joff, Mg, slab, xp, yp, prm.ndeg, g.neig, g.subc, g.mk_u, g.mk_v, g.mk_n, g.mkpe, g.mkpi)) {
                    lay.dense = true; lay.xper = xp; lay.yper = yp;
                }
            }
    if (!lay.dense && prm.dense_hint &&      // (a band of a frame with land too: slab)
        (long long)L * M < 2000000000ll && (long long)prm.ndeg * 10 >= (long long)L * M * 3 &&     // (at least 30 % of the rectangle in use)
        embed(lay, L, M, slab, prm.ndeg, g)) {
        lay.embedded = lay.dense = true;      // the dense kernels, with masks from arrays where a tile is not regular
        lay.reg4 = regular_tiles(L, M, prm.ndeg, g);
        lay.reg_nx = (L + 63) / 64;
    }
    if (lay.dense) lay.P = padded_pitch(L);
    if (prm.rgld > 0.5 || (lay.embedded && prm.flag_nudging && prm.mcbc < 0.5)) {      // the lid's tables, open-boundary segments
        const size_t n1h = (size_t)prm.ndeg + 1;
        lay.dev_index.assign(n1h, 0);
        for (size_t p = 1; p < n1h; ++p)
            lay.dev_index[p] = lay.embedded ? lay.slot_of[p]
                               : lay.dense  ? (int32_t)((p - 1) % L + 1 + ((p - 1) / L) * (size_t)lay.P) : (int32_t)p;
    }
    return lay;
}

// Table path (packed layout): per run of 64 cells (dN, dS) if the run is a uniform wet interior, else (0, 0)
struct WaveTable { std::vector<int32_t> woff; long long uniform = 0, total = 0; };
inline WaveTable plan_wave_table(long long ndeg, const Grid &g) {
    WaveTable t;
    const long long nw = (ndeg + 63) / 64;
    t.woff.assign((size_t)(2 * nw), 0);
    t.total = nw;
    for (long long w = 0; w < nw; ++w) {
        const long long p0 = 64 * w + 1;
        if (p0 + 63 > ndeg) break;
        const int32_t *r0 = g.neig + 8 * p0;
        const int dN = r0[2] - (int)p0, dS = (int)p0 - r0[6];
        bool ok = dN > 0 && dS > 0 && r0[2] != 0 && r0[6] != 0;
        for (long long p = p0; ok && p < p0 + 64; ++p) {
            const int32_t *r = g.neig + 8 * p;
            ok = r[0] == p + 1 && r[4] == p - 1 && r[2] == p + dN && r[6] == p - dS &&
                 r[1] == p + dN + 1 && r[3] == p + dN - 1 && r[5] == p - dS - 1 && r[7] == p - dS + 1 &&
                 r[3] >= 1 && r[5] >= 1 && r[1] <= ndeg &&
                 g.mk_u[p] == 1.0 && g.mk_v[p] == 1.0 && g.mk_n[p] == 1.0 && g.mkpe[p] == 1.0 && g.mkpi[p] == 1.0;
            for (int q = 0; ok && q < 8; ++q) ok = g.mk_n[r[q]] == 1.0;
        }
        if (ok) { t.woff[2 * w] = dN; t.woff[2 * w + 1] = dS; ++t.uniform; }
    }
    return t;
}

// Dense handles with nudging: which 64 x 4 tiles of the rectangle hold a non-zero relaxation rate at all (sponges are a few
// rows or columns); per tile, bit iv-1 = some cell has a non-zero nudg(:, iv).  Empty where no table pays.
inline std::vector<unsigned char> plan_nudging_tiles(const Layout &lay, int L, int M, long long ndeg, const double *nudg) {
    const size_t n1h = (size_t)ndeg + 1;
    const int ntx = (L + 63) / 64, nty = (M + 3) / 4;
    std::vector<unsigned char> ngt((size_t)ntx * nty, 0);
    for (size_t pk = 1; pk < n1h; ++pk) {
        // (i, j) of the packed cell on the rectangle — local rows: subc(:, 2) of a band holds the global row
        int ci, cj;
        if (lay.embedded) { const long long sl = lay.slot_of[pk]; ci = (int)((sl - 1) % lay.P) + 1; cj = (int)((sl - 1) / lay.P) + 1; }
        else { ci = (int)((pk - 1) % (size_t)L) + 1; cj = (int)((pk - 1) / (size_t)L) + 1; }
        if (ci < 1 || ci > L || cj < 1 || cj > M) continue;
        unsigned char &t = ngt[(size_t)((cj - 1) >> 2) * ntx + ((ci - 1) >> 6)];
        for (int iv = 0; iv < 3; ++iv) if (nudg[pk + (size_t)iv * n1h] != 0.0) t |= (unsigned char)(1u << iv);
    }
    size_t flagged = 0;
    for (unsigned char t : ngt) flagged += t != 0;
    // (the look-up is one more dependent load in front of the rate: it pays where most tiles are free of nudging — carrier
    //  beach 8192x1024x8 -2 % per step; a frame nudged over a third of its tiles goes without, wind case +1.5 % with it)
    if (3 * flagged > ngt.size()) ngt.clear();
    return ngt;
}

// Are the caller's velocity targets fnud(0:ndeg, nlay, ix_u | ix_v) +0 bit for bit: every layer, slots 0..ndeg, read as
// 64-bit words?  (DevView::vel_targets_zero.)  A -0.0 target counts as not zero: (-0)*0 = -0 where uv_core would put +0;
// so do a denormal and a NaN.  fnud(0:ndeg, nlay, 3): the two components are the last 2 * nlay * n1h words.
inline int vel_targets_zero(const double *fnud, size_t n1h, size_t nlay) {
    if (!fnud) return 0;
    const double *p = fnud + nlay * n1h;
    for (size_t k = 0; k < 2 * nlay * n1h; ++k) {
        uint64_t w;
        std::memcpy(&w, p + k, sizeof w);
        if (w != 0) return 0;
    }
    return 1;
}

// The rigid lid's pressure sweep as a pipeline of wavefronts (k_rgld_gs_front) and the terms of its right-hand side
struct LidPlan {
    std::vector<int32_t> order, start;         // device indices of the cells level by level; first entry of each level
    int dstep = 2;                             // time between two sweeps of the pipeline
    int maxwidth = 1;                          // cells of the widest level
    std::vector<int32_t> rhs_start, rhs_ent;   // per device cell: its first entry; entries 4 * source + code
};
// subc, neig: the caller's tables; dev_index: Layout::dev_index; n1: cells per layer on the device
inline LidPlan plan_lid(long long ndeg, int lm, int mm_glob, long long n1, const std::vector<int32_t> &subc,
                        const std::vector<int32_t> &neig, const std::vector<int32_t> &dev_index) {
    LidPlan lp;
    const size_t n1h = (size_t)ndeg + 1;
    // Levels of the serial sweep's dependency graph: a cell reads the NEW pressure of the neighbours before it in packed
    // order (it comes after them) and the OLD pressure of those after it (they come after it).  On a plain frame the
    // levels are the anti-diagonals i + j; the wrapped neighbours of an orphan column / row cell bend them.
    std::vector<int32_t> level(n1h, 0), after(n1h, 0);
    int nlevel = 1;
    auto reads = [&](size_t p, int32_t (&r)[4]) {
        const int i = subc[p], j = subc[p + n1h];
        const int32_t *nb = &neig[8 * p];
        r[0] = i < lm ? nb[0] : 0; r[1] = j < mm_glob ? nb[2] : 0; r[2] = i > 1 ? nb[4] : 0; r[3] = j > 1 ? nb[6] : 0;
    };
    for (size_t p = 1; p < n1h; ++p) {
        int32_t r[4];
        reads(p, r);
        int32_t lv = after[p];
        for (int32_t qn : r)
            if (qn > 0 && (size_t)qn < p) lv = std::max(lv, level[(size_t)qn] + 1);
        level[p] = lv;
        for (int32_t qn : r)
            if (qn > 0 && (size_t)qn > p) after[(size_t)qn] = std::max(after[(size_t)qn], lv + 1);
        nlevel = std::max(nlevel, lv + 1);
    }
    // time between two sweeps of the pipeline: sweep s + 1 may touch a cell once every neighbour AFTER it in packed order has
    // been updated by sweep s — 1 + the largest level difference along such an edge (2 on a plain frame; about lm where
    // a periodic seam makes a cell read the far end of its row)
    for (size_t p = 1; p < n1h; ++p) {
        int32_t r[4];
        reads(p, r);
        for (int32_t qn : r)
            if (qn > 0 && (size_t)qn > p) lp.dstep = std::max(lp.dstep, level[(size_t)qn] - level[p] + 1);
    }
    lp.start.assign((size_t)nlevel + 1, 0);
    lp.order.assign(n1h > 1 ? n1h - 1 : 1, 0);
    for (size_t p = 1; p < n1h; ++p) ++lp.start[(size_t)level[p] + 1];
    for (int k = 0; k < nlevel; ++k) lp.start[(size_t)k + 1] += lp.start[k];
    std::vector<int32_t> fill(lp.start.begin(), lp.start.end() - 1);
    for (size_t p = 1; p < n1h; ++p) lp.order[(size_t)fill[(size_t)level[p]]++] = dev_index[p];
    for (int k = 0; k < nlevel; ++k) lp.maxwidth = std::max(lp.maxwidth, (int)(lp.start[(size_t)k + 1] - lp.start[k]));
    // the terms of every cell's right-hand side in the order of the serial scatter loops (:1727-1752): the x loop over
    // the packed cells, then the y loop; a cell with i > 1 (j > 1) subtracts its transport from itself and adds it to neig(5)
    // (neig(7)); what goes to the sentinel is dropped
    std::vector<int32_t> &cnt = lp.rhs_start;
    cnt.assign((size_t)n1 + 2, 0);
    for (int pass = 0; pass < 2; ++pass) {                       // pass 0: count, pass 1: fill
        std::vector<int32_t> at;
        if (pass) {
            for (size_t k = 1; k < cnt.size(); ++k) cnt[k] += cnt[k - 1];          // cnt[dev] = first entry of cell dev
            at.assign(cnt.begin(), cnt.end());
            lp.rhs_ent.assign((size_t)cnt.back() + 1, 0);
        }
        for (int dir = 0; dir < 2; ++dir)
            for (size_t qk = 1; qk < n1h; ++qk) {
                if (subc[qk + dir * n1h] <= 1) continue;
                const int32_t src = dev_index[qk], tgt = neig[8 * qk + (dir ? 6 : 4)];
                if (!pass) { ++cnt[(size_t)src + 1]; if (tgt > 0) ++cnt[(size_t)dev_index[(size_t)tgt] + 1]; }
                else {
                    lp.rhs_ent[(size_t)at[src]++] = 4 * src + 2 * dir;
                    if (tgt > 0) lp.rhs_ent[(size_t)at[dev_index[(size_t)tgt]]++] = 4 * src + 2 * dir + 1;
                }
            }
    }
    return lp;
}

}  // namespace beom_dense
