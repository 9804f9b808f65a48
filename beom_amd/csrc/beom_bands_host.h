// beom_bands_host.h — host-side geometry of a frame cut into bands of rows (beom_multi.hip), and the ONE copy that moves
// rows between the caller's global arrays, a band's window, the companion frame of a ring and the orphan row.
// Plain C++17, no HIP call and no other header of the library: tests/band_rows_check.cpp compiles it alone.
//
// Every array is x[outer][0:n1][inner] around the packed cell index p = 1..n1-1 (slot 0 is the sentinel), packed row by
// row (j-major).  A row j of a frame is the packed range [st[j], st[j+1]) of its "starts" table: on a frame
// with land the rows differ in length (a row may be empty), on one without, st[j] = 1 + (j-1) L — the same geometry, so
// nothing downstream asks whether there is land.  The (ndeg, nlay) real*4 output records are the same ranges without
// the sentinel: cell p at p - 1, n1 - 1 slots per layer (Spans::records).
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace beom_bands {

constexpr int kGhost = 4;          // rows per neighbour; see DESIGN.md §5 for why 4 is enough
constexpr int kMiniLo = 6;         // rows 1..6 of a y-periodic frame that the companion frame carries
constexpr int kMiniRows = kMiniLo + kGhost + 1;   // the companion frame: rows 1..6, Mr-3..Mr and the orphan row Mr+1

// shapes of the caller's arrays around the packed index: x[outer][0:n][inner]
struct Shape { int outer_nl, outer_c, inner; constexpr size_t outer(int nl) const { return (size_t)outer_nl * nl + outer_c; } };
//                                   fcor     h_th     h_to     nudg     fnud     hdot     tide     taus
inline constexpr Shape kStatic[8] = {{0,1,1}, {0,1,1}, {0,1,1}, {0,3,1}, {3,0,1}, {1,0,1}, {0,3,2}, {0,2,1}};
//                                  hlay     u        v        h_u      h_v      rs_h     dmdx     dmdy     v_cc     v_ll     tt3d     tb3d     tu3d
inline constexpr Shape kState[13] = {{1,0,1}, {1,0,1}, {1,0,1}, {1,0,1}, {1,0,1}, {1,0,2}, {1,0,3}, {1,0,3}, {1,0,1}, {1,0,1}, {2,0,1}, {2,0,1}, {2,0,1}};

// starts of n rows of equal length L: st[j] = 1 + (j-1) L for j = 1..n+1 (st[0] unused)
inline std::vector<long long> dense_starts(int n, int L) {
    std::vector<long long> st((size_t)n + 2, 0);
    for (int j = 1; j <= n + 1; ++j) st[(size_t)j] = 1 + (long long)(j - 1) * L;
    return st;
}
// starts of a window that holds the listed rows of a frame, one behind the other
inline std::vector<long long> local_starts(const std::vector<int> &rows, const std::vector<long long> &gst) {
    std::vector<long long> st(rows.size() + 2, 0);
    st[1] = 1;
    for (size_t r = 0; r < rows.size(); ++r) st[r + 2] = st[r + 1] + (gst[(size_t)rows[r] + 1] - gst[(size_t)rows[r]]);
    return st;
}

struct Band {
    int index = 0;                 // position in the chain / ring of nb bands
    int own0 = 0, own1 = 0;        // owned global rows (1-based, inclusive)
    int gs = 0, gn = 0;            // ghost rows on the south / north side
    int L = 0;                     // columns = lm + 1
    int Mr = 0;                    // rows of the ring (frames periodic in y), else 0
    std::vector<long long> lst;    // first local packed cell of local row j = 1..rows()+1
    int nown() const { return own1 - own0 + 1; }
    int rows() const { return gs + nown() + gn; }
    long long n_loc() const { return lst[(size_t)rows() + 1] - 1; }
    int grow(int j) const {        // global row of local row j (ghosts of a ring wrap)
        int g = own0 - gs + (j - 1);
        if (Mr) { while (g < 1) g += Mr; while (g > Mr) g -= Mr; }
        return g;
    }
    std::vector<int> row_list() const { std::vector<int> r; for (int j = 1; j <= rows(); ++j) r.push_back(grow(j)); return r; }
};

// rows of the chain / ring dealt to nb bands: equal counts, remainders to the first bands
inline void deal_rows(int nrows_total, int nb, int idx, int *own0, int *own1) {
    const int base = nrows_total / nb, rem = nrows_total % nb;
    int j = 1;
    for (int k = 0; k < nb; ++k) {
        const int cnt = base + (k < rem ? 1 : 0);
        if (k == idx) { *own0 = j; *own1 = j + cnt - 1; }
        j += cnt;
    }
}

// geometry of band idx of a frame of lm+1 columns and mm+1 rows without land; a single band of a non-periodic frame is
// the whole frame (no slab at all)
inline Band make_band(int lm, int mm, int nb, int idx, bool ring) {
    Band s;
    s.index = idx; s.L = lm + 1; s.Mr = ring ? mm : 0;
    deal_rows(ring ? mm : mm + 1, nb, idx, &s.own0, &s.own1);
    s.gs = (ring || idx > 0) ? kGhost : 0;
    s.gn = (ring || idx < nb - 1) ? kGhost : 0;
    s.lst = dense_starts(s.rows(), s.L);
    return s;
}

// global row of every row of the companion frame of a ring of Mr rows
inline std::vector<int> mini_row_list(int Mr) {
    std::vector<int> r;
    for (int j = 1; j <= kMiniLo; ++j) r.push_back(j);
    for (int j = Mr - kGhost + 1; j <= Mr; ++j) r.push_back(j);
    r.push_back(Mr + 1);
    return r;
}

// ---- row spans and the one copy ------------------------------------------------------------------------------------------
struct Span { size_t src, dst, len; };          // cells [src, src+len) of the source -> [dst, dst+len), packed indices
struct Spans {
    size_t n1src = 0, n1dst = 0;   // slots of one outer slice of either side
    int base = 1;                  // 1: slot 0 is a sentinel, cell p at p; 0: records without one, cell p at p - 1
    bool sentinel = false;         // copy slot 0 of every outer slice too (base 1 only)
    std::vector<Span> v;
    void add(long long src, long long dst, long long len) {
        if (len <= 0) return;
        if (!v.empty() && v.back().src + v.back().len == (size_t)src && v.back().dst + v.back().len == (size_t)dst) v.back().len += (size_t)len;
        else v.push_back({(size_t)src, (size_t)dst, (size_t)len});
    }
    Spans records() const { Spans r = *this; r.base = 0; r.sentinel = false; --r.n1src; --r.n1dst; return r; }
};

// dst[o][.][inner] <- src[o][.][inner] for every outer slice o: the sentinel if asked, then one memcpy per span; no other slot
// of dst is touched.  A null src or dst: nothing to do.
template <class T>
void copy_rows(T *dst, const T *src, size_t outer, size_t inner, const Spans &s) {
    if (!dst || !src) return;
    const size_t off = (size_t)(1 - s.base);
    for (size_t o = 0; o < outer; ++o) {
        T *d = dst + o * s.n1dst * inner;
        const T *x = src + o * s.n1src * inner;
        if (s.sentinel) std::memcpy(d, x, inner * sizeof(T));
        for (const Span &r : s.v) std::memcpy(d + (r.dst - off) * inner, x + (r.src - off) * inner, r.len * inner * sizeof(T));
    }
}
// the destination as a new array (every slot outside the spans 0); empty for a null src
template <class T>
std::vector<T> cut_rows(const T *src, size_t outer, size_t inner, const Spans &s) {
    std::vector<T> z;
    if (!src) return z;
    z.resize(outer * s.n1dst * inner);
    copy_rows(z.data(), src, outer, inner, s);
    return z;
}

// global arrays (starts gst, n1g slots) -> a window of the listed rows, one behind the other, sentinel included: a band's
// row_list() (a ring's ghosts wrapped) or the companion frame's mini_row_list()
inline Spans spans_in(const std::vector<int> &rows, const std::vector<long long> &gst, size_t n1g) {
    Spans s;
    s.n1src = n1g; s.sentinel = true;
    long long at = 1;
    for (int g : rows) {
        const long long len = gst[(size_t)g + 1] - gst[(size_t)g];
        s.add(gst[(size_t)g], at, len);
        at += len;
    }
    s.n1dst = (size_t)at;
    return s;
}
// a band's owned rows -> global arrays.  Every band's window holds the sentinel; the global one is pasted from band 0 only.
inline Spans spans_out(const Band &b, const std::vector<long long> &gst, size_t n1g) {
    Spans s;
    s.n1src = (size_t)b.n_loc() + 1; s.n1dst = n1g; s.sentinel = b.index == 0;
    for (int j = b.gs + 1; j <= b.gs + b.nown(); ++j)
        s.add(b.lst[(size_t)j], gst[(size_t)(b.own0 + j - b.gs - 1)], b.lst[(size_t)j + 1] - b.lst[(size_t)j]);
    return s;
}
// the companion frame's last row -> the orphan row Mr+1 of the global arrays
inline Spans spans_orphan_out(int Mr, int L, const std::vector<long long> &gst, size_t n1g) {
    Spans s;
    s.n1src = (size_t)kMiniRows * L + 1; s.n1dst = n1g;
    s.add(1 + (long long)(kMiniRows - 1) * L, gst[(size_t)Mr + 1], L);
    return s;
}
// window of band 0 of a ring -> the companion frame: rows 1..kMiniLo are the band's first owned rows, rows Mr-3..Mr its
// south ghosts; the orphan row comes from spans_orphan_to_mini
inline Spans spans_window_to_mini(const Band &b0) {
    Spans s;
    s.n1src = (size_t)b0.n_loc() + 1; s.n1dst = (size_t)kMiniRows * b0.L + 1; s.sentinel = true;
    s.add(b0.lst[(size_t)b0.gs + 1], 1, (long long)kMiniLo * b0.L);
    s.add(b0.lst[1], 1 + (long long)kMiniLo * b0.L, (long long)kGhost * b0.L);
    return s;
}
// a one-row array [outer][0:L+1][inner] that holds the orphan row <-> the companion frame's last row
inline Spans spans_orphan_to_mini(int L) {
    Spans s;
    s.n1src = (size_t)L + 1; s.n1dst = (size_t)kMiniRows * L + 1;
    s.add(1, 1 + (long long)(kMiniRows - 1) * L, L);
    return s;
}
inline Spans spans_mini_to_orphan(int L) {
    Spans s;
    s.n1src = (size_t)kMiniRows * L + 1; s.n1dst = (size_t)L + 1; s.sentinel = true;
    s.add(1 + (long long)(kMiniRows - 1) * L, 1, L);
    return s;
}
// a window as it stands (a handle created from its band's window: nothing to cut)
inline Spans spans_whole(const Band &b) {
    Spans s;
    s.n1src = s.n1dst = (size_t)b.n_loc() + 1; s.sentinel = true;
    s.add(1, 1, b.n_loc());
    return s;
}

// ---- open-boundary passes (no_gradient_obc, private_mod.f95:2613-2679) re-indexed to a window ---------------------------
// A row of the table segm(nseg, 18) carries two passes: the first updates the cell of column 10 from the cell of column 16,
// the second the cell of column 1 from the cell of column 13.  A window gets every pass as a row of its own.
using ObcRow = std::array<int32_t, 18>;

// the pass (0 / 1) of the row with the columns c[0..17]: both passes off, then this one on, its updated cell qu and its
// source cell qs (0 = none) in the window's own indices
inline ObcRow obc_pass_row(const ObcRow &c, int pass, int32_t qu, int32_t qs) {
    ObcRow r = c;
    r[0] = r[9] = -1; r[12] = r[15] = r[6] = 0;
    r[pass == 0 ? 9 : 0] = qu;
    r[pass == 0 ? 15 : 12] = qs;
    return r;
}
inline ObcRow obc_columns(const int32_t *segm, int nseg, int is) {
    ObcRow c;
    for (size_t k = 0; k < 18; ++k) c[k] = segm[(size_t)is + (size_t)nseg * k];
    return c;
}
// rows -> the column-major table tab(n, 18) that beom_set_open_boundaries takes
inline std::vector<int32_t> obc_table(const std::vector<ObcRow> &rows) {
    const size_t n = rows.size();
    std::vector<int32_t> tab(n * 18);
    for (size_t is = 0; is < n; ++is)
        for (size_t c = 0; c < 18; ++c) tab[is + n * c] = rows[is][c];
    return tab;
}
// The passes of a table with GLOBAL cell indices (a frame without land, L columns) for the window whose local row jl + 1
// is global row wrows[jl].  A pass goes to EVERY local row that holds the updated cell's global row — in a ring a row can
// be there twice, owned and as a wrapped ghost — with the source cell taken from the local row next to it (or itself) that
// holds the source's row; where there is none, the pass is another band's.
inline std::vector<ObcRow> obc_window_rows(int nseg, const int32_t *segm, const std::vector<int> &wrows, int L) {
    std::vector<ObcRow> out;
    auto row_of = [&](int32_t q) { return (q - 1) / L + 1; };
    auto col_of = [&](int32_t q) { return (q - 1) % L + 1; };
    const long long nw = (long long)wrows.size();
    for (int is = 0; is < nseg; ++is) {
        const ObcRow c = obc_columns(segm, nseg, is);
        for (int pass = 0; pass < 2; ++pass) {
            const int32_t qu = c[pass == 0 ? 9 : 0], qs = c[pass == 0 ? 15 : 12];
            if (qu < 1) continue;
            for (long long jl = 0; jl < nw; ++jl) {
                if (wrows[(size_t)jl] != row_of(qu)) continue;
                int32_t src = qs == 0 ? 0 : -1;
                if (qs > 0)
                    for (long long js = jl - 1; js <= jl + 1; ++js)
                        if (js >= 0 && js < nw && wrows[(size_t)js] == row_of(qs)) { src = (int32_t)(col_of(qs) + js * L); break; }
                if (src < 0) continue;
                out.push_back(obc_pass_row(c, pass, (int32_t)(col_of(qu) + jl * L), src));
            }
        }
    }
    return out;
}

}  // namespace beom_bands
