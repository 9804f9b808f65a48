// band_rows_check.cpp — the band geometry and the one row copy of beom_amd/csrc/beom_bands_host.h against their definition
// written out index by index (test_band_rows_cpu.py builds this with ASan and UBSan and runs it; exit status 0 = all held).
// The restatement below never calls copy_rows: it computes, for every destination cell, the source cell from the row, the
// column and the starts tables, and counts who writes what.
#include "../beom_amd/csrc/beom_bands_host.h"

#include <cstdio>
#include <cstdlib>

using namespace beom_bands;

namespace {

int g_checks = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                        \
            std::fprintf(stderr, "\n");                                               \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

constexpr size_t kGuard = 64;      // guard elements before and after every buffer

template <class T> T poison();     // a NaN with a payload: no source value has these bits
template <> double poison<double>() { const uint64_t b = 0x7ff8dead0000beefull; double x; std::memcpy(&x, &b, 8); return x; }
template <> float poison<float>() { const uint32_t b = 0x7fc0deadu; float x; std::memcpy(&x, &b, 4); return x; }
template <class T> T guard_value();
template <> double guard_value<double>() { const uint64_t b = 0x7ff8600d0000600dull; double x; std::memcpy(&x, &b, 8); return x; }
template <> float guard_value<float>() { const uint32_t b = 0x7fc0600du; float x; std::memcpy(&x, &b, 4); return x; }
template <class T> bool same(const T &a, const T &b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

template <class T>
struct Buf {                       // n elements between two guards
    std::vector<T> all;
    size_t n;
    explicit Buf(size_t n_, bool distinct = false, int seed = 0) : all(n_ + 2 * kGuard, guard_value<T>()), n(n_) {
        for (size_t i = 0; i < n; ++i) at(i) = distinct ? (T)(1 + i + 100000 * (size_t)seed) : poison<T>();   // (exact in float: < 2^24)
    }
    T *p() { return all.data() + kGuard; }
    const T *p() const { return all.data() + kGuard; }
    T &at(size_t i) { return all[kGuard + i]; }
    const T &at(size_t i) const { return all[kGuard + i]; }
    void guards_intact(const char *what) const {
        for (size_t i = 0; i < kGuard; ++i)
            CHECK(same(all[i], guard_value<T>()) && same(all[kGuard + n + i], guard_value<T>()), "%s: guard element %zu overwritten", what, i);
    }
    bool equals(const Buf &o) const { return n == o.n && std::memcmp(p(), o.p(), n * sizeof(T)) == 0; }
};

struct Frame {                     // the caller's side: rows j = 1..Mg as packed ranges [gst[j], gst[j+1])
    int L = 0, Mg = 0, Mr = 0;     // Mr: rows of the ring, 0 = not periodic in y
    std::vector<long long> gst;
    std::vector<Band> bands;
    size_t n1g() const { return (size_t)gst[(size_t)Mg + 1]; }
    long long len(int g) const { return gst[(size_t)g + 1] - gst[(size_t)g]; }
};

// global row of local row jl of a band, restated: the window starts gs rows below own0, a ring's rows wrap into 1..Mr
int global_row(const Frame &F, const Band &b, int jl) {
    int g = b.own0 - b.gs + jl - 1;
    if (F.Mr) g = ((g - 1) % F.Mr + F.Mr) % F.Mr + 1;
    return g;
}

Frame chain(int L, int Mg, int nb) {
    Frame F;
    F.L = L; F.Mg = Mg;
    F.gst = dense_starts(Mg, L);
    for (int j = 1; j <= Mg + 1; ++j) CHECK(F.gst[(size_t)j] == 1 + (long long)(j - 1) * L, "dense_starts row %d", j);
    for (int k = 0; k < nb; ++k) F.bands.push_back(make_band(L - 1, Mg - 1, nb, k, false));
    return F;
}
Frame ring(int L, int Mr, int nb) {
    Frame F;
    F.L = L; F.Mg = Mr + 1; F.Mr = Mr;
    F.gst = dense_starts(F.Mg, L);
    for (int k = 0; k < nb; ++k) F.bands.push_back(make_band(L - 1, Mr, nb, k, true));
    return F;
}
// a frame with land: ragged rows (one empty, several of full length), the bands cut after the rows listed in `last`
Frame land(const std::vector<int> &last) {
    static const int lens[23] = {7, 5, 0, 3, 7, 6, 1, 4, 7, 2, 5, 0, 3, 7, 1, 4, 6, 2, 7, 5, 3, 6, 4};
    Frame F;
    F.L = 7; F.Mg = 23;
    F.gst.assign((size_t)F.Mg + 3, 0);
    F.gst[1] = 1;
    for (int j = 1; j <= F.Mg; ++j) F.gst[(size_t)j + 1] = F.gst[(size_t)j] + lens[j - 1];
    F.gst[(size_t)F.Mg + 2] = F.gst[(size_t)F.Mg + 1];
    const int nb = (int)last.size();
    for (int k = 0; k < nb; ++k) {
        Band b;
        b.index = k; b.L = F.L;
        b.own0 = k ? last[(size_t)k - 1] + 1 : 1; b.own1 = last[(size_t)k];
        b.gs = k > 0 ? kGhost : 0; b.gn = k < nb - 1 ? kGhost : 0;
        b.lst = local_starts(b.row_list(), F.gst);
        F.bands.push_back(b);
    }
    return F;
}

// the geometry itself: the bands tile the owned rows, the starts of a window are the running sums of its rows' lengths
void check_geometry(const Frame &F, const char *what) {
    const int nb = (int)F.bands.size(), nrows = F.Mr ? F.Mr : F.Mg;
    CHECK(F.bands[0].own0 == 1 && F.bands[(size_t)nb - 1].own1 == nrows, "%s: the bands do not span the rows", what);
    for (int k = 0; k < nb; ++k) {
        const Band &b = F.bands[(size_t)k];
        if (k) CHECK(b.own0 == F.bands[(size_t)k - 1].own1 + 1, "%s: band %d does not follow band %d", what, k, k - 1);
        CHECK(b.gs == ((F.Mr || k > 0) ? kGhost : 0) && b.gn == ((F.Mr || k < nb - 1) ? kGhost : 0), "%s: ghosts of band %d", what, k);
        CHECK(b.lst.size() == (size_t)b.rows() + 2 && b.lst[1] == 1, "%s: lst of band %d", what, k);
        const std::vector<int> rows = b.row_list();
        CHECK((int)rows.size() == b.rows(), "%s: row_list of band %d", what, k);
        long long at = 1;
        for (int jl = 1; jl <= b.rows(); ++jl) {
            const int g = global_row(F, b, jl);
            CHECK(rows[(size_t)jl - 1] == g && g >= 1 && g <= nrows, "%s: band %d local row %d is global row %d, not %d", what, k, jl, rows[(size_t)jl - 1], g);
            CHECK(b.lst[(size_t)jl] == at, "%s: band %d lst[%d]", what, k, jl);
            at += F.len(g);
        }
        CHECK(b.n_loc() == at - 1, "%s: n_loc of band %d", what, k);
    }
    if (F.Mr) {                    // a ring's ghosts wrap: rows Mr-3..Mr in front of band 0, rows 1..4 behind the last band
        const std::vector<int> first = F.bands[0].row_list(), last = F.bands[(size_t)nb - 1].row_list();
        for (int j = 0; j < kGhost; ++j)
            CHECK(first[(size_t)j] == F.Mr - kGhost + 1 + j && last[last.size() - kGhost + (size_t)j] == 1 + j, "%s: wrapped ghost row %d", what, j);
    }
}

// One array shape on one frame: cut every band's window, paste every band's owned rows back.  base 1: packed arrays with a
// sentinel in slot 0; base 0: records without one (cell p at p - 1).
template <class T>
void check_shape(const Frame &F, size_t outer, size_t inner, int base, const char *what) {
    const size_t n1g = F.n1g() - (size_t)(1 - base), off = (size_t)(1 - base);
    const Buf<T> glob(outer * n1g * inner, true, 1);
    Buf<T> back(outer * n1g * inner);                       // all parts pasted into one poisoned array
    std::vector<int> writes(n1g, 0);                        // ... and who wrote which slot, restated
    auto G = [&](size_t o, size_t slot, size_t i) { return (o * n1g + slot) * inner + i; };

    // paste one part into a poisoned array of its own: exactly the restated slots are written, with the part's values
    auto paste_part = [&](const Buf<T> &loc, size_t n1l, const Spans &sp, const std::vector<std::pair<size_t, size_t>> &cells /* (dst slot, src slot) */) {
        Buf<T> alone(outer * n1g * inner);
        const Buf<T> before = loc;
        copy_rows(alone.p(), loc.p(), outer, inner, sp);
        alone.guards_intact(what);
        CHECK(std::memcmp(loc.all.data(), before.all.data(), loc.all.size() * sizeof(T)) == 0, "%s: a paste changed its source", what);
        std::vector<char> mine(n1g, 0);
        for (const auto &c : cells) { CHECK(!mine[c.first], "%s: slot %zu restated twice", what, c.first); mine[c.first] = 1; ++writes[c.first]; }
        for (size_t o = 0; o < outer; ++o)
            for (size_t slot = 0; slot < n1g; ++slot)
                for (size_t i = 0; i < inner; ++i)
                    if (!mine[slot]) CHECK(same(alone.at(G(o, slot, i)), poison<T>()), "%s: slot %zu outside the spans was written", what, slot);
        for (const auto &c : cells)
            for (size_t o = 0; o < outer; ++o)
                for (size_t i = 0; i < inner; ++i) {
                    const T &x = loc.at((o * n1l + c.second) * inner + i);
                    CHECK(same(alone.at(G(o, c.first, i)), x), "%s: slot %zu pasted from the wrong place", what, c.first);
                    CHECK(same(back.at(G(o, c.first, i)), poison<T>()), "%s: slot %zu written by two parts", what, c.first);
                    back.at(G(o, c.first, i)) = x;
                }
    };

    std::vector<Buf<T>> windows;
    for (const Band &b : F.bands) {
        Spans in = spans_in(b.row_list(), F.gst, F.n1g()), out = spans_out(b, F.gst, F.n1g());
        if (!base) { in = in.records(); out = out.records(); }
        const size_t n1l = (size_t)b.n_loc() + (size_t)base;
        CHECK(in.n1dst == n1l && out.n1src == n1l && in.n1src == n1g && out.n1dst == n1g, "%s: band %d slot counts", what, b.index);
        Buf<T> win(outer * n1l * inner);
        copy_rows(win.p(), glob.p(), outer, inner, in);
        win.guards_intact(what);
        // every window cell is the defined global cell; nothing of the window is left poisoned
        size_t covered = 0;
        for (size_t o = 0; o < outer; ++o) {
            if (base)
                for (size_t i = 0; i < inner; ++i) CHECK(same(win.at(o * n1l * inner + i), glob.at(G(o, 0, i))), "%s: band %d sentinel of slice %zu", what, b.index, o);
            for (int jl = 1; jl <= b.rows(); ++jl) {
                const int g = global_row(F, b, jl);
                for (long long c = 0; c < F.len(g); ++c, ++covered)
                    for (size_t i = 0; i < inner; ++i)
                        CHECK(same(win.at((o * n1l + (size_t)(b.lst[(size_t)jl] + c) - off) * inner + i), glob.at(G(o, (size_t)(F.gst[(size_t)g] + c) - off, i))),
                              "%s: band %d slice %zu local row %d column %lld", what, b.index, o, jl, c);
            }
        }
        CHECK(covered == outer * (size_t)b.n_loc(), "%s: band %d: %zu cells covered", what, b.index, covered);
        // the band's owned rows back; the sentinel from band 0 only
        std::vector<std::pair<size_t, size_t>> cells;
        if (base && b.index == 0) cells.push_back({0, 0});
        for (int jl = b.gs + 1; jl <= b.gs + b.nown(); ++jl) {
            const int g = b.own0 + (jl - b.gs - 1);
            for (long long c = 0; c < F.len(g); ++c) cells.push_back({(size_t)(F.gst[(size_t)g] + c) - off, (size_t)(b.lst[(size_t)jl] + c) - off});
        }
        paste_part(win, n1l, out, cells);
        windows.push_back(win);
    }

    if (F.Mr) {                    // the companion frame of a ring: rows 1..6, Mr-3..Mr, Mr+1 of the global arrays
        const int L = F.L;
        const size_t n1m = (size_t)kMiniRows * L + (size_t)base;
        const std::vector<int> mrows = mini_row_list(F.Mr);
        CHECK((int)mrows.size() == kMiniRows && mrows[0] == 1 && mrows[kMiniLo] == F.Mr - 3 && mrows[kMiniRows - 1] == F.Mr + 1, "%s: mini_row_list", what);
        Spans in = spans_in(mrows, F.gst, F.n1g()), out = spans_orphan_out(F.Mr, L, F.gst, F.n1g());
        if (!base) { in = in.records(); out = out.records(); }
        CHECK(in.n1dst == n1m && out.n1src == n1m && out.n1dst == n1g, "%s: companion slot counts", what);
        Buf<T> mini(outer * n1m * inner);
        copy_rows(mini.p(), glob.p(), outer, inner, in);
        mini.guards_intact(what);
        for (size_t o = 0; o < outer; ++o) {
            if (base)
                for (size_t i = 0; i < inner; ++i) CHECK(same(mini.at(o * n1m * inner + i), glob.at(G(o, 0, i))), "%s: companion sentinel", what);
            for (int r = 0; r < kMiniRows; ++r) {
                const int g = r < kMiniLo ? r + 1 : r < kMiniLo + kGhost ? F.Mr - kGhost + 1 + (r - kMiniLo) : F.Mr + 1;
                for (int c = 0; c < L; ++c)
                    for (size_t i = 0; i < inner; ++i)
                        CHECK(same(mini.at((o * n1m + (size_t)(1 + r * L + c) - off) * inner + i), glob.at(G(o, (size_t)(1 + (g - 1) * L + c) - off, i))),
                              "%s: companion row %d column %d", what, r + 1, c);
            }
        }
        // the orphan row comes back from the companion's last row only, without the sentinel
        std::vector<std::pair<size_t, size_t>> cells;
        for (int c = 0; c < L; ++c) cells.push_back({(size_t)(1 + F.Mr * L + c) - off, (size_t)(1 + (kMiniRows - 1) * L + c) - off});
        paste_part(mini, n1m, out, cells);
        if (base) {
            // a rank that holds band 0's window and the orphan row builds the same companion frame from those two
            const size_t n1o = (size_t)L + 1;
            Buf<T> orph(outer * n1o * inner, true, 2);
            for (size_t o = 0; o < outer; ++o)
                for (int c = 0; c < L; ++c)
                    for (size_t i = 0; i < inner; ++i) orph.at((o * n1o + 1 + (size_t)c) * inner + i) = glob.at(G(o, (size_t)(1 + F.Mr * L + c), i));
            Buf<T> mini2(outer * n1m * inner);
            copy_rows(mini2.p(), windows[0].p(), outer, inner, spans_window_to_mini(F.bands[0]));
            copy_rows(mini2.p(), orph.p(), outer, inner, spans_orphan_to_mini(L));
            mini2.guards_intact(what);
            CHECK(mini2.equals(mini), "%s: window + orphan row -> companion differs from global -> companion", what);
            // ... and gets the orphan row back as a one-row array, the sentinel with it
            Buf<T> orph2(outer * n1o * inner);
            copy_rows(orph2.p(), mini.p(), outer, inner, spans_mini_to_orphan(L));
            orph2.guards_intact(what);
            for (size_t o = 0; o < outer; ++o)
                for (size_t slot = 0; slot < n1o; ++slot)
                    for (size_t i = 0; i < inner; ++i)
                        CHECK(same(orph2.at((o * n1o + slot) * inner + i), slot ? orph.at((o * n1o + slot) * inner + i) : glob.at(G(o, 0, i))),
                              "%s: orphan row slot %zu", what, slot);
            // the window as it stands
            Buf<T> w2(windows[0].n);
            copy_rows(w2.p(), windows[0].p(), outer, inner, spans_whole(F.bands[0]));
            CHECK(w2.equals(windows[0]), "%s: spans_whole", what);
        }
    }

    // all parts together reproduce the source bit for bit: every slot written by exactly one part, no poison left
    for (size_t slot = 0; slot < n1g; ++slot) CHECK(writes[slot] == 1, "%s: slot %zu written by %d parts", what, slot, writes[slot]);
    back.guards_intact(what);
    CHECK(back.equals(glob), "%s: the pasted array differs from the source", what);
}

void check_frame(const Frame &F, const char *what) {
    check_geometry(F, what);
    const int nl = 3;
    for (const Shape &s : kStatic) check_shape<double>(F, s.outer(nl), (size_t)s.inner, 1, what);
    for (const Shape &s : kState) check_shape<double>(F, s.outer(nl), (size_t)s.inner, 1, what);
    check_shape<float>(F, (size_t)nl, 1, 0, what);          // the (ndeg, nlay) real*4 records
}

void check_null_and_merge() {
    const Frame F = chain(7, 23, 3);
    const Spans in = spans_in(F.bands[1].row_list(), F.gst, F.n1g());
    CHECK(in.v.size() == 1, "adjacent rows were not merged into one span (%zu spans)", in.v.size());
    Buf<double> a(F.n1g(), true), b((size_t)F.bands[1].n_loc() + 1);
    const Buf<double> b0 = b;
    copy_rows<double>(b.p(), nullptr, 1, 1, in);
    copy_rows<double>(nullptr, a.p(), 1, 1, in);
    CHECK(b.equals(b0), "a null source wrote something");
    CHECK(cut_rows<double>(nullptr, 1, 1, in).empty(), "cut_rows of a null source is not empty");
    const std::vector<double> z = cut_rows<double>(a.p(), 1, 1, in);
    copy_rows(b.p(), a.p(), 1, 1, in);
    CHECK(z.size() == b.n && std::memcmp(z.data(), b.p(), b.n * sizeof(double)) == 0, "cut_rows differs from copy_rows");
}

// Open-boundary passes on the chain of 7 columns, 23 rows and 3 bands (windows: rows 1..12, 5..20, 13..23).  Cell (column i,
// row j) is i + 7 (j - 1).  Columns 1 / 13: updated and source cell of the second pass, 10 / 16: of the first; every other
// column is carried along (1000 (segment) + column), except column 7, which a re-indexed row sets to 0.
//   segment 1: first pass (3, 9) <- (3, 10), second pass (4, 9) without a source
//   segment 2: first pass off (-1), second pass (2, 5) <- (2, 4)
//   segment 3: first pass (7, 23) <- (6, 23), second pass (1, 13) <- (1, 12)
void check_open_boundaries() {
    const ObcRow seg[3] = {
        {60, 1002, 1003, 1004, 1005, 1006, 1007, 1008, 1009, 59, 1011, 1012, 0, 1014, 1015, 66, 1017, 1018},
        {30, 2002, 2003, 2004, 2005, 2006, 2007, 2008, 2009, -1, 2011, 2012, 23, 2014, 2015, 0, 2017, 2018},
        {85, 3002, 3003, 3004, 3005, 3006, 3007, 3008, 3009, 161, 3011, 3012, 78, 3014, 3015, 160, 3017, 3018}};
    const std::vector<int32_t> segm = obc_table({seg[0], seg[1], seg[2]});          // column-major segm(3, 18)
    for (int is = 0; is < 3; ++is)
        for (int c = 0; c < 18; ++c) CHECK(segm[(size_t)is + 3 * (size_t)c] == seg[is][(size_t)c], "obc_table (%d, %d)", is, c);
    // band 0, rows 1..12 (local = global indices): both passes of segment 1, the second of segment 2; row 13 and 23 are not here
    const std::vector<ObcRow> want0 = {
        {-1, 1002, 1003, 1004, 1005, 1006, 0, 1008, 1009, 59, 1011, 1012, 0, 1014, 1015, 66, 1017, 1018},
        {60, 1002, 1003, 1004, 1005, 1006, 0, 1008, 1009, -1, 1011, 1012, 0, 1014, 1015, 0, 1017, 1018},
        {30, 2002, 2003, 2004, 2005, 2006, 0, 2008, 2009, -1, 2011, 2012, 23, 2014, 2015, 0, 2017, 2018}};
    // band 1, rows 5..20 (row j is local row j - 4): (3, 9) = 3 + 7*4 = 31 <- (3, 10) = 38; (4, 9) = 32; the second pass of segment 2
    // has its source in row 4, which is another band's: dropped; (1, 13) = 1 + 7*8 = 57 <- (1, 12) = 50
    const std::vector<ObcRow> want1 = {
        {-1, 1002, 1003, 1004, 1005, 1006, 0, 1008, 1009, 31, 1011, 1012, 0, 1014, 1015, 38, 1017, 1018},
        {32, 1002, 1003, 1004, 1005, 1006, 0, 1008, 1009, -1, 1011, 1012, 0, 1014, 1015, 0, 1017, 1018},
        {57, 3002, 3003, 3004, 3005, 3006, 0, 3008, 3009, -1, 3011, 3012, 50, 3014, 3015, 0, 3017, 3018}};
    // band 2, rows 13..23 (row j is local row j - 12): (7, 23) = 7 + 7*10 = 77 <- (6, 23) = 76; the second pass of segment 3 has
    // its source in row 12: dropped
    const std::vector<ObcRow> want2 = {
        {-1, 3002, 3003, 3004, 3005, 3006, 0, 3008, 3009, 77, 3011, 3012, 0, 3014, 3015, 76, 3017, 3018}};
    const std::vector<ObcRow> *want[3] = {&want0, &want1, &want2};
    const Frame F = chain(7, 23, 3);
    for (int k = 0; k < 3; ++k) {
        const std::vector<ObcRow> got = obc_window_rows(3, segm.data(), F.bands[(size_t)k].row_list(), 7);
        CHECK(got.size() == want[k]->size(), "band %d: %zu passes, not %zu", k, got.size(), want[k]->size());
        for (size_t r = 0; r < got.size(); ++r)
            for (size_t c = 0; c < 18; ++c) CHECK(got[r][c] == (*want[k])[r][c], "band %d pass %zu column %zu: %d, not %d", k, r, c + 1, got[r][c], (*want[k])[r][c]);
    }
    CHECK(obc_table({}).empty(), "the table of no rows is not empty");
}

}  // namespace

int main() {
    check_frame(chain(7, 23, 3), "chain of 3 bands");
    check_frame(chain(7, 23, 1), "chain of 1 band");
    check_frame(ring(7, 22, 2), "ring of 2 bands");
    check_frame(ring(7, 22, 3), "ring of 3 bands");
    check_frame(land({11, 23}), "land, 2 bands");
    check_frame(land({8, 15, 23}), "land, 3 bands");
    check_null_and_merge();
    check_open_boundaries();
    std::printf("band_rows_check: %d checks held\n", g_checks);
    return 0;
}
