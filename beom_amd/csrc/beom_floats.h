// beom_floats.h — Lagrangian (isopycnal) floats carried by the layer velocities (no reference routine; DESIGN.md f-N7).
// Include after beom_kernels.h.
//
// A float has a position (x, y) in FP64 grid units and a fixed layer l.  Cell (i, j) spans [i-1, i] x [j-1, j]; u(p) sits on
// the cell's west face, v(p) on its south face; E = neig(1, p), N = neig(3, p).  cell(x, y) is the packed cell of
// i = floor(x)+1, j = floor(y)+1, or 0 if (i, j) lies outside 1..lm+1 x 1..mm+1 or holds no packed cell; wet(x, y) means
// mk_n(cell(x, y)) > 0.5.  xper (yper): the frame wraps in x (y), as its neig says.  All FP64, no contraction, in this order:
//     fx = floor(x); a = x - fx;   fy = floor(y); b = y - fy;   p = cell(x, y)
//     U(x,y) = (1.0 - a)*u(p,l) + a*u(E,l)          V(x,y) = (1.0 - b)*v(p,l) + b*v(N,l)
//     cdt = dt * i_dl                               (formed once on the host)
//     wrapx(z): if xper { if (z < 0.0) z = z + lm; if (z >= lm) z = z - lm }          (wrapy alike with mm, yper)
// Heun's method on the velocities before (stage 1) and after (stage 2) the step's momentum update:
//     stage 1:  k1 = (U, V)(x, y) * cdt;  (xs, ys) = (wrapx(x + k1x), wrapy(y + k1y));  if !wet(xs, ys): (xs, ys) = (x, y)
//     stage 2:  k2 = (U, V)(xs, ys) * cdt;  xn = wrapx(x + 0.5*(k1x + k2x)), yn alike
//     landing:  the first wet one of (xn, yn), (xn, y), (x, yn), (x, y); rejected += 1 if that is not the first
// A float that starts in a wet cell is therefore in a wet cell after every step, and both velocities are only ever
// evaluated with a wet home cell.  Slots of the rectangle that are no packed cell hold the sentinel's mask, so on dense and
// embedded handles cell() is the slot itself; on the table path it is the (i, j) -> packed cell map of the integrals.
//
// One thread per float.  A float depends on no other float, so stage 2 of a step and stage 1 of the next, which read the
// same velocity field, run in one launch (MODE 3): K steps of one beom_step call cost K + 1 launches.  The extra wet()
// lookups of the landing rule are taken only by the lanes whose first candidate is dry.
#pragma once

struct FloatView {
    long long n;
    double *x, *y;
    const int32_t *layer;
    int32_t *rejected;
    double *k1x, *k1y, *xs, *ys;  // stage 1's increment and provisional position, read by stage 2
    const int32_t *cellmap;       // table path: packed cell of (i, j) at (j-1)*L + (i-1), 0 = none; null otherwise
    double cdt, flm, fmm;         // dt * i_dl; lm and mm
    int xper, yper;
    double *rec;                  // the record stage 2 writes, [3][n] = x, y, thickness of the home cell; null = none
};

__device__ __forceinline__ double flt_wrap(double z, double len, int per) {
    if (per) {
        if (z < 0.0) z = z + len;
        if (z >= len) z = z - len;
    }
    return z;
}

// the context of cell (floor(x)+1, floor(y)+1), given the two floors; false: outside the rectangle (cell 0).  (The range
// test is made on the doubles: a position that is not finite converts to no index.)
__device__ __forceinline__ bool flt_locate(CellDense &c, const DevView &d, const FloatView &, double fx, double fy) {
    if (!(fx >= 0.0 && fx < (double)d.L && fy >= 0.0 && fy < (double)d.M)) return false;
    c.set_cell(d, (int)fx + 1, (int)fy + 1);
    return true;
}
__device__ __forceinline__ bool flt_locate(CellGather &c, const DevView &d, const FloatView &f, double fx, double fy) {
    if (!(fx >= 0.0 && fx < (double)d.L && fy >= 0.0 && fy < (double)d.M)) return false;
    c.ipnt = f.cellmap[(long long)(int)fy * d.L + (int)fx];
    c.row = d.neig + 8ll * c.ipnt;
    c.dv = &d;
    return c.ipnt != 0;
}

// ---- floats on a band of rows (beom_multi.hip; include/beom_hip.h "Floats on bands") -----------------------------------------
// Every band holds the arrays of ALL floats, positions in GLOBAL grid units; slot t is float t on every band.  A band's
// thread t acts only if the float's home row floor(y[t]) + 1 is one of the band's owned rows.  a, b, the wraps and every sum
// are formed from the global x, y exactly as above; only the integer row of a lookup is translated into the window (modulo
// the ring's rows on a frame periodic in y; a row the window holds twice is taken where it is owned).  A lookup whose row
// lies in the frame but not in the window reads nothing: the cell counts as 0 and stats[0] ("out of reach") goes up.
// A float that stage 2 carries out of the band's rows is handed over: the launch still runs stage 1 of the next step on it
// (the ghost rows hold the neighbour's values bit for bit) and appends one 64-byte record to the south or north outbox.
struct FloatBand {
    int own0, nown;               // owned global rows own0 .. own0 + nown - 1
    int gs;                       // window row gs + 1 is global row own0
    int lo, hi;                   // window rows a lookup may have as its home row: kFloatReach rows beyond the owned ones, where
                                  // a neighbour's rows follow (with cdt |u|, cdt |v| < 1 no lookup goes further), else to the frame's edge
    int Mf;                       // rows of the frame (mm + 1): the range test of cell()
    int nring;                    // rows of the ring (mm) on a frame periodic in y, else 0
    int capacity;                 // records an outbox holds
    unsigned long long *box_s, *box_n;   // outboxes: the count at [0], record r at byte 64 (r + 1); null = no neighbour
    unsigned long long *stats;    // [0] lookups out of reach, [1] records dropped by a full outbox, [2] records ingested
};
struct NoBand {};
constexpr int kFloatReach = 2;
constexpr int kFloatRecordWords = 8;      // id, x, y, k1x, k1y, xs, ys, rejected: 64 bytes

template <class C>
__device__ __forceinline__ bool flt_locate(C &c, const DevView &d, const FloatView &f, const NoBand &, double fx, double fy) {
    return flt_locate(c, d, f, fx, fy);
}
// r = global row - own0 brought next to the owned rows: 0 .. nown-1 owned, below / above = the ghost sides
__device__ __forceinline__ int flt_band_rel(const FloatBand &fb, int g) {
    int r = g - fb.own0;
    if (fb.nring) {
        if (r < 0) r += fb.nring;
        if (r >= fb.nown && r >= fb.nring - fb.gs) r -= fb.nring;
    }
    return r;
}
__device__ __forceinline__ bool flt_locate(CellDense &c, const DevView &d, const FloatView &, const FloatBand &fb, double fx, double fy) {
    if (!(fx >= 0.0 && fx < (double)d.L && fy >= 0.0 && fy < (double)fb.Mf)) return false;
    if (fb.nring && (int)fy >= fb.nring) return false;          // the ring's row mm + 1: dry, and no wet cell's neighbour
    const int jl = fb.gs + 1 + flt_band_rel(fb, (int)fy + 1);
    if (jl < fb.lo || jl > fb.hi) { atomicAdd(&fb.stats[0], 1ull); return false; }
    c.set_cell(d, (int)fx + 1, jl);
    return true;
}
// is floor(y) + 1 one of the band's owned rows?
__device__ __forceinline__ bool flt_owned(const FloatBand &fb, double y) {
    const double fy = floor(y);
    if (!(fy >= 0.0 && fy < (double)(fb.nring ? fb.nring : fb.Mf))) return false;
    int r = (int)fy + 1 - fb.own0;
    if (fb.nring && r < 0) r += fb.nring;
    return r >= 0 && r < fb.nown;
}

// wet(x, y); p = the home cell's device index if wet (else untouched).  B = NoBand: a handle of the whole frame; FloatBand: a band
template <class C, class B>
__device__ __forceinline__ bool flt_wet(const DevView &d, const FloatView &f, const B &fb, double x, double y, int &p) {
    C c;
    if (!flt_locate(c, d, f, fb, floor(x), floor(y))) return false;
    if (!(c.mk_n() > 0.5)) return false;
    p = c.ipnt;
    return true;
}
template <class C, class B>
__device__ __forceinline__ void flt_velocity(const DevView &d, const FloatView &f, const B &fb, double x, double y, int l, double &U, double &V) {
    const double fx = floor(x), fy = floor(y);
    const double a = x - fx, b = y - fy;
    C c;
    int p = 0, e = 0, n = 0;
    if (flt_locate(c, d, f, fb, fx, fy)) { p = c.ipnt; e = c.template nb<1>(); n = c.template nb<3>(); }
    U = (1.0 - a) * LL(d.u, p, l) + a * LL(d.u, e, l);
    V = (1.0 - b) * LL(d.v, p, l) + b * LL(d.v, n, l);
}
template <class C, class B>
__device__ __forceinline__ void flt_stage1(const DevView &d, const FloatView &f, const B &fb, long long t, double x, double y, int l) {
    double U, V;
    flt_velocity<C>(d, f, fb, x, y, l, U, V);
    const double k1x = U * f.cdt, k1y = V * f.cdt;
    double xs = flt_wrap(x + k1x, f.flm, f.xper), ys = flt_wrap(y + k1y, f.fmm, f.yper);
    int p;
    if (!flt_wet<C>(d, f, fb, xs, ys, p)) { xs = x; ys = y; }
    f.k1x[t] = k1x; f.k1y[t] = k1y; f.xs[t] = xs; f.ys[t] = ys;
}
template <class C, class B>
__device__ __forceinline__ void flt_stage2(const DevView &d, const FloatView &f, const B &fb, long long t, double &x, double &y, int l) {
    const double k1x = f.k1x[t], k1y = f.k1y[t];
    double U, V;
    flt_velocity<C>(d, f, fb, f.xs[t], f.ys[t], l, U, V);
    const double k2x = U * f.cdt, k2y = V * f.cdt;
    double xn = flt_wrap(x + 0.5 * (k1x + k2x), f.flm, f.xper), yn = flt_wrap(y + 0.5 * (k1y + k2y), f.fmm, f.yper);
    int p = 0;
    if (!flt_wet<C>(d, f, fb, xn, yn, p)) {          // the rare lanes: the landing rule's other candidates
        if (flt_wet<C>(d, f, fb, xn, y, p)) yn = y;
        else if (flt_wet<C>(d, f, fb, x, yn, p)) xn = x;
        else { xn = x; yn = y; (void)flt_wet<C>(d, f, fb, x, y, p); }
        f.rejected[t] = f.rejected[t] + 1;
    }
    x = xn; y = yn;
    f.x[t] = xn; f.y[t] = yn;
    if (f.rec) { f.rec[t] = xn; f.rec[f.n + t] = yn; f.rec[2 * f.n + t] = LL(d.hlay, p, l); }
}

// MODE 1: stage 1 alone (in front of the first step of a call), 2: stage 2 alone (behind the last),
// 3: stage 2 of a step, then stage 1 of the next on the same velocities
template <class C, int MODE>
__global__ __launch_bounds__(BEOM_BLOCK) void k_floats(DevView d, FloatView f) {
    const long long t = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x;
    if (t >= f.n) return;
    double x = f.x[t], y = f.y[t];
    const int l = f.layer[t];
    if (MODE & 2) flt_stage2<C>(d, f, NoBand{}, t, x, y, l);
    if (MODE & 1) flt_stage1<C>(d, f, NoBand{}, t, x, y, l);
}

// beom_upload_floats: the smallest index of a float whose start position (xs, ys hold the candidates) is not wet
template <class C>
__global__ __launch_bounds__(BEOM_BLOCK) void k_floats_check(DevView d, FloatView f, unsigned long long *first_dry) {
    const long long t = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x;
    if (t >= f.n) return;
    int p;
    if (!flt_wet<C>(d, f, NoBand{}, f.xs[t], f.ys[t], p)) atomicMin(first_dry, (unsigned long long)t);
}

// ---- the band's side of a hand-over --------------------------------------------------------------------------------------------
// one record into an outbox, as four aligned 16-byte stores; a full outbox drops it and counts
__device__ __forceinline__ void flt_hand_over(const FloatView &f, const FloatBand &fb, long long t, double x, double y) {
    int r = (int)floor(y) + 1 - fb.own0;                        // (y is wet: inside the frame)
    bool north = r > 0;
    if (fb.nring) { if (r < 0) r += fb.nring; north = r - fb.nown < fb.nring - r; }
    unsigned long long *box = north ? fb.box_n : fb.box_s;
    if (!box) { atomicAdd(&fb.stats[0], 1ull); return; }        // (no neighbour on that side: cannot be, the row is in the frame)
    const unsigned long long slot = atomicAdd(box, 1ull);
    if (slot >= (unsigned long long)fb.capacity) { atomicAdd(&fb.stats[1], 1ull); return; }
    ulonglong2 *rec = (ulonglong2 *)(box + kFloatRecordWords * (slot + 1));
    rec[0] = make_ulonglong2((unsigned long long)t, (unsigned long long)__double_as_longlong(x));
    rec[1] = make_ulonglong2((unsigned long long)__double_as_longlong(y), (unsigned long long)__double_as_longlong(f.k1x[t]));
    rec[2] = make_ulonglong2((unsigned long long)__double_as_longlong(f.k1y[t]), (unsigned long long)__double_as_longlong(f.xs[t]));
    rec[3] = make_ulonglong2((unsigned long long)__double_as_longlong(f.ys[t]), (unsigned long long)(unsigned)f.rejected[t]);
}

// the band form of k_floats (bands are dense handles: CellDense).  Lanes whose float lives elsewhere read y[t] and leave.
template <int MODE>
__global__ __launch_bounds__(BEOM_BLOCK) void k_floats_band(DevView d, FloatView f, FloatBand fb) {
    const long long t = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x;
    if (t >= f.n) return;
    double y = f.y[t];
    if (!flt_owned(fb, y)) return;
    double x = f.x[t];
    const int l = f.layer[t];
    if (MODE & 2) flt_stage2<CellDense>(d, f, fb, t, x, y, l);
    if (MODE & 1) flt_stage1<CellDense>(d, f, fb, t, x, y, l);
    if ((MODE & 2) && !flt_owned(fb, y)) flt_hand_over(f, fb, t, x, y);
}

__global__ __launch_bounds__(BEOM_BLOCK) void k_floats_check_band(DevView d, FloatView f, FloatBand fb, unsigned long long *first_dry) {
    const long long t = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x;
    if (t >= f.n) return;
    const double y = f.ys[t];
    if (!flt_owned(fb, y)) return;
    int p;
    if (!flt_wet<CellDense>(d, f, fb, f.xs[t], y, p)) atomicMin(first_dry, (unsigned long long)t);
}

// the neighbour side: blockIdx.y = 0 / 1 takes the inbox copied from the south / north neighbour's outbox; thread i < count
// writes record i into slot id.  The launch sits behind the neighbours' copies of THIS band's outboxes (stream events), so
// its first thread also empties them for the next float launch.
__global__ __launch_bounds__(BEOM_BLOCK) void k_floats_ingest(FloatView f, FloatBand fb, const unsigned long long *in_s, const unsigned long long *in_n) {
    const unsigned long long *in = blockIdx.y ? in_n : in_s;
    const long long i = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x;
    if (i == 0) {
        unsigned long long *own = blockIdx.y ? fb.box_n : fb.box_s;
        if (own) own[0] = 0ull;
    }
    if (!in) return;
    unsigned long long cnt = in[0];
    if (cnt > (unsigned long long)fb.capacity) cnt = (unsigned long long)fb.capacity;
    if ((unsigned long long)i >= cnt) return;
    if (i == 0) atomicAdd(&fb.stats[2], cnt);
    const ulonglong2 *rec = (const ulonglong2 *)(in + kFloatRecordWords * (i + 1));
    const ulonglong2 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    const long long t = (long long)r0.x;
    if (t < 0 || t >= f.n) return;
    f.x[t] = __longlong_as_double((long long)r0.y);
    f.y[t] = __longlong_as_double((long long)r1.x);
    f.k1x[t] = __longlong_as_double((long long)r1.y);
    f.k1y[t] = __longlong_as_double((long long)r2.x);
    f.xs[t] = __longlong_as_double((long long)r2.y);
    f.ys[t] = __longlong_as_double((long long)r3.x);
    f.rejected[t] = (int32_t)(unsigned)r3.y;
}
