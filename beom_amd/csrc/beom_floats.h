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

// wet(x, y); p = the home cell's device index if wet (else untouched)
template <class C>
__device__ __forceinline__ bool flt_wet(const DevView &d, const FloatView &f, double x, double y, int &p) {
    C c;
    if (!flt_locate(c, d, f, floor(x), floor(y))) return false;
    if (!(c.mk_n() > 0.5)) return false;
    p = c.ipnt;
    return true;
}

template <class C>
__device__ __forceinline__ void flt_velocity(const DevView &d, const FloatView &f, double x, double y, int l, double &U, double &V) {
    const double fx = floor(x), fy = floor(y);
    const double a = x - fx, b = y - fy;
    C c;
    int p = 0, e = 0, n = 0;
    if (flt_locate(c, d, f, fx, fy)) { p = c.ipnt; e = c.template nb<1>(); n = c.template nb<3>(); }
    U = (1.0 - a) * LL(d.u, p, l) + a * LL(d.u, e, l);
    V = (1.0 - b) * LL(d.v, p, l) + b * LL(d.v, n, l);
}

template <class C>
__device__ __forceinline__ void flt_stage1(const DevView &d, const FloatView &f, long long t, double x, double y, int l) {
    double U, V;
    flt_velocity<C>(d, f, x, y, l, U, V);
    const double k1x = U * f.cdt, k1y = V * f.cdt;
    double xs = flt_wrap(x + k1x, f.flm, f.xper), ys = flt_wrap(y + k1y, f.fmm, f.yper);
    int p;
    if (!flt_wet<C>(d, f, xs, ys, p)) { xs = x; ys = y; }
    f.k1x[t] = k1x; f.k1y[t] = k1y; f.xs[t] = xs; f.ys[t] = ys;
}

template <class C>
__device__ __forceinline__ void flt_stage2(const DevView &d, const FloatView &f, long long t, double &x, double &y, int l) {
    const double k1x = f.k1x[t], k1y = f.k1y[t];
    double U, V;
    flt_velocity<C>(d, f, f.xs[t], f.ys[t], l, U, V);
    const double k2x = U * f.cdt, k2y = V * f.cdt;
    double xn = flt_wrap(x + 0.5 * (k1x + k2x), f.flm, f.xper), yn = flt_wrap(y + 0.5 * (k1y + k2y), f.fmm, f.yper);
    int p = 0;
    if (!flt_wet<C>(d, f, xn, yn, p)) {          // the rare lanes: the landing rule's other candidates
        if (flt_wet<C>(d, f, xn, y, p)) yn = y;
        else if (flt_wet<C>(d, f, x, yn, p)) xn = x;
        else { xn = x; yn = y; (void)flt_wet<C>(d, f, x, y, p); }
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
    if (MODE & 2) flt_stage2<C>(d, f, t, x, y, l);
    if (MODE & 1) flt_stage1<C>(d, f, t, x, y, l);
}

// beom_upload_floats: the smallest index of a float whose start position (xs, ys hold the candidates) is not wet
template <class C>
__global__ __launch_bounds__(BEOM_BLOCK) void k_floats_check(DevView d, FloatView f, unsigned long long *first_dry) {
    const long long t = (long long)blockIdx.x * BEOM_BLOCK + threadIdx.x;
    if (t >= f.n) return;
    int p;
    if (!flt_wet<C>(d, f, f.xs[t], f.ys[t], p)) atomicMin(first_dry, (unsigned long long)t);
}
