// beom_engine.hip — C-ABI of include/beom_hip.h: device state, uploads/downloads, the
// step driver (integrate_time / first_three_timesteps / gener_forward_backward of the
// reference, private_mod.f95:1840-1919, 2151-2316) and kernel launches.
// No CPU fallback exists: every entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "beom_dev.h"
#include "beom_kernels.h"
#include "beom_integrals.h"
#include "beom_series.h"
#include "beom_tracers.h"
#include "beom_tracers_lim.h"
#include "beom_tracer_mix.h"
#include "beom_tracer_vmix.h"
#include "beom_floats.h"
#include "beom_moments.h"
#include "beom_harmonics.h"
#include "beom_tracer_moments.h"
#include "beom_tracer_series.h"
#include "beom_forcing.h"
#include "beom_dense_host.h"
#include "beom_plan.h"
#include "beom_recorder.h"
#include "beom_column_series.h"      // (behind every earlier header: the kernels before it keep their place in the code object)
#include "beom_tracer_column_series.h"      // (behind it, for the same reason)
#include "beom_maps.h"      // (last, for the same reason)

using beom_plan::StepFacts;
using beom_plan::StepPlan;

namespace {

void set_err(char *errm, int len, const char *fmt, ...) {
    if (!errm || len <= 0) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(errm, (size_t)len, fmt, ap);
    va_end(ap);
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            set_err(errm, errm_len, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                    __FILE__, __LINE__);                                                    \
            return -100 - (int)e_;                                                          \
        }                                                                                   \
    } while (0)

}  // namespace

constexpr int kLidBatch = 256;  // rigid lid: at most this many Gauss-Seidel sweeps in flight at once (lid_solve)

struct StepTimer {        // optional HIP-event bracket around each kernel class
    std::vector<hipEvent_t> ev; std::vector<int> cls;
    hipStream_t st;
    int stride = 1;       // only the steps with tstp % stride == 0 are bracketed (an event pair costs a few us of pipeline bubble)
    // rotate: a sampled step brackets ONE kind of sweep only — update_h | Montgomery, viscosity | momentum — by turns
    // ((tstp / stride) % 3), so no bracketed launch has another bracket's bubble in front of it
    bool rotate = false;
    int slot = -1;        // the kind this step brackets (-1: all)
    bool open = false;
    static int kind(int c) { return c == 0 ? 0 : (c == 1 || c == 2 || c == 5) ? 1 : 2; }
    void step(int tstp) { slot = rotate ? (tstp / stride) % 3 : -1; }
    void begin(int c) {
        open = slot < 0 || kind(c) == slot;
        if (!open) return;
        hipEvent_t a; (void)hipEventCreate(&a); (void)hipEventRecord(a, st); ev.push_back(a); cls.push_back(c);
    }
    void end() { if (!open) return; hipEvent_t b; (void)hipEventCreate(&b); (void)hipEventRecord(b, st); ev.push_back(b); open = false; }
};

// A time accumulator kept on the device: field moments and tracer moments share everything on the host but their kernels.
// The constant part: how many quantities have a reference and a shifted sum at level 1 and at levels 2 and 3, how many
// second moments level 3 adds, whether an array has the tracers' shape (else the state's), and the texts of the refusals.
struct AccumKind {
    int n1, n2, nsq;
    bool per_tracer;
    const char *bad_args, *no_tracer, *none, *no_sq;      // (no_tracer: null where no tracer is needed)
};
constexpr AccumKind kFieldMoments{3, 5, 5, false,
    "beom_set_moments: level %d, stride %d (level 0..3, stride >= 1)", nullptr,
    "beom_download_moments: the handle keeps no moments (beom_set_moments)",
    "beom_download_moments: the second moments are kept at level 3, this handle has level %d"};
constexpr AccumKind kTracerMoments{2, 4, 1, true,
    "beom_set_tracer_moments: level %d, stride %d (level 0..3, stride >= 1)",
    "beom_set_tracer_moments: the handle carries no tracer (beom_set_tracers comes first)",
    "beom_download_tracer_moments: the handle keeps no tracer moments (beom_set_tracer_moments)",
    "beom_download_tracer_moments: the second moment is kept at level 3, this handle has level %d"};
struct Accum {
    const AccumKind *kind;
    int level = 0, stride = 1;
    long long count = 0, launches = 0; // samples since the last reset | all launches so far
    int first = 0, last = 0;           // the steps of the first and the latest sample
    double *ref[5] = {}, *sum[5] = {}, *sq[5] = {};
    std::vector<void *> allocs;
};
static bool accum_due(const Accum &A, int tstp) { return A.level > 0 && tstp % A.stride == 0; }
static void accum_note_sample(Accum &A, int tstp) {      // the tail of a sample's launch
    if (A.count == 0) A.first = tstp;
    A.last = tstp;
    ++A.count;
    ++A.launches;
}

// The harmonic analysis (beom_set_harmonics; beom_harmonics.h): an accumulator whose sums are 1 + 2K per field.  acc carries
// level (1 | 2; 0 = none), stride, count, the steps and ref[f]; the normal matrix of the fit is kept here, on the host.
struct Harmonics {
    Accum acc{nullptr};
    int nfreq = 0;
    double omega[BEOM_MAX_HARMONICS] = {};
    double *sum[5][1 + 2 * BEOM_MAX_HARMONICS] = {};
    double gram[(1 + 2 * BEOM_MAX_HARMONICS) * (1 + 2 * BEOM_MAX_HARMONICS)] = {};      // (1+2K)^2 in use, row-major
};

// A recorder kept on the device, [nrec][rows][cnt] with the step of every held record: the series and the tracer series
// share everything on the host but their kernels.  The constant part: the highest level, the entries per row of a frame with
// ntrc tracers and nlay layers at a level, how the chunk partials of a launch are obtained (with the cell map, in the kind's
// own order), the launch of one record, and the texts (no_tracer, which takes the caller's name: null where no tracer is needed).
struct Recorder;
struct RecorderKind {
    int max_level;
    int (*count)(int ntrc, int nlay, int level);
    int (*scratch)(beom_engine *, Recorder &, int cnt, int nrows, char *errm, int errm_len);
    void (*launch)(beom_engine *, int tstp);
    const char *no_tracer, *none, *overflow;
    bool columns = false;              // the recorder's lines are the L columns, and jlo .. jlo+nrows-1 is its row window
    const char *what = nullptr;        // (columns) its name in the refusal of a handle on a band of rows
    int (*lines)(const beom_engine *) = nullptr;      // the maps: the lines of a record, where they are neither rows nor columns
};
static int series_scratch(beom_engine *E, Recorder &R, int cnt, int nrows, char *errm, int errm_len);
static int tracer_series_scratch(beom_engine *E, Recorder &R, int cnt, int nrows, char *errm, int errm_len);
static void launch_series(beom_engine *E, int tstp);
static void launch_tracer_series(beom_engine *E, int tstp);
static int column_series_scratch(beom_engine *E, Recorder &R, int cnt, int ncols, char *errm, int errm_len);
static void launch_column_series(beom_engine *E, int tstp);
static int tracer_column_series_scratch(beom_engine *E, Recorder &R, int cnt, int ncols, char *errm, int errm_len);
static void launch_tracer_column_series(beom_engine *E, int tstp);
static int maps_scratch(beom_engine *E, Recorder &R, int cnt, int nlines, char *errm, int errm_len);
static void launch_maps(beom_engine *E, int tstp);
static int maps_lines(const beom_engine *E);
constexpr RecorderKind kSeries{2, [](int, int nlay, int level) { return beom_series_count(nlay, level); },
    series_scratch, launch_series, nullptr,
    "beom_download_series: the handle keeps no series (beom_set_series)",
    "beom_step: steps %d..%d would write %lld records of the series (stride %d) but the recorder holds %lld of %d: "
    "empty it with beom_download_series, or take fewer steps per call"};
constexpr RecorderKind kTracerSeries{3, beom_tracer_series_count,
    tracer_series_scratch, launch_tracer_series,
    "%s: the handle carries no tracer (beom_set_tracers comes first)",
    "beom_download_tracer_series: the handle keeps no tracer series (beom_set_tracer_series)",
    "beom_step: steps %d..%d would write %lld records of the tracer series (stride %d) but the recorder holds %lld of %d: "
    "empty it with beom_download_tracer_series, or take fewer steps per call"};
constexpr RecorderKind kColumnSeries{2, [](int, int nlay, int level) { return beom_series_count(nlay, level); },
    column_series_scratch, launch_column_series, nullptr,
    "beom_download_column_series: the handle keeps no column series (beom_set_column_series)",
    "beom_step: steps %d..%d would write %lld records of the column series (stride %d) but the recorder holds %lld of %d: "
    "empty it with beom_download_column_series, or take fewer steps per call", true, "column series"};
constexpr RecorderKind kTracerColumnSeries{3, beom_tracer_series_count,
    tracer_column_series_scratch, launch_tracer_column_series,
    "%s: the handle carries no tracer (beom_set_tracers comes first)",
    "beom_download_tracer_column_series: the handle keeps no tracer column series (beom_set_tracer_column_series)",
    "beom_step: steps %d..%d would write %lld records of the tracer column series (stride %d) but the recorder holds %lld of %d: "
    "empty it with beom_download_tracer_column_series, or take fewer steps per call", true, "tracer column series"};
constexpr RecorderKind kMaps{3, beom_maps_count, maps_scratch, launch_maps, nullptr,
    "beom_download_maps: the handle keeps no maps (beom_set_maps)",
    "beom_step: steps %d..%d would write %lld records of the maps (stride %d) but the recorder holds %lld of %d: "
    "empty it with beom_download_maps, or take fewer steps per call", false, nullptr, maps_lines};
struct Recorder {
    const RecorderKind *kind;
    int level = 0, stride = 1, nrec = 0, jlo = 1, rows = 0;      // local rows jlo .. jlo+rows-1
    bool by_caller = false;            // a band: beom_step takes no record by itself (beom_band_set_series and its like)
    double *rec = nullptr;
    std::vector<int> tstp;             // the step of every held record (its size = the records held)
    double *part = nullptr;            // the tracer series: the chunk partials of `batch` rows at a time (kTracerSeriesScratch)
    int batch = 0;                     // (the column series: the block partials of `batch` 64-column chunks at a time)
    int wlo = 1, whi = 0;              // the column series: the row window
    std::vector<void *> allocs;
};
static bool recorder_due(const Recorder &R, int tstp) { return R.level > 0 && tstp % R.stride == 0 && (int)R.tstp.size() < R.nrec; }

// A frame set of one field (beom_set_forcing; beom_forcing.h): the frames in the device layout, the buffer the sweeps read
// (x; xc: the cells-only copy of taus) and the weight of the last launch, which a step with the same weight leaves out.
struct ForcingSet {
    int nfr = 0;
    double period = 0.0;
    std::vector<double> times;
    std::vector<double *> frames;
    double *x = nullptr, *xc = nullptr;
    int k0 = -1, k1 = -1;
    double a = 0.0;
    std::vector<void *> allocs;
};

struct beom_engine {
    beom_params P;
    int device = 0;
    hipStream_t stream = nullptr;      // stream in use (own_stream unless beom_set_stream)
    hipStream_t own_stream = nullptr;
    StepTimer *timer = nullptr;        // non-null between beom_profile_start/stop
    DevView d{};
    bool dense = false;
    std::vector<void *> allocs;
    const int32_t *slot_of_dev = nullptr;   // embedded frames: packed index -> slot (device copy; null otherwise)
    bool embedded = false;
    void *stage = nullptr;             // device image of ONE caller-layout slice [0:ndeg] (<= 32 B per cell) for uploads / downloads
    size_t stage_bytes = 0;
    // geometry of the launches
    dim3 grid_cells0, grid_cells_layers_flat;
    bool wind = false, bot = false, top = false;
    // distribute_stress inside the fused momentum sweep (option "fold_stress", default on): possible when the fractions are
    // constants (ocrp = 0) and nothing the sweep would have to read was uploaded into an array the engine does not refresh
    bool fold_stress = true, fold_static_ok = false;
    bool up_tt = false, up_tb = false, up_tu = false;   // a non-zero tt3d / tb3d / tu3d has been uploaded
    bool last_folded = false;          // the last step formed its stress inside the momentum sweep (beom_info "stress_folded")
    bool last_uv_fused = false;        // the last step's momentum ran as the fused u+v sweep (beom_info "uv_fused")
    float *h0r4_dev = nullptr, *out4[3] = {nullptr, nullptr, nullptr};   // device-side output staging
    float *diag4[3] = {nullptr, nullptr, nullptr};
    double *scan_dev = nullptr;
    int any_u = 0, any_v = 0;
    long long uniform_waves = 0, total_waves = 0;   // table path: runs of 64 cells handled by offset arithmetic
    bool obc = false;                  // no_gradient_obc active (flag_nudging, mcbc < 0.5, segments set)
    bool obc_set = false;              // beom_set_open_boundaries has been called (a band may hold no segment at all)
    bool fuse = true;                  // dense frames: Montgomery+Leith in one sweep (k_mont_visc)
    bool fuse_uv = true;               // dense frames: update_u + update_v in one sweep (k_uv_fused)
    bool lean_visc = true;             // zero viscosity (dvis = bvis = 0, v_cc = v_ll = +0): fused pair drops the viscous products
    bool visc_all_zero = true;         // no non-(+0) v_cc / v_ll has been uploaded
    bool lean_d2h = true;              // fused pair: d2hx, d2hy re-derived from hlay in k_uv_fused, not stored by k_mont_visc
    // rigid lid (rgld = 1): the caller's subc and the packed -> device index map, kept for beom_set_rigid_lid
    std::vector<int32_t> subc_host, neig_host, dev_index;
    bool lid = false, lid_ready = false;
    // the lid's Gauss-Seidel pipeline (k_rgld_gs_front): time between two sweeps, ring of pressure copies, per-sweep max |change|
    int lid_dstep = 2, lid_nring = 0, lid_maxwidth = 1;
    double *lid_ring = nullptr;
    unsigned long long *lid_maxd = nullptr;
    long long lid_sweeps = 0, lid_solves = 0, lid_launches = 0;    // statistics (beom_info)
    int lid_last = 0;                  // sweeps the last solve kept
    int profile_stride = 1;            // option "profile_stride"
    bool profile_rotate = false;       // option "profile_rotate"
    StepPlan split{};                  // split steps: the plan part 1 made of its step (tstp 0: none yet); parts 2 and 3 run from it
    bool tile4 = false;                // the tiled sweeps run the 64 x 4 geometry (frames of one or two rounds of workgroups)
    // History from Montgomery (option "mont_history", default on): d.mont rotates through four buffers, once
    // per step (rotate_mont), and the fused u+v sweep re-forms dmx / dmy from the three kept levels instead of reading them.
    bool mont_history = true;
    bool mont_keep = false;            // the handle has the three extra buffers (whole dense frame, no lid, g_fb != 0, fusable)
    int mont_levels_valid = 0;         // consecutive steps, up to the last one, whose Montgomery potential the buffers hold
    bool hist_stale = false;           // dmx, dmy lag behind: steps of the new form have left them alone (hist_sync)
    bool last_mont_hist = false;       // the last step ran the new form (beom_info "mont_history")
    // Plain sweeps (option "plain_sweeps", default on): a launch of the fused u+v sweep resp. of the Montgomery
    // sweep whose handle has none of the optional forcing takes the instantiation with that forcing compiled out.  Decided
    // per step by plan_step (beom_plan.h) from the facts of the moment (keep_diag, uploaded stress and options change between steps).
    bool plain_sweeps = true;
    int last_plain = 0;                // bit 0: the last step's u+v sweep ran plain, bit 1: its Montgomery sweep (beom_info "plain_sweeps")
    // conservation integrals (beom_integral_rows): chunk sums and row sums of up to M rows, allocated on the first call; on
    // the table path also the packed cell of every (i, j) and the wraps read off neig
    double *integ_part = nullptr, *integ_rows = nullptr;
    int integ_count = 0;               // entries per row the two are sized for (the series at level 2 asks for more)
    int32_t *integ_cellmap = nullptr;
    int integ_xper = 0, integ_yper = 0;
    // passive tracers (beom_set_tracers; beom_tracers.h): the contents and the partner the sweep writes them to, the two
    // tendency levels (rotated by pointer), the relaxation concentration (allocated by its first upload)
    int ntrc = 0;
    int trc_scheme = 1;                // 1 = upstream (k_tracers), 2 = flux-limited (k_tracers_lim); beom_set_tracer_scheme
    double *trc_q = nullptr, *trc_q_alt = nullptr, *trc_rq[2] = {nullptr, nullptr}, *trc_ctrg = nullptr;
    std::vector<void *> trc_allocs;
    // lateral diffusion, decay and sources of the tracers (beom_set_tracer_mixing; beom_tracer_mix.h): the coefficients
    // [3][ntrc][nlay] on the device, null while mixing is off; the launches so far
    double *trc_mix = nullptr;
    std::vector<void *> trc_mix_allocs;
    long long trc_mix_launches = 0;
    // vertical diffusion of the tracers between the layers (beom_set_tracer_vmixing; beom_tracer_vmix.h): rk = 1 / (dt *
    // kappa_v), [ntrc][nlay-1] on the device, null while it is off; the launches so far
    double *trc_vmix = nullptr;
    std::vector<void *> trc_vmix_allocs;
    long long trc_vmix_launches = 0;
    // Lagrangian floats (beom_set_floats; beom_floats.h): positions, layers, rejected steps, stage 1's increment and
    // provisional position; the track recorder [record][3][float] with the step of every held record
    long long nflt = 0;
    bool flt_ready = false;            // positions have been uploaded
    double *flt_x = nullptr, *flt_y = nullptr, *flt_k1x = nullptr, *flt_k1y = nullptr, *flt_xs = nullptr, *flt_ys = nullptr;
    int32_t *flt_layer = nullptr, *flt_rej = nullptr;
    unsigned long long *flt_first_dry = nullptr;
    double *flt_rec = nullptr;
    int flt_nrec = 0, flt_stride = 1;
    std::vector<int> flt_rec_tstp;     // (its size = the records held)
    long long flt_launches = 0;        // beom_info "float_launches"
    bool cellmap_known = false;        // integ_cellmap (table path) and integ_xper / integ_yper are set
    std::vector<void *> flt_allocs;
    // floats on a band of rows (beom_band_floats_*): the same arrays hold ALL floats of the frame; the band's rows, its two
    // outboxes and inboxes (count + capacity records each) and the three device counts
    bool flt_band = false;
    FloatBand flt_fb{};
    unsigned long long *flt_in_s = nullptr, *flt_in_n = nullptr;
    int flt_xper = 0, flt_yper = 0;
    double flt_fmm = 0.0;
    long long flt_handovers = 0;       // beom_info "float_handovers": records ingested, as the latest download read it
    // moments (beom_set_moments; beom_moments.h): per field the reference, the shifted sum and, at level 3, the shifted
    // second moment, in arrays of the state's shape; the steps of the first and the latest sample
    Accum mom{&kFieldMoments};
    bool mom_by_caller = false;        // option "moments_by_caller": beom_step takes no sample by itself
    int last_tstp = 0;                 // the last step taken (beom_step, beom_step_phase)
    // tracer moments (beom_set_tracer_moments; beom_tracer_moments.h): per quantity q, c, fu, fv the reference and the shifted
    // sum, at level 3 the shifted second moment of c, in arrays of the tracers' shape; level, stride and count of their own
    Accum tmom{&kTracerMoments};
    // harmonics (beom_set_harmonics; beom_harmonics.h): per field the reference and 1 + 2K shifted sums in arrays of the
    // state's shape, the normal matrix on the host; "moments_by_caller" governs their samples too
    Harmonics harm;
    // series (beom_set_series; beom_series.h): the row sums of the recorder's rows, one record behind every step with
    // tstp % stride == 0
    Recorder ser{&kSeries};
    // tracer series (beom_set_tracer_series; beom_tracer_series.h): a recorder [nrec][rows][ntrc*nlay*2*level] of its own,
    // with level, stride and rows of its own
    Recorder tser{&kTracerSeries};
    int tser_batch_opt = 0;            // option "tracer_series_batch": rows per launch (0 = by the bound on the scratch)
    // column series (beom_set_column_series; beom_column_series.h): a recorder [nrec][L][cnt] whose lines are the columns, with
    // level, stride, row window and scratch of its own
    Recorder cser{&kColumnSeries};
    int cser_batch_opt = 0;            // option "column_series_batch": 64-column chunks per launch (0 = by the bound on the scratch)
    // tracer column series (beom_set_tracer_column_series; beom_tracer_column_series.h): a recorder [nrec][L][ntrc*nlay*2*level]
    // whose lines are the columns, with level, stride, row window and scratch of its own
    Recorder tcser{&kTracerColumnSeries};
    // maps (beom_set_maps; beom_maps.h): a recorder [nrec][cnt][Mc][Lc] of sums over aligned blocks of 2^maps_logb cells a
    // side, whose lines are the Mc * Lc blocks; no scratch
    Recorder maps{&kMaps};
    int maps_logb = 0;
    long long map_launches = 0;
    int tcser_batch_opt = 0;           // option "tracer_column_series_batch": 64-column chunks per launch (0 = by the bound on the scratch)
    // forcing in time (beom_set_forcing; beom_forcing.h): frc[0] the wind stress, frc[1] hdot; what beom_create gave, to
    // return to when a set is cleared; a body force of exactly -0 (it bars the folded stress, see derive_forcing_flags)
    ForcingSet frc[2];
    long long frc_launches = 0;        // beom_info "forcing_launches"
    const double *taus0 = nullptr, *taus_cells0 = nullptr, *hdot0 = nullptr;
    bool wind0 = false, has_hdot0 = false, bodf_neg0 = false;
    char last_err[512] = {0};
};
static int hist_sync(beom_engine *E);
static int leave_mont_history(beom_engine *E);

namespace {

// A device array of n elements, zeroed unless told otherwise, owned by `owner` (free_list).
template <class T>
int alloc_plain(beom_engine *E, std::vector<void *> &owner, T **p, size_t n, char *errm, int errm_len, bool zero = true) {
    void *q = nullptr;
    HIP_TRY(hipMalloc(&q, n * sizeof(T)));
    owner.push_back(q);
    if (zero) HIP_TRY(hipMemsetAsync(q, 0, n * sizeof(T), E->stream));
    *p = (T *)q;
    return 0;
}
// Device arrays of doubles start kLead elements into their allocation so that cell index 1 is 128-byte
// aligned (hipMalloc aligns to 256 B); see DevView::P.  n + kLead + 1 elements are allocated.
constexpr size_t kLead = 15;
template <class T>
int alloc_aligned(beom_engine *E, std::vector<void *> &owner, T **p, size_t n, char *errm, int errm_len, bool zero = true) {
    const int rc = alloc_plain(E, owner, p, n + kLead + 1, errm, errm_len, zero);
    if (!rc) *p += kLead;
    return rc;
}
void free_list(std::vector<void *> &owner) {
    for (void *p : owner) (void)hipFree(p);
    owner.clear();
}
template <class T>
int dev_alloc(beom_engine *E, T **p, size_t n, char *errm, int errm_len, bool zero = true) {
    return sizeof(T) == 8 ? alloc_aligned(E, E->allocs, p, n, errm, errm_len, zero) : alloc_plain(E, E->allocs, p, n + 1, errm, errm_len, zero);
}
// elements of an array of the state's shape [nlay][n1] and of the tracers' shape [ntrc][nlay][n1]
size_t state_cells(const beom_engine *E) { return (size_t)E->d.nlay * (size_t)E->d.n1; }
size_t tracer_cells(const beom_engine *E) { return (size_t)E->ntrc * state_cells(E); }

int pow2_ceil(int n) { int p = 1; while (p < n) p <<= 1; return p; }
// The tree over a row of L columns (beom_integrals.h): chunks of 64 columns, their count padded to a power of two, and the
// lanes the first level of a chunk's own tree spans.
struct RowTree { int nch, nchp2, width; };
RowTree row_tree(int L) { return {(L + 63) / 64, pow2_ceil((L + 63) / 64), std::min(64, pow2_ceil(L))}; }

// one slice [0:ndeg][inner] (x K interleaved levels, level m) of a caller array <-> its device array
template <class T, bool REMAP = false>
int slice_to_device(beom_engine *E, T *dev, const T *host, int inner, int K, int m, char *errm, int errm_len) {
    const DevView &d = E->d;
    const size_t n = ((size_t)d.ndeg + 1) * inner * K;
    if (n * sizeof(T) > E->stage_bytes) { set_err(errm, errm_len, "internal: staging buffer too small"); return -11; }
    if (host) HIP_TRY(hipMemcpyAsync(E->stage, host, n * sizeof(T), hipMemcpyHostToDevice, E->stream));   // nullptr: the image is there already
    const long long work = ((long long)d.ndeg + 1) * inner;
    if (E->embedded) {                 // land slots: the sentinel's value of this slice
        const long long all = (d.ncell + 1) * inner;
        hipLaunchKernelGGL((k_fill_sentinel<T>), dim3((unsigned)((all + BEOM_BLOCK - 1) / BEOM_BLOCK)), dim3(BEOM_BLOCK), 0, E->stream,
                           dev, (const T *)E->stage, d.ncell + 1, inner, K, m);
    }
    hipLaunchKernelGGL((k_repack<T, true, REMAP>), dim3((unsigned)((work + BEOM_BLOCK - 1) / BEOM_BLOCK)), dim3(BEOM_BLOCK), 0, E->stream,
                       dev, (T *)E->stage, (long long)d.ndeg, d.L, d.P ? d.P : d.L, inner, K, m, E->slot_of_dev);
    return 0;
}
template <class T>
int slice_to_host(beom_engine *E, const T *dev, T *host, int inner, int K, char *errm, int errm_len) {   // all K levels: dev[m]
    (void)dev;
    const DevView &d = E->d;
    const size_t n = ((size_t)d.ndeg + 1) * inner * K;
    HIP_TRY(hipMemcpyAsync(host, E->stage, n * sizeof(T), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}
template <class T>
void slice_gather(beom_engine *E, const T *dev, int inner, int K, int m) {        // device array -> staging image (level m of K)
    const DevView &d = E->d;
    const long long work = ((long long)d.ndeg + 1) * inner;
    hipLaunchKernelGGL((k_repack<T, false, false>), dim3((unsigned)((work + BEOM_BLOCK - 1) / BEOM_BLOCK)), dim3(BEOM_BLOCK), 0, E->stream,
                       const_cast<T *>(dev), (T *)E->stage, (long long)d.ndeg, d.L, d.P ? d.P : d.L, inner, K, m, E->slot_of_dev);
}

// a static array [outer][0:ndeg][inner] of the caller -> a new device array; src == nullptr: zeros
template <class T, bool REMAP = false>
int dev_upload(beom_engine *E, const T **dst, const T *src, size_t outer, int inner, char *errm, int errm_len) {
    const DevView &d = E->d;
    T *q = nullptr;
    int rc = dev_alloc(E, &q, outer * (size_t)d.n1 * inner, errm, errm_len, true);
    if (rc) return rc;
    const size_t n1h = (size_t)d.ndeg + 1;
    if (src)
        for (size_t o = 0; o < outer; ++o)
            if ((rc = slice_to_device<T, REMAP>(E, q + o * (size_t)d.n1 * inner, src + o * n1h * inner, inner, 1, 0, errm, errm_len))) return rc;
    *dst = q;
    return 0;
}

bool any_nonzero(const double *a, size_t n) {
    if (!a) return false;
    for (size_t i = 0; i < n; ++i)
        if (a[i] != 0.0) return true;
    return false;
}

// ---- beom_create in steps: each returns 0 or an error code with its message in errm ---------------------------------
int check_create_args(const beom_params *prm, const beom_handle *out, int device, const beom_dense::Grid &g,
                      const beom_statics &st, char *errm, int errm_len) {
    if (!prm || !out) { set_err(errm, errm_len, "beom_create: null argument"); return -1; }
    if (prm->abi_version != BEOM_ABI_VERSION) { set_err(errm, errm_len, "beom_create: ABI version mismatch (%d vs %d)", prm->abi_version, BEOM_ABI_VERSION); return -2; }
    if (prm->nlay < 1 || prm->nlay > BEOM_MAX_LAYERS || prm->ndeg < 1 || prm->lm < 1 || prm->mm < 1) { set_err(errm, errm_len, "beom_create: bad sizes"); return -3; }
    if (prm->rgld > 0.5 && (prm->variant == 1 || prm->slab_mm > 0 || prm->ocrp < 0.5)) {
        // (private_mod3d.f95 has no lid; the Poisson operators are only initialised with ocrp = 1, :505-563; the pressure sweep
        // couples the whole frame, so no bands)
        set_err(errm, errm_len, "beom_create: rgld = 1 (rigid lid, private_mod.f95:1705-1838) needs variant 0, ocrp = 1 and a whole frame (no bands)");
        return -5;
    }
    if (prm->variant == 1 && prm->nlay < 3) { set_err(errm, errm_len, "beom_create: variant 1 (private_mod3d.f95) needs nlay >= 3"); return -7; }
    if (!g.neig || !g.subc || !g.mk_u || !g.mk_v || !g.mk_n || !g.mkpe || !g.mkpi || !st.fcor || !st.h_th || !st.nudg || !st.fnud) { set_err(errm, errm_len, "beom_create: null static array"); return -1; }
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0 || device < 0 || device >= ndev) { set_err(errm, errm_len, "beom_create: no usable HIP device (%d visible, asked for %d); there is no CPU fallback", ndev, device); return -8; }
    HIP_TRY(hipSetDevice(device));
    if (prm->slab_mm > 0 && (prm->slab_row0 < 0 || prm->slab_row0 + prm->mm + 1 > prm->slab_mm + 1)) { set_err(errm, errm_len, "beom_create: slab rows outside the global frame"); return -3; }
    return 0;
}

// the constants of the view (everything but the layout and the device arrays), and which optional terms are live
void fill_view(DevView &d, const beom_params &prm, const beom_statics &st) {
    const size_t n1h = (size_t)prm.ndeg + 1, nl = (size_t)prm.nlay;      // n1h: cells per layer in the caller's arrays
    d.ndeg = prm.ndeg; d.nlay = prm.nlay; d.lm = prm.lm; d.mm = prm.mm; d.nsal = prm.nsal;
    d.variant = prm.variant; d.n1 = (long long)n1h; d.ncell = prm.ndeg;
    d.L = prm.lm + 1; d.M = prm.mm + 1;
    d.dl = prm.dl; d.dt = prm.dt; d.grav = prm.grav; d.rho0 = prm.rho0; d.beta = prm.beta;
    d.epsi = prm.epsi; d.gamm = prm.gamm; d.del1 = prm.del1; d.del2 = prm.del2; d.hmin = prm.hmin;
    d.hsal = prm.hsal; d.bvis = prm.bvis; d.dvis = prm.dvis; d.bdrg = prm.bdrg; d.tdrg = prm.tdrg;
    d.qdrg = prm.qdrg; d.hsbl = prm.hsbl; d.hbbl = prm.hbbl; d.uadv = prm.uadv; d.ocrp = prm.ocrp;
    d.rgld = prm.rgld; d.invf = prm.invf; d.w_ti = prm.w_ti; d.svis = prm.svis;
    d.mm_glob = prm.slab_mm > 0 ? prm.slab_mm : prm.mm;
    for (int i = 0; i < BEOM_MAX_LAYERS; ++i) d.rhon[i] = prm.rhon[i];
    d.i_dl = 1.0 / prm.dl;                      // private_mod.f95:1428,1511,1599,2321
    d.i_gr = 1.0 / prm.grav;                    // :2322
    d.i_ns = 1.0 / (double)(prm.nsal - 1);      // :2328
    d.i_r0 = 1.0 / prm.rho0;                    // :1429
    d.i_r1 = 1.0 / prm.rhon[0];                 // :1430
    for (int i = 0; i < prm.nlay; ++i) d.i_rn[i] = 1.0 / prm.rhon[i];   // :2329
    d.nstrip = 1; d.jlo0 = 1; d.jhi0 = d.M; d.jlo1 = 1; d.jhi1 = 0;
    d.slab = prm.slab_mm > 0 ? 1 : 0;
    d.joff = d.slab ? prm.slab_row0 : 0;
    d.Mg = d.slab ? prm.slab_mm + 1 : d.M;
    d.has_tide = any_nonzero(st.tide, 6 * n1h);
    d.has_bodf = any_nonzero(st.bodf, 2 * nl);
    d.has_nudg = any_nonzero(st.nudg, 3 * n1h);
    d.has_hto = any_nonzero(st.h_to, n1h);
    d.vel_targets_zero = beom_dense::vel_targets_zero(st.fnud, n1h, nl);
    d.rho_top = prm.rhon[0]; d.rho_bot = prm.rhon[nl - 1];
}

// The flags that follow from the forcing fields: distribute_stress's three terms, has_stress (uploaded stresses count),
// has_hdot, and whether the stress may fold into the momentum sweep.  beom_create and beom_set_forcing share it; plan_step
// reads the result through facts_of.
void derive_forcing_flags(beom_engine *E, bool wind, bool has_hdot) {
    const beom_params &prm = E->P;
    DevView &d = E->d;
    E->wind = wind;                                                                                                   // :1945
    E->bot = prm.bdrg > 1.e-7;                                                                                        // :1969
    E->top = prm.tdrg > 1.e-7;                                                                                        // :1991
    d.has_wind = E->wind; d.has_bot = E->bot; d.has_top = E->top;
    const bool terms = E->wind || E->bot || E->top;
    d.has_stress = terms || E->up_tt || E->up_tb || E->up_tu;
    d.has_hdot = has_hdot;
    // (a body force of exactly -0 would make the sign of a skipped +-0 visible)
    E->fold_static_ok = E->dense && prm.ocrp < 0.5 && !E->lid && terms && !E->bodf_neg0;
}
bool any_wind(const double *taus, size_t n) {      // private_mod.f95:1945
    if (taus) for (size_t i = 0; i < n; ++i) if (std::fabs(taus[i]) > 1.e-7) return true;
    return false;
}

// which paths the steps take: fused sweeps, tile geometry, stress terms, stress folded into the momentum sweep
void choose_paths(beom_engine *E, const beom_dense::Grid &g, const beom_statics &st) {
    const beom_params &prm = E->P;
    DevView &d = E->d;
    const size_t n1h = (size_t)prm.ndeg + 1, nl = (size_t)prm.nlay;
    for (size_t i = 0; i < n1h; ++i) { if (g.mk_u[i] > 0.5) E->any_u = 1; if (g.mk_v[i] > 0.5) E->any_v = 1; }
    // frames of few rounds of workgroups: the 64 x 4 tile geometry, one row per thread (a workgroup's lifetime is what the
    // step time is made of there).  Same box, us per step, 64 x 8 -> 64 x 4: stommel 128^2 31.2 -> 24.0, soliton 2048x256
    // 53.5 -> 43.6, 1024x128x4 74.8 -> 56.3, sill 4096x512x4 614 -> 596; jet 2048^2 x 2 535 -> 557, 4096^2 x 4 and larger: slower
    E->tile4 = E->dense && (long long)((d.L + 63) / 64) * ((d.M + 7) / 8) <= 5000;
    if (getenv("BEOM_TILE4")) E->tile4 = E->dense && atoi(getenv("BEOM_TILE4")) != 0;      // (A/B switch)
    if (E->lid) E->fuse = E->fuse_uv = false;      // the lid's flux rebuild reads the stored d2hx, d2hy of the last layer
    if (st.bodf) for (size_t i = 0; i < 2 * nl; ++i) if (st.bodf[i] == 0.0 && std::signbit(st.bodf[i])) E->bodf_neg0 = true;
    E->wind0 = any_wind(st.taus, 2 * n1h);
    E->has_hdot0 = any_nonzero(st.hdot, nl * n1h);
    E->taus0 = d.taus; E->taus_cells0 = d.taus_cells; E->hdot0 = d.hdot;
    derive_forcing_flags(E, E->wind0, E->has_hdot0);
}

// a host table -> a new device array of n >= v.size() elements (the rest zeroed if zero)
template <class T>
int upload_table(beom_engine *E, const T **dst, const std::vector<T> &v, size_t n, bool zero, char *errm, int errm_len) {
    T *q = nullptr;
    const int rc = dev_alloc(E, &q, n, errm, errm_len, zero);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));      // (v is the caller's temporary)
    *dst = q;
    return 0;
}

// the staging buffer, the layout's tables, the caller's static arrays, the wave table, the nudging tiles (in this order)
int upload_statics(beom_engine *E, const beom_dense::Layout &lay, const beom_dense::WaveTable &wt,
                   const std::vector<unsigned char> &ngt, const beom_dense::Grid &g, const beom_statics &st,
                   char *errm, int errm_len) {
    DevView &d = E->d;
    const size_t n1h = (size_t)d.ndeg + 1, nl = (size_t)d.nlay;
    E->stage_bytes = n1h * 32;                        // the widest slice: neig (8 x int32), a history (3 doubles)
    HIP_TRY(hipMalloc(&E->stage, E->stage_bytes));
    int rc;
    if (E->embedded) {
        if ((rc = upload_table(E, &E->slot_of_dev, lay.slot_of, lay.slot_of.size(), false, errm, errm_len))) return rc;
        if ((rc = upload_table(E, &d.pk_of, lay.pk_of, (size_t)d.n1, true, errm, errm_len))) return rc;
        if ((rc = upload_table(E, &d.reg4, lay.reg4, lay.reg4.size(), false, errm, errm_len))) return rc;
    }
    if ((rc = dev_upload<int32_t, true>(E, &d.neig, g.neig, 1, 8, errm, errm_len))) return rc;
    if ((rc = dev_upload(E, &d.subc, g.subc, 2, 1, errm, errm_len))) return rc;
    auto up = [&](const double **dst, const double *src, size_t outer, int inner = 1) {
        if (!rc) rc = dev_upload(E, dst, src, outer, inner, errm, errm_len);
    };
    up(&d.mk_u, g.mk_u, 1); up(&d.mk_v, g.mk_v, 1); up(&d.mk_n, g.mk_n, 1); up(&d.mkpe, g.mkpe, 1); up(&d.mkpi, g.mkpi, 1);
    up(&d.fcor, st.fcor, 1); up(&d.h_th, st.h_th, 1); up(&d.h_to, st.h_to, 1);
    up(&d.nudg, st.nudg, 3); up(&d.fnud, st.fnud, 3 * nl); up(&d.hdot, st.hdot, nl);
    up(&d.tide, st.tide, 3, 2); up(&d.taus, st.taus, 2);
    d.fnud_vel = (rc || d.vel_targets_zero) ? nullptr : d.fnud + d.n1 * (long long)d.nlay;
    // the wind stress as tt3d holds it: at real cells only (distribute_stress writes cells 1..ndeg, :1945-1966; index 0 and
    // every device slot that is no cell stay +0)
    std::vector<double> tc(2 * n1h, 0.0);
    if (st.taus) { std::memcpy(tc.data(), st.taus, 2 * n1h * sizeof(double)); tc[0] = 0.0; tc[n1h] = 0.0; }
    up(&d.taus_cells, tc.data(), 2);
    if (rc) return rc;
    double *q = nullptr;                              // bodf(nlay, 2): no cell dimension
    if ((rc = dev_alloc(E, &q, 2 * nl, errm, errm_len, true))) return rc;
    if (st.bodf) HIP_TRY(hipMemcpyAsync(q, st.bodf, 2 * nl * sizeof(double), hipMemcpyHostToDevice, E->stream));
    d.bodf = q;
    if (wt.uniform > 0 && (rc = upload_table(E, &d.woff, wt.woff, wt.woff.size(), false, errm, errm_len))) return rc;
    if (!ngt.empty()) {
        if ((rc = upload_table(E, &d.ngt, ngt, ngt.size(), false, errm, errm_len))) return rc;
        d.ngt_nx = (d.L + 63) / 64;
    }
    return 0;
}

// the state, the scratch of the sweeps, and v_cc = v_ll = bvis everywhere, sentinel included (initialize_variables, :276-277)
int alloc_state(beom_engine *E, char *errm, int errm_len) {
    DevView &d = E->d;
    const size_t n = (size_t)d.nlay * (size_t)d.n1;
    int rc = 0;
    auto al = [&](std::initializer_list<double **> arrays, size_t len) {
        for (double **a : arrays) if (!rc) rc = dev_alloc(E, a, len, errm, errm_len);
    };
    al({&d.hlay, &d.u, &d.v, &d.h_u, &d.h_v, &d.rs[0], &d.rs[1], &d.dmx[0], &d.dmx[1], &d.dmx[2], &d.dmy[0], &d.dmy[1], &d.dmy[2]}, n);
    if (E->dense) al({&d.dmx[3], &d.dmy[3], &d.u_alt, &d.v_alt, &d.hu_alt, &d.hv_alt}, n);      // partners for the fused U+V sweep
    al({&d.v_cc, &d.v_ll}, n);
    al({&d.tt3d, &d.tb3d, &d.tu3d}, 2 * n);
    al({&d.pcd, &d.qlr, &d.mont, &d.rvor, &d.pvor, &d.dive, &d.d2hx, &d.d2hy}, n);
    // kept Montgomery levels: handles whose steps can run the fused pair with the multistep term (zeroed like mont: slot 0
    // and every slot that is no cell hold +0 in all four buffers and are never written)
    E->mont_keep = E->dense && !E->lid && !d.slab && E->P.g_fb != 0.0 && d.nlay <= 8 && !(E->P.svis > 0.0);
    if (E->mont_keep) al({&d.mo0, &d.mo1, &d.mo2}, n);
    if (E->P.svis > 0.0) al({&d.delu, &d.delv, &d.uu4, &d.vv4}, n);
    if (E->lid) al({&d.pi_s, &d.pi_rhs, &d.pi_prev}, (size_t)d.n1);
    if (rc) return rc;
    if (E->P.bvis != 0.0) {
        std::vector<double> b(n, E->P.bvis);      // (padding slots too: never read)
        HIP_TRY(hipMemcpyAsync(d.v_cc, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice, E->stream));
        HIP_TRY(hipMemcpyAsync(d.v_ll, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice, E->stream));
        HIP_TRY(hipStreamSynchronize(E->stream));
    }
    return 0;
}

// everything of beom_create after the argument checks, for a handle with P and device set
int setup(beom_engine *E, const beom_dense::Grid &g, const beom_statics &st, char *errm, int errm_len) {
    const beom_params &prm = E->P;
    DevView &d = E->d;
    HIP_TRY(hipStreamCreateWithFlags(&E->own_stream, hipStreamNonBlocking));
    E->stream = E->own_stream;
    fill_view(d, prm, st);
    beom_dense::Layout lay = beom_dense::plan_layout(prm, d.L, d.M, d.joff, d.Mg, d.slab, g);
    E->dense = lay.dense; E->embedded = lay.embedded;
    d.xper = lay.xper; d.yper = lay.yper; d.embedded = lay.embedded ? 1 : 0; d.reg_nx = lay.reg_nx;
    E->dev_index = std::move(lay.dev_index);
    E->lid = prm.rgld > 0.5;
    if (E->lid) {
        const size_t n1h = (size_t)prm.ndeg + 1;
        E->subc_host.assign(g.subc, g.subc + 2 * n1h);
        E->neig_host.assign(g.neig, g.neig + 8 * n1h);
    }
    if (E->dense) {            // padded row pitch (DevView::P)
        d.P = lay.P;
        d.ncell = (long long)d.P * d.M;
        d.n1 = (d.ncell + 1 + 15) / 16 * 16;
    }
    beom_dense::WaveTable wt;
    if (!E->dense) wt = beom_dense::plan_wave_table(prm.ndeg, g);
    E->uniform_waves = wt.uniform; E->total_waves = wt.total;
    const std::vector<unsigned char> ngt = E->dense && d.has_nudg ? beom_dense::plan_nudging_tiles(lay, d.L, d.M, prm.ndeg, st.nudg)
                                                                  : std::vector<unsigned char>();
    int rc;
    if ((rc = upload_statics(E, lay, wt, ngt, g, st, errm, errm_len))) return rc;
    choose_paths(E, g, st);
    if ((rc = alloc_state(E, errm, errm_len))) return rc;
    const unsigned gx = (unsigned)((d.ncell + BEOM_BLOCK - 1) / BEOM_BLOCK);          // launches over all cell slots
    const unsigned gx0 = (unsigned)((d.ncell + 1 + BEOM_BLOCK - 1) / BEOM_BLOCK);
    E->grid_cells_layers_flat = dim3(gx, (unsigned)prm.nlay, 1);
    E->grid_cells0 = dim3(gx0, 1, 1);
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

}  // namespace

extern "C" {

int beom_abi_version(void) { return BEOM_ABI_VERSION; }

int beom_device_count(char *errm, int errm_len) {
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    return n;
}

int beom_device_pci_bus_id(int device, char *out, int out_len) {
    if (!out || out_len < 16) return -1;
    return hipDeviceGetPCIBusId(out, out_len, device) == hipSuccess ? 0 : -9;
}

int beom_create(const beom_params *prm, int device, const int32_t *neig, const int32_t *subc,
                const double *mk_u, const double *mk_v, const double *mk_n, const double *mkpe,
                const double *mkpi, const double *fcor, const double *h_th, const double *h_to,
                const double *nudg, const double *fnud, const double *hdot, const double *tide,
                const double *bodf, const double *taus, beom_handle *out, char *errm, int errm_len) {
    const beom_dense::Grid g{neig, subc, mk_u, mk_v, mk_n, mkpe, mkpi};
    const beom_statics st{fcor, h_th, h_to, nudg, fnud, hdot, tide, bodf, taus};
    int rc = check_create_args(prm, out, device, g, st, errm, errm_len);
    if (rc) return rc;
    beom_engine *E = new beom_engine();
    E->P = *prm;
    E->device = device;
    if ((rc = setup(E, g, st, errm, errm_len))) {      // every failure releases the handle (its stream and device arrays)
        beom_destroy(E);
        return rc;
    }
    *out = E;
    return 0;
}

int beom_destroy(beom_handle E) {
    if (!E) return 0;
    (void)hipSetDevice(E->device);
    if (E->stream) (void)hipStreamSynchronize(E->stream);
    for (std::vector<void *> *l : {&E->allocs, &E->trc_allocs, &E->trc_mix_allocs, &E->trc_vmix_allocs, &E->flt_allocs, &E->mom.allocs, &E->tmom.allocs, &E->harm.acc.allocs, &E->ser.allocs, &E->tser.allocs, &E->cser.allocs, &E->tcser.allocs, &E->maps.allocs, &E->frc[0].allocs, &E->frc[1].allocs}) free_list(*l);
    if (E->stage) (void)hipFree(E->stage);
    if (E->timer) { for (hipEvent_t ev : E->timer->ev) (void)hipEventDestroy(ev); delete E->timer; }
    if (E->own_stream) (void)hipStreamDestroy(E->own_stream);
    delete E;
    return 0;
}

// ---- host <-> device copies with the Fortran layouts ------------------------------
// [outer][0:ndeg] arrays of the caller (outer = nlay, or 2*nlay for the stresses), slice by slice
static int copy_in(beom_engine *E, double *dst, const double *src, size_t outer, char *errm, int errm_len) {
    if (!src) return 0;
    const size_t n1h = (size_t)E->d.ndeg + 1;
    for (size_t o = 0; o < outer; ++o) {
        const int rc = slice_to_device<double>(E, dst + o * (size_t)E->d.n1, src + o * n1h, 1, 1, 0, errm, errm_len);
        if (rc) return rc;
    }
    return 0;
}
static int copy_out(beom_engine *E, double *dst, const double *src, size_t outer, char *errm, int errm_len) {
    if (!dst) return 0;
    const size_t n1h = (size_t)E->d.ndeg + 1;
    for (size_t o = 0; o < outer; ++o) {
        slice_gather<double>(E, src + o * (size_t)E->d.n1, 1, 1, 0);
        const int rc = slice_to_host<double>(E, src, dst + o * n1h, 1, 1, errm, errm_len);
        if (rc) return rc;
    }
    return 0;
}

// AoS history (m, 0:ndeg, nlay) <-> K separate (0:ndeg, nlay) device arrays, layer by layer
// (outer: slices per level; 0 = nlay)
static int hist_in(beom_engine *E, double *const *dev, int K, const double *src, char *errm, int errm_len, int outer = 0) {
    if (!src) return 0;
    const size_t n1h = (size_t)E->d.ndeg + 1;
    if (!outer) outer = E->d.nlay;
    for (int l = 0; l < outer; ++l)
        for (int m = 0; m < K; ++m) {       // the layer's image is uploaded once, then one scatter per level
            const int rc = slice_to_device<double>(E, dev[m] + (size_t)l * E->d.n1, m == 0 ? src + (size_t)l * n1h * K : nullptr, 1, K, m,
                                                   errm, errm_len);
            if (rc) return rc;
        }
    return 0;
}
static int hist_out(beom_engine *E, double *const *dev, int K, double *dst, char *errm, int errm_len, int outer = 0) {
    if (!dst) return 0;
    const size_t n1h = (size_t)E->d.ndeg + 1;
    if (!outer) outer = E->d.nlay;
    for (int l = 0; l < outer; ++l) {
        for (int m = 0; m < K; ++m) slice_gather<double>(E, dev[m] + (size_t)l * E->d.n1, 1, K, m);
        const int rc = slice_to_host<double>(E, dev[0], dst + (size_t)l * n1h * K, 1, K, errm, errm_len);
        if (rc) return rc;
    }
    return 0;
}

int beom_upload_state(beom_handle E, const double *hlay, const double *u, const double *v,
                      const double *h_u, const double *h_v, const double *rs_h, const double *dmdx,
                      const double *dmdy, const double *v_cc, const double *v_ll, const double *tt3d,
                      const double *tb3d, const double *tu3d, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    DevView &d = E->d;
    const size_t nl = (size_t)d.nlay, n = ((size_t)d.ndeg + 1) * nl;
    int rc;
    if ((rc = leave_mont_history(E))) { set_err(errm, errm_len, "beom_upload_state: the history arrays could not be brought up to date"); return rc; }
    if ((rc = copy_in(E, d.hlay, hlay, nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.u, u, nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.v, v, nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.h_u, h_u, nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.h_v, h_v, nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.v_cc, v_cc, nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.v_ll, v_ll, nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.tt3d, tt3d, 2 * nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.tb3d, tb3d, 2 * nl, errm, errm_len))) return rc;
    if ((rc = copy_in(E, d.tu3d, tu3d, 2 * nl, errm, errm_len))) return rc;
    if ((rc = hist_in(E, d.rs, 2, rs_h, errm, errm_len))) return rc;
    if ((rc = hist_in(E, d.dmx, 3, dmdx, errm, errm_len))) return rc;
    if ((rc = hist_in(E, d.dmy, 3, dmdy, errm, errm_len))) return rc;
    // a caller may upload stresses computed elsewhere: keep those terms live
    if (any_nonzero(tt3d, 2 * n)) E->up_tt = true;
    if (any_nonzero(tb3d, 2 * n)) E->up_tb = true;
    if (any_nonzero(tu3d, 2 * n)) E->up_tu = true;
    if (E->up_tt || E->up_tb || E->up_tu) d.has_stress = 1;
    // zero-viscosity shortcut: only while v_cc, v_ll are +0 bit for bit (-0 would flip the sign of the products)
    for (const double *a : {v_cc, v_ll})
        if (a) for (size_t i = 0; i < n && E->visc_all_zero; ++i) { uint64_t b; memcpy(&b, &a[i], 8); if (b != 0) E->visc_all_zero = false; }
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_download_state(beom_handle E, double *hlay, double *u, double *v, double *h_u, double *h_v,
                        double *rs_h, double *dmdx, double *dmdy, double *v_cc, double *v_ll,
                        double *tt3d, double *tb3d, double *tu3d, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    DevView &d = E->d;
    const size_t nl = (size_t)d.nlay;
    int rc;
    if ((rc = hist_sync(E))) { set_err(errm, errm_len, "beom_download_state: the history arrays could not be brought up to date"); return rc; }
    if ((rc = copy_out(E, hlay, d.hlay, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, u, d.u, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, v, d.v, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, h_u, d.h_u, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, h_v, d.h_v, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, v_cc, d.v_cc, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, v_ll, d.v_ll, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, tt3d, d.tt3d, 2 * nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, tb3d, d.tb3d, 2 * nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, tu3d, d.tu3d, 2 * nl, errm, errm_len))) return rc;
    if ((rc = hist_out(E, d.rs, 2, rs_h, errm, errm_len))) return rc;
    if ((rc = hist_out(E, d.dmx, 3, dmdx, errm, errm_len))) return rc;
    if ((rc = hist_out(E, d.dmy, 3, dmdy, errm, errm_len))) return rc;
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_download_scratch(beom_handle E, double *mont, double *rvor, double *pvor, double *dive,
                          double *d2hx, double *d2hy, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    DevView &d = E->d;
    const size_t nl = (size_t)d.nlay;
    int rc;
    if ((rc = copy_out(E, mont, d.mont, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, rvor, d.rvor, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, pvor, d.pvor, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, dive, d.dive, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, d2hx, d.d2hx, nl, errm, errm_len))) return rc;
    if ((rc = copy_out(E, d2hy, d.d2hy, nl, errm, errm_len))) return rc;
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

int beom_set_rigid_lid(beom_handle E, const double *Ow, const double *Os, const double *Osum_, const double *pi_s,
                       char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (!E->lid) { set_err(errm, errm_len, "beom_set_rigid_lid: the handle was created with rgld = 0"); return -5; }
    HIP_TRY(hipSetDevice(E->device));
    DevView &d = E->d;
    int rc;
    if (!E->lid_ready) {
        if (!Ow || !Os || !Osum_) { set_err(errm, errm_len, "beom_set_rigid_lid: the operators Ow, Os, Osum_ are needed on the first call"); return -1; }
        if ((long long)d.n1 >= (1ll << 29)) { set_err(errm, errm_len, "beom_set_rigid_lid: frame too large for the lid's tables"); return -3; }
        const beom_dense::LidPlan lp = beom_dense::plan_lid(d.ndeg, d.lm, d.mm_glob, d.n1, E->subc_host, E->neig_host, E->dev_index);
        if ((rc = dev_upload(E, &d.Ow, Ow, 1, 1, errm, errm_len))) return rc;
        if ((rc = dev_upload(E, &d.Os, Os, 1, 1, errm, errm_len))) return rc;
        if ((rc = dev_upload(E, &d.Osum_, Osum_, 1, 1, errm, errm_len))) return rc;
        if ((rc = upload_table(E, &d.sor_order, lp.order, lp.order.size(), false, errm, errm_len))) return rc;
        if ((rc = upload_table(E, &d.sor_dstart, lp.start, lp.start.size(), false, errm, errm_len))) return rc;
        d.sor_ndiag = (int)lp.start.size() - 1;
        E->lid_dstep = lp.dstep;
        E->lid_maxwidth = lp.maxwidth;
        // one copy of the pressure per sweep in flight: up to kLidBatch of them within ~6 GB
        E->lid_nring = (int)std::max<long long>(17, std::min<long long>(kLidBatch, (6ll << 30) / ((long long)d.n1 * 8))) + 1;
        if ((rc = dev_alloc(E, &E->lid_ring, (size_t)E->lid_nring * d.n1, errm, errm_len, true))) return rc;      // zeroed: index 0 and every slot that is no cell stay 0
        if ((rc = dev_alloc(E, &E->lid_maxd, (size_t)kLidBatch, errm, errm_len, true))) return rc;
        if ((rc = upload_table(E, &d.lid_rhs_start, lp.rhs_start, lp.rhs_start.size(), false, errm, errm_len))) return rc;
        if ((rc = upload_table(E, &d.lid_rhs_ent, lp.rhs_ent, lp.rhs_ent.size(), false, errm, errm_len))) return rc;
        E->lid_ready = true;
    }
    if (pi_s && (rc = slice_to_device<double>(E, d.pi_s, pi_s, 1, 1, 0, errm, errm_len))) return rc;
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_download_pressure(beom_handle E, double *pi_s, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (!E->lid) { set_err(errm, errm_len, "beom_download_pressure: the handle was created with rgld = 0"); return -5; }
    HIP_TRY(hipSetDevice(E->device));
    const int rc = copy_out(E, pi_s, E->d.pi_s, 1, errm, errm_len);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_sync(beom_handle E, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---- launches -------------------------------------------------------------------------
static inline void rot2(double *(&a)[2]) { double *t = a[0]; a[0] = a[1]; a[1] = t; }
static inline void rot3(double *(&a)[4]) { double *t = a[0]; a[0] = a[1]; a[1] = a[2]; a[2] = t; }
static inline void rot4(double *(&a)[4]) { double *t = a[0]; a[0] = a[1]; a[1] = a[2]; a[2] = a[3]; a[3] = t; }
static inline void swp(double *&a, double *&b) { double *t = a; a = b; b = t; }

// ---- history from Montgomery: the state machine ---------------------------------------------------------------------
// d.mont of the step about to run <- the oldest buffer; the three others are the levels of the three steps before it
static void rotate_mont(beom_engine *E) {
    if (!E->mont_keep) return;
    DevView &d = E->d;
    double *t = d.mo0; d.mo0 = d.mo1; d.mo1 = d.mo2; d.mo2 = d.mont; d.mont = t;
}
// dmx[0..2], dmy[0..2] brought up to date after steps of the new form (k_hist_from_mont: 3 words read, 6 written per
// cell-layer).  Between steps only: d.mont is the last step's.  The kept levels stay valid.
static int hist_sync(beom_engine *E) {
    if (!E->hist_stale) return 0;
    if (hipSetDevice(E->device) != hipSuccess) return -9;
    hipLaunchKernelGGL(k_hist_from_mont, CellDense::grid(E->d, E->d.nlay), dim3(BEOM_BLOCK), 0, E->stream, E->d);
    E->hist_stale = false;
    return hipGetLastError() == hipSuccess ? 0 : -10;
}
// everything that works on the history arrays or writes d.mont outside beom_step: arrays first, and the levels no longer
// line up with the history afterwards
static int leave_mont_history(beom_engine *E) {
    const int rc = hist_sync(E);
    E->mont_levels_valid = 0;
    return rc;
}

// LAUNCH(kernel-template-name, extra template args..., nz, args...) picks the cell context.
#define LAUNCH_CTX(KERNEL_G, KERNEL_D, nz, ...)                                                            \
    do {                                                                                                  \
        if (E->dense) hipLaunchKernelGGL(KERNEL_D, CellDense::grid(E->d, (nz)), dim3(BEOM_BLOCK), 0, E->stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL_G, CellGather::grid(E->d, (nz)), dim3(BEOM_BLOCK), 0, E->stream, __VA_ARGS__);         \
    } while (0)

// Run-time values as template arguments: pick(f, a, b, ...) calls the generic lambda f with one std::bool_constant per
// flag; pick_int<FROM, TO>(v, f) calls f with the std::integral_constant of v, trying FROM first and stepping towards TO
// (a v outside the range counts as TO).  f names the kernel; what it discards with `if constexpr` is never instantiated.
// The kernels come out in the order tried, true before false: the code object keeps the layout the ladders of old gave it.
template <class F>
static void pick(F &&f) { f(); }
template <class F, class... R>
static void pick(F &&f, bool b, R... rest) {
    if (b) pick([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else pick([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <int FROM, int TO, class F>
static void pick_int(int v, F &&f) {
    if (FROM == TO || v == FROM) f(std::integral_constant<int, FROM>{});
    else if constexpr (FROM != TO) pick_int<FROM + (TO > FROM ? 1 : -1), TO>(v, f);
}

static void launch_rebuild(beom_engine *E) {
    LAUNCH_CTX(k_rebuild_fluxes<CellGather>, k_rebuild_fluxes<CellDense>, E->d.nlay, E->d);
}
// FORCE of k_update_h and of the tracer sweeps: 0 = no relaxation, 1 = nudging, 2 = nudging and tide
static int forcing(const DevView &d) { return d.has_nudg ? (d.has_tide ? 2 : 1) : 0; }
static void launch_h(beom_engine *E, double gene, double ramp, double ctim, bool rotate = true) {
    // variant 1 couples layers inside a cell -> one thread walks nlay..1; variant 0: layer = blockIdx.y
    int nz = (E->d.variant == 1) ? 1 : E->d.nlay;
    // nudged frames: one thread walks the layers of its cell, so the cell's relaxation rate is read once instead of once per
    // layer (carrier beach 8192x1024x8: 802 -> 747 us per launch, sill 4096x512x4: 89 -> 83; same-box A/B, round 3)
    if (E->d.has_nudg) nz = 1;
    pick_int<2, 0>(forcing(E->d), [&](auto fo) { LAUNCH_CTX((k_update_h<CellGather, fo>), (k_update_h<CellDense, fo>), nz, E->d, gene, ramp, ctim, 0); });
    if (rotate) rot2(E->d.rs);
}
// diffusion, decay and sources of the tracers (beom_tracer_mix.h): all tracers in one launch, q -> q_alt
static void launch_tracer_mix(beom_engine *E) {
    const TrcMixView m{E->ntrc, E->trc_q, E->trc_q_alt, E->trc_mix};
    LAUNCH_CTX(k_tracer_mix<CellGather>, k_tracer_mix<CellDense>, E->d.nlay, E->d, m);
    swp(E->trc_q, E->trc_q_alt);
    ++E->trc_mix_launches;
}
// vertical diffusion of the tracers (beom_tracer_vmix.h): all tracers in one launch, one thread per water column, q in place
static void launch_tracer_vmix(beom_engine *E) {
    const TrcVmixView m{E->ntrc, E->trc_q, E->trc_vmix};
    pick_int<2, BEOM_MAX_LAYERS>(E->d.nlay, [&](auto nl) { LAUNCH_CTX((k_tracer_vmix<CellGather, nl>), (k_tracer_vmix<CellDense, nl>), 1, E->d, m); });
    ++E->trc_vmix_launches;
}
// the tracer sweep of a step (beom_tracers.h): all tracers in one launch, in front of the step's update_h; a step of a
// handle with mixing runs the lateral mixing launch first, then the vertical one, on the q and hlay of the same time level
static void launch_tracers(beom_engine *E, double gene, double ramp, double ctim, bool mix = true) {
    if (mix && E->trc_mix) launch_tracer_mix(E);
    if (mix && E->trc_vmix) launch_tracer_vmix(E);
    TrcView tv{E->ntrc, E->trc_ctrg ? 1 : 0, E->trc_q, E->trc_q_alt, E->trc_rq[0], E->trc_rq[1], E->trc_ctrg};
    const int nz = E->d.nlay;
    // scheme 2 (beom_tracers_lim.h): the tiled kernel in the handle's tile geometry, or the table path
    if (E->trc_scheme == 2) pick_int<2, 0>(forcing(E->d), [&](auto fo) {
        if (!E->dense) hipLaunchKernelGGL((k_tracers_lim<CellGather, fo>), CellGather::grid(E->d, nz), dim3(BEOM_BLOCK), 0, E->stream, E->d, tv, gene, ramp, ctim);
        else if (E->tile4) hipLaunchKernelGGL((k_tracers_lim<TrcTiled<1>, fo>), tracers_lim_grid<1>(E->d), dim3(BEOM_BLOCK), 0, E->stream, E->d, tv, gene, ramp, ctim);
        else hipLaunchKernelGGL((k_tracers_lim<TrcTiled<2>, fo>), tracers_lim_grid<2>(E->d), dim3(BEOM_BLOCK), 0, E->stream, E->d, tv, gene, ramp, ctim);
    });
    else pick_int<2, 0>(forcing(E->d), [&](auto fo) { LAUNCH_CTX((k_tracers<CellGather, fo>), (k_tracers<CellDense, fo>), nz, E->d, tv, gene, ramp, ctim); });
    swp(E->trc_q, E->trc_q_alt);
    rot2(E->trc_rq);
}
// a float launch (beom_floats.h): mode 1 = stage 1, 2 = stage 2, 3 = stage 2 then stage 1; rec: the record stage 2 writes
static FloatView float_view(const beom_engine *E, double *rec) {
    const DevView &d = E->d;
    return FloatView{E->nflt, E->flt_x, E->flt_y, E->flt_layer, E->flt_rej, E->flt_k1x, E->flt_k1y, E->flt_xs, E->flt_ys,
                     E->integ_cellmap, d.dt * d.i_dl, (double)d.lm, (double)d.mm, E->integ_xper, E->integ_yper, rec};
}
static void launch_floats(beom_engine *E, int mode, double *rec) {
    const DevView &d = E->d;
    FloatView f = float_view(E, rec);
    if (E->flt_band) {                 // a band: the frame's wraps and rows, not the window's
        f.fmm = E->flt_fmm; f.xper = E->flt_xper; f.yper = E->flt_yper; f.cellmap = nullptr;
        const dim3 g((unsigned)((E->nflt + BEOM_BLOCK - 1) / BEOM_BLOCK)), b(BEOM_BLOCK);
        pick_int<1, 3>(mode, [&](auto m) { hipLaunchKernelGGL(k_floats_band<m>, g, b, 0, E->stream, d, f, E->flt_fb); });
        ++E->flt_launches;
        return;
    }
    const dim3 g((unsigned)((E->nflt + BEOM_BLOCK - 1) / BEOM_BLOCK)), b(BEOM_BLOCK);
    pick_int<1, 3>(mode, [&](auto m) {
        if (E->dense) hipLaunchKernelGGL((k_floats<CellDense, m>), g, b, 0, E->stream, d, f);
        else hipLaunchKernelGGL((k_floats<CellGather, m>), g, b, 0, E->stream, d, f);
    });
    ++E->flt_launches;
}
// stage 2 of step tstp (then stage 1 of the next step if `then_stage1`), with the step's record if it is due
static void launch_floats_after(beom_engine *E, int tstp, bool then_stage1) {
    double *rec = nullptr;
    if (E->flt_nrec > 0 && tstp % E->flt_stride == 0 && (int)E->flt_rec_tstp.size() < E->flt_nrec) {
        rec = E->flt_rec + 3 * (size_t)E->nflt * E->flt_rec_tstp.size();
        E->flt_rec_tstp.push_back(tstp);
    }
    launch_floats(E, then_stage1 ? 3 : 2, rec);
}
// one sample of the moments (beom_moments.h) of the fields as they stand, recorded under step tstp
static void launch_moments(beom_engine *E, int tstp) {
    const DevView &d = E->d;
    double *const *r = E->mom.ref, *const *s = E->mom.sum, *const *q = E->mom.sq;
    const MomentView m{(long long)d.nlay * d.n1, d.hlay, d.u, d.v, d.h_u, d.h_v, r[0], r[1], r[2], r[3], r[4],
                       s[0], s[1], s[2], s[3], s[4], q[0], q[1], q[2], q[3], q[4]};
    const long long pairs = (m.n - 1) / 2;
    const dim3 g((unsigned)std::max<long long>(1, std::min<long long>((pairs + BEOM_BLOCK - 1) / BEOM_BLOCK, 2048))), b(BEOM_BLOCK);
    pick_int<1, 3>(E->mom.level, [&](auto lv) {
        pick([&](auto first) { hipLaunchKernelGGL((k_moments<lv, first>), g, b, 0, E->stream, m); }, E->mom.count == 0);
    });
    accum_note_sample(E->mom, tstp);
}
// one sample of the harmonics (beom_harmonics.h) of the fields as they stand at time ctim, recorded under step tstp: the
// weights and the normal matrix on the host, one launch per field
static void launch_harmonics(beom_engine *E, int tstp, double ctim) {
    const DevView &d = E->d;
    Harmonics &H = E->harm;
    const int K = H.nfreq, nw = 1 + 2 * K, nf = H.acc.level >= 2 ? 5 : 3;
    double w[1 + 2 * BEOM_MAX_HARMONICS] = {1.0};
    for (int k = 0; k < K; ++k) (void)beom_harmonic_weights(H.omega[k], ctim, &w[1 + 2 * k], &w[2 + 2 * k]);
    for (int i = 0; i < nw; ++i)
        for (int j = 0; j < nw; ++j) H.gram[i * nw + j] = H.gram[i * nw + j] + w[i] * w[j];
    const double *const x[5] = {d.hlay, d.u, d.v, d.h_u, d.h_v};
    const long long n = (long long)d.nlay * d.n1, pairs = (n - 1) / 2;
    const dim3 g((unsigned)std::max<long long>(1, std::min<long long>((pairs + BEOM_BLOCK - 1) / BEOM_BLOCK, 2048))), b(BEOM_BLOCK);
    for (int f = 0; f < nf; ++f) {
        double *const *s = H.sum[f];
        const HarmView v{n, x[f], H.acc.ref[f], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8],
                         w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]};
        pick_int<1, BEOM_MAX_HARMONICS>(K, [&](auto kk) {
            pick([&](auto first) { hipLaunchKernelGGL((k_harmonics<kk, first>), g, b, 0, E->stream, v); }, H.acc.count == 0);
        });
    }
    accum_note_sample(H.acc, tstp);
    H.acc.launches += nf - 1;          // (one launch per field)
}
// one sample of the tracer moments (beom_tracer_moments.h) of q, hlay, h_u, h_v as they stand, recorded under step tstp
static void launch_tracer_moments(beom_engine *E, int tstp) {
    double *const *r = E->tmom.ref, *const *s = E->tmom.sum;
    const TrcMomentView m{E->ntrc, E->trc_q, r[0], r[1], r[2], r[3], s[0], s[1], s[2], s[3], E->tmom.sq[0]};
    const int nz = E->d.nlay;
    pick_int<1, 3>(E->tmom.level, [&](auto lv) {
        pick([&](auto first) { LAUNCH_CTX((k_tracer_moments<CellGather, lv, first>), (k_tracer_moments<CellDense, lv, first>), nz, E->d, m); },
             E->tmom.count == 0);
    });
    accum_note_sample(E->tmom, tstp);
}
// one record of the series (beom_series.h) of the fields as they stand into the next free slot, under step tstp
static void launch_series(beom_engine *E, int tstp) {
    const DevView &d = E->d;
    Recorder &R = E->ser;
    const int count = beom_series_count(d.nlay, R.level);
    const RowTree t = row_tree(d.L);
    double *rec = R.rec + R.tstp.size() * (size_t)R.rows * count;
    const dim3 g((unsigned)t.nch, (unsigned)((R.rows + BEOM_TILE_Y - 1) / BEOM_TILE_Y), 1), b(BEOM_BLOCK);
    const int32_t *map = E->dense ? nullptr : E->integ_cellmap;
    // (the two kernels take the same arguments; named here and not through pick, which would move k_integral_rows behind
    // its other user, beom_integral_rows, in the code object)
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, g, b, 0, E->stream, d, R.jlo, R.rows, t.width, E->integ_xper, E->integ_yper, map, E->integ_part); };
    if (R.level == 1) { if (E->dense) go(k_integral_rows<true>); else go(k_integral_rows<false>); }
    else if (E->dense) go(k_series_rows<true>); else go(k_series_rows<false>);
    hipLaunchKernelGGL(k_integral_chunks, dim3((unsigned)R.rows), dim3(64), 0, E->stream,
                       (const double *)E->integ_part, rec, count, t.nch, t.nchp2);
    R.tstp.push_back(tstp);
}
// one record of the tracer series (beom_tracer_series.h) of q, hlay, h_u, h_v as they stand into the next free slot, under step
// tstp: `batch` rows per launch, every row finished on its own
static void launch_tracer_series(beom_engine *E, int tstp) {
    const DevView &d = E->d;
    Recorder &R = E->tser;
    const int nq = 2 * R.level, per = E->ntrc * d.nlay, cnt = per * nq;
    const RowTree t = row_tree(d.L);
    double *rec = R.rec + R.tstp.size() * (size_t)R.rows * cnt;
    const int32_t *map = E->dense ? nullptr : E->integ_cellmap;
    for (int r0 = 0; r0 < R.rows; r0 += R.batch) {
        const int nr = std::min(R.batch, R.rows - r0);
        const dim3 g((unsigned)t.nch, (unsigned)((nr + BEOM_TILE_Y - 1) / BEOM_TILE_Y), 1), b(BEOM_BLOCK);
        pick_int<1, 3>(R.level, [&](auto lv) {
            pick([&](auto dense) {
                hipLaunchKernelGGL((k_tracer_series_rows<dense, lv>), g, b, 0, E->stream, d, (const double *)E->trc_q, E->ntrc, R.jlo + r0, nr,
                                   t.width, E->integ_xper, E->integ_yper, map, R.part);
            }, E->dense);
        });
        hipLaunchKernelGGL(k_tracer_series_chunks, dim3((unsigned)nr, (unsigned)per), dim3(64), 0, E->stream,
                           (const double *)R.part, rec + (size_t)r0 * cnt, cnt, nq, t.nch, t.nchp2);
    }
    R.tstp.push_back(tstp);
}
static void launch_mont(beom_engine *E, int ilay) {
    if (ilay == 0 && E->d.nlay <= 8) {         // all layers of a column in one thread: instantiated for 1..8 layers
        if (E->dense) pick_int<1, 8>(E->d.nlay, [&](auto n) { hipLaunchKernelGGL((k_update_mont_all<CellDense, n>), CellDense::grid(E->d, 1), dim3(BEOM_BLOCK), 0, E->stream, E->d); });
        else pick_int<1, 8>(E->d.nlay, [&](auto n) { hipLaunchKernelGGL((k_update_mont_all<CellGather, n>), CellGather::grid(E->d, 1), dim3(BEOM_BLOCK), 0, E->stream, E->d); });
        return;
    }
    const int nz = ilay ? 1 : E->d.nlay;
    LAUNCH_CTX(k_update_mont<CellGather>, k_update_mont<CellDense>, nz, E->d, ilay);
}
// update_viscosity's biharmonic part runs as the tiled sweep (k_biharm_tiled): every dense or embedded handle with svis > 0
static bool biharm_tiled(const beom_engine *E) { return E->dense && E->P.svis > 0.0; }
static void launch_visc(beom_engine *E, int ilay) {
    const int nz = ilay ? 1 : E->d.nlay;
    LAUNCH_CTX(k_update_visc<CellGather>, k_update_visc<CellDense>, nz, E->d, ilay);
    if (E->d.svis > 0.0 && biharm_tiled(E) && ilay == 0) {      // biharmonic part of update_viscosity (:2508-2599), one tiled sweep
        if (E->tile4) hipLaunchKernelGGL(k_biharm_tiled<1>, biharm_tiled_grid<1>(E->d), dim3(BEOM_BLOCK), 0, E->stream, E->d);
        else hipLaunchKernelGGL(k_biharm_tiled<2>, biharm_tiled_grid<2>(E->d), dim3(BEOM_BLOCK), 0, E->stream, E->d);
    } else if (E->d.svis > 0.0) {                  // packed handles, single-layer calls: the two table kernels
        const dim3 g = ilay ? E->grid_cells0 : E->grid_cells_layers_flat;
        hipLaunchKernelGGL(k_biharm_lap, g, dim3(BEOM_BLOCK), 0, E->stream, E->d, ilay);
        hipLaunchKernelGGL(k_biharm_flux, g, dim3(BEOM_BLOCK), 0, E->stream, E->d, ilay);
    }
}
template <bool XDIR>
static void launch_uv(beom_engine *E, int ilay, double gene, double ramp, double ctim, bool prod = false) {
    const int nz = ilay ? 1 : E->d.nlay;
    const int copy_hist = ilay ? 1 : 0;       // a single-layer call cannot rotate shared pointers
    if (prod) hipLaunchKernelGGL((k_update_uv<CellDense, XDIR, true>), CellDense::grid(E->d, nz), dim3(BEOM_BLOCK), 0, E->stream, E->d, ilay, gene, ramp, ctim, copy_hist);
    else LAUNCH_CTX((k_update_uv<CellGather, XDIR>), (k_update_uv<CellDense, XDIR>), nz, E->d, ilay, gene, ramp, ctim, copy_hist);
    if (!copy_hist) { if (XDIR) rot3(E->d.dmx); else rot3(E->d.dmy); }
}
// the tiled sweeps in the tile geometry Q (beom_kernels.h: TileGeom)
template <int Q>
static void raw_mont_visc(beom_engine *E, const StepPlan &p) {
    const dim3 g = mont_visc_grid<Q>(E->d), b(BEOM_BLOCK);
    pick_int<1, 8>(E->d.nlay, [&](auto n) {       // (p.mont.fused: nlay <= 8)
        pick([&](auto pl, auto le) { hipLaunchKernelGGL((k_mont_visc<Q, n, le, pl>), g, b, 0, E->stream, E->d); }, p.mont.plain, p.leith);
    });
}
template <int Q>
static void raw_uv_fused(beom_engine *E, const StepPlan &p) {
    const dim3 g = uv_fused_grid<Q>(E->d), b(TileGeom<Q>::BLOCK);
    // (sf: distribute_stress formed inside the sweep — its own instantiations, so that the unforced ones stay lean;
    // hm: the history-from-Montgomery form, plain: the optional forcing compiled out — both instantiated for the staged
    // k_uv_fused only.  beom_plan::uv_form_exists: the twelve forms a plan can name)
    pick([&](auto fx, auto pl, auto hm, auto sf, auto zv, auto pr) {
        if constexpr (!beom_plan::uv_form_exists(sf, pr, zv, hm, pl)) { fprintf(stderr, "beom: the plan names a form of the u+v sweep that does not exist\n"); std::abort(); }
        else if constexpr (sf) hipLaunchKernelGGL((k_uv_fused_sf<Q, fx, pr, zv>), g, b, 0, E->stream, E->d, p.gene, p.ramp, p.ctim);
        else hipLaunchKernelGGL((k_uv_fused<Q, fx, pr, zv, hm, pl>), g, b, 0, E->stream, E->d, p.gene, p.ramp, p.ctim);
    }, p.uv.first_x, p.uv.plain, p.uv.hm, p.stress_fold, p.uv.zv, p.uv.prod);
}
// fused Montgomery + Leith sweep (dense frames): p.leith refreshes the Leith viscosity (:2188, :2268); else the sweep forms
// the products of the standing v_cc, v_ll
static void launch_mont_visc(beom_engine *E, const StepPlan &p) { if (E->tile4) raw_mont_visc<1>(E, p); else raw_mont_visc<2>(E, p); }
// fused U+V sweep (dense frames): first_x = update_u first (even tstp)
static void uv_fused_swap(beom_engine *E, bool first_x, bool hm = false) {
    DevView &d = E->d;
    swp(d.u, d.u_alt); swp(d.v, d.v_alt);                 // both velocities are written out of place
    if (first_x) swp(d.h_v, d.hv_alt); else swp(d.h_u, d.hu_alt);
    if (hm) { E->hist_stale = true; return; }             // the history arrays were not touched: they lag from here on
    if (first_x) { rot4(d.dmx); rot3(d.dmy); }
    else         { rot4(d.dmy); rot3(d.dmx); }
}
static void launch_uv_fused(beom_engine *E, const StepPlan &p, bool swap = true) {
    if (E->tile4) raw_uv_fused<1>(E, p); else raw_uv_fused<2>(E, p);
    if (swap) uv_fused_swap(E, p.uv.first_x, p.uv.hm);
}
// rigid lid: rebuild the transports from the new h and velocities (steps 1-3: centred, :2166-2177; later: upstream with the
// curvatures of the last layer, :2237-2257), then the pressure solve and the velocity correction (surf_pressure, :1705-1838)
static void launch_lid_fluxes(beom_engine *E, bool first3) {
    if (first3) { launch_rebuild(E); return; }
    const dim3 g((unsigned)((E->d.ncell + BEOM_BLOCK - 1) / BEOM_BLOCK), (unsigned)E->d.nlay, 1);
    hipLaunchKernelGGL(k_rgld_upstream_fluxes, g, dim3(BEOM_BLOCK), 0, E->stream, E->d);
}
static void launch_lid_h_epilogue(beom_engine *E) {
    hipLaunchKernelGGL(k_rgld_h_epilogue, dim3((unsigned)((E->d.ncell + BEOM_BLOCK - 1) / BEOM_BLOCK)), dim3(BEOM_BLOCK), 0, E->stream, E->d);
}
// surf_pressure's iteration (:1757-1802): Gauss-Seidel sweeps until max |change| <= 1e-5 or 1000 sweeps, as a pipeline of
// wavefronts (k_rgld_gs_front): batches of up to kLidBatch sweeps in flight, one launch per time step of the pipeline, the
// host reads the batch's per-sweep maxima and picks the sweep the serial loop would have stopped after (one small
// device-to-host copy per batch: a lid step is not asynchronous).
static int lid_solve(beom_engine *E) {
    DevView &d = E->d;
    const int maxiters = 1000;
    const double pi_tol = 1.e-5;
    const int R = E->lid_nring, D = E->lid_dstep, nlev = d.sor_ndiag;
    const size_t bytes = (size_t)d.n1 * sizeof(double);
    if (hipMemcpyAsync(E->lid_ring, d.pi_s, bytes, hipMemcpyDeviceToDevice, E->stream) != hipSuccess) return -1;      // copy 0 = the pressure before the first sweep
    // A batch costs (levels + 2 * sweeps) dependent launches whatever it finds, and a launch costs the more the more sweeps are
    // in flight: the first batch is sized by what the step before needed (+ 25 %), later ones take all the ring holds.
    int s0 = 1, batch = std::min(R - 1, std::max(16, E->lid_last * 5 / 4 + 8)), chosen = 0;
    unsigned long long maxd[kLidBatch];
    while (!chosen) {
        const int nb = std::min(batch, maxiters - s0 + 1);
        if (hipMemsetAsync(E->lid_maxd, 0, nb * sizeof(unsigned long long), E->stream) != hipSuccess) return -1;
        const dim3 g((unsigned)((E->lid_maxwidth + BEOM_BLOCK - 1) / BEOM_BLOCK), (unsigned)nb, 1);
        const int tend = nlev - 1 + (nb - 1) * D;
        for (int t = 0; t <= tend; ++t)
            hipLaunchKernelGGL(k_rgld_gs_front, g, dim3(BEOM_BLOCK), 0, E->stream, d, E->lid_ring, R, s0, t, D, E->lid_maxd);
        E->lid_launches += tend + 1;
        if (hipMemcpyAsync(maxd, E->lid_maxd, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, E->stream) != hipSuccess) return -1;
        if (hipStreamSynchronize(E->stream) != hipSuccess) return -1;
        for (int b = 0; b < nb && !chosen; ++b) {
            double m; memcpy(&m, &maxd[b], sizeof(double));
            if (!(m > pi_tol) || s0 + b == maxiters) chosen = s0 + b;           // `do while (maxdiff > pi_tol .and. iters < maxiters)`
        }
        s0 += nb;
        batch = R - 1;
    }
    E->lid_sweeps += chosen; ++E->lid_solves; E->lid_last = chosen;
    if (hipMemcpyAsync(d.pi_s, E->lid_ring + (size_t)(chosen % R) * d.n1, bytes, hipMemcpyDeviceToDevice, E->stream) != hipSuccess) return -1;
    return 0;
}
static void launch_lid_pressure(beom_engine *E) {
    const dim3 g1((unsigned)((E->d.ncell + BEOM_BLOCK - 1) / BEOM_BLOCK)), g((unsigned)((E->d.ncell + BEOM_BLOCK - 1) / BEOM_BLOCK), (unsigned)E->d.nlay, 1);
    hipLaunchKernelGGL(k_rgld_rhs, g1, dim3(BEOM_BLOCK), 0, E->stream, E->d);
    if (lid_solve(E)) snprintf(E->last_err, sizeof(E->last_err), "the lid's pressure iteration failed: %s", hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(k_rgld_correct, g, dim3(BEOM_BLOCK), 0, E->stream, E->d);
}
static void launch_stress(beom_engine *E) {
    if (!(E->wind || E->bot || E->top)) return;
    const dim3 g((unsigned)((E->d.ncell + BEOM_BLOCK - 1) / BEOM_BLOCK));
    hipLaunchKernelGGL(k_stress, g, dim3(BEOM_BLOCK), 0, E->stream, E->d, (int)E->wind, (int)E->bot, (int)E->top);
}
// forcing in time (beom_forcing.h): one field's frames k0, k1 with weight a -> the buffer(s) the sweeps read
static void launch_forcing(beom_engine *E, int field, int k0, int k1, double a) {
    ForcingSet &S = E->frc[field];
    const DevView &d = E->d;
    const ForcingView v{d.n1, S.frames[(size_t)k0], S.frames[(size_t)k1], S.x, S.xc};
    const unsigned outer = field == 0 ? 2u : (unsigned)d.nlay;
    // pairs need the four arrays aligned alike (they are: all come from alloc_aligned)
    const uintptr_t lo = reinterpret_cast<uintptr_t>(v.A) & 15;
    const bool pairs = (reinterpret_cast<uintptr_t>(v.B) & 15) == lo && (reinterpret_cast<uintptr_t>(v.x) & 15) == lo &&
                       (!v.xc || (reinterpret_cast<uintptr_t>(v.xc) & 15) == lo);
    const long long work = pairs ? (d.n1 + 1) / 2 : d.n1;
    const dim3 g((unsigned)std::max<long long>(1, std::min<long long>((work + BEOM_BLOCK - 1) / BEOM_BLOCK, 2048)), outer), b(BEOM_BLOCK);
    pick([&](auto two, auto pr) { hipLaunchKernelGGL((k_forcing_lerp<two, pr>), g, b, 0, E->stream, v, a); }, field == 0, pairs);
    S.k0 = k0; S.k1 = k1; S.a = a;
    ++E->frc_launches;
}
// the fields of time ctim: a launch per field that has frames, left out where the buffer holds these bits already
static void apply_forcing(beom_engine *E, double ctim) {
    for (int f = 0; f < 2; ++f) {
        const ForcingSet &S = E->frc[f];
        if (S.nfr == 0) continue;
        int k0, k1;
        double a;
        beom_forcing::forcing_weight(S.nfr, S.times.data(), S.period, ctim, &k0, &k1, &a);
        if (k0 == S.k0 && k1 == S.k1 && std::memcmp(&a, &S.a, sizeof a) == 0) continue;
        launch_forcing(E, f, k0, k1, a);
    }
}

extern "C" {

#define NEED(E) do { if (!(E)) return -1; if (hipSetDevice((E)->device) != hipSuccess) return -9; } while (0)

#define LAUNCHED() (hipGetLastError() == hipSuccess ? 0 : -10)
// (a sweep called on its own works on the history arrays and breaks the sequence of kept Montgomery levels: NEED_ARRAYS)
#define NEED_ARRAYS(E) do { NEED(E); if (leave_mont_history(E)) return -10; } while (0)
int beom_update_h(beom_handle E, double gene, double ramp, double ctim) { NEED_ARRAYS(E); launch_h(E, gene, ramp, ctim); return LAUNCHED(); }
int beom_update_tracers(beom_handle E, double gene, double ramp, double ctim) { NEED_ARRAYS(E); if (E->ntrc < 1) return -3; launch_tracers(E, gene, ramp, ctim, false); return LAUNCHED(); }
int beom_update_tracer_mixing(beom_handle E) { NEED_ARRAYS(E); if (E->ntrc < 1 || !E->trc_mix) return -3; launch_tracer_mix(E); return LAUNCHED(); }
int beom_update_tracer_vmixing(beom_handle E) { NEED_ARRAYS(E); if (E->ntrc < 1 || !E->trc_vmix) return -3; launch_tracer_vmix(E); return LAUNCHED(); }
int beom_update_mont_rvor_pvor_dive_kine(beom_handle E, int ilay) { NEED_ARRAYS(E); if (ilay < 0 || ilay > E->d.nlay) return -3; launch_mont(E, ilay); return LAUNCHED(); }
int beom_update_viscosity(beom_handle E, int ilay) { NEED_ARRAYS(E); if (ilay < 0 || ilay > E->d.nlay) return -3; launch_visc(E, ilay); return LAUNCHED(); }
int beom_update_u(beom_handle E, int ilay, double gene, double ramp, double ctim) { NEED_ARRAYS(E); if (ilay < 0 || ilay > E->d.nlay) return -3; launch_uv<true>(E, ilay, gene, ramp, ctim); return LAUNCHED(); }
int beom_update_v(beom_handle E, int ilay, double gene, double ramp, double ctim) { NEED_ARRAYS(E); if (ilay < 0 || ilay > E->d.nlay) return -3; launch_uv<false>(E, ilay, gene, ramp, ctim); return LAUNCHED(); }
int beom_rebuild_fluxes(beom_handle E) { NEED_ARRAYS(E); launch_rebuild(E); return LAUNCHED(); }
int beom_distribute_stress(beom_handle E) { NEED_ARRAYS(E); launch_stress(E); return LAUNCHED(); }
#undef NEED_ARRAYS
#undef LAUNCHED

}  // extern "C"

// ---- the step driver: plan_step (beom_plan.h) decides the form of a step, the functions below execute it ---------------
static StepFacts facts_of(const beom_engine *E) {
    const DevView &d = E->d;
    StepFacts f;
    f.dense = E->dense; f.nlay = d.nlay; f.lid = E->lid;
    f.svis = E->P.svis; f.dvis = E->P.dvis; f.bvis = E->P.bvis; f.g_fb = E->P.g_fb; f.ocrp = d.ocrp;
    f.has_nudg = d.has_nudg; f.has_tide = d.has_tide; f.has_stress = d.has_stress; f.has_bodf = d.has_bodf; f.has_hto = d.has_hto;
    f.wind = E->wind; f.bot = E->bot; f.top = E->top; f.up_tt = E->up_tt; f.up_tb = E->up_tb; f.up_tu = E->up_tu;
    f.fold_static_ok = E->fold_static_ok; f.visc_all_zero = E->visc_all_zero; f.mont_keep = E->mont_keep;
    f.fuse = E->fuse; f.fuse_uv = E->fuse_uv; f.fold_stress = E->fold_stress; f.lean_d2h = E->lean_d2h; f.lean_visc = E->lean_visc;
    f.mont_history = E->mont_history; f.plain_sweeps = E->plain_sweeps; f.keep_diag = d.keep_diag != 0;
    f.mont_levels_valid = E->mont_levels_valid;
    return f;
}
// The one place that writes the per-launch fields of the view and what beom_info reports of the last step.
static void apply_plan(beom_engine *E, const StepPlan &p) {
    DevView &d = E->d;
    d.lean_d2h = p.mont.lean_d2h; d.keep_visc = p.mont.keep_visc; d.zero_visc = p.mont.zero_visc; d.stress_fold = p.stress_fold;
    E->last_folded = p.stress_fold;
    E->last_uv_fused = p.uv.fused_uv;
    E->last_mont_hist = p.uv.hm;
    E->last_plain = (p.uv.plain ? 1 : 0) | (p.mont.plain ? 2 : 0);
}

// the timer of a step, and of each part of a split step, if the step is sampled
static StepTimer *step_timer(beom_engine *E, int tstp) {
    StepTimer *T = (E->timer && tstp % E->timer->stride == 0) ? E->timer : nullptr;
    if (T) { T->st = E->stream; T->step(tstp); }
    return T;
}
// launches f, bracketed as kernel class c when the step is sampled
template <class F>
static void timed(StepTimer *T, int c, F &&f) {
    if (T) T->begin(c);
    f();
    if (T) T->end();
}

// The step up to the momentum sweeps: stress, the rebuild of steps 1-3, update_h, Montgomery + Leith.
static void step_front(beom_engine *E, const StepPlan &p, StepTimer *T) {
    apply_forcing(E, p.ctim);                                      // taus, hdot of this step's time, where they have frames
    if (p.launch_stress) launch_stress(E);
    if (E->lid) launch_lid_fluxes(E, p.first3);
    else if (p.rebuild) launch_rebuild(E);                         // :2166-2177
    if (E->ntrc > 0) timed(T, 7, [&] { launch_tracers(E, p.gene, p.ramp, p.ctim); });      // reads hlay, h_u, h_v as update_h is about to
    timed(T, 0, [&] {
        launch_h(E, p.gene, p.ramp, p.ctim);                       // :2181,2259
        if (E->lid) launch_lid_h_epilogue(E);                      // :1648-1700
    });
    timed(T, p.mont.fused ? 5 : 1, [&] {
        if (p.mont.fused) launch_mont_visc(E, p);                  // :2187-2188, 2266-2269 in one sweep
        else launch_mont(E, 0);
    });
    if (p.launch_visc) timed(T, 2, [&] { launch_visc(E, 0); });    // :2188,2268
}

// flt: -1 = the handle carries no floats; else bit 0 = the first step of its beom_step call, bit 1 = the last.  The float
// launches sit at the top and at the very end: stage 1 alone in front of the call's first step, stage 2 (+ the next step's
// stage 1, on the same velocities) behind every step.
static void one_step(beom_engine *E, const StepPlan &p, int flt = -1) {
    const int tstp = p.tstp;
    if (flt >= 0 && (flt & 1)) launch_floats(E, 1, nullptr);
    if (p.needs_arrays) (void)hist_sync(E);                        // a step on the arrays: bring them up to date first
    rotate_mont(E);                                                // the one place d.mont moves to its next buffer
    StepTimer *T = step_timer(E, tstp);
    apply_plan(E, p);
    step_front(E, p, T);
    if (E->mont_keep) E->mont_levels_valid = std::min(E->mont_levels_valid + 1, 3);      // this step's mont is in its buffer
    if (p.uv.fused_uv) timed(T, 6, [&] { launch_uv_fused(E, p); });
    else
        for (const bool x : {p.uv.first_x, !p.uv.first_x})
            timed(T, x ? 3 : 4, [&] {
                if (x) launch_uv<true>(E, 0, p.gene, p.ramp, p.ctim, p.uv.prod);
                else launch_uv<false>(E, 0, p.gene, p.ramp, p.ctim, p.uv.prod);
            });
    if (E->obc) {                                                  // :2201-2204, 2285-2288
        const dim3 g((unsigned)((E->d.nseg + BEOM_BLOCK - 1) / BEOM_BLOCK), (unsigned)E->d.nlay, 1);
        hipLaunchKernelGGL(k_no_gradient_obc, g, dim3(BEOM_BLOCK), 0, E->stream, E->d, 0);
        hipLaunchKernelGGL(k_no_gradient_obc, g, dim3(BEOM_BLOCK), 0, E->stream, E->d, 1);
    }
    if (E->lid) { launch_lid_fluxes(E, p.first3); launch_lid_pressure(E); }      // :2206-2222, 2290-2316
    if (flt >= 0) launch_floats_after(E, tstp, !(flt & 2));
    E->last_tstp = tstp; E->split.tstp = 0;      // (a whole step: no part 1 is pending)
    if (!E->mom_by_caller && accum_due(E->mom, tstp)) launch_moments(E, tstp);
    if (!E->mom_by_caller && accum_due(E->tmom, tstp)) launch_tracer_moments(E, tstp);
    if (!E->mom_by_caller && accum_due(E->harm.acc, tstp)) launch_harmonics(E, tstp, p.ctim);
    for (const Recorder *R : {&E->ser, &E->tser, &E->cser, &E->tcser, &E->maps})
        if (!R->by_caller && recorder_due(*R, tstp)) R->kind->launch(E, tstp);
}

// rows [jlo, jlo+nrows) of hlay,u,v,h_u,h_v  ->  dbuf (device memory, 5*nlay*nrows*(lm+1) doubles); the *2 forms move a second
// group of as many rows to / from a second buffer in the same launch
template <bool PACK>
static int rows_copy(beom_handle E, int jlo, int nrows, void *dbuf, int jlo2, void *dbuf2) {
    if (!E || !dbuf || jlo < 1 || nrows < 1 || jlo + nrows - 1 > E->d.M) return -3;
    if (dbuf2 && (jlo2 < 1 || jlo2 + nrows - 1 > E->d.M)) return -3;
    if (hipSetDevice(E->device) != hipSuccess) return -9;
    const long long total = 5ll * E->d.nlay * nrows * E->d.L;
    hipLaunchKernelGGL((k_rows_copy<PACK>), dim3((unsigned)((total + BEOM_BLOCK - 1) / BEOM_BLOCK), dbuf2 ? 2u : 1u), dim3(BEOM_BLOCK),
                       0, E->stream, E->d, jlo, nrows, (double *)dbuf, jlo2, (double *)dbuf2);
    if (E->ntrc > 0) {                  // the tracer contents behind the five fields
        const long long tq = (long long)E->ntrc * E->d.nlay * nrows * E->d.L;
        hipLaunchKernelGGL((k_rows_copy_q<PACK>), dim3((unsigned)((tq + BEOM_BLOCK - 1) / BEOM_BLOCK), dbuf2 ? 2u : 1u), dim3(BEOM_BLOCK),
                           0, E->stream, E->d, E->trc_q, E->ntrc, jlo, nrows, (double *)dbuf + total, jlo2, dbuf2 ? (double *)dbuf2 + total : nullptr);
    }
    return hipGetLastError() == hipSuccess ? 0 : -10;
}
extern "C" {

int beom_step(beom_handle E, int tstp_first, int nsteps, double tres, double dtd8, double dt_r,
              double rsta, int n_3d, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (tstp_first < 1 || nsteps < 0 || n_3d < 1) { set_err(errm, errm_len, "beom_step: bad arguments"); return -3; }
    if (E->P.flag_nudging && E->P.mcbc < 0.5 && !E->obc && !E->obc_set) { set_err(errm, errm_len, "beom_step: mcbc = 0 with nudging needs beom_set_open_boundaries (no_gradient_obc, private_mod.f95:2613-2679)"); return -6; }
    if (E->lid && !E->lid_ready) { set_err(errm, errm_len, "beom_step: rgld = 1 needs beom_set_rigid_lid (the Poisson operators Ow, Os, Osum_ and the lid pressure, private_mod.f95:505-563)"); return -6; }
    const bool flt = E->nflt > 0 && !E->flt_band;      // (a band's floats are launched by beom_multi_step, around the exchange)
    if (flt && !E->flt_ready) { set_err(errm, errm_len, "beom_step: the handle's %lld floats have no positions yet (beom_upload_floats)", E->nflt); return -3; }
    // a recorder must hold every record of the call: refused before anything is launched
    if (flt && E->flt_nrec > 0 &&
        !beom_recorder::holds(tstp_first, nsteps, E->flt_stride, E->flt_rec_tstp.size(), E->flt_nrec, errm, errm_len,
                              "beom_step: steps %d..%d would write %lld float records (stride %d) but the recorder holds %lld of %d: "
                              "empty it with beom_download_float_track, or take fewer steps per call")) return -3;
    for (const Recorder *R : {&E->ser, &E->tser, &E->cser, &E->tcser, &E->maps})
        if (R->level > 0 && !R->by_caller &&
            !beom_recorder::holds(tstp_first, nsteps, R->stride, R->tstp.size(), R->nrec, errm, errm_len, R->kind->overflow)) return -3;
    HIP_TRY(hipSetDevice(E->device));
    for (int tstp = tstp_first; tstp < tstp_first + nsteps; ++tstp)      // (the facts move with the steps: mont_levels_valid)
        one_step(E, beom_plan::plan_step(facts_of(E), tstp, tres, dtd8, dt_r, rsta, n_3d),
                 flt ? (tstp == tstp_first ? 1 : 0) | (tstp == tstp_first + nsteps - 1 ? 2 : 0) : -1);
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_profile_start(beom_handle E) {
    if (!E) return -1;
    if (E->timer) { for (hipEvent_t ev : E->timer->ev) (void)hipEventDestroy(ev); delete E->timer; }
    E->timer = new StepTimer();
    E->timer->st = E->stream;
    E->timer->stride = E->profile_stride;
    E->timer->rotate = E->profile_rotate;
    return 0;
}

int beom_profile_stop(beom_handle E, double *ms, int *launches, char *errm, int errm_len) {
    if (!E || !ms || !launches) { set_err(errm, errm_len, "null argument"); return -1; }
    if (!E->timer) { set_err(errm, errm_len, "beom_profile_stop without beom_profile_start"); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    StepTimer &T = *E->timer;
    for (int c = 0; c < 8; ++c) { ms[c] = 0.0; launches[c] = 0; }
    for (size_t k = 0; k < T.cls.size(); ++k) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, T.ev[2 * k], T.ev[2 * k + 1]);
        ms[T.cls[k]] += (double)t;
        launches[T.cls[k]] += 1;
    }
    for (hipEvent_t ev : T.ev) (void)hipEventDestroy(ev);
    delete E->timer;
    E->timer = nullptr;
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_profile_steps(beom_handle E, int tstp_first, int nsteps, double tres, double dtd8, double dt_r,
                       double rsta, int n_3d, double *ms, int *launches, char *errm, int errm_len) {
    int rc = beom_profile_start(E);
    if (rc) { set_err(errm, errm_len, "null handle"); return rc; }
    rc = beom_step(E, tstp_first, nsteps, tres, dtd8, dt_r, rsta, n_3d, errm, errm_len);
    if (rc) return rc;
    return beom_profile_stop(E, ms, launches, errm, errm_len);
}

// ---- split step for the ghost-row exchange overlap ------------------------
// A band's step in three parts, so that the rows the neighbours are waiting for are finished, packed and on their way
// while the bulk of the momentum sweep still runs — "boundary first" within ONE step; every part sees ghost rows that
// have landed, nothing in flight is read:
//   part 1: everything up to the momentum sweeps on all rows (stress, rebuild of steps 1-3, update_h, Montgomery + Leith);
//   part 2: the fused u+v sweep on the strips next to the ghost zones (rows 1..8 and M-7..M: the ghost rows and the
//           outermost owned rows, which are what beom_pack_rows sends) — the caller enqueues it on ANOTHER stream,
//           behind part 1, followed by pack -> transport -> unpack;
//   part 3: the same sweep on the rows in between, on the handle's usual stream, then the pointer rotations.
// The fused sweep writes out of place and every workgroup evaluates its own halo, so parts 2 and 3 may run side by side;
// the unpack writes rows 1..4 / M-3..M, part 3 reads no row below 6 / above M-5.  G = 4 ghost rows per neighbour
// (beom_amd/slab.py).  Needs the fused u+v sweep and no open-boundary pass; returns -20 when the caller must use
// beom_step instead (call part 1 first: it decides).
static void set_rows(DevView &d, int n, int lo0, int hi0, int lo1 = 1, int hi1 = 0) {
    d.nstrip = n; d.jlo0 = lo0; d.jhi0 = hi0; d.jlo1 = lo1; d.jhi1 = hi1;
}
constexpr int kEdgeRows = 8;           // ghost rows + the owned rows a neighbour receives

int beom_step_phase(beom_handle E, int tstp, double tres, double dtd8, double dt_r, double rsta, int n_3d,
                    int phase, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    DevView &d = E->d;
    if (E->P.flag_nudging && E->P.mcbc < 0.5 && !E->obc && !E->obc_set) { set_err(errm, errm_len, "beom_step_phase: mcbc = 0 with nudging needs beom_set_open_boundaries (no_gradient_obc, private_mod.f95:2613-2679)"); return -6; }
    const bool south = d.slab && d.joff > 0, north = d.slab && d.joff + d.M < d.Mg;
    // (svis > 0: a band's step stays whole)
    if (!beom_plan::fuses_uv(facts_of(E)) || !(south || north) || d.M < 4 * kEdgeRows || phase < 1 || phase > 3 || E->obc || E->lid || E->P.svis > 0.0) {
        set_err(errm, errm_len, "beom_step_phase: split step not available for this step/configuration");
        return -20;
    }
    const StepPlan &p = E->split;          // part 1 plans the step, parts 2 and 3 run from what it kept
    if (phase > 1 && (tstp < 1 || p.tstp != tstp)) {      // (the step's number is all that is matched; 0: no part 1 pending)
        set_err(errm, errm_len, "beom_step_phase: part %d of step %d, but part 1 prepared step %d", phase, tstp, p.tstp);
        return -3;
    }
    const int M = d.M;
    if (leave_mont_history(E)) { set_err(errm, errm_len, "beom_step_phase: the history arrays could not be brought up to date"); return -10; }
    if (phase == 1) E->split = beom_plan::plan_step(facts_of(E), tstp, tres, dtd8, dt_r, rsta, n_3d);      // (no levels kept: never hm)
    StepTimer *T = step_timer(E, tstp);
    if (phase == 1) {
        apply_plan(E, p);
        step_front(E, p, T);               // (p.uv.fused_uv holds: parts 2 and 3 are the fused u+v sweep it prepares)
    } else if (phase == 2) {
        // a side without a neighbour has no strip (its rows belong to part 3)
        if (south && north) set_rows(d, 2, 1, kEdgeRows, M - kEdgeRows + 1, M);
        else if (south) set_rows(d, 1, 1, kEdgeRows);
        else set_rows(d, 1, M - kEdgeRows + 1, M);
        timed(T, 6, [&] { launch_uv_fused(E, p, false); });
    } else {
        set_rows(d, 1, south ? kEdgeRows + 1 : 1, north ? M - kEdgeRows : M);
        timed(T, 6, [&] { launch_uv_fused(E, p, true); });
    }
    set_rows(d, 1, 1, M);
    E->last_tstp = tstp; if (phase == 3) E->split.tstp = 0;
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_pack_rows(beom_handle E, int jlo, int nrows, void *dbuf) { return rows_copy<true>(E, jlo, nrows, dbuf, 0, nullptr); }
int beom_unpack_rows(beom_handle E, int jlo, int nrows, const void *dbuf) { return rows_copy<false>(E, jlo, nrows, const_cast<void *>(dbuf), 0, nullptr); }
int beom_pack_rows2(beom_handle E, int nrows, int jlo_a, void *dbuf_a, int jlo_b, void *dbuf_b) {
    return rows_copy<true>(E, jlo_a, nrows, dbuf_a, jlo_b, dbuf_b);
}
int beom_unpack_rows2(beom_handle E, int nrows, int jlo_a, const void *dbuf_a, int jlo_b, const void *dbuf_b) {
    return rows_copy<false>(E, jlo_a, nrows, const_cast<void *>(dbuf_a), jlo_b, const_cast<void *>(dbuf_b));
}

// Output preparation on the device: replaces the array work of write_array for
// 'eta_', 'u___', 'v___' (private_mod.f95:2848-2883) and the min/max + thin-layer scans of
// write_outputs (:2772-2808).  Only real*4 records cross PCIe.
int beom_download_outputs(beom_handle E, const float *h0r4, float *eta, float *u4, float *v4,
                          double *minmax, int *thin_layer, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    DevView &d = E->d;
    const size_t n = (size_t)d.ndeg * d.nlay;
    if (!E->h0r4_dev) {
        if (!h0r4) { set_err(errm, errm_len, "beom_download_outputs: h_0 (real*4) needed on the first call"); return -3; }
        HIP_TRY(hipMalloc((void **)&E->h0r4_dev, n * sizeof(float)));
        E->allocs.push_back(E->h0r4_dev);
        for (int q = 0; q < 3; ++q) { HIP_TRY(hipMalloc((void **)&E->out4[q], n * sizeof(float))); E->allocs.push_back(E->out4[q]); }
        const size_t nb = (size_t)E->grid_cells0.x;
        HIP_TRY(hipMalloc((void **)&E->scan_dev, nb * d.nlay * 7 * sizeof(double)));
        E->allocs.push_back(E->scan_dev);
    }
    if (h0r4) HIP_TRY(hipMemcpyAsync(E->h0r4_dev, h0r4, n * sizeof(float), hipMemcpyHostToDevice, E->stream));
    const unsigned gx = (unsigned)((d.ncell + BEOM_BLOCK - 1) / BEOM_BLOCK);
    if (eta || u4 || v4) {
        hipLaunchKernelGGL(k_out_convert, dim3(gx), dim3(BEOM_BLOCK), 0, E->stream, d, E->h0r4_dev,
                           eta ? E->out4[0] : nullptr, u4 ? E->out4[1] : nullptr, v4 ? E->out4[2] : nullptr);
        float *host[3] = {eta, u4, v4};
        for (int q = 0; q < 3; ++q)
            if (host[q]) HIP_TRY(hipMemcpyAsync(host[q], E->out4[q], n * sizeof(float), hipMemcpyDeviceToHost, E->stream));
    }
    if (minmax || thin_layer) {
        const size_t nb = (size_t)E->grid_cells0.x;
        hipLaunchKernelGGL(k_out_scan, E->grid_cells0, dim3(BEOM_BLOCK), 0, E->stream, d, E->any_u, E->any_v, E->scan_dev);
        std::vector<double> part(nb * d.nlay * 7);
        HIP_TRY(hipMemcpyAsync(part.data(), E->scan_dev, part.size() * sizeof(double), hipMemcpyDeviceToHost, E->stream));
        HIP_TRY(hipStreamSynchronize(E->stream));
        if (thin_layer) *thin_layer = 0;
        for (int k = 0; k < d.nlay; ++k) {
            double r[7] = {1.7976931348623157e308, -1.7976931348623157e308, 1.7976931348623157e308,
                           -1.7976931348623157e308, 1.7976931348623157e308, -1.7976931348623157e308, 0.0};
            for (size_t b = 0; b < nb; ++b) {
                const double *p = &part[(b * d.nlay + k) * 7];
                for (int q = 0; q < 7; ++q) r[q] = (q == 0 || q == 2 || q == 4) ? std::fmin(r[q], p[q]) : std::fmax(r[q], p[q]);
            }
            if (minmax) for (int q = 0; q < 6; ++q) minmax[k * 6 + q] = r[q];
            if (thin_layer && r[6] > 0.5 && *thin_layer == 0) *thin_layer = k + 1;
        }
    }
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

// The three `diag` records of write_array (private_mod.f95:2884-2974) formed on the device: only real*4 crosses PCIe.
// Between time steps only: the work arrays are the step's d2hx / d2hy scratch (pcd / qlr with a lid), dead between the steps
// of every form test_gpu_outputs.py runs a download in front of and names by an assertion — the fused pair with the history
// kept in arrays or rebuilt from the Montgomery levels, keep_diag = 1, the folded stress, tiled biharmonic viscosity,
// dt3d > 0, 12 layers, the rectangle with land, the table path, the lid (state and scratch of the next step bit for bit),
// bands and a ring (state).
int beom_download_diag(beom_handle E, float *pvor4, float *mont4, float *vcc4, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    DevView &d = E->d;
    const size_t n = (size_t)d.ndeg * d.nlay;
    float *dst[3] = {pvor4, mont4, vcc4};
    if (!E->diag4[0])
        for (int q = 0; q < 3; ++q) { HIP_TRY(hipMalloc((void **)&E->diag4[q], n * sizeof(float))); E->allocs.push_back(E->diag4[q]); }
    const dim3 g = E->grid_cells_layers_flat, b(BEOM_BLOCK);
    // work arrays: scratch that is dead between steps — the curvatures, or with a lid (whose next step reads the stored
    // curvatures of the last layer, :2237-2257) the product arrays of the fused sweeps, which a lid handle never runs
    double *w1 = E->lid ? d.pcd : d.d2hx, *w2 = E->lid ? d.qlr : d.d2hy;
    if (vcc4) hipLaunchKernelGGL(k_diag_w12, g, b, 0, E->stream, d, w1, w2);
    hipLaunchKernelGGL(k_diag_records, g, b, 0, E->stream, d, (const double *)w1, (const double *)w2,
                       pvor4 ? E->diag4[0] : nullptr, mont4 ? E->diag4[1] : nullptr, vcc4 ? E->diag4[2] : nullptr);
    for (int q = 0; q < 3; ++q)
        if (dst[q]) HIP_TRY(hipMemcpyAsync(dst[q], E->diag4[q], n * sizeof(float), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- conservation integrals (beom_integrals.h) -----------------------------------------------------------------------
int beom_integral_count(int nlay) { return 4 * nlay + 1; }

// Whether the frame wraps (integ_xper, integ_yper) and, on the table path, the packed cell of every (i, j) (integ_cellmap):
// built on the first use by the integrals or by the floats.
static int ensure_cellmap(beom_engine *E, char *errm, int errm_len) {
    if (E->cellmap_known) return 0;
    DevView &d = E->d;
    E->integ_xper = d.xper; E->integ_yper = d.yper;
    if (!E->dense) {
        int32_t *flags = nullptr;
        HIP_TRY(hipMalloc((void **)&E->integ_cellmap, ((size_t)d.L * d.M + 2) * sizeof(int32_t)));
        E->allocs.push_back(E->integ_cellmap);
        HIP_TRY(hipMemsetAsync(E->integ_cellmap, 0, ((size_t)d.L * d.M + 2) * sizeof(int32_t), E->stream));
        flags = E->integ_cellmap + (size_t)d.L * d.M;
        hipLaunchKernelGGL(k_integral_cellmap, dim3((unsigned)((d.ndeg + BEOM_BLOCK - 1) / BEOM_BLOCK)), dim3(BEOM_BLOCK), 0, E->stream,
                           d, E->integ_cellmap, flags);
        int32_t fl[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(fl, flags, sizeof(fl), hipMemcpyDeviceToHost, E->stream));
        HIP_TRY(hipStreamSynchronize(E->stream));
        E->integ_xper = fl[0]; E->integ_yper = fl[1];
    }
    E->cellmap_known = true;
    return 0;
}

// The chunk sums and row sums of up to M rows of `count` entries each: allocated on the first use, again when a later user
// (the series at level 2) asks for more entries per row.
static int ensure_integ_scratch(beom_engine *E, int count, char *errm, int errm_len) {
    if (E->integ_count >= count) return 0;
    const DevView &d = E->d;
    const int nch = (d.L + 63) / 64;
    if (E->integ_part) {
        HIP_TRY(hipStreamSynchronize(E->stream));
        for (double **p : {&E->integ_part, &E->integ_rows}) {
            E->allocs.erase(std::remove(E->allocs.begin(), E->allocs.end(), (void *)*p), E->allocs.end());
            (void)hipFree(*p);
            *p = nullptr;
        }
        E->integ_count = 0;
    }
    HIP_TRY(hipMalloc((void **)&E->integ_part, (size_t)d.M * nch * count * sizeof(double)));
    E->allocs.push_back(E->integ_part);
    HIP_TRY(hipMalloc((void **)&E->integ_rows, (size_t)d.M * count * sizeof(double)));
    E->allocs.push_back(E->integ_rows);
    E->integ_count = count;
    return 0;
}

int beom_integral_rows(beom_handle E, int jlo, int nrows, double *rows, char *errm, int errm_len) {
    if (!E || !rows) { set_err(errm, errm_len, "beom_integral_rows: null argument"); return -1; }
    DevView &d = E->d;
    if (jlo < 1 || nrows < 1 || jlo + nrows - 1 > d.M) { set_err(errm, errm_len, "beom_integral_rows: rows %d..%d outside 1..%d", jlo, jlo + nrows - 1, d.M); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const int count = 4 * d.nlay + 1;
    const RowTree t = row_tree(d.L);
    if (t.nchp2 / 64 > kIntegralMaxGroups) { set_err(errm, errm_len, "beom_integral_rows: rows of more than %d columns", 64 * 64 * kIntegralMaxGroups); return -4; }
    if (const int rc = ensure_integ_scratch(E, count, errm, errm_len)) return rc;
    if (const int rc = ensure_cellmap(E, errm, errm_len)) return rc;
    const dim3 g((unsigned)t.nch, (unsigned)((nrows + BEOM_TILE_Y - 1) / BEOM_TILE_Y), 1), b(BEOM_BLOCK);
    if (E->dense) hipLaunchKernelGGL(k_integral_rows<true>, g, b, 0, E->stream, d, jlo, nrows, t.width, E->integ_xper, E->integ_yper,
                                     (const int32_t *)nullptr, E->integ_part);
    else hipLaunchKernelGGL(k_integral_rows<false>, g, b, 0, E->stream, d, jlo, nrows, t.width, E->integ_xper, E->integ_yper,
                            (const int32_t *)E->integ_cellmap, E->integ_part);
    const long long nt = (long long)nrows * count;
    hipLaunchKernelGGL(k_integral_chunks, dim3((unsigned)nrows), dim3(64), 0, E->stream,
                       (const double *)E->integ_part, E->integ_rows, count, t.nch, t.nchp2);
    HIP_TRY(hipMemcpyAsync(rows, E->integ_rows, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

// host only: the tree over the row sums, rows padded with +0.0 to the next power of two
int beom_integral_combine(const double *rows, int nrows_total, int count, double *out) {
    if (!rows || !out || nrows_total < 1 || count < 1) return -1;
    const int n2 = pow2_ceil(nrows_total);
    std::vector<double> w((size_t)n2);
    for (int k = 0; k < count; ++k) {
        for (int r = 0; r < n2; ++r) w[(size_t)r] = r < nrows_total ? rows[(size_t)r * count + k] : 0.0;
        for (int n = n2; n > 1; n >>= 1)
            for (int m = 0; m < n / 2; ++m) w[(size_t)m] = w[(size_t)(2 * m)] + w[(size_t)(2 * m + 1)];
        out[k] = w[0];
    }
    return 0;
}

int beom_integrals(beom_handle E, double *out, char *errm, int errm_len) {
    if (!E || !out) { set_err(errm, errm_len, "beom_integrals: null argument"); return -1; }
    const int count = 4 * E->d.nlay + 1, M = E->d.M;
    std::vector<double> rows((size_t)M * count);
    const int rc = beom_integral_rows(E, 1, M, rows.data(), errm, errm_len);
    if (rc) return rc;
    return beom_integral_combine(rows.data(), M, count, out);
}

// ---- the recorders: series of row sums (beom_series.h) and tracer series (beom_tracer_series.h) ---------------------------
int beom_series_count(int nlay, int level) { return (level >= 2 ? 6 : 4) * nlay + 1; }
int beom_tracer_series_count(int ntrc, int nlay, int level) { return ntrc * nlay * 2 * level; }

// The series' chunk partials go to the integrals' scratch, sized for the larger count.
static int series_scratch(beom_engine *E, Recorder &, int cnt, int, char *errm, int errm_len) {
    if (const int rc = ensure_integ_scratch(E, cnt, errm, errm_len)) return rc;
    return ensure_cellmap(E, errm, errm_len);
}
// The tracer series' chunk partials of a launch stay under this many bytes: a record is taken in batches of rows (whole
// workgroups of BEOM_TILE_Y rows; never fewer than one), every row finished on its own, so the batches cannot change a bit.
constexpr size_t kTracerSeriesScratch = 64u << 20;
static int tracer_series_scratch(beom_engine *E, Recorder &R, int cnt, int nrows, char *errm, int errm_len) {
    const size_t per_row = (size_t)row_tree(E->d.L).nch * cnt;
    size_t batch = E->tser_batch_opt > 0 ? (size_t)E->tser_batch_opt : kTracerSeriesScratch / (per_row * sizeof(double));
    batch = std::max<size_t>(batch / BEOM_TILE_Y * BEOM_TILE_Y, BEOM_TILE_Y);
    batch = std::min<size_t>(batch, (size_t)nrows);
    R.batch = (int)batch;
    if (const int rc = ensure_cellmap(E, errm, errm_len)) return rc;
    return alloc_plain(E, R.allocs, &R.part, batch * per_row, errm, errm_len, false);
}

static void recorder_free(Recorder &R) {
    free_list(R.allocs);
    R.level = 0; R.stride = 1; R.nrec = 0; R.jlo = 1; R.rows = 0; R.batch = 0; R.by_caller = false; R.wlo = 1; R.whi = 0;
    R.rec = R.part = nullptr;
    R.tstp.clear();
}

// level 0 frees; else a recorder of nrec records of local rows jlo .. jlo+nrows-1.  A failed allocation leaves level 0
static int recorder_set(beom_engine *E, Recorder beom_engine::*which, const char *who, int level, int stride, int nrec, int jlo,
                        int nrows, bool by_caller, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    Recorder &R = E->*which;
    const RecorderKind &K = *R.kind;
    if (level < 0 || level > K.max_level || (level > 0 && (stride < 1 || nrec < 1))) {
        set_err(errm, errm_len, "%s: level %d, stride %d, %d records (level 0..%d, stride >= 1, records >= 1)", who, level, stride, nrec, K.max_level);
        return -3;
    }
    if (K.no_tracer && level > 0 && E->ntrc < 1) { set_err(errm, errm_len, K.no_tracer, who); return -3; }
    const DevView &d = E->d;
    if (level > 0 && (jlo < 1 || nrows < 1 || jlo + nrows - 1 > d.M)) { set_err(errm, errm_len, "%s: rows %d..%d outside 1..%d", who, jlo, jlo + nrows - 1, d.M); return -3; }
    if (K.columns && level > 0 && (d.slab || d.joff != 0 || d.Mg != d.M)) {
        set_err(errm, errm_len, "%s: a handle on a band of rows keeps no %s (a column's tree crosses the bands)", who, K.what);
        return -6;
    }
    if (!K.columns && !K.lines && level > 0 && row_tree(d.L).nchp2 / 64 > kIntegralMaxGroups) { set_err(errm, errm_len, "%s: rows of more than %d columns", who, 64 * 64 * kIntegralMaxGroups); return -4; }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    recorder_free(R);
    if (level == 0) return 0;
    const int cnt = K.count(E->ntrc, d.nlay, level);
    const int wlo = jlo, whi = jlo + nrows - 1;
    if (K.columns) { jlo = 1; nrows = d.L; }          // (the lines of the record are the columns)
    if (K.lines) { jlo = 1; nrows = K.lines(E); }     // (the maps: its blocks)
    int rc = K.scratch(E, R, cnt, nrows, errm, errm_len);
    if (!rc) rc = alloc_aligned(E, R.allocs, &R.rec, (size_t)nrec * nrows * cnt, errm, errm_len);
    if (rc) { recorder_free(R); return rc; }
    R.level = level; R.stride = stride; R.nrec = nrec; R.jlo = jlo; R.rows = nrows; R.by_caller = by_caller; R.wlo = wlo; R.whi = whi;
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

static int recorder_sample(beom_engine *E, Recorder beom_engine::*which) {
    if (!E) return -1;
    const Recorder &R = E->*which;
    if (R.level < 1 || (int)R.tstp.size() >= R.nrec) return -3;
    if (hipSetDevice(E->device) != hipSuccess) return -9;
    R.kind->launch(E, E->last_tstp);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// the records held, oldest first, with their steps; empties the recorder
static int recorder_download(beom_engine *E, Recorder beom_engine::*which, double *rows, int *tstp, int *count, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    Recorder &R = E->*which;
    if (R.level < 1) { set_err(errm, errm_len, "%s", R.kind->none); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const size_t n = R.tstp.size(), per = (size_t)R.rows * R.kind->count(E->ntrc, E->d.nlay, R.level);
    if (rows && n) {
        HIP_TRY(hipMemcpyAsync(rows, R.rec, n * per * sizeof(double), hipMemcpyDeviceToHost, E->stream));
        HIP_TRY(hipStreamSynchronize(E->stream));
        HIP_TRY(hipGetLastError());
    }
    if (tstp) std::copy(R.tstp.begin(), R.tstp.end(), tstp);
    if (count) *count = (int)n;
    R.tstp.clear();
    return 0;
}

int beom_set_series(beom_handle E, int level, int stride, int nrec, char *errm, int errm_len) {
    return recorder_set(E, &beom_engine::ser, "beom_set_series", level, stride, nrec, 1, E ? E->d.M : 0, false, errm, errm_len);
}
int beom_band_set_series(beom_handle E, int level, int stride, int nrec, int jlo, int nrows, char *errm, int errm_len) {
    return recorder_set(E, &beom_engine::ser, "beom_band_set_series", level, stride, nrec, jlo, nrows, true, errm, errm_len);
}
int beom_set_tracer_series(beom_handle E, int level, int stride, int nrec, char *errm, int errm_len) {
    return recorder_set(E, &beom_engine::tser, "beom_set_tracer_series", level, stride, nrec, 1, E ? E->d.M : 0, false, errm, errm_len);
}
int beom_band_set_tracer_series(beom_handle E, int level, int stride, int nrec, int jlo, int nrows, char *errm, int errm_len) {
    return recorder_set(E, &beom_engine::tser, "beom_band_set_tracer_series", level, stride, nrec, jlo, nrows, true, errm, errm_len);
}

int beom_set_column_series(beom_handle E, int level, int stride, int nrec, int jlo, int jhi, char *errm, int errm_len) {
    return recorder_set(E, &beom_engine::cser, "beom_set_column_series", level, stride, nrec, jlo, jhi - jlo + 1, false, errm, errm_len);
}
int beom_sample_column_series(beom_handle E) { return recorder_sample(E, &beom_engine::cser); }
int beom_download_column_series(beom_handle E, double *cols, int *tstp, int *count, char *errm, int errm_len) {
    return recorder_download(E, &beom_engine::cser, cols, tstp, count, errm, errm_len);
}
int beom_set_tracer_column_series(beom_handle E, int level, int stride, int nrec, int jlo, int jhi, char *errm, int errm_len) {
    return recorder_set(E, &beom_engine::tcser, "beom_set_tracer_column_series", level, stride, nrec, jlo, jhi - jlo + 1, false, errm, errm_len);
}
int beom_sample_tracer_column_series(beom_handle E) { return recorder_sample(E, &beom_engine::tcser); }
int beom_download_tracer_column_series(beom_handle E, double *cols, int *tstp, int *count, char *errm, int errm_len) {
    return recorder_download(E, &beom_engine::tcser, cols, tstp, count, errm, errm_len);
}
// Maps (beom_maps.h): the block edge is checked here and kept beside the recorder; the rest is the recorders' own.
int beom_maps_count(int ntrc, int nlay, int level) {
    return level < 1 ? 0 : 1 + (level >= 2 ? 6 : 3) * nlay + (level >= 3 ? ntrc * nlay : 0);
}
int beom_set_maps(beom_handle E, int level, int block, int stride, int nrec, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    int logb = 0;
    while (logb < kMapMaxLog && (1 << logb) < block) ++logb;
    if (level < 0 || level > kMaps.max_level || (level > 0 && (block < 2 || block != (1 << logb) || stride < 1 || nrec < 1))) {
        set_err(errm, errm_len, "beom_set_maps: level %d, block %d, stride %d, %d records (level 0..%d, block a power of two in 2..%d, "
                                "stride >= 1, records >= 1)", level, block, stride, nrec, kMaps.max_level, 1 << kMapMaxLog);
        return -3;
    }
    if (level >= 3 && E->ntrc < 1) { set_err(errm, errm_len, kTracerSeries.no_tracer, "beom_set_maps"); return -3; }
    if (level > 0 && (E->d.slab || E->d.joff != 0 || E->d.Mg != E->d.M)) {
        set_err(errm, errm_len, "beom_set_maps: a handle on a band of rows keeps no maps (a block's tree must not cross a seam, and "
                                "nothing aligns the seams to the block edge yet)");
        return -6;
    }
    if (level > 0) E->maps_logb = logb;       // (before the recorder is sized: maps_lines)
    return recorder_set(E, &beom_engine::maps, "beom_set_maps", level, stride, nrec, 1, E->d.M, false, errm, errm_len);
}
int beom_sample_maps(beom_handle E) { return recorder_sample(E, &beom_engine::maps); }
int beom_download_maps(beom_handle E, double *maps, int *tstp, int *count, char *errm, int errm_len) {
    return recorder_download(E, &beom_engine::maps, maps, tstp, count, errm, errm_len);
}
int beom_sample_series(beom_handle E) { return recorder_sample(E, &beom_engine::ser); }
int beom_sample_tracer_series(beom_handle E) { return recorder_sample(E, &beom_engine::tser); }

int beom_download_series(beom_handle E, double *rows, int *tstp, int *count, char *errm, int errm_len) {
    return recorder_download(E, &beom_engine::ser, rows, tstp, count, errm, errm_len);
}
int beom_download_tracer_series(beom_handle E, double *rows, int *tstp, int *count, char *errm, int errm_len) {
    return recorder_download(E, &beom_engine::tser, rows, tstp, count, errm, errm_len);
}

// ---- passive tracers (beom_tracers.h) -----------------------------------------------------------------------------------
static void accum_free(Accum &A);
static void free_tracer_mixing(beom_engine *E) {
    free_list(E->trc_mix_allocs);
    E->trc_mix = nullptr;
}
static void free_tracer_vmixing(beom_engine *E) {
    free_list(E->trc_vmix_allocs);
    E->trc_vmix = nullptr;
}
static void free_tracers(beom_engine *E) {
    free_list(E->trc_allocs);
    E->ntrc = 0;
    E->trc_q = E->trc_q_alt = E->trc_rq[0] = E->trc_rq[1] = E->trc_ctrg = nullptr;
}
int beom_set_tracers(beom_handle E, int ntrc, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (ntrc < 0 || ntrc > BEOM_MAX_TRACERS) { set_err(errm, errm_len, "beom_set_tracers: %d tracers (0..%d)", ntrc, BEOM_MAX_TRACERS); return -3; }
    if (ntrc > 0 && E->P.variant == 1) { set_err(errm, errm_len, "beom_set_tracers: variant 1 changes the thickness in an epilogue (private_mod3d.f95:1635-1683) that the tracer scheme does not follow"); return -6; }
    if (ntrc > 0 && E->lid) { set_err(errm, errm_len, "beom_set_tracers: rgld = 1 changes the thickness in the lid's misfit epilogue (private_mod.f95:1648-1700), which the tracer scheme does not follow"); return -6; }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    if (ntrc != E->ntrc) { accum_free(E->tmom); free_tracer_mixing(E); free_tracer_vmixing(E); recorder_free(E->tser); recorder_free(E->tcser); if (E->maps.level >= 3) recorder_free(E->maps); }        // (their arrays have the tracers' shape)
    free_tracers(E);
    if (ntrc == 0) return 0;
    E->ntrc = ntrc;
    int rc = 0;
    for (double **a : {&E->trc_q, &E->trc_q_alt, &E->trc_rq[0], &E->trc_rq[1]})
        if ((rc = alloc_aligned(E, E->trc_allocs, a, tracer_cells(E), errm, errm_len))) { free_tracers(E); return rc; }
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

// the scheme of the tracer sweep; kept for the handle's life (beom_set_tracers leaves it).  The argument is looked at first
int beom_set_tracer_scheme(beom_handle E, int scheme, char *errm, int errm_len) {
    if (scheme != 1 && scheme != 2) { set_err(errm, errm_len, "beom_set_tracer_scheme: scheme %d (1 = upstream, 2 = limited)", scheme); return -3; }
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    E->trc_scheme = scheme;
    return 0;
}

// Diffusion, decay and sources (beom_tracer_mix.h).  Everything is looked at before anything is touched; all null or all
// zero switches the mixing off and frees the coefficients.
int beom_set_tracer_mixing(beom_handle E, const double *kappa, const double *decay, const double *source, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (E->ntrc < 1) { set_err(errm, errm_len, "beom_set_tracer_mixing: the handle carries no tracer (beom_set_tracers comes first)"); return -3; }
    const int per = E->ntrc * E->d.nlay;
    // (the caps allow for the roundings of a coefficient that was itself computed as 0.25*dl*dl/dt or 1/dt)
    const double dt = E->d.dt, cfl = dt / (E->d.dl * E->d.dl), slack = 1.0 + 8.0 * 2.220446049250313e-16;
    std::vector<double> co(3 * (size_t)per, 0.0);
    const double *src[3] = {kappa, decay, source};
    const char *nm[3] = {"kappa", "decay", "source"};
    bool any = false;
    for (int k = 0; k < 3; ++k)
        for (int i = 0; src[k] && i < per; ++i) {
            const double v = src[k][i];
            const int t = i / E->d.nlay + 1, l = i % E->d.nlay + 1;
            if (!std::isfinite(v)) { set_err(errm, errm_len, "beom_set_tracer_mixing: %s of tracer %d, layer %d is not finite", nm[k], t, l); return -3; }
            if (k < 2 && v < 0.0) { set_err(errm, errm_len, "beom_set_tracer_mixing: %s of tracer %d, layer %d is negative (%g)", nm[k], t, l, v); return -3; }
            if (k == 0 && v * cfl > 0.25 * slack) { set_err(errm, errm_len, "beom_set_tracer_mixing: kappa of tracer %d, layer %d: kappa*dt/dl^2 = %g exceeds 0.25 (the forward step's maximum principle)", t, l, v * cfl); return -3; }
            if (k == 1 && v * dt > slack) { set_err(errm, errm_len, "beom_set_tracer_mixing: decay of tracer %d, layer %d: decay*dt = %g exceeds 1 (the forward step would change the sign)", t, l, v * dt); return -3; }
            co[(size_t)k * per + i] = v == 0.0 ? 0.0 : v;       // (-0 counts as +0)
            any = any || v != 0.0;
        }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    if (!any) { free_tracer_mixing(E); return 0; }
    int rc;
    if (!E->trc_mix && (rc = alloc_plain(E, E->trc_mix_allocs, &E->trc_mix, co.size(), errm, errm_len))) { free_tracer_mixing(E); return rc; }
    HIP_TRY(hipMemcpyAsync(E->trc_mix, co.data(), co.size() * sizeof(double), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

// Vertical diffusion (beom_tracer_vmix.h).  Everything is looked at before anything is touched; null or all zero switches it
// off and frees the coefficients.  The device holds rk = 1 / (dt * kappa_v), +0 where kappa_v is 0: a closed interface.
int beom_set_tracer_vmixing(beom_handle E, const double *kappa_v, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (E->ntrc < 1) { set_err(errm, errm_len, "beom_set_tracer_vmixing: the handle carries no tracer (beom_set_tracers comes first)"); return -3; }
    const int nk = E->d.nlay - 1;
    if (kappa_v && nk < 1) { set_err(errm, errm_len, "beom_set_tracer_vmixing: a handle with one layer has no interface to mix through"); return -3; }
    const double dt = E->d.dt;
    std::vector<double> rk(kappa_v ? (size_t)E->ntrc * nk : 0, 0.0);
    bool any = false;
    for (size_t i = 0; i < rk.size(); ++i) {
        const double v = kappa_v[i];
        const int t = (int)(i / nk) + 1, k = (int)(i % nk) + 1;
        if (!std::isfinite(v)) { set_err(errm, errm_len, "beom_set_tracer_vmixing: kappa_v of tracer %d, interface %d is not finite", t, k); return -3; }
        if (v < 0.0) { set_err(errm, errm_len, "beom_set_tracer_vmixing: kappa_v of tracer %d, interface %d is negative (%g)", t, k, v); return -3; }
        if (v == 0.0) continue;                                 // (-0 counts as +0)
        const double prod = dt * v;
        const double r = 1.0 / prod;
        if (!(std::isnormal(r) && r > 0.0)) { set_err(errm, errm_len, "beom_set_tracer_vmixing: kappa_v of tracer %d, interface %d: 1/(dt*kappa_v) = %g is no positive normal number (dt*kappa_v = %g)", t, k, r, prod); return -3; }
        rk[i] = r;
        any = true;
    }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    if (!any) { free_tracer_vmixing(E); return 0; }
    int rc;
    if (!E->trc_vmix && (rc = alloc_plain(E, E->trc_vmix_allocs, &E->trc_vmix, rk.size(), errm, errm_len))) { free_tracer_vmixing(E); return rc; }
    HIP_TRY(hipMemcpyAsync(E->trc_vmix, rk.data(), rk.size() * sizeof(double), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

int beom_upload_tracers(beom_handle E, const double *q, const double *rq, const double *ctrg, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (E->ntrc < 1) { set_err(errm, errm_len, "beom_upload_tracers: the handle carries no tracer (beom_set_tracers)"); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const int outer = E->ntrc * E->d.nlay;
    int rc;
    if (ctrg && !E->trc_ctrg && (rc = alloc_aligned(E, E->trc_allocs, &E->trc_ctrg, tracer_cells(E), errm, errm_len))) return rc;
    if ((rc = copy_in(E, E->trc_q, q, (size_t)outer, errm, errm_len))) return rc;
    if ((rc = copy_in(E, E->trc_ctrg, ctrg, (size_t)outer, errm, errm_len))) return rc;
    if ((rc = hist_in(E, E->trc_rq, 2, rq, errm, errm_len, outer))) return rc;
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_download_tracers(beom_handle E, double *q, double *rq, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (E->ntrc < 1) { set_err(errm, errm_len, "beom_download_tracers: the handle carries no tracer (beom_set_tracers)"); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const int outer = E->ntrc * E->d.nlay;
    int rc;
    if ((rc = copy_out(E, q, E->trc_q, (size_t)outer, errm, errm_len))) return rc;
    if ((rc = hist_out(E, E->trc_rq, 2, rq, errm, errm_len, outer))) return rc;
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- Lagrangian floats (beom_floats.h) -------------------------------------------------------------------------------------
static void free_floats(beom_engine *E) {
    free_list(E->flt_allocs);
    E->nflt = 0; E->flt_ready = false; E->flt_nrec = 0; E->flt_stride = 1;
    E->flt_rec_tstp.clear();
    E->flt_x = E->flt_y = E->flt_k1x = E->flt_k1y = E->flt_xs = E->flt_ys = E->flt_rec = nullptr;
    E->flt_layer = E->flt_rej = nullptr;
    E->flt_first_dry = nullptr;
    E->flt_band = false; E->flt_fb = FloatBand{}; E->flt_in_s = E->flt_in_n = nullptr; E->flt_handovers = 0;
}
int beom_set_floats(beom_handle E, int64_t n, int nrec, int stride, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (n < 0 || nrec < 0 || stride < 1) { set_err(errm, errm_len, "beom_set_floats: %lld floats, %d records, stride %d (n >= 0, nrec >= 0, stride >= 1)", (long long)n, nrec, stride); return -3; }
    if (n > 0 && (double)n * 3.0 * (double)std::max(nrec, 1) >= 9.0e15) { set_err(errm, errm_len, "beom_set_floats: %lld floats x %d records is too much", (long long)n, nrec); return -3; }
    if (n > 0 && E->d.slab) {
        set_err(errm, errm_len, "beom_set_floats: this handle holds one band of rows (slab_mm = %d): a float leaves its band, and floats do not "
                "migrate between devices yet; carry them on a single handle of the whole frame", E->P.slab_mm);
        return -6;
    }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    free_floats(E);
    if (n == 0) return 0;
    int rc = ensure_cellmap(E, errm, errm_len);
    if (rc) return rc;
    E->nflt = (long long)n;
    const size_t m = (size_t)n;
    for (double **a : {&E->flt_x, &E->flt_y, &E->flt_k1x, &E->flt_k1y, &E->flt_xs, &E->flt_ys})
        if ((rc = alloc_plain(E, E->flt_allocs, a, m, errm, errm_len))) { free_floats(E); return rc; }
    for (int32_t **a : {&E->flt_layer, &E->flt_rej})
        if ((rc = alloc_plain(E, E->flt_allocs, a, m, errm, errm_len))) { free_floats(E); return rc; }
    if ((rc = alloc_plain(E, E->flt_allocs, &E->flt_first_dry, 1, errm, errm_len))) { free_floats(E); return rc; }
    if (nrec > 0 && (rc = alloc_plain(E, E->flt_allocs, &E->flt_rec, 3 * m * (size_t)nrec, errm, errm_len))) { free_floats(E); return rc; }
    E->flt_nrec = nrec; E->flt_stride = stride;
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

int beom_upload_floats(beom_handle E, const double *x, const double *y, const int32_t *layer, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (E->flt_band) { set_err(errm, errm_len, "beom_upload_floats: this handle is a band; its floats belong to the multi handle (beom_multi_upload_floats)"); return -3; }
    if (E->nflt < 1) { set_err(errm, errm_len, "beom_upload_floats: the handle carries no float (beom_set_floats)"); return -3; }
    if (!x || !y || !layer) { set_err(errm, errm_len, "beom_upload_floats: null array"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    const DevView &d = E->d;
    const size_t n = (size_t)E->nflt;
    long long bad_layer = -1;
    for (size_t t = 0; t < n && bad_layer < 0; ++t)
        if (layer[t] < 1 || layer[t] > d.nlay) bad_layer = (long long)t;
    // the candidates go to the scratch of stage 1; the floats the handle holds are replaced only if every one is accepted
    const unsigned long long none = ~0ull;
    unsigned long long first_dry = none;
    HIP_TRY(hipMemcpyAsync(E->flt_xs, x, n * sizeof(double), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipMemcpyAsync(E->flt_ys, y, n * sizeof(double), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipMemcpyAsync(E->flt_first_dry, &none, sizeof(none), hipMemcpyHostToDevice, E->stream));
    const FloatView f = float_view(E, nullptr);
    const dim3 g((unsigned)((E->nflt + BEOM_BLOCK - 1) / BEOM_BLOCK)), b(BEOM_BLOCK);
    if (E->dense) hipLaunchKernelGGL(k_floats_check<CellDense>, g, b, 0, E->stream, d, f, E->flt_first_dry);
    else hipLaunchKernelGGL(k_floats_check<CellGather>, g, b, 0, E->stream, d, f, E->flt_first_dry);
    HIP_TRY(hipMemcpyAsync(&first_dry, E->flt_first_dry, sizeof(first_dry), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    if (bad_layer >= 0 && (first_dry == none || (unsigned long long)bad_layer <= first_dry)) {
        set_err(errm, errm_len, "beom_upload_floats: float %lld has layer %d, outside 1..%d (nothing uploaded)", bad_layer, (int)layer[bad_layer], d.nlay);
        return -3;
    }
    if (first_dry != none) {
        const double px = x[first_dry], py = y[first_dry];
        set_err(errm, errm_len, "beom_upload_floats: float %llu at (%.17g, %.17g) does not start in a wet cell: cell (%.0f, %.0f) of the "
                "%d x %d frame is dry, land or outside (nothing uploaded)", first_dry, px, py, std::floor(px) + 1.0, std::floor(py) + 1.0, d.lm, d.mm);
        return -3;
    }
    HIP_TRY(hipMemcpyAsync(E->flt_x, E->flt_xs, n * sizeof(double), hipMemcpyDeviceToDevice, E->stream));
    HIP_TRY(hipMemcpyAsync(E->flt_y, E->flt_ys, n * sizeof(double), hipMemcpyDeviceToDevice, E->stream));
    HIP_TRY(hipMemcpyAsync(E->flt_layer, layer, n * sizeof(int32_t), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipMemsetAsync(E->flt_rej, 0, n * sizeof(int32_t), E->stream));
    HIP_TRY(hipMemsetAsync(E->flt_k1x, 0, n * sizeof(double), E->stream));
    HIP_TRY(hipMemsetAsync(E->flt_k1y, 0, n * sizeof(double), E->stream));
    E->flt_rec_tstp.clear();
    HIP_TRY(hipStreamSynchronize(E->stream));
    E->flt_ready = true;
    return 0;
}

int beom_download_floats(beom_handle E, double *x, double *y, int32_t *layer, int32_t *rejected, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (E->nflt < 1) { set_err(errm, errm_len, "beom_download_floats: the handle carries no float (beom_set_floats)"); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const size_t n = (size_t)E->nflt;
    if (x) HIP_TRY(hipMemcpyAsync(x, E->flt_x, n * sizeof(double), hipMemcpyDeviceToHost, E->stream));
    if (y) HIP_TRY(hipMemcpyAsync(y, E->flt_y, n * sizeof(double), hipMemcpyDeviceToHost, E->stream));
    if (layer) HIP_TRY(hipMemcpyAsync(layer, E->flt_layer, n * sizeof(int32_t), hipMemcpyDeviceToHost, E->stream));
    if (rejected) HIP_TRY(hipMemcpyAsync(rejected, E->flt_rej, n * sizeof(int32_t), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_download_float_track(beom_handle E, double *rec, int *count, int *tstp_of_record, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (E->nflt < 1 || E->flt_nrec < 1) { set_err(errm, errm_len, "beom_download_float_track: the handle has no track recorder (beom_set_floats with nrec > 0)"); return -3; }
    if (!count) { set_err(errm, errm_len, "beom_download_float_track: null count"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    const size_t held = E->flt_rec_tstp.size();
    if (held && !rec) { set_err(errm, errm_len, "beom_download_float_track: %d records held and no array to put them in", (int)held); return -1; }
    if (held) HIP_TRY(hipMemcpyAsync(rec, E->flt_rec, held * 3 * (size_t)E->nflt * sizeof(double), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    *count = (int)held;
    if (tstp_of_record) for (size_t k = 0; k < held; ++k) tstp_of_record[k] = E->flt_rec_tstp[k];
    E->flt_rec_tstp.clear();
    return 0;
}

int beom_update_floats(beom_handle E, int stage) {
    if (!E) return -1;
    if (hipSetDevice(E->device) != hipSuccess) return -9;
    if (E->nflt < 1 || !E->flt_ready || E->flt_band || (stage != 1 && stage != 2)) return -3;
    launch_floats(E, stage, nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// ---- floats on a band of rows: what beom_multi.hip builds its float calls from (include/beom_hip.h) ------------------------
int beom_band_floats_set(beom_handle E, int64_t n, int capacity, int own0, int nown, int ghost_s, int has_south, int has_north,
                         int frame_mm, int xper, int ring, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    free_floats(E);
    if (n == 0) return 0;
    if (n < 0 || capacity < 1 || !E->dense || !E->d.slab || nown < 1 || ghost_s < 0 || ghost_s + nown > E->d.M || own0 < 1 ||
        own0 + nown - 1 > frame_mm + 1) {
        set_err(errm, errm_len, "beom_band_floats_set: %lld floats, capacity %d, rows %d..%d (+%d) of %d on a window of %d rows: needs a dense band",
                (long long)n, capacity, own0, own0 + nown - 1, ghost_s, frame_mm + 1, E->d.M);
        return -3;
    }
    int rc = 0;
    E->nflt = (long long)n;
    const size_t m = (size_t)n, box = (size_t)kFloatRecordWords * ((size_t)capacity + 1);
    for (double **a : {&E->flt_x, &E->flt_y, &E->flt_k1x, &E->flt_k1y, &E->flt_xs, &E->flt_ys})
        if ((rc = alloc_plain(E, E->flt_allocs, a, m, errm, errm_len))) { free_floats(E); return rc; }
    for (int32_t **a : {&E->flt_layer, &E->flt_rej})
        if ((rc = alloc_plain(E, E->flt_allocs, a, m, errm, errm_len))) { free_floats(E); return rc; }
    if ((rc = alloc_plain(E, E->flt_allocs, &E->flt_first_dry, 1, errm, errm_len))) { free_floats(E); return rc; }
    FloatBand fb{};
    fb.own0 = own0; fb.nown = nown; fb.gs = ghost_s; fb.Mf = frame_mm + 1; fb.nring = ring ? frame_mm : 0; fb.capacity = capacity;
    fb.lo = (ring || has_south) ? std::max(1, ghost_s + 1 - kFloatReach) : 1;
    fb.hi = (ring || has_north) ? std::min(E->d.M - 1, ghost_s + nown + kFloatReach) : E->d.M;
    if ((rc = alloc_plain(E, E->flt_allocs, &fb.stats, 4, errm, errm_len))) { free_floats(E); return rc; }
    if (has_south && ((rc = alloc_plain(E, E->flt_allocs, &fb.box_s, box, errm, errm_len)) ||
                      (rc = alloc_plain(E, E->flt_allocs, &E->flt_in_s, box, errm, errm_len)))) { free_floats(E); return rc; }
    if (has_north && ((rc = alloc_plain(E, E->flt_allocs, &fb.box_n, box, errm, errm_len)) ||
                      (rc = alloc_plain(E, E->flt_allocs, &E->flt_in_n, box, errm, errm_len)))) { free_floats(E); return rc; }
    E->flt_fb = fb; E->flt_band = true;
    E->flt_xper = xper != 0; E->flt_yper = ring != 0; E->flt_fmm = (double)frame_mm;
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

// the candidates go to the scratch of stage 1; *first_dry = the smallest index of a float of this band's rows that does not
// start in a wet cell (~0 = none).  Nothing the handle holds is replaced until beom_band_floats_commit.
int beom_band_floats_check(beom_handle E, const double *x, const double *y, unsigned long long *first_dry, char *errm, int errm_len) {
    if (!E || !x || !y || !first_dry) { set_err(errm, errm_len, "beom_band_floats_check: null argument"); return -1; }
    if (!E->flt_band) { set_err(errm, errm_len, "beom_band_floats_check: the handle carries no band floats (beom_band_floats_set)"); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const size_t n = (size_t)E->nflt;
    const unsigned long long none = ~0ull;
    HIP_TRY(hipMemcpyAsync(E->flt_xs, x, n * sizeof(double), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipMemcpyAsync(E->flt_ys, y, n * sizeof(double), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipMemcpyAsync(E->flt_first_dry, &none, sizeof(none), hipMemcpyHostToDevice, E->stream));
    FloatView f = float_view(E, nullptr);
    f.fmm = E->flt_fmm; f.xper = E->flt_xper; f.yper = E->flt_yper; f.cellmap = nullptr;
    const dim3 g((unsigned)((E->nflt + BEOM_BLOCK - 1) / BEOM_BLOCK)), b(BEOM_BLOCK);
    hipLaunchKernelGGL(k_floats_check_band, g, b, 0, E->stream, E->d, f, E->flt_fb, E->flt_first_dry);
    HIP_TRY(hipMemcpyAsync(first_dry, E->flt_first_dry, sizeof(none), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_band_floats_commit(beom_handle E, const int32_t *layer, char *errm, int errm_len) {
    if (!E || !layer) { set_err(errm, errm_len, "beom_band_floats_commit: null argument"); return -1; }
    if (!E->flt_band) { set_err(errm, errm_len, "beom_band_floats_commit: the handle carries no band floats"); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const size_t n = (size_t)E->nflt, box = sizeof(unsigned long long) * kFloatRecordWords;
    HIP_TRY(hipMemcpyAsync(E->flt_x, E->flt_xs, n * sizeof(double), hipMemcpyDeviceToDevice, E->stream));
    HIP_TRY(hipMemcpyAsync(E->flt_y, E->flt_ys, n * sizeof(double), hipMemcpyDeviceToDevice, E->stream));
    HIP_TRY(hipMemcpyAsync(E->flt_layer, layer, n * sizeof(int32_t), hipMemcpyHostToDevice, E->stream));
    HIP_TRY(hipMemsetAsync(E->flt_rej, 0, n * sizeof(int32_t), E->stream));
    HIP_TRY(hipMemsetAsync(E->flt_k1x, 0, n * sizeof(double), E->stream));
    HIP_TRY(hipMemsetAsync(E->flt_k1y, 0, n * sizeof(double), E->stream));
    HIP_TRY(hipMemsetAsync(E->flt_fb.stats, 0, 4 * sizeof(unsigned long long), E->stream));
    for (unsigned long long *q : {E->flt_fb.box_s, E->flt_fb.box_n, E->flt_in_s, E->flt_in_n})
        if (q) HIP_TRY(hipMemsetAsync(q, 0, box, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    E->flt_ready = true;
    return 0;
}

int beom_band_floats_launch(beom_handle E, int mode) {
    if (!E) return -1;
    if (hipSetDevice(E->device) != hipSuccess) return -9;
    if (!E->flt_band || !E->flt_ready || mode < 1 || mode > 3) return -3;
    launch_floats(E, mode, nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int beom_band_floats_boxes(beom_handle E, void **out_s, void **out_n, void **in_s, void **in_n, size_t *bytes) {
    if (!E || !E->flt_band) return -3;
    if (out_s) *out_s = E->flt_fb.box_s;
    if (out_n) *out_n = E->flt_fb.box_n;
    if (in_s) *in_s = E->flt_in_s;
    if (in_n) *in_n = E->flt_in_n;
    if (bytes) *bytes = sizeof(unsigned long long) * kFloatRecordWords * ((size_t)E->flt_fb.capacity + 1);
    return 0;
}

int beom_band_floats_ingest(beom_handle E) {
    if (!E) return -1;
    if (hipSetDevice(E->device) != hipSuccess) return -9;
    if (!E->flt_band || !E->flt_ready) return -3;
    FloatView f = float_view(E, nullptr);
    const dim3 g((unsigned)((E->flt_fb.capacity + BEOM_BLOCK - 1) / BEOM_BLOCK), 2u), b(BEOM_BLOCK);
    hipLaunchKernelGGL(k_floats_ingest, g, b, 0, E->stream, f, E->flt_fb, E->flt_in_s, E->flt_in_n);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int beom_band_floats_download(beom_handle E, double *x, double *y, int32_t *layer, int32_t *rejected, unsigned long long *stats3,
                              char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (!E->flt_band) { set_err(errm, errm_len, "beom_band_floats_download: the handle carries no band floats"); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const size_t n = (size_t)E->nflt;
    unsigned long long st[3] = {0, 0, 0};
    if (x) HIP_TRY(hipMemcpyAsync(x, E->flt_x, n * sizeof(double), hipMemcpyDeviceToHost, E->stream));
    if (y) HIP_TRY(hipMemcpyAsync(y, E->flt_y, n * sizeof(double), hipMemcpyDeviceToHost, E->stream));
    if (layer) HIP_TRY(hipMemcpyAsync(layer, E->flt_layer, n * sizeof(int32_t), hipMemcpyDeviceToHost, E->stream));
    if (rejected) HIP_TRY(hipMemcpyAsync(rejected, E->flt_rej, n * sizeof(int32_t), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipMemcpyAsync(st, E->flt_fb.stats, sizeof(st), hipMemcpyDeviceToHost, E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    E->flt_handovers = (long long)st[2];
    if (stats3) for (int q = 0; q < 3; ++q) stats3[q] = st[q];
    return 0;
}

// ---- the time accumulators: moments (beom_moments.h) and tracer moments (beom_tracer_moments.h) ----------------------------
static void accum_free(Accum &A) {
    free_list(A.allocs);
    A.level = 0; A.stride = 1; A.count = 0; A.first = A.last = 0;
    for (int f = 0; f < 5; ++f) A.ref[f] = A.sum[f] = A.sq[f] = nullptr;
}

// level 0 frees; else zeroed arrays for the level's quantities.  A failed allocation frees them all and leaves level 0
static int accum_set(beom_engine *E, Accum beom_engine::*which, int level, int stride, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    Accum &A = E->*which;
    const AccumKind &K = *A.kind;
    if (level < 0 || level > 3 || stride < 1) { set_err(errm, errm_len, K.bad_args, level, stride); return -3; }
    if (K.no_tracer && level > 0 && E->ntrc < 1) { set_err(errm, errm_len, "%s", K.no_tracer); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    accum_free(A);
    if (level == 0) return 0;
    int rc = 0;
    const size_t n = K.per_tracer ? tracer_cells(E) : state_cells(E);
    const int nq = level >= 2 ? K.n2 : K.n1;
    for (int f = 0; f < nq && !rc; ++f) {
        rc = alloc_aligned(E, A.allocs, &A.ref[f], n, errm, errm_len);
        if (!rc) rc = alloc_aligned(E, A.allocs, &A.sum[f], n, errm, errm_len);
    }
    for (int m = 0; m < K.nsq && !rc && level >= 3; ++m) rc = alloc_aligned(E, A.allocs, &A.sq[m], n, errm, errm_len);
    if (rc) { accum_free(A); return rc; }
    A.level = level; A.stride = stride;
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

static int accum_reset(Accum &A) {
    if (A.level < 1) return -3;
    A.count = 0; A.first = A.last = 0;
    return 0;
}

// ref, sum [quantities][rows][0:ndeg] and sq [second moments][rows][0:ndeg] of the caller (null: not wanted)
static int accum_download(beom_engine *E, Accum beom_engine::*which, double *ref, double *sum, double *sq, long long *count,
                          int *tstp_first, int *tstp_last, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    const Accum &A = E->*which;
    if (A.level < 1) { set_err(errm, errm_len, "%s", A.kind->none); return -3; }
    if (sq && A.level < 3) { set_err(errm, errm_len, A.kind->no_sq, A.level); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const size_t rows = (size_t)(A.kind->per_tracer ? E->ntrc : 1) * (size_t)E->d.nlay, slab = ((size_t)E->d.ndeg + 1) * rows;
    const int nq = A.level >= 2 ? A.kind->n2 : A.kind->n1, nsq = A.kind->nsq;
    if (count) *count = A.count;
    if (tstp_first) *tstp_first = A.first;
    if (tstp_last) *tstp_last = A.last;
    if (A.count == 0) {                // nothing sampled yet: the arrays hold whatever an earlier average left
        if (ref) std::fill(ref, ref + nq * slab, 0.0);
        if (sum) std::fill(sum, sum + nq * slab, 0.0);
        if (sq) std::fill(sq, sq + nsq * slab, 0.0);
        return 0;
    }
    int rc;
    for (int f = 0; f < nq; ++f) {
        if (ref && (rc = copy_out(E, ref + f * slab, A.ref[f], rows, errm, errm_len))) return rc;
        if (sum && (rc = copy_out(E, sum + f * slab, A.sum[f], rows, errm, errm_len))) return rc;
    }
    for (int m = 0; m < nsq && sq; ++m)
        if ((rc = copy_out(E, sq + m * slab, A.sq[m], rows, errm, errm_len))) return rc;
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_set_moments(beom_handle E, int level, int stride, char *errm, int errm_len) {
    return accum_set(E, &beom_engine::mom, level, stride, errm, errm_len);
}
int beom_set_tracer_moments(beom_handle E, int level, int stride, char *errm, int errm_len) {
    return accum_set(E, &beom_engine::tmom, level, stride, errm, errm_len);
}

int beom_reset_moments(beom_handle E) { return E ? accum_reset(E->mom) : -1; }
int beom_reset_tracer_moments(beom_handle E) { return E ? accum_reset(E->tmom) : -1; }

static int accum_sample(beom_engine *E, Accum beom_engine::*which, void (*launch)(beom_engine *, int)) {
    if (!E) return -1;
    const Accum &A = E->*which;
    if (A.level < 1 || (A.kind->per_tracer && E->ntrc < 1)) return -3;
    if (hipSetDevice(E->device) != hipSuccess) return -9;
    launch(E, E->last_tstp);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}
int beom_sample_moments(beom_handle E) { return accum_sample(E, &beom_engine::mom, launch_moments); }
int beom_sample_tracer_moments(beom_handle E) { return accum_sample(E, &beom_engine::tmom, launch_tracer_moments); }

int beom_download_moments(beom_handle E, double *ref, double *sum, double *sq, long long *count, int *tstp_first, int *tstp_last,
                          char *errm, int errm_len) {
    return accum_download(E, &beom_engine::mom, ref, sum, sq, count, tstp_first, tstp_last, errm, errm_len);
}
int beom_download_tracer_moments(beom_handle E, double *ref, double *sum, double *sq, long long *count, int *tstp_first, int *tstp_last,
                                 char *errm, int errm_len) {
    return accum_download(E, &beom_engine::tmom, ref, sum, sq, count, tstp_first, tstp_last, errm, errm_len);
}

// ---- harmonics (beom_harmonics.h): the accumulator's host side, with the frequencies and the normal matrix ----
int beom_harmonic_weights(double omega, double ctim, double *cw, double *sw) {
    if (!cw || !sw) return -3;
    const double th = omega * ctim;
    *cw = cos(th);
    *sw = sin(th);
    return 0;
}

static void harmonics_free(Harmonics &H) {
    accum_free(H.acc);
    const long long launches = H.acc.launches;      // (all calls so far: kept, as accum_free keeps it)
    H = Harmonics{};
    H.acc.launches = launches;
}

int beom_set_harmonics(beom_handle E, int nfreq, const double *omega, int level, int stride, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    if (nfreq != 0) {
        if (nfreq < 1 || nfreq > BEOM_MAX_HARMONICS || level < 1 || level > 2 || stride < 1 || !omega) {
            set_err(errm, errm_len, "beom_set_harmonics: nfreq %d, level %d, stride %d (nfreq 0..%d with omega given, level 1..2, stride >= 1)",
                    nfreq, level, stride, BEOM_MAX_HARMONICS);
            return -3;
        }
        for (int k = 0; k < nfreq; ++k) {
            if (!std::isfinite(omega[k]) || !(omega[k] > 0.0)) {
                set_err(errm, errm_len, "beom_set_harmonics: omega[%d] = %g rad/day (finite and > 0)", k, omega[k]);
                return -3;
            }
            for (int j = 0; j < k; ++j)
                if (omega[j] == omega[k]) { set_err(errm, errm_len, "beom_set_harmonics: omega[%d] == omega[%d] = %g (the normal matrix would be singular)", j, k, omega[k]); return -3; }
        }
    }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    Harmonics &H = E->harm;
    harmonics_free(H);
    if (nfreq == 0) return 0;
    int rc = 0;
    const size_t n = state_cells(E);
    const int nf = level >= 2 ? 5 : 3;
    for (int f = 0; f < nf && !rc; ++f) {
        rc = alloc_aligned(E, H.acc.allocs, &H.acc.ref[f], n, errm, errm_len);
        for (int m = 0; m < 1 + 2 * nfreq && !rc; ++m) rc = alloc_aligned(E, H.acc.allocs, &H.sum[f][m], n, errm, errm_len);
    }
    if (rc) { harmonics_free(H); return rc; }
    H.acc.level = level; H.acc.stride = stride; H.nfreq = nfreq;
    std::copy(omega, omega + nfreq, H.omega);
    HIP_TRY(hipStreamSynchronize(E->stream));
    return 0;
}

int beom_reset_harmonics(beom_handle E) {
    if (!E) return -1;
    const int rc = accum_reset(E->harm.acc);
    if (!rc) std::fill(std::begin(E->harm.gram), std::end(E->harm.gram), 0.0);
    return rc;
}

int beom_sample_harmonics(beom_handle E, double ctim) {
    if (!E) return -1;
    if (E->harm.acc.level < 1) return -3;
    if (hipSetDevice(E->device) != hipSuccess) return -9;
    launch_harmonics(E, E->last_tstp, ctim);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// ref [fields][nlay][0:ndeg], sum [fields][1+2K][nlay][0:ndeg], gram [(1+2K)^2], omega [K] of the caller (null: not wanted)
int beom_download_harmonics(beom_handle E, double *ref, double *sum, double *gram, double *omega, long long *count,
                            int *tstp_first, int *tstp_last, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    const Harmonics &H = E->harm;
    const Accum &A = H.acc;
    if (A.level < 1) { set_err(errm, errm_len, "beom_download_harmonics: the handle keeps no harmonics (beom_set_harmonics)"); return -3; }
    HIP_TRY(hipSetDevice(E->device));
    const size_t rows = (size_t)E->d.nlay, slab = ((size_t)E->d.ndeg + 1) * rows;
    const int nf = A.level >= 2 ? 5 : 3, nw = 1 + 2 * H.nfreq;
    if (count) *count = A.count;
    if (tstp_first) *tstp_first = A.first;
    if (tstp_last) *tstp_last = A.last;
    if (gram) std::copy(H.gram, H.gram + nw * nw, gram);
    if (omega) std::copy(H.omega, H.omega + H.nfreq, omega);
    if (A.count == 0) {                // nothing sampled yet: the arrays hold whatever an earlier analysis left
        if (ref) std::fill(ref, ref + nf * slab, 0.0);
        if (sum) std::fill(sum, sum + (size_t)nf * nw * slab, 0.0);
        return 0;
    }
    int rc;
    for (int f = 0; f < nf; ++f) {
        if (ref && (rc = copy_out(E, ref + f * slab, A.ref[f], rows, errm, errm_len))) return rc;
        for (int m = 0; m < nw && sum; ++m)
            if ((rc = copy_out(E, sum + ((size_t)f * nw + m) * slab, H.sum[f][m], rows, errm, errm_len))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

// Replaces index_boundary_points' product (private_mod.f95:1060-1240): the table segm(nseg, 18)
// of nudged open-boundary segments, Fortran storage.  Activates no_gradient_obc after the
// momentum sweeps of every step when flag_nudging and mcbc < 0.5 (:2201-2204, 2285-2288).
// ---- forcing in time (beom_forcing.h) ----
int beom_forcing_weight(int nfr, const double *times, double period, double ctim, int *k0, int *k1, double *a) {
    if (nfr < 1 || !times || !k0 || !k1 || !a) return -1;
    beom_forcing::forcing_weight(nfr, times, period, ctim, k0, k1, a);
    return 0;
}

static void forcing_free(ForcingSet &S) {
    free_list(S.allocs);
    S = ForcingSet{};
}

int beom_set_forcing(beom_handle E, int field, int nfr, const double *times, double period, const double *frames,
                     char *errm, int errm_len) {
    char msg[256] = {0};
    // (field, times and period are looked at before the handle; the frames' values need its sizes)
    if (beom_forcing::check_set("beom_set_forcing", field, nfr, times, period, frames, 0, msg, sizeof msg)) {
        set_err(errm, errm_len, "%s", msg);
        return -3;
    }
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    DevView &d = E->d;
    const size_t n1h = (size_t)d.ndeg + 1, nl = (size_t)d.nlay;
    const size_t outer = field == BEOM_FORCING_TAUS ? 2 : nl, count = outer * n1h;
    if (beom_forcing::check_set("beom_set_forcing", field, nfr, times, period, frames, count, msg, sizeof msg)) {
        set_err(errm, errm_len, "%s", msg);
        return -3;
    }
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    const int f = field - 1;
    const bool had_wind = E->wind;
    ForcingSet &S = E->frc[f];
    forcing_free(S);
    // back to what beom_create gave; a new set then takes its place
    if (f == 0) { d.taus = E->taus0; d.taus_cells = E->taus_cells0; }
    else d.hdot = E->hdot0;
    int rc = 0;
    if (nfr > 0) {
        const size_t n = outer * (size_t)d.n1;
        rc = alloc_aligned(E, S.allocs, &S.x, n, errm, errm_len);
        if (!rc && f == 0) rc = alloc_aligned(E, S.allocs, &S.xc, n, errm, errm_len);
        S.frames.assign((size_t)nfr, nullptr);
        std::vector<double> img(n1h);
        for (int k = 0; k < nfr && !rc; ++k) {
            rc = alloc_aligned(E, S.allocs, &S.frames[(size_t)k], n, errm, errm_len);
            for (size_t o = 0; o < outer && !rc; ++o) {
                const double *src = frames + ((size_t)k * outer + o) * n1h;
                double *dst = S.frames[(size_t)k] + o * (size_t)d.n1;
                if (f == 0) {
                    // the wind stress as the cells-only copy wants it: +0 in every slot that is no cell; the sentinel's own
                    // value goes to slot 0 alone, which the launch writes to d.taus only
                    std::memcpy(img.data(), src, n1h * sizeof(double));
                    img[0] = 0.0;
                    rc = slice_to_device<double>(E, dst, img.data(), 1, 1, 0, errm, errm_len);
                    if (!rc) HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double), hipMemcpyHostToDevice, E->stream));
                } else {
                    rc = slice_to_device<double>(E, dst, src, 1, 1, 0, errm, errm_len);
                }
                if (!rc) HIP_TRY(hipStreamSynchronize(E->stream));      // (img and the staging image are used again)
            }
        }
        if (rc) forcing_free(S);
    }
    if (S.x) {
        S.nfr = nfr; S.period = period; S.times.assign(times, times + nfr);
        if (f == 0) { d.taus = S.x; d.taus_cells = S.xc; }
        else d.hdot = S.x;
        launch_forcing(E, f, 0, 0, 0.0);           // the buffers are defined from here on: the first frame
    }
    // the flags of the frames in force, or of the arrays of beom_create
    const ForcingSet &T = E->frc[0], &H = E->frc[1];
    const bool wind = T.nfr ? (f == 0 ? any_wind(frames, (size_t)nfr * count) : E->wind) : E->wind0;
    const bool has_hdot = H.nfr ? (f == 1 ? any_nonzero(frames, (size_t)nfr * count) : d.has_hdot != 0) : E->has_hdot0;
    derive_forcing_flags(E, wind, has_hdot);
    // a wind that is gone leaves nothing behind in tt3d (distribute_stress would never have written it)
    if (had_wind && !E->wind && !E->up_tt) HIP_TRY(hipMemsetAsync(d.tt3d, 0, 2 * nl * (size_t)d.n1 * sizeof(double), E->stream));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipGetLastError());
    return rc;
}

int beom_apply_forcing(beom_handle E, double ctim, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    apply_forcing(E, ctim);
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_download_forcing(beom_handle E, double *taus, double *hdot, char *errm, int errm_len) {
    if (!E) { set_err(errm, errm_len, "null handle"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    int rc;
    if ((rc = copy_out(E, taus, E->d.taus, 2, errm, errm_len))) return rc;
    if ((rc = copy_out(E, hdot, E->d.hdot, (size_t)E->d.nlay, errm, errm_len))) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int beom_set_open_boundaries(beom_handle E, int nseg, const int32_t *segm, char *errm, int errm_len) {
    if (!E || nseg < 0 || (nseg > 0 && !segm)) { set_err(errm, errm_len, "beom_set_open_boundaries: bad arguments"); return -1; }
    HIP_TRY(hipSetDevice(E->device));
    if (nseg == 0) {                    // (a band of a frame whose segments all lie in other bands)
        E->d.segm = nullptr; E->d.nseg = 0; E->obc = false; E->obc_set = true;
        return 0;
    }
    auto S = [&](int is, int col) { return segm[(size_t)is + (size_t)nseg * (col - 1)]; };
    // The reference loops are serial.  A parallel pass is equivalent iff nothing it writes is read
    // or written by another segment of the same pass: check (component, cell) sets.
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<long long> wr, rd;
        for (int is = 0; is < nseg; ++is) {
            const bool ns = S(is, 5) == 1, ew = S(is, 4) == 1;
            const int comp = pass == 0 ? (ns ? 0 : (ew ? 1 : -1)) : (ns ? 1 : (ew ? 0 : -1));
            if (comp < 0) continue;
            const int ip = pass == 0 ? S(is, 10) : S(is, 1), in = pass == 0 ? S(is, 16) : S(is, 13);
            if (ip == -1) continue;      // (this pass of the segment belongs to another band: beom_multi_set_open_boundaries)
            if (ip < 1 || ip > E->d.ndeg || in < 0 || in > E->d.ndeg) { set_err(errm, errm_len, "beom_set_open_boundaries: index out of range"); return -3; }
            wr.push_back(2ll * ip + comp);
            rd.push_back(2ll * in + comp);
        }
        std::vector<long long> w2 = wr;
        std::sort(w2.begin(), w2.end());
        if (std::adjacent_find(w2.begin(), w2.end()) != w2.end()) { set_err(errm, errm_len, "beom_set_open_boundaries: two segments update the same point (serial order would matter)"); return -7; }
        for (long long r : rd)
            if (std::binary_search(w2.begin(), w2.end(), r)) { set_err(errm, errm_len, "beom_set_open_boundaries: a segment reads a point another segment updates in the same pass (serial order would matter)"); return -7; }
    }
    // columns 1, 7, 10, 13, 16 are cell indices: to the device pitch
    std::vector<int32_t> sg(segm, segm + (size_t)nseg * 18);
    if (E->embedded) {                   // frames with land on the rectangle: packed index -> slot
        for (int col : {1, 7, 10, 13, 16})
            for (int is = 0; is < nseg; ++is) {
                int32_t &q = sg[(size_t)is + (size_t)nseg * (col - 1)];
                if (q > 0) { if ((size_t)q >= E->dev_index.size()) { set_err(errm, errm_len, "beom_set_open_boundaries: index out of range"); return -3; } q = E->dev_index[(size_t)q]; }
            }
    } else if (E->d.P)
        for (int col : {1, 7, 10, 13, 16})
            for (int is = 0; is < nseg; ++is) {
                int32_t &q = sg[(size_t)is + (size_t)nseg * (col - 1)];
                if (q > 0) q = (int32_t)(1 + (long long)((q - 1) / E->d.L) * E->d.P + (q - 1) % E->d.L);
            }
    int32_t *dev = nullptr;
    HIP_TRY(hipMalloc((void **)&dev, (size_t)nseg * 18 * sizeof(int32_t)));
    E->allocs.push_back(dev);
    HIP_TRY(hipMemcpy(dev, sg.data(), (size_t)nseg * 18 * sizeof(int32_t), hipMemcpyHostToDevice));
    E->d.segm = dev;
    E->d.nseg = nseg;
    E->obc = E->P.flag_nudging && E->P.mcbc < 0.5;
    E->obc_set = true;
    return 0;
}

int beom_info(beom_handle E, const char *what) {
    if (!E || !what) return -1;
    if (!strcmp(what, "stress_folded")) return E->last_folded ? 1 : 0;
    if (!strcmp(what, "tile_rows")) return E->dense ? (E->tile4 ? 4 : 8) : 0;
    if (!strcmp(what, "biharm_tiled")) return biharm_tiled(E) ? 1 : 0;
    if (!strcmp(what, "uv_fused")) return E->last_uv_fused ? 1 : 0;
    if (!strcmp(what, "mont_history")) return E->last_mont_hist ? 1 : 0;
    if (!strcmp(what, "plain_sweeps")) return E->last_plain;
    if (!strcmp(what, "vel_targets_zero")) return E->d.vel_targets_zero;
    if (!strcmp(what, "tracers")) return E->ntrc;
    if (!strcmp(what, "tracer_scheme")) return E->trc_scheme;
    if (!strcmp(what, "tracer_mixing")) return E->trc_mix ? 1 : 0;
    if (!strcmp(what, "tracer_mix_launches")) return (int)std::min<long long>(E->trc_mix_launches, 2000000000ll);      // all calls so far
    if (!strcmp(what, "tracer_vmixing")) return E->trc_vmix ? 1 : 0;
    if (!strcmp(what, "tracer_vmix_launches")) return (int)std::min<long long>(E->trc_vmix_launches, 2000000000ll);      // all calls so far
    if (!strcmp(what, "floats")) return (int)std::min<long long>(E->nflt, 2000000000ll);
    if (!strcmp(what, "float_records")) return (int)E->flt_rec_tstp.size();
    if (!strcmp(what, "float_launches")) return (int)std::min<long long>(E->flt_launches, 2000000000ll);      // all calls so far
    if (!strcmp(what, "float_handovers")) return (int)std::min<long long>(E->flt_handovers, 2000000000ll);   // (bands; as of the latest download)
    if (!strcmp(what, "tracer_moments")) return E->tmom.level;
    if (!strcmp(what, "tracer_moment_samples")) return (int)std::min<long long>(E->tmom.count, 2000000000ll);
    if (!strcmp(what, "tracer_moment_launches")) return (int)std::min<long long>(E->tmom.launches, 2000000000ll);     // all calls so far
    if (!strcmp(what, "tracer_series")) return E->tser.level;
    if (!strcmp(what, "tracer_series_records")) return (int)E->tser.tstp.size();
    if (!strcmp(what, "tracer_column_series")) return E->tcser.level;
    if (!strcmp(what, "tracer_column_series_records")) return (int)E->tcser.tstp.size();
    if (!strcmp(what, "column_series")) return E->cser.level;
    if (!strcmp(what, "column_series_records")) return (int)E->cser.tstp.size();
    if (!strcmp(what, "maps")) return E->maps.level;
    if (!strcmp(what, "maps_block")) return E->maps.level > 0 ? 1 << E->maps_logb : 0;
    if (!strcmp(what, "maps_records")) return (int)E->maps.tstp.size();
    if (!strcmp(what, "map_launches")) return (int)std::min<long long>(E->map_launches, 2000000000ll);      // all calls so far
    if (!strcmp(what, "series")) return E->ser.level;
    if (!strcmp(what, "series_records")) return (int)E->ser.tstp.size();
    if (!strcmp(what, "harmonics")) return E->harm.nfreq;
    if (!strcmp(what, "harmonic_level")) return E->harm.acc.level;
    if (!strcmp(what, "harmonic_samples")) return (int)std::min<long long>(E->harm.acc.count, 2000000000ll);
    if (!strcmp(what, "harmonic_launches")) return (int)std::min<long long>(E->harm.acc.launches, 2000000000ll);     // all calls so far
    if (!strcmp(what, "forcing_taus_frames")) return E->frc[0].nfr;
    if (!strcmp(what, "forcing_hdot_frames")) return E->frc[1].nfr;
    if (!strcmp(what, "forcing_launches")) return (int)std::min<long long>(E->frc_launches, 2000000000ll);          // all so far
    if (!strcmp(what, "moments")) return E->mom.level;
    if (!strcmp(what, "moment_samples")) return (int)std::min<long long>(E->mom.count, 2000000000ll);
    if (!strcmp(what, "moment_launches")) return (int)std::min<long long>(E->mom.launches, 2000000000ll);     // all calls so far
    if (!strcmp(what, "lid_sweeps")) return (int)std::min<long long>(E->lid_sweeps, 2000000000ll);        // Gauss-Seidel sweeps kept, all steps so far
    if (!strcmp(what, "lid_solves")) return (int)std::min<long long>(E->lid_solves, 2000000000ll);
    if (!strcmp(what, "lid_launches")) return (int)std::min<long long>(E->lid_launches, 2000000000ll);
    if (!strcmp(what, "lid_sweep_distance")) return E->lid_dstep;
    return -3;
}

int beom_set_option(beom_handle E, const char *name, int value) {
    if (!E || !name) return -1;
    if (!strncmp(name, "fuse", 4) && hist_sync(E)) return -10;      // fuse, fuse_mont_visc, fuse_uv: the other paths read the arrays
    if (!strcmp(name, "fuse")) { E->fuse = value != 0; E->fuse_uv = value != 0; }
    else if (!strcmp(name, "fuse_mont_visc")) E->fuse = value != 0 && !E->lid;      // (a lid handle keeps the separate sweeps)
    else if (!strcmp(name, "fuse_uv")) E->fuse_uv = value != 0 && !E->lid;
    else if (!strcmp(name, "keep_diag")) E->d.keep_diag = value != 0;
    else if (!strcmp(name, "fold_stress")) E->fold_stress = value != 0;
    else if (!strcmp(name, "profile_stride")) E->profile_stride = value > 0 ? value : 1;
    else if (!strcmp(name, "profile_rotate")) E->profile_rotate = value != 0;
    else if (!strcmp(name, "lean_d2h")) E->lean_d2h = value != 0;
    else if (!strcmp(name, "lean_visc")) E->lean_visc = value != 0;
    else if (!strcmp(name, "mont_history")) E->mont_history = value != 0;
    else if (!strcmp(name, "plain_sweeps")) E->plain_sweeps = value != 0;
    else if (!strcmp(name, "moments_by_caller")) E->mom_by_caller = value != 0;
    else if (!strcmp(name, "column_series_batch")) E->cser_batch_opt = value > 0 ? value : 0;      // (looked at by the next beom_set_column_series)
    else if (!strcmp(name, "tracer_column_series_batch")) E->tcser_batch_opt = value > 0 ? value : 0;      // (looked at by the next beom_set_tracer_column_series)
    else if (!strcmp(name, "tracer_series_batch")) E->tser_batch_opt = value > 0 ? value : 0;      // (looked at by the next beom_set_tracer_series)
    else return -3;
    return 0;
}

int beom_set_stream(beom_handle E, void *hip_stream, int use_own) {
    if (!E) return -1;
    // hip_stream == NULL is a valid stream (the legacy default stream torch uses by default)
    E->stream = use_own ? E->own_stream : (hipStream_t)hip_stream;
    return 0;
}

int beom_is_dense(beom_handle E) { return (E && E->dense) ? (E->embedded ? 2 : 1) : 0; }

int beom_device_field(beom_handle E, const char *name, void **dptr, int64_t *stride_layer,
                      int64_t *stride_row, int64_t *row0_offset) {
    if (!E || !name || !dptr) return -1;
    const DevView &d = E->d;
    double *p = nullptr;
    if (!strcmp(name, "hlay")) p = d.hlay;
    else if (!strcmp(name, "u")) p = d.u;
    else if (!strcmp(name, "v")) p = d.v;
    else if (!strcmp(name, "h_u")) p = d.h_u;
    else if (!strcmp(name, "h_v")) p = d.h_v;
    else return -3;
    *dptr = p;
    if (stride_layer) *stride_layer = d.n1;
    if (stride_row) *stride_row = d.P ? d.P : (E->dense ? d.L : 0);
    if (row0_offset) *row0_offset = 1;
    return 0;
}

}  // extern "C"

// ---- column series (beom_column_series.h): defined last, so that its kernels are instantiated behind every other one ------
// The column series' block partials of a launch stay under the tracer series' bound: a record is taken in batches of 64-column
// chunks (never fewer than one); columns are independent, so the batches cannot change a bit.
static int column_series_scratch(beom_engine *E, Recorder &R, int cnt, int ncols, char *errm, int errm_len) {
    const size_t nch = (size_t)(ncols + 63) / 64, per_chunk = (size_t)((E->d.M + kColBlockRows - 1) / kColBlockRows) * cnt * 64;
    size_t batch = E->cser_batch_opt > 0 ? (size_t)E->cser_batch_opt : kTracerSeriesScratch / (per_chunk * sizeof(double));
    batch = std::min<size_t>(std::max<size_t>(batch, 1), nch);
    R.batch = (int)batch;
    if (const int rc = ensure_cellmap(E, errm, errm_len)) return rc;
    return alloc_plain(E, R.allocs, &R.part, batch * per_chunk, errm, errm_len, false);
}
// one record of the column series (beom_column_series.h) of the fields as they stand into the next free slot, under step tstp:
// `batch` chunks of columns per launch, every column finished on its own
static void launch_column_series(beom_engine *E, int tstp) {
    const DevView &d = E->d;
    Recorder &R = E->cser;
    const int cnt = beom_series_count(d.nlay, R.level), nch = (d.L + 63) / 64;
    const int M2 = pow2_ceil(d.M), nblk = (d.M + kColBlockRows - 1) / kColBlockRows, nblkp2 = std::max(1, M2 / kColBlockRows);
    double *rec = R.rec + R.tstp.size() * (size_t)R.rows * cnt;
    const int32_t *map = E->dense ? nullptr : E->integ_cellmap;
    const int colpad = R.batch * 64;
    for (int c0 = 0; c0 < nch; c0 += R.batch) {
        const int nc = std::min(R.batch, nch - c0), ncols = std::min(nc * 64, d.L - c0 * 64);
        pick_int<1, 2>(R.level, [&](auto lv) {
            pick([&](auto dense) {
                hipLaunchKernelGGL((k_column_blocks<dense, lv>), dim3((unsigned)nc, (unsigned)nblk), dim3(BEOM_BLOCK), 0, E->stream, d, c0,
                                   R.wlo, R.whi, M2, E->integ_xper, E->integ_yper, map, R.part, colpad);
            }, E->dense);
        });
        hipLaunchKernelGGL(k_column_finish<kColFinishLevels>, dim3((unsigned)((ncols + BEOM_BLOCK - 1) / BEOM_BLOCK), (unsigned)cnt), dim3(BEOM_BLOCK), 0, E->stream,
                           (const double *)R.part, rec + (size_t)c0 * 64 * cnt, cnt, colpad, ncols, nblk, nblkp2);
    }
    R.tstp.push_back(tstp);
}

// ---- tracer column series (beom_tracer_column_series.h): behind the column series', for the same reason ------------------
// The block partials of a launch stay under the tracer series' bound, in a scratch of its own: a record is taken in batches of
// 64-column chunks (never fewer than one); columns are independent, so the batches cannot change a bit.
static int tracer_column_series_scratch(beom_engine *E, Recorder &R, int cnt, int ncols, char *errm, int errm_len) {
    const size_t nch = (size_t)(ncols + 63) / 64, per_chunk = (size_t)((E->d.M + kColBlockRows - 1) / kColBlockRows) * cnt * 64;
    size_t batch = E->tcser_batch_opt > 0 ? (size_t)E->tcser_batch_opt : kTracerSeriesScratch / (per_chunk * sizeof(double));
    batch = std::min<size_t>(std::max<size_t>(batch, 1), nch);
    R.batch = (int)batch;
    if (const int rc = ensure_cellmap(E, errm, errm_len)) return rc;
    return alloc_plain(E, R.allocs, &R.part, batch * per_chunk, errm, errm_len, false);
}
// one record of the tracer column series of q, hlay, h_u, h_v as they stand into the next free slot, under step tstp: `batch`
// chunks of columns per launch, every column finished on its own
static void launch_tracer_column_series(beom_engine *E, int tstp) {
    const DevView &d = E->d;
    Recorder &R = E->tcser;
    const int nq = 2 * R.level, cnt = beom_tracer_series_count(E->ntrc, d.nlay, R.level), nch = (d.L + 63) / 64;
    const int M2 = pow2_ceil(d.M), nblk = (d.M + kColBlockRows - 1) / kColBlockRows, nblkp2 = std::max(1, M2 / kColBlockRows);
    double *rec = R.rec + R.tstp.size() * (size_t)R.rows * cnt;
    const int32_t *map = E->dense ? nullptr : E->integ_cellmap;
    const int colpad = R.batch * 64;
    for (int c0 = 0; c0 < nch; c0 += R.batch) {
        const int nc = std::min(R.batch, nch - c0), ncols = std::min(nc * 64, d.L - c0 * 64);
        pick_int<1, 3>(R.level, [&](auto lv) {
            pick([&](auto dense) {
                hipLaunchKernelGGL((k_tracer_column_blocks<dense, lv>), dim3((unsigned)nc, (unsigned)nblk), dim3(BEOM_BLOCK), 0, E->stream, d,
                                   (const double *)E->trc_q, E->ntrc, c0, R.wlo, R.whi, M2, E->integ_xper, E->integ_yper, map, R.part, colpad);
            }, E->dense);
        });
        hipLaunchKernelGGL(k_tracer_column_finish<kColFinishLevels>, dim3((unsigned)((ncols + BEOM_BLOCK - 1) / BEOM_BLOCK), (unsigned)cnt), dim3(BEOM_BLOCK), 0,
                           E->stream, (const double *)R.part, rec + (size_t)c0 * 64 * cnt, cnt, nq, colpad, ncols, nblk, nblkp2);
    }
    R.tstp.push_back(tstp);
}

// ---- maps (beom_maps.h): behind the tracer column series', for the same reason --------------------------------------------
static int maps_lines(const beom_engine *E) {
    const int B = 1 << E->maps_logb;
    return ((E->d.M + B - 1) / B) * ((E->d.L + B - 1) / B);
}
// A block is finished inside one wavefront: the maps need the cell map and the frame's wraps, and no scratch.
static int maps_scratch(beom_engine *E, Recorder &, int, int, char *errm, int errm_len) { return ensure_cellmap(E, errm, errm_len); }
// one record of the maps (beom_maps.h) of the fields as they stand into the next free slot, under step tstp: one launch
static void launch_maps(beom_engine *E, int tstp) {
    const DevView &d = E->d;
    Recorder &R = E->maps;
    const int B = 1 << E->maps_logb, Lc = (d.L + B - 1) / B, Mc = (d.M + B - 1) / B, nch = (d.L + 63) / 64;
    const int cnt = beom_maps_count(E->ntrc, d.nlay, R.level);
    double *rec = R.rec + R.tstp.size() * (size_t)R.rows * cnt;
    const int32_t *map = E->dense ? nullptr : E->integ_cellmap;
    pick_int<1, 3>(R.level, [&](auto lv) {
        pick([&](auto dense) {
            hipLaunchKernelGGL((k_map_blocks<dense, lv>), dim3((unsigned)((nch + kMapWaves - 1) / kMapWaves), (unsigned)Mc), dim3(BEOM_BLOCK), 0,
                               E->stream, d, (const double *)E->trc_q, E->ntrc, E->maps_logb, E->integ_xper, E->integ_yper, map, rec, Lc, Mc);
        }, E->dense);
    });
    ++E->map_launches;
    R.tstp.push_back(tstp);
}
