// beom_multi.hip — the j-slab decomposition of SURVEY.md §8(e) behind the C-ABI: a dense frame cut
// into bands of rows, one band per GPU, ghost rows exchanged once per time step, the exchange of
// step n overlapped with the interior rows of step n+1.  The reference has no counterpart (OpenMP
// only).  Built only from the public entry points of include/beom_hip.h.
//
//   * every band is an ordinary slab handle (beom_params.slab_row0/slab_mm) with G = 4 ghost rows per
//     neighbour; per step ONE exchange of hlay,u,v,h_u,h_v (beom_pack_rows -> transport ->
//     beom_unpack_rows on the band's second stream), beom_step_phase 1/2 around it;
//   * transports: peer copies between the bands of ONE process (hipMemcpyPeerAsync over xGMI), or RCCL
//     (grouped ncclSend/ncclRecv; librccl is loaded at run time) — either all bands in one process
//     (ncclCommInitAll) or ONE band per process (ncclCommInitRank: bench.py under torchrun);
//   * two ways in: GLOBAL arrays that the library cuts (beom_multi_create: the Fortran host), or this
//     band's WINDOW only (beom_multi_create_local: nothing of global size exists on any rank);
//   * frames periodic in y: the bands form a ring over rows 1..mm (a band of a ring is a slab deep inside
//     a taller fake frame: every mask is 1, the wrap comes from the exchange).  The orphan row mm+1
//     keeps its slot in every array and output record (private_mod.f95:642-668: its E/W neighbours are
//     cells of row 1, its S neighbours cells of row mm, nothing points to it) and is carried by a
//     companion frame on band 0's device: rows 1..6, mm-3..mm and mm+1 as ONE small y-periodic frame,
//     its first ten rows refreshed from band 0 before every step.
// The K steps of one call run inside the library: no per-step host language in the loop.
// No CPU fallback: every call needs its HIP devices.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <time.h>
#include <unistd.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <string>
#include <vector>

#include "../../include/beom_hip.h"
#include "beom_bands_host.h"
#include "beom_dense_host.h"
#include "beom_recorder.h"
#include "beom_forcing.h"

using namespace beom_bands;

namespace {

constexpr int kFields = 5;         // hlay, u, v, h_u, h_v
constexpr int kFakePad = 8;        // a ring band is presented as rows 9.. of a frame 16 rows taller

void m_err(char *errm, int len, const char *fmt, ...) {
    if (!errm || len <= 0) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(errm, (size_t)len, fmt, ap);
    va_end(ap);
}

#define M_HIP(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            m_err(errm, errm_len, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                  __FILE__, __LINE__);                                                       \
            return -100 - (int)e_;                                                           \
        }                                                                                    \
    } while (0)
#define M_RC(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

// ---- RCCL, bound at run time (one copy per process: PyTorch-ROCm ships librccl.so.1 too) --------
typedef void *nccl_comm;
struct nccl_uid { char internal[128]; };
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(nccl_uid *) = nullptr;
    int (*CommInitRank)(nccl_comm *, int, nccl_uid, int) = nullptr;
    int (*CommInitAll)(nccl_comm *, int, const int *) = nullptr;
    int (*CommDestroy)(nccl_comm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *, size_t, int, int, nccl_comm, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, nccl_comm, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int *) = nullptr;
    bool load(char *errm, int errm_len) {
        if (lib) return true;
        if (getenv("BEOM_RCCL_DISABLE")) { m_err(errm, errm_len, "RCCL switched off by BEOM_RCCL_DISABLE (rehearsal of a machine without it)"); return false; }
        const char *names[] = {getenv("BEOM_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *nm : names) {
            if (!nm || !*nm) continue;
            lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) { m_err(errm, errm_len, "RCCL transport: librccl.so.1 not found (%s)", dlerror()); return false; }
#define SYM(field, name) do { *(void **)(&field) = dlsym(lib, name); if (!field) { m_err(errm, errm_len, "RCCL transport: %s missing in librccl", name); lib = nullptr; return false; } } while (0)
        SYM(GetUniqueId, "ncclGetUniqueId"); SYM(CommInitRank, "ncclCommInitRank"); SYM(CommInitAll, "ncclCommInitAll");
        SYM(CommDestroy, "ncclCommDestroy"); SYM(GroupStart, "ncclGroupStart"); SYM(GroupEnd, "ncclGroupEnd");
        SYM(Send, "ncclSend"); SYM(Recv, "ncclRecv"); SYM(GetErrorString, "ncclGetErrorString"); SYM(GetVersion, "ncclGetVersion");
#undef SYM
        return true;
    }
};
Rccl g_rccl;
constexpr int kNcclChar = 0;       // ncclInt8 / ncclChar (rccl.h): the rows travel as bytes

#define M_NCCL(expr)                                                                         \
    do {                                                                                     \
        int e_ = (expr);                                                                     \
        if (e_ != 0) {                                                                       \
            m_err(errm, errm_len, "%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(e_), \
                  __FILE__, __LINE__);                                                       \
            return -300 - e_;                                                                \
        }                                                                                    \
    } while (0)

// ---- ghost rows staged through a POSIX shared-memory segment (BEOM_XCHG_SHM) ---------------------------
// One band per process, the processes on ONE node — several of them may share a device, which RCCL refuses
// ("duplicate GPU"): the -m gpu tests run two and three ranks of beom_multi_create_local on the one GPU of
// the box this way, through the same multi_one_step as the RCCL branch.  In stream order on a band's second
// stream, where RCCL has its grouped send/recv:
//     copy both send buffers into this band's slots of the segment -> host function: publish "exchange s is there"
//     host function: wait for the north neighbour's s -> copy its south-going slot into recv_n; the same for the south
// Slots are double-buffered by the parity of s; a band reaches exchange s + 2 only after it has seen its neighbours'
// s + 1, and a neighbour publishes s + 1 only after its step has consumed this band's s — so no slot is overwritten
// before it has been read.  A wait that lasts longer than BEOM_SHM_TIMEOUT_S (default 60) marks the handle failed
// instead of hanging the stream.
struct ShmCtl { volatile uint64_t ready; volatile uint64_t seq; char pad[112]; };      // one per band, 128 B apart
struct ShmHdr { uint64_t magic; uint64_t nb; uint64_t xbytes; uint64_t slot_stride; };
constexpr uint64_t kShmMagic = 0x42454f4d58434847ull;            // "BEOMXCHG"
constexpr size_t kShmCtl0 = 4096;

struct ShmXchg {
    std::string name;
    char *base = nullptr;
    size_t size = 0, slot_stride = 0, data0 = 0;
    int nb = 0;
    bool registered = false;
    uint64_t seq = 0;                       // exchanges issued by this band so far
    volatile int failed = 0;                // a wait timed out (set from a host function)
    double timeout_s = 60.0;
    ShmCtl *ctl(int band) const { return (ShmCtl *)(base + kShmCtl0 + (size_t)band * sizeof(ShmCtl)); }
    // what band `band` sends towards dir (0 = south, 1 = north) in exchange s
    char *slot(int band, int dir, uint64_t s) const { return base + data0 + (((size_t)band * 2 + dir) * 2 + (size_t)(s & 1)) * slot_stride; }
};

static double mono_s() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
static void nap_us(long us) { timespec ts{0, us * 1000}; nanosleep(&ts, nullptr); }

struct ShmOp { ShmXchg *x; int band; uint64_t seq; };
// host functions (hipLaunchHostFunc): no HIP call inside
static void shm_publish(void *p) {
    ShmOp *op = (ShmOp *)p;
    __atomic_store_n(&op->x->ctl(op->band)->seq, op->seq, __ATOMIC_RELEASE);
    delete op;
}
static void shm_wait(void *p) {
    ShmOp *op = (ShmOp *)p;
    const double t0 = mono_s();
    int spins = 0;
    while (__atomic_load_n(&op->x->ctl(op->band)->seq, __ATOMIC_ACQUIRE) < op->seq) {
        if (op->x->failed) break;
        if (++spins > 2000) nap_us(20);
        if ((spins & 1023) == 0 && mono_s() - t0 > op->x->timeout_s) { op->x->failed = 1; break; }
    }
    delete op;
}

static void shm_close(ShmXchg *x) {
    if (!x) return;
    if (x->base) {
        if (x->registered) (void)hipHostUnregister(x->base);
        munmap(x->base, x->size);
    }
    delete x;
}

// every band maps the segment `name` (created by whoever comes first), announces itself and waits for the others;
// band 0 then removes the name, so nothing is left in /dev/shm once the last process has gone
static int shm_open_all(ShmXchg **out, const char *name, int nb, int band, size_t xbytes, bool loopback, char *errm, int errm_len) {
    if (!name || name[0] != '/' || strlen(name) > 200) { m_err(errm, errm_len, "beom_multi: the shared-memory transport needs a segment name \"/...\" common to all ranks"); return -3; }
    ShmXchg *x = new ShmXchg();
    x->name = name; x->nb = nb;
    x->slot_stride = (xbytes + 4095) / 4096 * 4096;
    x->data0 = (kShmCtl0 + (size_t)nb * sizeof(ShmCtl) + 4095) / 4096 * 4096;
    x->size = x->data0 + (size_t)nb * 4 * x->slot_stride;
    if (const char *t = getenv("BEOM_SHM_TIMEOUT_S")) { const double v = atof(t); if (v > 0.0) x->timeout_s = v; }
    const int fd = shm_open(name, O_CREAT | O_RDWR, 0600);
    if (fd < 0) { m_err(errm, errm_len, "beom_multi: shm_open(%s) failed: %s", name, strerror(errno)); delete x; return -33; }
    if (ftruncate(fd, (off_t)x->size) != 0) { m_err(errm, errm_len, "beom_multi: ftruncate(%s, %zu) failed: %s", name, x->size, strerror(errno)); close(fd); delete x; return -33; }
    void *m = mmap(nullptr, x->size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (m == MAP_FAILED) { m_err(errm, errm_len, "beom_multi: mmap(%s) failed: %s", name, strerror(errno)); delete x; return -33; }
    x->base = (char *)m;
    ShmHdr *h = (ShmHdr *)x->base;
    if (band == 0 || loopback) { h->nb = (uint64_t)nb; h->xbytes = xbytes; h->slot_stride = x->slot_stride; __atomic_store_n(&h->magic, kShmMagic, __ATOMIC_RELEASE); }
    __atomic_store_n(&x->ctl(band)->ready, (uint64_t)1, __ATOMIC_RELEASE);
    const double t0 = mono_s();
    for (;;) {
        bool all = __atomic_load_n(&h->magic, __ATOMIC_ACQUIRE) == kShmMagic;
        for (int b = 0; b < nb && all && !loopback; ++b) all = __atomic_load_n(&x->ctl(b)->ready, __ATOMIC_ACQUIRE) != 0;
        if (all) break;
        if (mono_s() - t0 > 2.0 * x->timeout_s) {
            m_err(errm, errm_len, "beom_multi: band %d waited %.0f s for the other %d bands at segment %s", band, 2.0 * x->timeout_s, nb - 1, name);
            shm_unlink(name); shm_close(x); return -34;
        }
        nap_us(200);
    }
    if (h->nb != (uint64_t)nb || h->xbytes != xbytes) {
        m_err(errm, errm_len, "beom_multi: segment %s belongs to another frame (bands %llu, bytes %llu)", name, (unsigned long long)h->nb, (unsigned long long)h->xbytes);
        shm_close(x); return -34;
    }
    if (band == 0 || loopback) shm_unlink(name);
    // pinned: the copies to and from the segment are then asynchronous like any other (without it they still work, staged)
    if (hipHostRegister(x->base, x->size, hipHostRegisterDefault) == hipSuccess) x->registered = true;
    else (void)hipGetLastError();
    *out = x;
    return 0;
}

// ---- the caller's arrays cut into windows: geometry and the copy are beom_bands_host.h's ---------------------------------
template <class T> const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
template <class T> T *ptr(std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

struct StaticsV {                  // one band's (or the companion frame's) static arrays in window layout
    std::vector<double> a[8];
    const double *bodf = nullptr;
};
struct StateV { std::vector<double> a[13]; };
int upload_state_v(beom_handle h, const StateV &a, char *errm, int errm_len) {
    return beom_upload_state(h, ptr(a.a[0]), ptr(a.a[1]), ptr(a.a[2]), ptr(a.a[3]), ptr(a.a[4]), ptr(a.a[5]), ptr(a.a[6]), ptr(a.a[7]),
                             ptr(a.a[8]), ptr(a.a[9]), ptr(a.a[10]), ptr(a.a[11]), ptr(a.a[12]), errm, errm_len);
}
int download_state_v(beom_handle h, StateV &a, char *errm, int errm_len) {
    return beom_download_state(h, ptr(a.a[0]), ptr(a.a[1]), ptr(a.a[2]), ptr(a.a[3]), ptr(a.a[4]), ptr(a.a[5]), ptr(a.a[6]), ptr(a.a[7]),
                               ptr(a.a[8]), ptr(a.a[9]), ptr(a.a[10]), ptr(a.a[11]), ptr(a.a[12]), errm, errm_len);
}
// an engine from tables and masks (mk_u, mk_v, mk_n, mkpe, mkpi) and a window's statics
int create_engine(const beom_params &lp, int dev, const int32_t *neig, const int32_t *subc, const double *const (&mk)[5], const StaticsV &st,
                  beom_handle *out, char *errm, int errm_len) {
    return beom_create(&lp, dev, neig, subc, mk[0], mk[1], mk[2], mk[3], mk[4], ptr(st.a[0]), ptr(st.a[1]), ptr(st.a[2]), ptr(st.a[3]),
                       ptr(st.a[4]), ptr(st.a[5]), ptr(st.a[6]), st.bodf, ptr(st.a[7]), out, errm, errm_len);
}

const double *const *statics_ptrs(const beom_statics *s, const double *(&p)[8]) {
    p[0] = s->fcor; p[1] = s->h_th; p[2] = s->h_to; p[3] = s->nudg; p[4] = s->fnud; p[5] = s->hdot; p[6] = s->tide; p[7] = s->taus;
    return p;
}
void state_ptrs(const beom_state *s, double *(&p)[13]) {
    p[0] = s->hlay; p[1] = s->u; p[2] = s->v; p[3] = s->h_u; p[4] = s->h_v; p[5] = s->rs_h; p[6] = s->dmdx; p[7] = s->dmdy;
    p[8] = s->v_cc; p[9] = s->v_ll; p[10] = s->tt3d; p[11] = s->tb3d; p[12] = s->tu3d;
}

}  // namespace

struct beom_multi {
    beom_params P{};               // global frame
    int nb = 0;                    // bands in the chain / ring, over all processes
    int n = 0;                     // bands of THIS process
    bool ring = false;             // frame periodic in y
    int xper = 0;
    int transport = BEOM_XCHG_PEER;
    bool local_mode = false;       // created from this band's window (beom_multi_create_local)
    bool failed = false;           // a step failed half way: the state is undefined, only destroy is allowed
    bool overlap = true;           // steps cut boundary first, the exchange inside the interior sweep (beom_multi_set_option "overlap")
    size_t n1g = 0;
    bool land = false;             // a frame with land: bands are packed row ranges of unequal length, on the rectangle ("embedded") form
    std::vector<long long> gst;    // first packed cell of every global row j = 1..mm+2 (handles from global arrays; land or not)
    std::vector<int> dev;
    std::vector<Band> band;
    std::vector<beom_handle> eng;
    std::vector<hipStream_t> main_s, comm_s;          // a band's sweeps | the edge strips of a cut step and its exchange
    std::vector<hipEvent_t> packed, landed, p1done;
    std::vector<char> pending;     // an exchange into this band is in flight
    std::vector<double *> send_s, recv_s, send_n, recv_n;   // device buffers on the band's device
    std::vector<nccl_comm> comm;
    ShmXchg *shm = nullptr;        // BEOM_XCHG_SHM: the segment shared by the bands' processes
    bool loopback = false;         // BEOM_XCHG_LOOPBACK: this band receives what it sends (timing rehearsals)
    size_t xbytes = 0;
    long long n_split = 0, n_plain = 0;   // band-steps taken in two phases / in one piece
    int ntrc = 0;                  // passive tracers carried by every band (beom_multi_set_tracers): q joins the exchange
    // moments kept by every band (beom_multi_set_moments): the bands sample on request ("moments_by_caller"), the step whose
    // sample is still owed (0 = none) is taken where the main streams next join the exchange
    struct Moments { int level = 0, stride = 1, due = 0; };
    Moments mom, tmom;             // (tmom: the tracer moments likewise, beom_multi_set_tracer_moments)
    // harmonics kept by every band (beom_multi_set_harmonics), sampled where the moments are: the step whose sample is owed
    // and that step's time ctim = tres + dtd8*(double)due
    struct Harmonics { int nfreq = 0, level = 0, stride = 1, due = 0; double due_ctim = 0.0; };
    Harmonics harm;
    // series kept by every band over its owned rows (beom_multi_set_series): the record a step left owing is taken where the
    // moments' sample is; the steps of the records held (every band holds as many)
    struct Series { int level = 0, stride = 1, nrec = 0, due = 0; std::vector<int> tstp; };
    Series ser;
    Series tser;                   // the tracer series likewise (beom_multi_set_tracer_series)
    // Lagrangian floats on the bands (beom_multi_set_floats): every band holds all nflt slots; flt_mode is the float launch
    // owed where the main streams next join the exchange (0 none, 1 stage 1, 3 stage 2 + stage 1 of the next step)
    long long nflt = 0;
    int flt_cap = 0, flt_mode = 0;
    bool flt_ready = false;
    size_t flt_box_bytes = 0;
    std::vector<hipEvent_t> flt_done, flt_copied;     // behind a band's float launch | behind its copies of the neighbours' outboxes
    std::vector<void *> flt_out_s, flt_out_n, flt_in_s, flt_in_n;
    // companion frame of a y-periodic ring (lives with band 0): rows 1..kMiniLo, Mr-3..Mr, Mr+1
    beom_handle mini = nullptr;
    int mini_k = -1;               // local index of band 0, or -1 if band 0 is not here
    hipStream_t mini_s = nullptr;
    double *mini_lo = nullptr, *mini_hi = nullptr;
    hipEvent_t ev_hi = nullptr, ev_free = nullptr;
    bool free_recorded = false;
    std::vector<int> mini_rows;

    int local_of(int gidx) const { for (int k = 0; k < n; ++k) if (band[k].index == gidx) return k; return -1; }
    bool has_s(int k) const { return ring || band[k].index > 0; }
    bool has_n(int k) const { return ring || band[k].index < nb - 1; }
    int south_of(int k) const { return loopback ? band[k].index : (band[k].index - 1 + nb) % nb; }
    int north_of(int k) const { return loopback ? band[k].index : (band[k].index + 1) % nb; }
    int rank_of(int gidx) const { return loopback ? 0 : gidx; }        // RCCL rank of a band (a looped-back band is alone in its communicator)
};

namespace {

// A part of the frame: band k of this process, or (k = -1) the companion frame of a ring.  "in" cuts the caller's arrays to
// the part's window (all its rows), "out" pastes what the part owns back: a band's owned rows, the companion's orphan row.
// A handle that holds one band's window has that window in the caller's place (and the orphan row in a one-row array).
struct Part {
    int k;
    beom_handle eng;               // (null while the handle is being created)
    Spans in, out;
    size_t n1() const { return in.n1dst; }      // slots of the part's own arrays
};
std::vector<Part> parts(const beom_multi *M) {
    std::vector<Part> v;
    const int L = M->P.lm + 1;
    for (int k = 0; k < M->n; ++k) {
        const Band &b = M->band[k];
        if (M->local_mode) v.push_back({k, M->eng[k], spans_whole(b), spans_whole(b)});
        else v.push_back({k, M->eng[k], spans_in(b.row_list(), M->gst, M->n1g), spans_out(b, M->gst, M->n1g)});
    }
    if (M->mini_k >= 0) {
        if (M->local_mode) v.push_back({-1, M->mini, spans_window_to_mini(M->band[M->mini_k]), spans_mini_to_orphan(L)});
        else v.push_back({-1, M->mini, spans_in(M->mini_rows, M->gst, M->n1g), spans_orphan_out(M->P.mm, L, M->gst, M->n1g)});
    }
    return v;
}

void destroy_all(beom_multi *M) {
    if (!M) return;
    for (int k = 0; k < M->n; ++k) {
        (void)hipSetDevice(M->dev[k]);
        if (k < (int)M->main_s.size() && M->main_s[k]) (void)hipStreamSynchronize(M->main_s[k]);
        if (k < (int)M->comm_s.size() && M->comm_s[k]) (void)hipStreamSynchronize(M->comm_s[k]);
    }
    if (M->mini_k >= 0) {
        (void)hipSetDevice(M->dev[M->mini_k]);
        if (M->mini_s) (void)hipStreamSynchronize(M->mini_s);
        if (M->mini) (void)beom_destroy(M->mini);
        if (M->mini_lo) (void)hipFree(M->mini_lo);
        if (M->mini_hi) (void)hipFree(M->mini_hi);
        for (hipEvent_t e : {M->ev_hi, M->ev_free}) if (e) (void)hipEventDestroy(e);
        if (M->mini_s) (void)hipStreamDestroy(M->mini_s);
    }
    if (M->shm) { if (M->n > 0) (void)hipSetDevice(M->dev[0]); shm_close(M->shm); M->shm = nullptr; }
    for (int k = 0; k < M->n; ++k) {
        (void)hipSetDevice(M->dev[k]);
        if (k < (int)M->comm.size() && M->comm[k] && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(M->comm[k]);
        if (k < (int)M->eng.size() && M->eng[k]) (void)beom_destroy(M->eng[k]);
        for (auto *v : {&M->send_s, &M->recv_s, &M->send_n, &M->recv_n})
            if (k < (int)v->size() && (*v)[k]) (void)hipFree((*v)[k]);
        if (k < (int)M->packed.size() && M->packed[k]) (void)hipEventDestroy(M->packed[k]);
        if (k < (int)M->landed.size() && M->landed[k]) (void)hipEventDestroy(M->landed[k]);
        if (k < (int)M->p1done.size() && M->p1done[k]) (void)hipEventDestroy(M->p1done[k]);
        if (k < (int)M->flt_done.size() && M->flt_done[k]) (void)hipEventDestroy(M->flt_done[k]);
        if (k < (int)M->flt_copied.size() && M->flt_copied[k]) (void)hipEventDestroy(M->flt_copied[k]);
        if (k < (int)M->comm_s.size() && M->comm_s[k]) (void)hipStreamDestroy(M->comm_s[k]);
        if (k < (int)M->main_s.size() && M->main_s[k]) (void)hipStreamDestroy(M->main_s[k]);
    }
    delete M;
}

int check_frame(const beom_params *prm, int nb, int yper, bool global_arrays, bool land, char *errm, int errm_len) {
    const int L = prm->lm + 1, Mg = prm->mm + 1;
    if (prm->abi_version != BEOM_ABI_VERSION) { m_err(errm, errm_len, "beom_multi: ABI version mismatch"); return -2; }
    if (nb < 1 || nb > 64) { m_err(errm, errm_len, "beom_multi: bad band count %d", nb); return -3; }
    if ((!land && (long long)prm->ndeg != (long long)L * Mg) || prm->slab_mm != 0) {
        m_err(errm, errm_len, "beom_multi: the row decomposition needs a whole frame; one with land (ndeg < (lm+1)(mm+1)) only from the global arrays");
        return -3;
    }
    if (land && (yper || prm->svis > 0.0 || (prm->flag_nudging && prm->mcbc < 0.5) || prm->rgld > 0.5)) {
        m_err(errm, errm_len, "beom_multi: bands of a frame with land: not periodic in y, no biharmonic viscosity, no mcbc = 0, no rigid lid");
        return -4;
    }
    const int ring_rows = yper ? prm->mm : Mg;
    // every band sends its outermost kGhost owned rows; band 0 of a ring also lends rows 1..kMiniLo to the companion frame
    if (ring_rows < nb * (yper ? (kGhost > kMiniLo ? kGhost : kMiniLo) : kGhost + 1)) { m_err(errm, errm_len, "beom_multi: %d rows are too few for %d bands", ring_rows, nb); return -3; }
    (void)global_arrays;      // (mcbc = 0: a handle from global arrays gets the global segment table, beom_multi_set_open_boundaries; a
                              //  rank that holds only its window brings the segments of its own rows, ..._local; beom_step refuses until then)
    if (yper && prm->svis > 0.0) { m_err(errm, errm_len, "beom_multi: biharmonic viscosity on a frame periodic in y runs on a single-device handle only"); return -4; }
    return 0;
}

int finish_band(beom_multi *M, int k, char *errm, int errm_len);

// one band's engine from its window statics (tables come from the closed form)
int create_band(beom_multi *M, int k, const StaticsV &st, char *errm, int errm_len) {
    const Band &s = M->band[k];
    beom_params lp = M->P;
    lp.mm = s.rows() - 1; lp.ndeg = (int32_t)s.n_loc();
    lp.dense_hint = 1;
    int joff = 0, Mg = s.rows(), slab = 0;
    if (M->ring) { joff = kFakePad; Mg = s.rows() + 2 * kFakePad; slab = 1; }                 // deep inside a taller frame
    else if (M->nb > 1) { joff = s.own0 - s.gs - 1; Mg = M->P.mm + 1; slab = 1; }
    lp.slab_row0 = slab ? joff : 0; lp.slab_mm = slab ? Mg - 1 : 0;
    const beom_dense::Tables t = beom_dense::generate(s.L, s.rows(), joff, Mg, slab, M->xper, 0);
    M_RC(create_engine(lp, M->dev[k], t.neig.data(), t.subc.data(), {t.mk_u.data(), t.mk_v.data(), t.mk_n.data(), t.mkpe.data(), t.mkpi.data()},
                       st, &M->eng[k], errm, errm_len));
    if (!beom_is_dense(M->eng[k])) { m_err(errm, errm_len, "beom_multi: band %d did not qualify for the dense path", s.index); return -4; }
    return finish_band(M, k, errm, errm_len);
}

// Band k of a frame WITH land: the rows' packed cells with the caller's own tables, re-indexed to the window (links that
// leave the window become the sentinel: they start in the outermost ghost row, whose values nobody uses).  The engine
// lays such a band out on its rectangle ("embedded", beom_engine.hip) — that is what the ghost-row copies rely on.
int create_band_land(beom_multi *M, int k, const Spans &in, const int32_t *neig, const int32_t *subc, const double *const (&masks)[5],
                     const StaticsV &st, char *errm, int errm_len) {
    const Band &s = M->band[k];
    const size_t n1g = M->n1g, nloc = (size_t)s.n_loc(), n1l = nloc + 1;
    const int row0 = s.own0 - s.gs;                               // global row of local row 1
    const std::vector<int> rows = s.row_list();
    auto to_local = [&](int32_t p) -> int32_t {
        if (p <= 0) return 0;
        const int jl = subc[(size_t)p + n1g] - row0 + 1;
        if (jl < 1 || jl > s.rows()) return 0;
        return (int32_t)(s.lst[(size_t)jl] + ((long long)p - M->gst[(size_t)(row0 + jl - 1)]));
    };
    std::vector<int32_t> ln(8 * n1l, 0), lsub(2 * n1l, 0);
    size_t q = 1;
    for (int g : rows)
        for (long long p = M->gst[(size_t)g]; p < M->gst[(size_t)g + 1]; ++p, ++q) {
            for (int c = 0; c < 8; ++c) ln[8 * q + c] = to_local(neig[8 * (size_t)p + c]);
            lsub[q] = subc[(size_t)p];
            lsub[q + n1l] = subc[(size_t)p + n1g] - row0 + 1;
        }
    std::vector<double> lm[5];
    for (int f = 0; f < 5; ++f) lm[f] = cut_rows(masks[f], 1, 1, in);
    beom_params lp = M->P;
    lp.mm = s.rows() - 1; lp.ndeg = (int32_t)nloc; lp.dense_hint = 1;
    lp.slab_row0 = row0 - 1; lp.slab_mm = M->P.mm;              // a window of the global frame: the engine splits its steps around the exchange
    M_RC(create_engine(lp, M->dev[k], ln.data(), lsub.data(), {lm[0].data(), lm[1].data(), lm[2].data(), lm[3].data(), lm[4].data()},
                       st, &M->eng[k], errm, errm_len));
    if (beom_is_dense(M->eng[k]) < 1) {           // (2: the rectangle form with land; 1: no land at all in this window)
        m_err(errm, errm_len, "beom_multi: band %d (rows %d..%d) does not fit the rectangle form (fewer than 30 %% of its cells wet, or a coast on a periodic seam)",
              s.index, s.own0, s.own1);
        return -4;
    }
    return finish_band(M, k, errm, errm_len);
}

int finish_band(beom_multi *M, int k, char *errm, int errm_len) {
    M_HIP(hipSetDevice(M->dev[k]));
    M_HIP(hipStreamCreateWithFlags(&M->main_s[k], hipStreamNonBlocking));
    {   // the second stream at the highest priority the device offers: its kernels (the edge strips of the momentum sweep, the
        // packing, RCCL's send/recv) are few workgroups that must get through while the interior sweep fills the chip
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
            M_HIP(hipStreamCreateWithPriority(&M->comm_s[k], hipStreamNonBlocking, greatest));
        else { (void)hipGetLastError(); M_HIP(hipStreamCreateWithFlags(&M->comm_s[k], hipStreamNonBlocking)); }
    }
    M_HIP(hipEventCreateWithFlags(&M->packed[k], hipEventDisableTiming));
    M_HIP(hipEventCreateWithFlags(&M->landed[k], hipEventDisableTiming));
    M_HIP(hipEventCreateWithFlags(&M->p1done[k], hipEventDisableTiming));
    if (M->has_s(k)) { M_HIP(hipMalloc((void **)&M->send_s[k], M->xbytes)); M_HIP(hipMalloc((void **)&M->recv_s[k], M->xbytes)); }
    if (M->has_n(k)) { M_HIP(hipMalloc((void **)&M->send_n[k], M->xbytes)); M_HIP(hipMalloc((void **)&M->recv_n[k], M->xbytes)); }
    (void)beom_set_stream(M->eng[k], (void *)M->main_s[k], 0);
    return 0;
}

// the companion frame of a ring: a y-periodic frame of kMiniLo + kGhost + 1 rows on band 0's device
int create_mini(beom_multi *M, const StaticsV &st, char *errm, int errm_len) {
    const int k = M->mini_k, L = M->P.lm + 1, Mm = kMiniRows;
    beom_params lp = M->P;
    lp.mm = Mm - 1; lp.ndeg = Mm * L; lp.dense_hint = 1; lp.slab_row0 = 0; lp.slab_mm = 0;
    const beom_dense::Tables t = beom_dense::generate(L, Mm, 0, Mm, 0, M->xper, 1);
    M_RC(create_engine(lp, M->dev[k], t.neig.data(), t.subc.data(), {t.mk_u.data(), t.mk_v.data(), t.mk_n.data(), t.mkpe.data(), t.mkpi.data()},
                       st, &M->mini, errm, errm_len));
    if (!beom_is_dense(M->mini)) { m_err(errm, errm_len, "beom_multi: the companion frame did not qualify for the dense path"); return -4; }
    M_HIP(hipSetDevice(M->dev[k]));
    M_HIP(hipStreamCreateWithFlags(&M->mini_s, hipStreamNonBlocking));
    for (hipEvent_t *e : {&M->ev_hi, &M->ev_free}) M_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    const size_t row = (size_t)kFields * M->P.nlay * L * sizeof(double);
    M_HIP(hipMalloc((void **)&M->mini_lo, row * kMiniLo));
    M_HIP(hipMalloc((void **)&M->mini_hi, row * kGhost));
    (void)beom_set_stream(M->mini, (void *)M->mini_s, 0);
    return 0;
}

int init_transport(beom_multi *M, const void *rccl_id, char *errm, int errm_len) {
    const bool all_local = M->n == M->nb;
    if (M->transport == BEOM_XCHG_PEER) {
        if (!all_local) { m_err(errm, errm_len, "beom_multi: peer copies need all bands in one process; use BEOM_XCHG_RCCL"); return -3; }
        for (int k = 0; k < M->n; ++k) {           // direct peer copies over xGMI where the devices allow it (already-enabled is fine)
            M_HIP(hipSetDevice(M->dev[k]));
            for (int q : {M->south_of(k), M->north_of(k)}) {
                const int ql = M->local_of(q);
                if (ql < 0 || M->dev[ql] == M->dev[k]) continue;
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, M->dev[k], M->dev[ql]) == hipSuccess && can) {
                    hipError_t pe = hipDeviceEnablePeerAccess(M->dev[ql], 0);
                    if (pe != hipSuccess) (void)hipGetLastError();
                }
            }
        }
        return 0;
    }
    if (M->transport == BEOM_XCHG_SHM) {
        if (M->n != 1) { m_err(errm, errm_len, "beom_multi: the shared-memory transport carries one band per process"); return -3; }
        M_HIP(hipSetDevice(M->dev[0]));
        return shm_open_all(&M->shm, (const char *)rccl_id, M->nb, M->band[0].index, M->xbytes, M->loopback, errm, errm_len);
    }
    if (M->transport != BEOM_XCHG_RCCL) { m_err(errm, errm_len, "beom_multi: unknown transport %d", M->transport); return -3; }
    if (!(all_local || M->n == 1)) { m_err(errm, errm_len, "beom_multi: RCCL transport: all bands in one process, or one band per process"); return -3; }
    if (!g_rccl.load(errm, errm_len)) return -31;
    M->comm.assign(M->n, nullptr);
    if (all_local && !rccl_id) {
        for (int k = 0; k < M->n; ++k)
            for (int q = 0; q < k; ++q)
                if (M->dev[k] == M->dev[q]) { m_err(errm, errm_len, "beom_multi: RCCL needs one distinct device per band (device %d named twice)", M->dev[k]); return -3; }
        M_NCCL(g_rccl.CommInitAll(M->comm.data(), M->n, M->dev.data()));
    } else {
        if (!rccl_id) { m_err(errm, errm_len, "beom_multi: RCCL transport across processes needs the unique id of beom_rccl_unique_id"); return -3; }
        nccl_uid id;
        std::memcpy(&id, rccl_id, sizeof(id));
        M_HIP(hipSetDevice(M->dev[0]));
        M_NCCL(g_rccl.CommInitRank(&M->comm[0], M->loopback ? 1 : M->nb, id, M->rank_of(M->band[0].index)));
    }
    return 0;
}

void size_vectors(beom_multi *M) {
    const int n = M->n;
    M->eng.assign(n, nullptr);
    M->main_s.assign(n, nullptr); M->comm_s.assign(n, nullptr);
    M->packed.assign(n, nullptr); M->landed.assign(n, nullptr); M->p1done.assign(n, nullptr);
    M->pending.assign(n, 0);
    M->send_s.assign(n, nullptr); M->recv_s.assign(n, nullptr);
    M->send_n.assign(n, nullptr); M->recv_n.assign(n, nullptr);
    M->xbytes = (size_t)kFields * M->P.nlay * kGhost * (M->P.lm + 1) * sizeof(double);
}

}  // namespace

extern "C" {

int beom_rccl_unique_id(void *id128, char *errm, int errm_len) {
    if (!id128) { m_err(errm, errm_len, "beom_rccl_unique_id: null argument"); return -1; }
    if (!g_rccl.load(errm, errm_len)) return -31;
    nccl_uid id;
    M_NCCL(g_rccl.GetUniqueId(&id));
    std::memcpy(id128, &id, sizeof(id));
    return 0;
}

int beom_rccl_version(char *errm, int errm_len) {
    if (!g_rccl.load(errm, errm_len)) return -31;
    int v = 0;
    M_NCCL(g_rccl.GetVersion(&v));
    return v;
}

int beom_multi_create_ex(const beom_params *prm, int ndev, const int *devices, int transport_and_flags,
                         const int32_t *neig, const int32_t *subc,
                         const double *mk_u, const double *mk_v, const double *mk_n,
                         const double *mkpe, const double *mkpi,
                         const double *fcor, const double *h_th, const double *h_to,
                         const double *nudg, const double *fnud, const double *hdot,
                         const double *tide, const double *bodf, const double *taus,
                         beom_multi_handle *out, char *errm, int errm_len) {
    if (!prm || !out || !devices || !neig || !subc || !mk_u || !mk_v || !mk_n || !mkpe || !mkpi || !fcor || !h_th || !nudg || !fnud) {
        m_err(errm, errm_len, "beom_multi_create: null argument"); return -1;
    }
    *out = nullptr;
    const int L = prm->lm + 1, Mg = prm->mm + 1, nl = prm->nlay;
    // periodicity is encoded only in neig (private_mod.f95:614-685): W of cell (1,1) / S of cell (1,1)
    const int xper = neig[8 * 1 + 4] != 0, yper = neig[8 * 1 + 6] != 0;
    const int transport = transport_and_flags & 0xff;
    const bool whole = ndev == 1 && !(yper && (transport_and_flags & BEOM_XCHG_RING1));      // one band = the frame itself
    bool land = false;
    if (!whole) {
        land = (long long)prm->ndeg != (long long)L * Mg;
        M_RC(check_frame(prm, ndev, yper, true, land, errm, errm_len));
        if (!land && !beom_dense::verify(L, Mg, 0, Mg, 0, xper, yper, prm->ndeg, neig, subc, mk_u, mk_v, mk_n, mkpe, mkpi)) {
            m_err(errm, errm_len, "beom_multi_create: the row decomposition needs a dense frame (interior entirely wet)");
            return -4;
        }
    } else if (prm->abi_version != BEOM_ABI_VERSION) { m_err(errm, errm_len, "beom_multi_create: ABI version mismatch"); return -2; }
    beom_multi *M = new beom_multi();
    M->P = *prm; M->nb = ndev; M->n = ndev; M->n1g = (size_t)prm->ndeg + 1;
    M->ring = !whole && yper; M->xper = xper; M->transport = transport;
    M->dev.assign(devices, devices + ndev);
    if (getenv("BEOM_MULTI_WRAP_DEVICES")) {     // rehearsals: more bands than GPUs, ids taken modulo the visible count
        int nvis = 0;
        if (hipGetDeviceCount(&nvis) == hipSuccess && nvis > 0)
            for (int &dv : M->dev) dv %= nvis;
    }
    size_vectors(M);
    const size_t n1g = M->n1g;
    int rc = 0;
    if (whole) {                                  // the caller's own tables, any coastline
        Band s; s.index = 0; s.own0 = 1; s.own1 = Mg; s.L = L;      // (no window: nothing is cut, lst stays empty)
        M->band.push_back(s);
        rc = beom_create(prm, M->dev[0], neig, subc, mk_u, mk_v, mk_n, mkpe, mkpi, fcor, h_th, h_to, nudg, fnud, hdot, tide, bodf, taus,
                         &M->eng[0], errm, errm_len);
        if (!rc && hipStreamCreateWithFlags(&M->main_s[0], hipStreamNonBlocking) != hipSuccess) { m_err(errm, errm_len, "hipStreamCreate failed"); rc = -100; }
        if (!rc) (void)beom_set_stream(M->eng[0], (void *)M->main_s[0], 0);
        if (rc) { destroy_all(M); return rc; }
        *out = M;
        return 0;
    }
    const double *src[8] = {fcor, h_th, h_to, nudg, fnud, hdot, tide, taus};
    const double *const masks[5] = {mk_u, mk_v, mk_n, mkpe, mkpi};
    if (land) {
        // rows as packed ranges (packing is j-major: subc's row number never decreases along the packed index)
        M->land = true;
        M->gst.assign((size_t)Mg + 3, 0);
        int jprev = 1;
        M->gst[1] = 1;
        for (size_t p = 1; p < n1g && !rc; ++p) {
            const int j = subc[p + n1g];
            if (j < jprev || j > Mg) { m_err(errm, errm_len, "beom_multi_create: the packed cells are not ordered by row (cell %d)", (int)p); rc = -4; break; }
            for (; jprev < j; ++jprev) M->gst[(size_t)jprev + 1] = (long long)p;
        }
        for (; jprev <= Mg + 1; ++jprev) M->gst[(size_t)jprev + 1] = (long long)n1g;
        // bands of equal packed-cell count (balance on the cells of a row range), at least kGhost + 1 rows each
        const int minrows = kGhost + 1;
        int j = 1;
        for (int k = 0; k < ndev && !rc; ++k) {
            Band b; b.index = k; b.L = L;
            b.own0 = j;
            const long long target = (long long)prm->ndeg * (k + 1) / ndev;
            const int last_allowed = Mg - (ndev - 1 - k) * minrows;
            int e = j + minrows - 1;
            while (e < last_allowed && M->gst[(size_t)e + 1] - 1 < target) ++e;
            if (k == ndev - 1) e = Mg;
            if (e > last_allowed || e < j) { m_err(errm, errm_len, "beom_multi_create: %d rows are too few for %d bands", Mg, ndev); rc = -3; break; }
            b.own1 = e; j = e + 1;
            b.gs = k > 0 ? kGhost : 0; b.gn = k < ndev - 1 ? kGhost : 0;
            b.lst = local_starts(b.row_list(), M->gst);
            M->band.push_back(b);
        }
    } else {                                      // the same geometry in closed form: every row L cells long
        M->gst = dense_starts(Mg, L);
        for (int k = 0; k < ndev; ++k) M->band.push_back(make_band(prm->lm, prm->mm, ndev, k, M->ring));
        if (M->ring) { M->mini_k = 0; M->mini_rows = mini_row_list(prm->mm); }
    }
    if (!rc)
        for (const Part &p : parts(M)) {
            StaticsV st;
            for (int f = 0; f < 8; ++f) st.a[f] = cut_rows(src[f], kStatic[f].outer(nl), kStatic[f].inner, p.in);
            st.bodf = bodf;
            rc = p.k < 0 ? create_mini(M, st, errm, errm_len)
                 : land  ? create_band_land(M, p.k, p.in, neig, subc, masks, st, errm, errm_len)
                         : create_band(M, p.k, st, errm, errm_len);
            if (rc) break;
        }
    if (!rc) rc = init_transport(M, nullptr, errm, errm_len);
    if (rc) { destroy_all(M); return rc; }
    *out = M;
    return 0;
}

int beom_multi_create(const beom_params *prm, int ndev, const int *devices,
                      const int32_t *neig, const int32_t *subc,
                      const double *mk_u, const double *mk_v, const double *mk_n,
                      const double *mkpe, const double *mkpi,
                      const double *fcor, const double *h_th, const double *h_to,
                      const double *nudg, const double *fnud, const double *hdot,
                      const double *tide, const double *bodf, const double *taus,
                      beom_multi_handle *out, char *errm, int errm_len) {
    const char *t = getenv("BEOM_XCHG");          // "rccl": the Fortran host picks the transport by environment
    const int transport = (t && (!strcmp(t, "rccl") || !strcmp(t, "RCCL"))) ? BEOM_XCHG_RCCL : BEOM_XCHG_PEER;
    return beom_multi_create_ex(prm, ndev, devices, transport, neig, subc, mk_u, mk_v, mk_n, mkpe, mkpi, fcor, h_th, h_to,
                                nudg, fnud, hdot, tide, bodf, taus, out, errm, errm_len);
}

int beom_multi_window(const beom_params *prm, int nb, int band, int yper, int *own0, int *own1, int *ghost_s, int *ghost_n) {
    if (!prm || nb < 1 || band < 0 || band >= nb) return -3;
    const Band s = make_band(prm->lm, prm->mm, nb, band, yper != 0);
    if (own0) *own0 = s.own0;
    if (own1) *own1 = s.own1;
    if (ghost_s) *ghost_s = s.gs;
    if (ghost_n) *ghost_n = s.gn;
    return 0;
}

int beom_multi_create_local(const beom_params *prm, int nb, int band, int device, int xper, int yper,
                            const void *rccl_id, const beom_statics *win, const beom_statics *orphan,
                            beom_multi_handle *out, char *errm, int errm_len) {
    return beom_multi_create_local_ex(prm, nb, band, device, xper, yper, BEOM_XCHG_RCCL, rccl_id, win, orphan, out, errm, errm_len);
}

int beom_multi_create_local_ex(const beom_params *prm, int nb, int band, int device, int xper, int yper,
                               int transport_and_flags, const void *xchg_id, const beom_statics *win, const beom_statics *orphan,
                               beom_multi_handle *out, char *errm, int errm_len) {
    if (!prm || !out || !win || !win->fcor || !win->h_th || !win->nudg || !win->fnud) { m_err(errm, errm_len, "beom_multi_create_local: null argument"); return -1; }
    *out = nullptr;
    const int transport = transport_and_flags & 0xff;
    const void *rccl_id = xchg_id;
    if (transport != BEOM_XCHG_RCCL && transport != BEOM_XCHG_SHM) { m_err(errm, errm_len, "beom_multi_create_local: one band per process exchanges over RCCL or shared memory"); return -3; }
    if (band < 0 || band >= nb) { m_err(errm, errm_len, "beom_multi_create_local: band %d of %d", band, nb); return -3; }
    M_RC(check_frame(prm, nb, yper, false, false, errm, errm_len));
    const bool ring = yper != 0;
    if (ring && band == 0 && (!orphan || !orphan->fcor || !orphan->h_th || !orphan->nudg || !orphan->fnud)) {
        m_err(errm, errm_len, "beom_multi_create_local: band 0 of a frame periodic in y also carries row mm+1 (orphan statics needed)");
        return -1;
    }
    beom_multi *M = new beom_multi();
    M->P = *prm; M->nb = nb; M->n = 1; M->n1g = (size_t)prm->ndeg + 1;
    M->ring = ring; M->xper = xper != 0; M->transport = transport; M->local_mode = true;
    M->loopback = (transport_and_flags & BEOM_XCHG_LOOPBACK) != 0;
    M->dev.assign(1, device);
    size_vectors(M);
    M->band.push_back(make_band(prm->lm, prm->mm, nb, band, ring));
    if (ring && band == 0) { M->mini_k = 0; M->mini_rows = mini_row_list(prm->mm); }
    const int nl = prm->nlay;
    const double *wp[8], *op[8] = {};
    statics_ptrs(win, wp);
    if (M->mini_k >= 0) statics_ptrs(orphan, op);
    int rc = 0;
    for (const Part &p : parts(M)) {              // the band from its window as it stands, the companion frame from window and orphan row
        StaticsV st;
        for (int f = 0; f < 8; ++f) {
            st.a[f] = cut_rows(wp[f], kStatic[f].outer(nl), kStatic[f].inner, p.in);
            if (p.k < 0) copy_rows(ptr(st.a[f]), op[f], kStatic[f].outer(nl), kStatic[f].inner, spans_orphan_to_mini(prm->lm + 1));
        }
        st.bodf = win->bodf;
        rc = p.k < 0 ? create_mini(M, st, errm, errm_len) : create_band(M, p.k, st, errm, errm_len);
        if (rc) break;
    }
    if (!rc && (nb > 1 || ring)) rc = init_transport(M, rccl_id, errm, errm_len);
    if (rc) { destroy_all(M); return rc; }
    *out = M;
    return 0;
}

int beom_multi_destroy(beom_multi_handle M) { destroy_all(M); return 0; }

int beom_multi_count(beom_multi_handle M) { return M ? M->n : -1; }

int beom_multi_band(beom_multi_handle M, int k, int *own0, int *own1, int *win0, int *win1, int *device) {
    if (!M || k < 0 || k >= M->n) return -3;
    if (own0) *own0 = M->band[k].own0;
    if (own1) *own1 = M->band[k].own1;
    if (win0) *win0 = M->band[k].own0 - M->band[k].gs;        // <= 0 / > mm: ghost rows of a ring wrap
    if (win1) *win1 = M->band[k].own1 + M->band[k].gn;
    if (device) *device = M->dev[k];
    return 0;
}

int beom_multi_engine(beom_multi_handle M, int k, beom_handle *out) {
    if (!M || !out || k < -1 || k >= M->n) return -3;
    *out = k < 0 ? M->mini : M->eng[k];
    return 0;
}

int beom_multi_stats(beom_multi_handle M, long long *split_band_steps, long long *plain_band_steps) {
    if (!M) return -1;
    if (split_band_steps) *split_band_steps = M->n_split;
    if (plain_band_steps) *plain_band_steps = M->n_plain;
    return 0;
}

// "overlap" (default 1): steps run in two phases around the ghost exchange still in flight; 0 = every step waits
// for its ghosts first (same results; bench.py checks one form against the other on the machine at hand).
// Any other name is forwarded to every local band (beom_set_option).
int beom_multi_set_option(beom_multi_handle M, const char *name, int value) {
    if (!M || !name) return -1;
    if (!strcmp(name, "overlap")) { M->overlap = value != 0; return 0; }
    if (!strcmp(name, "edge_stream")) return 0;       // (an option of the earlier split form; accepted, without effect)
    if (!strcmp(name, "moments_by_caller")) return -3;   // (the bands' samples are placed by beom_multi_step)
    int rc = 0;
    for (int k = 0; k < M->n && !rc; ++k) rc = beom_set_option(M->eng[k], name, value);
    if (!rc && M->mini) rc = beom_set_option(M->mini, name, value);
    return rc;
}

int beom_multi_describe(beom_multi_handle M, int *bands_total, int *bands_local, int *transport, int *ring, int *rccl_version) {
    if (!M) return -1;
    if (bands_total) *bands_total = M->nb;
    if (bands_local) *bands_local = M->n;
    if (transport) *transport = M->transport;
    if (ring) *ring = M->ring ? 1 : 0;
    if (rccl_version) { *rccl_version = 0; if (g_rccl.lib) (void)g_rccl.GetVersion(rccl_version); }
    return 0;
}

int beom_multi_sync(beom_multi_handle M, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    for (int k = 0; k < M->n; ++k) {
        M_HIP(hipSetDevice(M->dev[k]));
        M_HIP(hipStreamSynchronize(M->main_s[k]));
        if (M->comm_s[k]) M_HIP(hipStreamSynchronize(M->comm_s[k]));
        M->pending[k] = 0;          // whatever was in flight has landed
    }
    if (M->mini) { M_HIP(hipSetDevice(M->dev[M->mini_k])); M_HIP(hipStreamSynchronize(M->mini_s)); }
    M_HIP(hipGetLastError());
    if (M->shm && M->shm->failed) { M->failed = true; m_err(errm, errm_len, "beom_multi: a neighbour's ghost rows did not arrive within %.0f s (shared-memory transport)", M->shm->timeout_s); return -35; }
    return 0;
}

int beom_multi_upload_state(beom_multi_handle M, const double *hlay, const double *u, const double *v,
                            const double *h_u, const double *h_v, const double *rs_h, const double *dmdx,
                            const double *dmdy, const double *v_cc, const double *v_ll, const double *tt3d,
                            const double *tb3d, const double *tu3d, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_upload_state: this handle holds a window (use beom_multi_upload_local)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    const int nl = M->P.nlay;
    const double *src[13] = {hlay, u, v, h_u, h_v, rs_h, dmdx, dmdy, v_cc, v_ll, tt3d, tb3d, tu3d};
    if (M->nb == 1 && !M->ring)
        return beom_upload_state(M->eng[0], hlay, u, v, h_u, h_v, rs_h, dmdx, dmdy, v_cc, v_ll, tt3d, tb3d, tu3d, errm, errm_len);
    for (const Part &p : parts(M)) {
        StateV a;
        for (int f = 0; f < 13; ++f) a.a[f] = cut_rows(src[f], kState[f].outer(nl), kState[f].inner, p.in);
        M_RC(upload_state_v(p.eng, a, errm, errm_len));
    }
    return 0;
}

int beom_multi_download_state(beom_multi_handle M, double *hlay, double *u, double *v, double *h_u, double *h_v,
                              double *rs_h, double *dmdx, double *dmdy, double *v_cc, double *v_ll,
                              double *tt3d, double *tb3d, double *tu3d, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_download_state: this handle holds a window (use beom_multi_download_local)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    const int nl = M->P.nlay;
    double *dst[13] = {hlay, u, v, h_u, h_v, rs_h, dmdx, dmdy, v_cc, v_ll, tt3d, tb3d, tu3d};
    if (M->nb == 1 && !M->ring)
        return beom_download_state(M->eng[0], hlay, u, v, h_u, h_v, rs_h, dmdx, dmdy, v_cc, v_ll, tt3d, tb3d, tu3d, errm, errm_len);
    for (const Part &p : parts(M)) {
        StateV a;
        for (int f = 0; f < 13; ++f) if (dst[f]) a.a[f].assign(kState[f].outer(nl) * p.n1() * kState[f].inner, 0.0);
        M_RC(download_state_v(p.eng, a, errm, errm_len));
        for (int f = 0; f < 13; ++f) copy_rows(dst[f], ptr(a.a[f]), kState[f].outer(nl), kState[f].inner, p.out);
    }
    return 0;
}

// ---- passive tracers (beom_set_tracers) on the bands: global arrays cut and pasted as the state is; q travels with the
//      five fields of the exchange (beom_pack_rows packs it behind them), so the buffers grow to 5 + ntrc fields ----
static int tracers_refused(beom_multi *M, const char *who, char *errm, int errm_len) {
    if (M->local_mode) { m_err(errm, errm_len, "%s: a handle that holds one band's window does not carry tracers (its exchange is sized at creation)", who); return -6; }
    if (M->ring) { m_err(errm, errm_len, "%s: bands of a frame periodic in y do not carry tracers (the ring's companion frame has no q); use a single handle", who); return -6; }
    return 0;
}

int beom_multi_set_tracers(beom_multi_handle M, int ntrc, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "beom_multi_set_tracers: an earlier step failed half way; destroy the handle"); return -30; }
    if (ntrc < 0 || ntrc > BEOM_MAX_TRACERS) { m_err(errm, errm_len, "beom_multi_set_tracers: %d tracers (0..%d)", ntrc, BEOM_MAX_TRACERS); return -3; }
    M_RC(tracers_refused(M, "beom_multi_set_tracers", errm, errm_len));
    M_RC(beom_multi_sync(M, errm, errm_len));
    for (int k = 0; k < M->n; ++k) M_RC(beom_set_tracers(M->eng[k], ntrc, errm, errm_len));
    if (ntrc != M->ntrc) { M->tmom = {}; M->tser = {}; }       // (the bands freed their tracer moments and tracer series)
    M->ntrc = ntrc;
    if (M->nb == 1) return 0;
    // the exchange buffers for 5 + ntrc fields (nothing is in flight after the sync)
    M->xbytes = (size_t)(kFields + ntrc) * M->P.nlay * kGhost * (M->P.lm + 1) * sizeof(double);
    for (int k = 0; k < M->n; ++k) {
        M_HIP(hipSetDevice(M->dev[k]));
        M->pending[k] = 0;
        for (auto *v : {&M->send_s, &M->recv_s, &M->send_n, &M->recv_n}) {
            const bool south = v == &M->send_s || v == &M->recv_s;
            if ((*v)[k]) { M_HIP(hipFree((*v)[k])); (*v)[k] = nullptr; }
            if (south ? M->has_s(k) : M->has_n(k)) M_HIP(hipMalloc((void **)&(*v)[k], M->xbytes));
        }
    }
    return 0;
}

int beom_multi_set_tracer_scheme(beom_multi_handle M, int scheme, char *errm, int errm_len) {
    if (scheme != 1 && scheme != 2) { m_err(errm, errm_len, "beom_multi_set_tracer_scheme: scheme %d (1 = upstream, 2 = limited)", scheme); return -3; }
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "beom_multi_set_tracer_scheme: an earlier step failed half way; destroy the handle"); return -30; }
    for (int k = 0; k < M->n; ++k) M_RC(beom_set_tracer_scheme(M->eng[k], scheme, errm, errm_len));
    return 0;
}

// beom_set_tracer_mixing on every band: the same coefficients, looked at by band 0 before any band is touched
int beom_multi_set_tracer_mixing(beom_multi_handle M, const double *kappa, const double *decay, const double *source, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "beom_multi_set_tracer_mixing: an earlier step failed half way; destroy the handle"); return -30; }
    M_RC(tracers_refused(M, "beom_multi_set_tracer_mixing", errm, errm_len));
    if (M->ntrc < 1) { m_err(errm, errm_len, "beom_multi_set_tracer_mixing: the handle carries no tracer (beom_multi_set_tracers comes first)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    for (int k = 0; k < M->n; ++k) M_RC(beom_set_tracer_mixing(M->eng[k], kappa, decay, source, errm, errm_len));
    return 0;
}

// beom_set_tracer_vmixing on every band: the same coefficients, looked at by band 0 before any band is touched.  A column
// is its own cell's: the launch covers a band's whole window and the ghost rows come out as the neighbour's own rows do.
int beom_multi_set_tracer_vmixing(beom_multi_handle M, const double *kappa_v, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "beom_multi_set_tracer_vmixing: an earlier step failed half way; destroy the handle"); return -30; }
    M_RC(tracers_refused(M, "beom_multi_set_tracer_vmixing", errm, errm_len));
    if (M->ntrc < 1) { m_err(errm, errm_len, "beom_multi_set_tracer_vmixing: the handle carries no tracer (beom_multi_set_tracers comes first)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    for (int k = 0; k < M->n; ++k) M_RC(beom_set_tracer_vmixing(M->eng[k], kappa_v, errm, errm_len));
    return 0;
}

int beom_multi_upload_tracers(beom_multi_handle M, const double *q, const double *rq, const double *ctrg, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    M_RC(tracers_refused(M, "beom_multi_upload_tracers", errm, errm_len));
    if (M->ntrc < 1) { m_err(errm, errm_len, "beom_multi_upload_tracers: the handle carries no tracer (beom_multi_set_tracers)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (M->nb == 1) return beom_upload_tracers(M->eng[0], q, rq, ctrg, errm, errm_len);
    const size_t outer = (size_t)M->ntrc * M->P.nlay;
    const double *src[3] = {q, rq, ctrg};
    const size_t inner[3] = {1, 2, 1};
    for (const Part &p : parts(M)) {
        std::vector<double> a[3];
        for (int f = 0; f < 3; ++f) a[f] = cut_rows(src[f], outer, inner[f], p.in);
        M_RC(beom_upload_tracers(p.eng, ptr(a[0]), ptr(a[1]), ptr(a[2]), errm, errm_len));
    }
    return 0;
}

int beom_multi_download_tracers(beom_multi_handle M, double *q, double *rq, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    M_RC(tracers_refused(M, "beom_multi_download_tracers", errm, errm_len));
    if (M->ntrc < 1) { m_err(errm, errm_len, "beom_multi_download_tracers: the handle carries no tracer (beom_multi_set_tracers)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (M->nb == 1) return beom_download_tracers(M->eng[0], q, rq, errm, errm_len);
    const size_t outer = (size_t)M->ntrc * M->P.nlay;
    double *dst[2] = {q, rq};
    const size_t inner[2] = {1, 2};
    for (const Part &p : parts(M)) {
        std::vector<double> a[2];
        for (int f = 0; f < 2; ++f) if (dst[f]) a[f].assign(outer * p.n1() * inner[f], 0.0);
        M_RC(beom_download_tracers(p.eng, ptr(a[0]), ptr(a[1]), errm, errm_len));
        for (int f = 0; f < 2; ++f) copy_rows(dst[f], ptr(a[f]), outer, inner[f], p.out);
    }
    return 0;
}

// ---- Lagrangian floats (beom_set_floats) on the bands: replicated slots, the owner acts, a float that leaves its band's rows
//      travels as one 64-byte record through an outbox (include/beom_hip.h "Floats on bands"; beom_floats.h) ----
static bool multi_whole(const beom_multi *M) { return M->nb == 1 && !M->ring; }

// is floor(y) + 1 a row of band b?  (the kernels' owner test, on the host)
static bool band_owns(const beom_multi *M, const Band &b, double y) {
    const double fy = std::floor(y);
    const int lim = M->ring ? M->P.mm : M->P.mm + 1;
    if (!(fy >= 0.0 && fy < (double)lim)) return false;
    const int g = (int)fy + 1;
    return g >= b.own0 && g <= b.own1;
}

int beom_multi_set_floats(beom_multi_handle M, int64_t n, int capacity, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "beom_multi_set_floats: an earlier step failed half way; destroy the handle"); return -30; }
    if (n < 0 || capacity < 0) { m_err(errm, errm_len, "beom_multi_set_floats: %lld floats, capacity %d (n >= 0, capacity >= 0)", (long long)n, capacity); return -3; }
    if (M->local_mode) {
        m_err(errm, errm_len, "beom_multi_set_floats: a handle that holds one band's window does not carry floats: a float that leaves the band would "
              "have to travel to another process (fixed-size messages over RCCL or shared memory), which is not built; use a handle created from the global arrays");
        return -6;
    }
    M_RC(beom_multi_sync(M, errm, errm_len));
    M->nflt = 0; M->flt_ready = false; M->flt_mode = 0;
    if (multi_whole(M)) {
        M_RC(beom_set_floats(M->eng[0], n, 0, 1, errm, errm_len));
        M->nflt = (long long)n;
        return 0;
    }
    if (capacity == 0) capacity = (int)std::min<long long>(std::max<long long>(4096, (long long)n / 8), 1ll << 24);
    const int nb = M->n;
    if (M->flt_done.empty()) {
        M->flt_done.assign(nb, nullptr); M->flt_copied.assign(nb, nullptr);
        for (int k = 0; k < nb; ++k) {
            M_HIP(hipSetDevice(M->dev[k]));
            M_HIP(hipEventCreateWithFlags(&M->flt_done[k], hipEventDisableTiming));
            M_HIP(hipEventCreateWithFlags(&M->flt_copied[k], hipEventDisableTiming));
        }
    }
    M->flt_out_s.assign(nb, nullptr); M->flt_out_n.assign(nb, nullptr); M->flt_in_s.assign(nb, nullptr); M->flt_in_n.assign(nb, nullptr);
    for (int k = 0; k < nb; ++k) {
        const Band &b = M->band[k];
        const bool one = M->nb == 1;           // a ring of one band: nothing ever leaves it
        M_RC(beom_band_floats_set(M->eng[k], n, capacity, b.own0, b.nown(), b.gs, !one && M->has_s(k), !one && M->has_n(k), M->P.mm, M->xper,
                                  M->ring ? 1 : 0, errm, errm_len));
        if (n > 0 && beom_band_floats_boxes(M->eng[k], &M->flt_out_s[k], &M->flt_out_n[k], &M->flt_in_s[k], &M->flt_in_n[k], &M->flt_box_bytes)) {
            m_err(errm, errm_len, "beom_band_floats_boxes failed on band %d", b.index); return -3;
        }
    }
    M->nflt = (long long)n; M->flt_cap = n > 0 ? capacity : 0;
    return 0;
}

int beom_multi_upload_floats(beom_multi_handle M, const double *x, const double *y, const int32_t *layer, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->nflt < 1) { m_err(errm, errm_len, "beom_multi_upload_floats: the handle carries no float (beom_multi_set_floats)"); return -3; }
    if (!x || !y || !layer) { m_err(errm, errm_len, "beom_multi_upload_floats: null array"); return -1; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (multi_whole(M)) {
        M_RC(beom_upload_floats(M->eng[0], x, y, layer, errm, errm_len));
        M->flt_ready = true;
        return 0;
    }
    const unsigned long long none = ~0ull, n = (unsigned long long)M->nflt;
    unsigned long long bad_layer = none, nobody = none, first_dry = none;
    for (unsigned long long t = 0; t < n && bad_layer == none; ++t)
        if (layer[t] < 1 || layer[t] > M->P.nlay) bad_layer = t;
    for (unsigned long long t = 0; t < n && nobody == none; ++t) {
        bool owned = false;
        for (int k = 0; k < M->n && !owned; ++k) owned = band_owns(M, M->band[k], y[t]);
        if (!owned) nobody = t;
    }
    for (int k = 0; k < M->n; ++k) {            // every band checks the floats of its rows
        unsigned long long fd = none;
        M_RC(beom_band_floats_check(M->eng[k], x, y, &fd, errm, errm_len));
        if (fd < first_dry) first_dry = fd;
    }
    const unsigned long long first = std::min(bad_layer, std::min(nobody, first_dry));
    if (first != none) {
        if (first == bad_layer)
            m_err(errm, errm_len, "beom_multi_upload_floats: float %llu has layer %d, outside 1..%d (nothing uploaded)", first, (int)layer[first], M->P.nlay);
        else if (first == nobody)
            m_err(errm, errm_len, "beom_multi_upload_floats: float %llu at (%.17g, %.17g) lies in no band's rows (row %.0f of 1..%d; nothing uploaded)",
                  first, x[first], y[first], std::floor(y[first]) + 1.0, M->ring ? M->P.mm : M->P.mm + 1);
        else
            m_err(errm, errm_len, "beom_multi_upload_floats: float %llu at (%.17g, %.17g) does not start in a wet cell: cell (%.0f, %.0f) of the "
                  "%d x %d frame is dry, land or outside (nothing uploaded)", first, x[first], y[first], std::floor(x[first]) + 1.0,
                  std::floor(y[first]) + 1.0, M->P.lm, M->P.mm);
        return -3;
    }
    for (int k = 0; k < M->n; ++k) M_RC(beom_band_floats_commit(M->eng[k], layer, errm, errm_len));
    M->flt_ready = true; M->flt_mode = 0;
    return 0;
}

int beom_multi_download_floats(beom_multi_handle M, double *x, double *y, int32_t *layer, int32_t *rejected, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->nflt < 1) { m_err(errm, errm_len, "beom_multi_download_floats: the handle carries no float (beom_multi_set_floats)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (multi_whole(M)) return beom_download_floats(M->eng[0], x, y, layer, rejected, errm, errm_len);
    if (!M->flt_ready) { m_err(errm, errm_len, "beom_multi_download_floats: the floats have no positions yet (beom_multi_upload_floats)"); return -3; }
    const size_t n = (size_t)M->nflt;
    std::vector<double> bx(n), by(n);
    std::vector<int32_t> br(n);
    std::vector<unsigned char> claims(n, 0);
    unsigned long long reach = 0, dropped = 0;
    for (int k = 0; k < M->n; ++k) {
        unsigned long long st[3] = {0, 0, 0};
        M_RC(beom_band_floats_download(M->eng[k], bx.data(), by.data(), k == 0 ? layer : nullptr, br.data(), st, errm, errm_len));
        reach += st[0]; dropped += st[1];
        for (size_t t = 0; t < n; ++t) {
            if (!band_owns(M, M->band[k], by[t])) continue;      // a stale copy: it points outside this band
            if (claims[t] < 255) ++claims[t];
            if (x) x[t] = bx[t];
            if (y) y[t] = by[t];
            if (rejected) rejected[t] = br[t];
        }
    }
    if (reach) {
        m_err(errm, errm_len, "beom_multi_download_floats: %llu lookups fell on rows of the frame outside their band's window (cdt |v| >= 1: a float moved "
              "more than a row per stage); the positions are not valid", reach);
        return BEOM_ERR_FLOAT_REACH;
    }
    if (dropped) {
        m_err(errm, errm_len, "beom_multi_download_floats: %llu hand-over records were dropped by a full outbox (capacity %d records per side and step); "
              "the positions are not valid: set a larger capacity", dropped, M->flt_cap);
        return BEOM_ERR_FLOAT_OVERFLOW;
    }
    for (size_t t = 0; t < n; ++t)
        if (claims[t] != 1) {
            m_err(errm, errm_len, "beom_multi_download_floats: float %zu is claimed by %d bands instead of one", t, (int)claims[t]);
            return BEOM_ERR_FLOAT_CLAIM;
        }
    return 0;
}

// a float launch on every band's main stream (which has joined the exchange: the ghost rows are the neighbours' values), and
// behind a stage 2 the hand-over: every band copies its neighbours' outboxes, then ingests them.  Stream events only: a copy
// waits for the sender's float launch; the ingest, which also empties this band's own outboxes, for the neighbours' copies.
static int multi_float_launch(beom_multi *M, int mode, char *errm, int errm_len) {
    const int n = M->n;
    for (int k = 0; k < n; ++k)
        if (beom_band_floats_launch(M->eng[k], mode)) { m_err(errm, errm_len, "beom_band_floats_launch failed on band %d", M->band[k].index); return -3; }
    if (!(mode & 2) || M->nb == 1) return 0;
    for (int k = 0; k < n; ++k) {
        M_HIP(hipSetDevice(M->dev[k]));
        M_HIP(hipEventRecord(M->flt_done[k], M->main_s[k]));
    }
    for (int k = 0; k < n; ++k) {
        M_HIP(hipSetDevice(M->dev[k]));
        if (M->has_s(k)) {          // what the south neighbour sent north
            const int q = M->local_of(M->south_of(k));
            M_HIP(hipStreamWaitEvent(M->main_s[k], M->flt_done[q], 0));
            M_HIP(hipMemcpyPeerAsync(M->flt_in_s[k], M->dev[k], M->flt_out_n[q], M->dev[q], M->flt_box_bytes, M->main_s[k]));
        }
        if (M->has_n(k)) {
            const int q = M->local_of(M->north_of(k));
            M_HIP(hipStreamWaitEvent(M->main_s[k], M->flt_done[q], 0));
            M_HIP(hipMemcpyPeerAsync(M->flt_in_n[k], M->dev[k], M->flt_out_s[q], M->dev[q], M->flt_box_bytes, M->main_s[k]));
        }
        M_HIP(hipEventRecord(M->flt_copied[k], M->main_s[k]));
    }
    for (int k = 0; k < n; ++k) {
        M_HIP(hipSetDevice(M->dev[k]));
        for (int q : {M->south_of(k), M->north_of(k)}) M_HIP(hipStreamWaitEvent(M->main_s[k], M->flt_copied[M->local_of(q)], 0));
        if (beom_band_floats_ingest(M->eng[k])) { m_err(errm, errm_len, "beom_band_floats_ingest failed on band %d", M->band[k].index); return -3; }
    }
    return 0;
}

// every band's main stream joins the exchange in flight
static int multi_join_exchange(beom_multi *M, char *errm, int errm_len) {
    for (int k = 0; k < M->n; ++k) {
        if (!M->pending[k]) continue;
        M_HIP(hipSetDevice(M->dev[k]));
        M_HIP(hipStreamWaitEvent(M->main_s[k], M->landed[k], 0));
    }
    return 0;
}

int beom_multi_update_floats(beom_multi_handle M, int stage) {
    if (!M) return -1;
    if (M->failed) return -30;
    if (M->nflt < 1 || !M->flt_ready || (stage != 1 && stage != 2)) return -3;
    if (multi_whole(M)) return beom_update_floats(M->eng[0], stage);
    char errm[8]; const int errm_len = 0;
    M_RC(multi_join_exchange(M, errm, errm_len));
    return multi_float_launch(M, stage, errm, errm_len);
}

// ---- moments (beom_set_moments) on the bands: every band accumulates over all its rows, ghosts included, and the global
//      arrays take the owned rows; a ring's row mm+1 comes from the companion frame, which samples behind its own steps.
//      Tracer moments (beom_set_tracer_moments) likewise: every band samples over its whole window, behind the wait for
//      the landed ghost rows (the S row of a band's first owned row then holds the neighbour's owned values).  Rings and
//      handles that hold one band's window carry no tracers, hence no tracer moments. ----
static int moments_refused(beom_multi *M, const char *text, char *errm, int errm_len) {
    if (M->local_mode && text) { m_err(errm, errm_len, "%s", text); return -6; }
    return 0;
}
static int tracer_moments_refused(beom_multi *M, const char *who, char *errm, int errm_len) {
    if (M->local_mode) { m_err(errm, errm_len, "%s: a handle that holds one band's window carries no tracers (its exchange is sized at creation), so there is nothing to average", who); return -6; }
    if (M->ring) { m_err(errm, errm_len, "%s: bands of a frame periodic in y carry no tracers (the ring's companion frame has no q), so there is nothing to average; use a single handle", who); return -6; }
    return 0;
}

// What tells the two accumulators apart on the bands: the record, the engine's entry points, who is refused (and what the
// refusal of set, reset and download is told), the quantities at level 1 and at levels 2 and 3, the second moments, the
// arrays' outer size, and the texts.
struct MomentKind {
    beom_multi::Moments beom_multi::*rec;
    int (*set)(beom_handle, int, int, char *, int);
    int (*reset)(beom_handle);
    int (*sample)(beom_handle);
    int (*download)(beom_handle, double *, double *, double *, long long *, int *, int *, char *, int);
    int (*refused)(beom_multi *, const char *, char *, int);
    const char *refusal[3];
    int n1, n2, nsq;
    bool per_tracer;
    const char *failed, *bad_args, *no_tracer, *option, *reset_none, *none, *no_sq, *sample_failed;
};
static const MomentKind kFieldMoments{
    &beom_multi::mom, beom_set_moments, beom_reset_moments, beom_sample_moments, beom_download_moments, moments_refused,
    {"beom_multi_set_moments: a handle that holds one band's window does not keep moments yet (its global arrays are nowhere assembled); use a handle created from the global arrays",
     nullptr, "beom_multi_download_moments: this handle holds a window and keeps no moments"},
    3, 5, 5, false,
    "beom_multi_set_moments: an earlier step failed half way; destroy the handle",
    "beom_multi_set_moments: level %d, stride %d (level 0..3, stride >= 1)", nullptr,
    "beom_multi_set_moments: option refused",
    "beom_multi_reset_moments: the handle keeps no moments (beom_multi_set_moments)",
    "beom_multi_download_moments: the handle keeps no moments (beom_multi_set_moments)",
    "beom_multi_download_moments: the second moments are kept at level 3, this handle has level %d",
    "beom_sample_moments failed on band %d (step %d)"};
static const MomentKind kTracerMoments{
    &beom_multi::tmom, beom_set_tracer_moments, beom_reset_tracer_moments, beom_sample_tracer_moments, beom_download_tracer_moments,
    tracer_moments_refused,
    {"beom_multi_set_tracer_moments", "beom_multi_reset_tracer_moments", "beom_multi_download_tracer_moments"},
    2, 4, 1, true,
    "beom_multi_set_tracer_moments: an earlier step failed half way; destroy the handle",
    "beom_multi_set_tracer_moments: level %d, stride %d (level 0..3, stride >= 1)",
    "beom_multi_set_tracer_moments: the handle carries no tracer (beom_multi_set_tracers comes first)",
    "beom_multi_set_tracer_moments: option refused",
    "beom_multi_reset_tracer_moments: the handle keeps no tracer moments (beom_multi_set_tracer_moments)",
    "beom_multi_download_tracer_moments: the handle keeps no tracer moments (beom_multi_set_tracer_moments)",
    "beom_multi_download_tracer_moments: the second moment is kept at level 3, this handle has level %d",
    "beom_sample_tracer_moments failed on band %d (step %d)"};

// (the companion frame, M->mini, exists on rings only: the tracer moments, which refuse rings, never reach it)
static int multi_set_accum(beom_multi *M, const MomentKind &K, int level, int stride, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "%s", K.failed); return -30; }
    if (level < 0 || level > 3 || stride < 1) { m_err(errm, errm_len, K.bad_args, level, stride); return -3; }
    M_RC(K.refused(M, K.refusal[0], errm, errm_len));
    if (K.no_tracer && level > 0 && M->ntrc < 1) { m_err(errm, errm_len, "%s", K.no_tracer); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    for (int k = 0; k < M->n; ++k) {
        M_RC(K.set(M->eng[k], level, stride, errm, errm_len));
        // a whole frame steps through beom_step: the handle samples by itself
        if (beom_set_option(M->eng[k], "moments_by_caller", multi_whole(M) ? 0 : 1)) { m_err(errm, errm_len, "%s", K.option); return -3; }
    }
    if (M->mini) M_RC(K.set(M->mini, level, stride, errm, errm_len));
    M->*K.rec = {level, stride, 0};
    return 0;
}

static int multi_reset_accum(beom_multi *M, const MomentKind &K, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    M_RC(K.refused(M, K.refusal[1], errm, errm_len));
    if ((M->*K.rec).level < 1) { m_err(errm, errm_len, "%s", K.reset_none); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    for (int k = 0; k < M->n; ++k) M_RC(K.reset(M->eng[k]));
    if (M->mini) M_RC(K.reset(M->mini));
    (M->*K.rec).due = 0;
    return 0;
}

static int multi_download_accum(beom_multi *M, const MomentKind &K, double *ref, double *sum, double *sq, long long *count,
                                int *tstp_first, int *tstp_last, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    M_RC(K.refused(M, K.refusal[2], errm, errm_len));
    const int level = (M->*K.rec).level;
    if (level < 1) { m_err(errm, errm_len, "%s", K.none); return -3; }
    if (sq && level < 3) { m_err(errm, errm_len, K.no_sq, level); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (multi_whole(M)) return K.download(M->eng[0], ref, sum, sq, count, tstp_first, tstp_last, errm, errm_len);
    const size_t per = (size_t)(K.per_tracer ? M->ntrc : 1) * M->P.nlay, nq = level >= 2 ? K.n2 : K.n1;
    double *dst[3] = {ref, sum, sq};
    const size_t outer[3] = {nq * per, nq * per, K.nsq * per};
    for (const Part &p : parts(M)) {
        std::vector<double> a[3];
        for (int f = 0; f < 3; ++f) if (dst[f]) a[f].assign(outer[f] * p.n1(), 0.0);
        long long cnt = 0;
        int t0 = 0, t1 = 0;
        M_RC(K.download(p.eng, ptr(a[0]), ptr(a[1]), ptr(a[2]), &cnt, &t0, &t1, errm, errm_len));
        if (p.k == 0) { if (count) *count = cnt; if (tstp_first) *tstp_first = t0; if (tstp_last) *tstp_last = t1; }
        for (int f = 0; f < 3; ++f) copy_rows(dst[f], ptr(a[f]), outer[f], 1, p.out);
    }
    return 0;
}

int beom_multi_set_moments(beom_multi_handle M, int level, int stride, char *errm, int errm_len) { return multi_set_accum(M, kFieldMoments, level, stride, errm, errm_len); }
int beom_multi_set_tracer_moments(beom_multi_handle M, int level, int stride, char *errm, int errm_len) { return multi_set_accum(M, kTracerMoments, level, stride, errm, errm_len); }
int beom_multi_reset_moments(beom_multi_handle M, char *errm, int errm_len) { return multi_reset_accum(M, kFieldMoments, errm, errm_len); }
int beom_multi_reset_tracer_moments(beom_multi_handle M, char *errm, int errm_len) { return multi_reset_accum(M, kTracerMoments, errm, errm_len); }
int beom_multi_download_moments(beom_multi_handle M, double *ref, double *sum, double *sq, long long *count, int *tstp_first,
                                int *tstp_last, char *errm, int errm_len) {
    return multi_download_accum(M, kFieldMoments, ref, sum, sq, count, tstp_first, tstp_last, errm, errm_len);
}
int beom_multi_download_tracer_moments(beom_multi_handle M, double *ref, double *sum, double *sq, long long *count, int *tstp_first,
                                       int *tstp_last, char *errm, int errm_len) {
    return multi_download_accum(M, kTracerMoments, ref, sum, sq, count, tstp_first, tstp_last, errm, errm_len);
}

// ---- harmonics (beom_set_harmonics) on the bands: as the moments, every band accumulates over all its rows and keeps the
//      same normal matrix; a ring's companion frame samples behind its own steps ----
int beom_multi_set_harmonics(beom_multi_handle M, int nfreq, const double *omega, int level, int stride, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "beom_multi_set_harmonics: an earlier step failed half way; destroy the handle"); return -30; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_set_harmonics: a handle that holds one band's window does not keep harmonics (its global arrays are nowhere assembled); use a handle created from the global arrays"); return -6; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    // band 0 checks the arguments before it touches anything; the others are given what it accepted.  A band that cannot
    // allocate leaves the whole handle without harmonics
    int rc = 0;
    for (int k = 0; k < M->n && !rc; ++k) {
        rc = beom_set_harmonics(M->eng[k], nfreq, omega, level, stride, errm, errm_len);
        if (rc == -3 && k == 0) return rc;          // (refused arguments: nothing touched)
        if (!rc && beom_set_option(M->eng[k], "moments_by_caller", multi_whole(M) ? 0 : 1)) { m_err(errm, errm_len, "beom_multi_set_harmonics: option refused"); rc = -3; }
    }
    if (!rc && M->mini) rc = beom_set_harmonics(M->mini, nfreq, omega, level, stride, errm, errm_len);
    if (rc) {
        for (int k = 0; k < M->n; ++k) (void)beom_set_harmonics(M->eng[k], 0, nullptr, 0, 0, nullptr, 0);
        if (M->mini) (void)beom_set_harmonics(M->mini, 0, nullptr, 0, 0, nullptr, 0);
        M->harm = {};
        return rc;
    }
    M->harm = {};
    if (nfreq > 0) { M->harm.nfreq = nfreq; M->harm.level = level; M->harm.stride = stride; }
    return 0;
}

int beom_multi_reset_harmonics(beom_multi_handle M, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_reset_harmonics: this handle holds a window and keeps no harmonics"); return -6; }
    if (M->harm.level < 1) { m_err(errm, errm_len, "beom_multi_reset_harmonics: the handle keeps no harmonics (beom_multi_set_harmonics)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    for (int k = 0; k < M->n; ++k) M_RC(beom_reset_harmonics(M->eng[k]));
    if (M->mini) M_RC(beom_reset_harmonics(M->mini));
    M->harm.due = 0;
    return 0;
}

int beom_multi_download_harmonics(beom_multi_handle M, double *ref, double *sum, double *gram, double *omega, long long *count,
                                  int *tstp_first, int *tstp_last, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_download_harmonics: this handle holds a window and keeps no harmonics"); return -6; }
    if (M->harm.level < 1) { m_err(errm, errm_len, "beom_multi_download_harmonics: the handle keeps no harmonics (beom_multi_set_harmonics)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (multi_whole(M)) return beom_download_harmonics(M->eng[0], ref, sum, gram, omega, count, tstp_first, tstp_last, errm, errm_len);
    const size_t nf = M->harm.level >= 2 ? 5 : 3, nw = 1 + 2 * (size_t)M->harm.nfreq;
    double *dst[2] = {ref, sum};
    const size_t outer[2] = {nf * M->P.nlay, nf * nw * M->P.nlay};
    for (const Part &p : parts(M)) {
        std::vector<double> a[2];
        for (int f = 0; f < 2; ++f) if (dst[f]) a[f].assign(outer[f] * p.n1(), 0.0);
        const bool lead = p.k == 0;          // gram, omega, count and the steps are band 0's
        M_RC(beom_download_harmonics(p.eng, ptr(a[0]), ptr(a[1]), lead ? gram : nullptr, lead ? omega : nullptr, lead ? count : nullptr,
                                     lead ? tstp_first : nullptr, lead ? tstp_last : nullptr, errm, errm_len));
        for (int f = 0; f < 2; ++f) copy_rows(dst[f], ptr(a[f]), outer[f], 1, p.out);
    }
    return 0;
}

// ---- forcing in time (beom_set_forcing) on the bands: every frame is cut into the windows as beom_multi_create cuts taus
//      and hdot, the companion frame of a ring included; each band interpolates its own window at the top of its step ----
int beom_multi_set_forcing(beom_multi_handle M, int field, int nfr, const double *times, double period, const double *frames,
                           char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "beom_multi_set_forcing: an earlier step failed half way; destroy the handle"); return -30; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_set_forcing: a handle that holds one band's window does not take frames (its global arrays are nowhere assembled); use a handle created from the global arrays"); return -6; }
    const int nl = M->P.nlay;
    const Shape shape = kStatic[field == BEOM_FORCING_TAUS ? 7 : 5];
    const size_t outer = shape.outer(nl), count = outer * M->n1g;
    char msg[256] = {0};
    if (beom_forcing::check_set("beom_multi_set_forcing", field, nfr, times, period, frames, count, msg, sizeof msg)) {
        m_err(errm, errm_len, "%s", msg);
        return -3;
    }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (multi_whole(M)) return beom_set_forcing(M->eng[0], field, nfr, times, period, frames, errm, errm_len);
    int rc = 0;
    for (const Part &p : parts(M)) {
        std::vector<double> win;               // [nfr][outer][the part's slots]
        for (int k = 0; k < nfr; ++k) {
            const std::vector<double> one = cut_rows(frames + (size_t)k * count, outer, shape.inner, p.in);
            win.insert(win.end(), one.begin(), one.end());
        }
        if ((rc = beom_set_forcing(p.eng, field, nfr, times, period, ptr(win), errm, errm_len))) break;
    }
    if (rc)                                    // (an allocation failed: no band keeps the set)
        for (const Part &p : parts(M)) (void)beom_set_forcing(p.eng, field, 0, nullptr, 0.0, nullptr, nullptr, 0);
    return rc;
}

int beom_multi_download_forcing(beom_multi_handle M, double *taus, double *hdot, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_download_forcing: this handle holds a window and takes no frames"); return -6; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (multi_whole(M)) return beom_download_forcing(M->eng[0], taus, hdot, errm, errm_len);
    double *dst[2] = {taus, hdot};
    const size_t outer[2] = {kStatic[7].outer(M->P.nlay), kStatic[5].outer(M->P.nlay)};
    for (const Part &p : parts(M)) {
        std::vector<double> a[2];
        for (int f = 0; f < 2; ++f) if (dst[f]) a[f].assign(outer[f] * p.n1(), 0.0);
        M_RC(beom_download_forcing(p.eng, ptr(a[0]), ptr(a[1]), errm, errm_len));
        for (int f = 0; f < 2; ++f) copy_rows(dst[f], ptr(a[f]), outer[f], 1, p.out);
    }
    return 0;
}

// ---- output records of all bands (SURVEY §8f N2 for the multi-device handle): as beom_download_outputs /
//      beom_download_diag with GLOBAL (ndeg, nlay) real*4 records; every band forms its rows on its device.
int beom_multi_download_outputs(beom_multi_handle M, const float *h0r4, float *eta, float *u4, float *v4,
                                double *minmax, int *thin_layer, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_download_outputs: this handle holds a window"); return -3; }
    if (!h0r4) { m_err(errm, errm_len, "beom_multi_download_outputs: h_0 (real*4) is needed"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (M->nb == 1 && !M->ring) return beom_download_outputs(M->eng[0], h0r4, eta, u4, v4, minmax, thin_layer, errm, errm_len);
    const int nl = M->P.nlay;
    if (thin_layer) *thin_layer = 0;
    for (const Part &p : parts(M)) {
        const Spans in = p.in.records(), out = p.out.records();
        const size_t nloc = in.n1dst;
        const std::vector<float> h0 = cut_rows(h0r4, nl, 1, in);
        std::vector<float> e(eta ? nloc * nl : 0), a(u4 ? nloc * nl : 0), b(v4 ? nloc * nl : 0);
        std::vector<double> mm((size_t)nl * 6);
        int thin = 0;
        M_RC(beom_download_outputs(p.eng, h0.data(), ptr(e), ptr(a), ptr(b), mm.data(), &thin, errm, errm_len));
        copy_rows(eta, ptr(e), nl, 1, out);
        copy_rows(u4, ptr(a), nl, 1, out);
        copy_rows(v4, ptr(b), nl, 1, out);
        if (p.k < 0) continue;                     // the orphan row's scans are not merged
        // a band's scans cover its ghost rows too: they hold the neighbours' owned values (the exchange has landed)
        if (minmax)
            for (int q = 0; q < nl * 6; ++q)
                minmax[q] = (p.k == 0) ? mm[q] : ((q % 2 == 0) ? std::fmin(minmax[q], mm[q]) : std::fmax(minmax[q], mm[q]));
        if (thin_layer && thin > 0 && (*thin_layer == 0 || thin < *thin_layer)) *thin_layer = thin;
    }
    return 0;
}

// no_gradient_obc (private_mod.f95:2613-2679) on a frame cut into bands: the table segm(nseg, 18) of beom_set_open_boundaries
// with GLOBAL cell indices; every band gets the passes of the segments whose updated cell and source cell lie in its rows
// (owned or ghost), re-indexed to its window.  A band's step applies them after its momentum sweeps, as the single handle does
// (such steps are not split: the exchange follows the whole step).
int beom_multi_set_open_boundaries(beom_multi_handle M, int nseg, const int32_t *segm, char *errm, int errm_len) {
    if (!M || nseg < 1 || !segm) { m_err(errm, errm_len, "beom_multi_set_open_boundaries: bad arguments"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_set_open_boundaries: needs a handle created from the global arrays"); return -3; }
    if (M->land) { m_err(errm, errm_len, "beom_multi_set_open_boundaries: not for bands of a frame with land"); return -3; }
    if (M->nb == 1 && !M->ring) return beom_set_open_boundaries(M->eng[0], nseg, segm, errm, errm_len);
    // (the companion frame of a ring — rows 1..6, mm-3..mm, mm+1 — holds the orphan row's end of every segment)
    for (const Part &p : parts(M)) {
        const std::vector<int32_t> tab = obc_table(obc_window_rows(nseg, segm, p.k < 0 ? M->mini_rows : M->band[p.k].row_list(), M->P.lm + 1));
        const int nloc = (int)tab.size() / 18;
        M_RC(beom_set_open_boundaries(p.eng, nloc, nloc ? tab.data() : nullptr, errm, errm_len));
    }
    return 0;
}

// The same for a handle that holds ONE band's window (beom_multi_create_local): the caller found the segments of its own
// rows — the finder (index_boundary_points, private_mod.f95:1060-1240) looks at a cell and its four neighbours only, so a
// window's rows (ghost rows included, the row below and above them known) give exactly the global table's entries of those
// rows — with cell indices of the window.  Band 0 of a ring also passes the segments of the orphan row mm+1 (indices of a
// one-row frame); the companion frame's table is put together here from both.
int beom_multi_set_open_boundaries_local(beom_multi_handle M, int nseg, const int32_t *segm, int nseg_orphan, const int32_t *segm_orphan,
                                         char *errm, int errm_len) {
    if (!M || nseg < 0 || (nseg > 0 && !segm) || nseg_orphan < 0 || (nseg_orphan > 0 && !segm_orphan)) { m_err(errm, errm_len, "beom_multi_set_open_boundaries_local: bad arguments"); return -1; }
    if (!M->local_mode) { m_err(errm, errm_len, "beom_multi_set_open_boundaries_local: this handle was created from global arrays"); return -3; }
    M_RC(beom_set_open_boundaries(M->eng[0], nseg, nseg ? segm : nullptr, errm, errm_len));
    if (!M->mini) return 0;
    const int L = M->P.lm + 1, gs = M->band[0].gs;
    std::vector<ObcRow> rowsv;
    // window row jl (1-based) -> row of the companion frame, 0 = not there
    auto from_window = [&](int jl) { return (jl >= 1 && jl <= gs) ? kMiniLo + jl : (jl > gs && jl <= gs + kMiniLo) ? jl - gs : 0; };
    auto from_orphan = [&](int jl) { return jl == 1 ? kMiniRows : 0; };
    for (int src = 0; src < 2; ++src) {
        const int n = src ? nseg_orphan : nseg;
        const int32_t *tab = src ? segm_orphan : segm;
        for (int is = 0; is < n; ++is)
            for (int pass = 0; pass < 2; ++pass) {
                const ObcRow c = obc_columns(tab, n, is);
                const int32_t qu = c[pass == 0 ? 9 : 0], qs = c[pass == 0 ? 15 : 12];
                if (qu < 1) continue;
                const int mu = src ? from_orphan((qu - 1) / L + 1) : from_window((qu - 1) / L + 1);
                const int ms = qs > 0 ? (src ? from_orphan((qs - 1) / L + 1) : from_window((qs - 1) / L + 1)) : 0;
                if (!mu || (qs > 0 && !ms)) continue;
                rowsv.push_back(obc_pass_row(c, pass, (int32_t)((qu - 1) % L + 1 + (long long)(mu - 1) * L),
                                             qs > 0 ? (int32_t)((qs - 1) % L + 1 + (long long)(ms - 1) * L) : 0));
            }
    }
    const std::vector<int32_t> t2 = obc_table(rowsv);
    const int nloc = (int)rowsv.size();
    return beom_set_open_boundaries(M->mini, nloc, nloc ? t2.data() : nullptr, errm, errm_len);
}

int beom_multi_download_diag(beom_multi_handle M, float *pvor4, float *mont4, float *vcc4, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_download_diag: this handle holds a window"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (M->nb == 1 && !M->ring) return beom_download_diag(M->eng[0], pvor4, mont4, vcc4, errm, errm_len);
    const int nl = M->P.nlay;
    for (const Part &p : parts(M)) {
        const Spans out = p.out.records();
        const size_t nloc = out.n1src;
        std::vector<float> a(pvor4 ? nloc * nl : 0), b(mont4 ? nloc * nl : 0), c(vcc4 ? nloc * nl : 0);
        M_RC(beom_download_diag(p.eng, ptr(a), ptr(b), ptr(c), errm, errm_len));
        copy_rows(pvor4, ptr(a), nl, 1, out);
        copy_rows(mont4, ptr(b), nl, 1, out);
        copy_rows(vcc4, ptr(c), nl, 1, out);
    }
    return 0;
}

// Conservation integrals of a frame cut into bands (beom_integrals.h): a band owns whole rows, so its row sums are the
// frame's; the tree over rows (beom_integral_combine) does not care who formed them.
static int band_integral_rows(beom_multi *M, int k, double *rows, char *errm, int errm_len) {
    const Band &s = M->band[k];
    return beom_integral_rows(M->eng[k], s.gs + 1, s.nown(), rows, errm, errm_len);
}

int beom_multi_integrals(beom_multi_handle M, double *out, char *errm, int errm_len) {
    if (!M || !out) { m_err(errm, errm_len, "beom_multi_integrals: null argument"); return -1; }
    if (M->local_mode) { m_err(errm, errm_len, "beom_multi_integrals: this handle holds a window (beom_multi_integral_rows_local)"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (M->nb == 1 && !M->ring) return beom_integrals(M->eng[0], out, errm, errm_len);
    const int count = beom_integral_count(M->P.nlay), Mg = M->P.mm + 1;
    // (a ring's orphan row mm+1 duplicates row 1: every sum of it is +0, the companion frame is not asked)
    std::vector<double> rows((size_t)Mg * count, 0.0);
    for (int k = 0; k < M->n; ++k)
        M_RC(band_integral_rows(M, k, &rows[(size_t)(M->band[k].own0 - 1) * count], errm, errm_len));
    return beom_integral_combine(rows.data(), Mg, count, out);
}

int beom_multi_integral_rows_local(beom_multi_handle M, int *own0, int *own1, double *rows, char *errm, int errm_len) {
    if (!M || !rows || M->n != 1) { m_err(errm, errm_len, "beom_multi_integral_rows_local: needs a handle with one band"); return -1; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (own0) *own0 = M->band[0].own0;
    if (own1) *own1 = M->band[0].own1;
    return band_integral_rows(M, 0, rows, errm, errm_len);
}

// Series (beom_series.h) and tracer series (beom_tracer_series.h) of a frame cut into bands: a band owns whole rows, so its
// records' rows are the frame's.  What tells the two recorders apart: the record, the engine's entry points, the entries per
// row, who is refused (and what the refusal of set and download is told), the highest level, and the texts.
struct SeriesKind {
    beom_multi::Series beom_multi::*rec;
    int (*set)(beom_handle, int, int, int, char *, int);
    int (*band_set)(beom_handle, int, int, int, int, int, char *, int);
    int (*sample)(beom_handle);
    int (*download)(beom_handle, double *, int *, int *, char *, int);
    int (*count)(int ntrc, int nlay, int level);
    int (*refused)(beom_multi *, const char *, char *, int);
    const char *refusal[2];
    int max_level;
    const char *failed, *bad_args, *no_tracer, *none, *band_held, *sample_failed, *overflow;
};
static const SeriesKind kSeries{
    &beom_multi::ser, beom_set_series, beom_band_set_series, beom_sample_series, beom_download_series,
    [](int, int nlay, int level) { return beom_series_count(nlay, level); }, moments_refused,
    {"beom_multi_set_series: a handle that holds one band's window keeps no series (its rows are nowhere assembled); use a handle created from the global arrays",
     "beom_multi_download_series: this handle holds a window and keeps no series"},
    2,
    "beom_multi_set_series: an earlier step failed half way; destroy the handle",
    "beom_multi_set_series: level %d, stride %d, %d records (level 0..2, stride >= 1, records >= 1)", nullptr,
    "beom_multi_download_series: the handle keeps no series (beom_multi_set_series)",
    "beom_multi_download_series: band %d holds %d records, the handle %zu",
    "beom_sample_series failed on band %d (step %d)",
    "beom_multi_step: steps %d..%d would write %lld records of the series (stride %d) but the recorder holds %lld of %d: "
    "empty it with beom_multi_download_series, or take fewer steps per call"};
static const SeriesKind kTracerSeries{
    &beom_multi::tser, beom_set_tracer_series, beom_band_set_tracer_series, beom_sample_tracer_series, beom_download_tracer_series,
    beom_tracer_series_count, tracers_refused,
    {"beom_multi_set_tracer_series", "beom_multi_download_tracer_series"},
    3,
    "beom_multi_set_tracer_series: an earlier step failed half way; destroy the handle",
    "beom_multi_set_tracer_series: level %d, stride %d, %d records (level 0..3, stride >= 1, records >= 1)",
    "beom_multi_set_tracer_series: the handle carries no tracer (beom_multi_set_tracers comes first)",
    "beom_multi_download_tracer_series: the handle keeps no tracer series (beom_multi_set_tracer_series)",
    "beom_multi_download_tracer_series: band %d holds %d records, the handle %zu",
    "beom_sample_tracer_series failed on band %d (step %d)",
    "beom_multi_step: steps %d..%d would write %lld records of the tracer series (stride %d) but the recorder holds %lld of %d: "
    "empty it with beom_multi_download_tracer_series, or take fewer steps per call"};

static int multi_set_recorder(beom_multi *M, const SeriesKind &K, int level, int stride, int nrec, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "%s", K.failed); return -30; }
    if (level < 0 || level > K.max_level || (level > 0 && (stride < 1 || nrec < 1))) { m_err(errm, errm_len, K.bad_args, level, stride, nrec); return -3; }
    M_RC(K.refused(M, K.refusal[0], errm, errm_len));
    if (K.no_tracer && level > 0 && M->ntrc < 1) { m_err(errm, errm_len, "%s", K.no_tracer); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    beom_multi::Series &S = M->*K.rec;
    S = {};
    int rc = 0;
    for (int k = 0; k < M->n && !rc; ++k) {
        const Band &s = M->band[k];
        rc = multi_whole(M) ? K.set(M->eng[k], level, stride, nrec, errm, errm_len)
                            : K.band_set(M->eng[k], level, stride, nrec, s.gs + 1, s.nown(), errm, errm_len);
    }
    if (rc) {                           // all bands or none
        for (int k = 0; k < M->n; ++k) (void)K.set(M->eng[k], 0, 1, 1, nullptr, 0);
        return rc;
    }
    S.level = level; S.stride = stride; S.nrec = nrec;
    return 0;
}

static int multi_download_recorder(beom_multi *M, const SeriesKind &K, double *rows, int *tstp, int *count, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    M_RC(K.refused(M, K.refusal[1], errm, errm_len));
    beom_multi::Series &S = M->*K.rec;
    if (S.level < 1) { m_err(errm, errm_len, "%s", K.none); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (multi_whole(M)) return K.download(M->eng[0], rows, tstp, count, errm, errm_len);
    const size_t n = S.tstp.size(), cnt = (size_t)K.count(M->ntrc, M->P.nlay, S.level), Mg = (size_t)M->P.mm + 1;
    // (a ring's orphan row mm+1 duplicates row 1: every sum of it is +0, the companion frame is not asked)
    if (rows) std::fill(rows, rows + n * Mg * cnt, 0.0);
    for (int k = 0; k < M->n; ++k) {
        const Band &s = M->band[k];
        const size_t per = (size_t)s.nown() * cnt;
        std::vector<double> a(rows ? n * per : 0);
        int held = 0;
        M_RC(K.download(M->eng[k], rows ? ptr(a) : nullptr, nullptr, &held, errm, errm_len));
        if ((size_t)held != n) { m_err(errm, errm_len, K.band_held, s.index, held, n); return -3; }
        for (size_t r = 0; r < n && rows; ++r)
            std::copy(a.begin() + r * per, a.begin() + (r + 1) * per, rows + (r * Mg + (size_t)(s.own0 - 1)) * cnt);
    }
    if (tstp) std::copy(S.tstp.begin(), S.tstp.end(), tstp);
    if (count) *count = (int)n;
    S.tstp.clear();
    return 0;
}

int beom_multi_set_series(beom_multi_handle M, int level, int stride, int nrec, char *errm, int errm_len) {
    return multi_set_recorder(M, kSeries, level, stride, nrec, errm, errm_len);
}
int beom_multi_set_tracer_series(beom_multi_handle M, int level, int stride, int nrec, char *errm, int errm_len) {
    return multi_set_recorder(M, kTracerSeries, level, stride, nrec, errm, errm_len);
}
int beom_multi_download_series(beom_multi_handle M, double *rows, int *tstp, int *count, char *errm, int errm_len) {
    return multi_download_recorder(M, kSeries, rows, tstp, count, errm, errm_len);
}
int beom_multi_download_tracer_series(beom_multi_handle M, double *rows, int *tstp, int *count, char *errm, int errm_len) {
    return multi_download_recorder(M, kTracerSeries, rows, tstp, count, errm, errm_len);
}

// Column series (beom_column_series.h): a column's tree crosses the bands, and the same bits would need every band's canonical
// tree nodes per column and record, which nothing combines yet.  Refused on every handle on bands, whatever it was created from.
static int column_series_refused(beom_multi *M, const char *who, char *errm, int errm_len, const char *tracer = "", const char *stem = "") {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    m_err(errm, errm_len, "%s: a handle on bands keeps no %scolumn series (a column's tree over the global rows crosses the bands, "
                          "and nothing combines the bands' tree nodes yet); use a single handle (beom_set_%scolumn_series)", who, tracer, stem);
    return -6;
}
int beom_multi_set_column_series(beom_multi_handle M, int, int, int, int, int, char *errm, int errm_len) {
    return column_series_refused(M, "beom_multi_set_column_series", errm, errm_len);
}
int beom_multi_download_column_series(beom_multi_handle M, double *, int *, int *, char *errm, int errm_len) {
    return column_series_refused(M, "beom_multi_download_column_series", errm, errm_len);
}
// Tracer column series (beom_tracer_column_series.h): refused for the same reason.
int beom_multi_set_tracer_column_series(beom_multi_handle M, int, int, int, int, int, char *errm, int errm_len) {
    return column_series_refused(M, "beom_multi_set_tracer_column_series", errm, errm_len, "tracer ", "tracer_");
}
int beom_multi_download_tracer_column_series(beom_multi_handle M, double *, int *, int *, char *errm, int errm_len) {
    return column_series_refused(M, "beom_multi_download_tracer_column_series", errm, errm_len, "tracer ", "tracer_");
}

// Maps (beom_maps.h): a block's tree must not cross a seam between bands, and nothing places the seams on multiples of the
// block edge yet.  Refused on every handle on bands, whatever it was created from.
static int maps_refused(beom_multi *M, const char *who, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    m_err(errm, errm_len, "%s: a handle on bands keeps no maps (a block's tree must not cross a seam between bands, and nothing "
                          "aligns the seams to the block edge yet); use a single handle (beom_set_maps)", who);
    return -6;
}
int beom_multi_set_maps(beom_multi_handle M, int, int, int, int, char *errm, int errm_len) {
    return maps_refused(M, "beom_multi_set_maps", errm, errm_len);
}
int beom_multi_download_maps(beom_multi_handle M, double *, int *, int *, char *errm, int errm_len) {
    return maps_refused(M, "beom_multi_download_maps", errm, errm_len);
}

int beom_multi_upload_local(beom_multi_handle M, const beom_state *win, const beom_state *orphan, char *errm, int errm_len) {
    if (!M || !win) { m_err(errm, errm_len, "null argument"); return -1; }
    if (!M->local_mode) { m_err(errm, errm_len, "beom_multi_upload_local: this handle was created from global arrays"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    M_RC(beom_upload_state(M->eng[0], win->hlay, win->u, win->v, win->h_u, win->h_v, win->rs_h, win->dmdx, win->dmdy,
                           win->v_cc, win->v_ll, win->tt3d, win->tb3d, win->tu3d, errm, errm_len));
    if (M->mini) {
        if (!orphan) { m_err(errm, errm_len, "beom_multi_upload_local: band 0 of a ring needs the orphan row's state"); return -1; }
        double *wp[13], *op[13];
        state_ptrs(win, wp); state_ptrs(orphan, op);
        const Spans from_win = spans_window_to_mini(M->band[0]), from_orphan = spans_orphan_to_mini(M->P.lm + 1);
        StateV a;
        for (int f = 0; f < 13; ++f) {
            a.a[f] = cut_rows<double>(wp[f], kState[f].outer(M->P.nlay), kState[f].inner, from_win);
            copy_rows<double>(ptr(a.a[f]), op[f], kState[f].outer(M->P.nlay), kState[f].inner, from_orphan);
        }
        M_RC(upload_state_v(M->mini, a, errm, errm_len));
    }
    return 0;
}

int beom_multi_download_local(beom_multi_handle M, beom_state *win, beom_state *orphan, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null argument"); return -1; }
    if (!M->local_mode) { m_err(errm, errm_len, "beom_multi_download_local: this handle was created from global arrays"); return -3; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    if (win)
        M_RC(beom_download_state(M->eng[0], win->hlay, win->u, win->v, win->h_u, win->h_v, win->rs_h, win->dmdx, win->dmdy,
                                 win->v_cc, win->v_ll, win->tt3d, win->tb3d, win->tu3d, errm, errm_len));
    if (orphan && M->mini) {
        const int nl = M->P.nlay;
        const Spans out = spans_mini_to_orphan(M->P.lm + 1);
        double *op[13];
        state_ptrs(orphan, op);
        StateV a;
        for (int f = 0; f < 13; ++f) if (op[f]) a.a[f].assign(kState[f].outer(nl) * out.n1src * kState[f].inner, 0.0);
        M_RC(download_state_v(M->mini, a, errm, errm_len));
        for (int f = 0; f < 13; ++f) copy_rows(op[f], ptr(a.a[f]), kState[f].outer(nl), kState[f].inner, out);
    }
    return 0;
}

int beom_multi_profile_start(beom_multi_handle M) {
    if (!M) return -1;
    for (int k = 0; k < M->n; ++k) (void)beom_profile_start(M->eng[k]);
    return 0;
}
// per sweep class: the slowest local band (ms summed over its launches) and that band's launch count
int beom_multi_profile_stop(beom_multi_handle M, double *ms, int *launches, char *errm, int errm_len) {
    if (!M || !ms || !launches) { m_err(errm, errm_len, "null argument"); return -1; }
    M_RC(beom_multi_sync(M, errm, errm_len));
    for (int c = 0; c < 8; ++c) { ms[c] = 0.0; launches[c] = 0; }
    for (int k = 0; k < M->n; ++k) {
        double m[8] = {0}; int l[8] = {0};
        M_RC(beom_profile_stop(M->eng[k], m, l, errm, errm_len));
        for (int c = 0; c < 8; ++c) if (m[c] > ms[c]) { ms[c] = m[c]; launches[c] = l[c]; }
    }
    return 0;
}

}  // extern "C"

// ---- one time step of all local bands -------------------------------------------------------------
// Boundary first (beom_step_phase): a band's main stream runs the step up to the momentum sweeps on all rows, then the
// momentum sweep on the rows in between; its second stream, behind the first part, runs the momentum sweep on the strips
// next to the ghost zones, packs the outermost owned rows, moves them, unpacks what the neighbours sent.  The main stream
// looks at the second one exactly once per step — "have my ghost rows landed?" before the next step starts — and by then
// the exchange has had the whole interior sweep to finish.  Steps that cannot be cut that way (open-boundary passes, the
// separate u and v sweeps, option "overlap" = 0) run whole, the exchange after them.
// the moments' sample a step left owing, on every band's main stream (which has joined the exchange of that step)
static int multi_sample_due(beom_multi *M, char *errm, int errm_len) {
    for (const MomentKind *K : {&kFieldMoments, &kTracerMoments}) {
        int &due = (M->*K->rec).due;
        for (int k = 0; k < M->n && due; ++k)
            if (K->sample(M->eng[k])) { m_err(errm, errm_len, K->sample_failed, M->band[k].index, due); return -3; }
        due = 0;
    }
    if (M->harm.due) {
        for (int k = 0; k < M->n; ++k)
            if (beom_sample_harmonics(M->eng[k], M->harm.due_ctim)) { m_err(errm, errm_len, "beom_sample_harmonics failed on band %d (step %d)", M->band[k].index, M->harm.due); return -3; }
        M->harm.due = 0;
    }
    for (const SeriesKind *K : {&kSeries, &kTracerSeries}) {
        beom_multi::Series &S = M->*K->rec;
        if (!S.due) continue;
        for (int k = 0; k < M->n; ++k)
            if (K->sample(M->eng[k])) { m_err(errm, errm_len, K->sample_failed, M->band[k].index, S.due); return -3; }
        S.tstp.push_back(S.due);
        S.due = 0;
    }
    return 0;
}

static int multi_one_step(beom_multi *M, int t, double tres, double dtd8, double dt_r, double rsta, int n_3d,
                          char *errm, int errm_len) {
    const int n = M->n;
    const int mk = M->mini_k;
    if (M->shm && M->shm->failed) { m_err(errm, errm_len, "beom_multi: a neighbour's ghost rows did not arrive within %.0f s (shared-memory transport)", M->shm->timeout_s); return -35; }
    // the ghost rows of the previous step have landed: before this step reads them
    for (int k = 0; k < n; ++k) {
        if (!M->pending[k]) continue;
        M_HIP(hipSetDevice(M->dev[k]));
        M_HIP(hipStreamWaitEvent(M->main_s[k], M->landed[k], 0));
    }
    M_RC(multi_sample_due(M, errm, errm_len));          // the sample of the step before: its strips and ghost rows are in place
    if (M->flt_mode) M_RC(multi_float_launch(M, M->flt_mode, errm, errm_len));      // the floats likewise, in front of anything that writes u, v
    // companion frame of a ring: rows 1..6 of band 0 and its south ghosts (= rows mm-3..mm) as they stand before this
    // step, then the companion's own step on its own stream
    if (M->mini) {
        M_HIP(hipSetDevice(M->dev[mk]));
        if (M->free_recorded) M_HIP(hipStreamWaitEvent(M->main_s[mk], M->ev_free, 0));      // (the companion has taken the copies of the step before)
        if (beom_pack_rows(M->eng[mk], M->band[mk].gs + 1, kMiniLo, M->mini_lo) || beom_pack_rows(M->eng[mk], 1, kGhost, M->mini_hi)) {
            m_err(errm, errm_len, "beom_pack_rows failed"); return -3;
        }
        M_HIP(hipEventRecord(M->ev_hi, M->main_s[mk]));
        M_HIP(hipStreamWaitEvent(M->mini_s, M->ev_hi, 0));
        if (beom_unpack_rows(M->mini, 1, kMiniLo, M->mini_lo) || beom_unpack_rows(M->mini, kMiniLo + 1, kGhost, M->mini_hi)) {
            m_err(errm, errm_len, "beom_unpack_rows failed"); return -3;
        }
        M_HIP(hipEventRecord(M->ev_free, M->mini_s));
        M->free_recorded = true;
        M_RC(beom_step(M->mini, t, 1, tres, dtd8, dt_r, rsta, n_3d, errm, errm_len));
    }
    // the step; a band's packing stream X is its second stream when the step is cut, else its main stream
    std::vector<hipStream_t> X(n, nullptr);
    for (int k = 0; k < n; ++k) {
        const Band &s = M->band[k];
        M_HIP(hipSetDevice(M->dev[k]));
        struct Back { beom_multi *M; int k; ~Back() { (void)beom_set_stream(M->eng[k], (void *)M->main_s[k], 0); } } back{M, k};
        int rc = M->overlap ? beom_step_phase(M->eng[k], t, tres, dtd8, dt_r, rsta, n_3d, 1, errm, errm_len) : -20;
        if (rc == 0) {
            M_HIP(hipEventRecord(M->p1done[k], M->main_s[k]));
            M_HIP(hipStreamWaitEvent(M->comm_s[k], M->p1done[k], 0));
            (void)beom_set_stream(M->eng[k], (void *)M->comm_s[k], 0);
            M_RC(beom_step_phase(M->eng[k], t, tres, dtd8, dt_r, rsta, n_3d, 2, errm, errm_len));
            (void)beom_set_stream(M->eng[k], (void *)M->main_s[k], 0);
            M_RC(beom_step_phase(M->eng[k], t, tres, dtd8, dt_r, rsta, n_3d, 3, errm, errm_len));
            X[k] = M->comm_s[k];
            ++M->n_split;
        } else if (rc == -20) {
            M_RC(beom_step(M->eng[k], t, 1, tres, dtd8, dt_r, rsta, n_3d, errm, errm_len));
            // peer copies read a neighbour's send buffer from ITS stream: keep the exchange of a whole step on the second
            // stream there; RCCL and the shared-memory transport order everything themselves: no stream hop at all
            X[k] = M->transport == BEOM_XCHG_PEER ? M->comm_s[k] : M->main_s[k];
            if (X[k] != M->main_s[k]) {
                M_HIP(hipEventRecord(M->p1done[k], M->main_s[k]));
                M_HIP(hipStreamWaitEvent(X[k], M->p1done[k], 0));
            }
            ++M->n_plain;
        } else return rc;
        // what the neighbours need = my outermost OWNED rows.  With peer copies my neighbours still read the send buffers
        // of the step before until THEIR ghosts have landed.
        if (M->transport == BEOM_XCHG_PEER)
            for (int q : {M->south_of(k), M->north_of(k)}) {
                const int ql = M->local_of(q);
                if (ql >= 0 && ql != k && M->pending[ql]) M_HIP(hipStreamWaitEvent(X[k], M->landed[ql], 0));
            }
        (void)beom_set_stream(M->eng[k], (void *)X[k], 0);
        if (M->has_s(k) && M->has_n(k)) {
            if (beom_pack_rows2(M->eng[k], kGhost, s.gs + 1, M->send_s[k], s.gs + s.nown() - kGhost + 1, M->send_n[k])) { m_err(errm, errm_len, "beom_pack_rows2 failed"); return -3; }
        } else {
            if (M->has_s(k) && beom_pack_rows(M->eng[k], s.gs + 1, kGhost, M->send_s[k])) { m_err(errm, errm_len, "beom_pack_rows failed"); return -3; }
            if (M->has_n(k) && beom_pack_rows(M->eng[k], s.gs + s.nown() - kGhost + 1, kGhost, M->send_n[k])) { m_err(errm, errm_len, "beom_pack_rows failed"); return -3; }
        }
        M_HIP(hipEventRecord(M->packed[k], X[k]));
    }
    for (int k = 0; k < n; ++k) M->pending[k] = 0;
    // the exchange, in the packing stream's order
    if (M->transport == BEOM_XCHG_RCCL) {
        // sends in the order (south, north), receives in the order (north, south): with two bands in a ring, or
        // one, both neighbours are the same peer and RCCL matches a pair's messages in issue order
        M_NCCL(g_rccl.GroupStart());
        int e = 0;                                  // (a failed call must not leave the process-wide group open)
        for (int k = 0; k < n && !e; ++k) {
            if (hipSetDevice(M->dev[k]) != hipSuccess) { e = 1; break; }
            const int S = M->rank_of(M->south_of(k)), N = M->rank_of(M->north_of(k));
            if (!e && M->has_s(k)) e = g_rccl.Send(M->send_s[k], M->xbytes, kNcclChar, S, M->comm[k], X[k]);
            if (!e && M->has_n(k)) e = g_rccl.Send(M->send_n[k], M->xbytes, kNcclChar, N, M->comm[k], X[k]);
            if (!e && M->has_n(k)) e = g_rccl.Recv(M->recv_n[k], M->xbytes, kNcclChar, N, M->comm[k], X[k]);
            if (!e && M->has_s(k)) e = g_rccl.Recv(M->recv_s[k], M->xbytes, kNcclChar, S, M->comm[k], X[k]);
        }
        const int ge = g_rccl.GroupEnd();
        if (e || ge) { m_err(errm, errm_len, "RCCL ghost exchange failed: %s", g_rccl.GetErrorString(e ? e : ge)); return -300 - (e ? e : ge); }
    } else if (M->transport == BEOM_XCHG_SHM) {
        // the same place in the same stream order as the grouped send/recv above (see ShmXchg)
        ShmXchg *x = M->shm;
        const int k = 0;
        const uint64_t sq = ++x->seq;
        const int me = M->band[k].index;
        M_HIP(hipSetDevice(M->dev[k]));
        if (M->has_s(k)) M_HIP(hipMemcpyAsync(x->slot(me, 0, sq), M->send_s[k], M->xbytes, hipMemcpyDeviceToHost, X[k]));
        if (M->has_n(k)) M_HIP(hipMemcpyAsync(x->slot(me, 1, sq), M->send_n[k], M->xbytes, hipMemcpyDeviceToHost, X[k]));
        M_HIP(hipLaunchHostFunc(X[k], shm_publish, new ShmOp{x, me, sq}));
        if (M->has_n(k)) {          // what my north neighbour sent south (looped back: what I sent myself)
            const int q = M->north_of(k), dir = M->loopback ? (M->has_s(k) ? 0 : 1) : 0;
            M_HIP(hipLaunchHostFunc(X[k], shm_wait, new ShmOp{x, q, sq}));
            M_HIP(hipMemcpyAsync(M->recv_n[k], x->slot(q, dir, sq), M->xbytes, hipMemcpyHostToDevice, X[k]));
        }
        if (M->has_s(k)) {
            const int q = M->south_of(k), dir = M->loopback ? (M->has_n(k) ? 1 : 0) : 1;
            M_HIP(hipLaunchHostFunc(X[k], shm_wait, new ShmOp{x, q, sq}));
            M_HIP(hipMemcpyAsync(M->recv_s[k], x->slot(q, dir, sq), M->xbytes, hipMemcpyHostToDevice, X[k]));
        }
    }
    for (int k = 0; k < n; ++k) {
        const Band &s = M->band[k];
        M_HIP(hipSetDevice(M->dev[k]));
        struct Restore { beom_multi *M; int k; ~Restore() { (void)beom_set_stream(M->eng[k], (void *)M->main_s[k], 0); } } restore{M, k};
        (void)beom_set_stream(M->eng[k], (void *)X[k], 0);
        if (M->has_s(k)) {
            if (M->transport == BEOM_XCHG_PEER) {
                const int q = M->local_of(M->south_of(k));
                if (q != k) M_HIP(hipStreamWaitEvent(X[k], M->packed[q], 0));
                M_HIP(hipMemcpyPeerAsync(M->recv_s[k], M->dev[k], M->send_n[q], M->dev[q], M->xbytes, X[k]));
            }
            if (!M->has_n(k) && beom_unpack_rows(M->eng[k], 1, kGhost, M->recv_s[k])) { m_err(errm, errm_len, "beom_unpack_rows failed"); return -3; }
        }
        if (M->has_n(k)) {
            if (M->transport == BEOM_XCHG_PEER) {
                const int q = M->local_of(M->north_of(k));
                if (q != k) M_HIP(hipStreamWaitEvent(X[k], M->packed[q], 0));
                M_HIP(hipMemcpyPeerAsync(M->recv_n[k], M->dev[k], M->send_s[q], M->dev[q], M->xbytes, X[k]));
            }
            if (!M->has_s(k) && beom_unpack_rows(M->eng[k], s.gs + s.nown() + 1, kGhost, M->recv_n[k])) { m_err(errm, errm_len, "beom_unpack_rows failed"); return -3; }
        }
        if (M->has_s(k) && M->has_n(k) && beom_unpack_rows2(M->eng[k], kGhost, 1, M->recv_s[k], s.gs + s.nown() + 1, M->recv_n[k])) {
            m_err(errm, errm_len, "beom_unpack_rows2 failed"); return -3;       // both sides in one launch, behind both transfers
        }
        if (X[k] != M->main_s[k] || M->transport == BEOM_XCHG_PEER) {
            M_HIP(hipEventRecord(M->landed[k], X[k]));
            M->pending[k] = 1;
        }
    }
    for (beom_multi::Moments *m : {&M->mom, &M->tmom})
        if (m->level > 0 && t % m->stride == 0) m->due = t;
    if (M->harm.level > 0 && t % M->harm.stride == 0) { M->harm.due = t; M->harm.due_ctim = tres + dtd8 * (double)t; }
    for (beom_multi::Series *s : {&M->ser, &M->tser})
        if (s->level > 0 && t % s->stride == 0) s->due = t;
    if (M->nflt > 0) M->flt_mode = 3;
    return 0;
}

extern "C" {

int beom_multi_step(beom_multi_handle M, int tstp_first, int nsteps, double tres, double dtd8, double dt_r,
                    double rsta, int n_3d, char *errm, int errm_len) {
    if (!M) { m_err(errm, errm_len, "null handle"); return -1; }
    if (M->failed) { m_err(errm, errm_len, "beom_multi_step: an earlier step failed half way; destroy the handle"); return -30; }
    if (tstp_first < 1 || nsteps < 0 || n_3d < 1) { m_err(errm, errm_len, "beom_multi_step: bad arguments"); return -3; }
    if (M->nb == 1 && !M->ring) return beom_step(M->eng[0], tstp_first, nsteps, tres, dtd8, dt_r, rsta, n_3d, errm, errm_len);
    if (M->nflt > 0 && !M->flt_ready) { m_err(errm, errm_len, "beom_multi_step: the handle's %lld floats have no positions yet (beom_multi_upload_floats)", M->nflt); return -3; }
    for (const SeriesKind *K : {&kSeries, &kTracerSeries}) {      // a recorder must hold every record of the call: refused before anything is launched
        const beom_multi::Series &S = M->*K->rec;
        if (S.level > 0 && !beom_recorder::holds(tstp_first, nsteps, S.stride, S.tstp.size(), S.nrec, errm, errm_len, K->overflow)) return -3;
    }
    M->flt_mode = (M->nflt > 0 && nsteps > 0) ? 1 : 0;          // stage 1 alone in front of the call's first step
    for (int t = tstp_first; t < tstp_first + nsteps; ++t) {
        const int rc = multi_one_step(M, t, tres, dtd8, dt_r, rsta, n_3d, errm, errm_len);
        if (rc) {       // streams and events are in an unknown order: refuse further steps, keep destroy safe
            M->failed = true;
            for (int k = 0; k < M->n; ++k) { (void)beom_set_stream(M->eng[k], (void *)M->main_s[k], 0); M->pending[k] = 0; }
            M->flt_mode = 0;
            return rc;
        }
    }
    if (M->mom.due || M->tmom.due || M->harm.due || M->ser.due || M->tser.due || M->flt_mode) {       // the last step's sample and stage 2: behind the same wait the next step would begin with
        M_RC(multi_join_exchange(M, errm, errm_len));
        M_RC(multi_sample_due(M, errm, errm_len));
        if (M->flt_mode) {
            M->flt_mode = 0;
            M_RC(multi_float_launch(M, 2, errm, errm_len));
        }
    }
    return 0;
}

}  // extern "C"
