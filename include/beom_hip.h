/*
 * beom_hip.h — C-ABI of the MI355X-native BEOM time-step engine (libbeom_hip.so).
 *
 * The reference (zhazorken/beom) has no plugin/FFI interface: `program main` calls
 * `run()` (main.f95:34) and the five hot routines communicate through module-global
 * arrays (private_mod.f95:27-93).  The cut is therefore made one level above the hot
 * routines, at the time step.  Each entry point below names the
 * reference code it replaces.  Every array argument is a plain host pointer with the
 * exact Fortran storage of the corresponding module array, index 0 (land sentinel)
 * included:
 *
 *   X(0:ndeg, nlay)        -> x[ipnt + (ndeg+1)*(ilay-1)]
 *   neig(8, 0:ndeg)        -> neig[(k-1) + 8*ipnt]           default integer (4 B)
 *   rs_h(2, 0:ndeg, nlay)  -> rs_h[(m-1) + 2*(ipnt + (ndeg+1)*(ilay-1))]
 *   dmdx(3, 0:ndeg, nlay)  -> dmdx[(m-1) + 3*(ipnt + (ndeg+1)*(ilay-1))]
 *   fnud(0:ndeg, nlay, 3)  -> fnud[ipnt + (ndeg+1)*((ilay-1) + nlay*(ivar-1))]
 *   nudg(0:ndeg, 3)        -> nudg[ipnt + (ndeg+1)*(ivar-1)]
 *   tide(2, 1, 0:ndeg, 3)  -> tide[(m-1) + 2*(ipnt + (ndeg+1)*(ivar-1))]
 *   tt3d(0:ndeg, 2, nlay)  -> tt3d[ipnt + (ndeg+1)*((idir-1) + 2*(ilay-1))]
 *   bodf(nlay, 2)          -> bodf[(ilay-1) + nlay*(idir-1)]
 *   taus(0:ndeg, 2)        -> taus[ipnt + (ndeg+1)*(idir-1)]
 *
 * Ownership: the caller owns every host array; the library copies at create/upload and
 * never keeps a host pointer.  Device memory belongs to the handle.
 * Errors: every function returns 0 on success and a negative code on failure, and
 * writes a NUL-terminated message into errm (capacity errm_len; may be NULL) — the
 * errc/errm convention of shared_mod.f95:113-157.  There is NO CPU fallback: without a
 * usable HIP device beom_create fails.
 * Threading: one host thread per handle, never from inside an OpenMP region
 * (the reference calls the hot routines from the master thread, private_mod.f95:1867-1906).
 */
#ifndef BEOM_HIP_H
#define BEOM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEOM_MAX_LAYERS 16
#define BEOM_ABI_VERSION 2
#define BEOM_MAX_TRACERS 8

/* Constants of shared_mod.f95:41-99, passed BY VALUE from the host so that the
 * single-precision literals widened to double (grav = 9.8, beta = 0.281105, ...) keep
 * the host compiler's bits.  Fortran side: type, bind(C) :: beom_params. */
typedef struct beom_params {
    int32_t abi_version;        /* BEOM_ABI_VERSION                                  */
    int32_t lm, mm, nlay, ndeg; /* shared_mod.f95:41-45                              */
    int32_t nsal;               /* shared_mod.f95:105 Salmon exponent (4)            */
    int32_t variant;            /* 0: update_h of private_mod.f95:1593-1702;
                                   1: epilogue of private_mod3d.f95:1635-1683        */
    int32_t flag_nudging;       /* private_mod.f95:93,868-871                        */
    int32_t dense_hint;         /* 1: let the library verify neig against the dense
                                   closed form and use the fast path */
    int32_t slab_row0;          /* j-slab of a larger frame (multi-GPU): the
                                   handle's row 1 is global row slab_row0 + 1 ...        */
    int32_t slab_mm;            /* ... of a frame with this many rows (global mm);
                                   0 = the handle holds the whole frame                  */
    double dl, dt;              /* shared_mod.f95:47,84                              */
    double grav, rho0;          /* :89-90                                            */
    double beta, epsi, gamm, del1, del2; /* :91-95                                   */
    double hmin, hsal;          /* :59,85                                            */
    double bvis, dvis, svis;    /* :56-57 (+fork's svis)                             */
    double bdrg, tdrg, qdrg;    /* :58,65 (+fork's tdrg)                             */
    double hsbl, hbbl;          /* :60-61                                            */
    double g_fb, uadv, ocrp, rgld, mcbc; /* :63-72                                   */
    double invf;                /* private_mod.f95:223-229                           */
    double w_ti;                /* private_mod.f95:85,953  tidal frequency (rad/day) */
    double rhon[BEOM_MAX_LAYERS]; /* shared_mod.f95:50                               */
} beom_params;

typedef struct beom_engine *beom_handle;

/* Version/ABI probe (no GPU needed). */
int beom_abi_version(void);
/* sha1 prefix of the sources the library was built from (Makefile); bindings compare it with the tree. */
const char *beom_source_hash(void);
/* Number of visible HIP devices, or a negative error code. */
int beom_device_count(char *errm, int errm_len);
/* PCI address "dddd:bb:dd.f" of a HIP device (to find its sysfs node for clock / power read-outs). */
int beom_device_pci_bus_id(int device, char *out, int out_len);

/* Replaces the static part of the module state built by read_input_data
 * (private_mod.f95:105-250): connectivity (index_grid_points :567-764), masks,
 * Coriolis, depth, and the optional forcings of read_input_file (:766-967).
 * hdot, tide, bodf, taus, h_to may be NULL (= all zero, i.e. file absent). */
int beom_create(const beom_params *prm, int device,
                const int32_t *neig, const int32_t *subc,
                const double *mk_u, const double *mk_v, const double *mk_n,
                const double *mkpe, const double *mkpi,
                const double *fcor, const double *h_th, const double *h_to,
                const double *nudg, const double *fnud, const double *hdot,
                const double *tide, const double *bodf, const double *taus,
                beom_handle *out, char *errm, int errm_len);

int beom_destroy(beom_handle h);

/* Replaces the product of index_boundary_points (private_mod.f95:1060-1240): segm(nseg, 18),
 * Fortran storage segm[(iseg-1) + nseg*(col-1)], default integers.  With flag_nudging and
 * mcbc < 0.5 the engine then applies no_gradient_obc (:2613-2679) after the momentum sweeps of
 * every step (:2201-2204, 2285-2288); beom_step refuses such a configuration until this call
 * has been made.  nseg = 0 (segm NULL) declares that the handle holds no segment; a pass of a segment whose updated cell
 * (column 10 for the first pass, 1 for the second) is -1 is skipped — both are what beom_multi_set_open_boundaries gives
 * the bands of a frame. */
int beom_set_open_boundaries(beom_handle h, int nseg, const int32_t *segm, char *errm, int errm_len);

/* Prognostic + history state, host -> device.  Any pointer may be NULL (left as is;
 * a fresh handle holds the values of initialize_variables, private_mod.f95:252-307). */
int beom_upload_state(beom_handle h,
                      const double *hlay, const double *u, const double *v,
                      const double *h_u, const double *h_v,
                      const double *rs_h, const double *dmdx, const double *dmdy,
                      const double *v_cc, const double *v_ll,
                      const double *tt3d, const double *tb3d, const double *tu3d,
                      char *errm, int errm_len);

/* Device -> host; any pointer may be NULL.  Needed before write_outputs
 * (private_mod.f95:1908-1910) and for restart/parity checks. */
int beom_download_state(beom_handle h,
                        double *hlay, double *u, double *v, double *h_u, double *h_v,
                        double *rs_h, double *dmdx, double *dmdy,
                        double *v_cc, double *v_ll,
                        double *tt3d, double *tb3d, double *tu3d,
                        char *errm, int errm_len);

/* Output preparation on the device: replaces the array work of write_array for 'eta_', 'u___',
 * 'v___' (private_mod.f95:2848-2883; eta = interface elevation accumulated bottom-up in real*4)
 * and the scans of write_outputs (:2772-2808).  h0r4 = the (ndeg, nlay) real*4 content of
 * h_0.bin (needed on the first call, may be NULL afterwards); eta/u4/v4 = (ndeg, nlay) real*4
 * host records (any may be NULL); minmax[nlay][6] = min/max of h over wet cells, of u and of v
 * over their points (over all cells 0..ndeg if a mask is empty, :2776-2793); *thin_layer = first
 * layer with a wet cell thinner than 0.5*hmin, or 0 (:2798-2808). */
int beom_download_outputs(beom_handle h, const float *h0r4, float *eta, float *u4, float *v4,
                          double *minmax, int *thin_layer, char *errm, int errm_len);

/* The `diag` records of write_array (private_mod.f95:2884-2974), formed on the device from the state: 'pvor', 'mont'
 * (without the kinetic part, real*4 accumulation as in the reference) and 'v_cc' (Leith viscosity diagnosed from u, v) —
 * each (ndeg, nlay) real*4, any pointer may be NULL.  Call between time steps (uses the step's scratch arrays). */
int beom_download_diag(beom_handle h, float *pvor, float *mont, float *v_cc, char *errm, int errm_len);

/* Rigid lid (rgld = 1; the fork's addition, private_mod.f95:64-67, 91, 505-563, 1648-1700, 1705-1838, 2207-2221,
 * 2237-2257, 2292-2314).  A handle created with prm->rgld = 1 (needs variant 0, ocrp = 1 — the reference only
 * initialises the operators then — and a whole frame) steps as the reference does: transports rebuilt before update_h
 * and after the momentum sweeps, the column-misfit epilogue of update_h, then surf_pressure — the Poisson right-hand
 * side, Gauss-Seidel sweeps in packed order until max|change| <= 1e-5 or 1000 sweeps (on the device as wavefronts over
 * the anti-diagonals, same arithmetic), and the velocity correction.  beom_set_rigid_lid uploads the module arrays
 * Ow, Os, Osum_ (0:ndeg) (first call: required) and the lid pressure pi_s(0:ndeg) (NULL: keep; zero after create);
 * beom_step refuses (-6) until it has been called.  beom_download_pressure returns pi_s; beom_download_outputs puts
 * real(pi_s) into the top 'eta_' record as write_array does (:2864-2872). */
int beom_set_rigid_lid(beom_handle h, const double *Ow, const double *Os, const double *Osum_, const double *pi_s,
                       char *errm, int errm_len);
int beom_download_pressure(beom_handle h, double *pi_s, char *errm, int errm_len);

/* The six per-layer diagnostics of update_mont_rvor_pvor_dive_kine, which the library
 * keeps per layer: each is (0:ndeg, nlay).  (The reference keeps (0:ndeg) and reuses it
 * layer after layer, private_mod.f95:48-61.) */
int beom_download_scratch(beom_handle h,
                          double *mont, double *rvor, double *pvor, double *dive,
                          double *d2hx, double *d2hy, char *errm, int errm_len);

/* Replaces the body of integrate_time (private_mod.f95:1853-1912) for time steps
 * tstp_first .. tstp_first+nsteps-1: ctim (:1862,1887), ramp (:1864-1866,1898-1901),
 * gene (:1859,1877), distribute_stress cadence (:1863,1889-1896), and per step
 * first_three_timesteps (:2151-2223) for tstp <= 3 or gener_forward_backward
 * (:2225-2316) afterwards.  Asynchronous on the handle's stream; beom_sync to wait. */
int beom_step(beom_handle h, int tstp_first, int nsteps,
              double tres, double dtd8, double dt_r, double rsta, int n_3d,
              char *errm, int errm_len);

int beom_sync(beom_handle h, char *errm, int errm_len);

/* Multi-GPU j-slabs (no reference counterpart — the reference is OpenMP only).
 * One time step of a band (a handle with slab_mm != 0) in three parts, "boundary first", so that the rows its neighbours
 * wait for are finished, packed and on their way while the bulk of the momentum sweep still runs:
 *   phase 1 = the step up to the momentum sweeps on all rows (stress, the transports of steps 1-3, update_h,
 *             update_mont..., update_viscosity);
 *   phase 2 = update_u/update_v (the fused sweep) on the strips next to the ghost zones: rows 1..8 and M-7..M — call it
 *             with ANOTHER stream set (beom_set_stream) that waits for phase 1, and follow it there with
 *             beom_pack_rows -> transport -> beom_unpack_rows;
 *   phase 3 = the same sweep on the rows in between, on the usual stream, then the pointer rotations (call it last).
 * All three see ghost rows that have landed; the next step may start once this step's unpack has run.
 * -20 (from phase 1) = this step cannot be cut that way (separate u and v sweeps, open-boundary passes, rigid lid, fewer
 * than 32 rows): use beom_step. */
int beom_step_phase(beom_handle h, int tstp, double tres, double dtd8, double dt_r, double rsta,
                    int n_3d, int phase, char *errm, int errm_len);
/* Rows [jlo, jlo+nrows) (local, 1-based) of hlay,u,v,h_u,h_v <-> one contiguous DEVICE buffer
 * of 5*nlay*nrows*(lm+1) doubles ([field][layer][row][column]); one launch each, on the
 * handle's stream.  A handle that carries ntrc tracers (beom_set_tracers) moves their contents too: the buffer then holds
 * (5 + ntrc)*nlay*nrows*(lm+1) doubles, q behind the five fields as [tracer][layer][row][column]. */
int beom_pack_rows(beom_handle h, int jlo, int nrows, void *device_buffer);
int beom_unpack_rows(beom_handle h, int jlo, int nrows, const void *device_buffer);
/* two groups of nrows rows (a band's south and north side) <-> two buffers in ONE launch */
int beom_pack_rows2(beom_handle h, int nrows, int jlo_a, void *buffer_a, int jlo_b, void *buffer_b);
int beom_unpack_rows2(beom_handle h, int nrows, int jlo_a, const void *buffer_a, int jlo_b, const void *buffer_b);

/* Options (dense frames only; results are bit-identical either way):
 *  "fuse_mont_visc" (default 1): with the Leith viscosity refreshed every step (dvis > 1e-3,
 *      n_3d = 1) update_mont... and update_viscosity run as ONE sweep that hands update_u/v
 *      the products v_cc*dive and v_ll*rvor; v_cc, v_ll, rvor, dive are then kept up to date
 *      only with "keep_diag" = 1 (default 0).  With dvis <= 1e-3 (and svis = 0) the same sweep,
 *      from step 4 on, forms the products of the standing v_cc, v_ll instead (rvor, dive again
 *      only with "keep_diag"); with n_3d > 1 the refresh steps also store v_cc, v_ll and the
 *      steps in between use that standing-viscosity form.
 *  "lean_d2h", "lean_visc" (default 1): the fused pair re-derives d2hx, d2hy in the momentum sweep,
 *      and drops the viscous products altogether when v_cc = v_ll = +0 and never refreshed.
 *  "fuse_uv" (default 1): update_u and update_v of a step run as ONE sweep.
 *  "fuse": sets both.  0 = always five separate sweeps.
 *  "profile_stride" (default 1): beom_profile_start brackets only the steps with tstp % stride == 0 with HIP events
 *      (an event pair between two launches costs a few microseconds of pipeline bubble: sampled, the timed region is
 *      hardly disturbed; the launch counts beom_profile_stop returns are those of the sampled steps).
 *  "profile_rotate" (default 0): a sampled step brackets only ONE kind of sweep — update_h | update_mont, update_viscosity |
 *      update_u, update_v — by turns ((tstp / stride) % 3 = 0 | 1 | 2), so that no bracketed launch starts behind another
 *      bracket's bubble; the launch counts are then those of the steps that bracketed that kind.
 *  "fold_stress" (default 1): with constant layer fractions (ocrp = 0) and a stress refresh on every step (n_3d = 1), steps
 *      after the third form distribute_stress (private_mod.f95:1921-2149) inside the fused update_u/update_v sweep: no
 *      launch of its own, tt3d/tb3d/tu3d neither written nor read (they keep their values of step 1 unless "keep_diag" = 1).
 *  "plain_sweeps" (default 1): a launch of the fused update_u/update_v sweep whose handle has no nudging, tide, stress, body
 *      force, lid or svis, and a launch of the fused Montgomery sweep with ocrp = 0, no lid, no h_to and "keep_diag" = 0, take
 *      the instantiations with those branches compiled out (same statements, same results).  0 = the general ones.
 * Returns -3 for an unknown name. */
int beom_set_option(beom_handle h, const char *name, int value);
/* Introspection (>= 0, or -3 for an unknown name): "stress_folded" = the last step formed its stress inside the momentum
 * sweep (1) or through distribute_stress' own launch and the three arrays (0); "tile_rows" = rows of a tile of the tiled
 * sweeps (8 | 4; 0 on the table path); "biharm_tiled" = the biharmonic part of this handle's update_viscosity (svis > 0,
 * private_mod.f95:2508-2599) runs as the tiled sweep k_biharm_tiled (1: every dense or embedded handle with svis > 0) or
 * not (0: the table kernels of a packed handle, and every handle with svis = 0); "uv_fused" = the last step's update_u and
 * update_v ran as the fused sweep (1) or as two sweeps (0; 0 before the first step); "plain_sweeps" = which sweeps of the
 * last step ran their plain form: bit 0 (1) the fused update_u/update_v sweep, bit 1 (2) the fused Montgomery sweep;
 * "vel_targets_zero" = the velocity targets fnud(0:ndeg, nlay, ix_u | ix_v) given to beom_create are +0 bit for bit in every
 * slot (1: update_u / update_v never fetch the target of a point whose new velocity is an exact zero) or not (0). */
int beom_info(beom_handle h, const char *what);

/* Run all launches of this handle on the caller's HIP stream (e.g. the stream a
 * ghost-row exchange is enqueued on).  hip_stream may be NULL = the default stream;
 * use_own != 0 restores the handle's own stream. */
int beom_set_stream(beom_handle h, void *hip_stream, int use_own);

/* Per-sweep entry points with the reference routines' meaning; used by parity tests.
 * ilay is 1-based as in Fortran; ilay = 0 means "all layers" (one batched launch).
 * The per-step scalars gene/ramp/ctim are module variables in the reference
 * (private_mod.f95:70-73) and are passed explicitly here. */
int beom_update_h(beom_handle h, double gene, double ramp, double ctim);          /* :1593 */
int beom_update_mont_rvor_pvor_dive_kine(beom_handle h, int ilay);               /* :2318 */
int beom_update_viscosity(beom_handle h, int ilay);                              /* :2441 */
int beom_update_u(beom_handle h, int ilay, double gene, double ramp, double ctim); /* :1422 */
int beom_update_v(beom_handle h, int ilay, double gene, double ramp, double ctim); /* :1505 */
int beom_rebuild_fluxes(beom_handle h);                                          /* :2166-2177 */
int beom_distribute_stress(beom_handle h);                                       /* :1921 */

/* Introspection for measurement and zero-copy interop. */
/* name in {hlay,u,v,h_u,h_v}: device pointer + layout of the library's internal copy.
 * stride_layer/stride_row in elements; for the packed (gather) layout stride_row = 0. */
int beom_device_field(beom_handle h, const char *name, void **dptr,
                      int64_t *stride_layer, int64_t *stride_row, int64_t *row0_offset);
/* 1 if the dense fast path is active for this handle, else 0. */
int beom_is_dense(beom_handle h);
/* Per-kernel device time, measured with HIP events on the handle's stream around every
 * sweep launched by beom_step between start and stop (no host synchronisation in
 * between): ms[0..7] = update_h, update_mont, update_viscosity, update_u, update_v,
 * fused mont+viscosity, fused u+v, the tracer sweep (sums over launches), launches[0..7] = number of
 * launches in each class.  Both arrays need 8 entries. */
int beom_profile_start(beom_handle h);
int beom_profile_stop(beom_handle h, double *ms, int *launches, char *errm, int errm_len);
/* = beom_profile_start; beom_step(...); beom_profile_stop. */
int beom_profile_steps(beom_handle h, int tstp_first, int nsteps,
                       double tres, double dtd8, double dt_r, double rsta, int n_3d,
                       double *ms, int *launches, char *errm, int errm_len);

/* ---- Passive tracers carried by the layer transports (no reference routine; DESIGN.md f-N6).  Per tracer t = 1..ntrc the
 * handle holds the layer CONTENT q = thickness x concentration and two history levels of its tendency, stored as the other
 * arrays with the tracer index slowest:
 *   q(0:ndeg, nlay, ntrc)      -> q[ipnt + (ndeg+1)*((ilay-1) + nlay*(t-1))]             (ctrg alike)
 *   rq(2, 0:ndeg, nlay, ntrc)  -> rq[(m-1) + 2*(ipnt + (ndeg+1)*((ilay-1) + nlay*(t-1)))]
 * Index 0 (the land sentinel) is never written and is meant to hold 0.  One update per time step, immediately before that
 * step's update_h, from the thicknesses and face transports update_h is about to read and with update_h's time scheme
 * (E, N, W, S = neig(1|3|5|7, p); all FP64, in this order):
 *   c(x)  = hlay(x,l) > 0 ? q(x,l) / hlay(x,l) : +0.0                 wet(x) = hlay(x,l) > 0
 *   Fu(p) = h_u(p,l) * cf,  (a,b) = h_u(p,l) > 0 ? (W,p) : (p,W),  cf = wet(a) ? c(a) : c(b)      (Fv alike with h_v and S)
 *   src   = hdot present ? hdot(p,l) * (hdot(p,l) > 0 ? ctrg(p,l) : c(p)) : +0.0
 *   r3    = ((Fu(p) - Fu(E)) * i_dl + (Fv(p) - Fv(N)) * i_dl + src) * mk_n(p)
 *   qh    = q + ((1.5+beta)*r3 - (0.5+2*beta)*rq(2) + beta*rq(1)) * dt * gene + r3 * dt * (1-gene)
 *   q_new = (ctrg(p,l) * hfor) * nudg(p,1) + (1 - nudg(p,1)) * qh,   hfor = update_h's target thickness (fnud + tide)
 *   rq(1) <- rq(2);  rq(2) <- r3
 * First-order upstream with the no-gradient rule at an empty upwind cell: conservative, consistent with the continuity
 * equation by construction (a tracer of concentration 1 with ctrg = 1 IS hlay, bit for bit), NOT monotone — small negative
 * concentrations occur.  Water that a sponge or hdot > 0 brings in carries the relaxation concentration ctrg (+0.0 until
 * uploaded); withdrawal carries the local concentration.
 * beom_set_tracers allocates (q, rq, ctrg = 0; ntrc = 0 frees; between steps only) and refuses (-6) the configurations whose
 * thickness is changed by something the scheme does not follow: variant = 1 and rgld = 1.  beom_step and beom_step_phase
 * (phase 1) then run the tracer sweep; beom_update_tracers is the per-sweep entry (as beom_update_h; beom_update_h itself
 * does not move tracers).  beom_info(h, "tracers") returns the count. */
int beom_set_tracers(beom_handle h, int ntrc, char *errm, int errm_len);
/* any pointer may be NULL = keep */
int beom_upload_tracers(beom_handle h, const double *q, const double *rq, const double *ctrg, char *errm, int errm_len);
int beom_download_tracers(beom_handle h, double *q, double *rq, char *errm, int errm_len);
int beom_update_tracers(beom_handle h, double gene, double ramp, double ctim);
/* The scheme of the tracer sweep, chosen per handle: 1 = the first-order upstream faces above (the default), 2 = "limited",
 * a flux-limited third-order face.  Everything of beom_update_tracers stays except the face concentration cf.  For the face
 * of cell x towards its back neighbour B (B = W(x) for Fu, B = S(x) for Fv), with F = the stored transport at x:
 *   (U, D, UU) = F > 0 ? (B, x, back(B)) : (x, B, fwd(x))     back = W|S link, fwd = E|N link, each of the cell named
 *   first      = wet(U) ? c(U) : c(D)                          (today's cf, no-gradient rule included)
 *   if !(wet(U) && wet(D) && wet(UU))   cf = first
 *   else  du = c(U) - c(UU);  dd = c(D) - c(U)
 *         if (du*dd > 0.0)  m   = fmin(fmin(2.0*fabs(du), 2.0*fabs(dd)), fabs((du + 2.0*dd) * T3)),   T3 = 1.0/3.0 (FP64)
 *                           lim = copysign(m, dd)
 *         else              lim = +0.0
 *         cf = c(U) + 0.5*lim
 *   flux = F * cf
 * All arithmetic is FP64, in this order, with no contraction.  This is Koren's limiter.  It is the kappa = 1/3 third-order
 * upwind-biased face value where the field is smooth, clipped to stay between the upwind and downwind cell.
 *  - Fu(E) and Fv(N) are the same expressions at cell E (N) with that cell's own links, as today.
 *  - The links of the sentinel are all 0 and hlay(0) = 0.  So next to land, a dry cell or the frame's edge, the face falls
 *    back to today's value.
 *  - With every concentration equal, du = dd = 0, lim = +0.0 and cf = c(U) exactly.  Hence the identity with hlay.
 * Limits (documented, not asserted by the engine):
 *  - This is a method-of-lines limiter under the thickness equation's three-level time scheme.
 *  - In the runs measured with the numpy restatement it preserved bounds for |u|dt/dl = 0.1 with |v|dt/dl = 0.05, and for
 *    0.15 with 0.075.  That is the range measured; free-surface runs sit at about 0.01.
 *  - It goes unstable at 0.25 + 0.125 (variance x3.8 over 40 steps).  Upstream itself goes unstable at 0.4 + 0.2.
 * Returns -3 for any other scheme (the argument is looked at before the handle).  Between steps only.  The choice is kept on
 * the handle for its life: beom_set_tracers does not reset it, and a handle without tracers just keeps it.  It may change
 * between steps of a run; rq then holds the other scheme's tendencies, as after a restart from another scheme's files.
 * beom_info(h, "tracer_scheme") returns it. */
int beom_set_tracer_scheme(beom_handle h, int scheme, char *errm, int errm_len);
/* Lateral diffusion, decay and sources of the tracers (no reference routine; DESIGN.md f-N11): an operator-split
 * forward-Euler update of q in a launch of its own in front of the tracer sweep of either scheme, while q and hlay still
 * belong to the same time level.  Per tracer t, layer l and cell p (E, N, W, S = neig(1|3|5|7, p)), all FP64, no
 * contraction, in this order:
 *   c(x)     = hlay(x,l) > 0 ? q(x,l) / hlay(x,l) : +0.0
 *   kd       = kappa(t,l) * i_dl
 *   G(b, x)  = hf > 0 ? (kd * hf) * (c(b) - c(x)) : +0.0,   hf = fmin(hlay(b,l), hlay(x,l))
 *   Gu(p) = G(W(p), p)    Gu(E) = G(W(E), E)    Gv(p) = G(S(p), p)    Gv(N) = G(S(N), N)
 *   div      = ((Gu(p) - Gu(E)) + (Gv(p) - Gv(N))) * i_dl
 *   r        = ((div + source(t,l) * hlay(p,l)) - decay(t,l) * q(p,l)) * mk_n(p)
 *   q_mix    = hlay(p,l) > 0 ? q(p,l) + dt * r : q(p,l)
 *  - W(E) and S(N) are cell E's and N's own back links, as for Fu(E), Fv(N) above: the sentinel's links are 0.
 *  - G(b, x) is the diffusive flux of content into x through the face it shares with b: div(kappa h grad c) in flux form.
 *    The face is as thick as the thinner of its two cells.  A face next to land, a dry cell, the frame's edge or an open
 *    boundary carries nothing, because hlay(0) = 0.  Every weight hf / hlay(p) is at most 1, so kappa*dt/dl^2 <= 1/4 makes
 *    the new concentration a convex combination of the five old ones: a maximum principle, whatever the thickness contrast.
 *  - decay is a rate in 1/s, source adds concentration per second.  source = 1 in the interior layers with a large decay in
 *    layer 1 gives a ventilation age in seconds; decay alone a radioactive tracer.
 *  - dt is the handle's dt, in steps 1-3 too.  rq is not touched: the multistep history stays the advective tendency.
 *  - With q = hlay, decay = source = +0 and any kappa every c is exactly 1, every G is +0, r = +0 and q_mix = q: the
 *    identity with hlay holds with diffusion on, under both schemes.
 *  - The tracer moments' fu, fv remain the advective faces: the diffusive flux is not in their mean budget.
 * beom_set_tracer_mixing: kappa (m2/s), decay, source are [ntrc][nlay] each (x[(l-1) + nlay*(t-1)]); NULL = all +0.  All
 * NULL or all zero switches the mixing off: its array is freed and no launch follows, the step is what it was.  Between
 * steps only, after beom_set_tracers (-3 otherwise).  Refused with -3 and a message, nothing touched: a value that is not
 * finite, kappa < 0, kappa*dt/dl^2 > 0.25, decay < 0, decay*dt > 1 (the two caps are held to a few units of rounding, so
 * that kappa = 0.25*dl*dl/dt passes).  beom_set_tracers with another count drops the mixing, the same count keeps it;
 * uploads leave it alone.  beom_step and beom_step_phase (phase 1) then run the launch in front of the tracer sweep;
 * beom_update_tracer_mixing is the launch on its own (-3 without mixing), and beom_update_tracers stays the advective sweep
 * alone.  beom_info: "tracer_mixing" (0 | 1), "tracer_mix_launches" (all calls so far). */
int beom_set_tracer_mixing(beom_handle h, const double *kappa, const double *decay, const double *source, char *errm, int errm_len);
int beom_update_tracer_mixing(beom_handle h);
/* Vertical (diapycnal) diffusion of the tracers between the layers of a water column (no reference routine; DESIGN.md
 * f-N12): an operator-split backward-Euler update of q in a launch of its own, behind the lateral mixing and in front of the
 * tracer sweep of either scheme, while q and hlay still belong to the same time level.  The unknowns are the FLUXES through
 * the interfaces k = 1..nlay-1 (between layers k and k+1, 1 = top), not the concentrations.  Per cell p and tracer t, all
 * FP64, no contraction, in this order:
 *   m_l   = hlay(p,l) > 0
 *   c_l   = m_l ? q_l / h_l : +0.0
 *   b_l   = m_l ? 1.0 / h_l : +0.0                (once per cell, for every tracer)
 *   rk(t,k) = 1.0 / (dt * kappa_v(t,k))           formed on the host in FP64 (product first, then reciprocal);
 *                                                 +0.0 where kappa_v(t,k) == 0
 *   open(k) = mk_n(p) > 0.5 && m_k && m_{k+1} && rk(t,k) > 0
 *   forward, k = 1 .. nlay-1, with s_0 = 1.0, y_0 = +0.0:
 *       R   = (0.5 * (h_k + h_{k+1})) * rk(t,k)
 *       pp  = R + b_k * s_{k-1}
 *       den = pp + b_{k+1}
 *       inv = 1.0 / den
 *       num = (c_k - c_{k+1}) + b_k * y_{k-1}
 *       open(k):  g_k = b_{k+1} * inv;  y_k = num * inv;  s_k = pp * inv
 *       else:     g_k = +0.0;           y_k = +0.0;       s_k = 1.0
 *   back:  G_{nlay-1} = y_{nlay-1};   G_k = y_k + g_k * G_{k+1};   G_0 = G_nlay = +0.0
 *   q'_l = m_l ? (q_l + G_{l-1}) - G_l : q_l
 *  - G_k is the content moved from layer k into layer k+1 during the step.  It solves
 *    G_k (R_k + b_k + b_{k+1}) - b_k G_{k-1} - b_{k+1} G_{k+1} = c_k - c_{k+1}, that is G = (dt kappa_v / hbar)(c'_k - c'_{k+1})
 *    with c' = q'/h and hbar the mean of the two thicknesses: backward Euler in the column.
 *  - The elimination carries s_k = 1 - g_k as pp/den: nothing nearly equal and positive is subtracted.
 *  - No cap on kappa_v: the matrix's row sum is R_k >= 0, the scheme is unconditionally stable, and kappa_v -> infinity gives
 *    the thickness-weighted column mean.
 *  - Every G_k enters two layers with opposite sign: the column sum of q changes by rounding only.
 *  - With q = hlay every c is exactly 1, every num, y and G is +0 and q' = q: the identity with hlay holds with vertical
 *    mixing on, under both schemes and with lateral mixing.
 *  - A dry layer, a land cell (mk_n = 0), the sentinel or kappa_v(t,k) = 0 closes an interface; the column falls into
 *    independent pieces there.  A thin wet layer conducts: its resistance is its thickness.
 *  - The error is rounding of the CONTENT: a few units of 2^-52 * (|q_l| + |G_{l-1}| + |G_l|).  A massless layer's
 *    concentration is therefore accurate only to the rounding of the content that passes through it, as in any conservative
 *    form.
 *  - dt is the handle's dt, in steps 1-3 too.  rq is not touched.  q is updated in place: a column reads its own cell only.
 * beom_set_tracer_vmixing: kappa_v (m2/s) is [ntrc][nlay-1], kappa_v[(k-1) + (nlay-1)*(t-1)].  NULL or all zero switches it
 * off: the device array is freed and no launch follows, the step is what it was.  Between steps only, after beom_set_tracers.
 * Refused with -3 and a message, nothing touched: a handle without tracers; a value that is not finite or is negative; a
 * non-NULL kappa_v on a handle with nlay = 1; a kappa_v > 0 whose 1.0/(dt*kappa_v) is not a positive normal number (so that
 * rk = 0 means "closed" and nothing else).  beom_set_tracers with another count drops it, the same count keeps it; uploads
 * leave it alone.  beom_step and beom_step_phase (phase 1) then run: lateral mixing, vertical mixing, the sweep.
 * beom_update_tracer_vmixing is the launch on its own (-3 without vertical mixing); beom_update_tracers stays the advective
 * sweep alone.  beom_info: "tracer_vmixing" (0 | 1), "tracer_vmix_launches" (all calls so far). */
int beom_set_tracer_vmixing(beom_handle h, const double *kappa_v, char *errm, int errm_len);
int beom_update_tracer_vmixing(beom_handle h);

/* ---- Lagrangian (isopycnal) floats carried by the layer velocities (no reference routine; DESIGN.md f-N7).  A float has a
 * position (x, y) in FP64 grid units and a fixed layer l.  Cell (i, j) spans [i-1, i] x [j-1, j]; u(p) sits on the cell's west
 * face and v(p) on its south face; E = neig(1, p), N = neig(3, p).  cell(x, y) is the packed cell of i = floor(x)+1,
 * j = floor(y)+1, or 0 if (i, j) lies outside 1..lm+1 x 1..mm+1 or holds no packed cell; wet(x, y) means
 * mk_n(cell(x, y)) > 0.5.  xper (yper): the frame wraps in x (y) — some cell of column (row) 1 has a W (S) neighbour.
 * The velocity at a position is linear between the two faces of the home cell, each component along its own axis only (the
 * usual C-grid float interpolation: the wall-normal velocity is exactly the stored masked zero on a coast face).  All
 * arithmetic FP64, in this order, no contraction:
 *   fx = floor(x); a = x - fx;   fy = floor(y); b = y - fy;   p = cell(x, y)
 *   U(x,y) = (1.0 - a)*u(p,l) + a*u(E,l)        V(x,y) = (1.0 - b)*v(p,l) + b*v(N,l)
 *   cdt = dt * i_dl     (formed once on the host; i_dl is the engine's own 1.0/dl)
 *   wrapx(z): if xper { if (z < 0.0) z = z + lm; if (z >= lm) z = z - lm }     (wrapy alike with mm, yper)
 * A step is Heun's method on the velocities before and after that step's momentum update:
 *   stage 1 (u, v as they stand when the step begins):
 *     k1 = (U, V)(x, y)*cdt;  (xs, ys) = (wrapx(x + k1x), wrapy(y + k1y));  if !wet(xs, ys) then (xs, ys) = (x, y)
 *   stage 2 (u, v as the step leaves them: after the open-boundary pass and, with a lid, after the pressure correction):
 *     k2 = (U, V)(xs, ys)*cdt;  xn = wrapx(x + 0.5*(k1x + k2x)), yn alike
 *   landing rule: the float takes the first wet candidate of (xn, yn), (xn, y), (x, yn), (x, y); the per-float counter
 *     `rejected` counts the steps whose first candidate was not taken.
 * So a float that starts in a wet cell is in a wet cell after every step, by construction.  Neighbours come from the handle's
 * own connectivity, so periodic seams behave as for every other sweep; a position is wrapped, so the duplicated column lm+1 /
 * row mm+1 of a periodic frame is never a home cell.
 *
 * beom_set_floats allocates n floats (n = 0 frees them; between steps only) and a track recorder of nrec records (0 = none):
 * behind stage 2 of every step with tstp % stride == 0, beom_step keeps (x, y, h) of every float on the device, h = hlay of
 * the home cell as the step leaves it.  It refuses (-6) handles that hold one band of rows (slab_mm != 0): a float leaves
 * its band (bands carry floats through their multi handle: "Floats on bands" below).  beom_upload_floats sets positions and layers (1-based), zeroes `rejected` and empties the recorder; it refuses
 * (-3, naming the first offender, the handle's floats untouched) a layer outside 1..nlay and a position whose cell is not
 * wet.  beom_step then moves the floats: K steps of one call cost K + 1 float launches (stage 2 of a step and stage 1 of
 * the next read the same velocities); it refuses (-3), before launching anything, a call whose steps would write more
 * records than the recorder has free.  beom_download_floats: any pointer may be NULL.  beom_download_float_track copies
 * the held records, rec[(k*3 + c)*n + f] (record k; c = 0, 1, 2: x, y, h; float f), their number and steps, and empties
 * the recorder; rec needs room for nrec records.  beom_update_floats is the per-sweep entry (stage = 1 | 2, on the state as it
 * stands; writes no record).  beom_info: "floats" (the count), "float_records" (held), "float_launches" (so far). */
int beom_set_floats(beom_handle h, int64_t n, int nrec, int stride, char *errm, int errm_len);
int beom_upload_floats(beom_handle h, const double *x, const double *y, const int32_t *layer, char *errm, int errm_len);
int beom_download_floats(beom_handle h, double *x, double *y, int32_t *layer, int32_t *rejected, char *errm, int errm_len);
int beom_download_float_track(beom_handle h, double *rec, int *count, int *tstp_of_record, char *errm, int errm_len);
int beom_update_floats(beom_handle h, int stage);

/* ---- Moments: time means and second moments of the layer fields, accumulated on the device (no reference routine;
 * DESIGN.md f-N8).  The five fields are f = 0..4: hlay, u, v, h_u, h_v.  A SAMPLE is taken behind step tstp of beom_step when
 * tstp % stride == 0: after the open-boundary pass, the lid's pressure correction and its transport rebuild, so it reads the
 * fields exactly as beom_download_state would return them after that step.  K steps of one call take their samples without
 * returning to the host; the bits do not depend on how the steps are divided into calls.
 * The sums are shifted by a reference that the first sample sets.  All arithmetic FP64, in this order, no contraction, at
 * every element of the packed (0:ndeg, nlay) storage, the sentinel included (it holds constants: its sums are +0.0):
 *   first sample after beom_set_moments / beom_reset_moments:   ref_f = x_f;  S_f = +0.0;  Q_m = +0.0;  count = 1
 *   every later sample:   d_f = x_f - ref_f;  S_f = S_f + d_f;  Q_m = Q_m + d_a*d_b  (the product rounded, then added);  count += 1
 *   the five second moments m = 0..4 are (a, b) = (h,h) (u,u) (v,v) (u,h_u) (v,h_v)
 * Derived by the caller: mean = ref + S/count; (co)variance = Q/count - (S_a/count)*(S_b/count).  Why shifted: a plain
 * sum of x and x*x loses the signal of a deep layer.  On h = 4000 + 0.01*sin(0.0137*t + phi) + 0.003*noise, 16 cells,
 * 100 000 samples, the shifted variance is within 5.8e-14 relative of the long-double two-pass value; the plain form is
 * off by 7.2e-3 (tests/test_moments_cpu.py repeats both).
 * `level` chooses what is kept; nothing else is read or written:
 *   1: ref, S of hlay, u, v        2: level 1 plus ref, S of h_u, h_v        3: level 2 plus the five Q
 * (6 / 10 / 15 more arrays of the state's size; 12 / 20 / 30 words of traffic per cell-layer and sample).
 * beom_set_moments: level = 0 frees, stride >= 1; allocates, count = 0; between steps only; every handle kind (bands of
 * rows, variant = 1 and the rigid lid included); -3 for a level outside 0..3 or stride < 1.  beom_reset_moments sets
 * count = 0 and moves no memory: the next sample is a first sample.  beom_upload_state does NOT reset: a restart continues
 * an average.  beom_sample_moments is the per-sweep entry: one sample of the state as it stands, whatever the stride,
 * recorded under the step number of the handle's last step (0 before any).  beom_download_moments: any array pointer may be
 * NULL; the layout is that of the state arrays with the field index slowest, sum[ipnt + (ndeg+1)*((ilay-1) + nlay*f)] (ref
 * alike; sq with m for f); levels 1 and 2 fill only the fields they keep; -3 if sq is asked for below level 3 or the handle
 * has no moments; with count = 0 it returns zeros (tstp_first = tstp_last = 0) and no error.  tstp_first / tstp_last: the
 * steps of the first and the latest sample.  beom_info: "moments" (the level), "moment_samples" (the count, capped at
 * 2e9), "moment_launches" (so far).  beom_set_option(h, "moments_by_caller", 1): beom_step takes no sample by itself and the
 * caller places every sample with beom_sample_moments (what the bands of beom_multi_* do). */
int beom_set_moments(beom_handle h, int level, int stride, char *errm, int errm_len);
int beom_reset_moments(beom_handle h);
int beom_sample_moments(beom_handle h);
int beom_download_moments(beom_handle h, double *ref, double *sum, double *sq, long long *count, int *tstp_first, int *tstp_last,
                          char *errm, int errm_len);

/* ---- Harmonics: least-squares harmonic analysis of the layer fields, accumulated on the device (no reference routine;
 * DESIGN.md f-N14).  The fields are those of the moments, f = 0..4: hlay, u, v (level 1) and h_u, h_v (level 2), fitted at
 * K = nfreq <= BEOM_MAX_HARMONICS frequencies omega_k given by the caller in rad/day, the unit of w_ti.  A SAMPLE is taken
 * behind step tstp of beom_step when tstp % stride == 0, where the moments' sample sits (after the open-boundary pass, the
 * lid's pressure correction and its transport rebuild).  Its time is the step's own ctim = tres + dtd8*(double)tstp, in days.
 * K steps of one call take their samples without returning to the host; the bits do not depend on how the steps are
 * divided into calls.
 * The WEIGHTS of a sample are formed on the host in FP64 with libm: th = omega_k*ctim; cw_k = cos(th); sw_k = sin(th).
 * beom_harmonic_weights returns exactly them (host only, no device, as beom_integral_combine); the device receives them as
 * scalars and only subtracts, multiplies and adds.  Per field and per element of the packed (0:ndeg, nlay) storage, the
 * sentinel included (its sums are +0.0), all FP64, no contraction, in this order, k ascending:
 *   first sample after beom_set_harmonics / beom_reset_harmonics:   ref = x;  S0 = +0.0;  C_k = S_k = +0.0;  count = 1
 *   every later sample:   d = x - ref;  S0 = S0 + d;  C_k = C_k + d*cw_k;  S_k = S_k + d*sw_k  (the product rounded, then
 *   added);  count += 1
 * The NORMAL MATRIX is kept on the host, for every sample, the first included: with w = (1, cw_1, sw_1, ..., cw_K, sw_K),
 * G[i][j] = G[i][j] + w_i*w_j, (1+2K)^2 doubles, row-major; set and reset zero it.
 * Derived by the caller: solve G a = b per element with b = (S0, C_1, S_1, ...); mean = ref + a_0,
 * amp_k = hypot(a_{2k-1}, a_{2k}), phase_k = atan2(a_{2k}, a_{2k-1}), so x ~ mean + sum_k amp_k*cos(omega_k*t - phase_k).
 * (The first sample has d = 0: its row of the design matrix is in G and its right-hand side is zero, so a is the exact
 * least-squares fit of d over all `count` samples, for any record length and sampling.)  Why shifted by the first sample:
 * the mean is exact for a constant field, and a deep layer keeps its digits: a 0.01 m + 0.005 m signal on 4000 m, 3000
 * samples, is fitted to 2.2e-12 relative in amplitude shifted against 1.7e-11 unshifted (tests/test_harmonics_cpu.py).
 * Layout: sum[ipnt + (ndeg+1)*((ilay-1) + nlay*(m + (1+2K)*f))] with m = 0 for S0, m = 2k-1 for C_k, m = 2k for S_k
 * (k = 1..K); ref as the moments' ref.  fields*(2 + 2K) more arrays of the state's size; 4 + 4K words of traffic per
 * element, field and later sample, one launch per field.
 * beom_set_harmonics: nfreq = 0 frees (the other arguments are not looked at); else level 1 or 2, stride >= 1, nfreq
 * 1..BEOM_MAX_HARMONICS; -3 with a message and nothing touched for anything else, for an omega that is not finite or is
 * <= 0, and for two omega that are equal (nearly equal ones are the caller's affair: gram shows the conditioning).  It
 * allocates, count = 0; between steps only; a failed allocation leaves the handle without harmonics.  Every single handle
 * kind keeps them (embedded, table path, variant = 1, rigid lid, svis > 0, open boundaries).  beom_reset_harmonics sets
 * count = 0, zeroes G and moves no device memory.  beom_upload_state does NOT reset: a restart continues an analysis.
 * beom_sample_harmonics is the per-sweep entry: one sample at time ctim of the state as it stands, whatever the stride,
 * under the step number of the handle's last step.  beom_download_harmonics: any pointer may be NULL; gram has (1+2K)^2
 * and omega K entries; -3 on a handle without harmonics; with count = 0 it returns zeros.  beom_info: "harmonics" (nfreq),
 * "harmonic_level", "harmonic_samples" (capped at 2e9), "harmonic_launches" (so far: fields per sample).  The option
 * "moments_by_caller" governs these samples too.  A handle without harmonics launches exactly what it launched before. */
#define BEOM_MAX_HARMONICS 4
int beom_harmonic_weights(double omega, double ctim, double *cw, double *sw);
int beom_set_harmonics(beom_handle h, int nfreq, const double *omega, int level, int stride, char *errm, int errm_len);
int beom_reset_harmonics(beom_handle h);
int beom_sample_harmonics(beom_handle h, double ctim);
int beom_download_harmonics(beom_handle h, double *ref, double *sum, double *gram, double *omega, long long *count,
                            int *tstp_first, int *tstp_last, char *errm, int errm_len);

/* ---- Forcing in time: the wind stress taus(0:ndeg, 2) and the thickness source hdot(0:ndeg, nlay) interpolated between
 * frames at the top of every time step, on the device (no reference routine; DESIGN.md §4 "Forcing in time";
 * tests/forcing_ref.py is this rule in numpy).
 * A FRAME SET belongs to one field.  It has nfr >= 1 frames in the field's Fortran storage, frames[k][...] one behind the
 * other, and times[nfr] in days on the clock of ctim = tres + dtd8*(double)tstp, strictly increasing and finite.  period is
 * 0 (none) or greater than times[nfr-1] - times[0] (the set repeats with that period).
 * The WEIGHT of a time is formed on the host.  beom_forcing_weight returns exactly it (host only, no device, as
 * beom_harmonic_weights); FP64, every operation rounded once, written as here:
 *   nfr == 1:                                  (k0, k1, a) = (0, 0, 0)
 *   period == 0:  t = ctim
 *       t <  times[0]                          (0, 0, 0)
 *       t >= times[nfr-1]                      (nfr-1, nfr-1, 0)
 *       else  k0 = the largest k with times[k] <= t;  k1 = k0 + 1;  a = (t - times[k0]) / (times[k1] - times[k0])
 *   period > 0:   r = fmod(ctim - times[0], period);  if (r < 0) r += period;  t = times[0] + r
 *       t >= times[nfr-1]                      k0 = nfr-1;  k1 = 0;  a = (t - times[nfr-1]) / ((times[0] + period) - times[nfr-1])
 *       else  as for period == 0
 * The FIELD, per element, with A, B the values of frames k0, k1 (FP64, no contraction):
 *   d = B - A;    x = (a == 0 || d == 0) ? A : A + a*d
 * The select is deliberate: where two frames agree the result is the frame bit for bit, a -0 included, and at a = 0 it is
 * the frame itself; so a set of equal frames steps exactly as a handle created with that array.  (1-a)*A + a*B does not
 * have this property.
 * WHERE it acts: at the top of every time step, in front of the stress, the tracer launches and update_h — steps 1-3, every
 * step of a K-step beom_step call, and phase 1 of beom_step_phase.  From there the arrays the step reads hold the field at
 * that step's ctim: for taus the array distribute_stress reads and the cells-only copy the folded momentum sweep reads
 * (+0 at the sentinel and in every slot that is no cell); for hdot the array update_h and the tracer sweeps read.  The
 * launch (k_forcing_lerp, beom_forcing.h) is purely elementwise over frames kept in the device layout: 2 words read and
 * 2 (taus) | 1 (hdot) written per element.  It is left out where the array already holds these bits: the same (k0, k1, a)
 * as the field's last launch.  beom_info "forcing_launches" counts what ran.
 * FLAGS: the handle's wind follows private_mod.f95:1945 applied to the frames (any |element| of any frame > 1e-7), hdot is
 * live if any element of any frame is non-zero; the stress terms, has_stress and the folded stress are re-derived whenever a
 * set is given or cleared, so a handle created without taus or hdot gains the term, and "stress_folded" stays 1 while the
 * frames vary.  (The reference decides wind from the array of the moment: a step whose interpolated taus has nothing above
 * 1e-7 while a frame has differs from a host that replaces the array.)
 * beom_set_forcing(h, field, nfr, times, period, frames): field = BEOM_FORCING_TAUS | BEOM_FORCING_HDOT; between any two
 * steps; the frames are copied.  It launches the first frame into the field's buffers, so a download is defined at once.
 * nfr = 0 clears the set: the handle reads the arrays of beom_create again and steps as before.  Refused with -3 and a
 * message that names the fault, nothing touched: an unknown field, times that are not finite or not strictly increasing, a
 * period that is negative, not finite or not greater than the span of the times, a frame value that is not finite.  (Field,
 * times and period are looked at before the handle, the frames' values with its sizes.)
 * beom_apply_forcing(h, ctim): the launches of time ctim alone, as a step would place them.
 * beom_download_forcing(h, taus, hdot): what the next sweep would read, in Fortran storage; either pointer may be NULL;
 * without a frame set, the array of beom_create (zeros if that was NULL).
 * beom_info: "forcing_taus_frames", "forcing_hdot_frames" (nfr; 0 = none), "forcing_launches" (so far). */
#define BEOM_FORCING_TAUS 1
#define BEOM_FORCING_HDOT 2
int beom_forcing_weight(int nfr, const double *times, double period, double ctim, int *k0, int *k1, double *a);
int beom_set_forcing(beom_handle h, int field, int nfr, const double *times, double period, const double *frames,
                     char *errm, int errm_len);
int beom_apply_forcing(beom_handle h, double ctim, char *errm, int errm_len);
int beom_download_forcing(beom_handle h, double *taus, double *hdot, char *errm, int errm_len);

/* ---- Tracer moments: time means of a tracer's content, concentration and face fluxes and the variance of its concentration,
 * accumulated on the device (no reference routine; DESIGN.md f-N9).  With t the tracer, l the layer, p a real cell and
 * W, S = neig(5|7, p), c(x) is trc_conc of beom_tracers.h, c(x) = hlay(x,l) > 0 ? q(x,l,t)/hlay(x,l) : +0.0, and four
 * quantities k = 0..3 are sampled:
 *   x_q  = q(p,l,t)                 the content
 *   x_c  = c(p)                     the concentration
 *   x_fu = h_u(p,l) * cf            cf exactly from trc_face (upstream, no-gradient rule) between W and p:
 *                                   (a, b) = h_u(p,l) > 0 ? (W, p) : (p, W),  cf = hlay(a,l) > 0 ? c(a) : c(b)
 *   x_fv = h_v(p,l) * cf            likewise between S and p with h_v
 * They feed the moments' own shifted sums (see beom_set_moments), all FP64, no contraction, in this order:
 *   first sample after beom_set_tracer_moments / beom_reset_tracer_moments:  ref_k = x_k;  S_k = +0.0;  Q = +0.0;  count = 1
 *   every later sample:  d_k = x_k - ref_k;  S_k = S_k + d_k;  Q = Q + d_c*d_c  (the product rounded, then added);  count += 1
 * Derived by the caller: mean = ref + S/count; var_c = Q/count - (S_c/count)*(S_c/count).
 *   level 1: ref, S of q and c        level 2: level 1 plus ref, S of fu, fv        level 3: level 2 plus Q of (c, c)
 * (4 / 8 / 9 more arrays of the tracers' size; 3 + 15 ntrc words of traffic per cell-layer and level-3 sample, 3 + 10 ntrc for
 * a first sample.)  A SAMPLE is taken at the very end of step tstp of beom_step when tstp % stride == 0, where the field
 * moments' sample sits.  The q, hlay, h_u, h_v standing there are exactly what the next step's tracer sweep reads, so under
 * scheme 1 the sampled x_fu, x_fv are bit for bit the face fluxes Fu(p), Fv(p) that sweep applies: the mean content budget
 * closes against the mean of the model's own fluxes.  Under scheme 2 (beom_set_tracer_scheme) they are STILL the upstream
 * faces, not the limited ones the sweep applies.  Slots that are no real cell are not part of the contract; a download
 * returns +0.0 at index 0.
 * Level, stride and count are the tracer moments' own, independent of beom_set_moments.  beom_set_tracer_moments: level = 0
 * frees, stride >= 1; allocates, count = 0; between steps only; -3 for a level outside 0..3 or stride < 1, and -3 for a handle
 * without tracers.  beom_set_tracers with another count frees them; beom_upload_state and beom_upload_tracers do NOT reset
 * them: a restart continues the average.  beom_reset_tracer_moments sets count = 0 and moves no memory.
 * beom_sample_tracer_moments is the per-sweep entry: one sample of the state as it stands, whatever the stride, recorded
 * under the step number of the handle's last step.  beom_download_tracer_moments: any array pointer may be NULL; layout
 * ref[ipnt + (ndeg+1)*((ilay-1) + nlay*(t + ntrc*k))] (sum alike; sq without k), level 1 fills k = 0..1 only; -3 if sq is
 * asked for below level 3 or the handle keeps no tracer moments; with count = 0 it returns zeros and no error.  beom_info:
 * "tracer_moments" (the level), "tracer_moment_samples", "tracer_moment_launches".  The option "moments_by_caller" governs
 * these samples as it does the field moments'. */
int beom_set_tracer_moments(beom_handle h, int level, int stride, char *errm, int errm_len);
int beom_reset_tracer_moments(beom_handle h);
int beom_sample_tracer_moments(beom_handle h);
int beom_download_tracer_moments(beom_handle h, double *ref, double *sum, double *sq, long long *count, int *tstp_first,
                                 int *tstp_last, char *errm, int errm_len);

/* ---- Conservation integrals of the state as it stands between two steps (no reference routine: the reference's test
 * case 3 forms them from the output files, testcases/conservation.m:116-211).  All FP64, raw sums over the frame:
 *   out[(l-1)*4 + 0]  vol   sum of mk_n*h                                    layer volume / dl^2
 *   out[(l-1)*4 + 1]  ke    sum of mk_u*((u*u)*hcu) + mk_v*((v*v)*hcv)       kinetic energy = 0.5*rhon(l)*dl^2 * ke, the thickness
 *                           at a velocity point being the momentum sweeps' own (private_mod.f95:1438, 1521)
 *   out[(l-1)*4 + 2]  ens   sum of 0.5*(pvor*pvor)*(have/nm) where mkpi > 0.5 and nm > 0 (:2421-2433; conservation.m:203-206)
 *   out[(l-1)*4 + 3]  circ  sum of rvor (:2388-2389)
 *   out[4*nlay]       eta2  sum of mk_n*(eta*eta), eta = hcol - h_th (:2367-2373): ONLY the barotropic part of the potential
 *                           energy, 0.5*rhon(1)*grav*dl^2 * eta2 (as conservation.m:147-150; the interface part needs the rest
 *                           thicknesses, which the engine does not hold).  With a rigid lid (rgld = 1) eta is the column misfit.
 * rvor and pvor are what update_mont_rvor_pvor_dive_kine would store for this state (recomputed, not the step's scratch).
 * The duplicated column lm+1 of a frame periodic in x and row mm+1 of one periodic in y contribute +0 to every sum.
 * Order of summation: the terms on the rectangle c = i-1, r = j-1 (+0.0 where there is no packed cell); each row by the pairwise
 * tree over the aligned column index (level k+1 adds elements 2m and 2m+1 of level k, the row padded with +0.0 to a power of
 * two), then the row sums by the same tree over rows.  No atomics: the results are the same bits for a dense handle, the table
 * path and a frame cut into any number of bands. */
int beom_integral_count(int nlay);                          /* 4*nlay + 1 */
/* rows[(j-jlo)*count + k]: the row sums of local rows jlo..jlo+nrows-1; syncs the handle's stream */
int beom_integral_rows(beom_handle h, int jlo, int nrows, double *rows, char *errm, int errm_len);
/* host only, no device: the tree over rows; rows[r*count + k] in global row order */
int beom_integral_combine(const double *rows, int nrows_total, int count, double *out);
/* = beom_integral_rows(1..mm+1) + beom_integral_combine */
int beom_integrals(beom_handle h, double *out, char *errm, int errm_len);

/* ---- Series: a record of the row sums per sampled step, kept on the device (no reference routine).  What beom_integral_rows
 * returns for one moment, recorded behind every stride-th step of the K-step loop without a host copy or a synchronisation:
 * a time-latitude diagram of volume, energy, enstrophy and circulation and, at level 2, of the layer transports.
 * One record is rows[(j-1)*cnt + k] for the handle's rows j = 1..M (M = mm+1), cnt = beom_series_count(nlay, level):
 *   k = 0 .. 4*nlay        the quantities of beom_integral_rows in its layout: vol, ke, ens, circ per layer, then eta2
 *   k = 4*nlay + 1 + (l-1) level 2: tu[l] = sum over i of h_u(i, j, l)
 *   k = 5*nlay + 1 + (l-1) level 2: tv[l] = sum over i of h_v(i, j, l)
 * h_u, h_v are the stored transport arrays (thickness * velocity through the W resp. S face of the cell, m^2/s; update_u,
 * update_v, private_mod.f95:1492, 1578) as the step leaves them: with a rigid lid whatever the lid step rebuilt.  dl * tv[l]
 * is the volume transport of layer l through the south faces of row j; accumulated over layers, the overturning
 * streamfunction in layer coordinates.  Masking is the integrals' live rule: a position without a packed cell, the duplicated
 * column lm+1 of a frame periodic in x and row mm+1 of one periodic in y contribute +0.0.
 * Order of summation: the integrals' contract, unchanged.  Each row goes through the pairwise tree over the aligned column
 * index, padded with +0.0 to a power of two.  A level-1 record equals beom_integral_rows(1..M) of that moment bit for bit,
 * the first 4*nlay + 1 entries of a level-2 record likewise, and beom_integral_combine of a record equals beom_integrals.  The
 * bits do not depend on the handle kind, the tile geometry or how the frame is cut into bands.
 * A record is written behind every step with tstp % stride == 0, where the moments' sample sits (it reads the fields as
 * beom_download_state would return them after that step), straight into slot `count` of a device buffer [nrec][M][cnt].  The
 * host keeps the step numbers.  beom_step refuses with -3, before launching anything, a call whose steps would overflow the
 * recorder.  beom_sample_series: one record by hand of the fields as they stand, under the number of the handle's last step;
 * -3 on a full recorder or without a series.  beom_download_series copies the filled records (rows[n][M][cnt], oldest first)
 * and their steps, then sets the count to 0; any of rows, tstp, count may be NULL; -3 without a series.  Uploads of state
 * do not empty the recorder.  beom_set_series: level 0 frees (stride and nrec are then not looked at); other arguments
 * reallocate and empty; between steps only; -3 for a level outside 0..2, stride < 1 or nrec < 1; -4 for rows too long for
 * the integrals; a failed allocation leaves the handle without a series and returns the allocator's code with a message.
 * Every single handle keeps a series: dense, embedded, the table path, variant = 1, rigid lid, svis > 0, open boundaries.
 * beom_info: "series" (the level), "series_records" (records held).  beom_band_set_series is the band-side piece
 * beom_multi_set_series is built from: the recorder covers local rows jlo..jlo+nrows-1 only and beom_step takes no record
 * by itself; the caller places every record with beom_sample_series. */
int beom_series_count(int nlay, int level);      /* level 1: 4*nlay + 1;  level 2: 6*nlay + 1 */
int beom_set_series(beom_handle h, int level, int stride, int nrec, char *errm, int errm_len);
int beom_sample_series(beom_handle h);
int beom_download_series(beom_handle h, double *rows, int *tstp, int *count, char *errm, int errm_len);
int beom_band_set_series(beom_handle h, int level, int stride, int nrec, int jlo, int nrows, char *errm, int errm_len);

/* ---- Column series: a record of the sums along columns per sampled step, kept on the device (no reference routine).  The
 * other direction of the series: the volume transport of each layer through a line of W faces (the exchange flow over a sill,
 * the front of a lock exchange) and x-t diagrams of volume, energy and elevation, for the flows along x.
 * Terms: the series' own, on the rectangle c = i-1, r = j-1.  Level 1: per layer vol, ke, ens, circ, then eta2; level 2: also
 * per layer h_u, then h_v.  The layout within a record is the series' and cnt = beom_series_count(nlay, level).  The integrals'
 * live rule applies: +0.0 where there is no packed cell, on the duplicated column lm+1 of a frame periodic in x and on the
 * duplicated row mm+1 of one periodic in y.
 * One record is cols[(i-1)*cnt + k] for the columns i = 1..L (L = lm+1).  dl * tu[l] of column i is the volume transport of
 * layer l through the W faces of that column; accumulated over the layers, the exchange / zonal overturning streamfunction in
 * layer coordinates.
 * Order of summation: a column is summed by the pairwise tree over the aligned GLOBAL row index (level k+1 adds elements 2m
 * and 2m+1 of level k), the column padded with +0.0 to the next power of two of M = mm+1.  The padding is added, not skipped:
 * (-0.0) + (+0.0) = +0.0 is part of the contract.  No atomics; the bits do not depend on the handle kind, the tile geometry
 * or option "column_series_batch".
 * Row window jlo..jhi (1 <= jlo <= jhi <= M; the whole column is 1..M): rows outside the window contribute +0.0 and the tree
 * is unchanged — the transport through a strait that spans only part of a column.
 * Semantics as the series': a record is written behind every step with tstp % stride == 0, where the series' sample sits.
 * beom_step refuses with -3, before launching anything, a call whose steps would overflow the recorder (the message names
 * beom_download_column_series).  beom_sample_column_series: one record by hand under the number of the handle's last step;
 * -3 without a recorder or on a full one.  beom_download_column_series copies the filled records (cols[n][L][cnt], oldest
 * first) and their steps, then sets the count to 0; any of cols, tstp, count may be NULL; -3 without a column series.  Uploads
 * do not empty the recorder.  beom_set_column_series: level 0 frees (the other arguments are then not looked at); other
 * arguments reallocate and empty; between steps only; -3 for a level outside 0..2, stride < 1, nrec < 1 or a window outside
 * 1 <= jlo <= jhi <= M.  The recorder is independent of the series and the tracer series, and keeps a scratch of its own: the
 * block partials of a launch stay under 64 MiB, a record being taken in batches of 64-column chunks (option
 * "column_series_batch", beom_set_option, read by the next beom_set_column_series: chunks per launch, 0 = by that bound).
 * Every single handle keeps one: dense, embedded, the table path, variant = 1, rigid lid, svis > 0, open boundaries.
 * beom_info: "column_series" (the level), "column_series_records" (records held).  Handles on bands refuse with -6
 * (beom_multi_*, whether created from global arrays or holding one band's window; a handle that is a band of rows): a column's
 * tree crosses the bands, and the same bits would need each band's tree nodes per column and record, which nothing combines
 * yet.  The definition over the global aligned row index is what lets that be added.  The Fortran host keeps none. */
int beom_set_column_series(beom_handle h, int level, int stride, int nrec, int jlo, int jhi, char *errm, int errm_len);
int beom_sample_column_series(beom_handle h);
int beom_download_column_series(beom_handle h, double *cols, int *tstp, int *count, char *errm, int errm_len);

/* ---- Maps: a record of sums over aligned B x B blocks of cells per sampled step, kept on the device (no reference routine).
 * The picture in time: an animation of interface height or dye, a Hovmoeller diagram of an arbitrary section, a map of kinetic
 * energy every few steps, B*B times smaller than the state and without a download of it.
 * L = lm+1, M = mm+1; B = block, a power of two in 2..64; Lc = ceil(L/B), Mc = ceil(M/B).  Block (I, J) covers
 * i = (I-1)B+1 .. IB and j = (J-1)B+1 .. JB on the GLOBAL indices.  A position holds +0.0 unless it is live; the integrals'
 * live rule applies: not live is a position past L or M, one without a packed cell (land), the sentinel, and the duplicated
 * column lm+1 of a frame periodic in x resp. row mm+1 of one periodic in y.
 * Entries per block, cnt = beom_maps_count(ntrc, nlay, level):
 *   k = 0: n, the sum of 1.0 over the block's live cells (exact in any order): what a caller divides by.
 *   Level 1, per layer l at k = 1 + (l-1)*E + m, E = 3 at level 1 and 6 at level 2 and above:
 *     m = 0: h, the term mk_n * hlay (the integrals' vol term);  m = 1: u, the cell's own u;  m = 2: v, the cell's own v.
 *   Level 2 adds  m = 3: ke, the term mk_u*((u*u)*hcu) + mk_v*((v*v)*hcv) (the integrals' ke term);  m = 4: hu, the stored
 *     transport h_u;  m = 5: hv, the stored transport h_v.
 *   Level 3 adds the content q of tracer t and layer l at k = 1 + 6*nlay + t*nlay + (l-1); -3 on a handle without tracers, and
 *     beom_set_tracers with another count frees a level-3 recorder (as it frees the tracer series).
 * Order of summation, which is the contract: within a block, first each column's B rows go through the pairwise tree over the
 * row offset in the block (level k+1 adds elements 2m and 2m+1 of level k), then the B column sums go through the pairwise
 * tree over the column offset.  Blocks are aligned and B is a power of two: a complete binary tree whose only padding is the
 * +0.0 of the positions that are not live, which is added, not skipped.  No atomics; the bits do not depend on the handle kind.
 * Layout of a record: maps[(k*Mc + (J-1))*Lc + (I-1)], an image per entry; beom_download_maps gives maps[n][cnt][Mc][Lc].
 * Semantics as the series': a record is written behind every step with tstp % stride == 0, where the series' sample sits.
 * beom_step refuses with -3, before launching anything, a call whose steps would overflow the recorder (the message names
 * beom_download_maps).  beom_sample_maps: one record by hand under the number of the handle's last step; -3 without a recorder
 * or on a full one.  beom_download_maps copies the filled records (oldest first) and their steps, then sets the count to 0;
 * any of maps, tstp, count may be NULL; -3 without maps.  Uploads do not empty the recorder.  beom_set_maps: level 0 frees (the
 * other arguments are then not looked at); other arguments reallocate and empty; between steps only; -3 for a level outside
 * 0..3, a block that is no power of two in 2..64, stride < 1 or nrec < 1.  One launch per record and no scratch: a block is
 * finished inside one wavefront.  A handle without maps launches exactly what it launched before.  Every single handle keeps
 * them: dense, embedded, the table path, variant = 1, rigid lid, svis > 0, open boundaries; level 3 wherever tracers are
 * allowed.  beom_info: "maps" (the level), "maps_block" (B; 0 without maps), "maps_records" (records held), "map_launches".
 * Handles on bands refuse with -6 (beom_multi_*; a handle that is a band of rows): a block's tree must not cross a seam, and
 * nothing aligns the seams to B yet.  The Fortran host keeps none. */
int beom_maps_count(int ntrc, int nlay, int level);      /* 1 + 3*nlay;  level 2: 1 + 6*nlay;  level 3: 1 + 6*nlay + ntrc*nlay;  level 0: 0 */
int beom_set_maps(beom_handle h, int level, int block, int stride, int nrec, char *errm, int errm_len);
int beom_sample_maps(beom_handle h);
int beom_download_maps(beom_handle h, double *maps, int *tstp, int *count, char *errm, int errm_len);

/* ---- Tracer series: a record per sampled step of the tracers' row inventories, variance, face fluxes and bounds, kept on the
 * device (no reference routine): how much of a tracer is where, how fast it crosses a latitude, how quickly its variance is
 * mixed away and whether it has left its bounds, without a download.  A recorder of its own beside the series, as the tracer
 * moments stand beside the moments: level, stride and records are independent of beom_set_series, beom_set_moments and
 * beom_set_tracer_moments.
 * Sampled are q, hlay, h_u, h_v as they stand at the end of a step, exactly what the next step's tracer sweep reads (where
 * the tracer-moment sample stands).  For tracer t, layer l and packed cell p with W, S = neig(5|7, p), all FP64 without
 * contraction (trc_conc, trc_face: the sweep's own, "Passive tracers" above):
 *   x_q  = q(p,l,t)
 *   c    = hlay(p,l) > 0 ? q(p,l,t) / hlay(p,l) : +0.0
 *   x_v  = x_q * c                          the product rounded, then summed: its row sum is sum h c^2, which with the
 *                                           inventory gives the variance whose decay measures mixing
 *   x_fu = h_u(p,l) * cf between W and p    the upstream face of the tracer moments (x_fu, x_fv there)
 *   x_fv = h_v(p,l) * cf between S and p
 *   x_b  = c + 0.0                          enters the bounds only where the position is live and hlay(p,l) > 0
 * One record is rows[(j-1)*cnt + ((t*nlay + (l-1))*nq + m)] for the handle's rows j = 1..M (M = mm+1), t = 0..ntrc-1,
 * cnt = beom_tracer_series_count(ntrc, nlay, level) = ntrc * nlay * nq:
 *   level 1, nq = 2:  m = 0 inv = sum x_q, m = 1 var = sum x_v   (own-cell loads only)
 *   level 2, nq = 4:  and m = 2 fu = sum x_fu, m = 3 fv = sum x_fv
 *   level 3, nq = 6:  and m = 4 cmin, m = 5 cmax
 * Sums (m = 0..3): the integrals' live rule and order of summation, unchanged.  A position contributes +0.0 where there is no
 * packed cell, on the duplicated column lm+1 of a frame periodic in x and on row mm+1 of one periodic in y; a row is summed
 * by the pairwise tree over the aligned column index, padded with +0.0 to a power of two.  Bounds (m = 4, 5): the minimum
 * and maximum of x_b over the live positions of the row with hlay(p,l) > 0.  The + 0.0 turns a -0 into +0, so no signed zero
 * enters and the result does not depend on the order of comparison; a row with no live wet cell of that layer holds +inf,
 * -inf; NaNs are not considered.  The bits do not depend on the handle kind, the tile geometry, the division into calls or
 * the cut into bands.  dl * fv is the tracer transport through the south faces of row j.  Under scheme 2 the faces are still
 * the upstream ones; diffusive and diapycnal fluxes are not in fu, fv.
 * A record is written behind every step with tstp % stride == 0, beside the other samples, straight into the next slot of a
 * device buffer [nrec][M][cnt]; the host keeps the step numbers.  beom_step refuses with -3, before launching anything, a
 * call whose steps would overflow the recorder (the message names beom_download_tracer_series).  beom_sample_tracer_series:
 * one record by hand, under the number of the handle's last step; -3 on a full recorder or without a tracer series.
 * beom_download_tracer_series copies the filled records (rows[n][M][cnt], oldest first) and their steps, then sets the count
 * to 0; any of rows, tstp, count may be NULL; -3 without a tracer series.  Uploads leave the recorder alone; beom_set_tracers
 * with another count frees it.  beom_set_tracer_series: level 0 frees; other arguments reallocate and empty; between steps
 * only; -3 for a level outside 0..3, stride < 1, nrec < 1 or a handle without tracers; -4 for rows too long for the
 * integrals; a failed allocation leaves the handle without a tracer series.  Every single handle that carries tracers keeps
 * one: dense, embedded, the table path, svis > 0, open boundaries (variant = 1 and the rigid lid refuse tracers).  A handle
 * without a tracer series launches exactly what it launched before.  beom_info: "tracer_series" (the level),
 * "tracer_series_records" (records held).  Option "tracer_series_batch" (beom_set_option, read by the next
 * beom_set_tracer_series): rows per launch, 0 = as many as keep the chunk partials under 64 MiB; the bits do not depend on
 * it.  beom_band_set_tracer_series is the band-side piece (local rows jlo..jlo+nrows-1, beom_step takes no record by itself). */
int beom_tracer_series_count(int ntrc, int nlay, int level);      /* host only: ntrc * nlay * 2 * level */
int beom_set_tracer_series(beom_handle h, int level, int stride, int nrec, char *errm, int errm_len);
int beom_sample_tracer_series(beom_handle h);
int beom_download_tracer_series(beom_handle h, double *rows, int *tstp, int *count, char *errm, int errm_len);
int beom_band_set_tracer_series(beom_handle h, int level, int stride, int nrec, int jlo, int nrows, char *errm, int errm_len);

/* ---- Tracer column series: a record per sampled step of the tracers' column inventories, variance, face fluxes and bounds,
 * kept on the device (no reference routine).  The other direction of the tracer series, for the flows along x in which a dye
 * is the main observable: how much of the dense-water tracer has crossed the sill, the tracer flux through a strait section,
 * whether the dye front has left its bounds at some x, without a download.
 * The per-cell quantities are the tracer series' own, word for word (x_q, c = trc_conc, x_v = x_q * c rounded then summed,
 * x_fu, x_fv = trc_face, x_b = c + 0.0; "Tracer series" above), of q, hlay, h_u, h_v as the step leaves them.
 * One record is cols[(i-1)*cnt + ((t*nlay + (l-1))*nq + m)] for the columns i = 1..L (L = lm+1), t = 0..ntrc-1, nq = 2*level,
 * cnt = beom_tracer_series_count(ntrc, nlay, level):
 *   level 1:  m = 0 inv = sum x_q, m = 1 var = sum x_v;   level 2:  and m = 2 fu, m = 3 fv;   level 3:  and m = 4 cmin, m = 5 cmax
 * Live rule: the integrals' and the tracer series'.  A position with no packed cell holds +0.0, as do the duplicated column
 * lm+1 and row mm+1 of a periodic frame and every row outside the window jlo..jhi (1-based, inclusive; the whole column is 1..M).
 * Order of summation: the column series' — the pairwise tree over the aligned GLOBAL row index r = j-1, the column padded with
 * +0.0 to M2, the next power of two of M; the padding is added, not skipped.
 * Bounds: cmin, cmax are the minimum and maximum of x_b over the live positions of the column inside the window with
 * hlay(p,l) > 0; +inf, -inf where there is none.  No signed zero enters, so any order of comparison gives the same bits.
 * dl * fu of column i is the tracer transport of layer l through the W faces of that column.  Under scheme 2 the faces are
 * still the upstream ones; the fluxes of the lateral and vertical mixing are not in fu, fv.
 * A record is sampled where the tracer series' record is sampled, behind every step with tstp % stride == 0.  beom_step
 * refuses with -3, before launching anything, a call whose steps would overflow the recorder (the message names
 * beom_download_tracer_column_series).  beom_sample_tracer_column_series: one record by hand under the number of the handle's
 * last step; -3 without a recorder or on a full one.  beom_download_tracer_column_series copies the filled records
 * (cols[n][L][cnt], oldest first) and their steps, then sets the count to 0; any of cols, tstp, count may be NULL; -3 without a
 * recorder.  Uploads leave the recorder alone; beom_set_tracers with another count frees it.
 * beom_set_tracer_column_series: level 0 frees; other arguments reallocate and empty; between steps only; -3 for a level
 * outside 0..3, stride < 1, nrec < 1, a window outside 1 <= jlo <= jhi <= M or a handle without tracers.  The recorder is
 * independent of the other three and keeps a scratch of its own: the block partials of a launch stay under 64 MiB, a record
 * being taken in batches of 64-column chunks (option "tracer_column_series_batch", beom_set_option, read by the next
 * beom_set_tracer_column_series: chunks per launch, 0 = by that bound; the bits do not depend on it).  A handle without one
 * launches exactly what it launched before.  beom_info: "tracer_column_series" (the level),
 * "tracer_column_series_records" (records held).  Handles on bands refuse with -6 (beom_multi_*; a handle that is a band of
 * rows): a column's tree crosses the bands.  The Fortran host keeps none. */
int beom_set_tracer_column_series(beom_handle h, int level, int stride, int nrec, int jlo, int jhi, char *errm, int errm_len);
int beom_sample_tracer_column_series(beom_handle h);
int beom_download_tracer_column_series(beom_handle h, double *cols, int *tstp, int *count, char *errm, int errm_len);

/* ---- Several GPUs: the frame cut into bands of rows (SURVEY §8b "Threading", §8e) -------------
 * No reference counterpart (the reference is OpenMP only).  The whole DENSE frame (ndeg = (lm+1)(mm+1))
 * is cut into bands of rows, one band per HIP device, each an ordinary slab handle with 4 ghost rows
 * per neighbour; per time step ONE exchange of hlay,u,v,h_u,h_v (beom_pack_rows -> transport ->
 * beom_unpack_rows on the band's second stream) inside the interior rows of the step's own momentum sweep
 * (beom_step_phase); the steps of one beom_multi_step call run inside the library.  Results are bit-identical to the single handle.
 * Frames periodic in y: the bands form a ring over rows 1..mm and row mm+1 (which nothing points to but
 * every record contains, private_mod.f95:642-668) is carried by a small companion frame next to band 0.
 *
 * Transports of the exchange: */
#define BEOM_XCHG_PEER 0     /* hipMemcpyPeerAsync between the bands of ONE process (xGMI peer copies)      */
#define BEOM_XCHG_RCCL 1     /* grouped ncclSend/ncclRecv (librccl.so.1, bound at run time): all bands in one
                                process (ncclCommInitAll, distinct devices) or one band per process          */
#define BEOM_XCHG_SHM  2     /* one band per process, the processes on ONE node: the packed ghost rows are staged through a
                                POSIX shared-memory segment, in the same stream order as the RCCL send/recv (device -> segment,
                                publish; wait for the neighbour, segment -> device).  Unlike RCCL it lets several ranks share
                                a device: the -m gpu tests run 2 and 3 ranks of beom_multi_create_local on one GPU this way  */
#define BEOM_XCHG_LOOPBACK 0x200 /* flag for beom_multi_create_local_ex: the band receives what it sends itself (its own edge
                                rows arrive as its ghost rows).  ONE band of a frame cut nb ways then runs alone with the
                                whole exchange machinery — a timing rehearsal; the values are not the frame's              */
#define BEOM_XCHG_RING1 0x100 /* flag for beom_multi_create_ex: cut a frame periodic in y as a ring even when
                                there is ONE band (it then exchanges with itself; exercises the ring form)   */

typedef struct beom_multi *beom_multi_handle;

/* no_gradient_obc (mcbc = 0) on a frame cut into bands: beom_set_open_boundaries' table with GLOBAL cell indices; the
 * library deals the segments to the bands (a pass of a segment goes to every band whose rows hold both its updated and its
 * source cell).  Handles created from the global arrays (beom_multi_create[_ex]) of a frame not periodic in y; steps of
 * such a handle are not split (the exchange follows the whole step). */
int beom_multi_set_open_boundaries(beom_multi_handle m, int nseg, const int32_t *segm, char *errm, int errm_len);

/* (a) From GLOBAL arrays, all bands in this process — arguments as beom_create / beom_upload_state /
 * beom_download_state / beom_step.  Band k runs on HIP device devices[k] (with peer copies the same device may
 * be named more than once).  This is what the Fortran host under main.f95 uses (BEOM_NGPU); beom_multi_create
 * takes the transport from the environment (BEOM_XCHG=rccl), default peer copies. */
int beom_multi_create(const beom_params *prm, int ndev, const int *devices,
                      const int32_t *neig, const int32_t *subc,
                      const double *mk_u, const double *mk_v, const double *mk_n,
                      const double *mkpe, const double *mkpi,
                      const double *fcor, const double *h_th, const double *h_to,
                      const double *nudg, const double *fnud, const double *hdot,
                      const double *tide, const double *bodf, const double *taus,
                      beom_multi_handle *out, char *errm, int errm_len);
int beom_multi_create_ex(const beom_params *prm, int ndev, const int *devices, int transport_and_flags,
                         const int32_t *neig, const int32_t *subc,
                         const double *mk_u, const double *mk_v, const double *mk_n,
                         const double *mkpe, const double *mkpi,
                         const double *fcor, const double *h_th, const double *h_to,
                         const double *nudg, const double *fnud, const double *hdot,
                         const double *tide, const double *bodf, const double *taus,
                         beom_multi_handle *out, char *errm, int errm_len);
int beom_multi_destroy(beom_multi_handle h);
int beom_multi_count(beom_multi_handle h);       /* bands of this process */
/* band k: owned global rows own0..own1; local window = rows win0..win1 (1-based, inclusive; in a ring
 * win0 <= 0 and win1 > mm denote wrapped ghost rows); device */
int beom_multi_band(beom_multi_handle h, int k, int *own0, int *own1, int *win0, int *win1, int *device);
int beom_multi_upload_state(beom_multi_handle h,
                            const double *hlay, const double *u, const double *v,
                            const double *h_u, const double *h_v,
                            const double *rs_h, const double *dmdx, const double *dmdy,
                            const double *v_cc, const double *v_ll,
                            const double *tt3d, const double *tb3d, const double *tu3d,
                            char *errm, int errm_len);
int beom_multi_download_state(beom_multi_handle h,
                              double *hlay, double *u, double *v, double *h_u, double *h_v,
                              double *rs_h, double *dmdx, double *dmdy,
                              double *v_cc, double *v_ll,
                              double *tt3d, double *tb3d, double *tu3d,
                              char *errm, int errm_len);
/* as beom_download_outputs / beom_download_diag: GLOBAL (ndeg, nlay) real*4 records, every band forming its own rows on
 * its device (h_0 is needed on every call here); global-array handles only */
int beom_multi_download_outputs(beom_multi_handle h, const float *h0r4, float *eta, float *u4, float *v4,
                                double *minmax, int *thin_layer, char *errm, int errm_len);
int beom_multi_download_diag(beom_multi_handle h, float *pvor, float *mont, float *v_cc, char *errm, int errm_len);
int beom_multi_step(beom_multi_handle h, int tstp_first, int nsteps,
                    double tres, double dtd8, double dt_r, double rsta, int n_3d,
                    char *errm, int errm_len);
int beom_multi_sync(beom_multi_handle h, char *errm, int errm_len);
/* how many band-steps were cut boundary first (exchange inside the momentum sweep) and how many ran in one piece */
int beom_multi_stats(beom_multi_handle h, long long *split_band_steps, long long *plain_band_steps);
/* "overlap" (default 1; 0 = every step runs in one piece, the exchange after it); other names go to every band */
int beom_multi_set_option(beom_multi_handle h, const char *name, int value);
int beom_multi_describe(beom_multi_handle h, int *bands_total, int *bands_local, int *transport, int *ring,
                        int *rccl_version);
/* the slab handle of local band k (k = -1: the companion frame of a ring, NULL if it is not here);
 * owned by the multi handle — for introspection (beom_device_field, beom_set_option), not for stepping */
int beom_multi_engine(beom_multi_handle h, int k, beom_handle *out);
/* as beom_profile_start/stop: per sweep class the slowest local band */
int beom_multi_profile_start(beom_multi_handle h);
int beom_multi_profile_stop(beom_multi_handle h, double *ms, int *launches, char *errm, int errm_len);

/* (b) ONE band per process from that band's WINDOW only (bench.py under torchrun: one process per GPU; nothing
 * of global size exists on any rank).  prm describes the GLOBAL frame; xper/yper say whether it is periodic
 * (with global arrays the library reads that off neig).  The window's rows, south to north:
 *     ghost_s ghost rows | the owned rows own0..own1 | ghost_n ghost rows        (beom_multi_window)
 * (in a ring the ghosts of the first and the last band wrap); every array has the storage of the
 * corresponding beom_create / beom_upload_state argument for a frame of that many rows — index 0 = sentinel,
 * then rows*(lm+1) cells.  No connectivity or mask tables: bands are dense frames, the library generates them.
 * Band 0 of a frame periodic in y also passes row mm+1 ("orphan": index 0 + (lm+1) cells per array).
 * Exchange over RCCL: rccl_id = the 128 bytes beom_rccl_unique_id returned on ONE rank, distributed by the caller
 * (bench.py: through torch.distributed's store); may be NULL when nb = 1. */
typedef struct beom_statics {
    const double *fcor, *h_th, *h_to, *nudg, *fnud, *hdot, *tide, *bodf, *taus;   /* h_to, hdot, tide, bodf, taus may be NULL */
} beom_statics;
typedef struct beom_state {                                                        /* any pointer may be NULL */
    double *hlay, *u, *v, *h_u, *h_v, *rs_h, *dmdx, *dmdy, *v_cc, *v_ll, *tt3d, *tb3d, *tu3d;
} beom_state;
int beom_rccl_unique_id(void *id128, char *errm, int errm_len);
int beom_rccl_version(char *errm, int errm_len);        /* e.g. 22204, or a negative error code */
int beom_multi_window(const beom_params *prm, int nb, int band, int yper,
                      int *own0, int *own1, int *ghost_s, int *ghost_n);
int beom_multi_create_local(const beom_params *prm, int nb, int band, int device, int xper, int yper,
                            const void *rccl_id, const beom_statics *window, const beom_statics *orphan,
                            beom_multi_handle *out, char *errm, int errm_len);
/* The same with the transport named: BEOM_XCHG_RCCL (xchg_id = the 128-byte unique id, as above) or BEOM_XCHG_SHM
 * (xchg_id = NUL-terminated name "/..." of a shared-memory segment, the same on all nb ranks and not in use by any other
 * job; created by whoever comes first, removed again once all nb ranks have attached), optionally | BEOM_XCHG_LOOPBACK. */
int beom_multi_create_local_ex(const beom_params *prm, int nb, int band, int device, int xper, int yper,
                               int transport_and_flags, const void *xchg_id,
                               const beom_statics *window, const beom_statics *orphan,
                               beom_multi_handle *out, char *errm, int errm_len);
/* no_gradient_obc (mcbc = 0) for a handle that holds one band's window: the segments of the window's own rows, as
 * beom_set_open_boundaries takes them, with cell indices of the window (the finder of private_mod.f95:1060-1240 looks at a
 * cell and its four neighbours only, so a rank finds them from its rows alone); band 0 of a frame periodic in y adds those of
 * the orphan row mm+1 (indices of a one-row frame; else 0 / NULL).  nseg = 0: this band holds no segment. */
int beom_multi_set_open_boundaries_local(beom_multi_handle h, int nseg, const int32_t *segm, int nseg_orphan, const int32_t *segm_orphan,
                                         char *errm, int errm_len);
int beom_multi_upload_local(beom_multi_handle h, const beom_state *window, const beom_state *orphan,
                            char *errm, int errm_len);
int beom_multi_download_local(beom_multi_handle h, beom_state *window, beom_state *orphan,
                              char *errm, int errm_len);

/* Passive tracers on a frame cut into bands (see beom_set_tracers): GLOBAL arrays, handles created from the global arrays
 * (beom_multi_create[_ex]) of a frame not periodic in y.  q travels with hlay, u, v, h_u, h_v in the one exchange of a step
 * (the sweep reaches one row; the exchange buffers are reallocated here); cut steps stay cut.  Refused with -6: a frame
 * periodic in y (the ring's companion frame does not carry q yet) and handles that hold one band's window
 * (beom_multi_create_local*: their shared-memory segment and RCCL counts are sized at creation). */
int beom_multi_set_tracers(beom_multi_handle m, int ntrc, char *errm, int errm_len);
/* beom_set_tracer_scheme on every band.  Scheme 2 reaches two rows; the four ghost rows and the exchange of q suffice, so
 * cut steps stay cut and no buffer changes.  (beom_multi_set_tracers refuses rings and rank-local handles as before.) */
int beom_multi_set_tracer_scheme(beom_multi_handle m, int scheme, char *errm, int errm_len);
/* beom_set_tracer_mixing with the same coefficients on every band.  The mixing reaches one row, in front of a sweep that
 * reaches one or two: the four ghost rows still suffice, cut steps stay cut and no buffer changes.  Rings and rank-local
 * handles are refused with -6, as by beom_multi_set_tracers. */
int beom_multi_set_tracer_mixing(beom_multi_handle m, const double *kappa, const double *decay, const double *source, char *errm, int errm_len);
/* beom_set_tracer_vmixing with the same coefficients on every band; band 0 looks at them before any band is touched.  A
 * column reads its own cell only: every band's launch covers its whole window, ghost rows included, which hold the
 * neighbour's values bit for bit and so come out bit for bit; cut steps stay cut and no buffer changes.  Rings and
 * rank-local handles are refused with -6, as by beom_multi_set_tracers. */
int beom_multi_set_tracer_vmixing(beom_multi_handle m, const double *kappa_v, char *errm, int errm_len);
int beom_multi_upload_tracers(beom_multi_handle m, const double *q, const double *rq, const double *ctrg, char *errm, int errm_len);
int beom_multi_download_tracers(beom_multi_handle m, double *q, double *rq, char *errm, int errm_len);

/* Moments on a frame cut into bands (see beom_set_moments): GLOBAL arrays assembled from every band's OWNED rows, handles
 * created from the global arrays (beom_multi_create[_ex]), chains and rings; the bits are a single handle's.  A band's sample
 * of step t is placed where its main stream has joined the exchange of that step (in front of step t + 1, and once more
 * behind the last step of a beom_multi_step call), so cut steps stay cut and no stream hop is added.  A ring's row mm+1 comes
 * from the companion frame, which accumulates its own moments.  Refused with -6: handles that hold one band's window
 * (beom_multi_create_local*). */
int beom_multi_set_moments(beom_multi_handle m, int level, int stride, char *errm, int errm_len);
int beom_multi_reset_moments(beom_multi_handle m, char *errm, int errm_len);
int beom_multi_download_moments(beom_multi_handle m, double *ref, double *sum, double *sq, long long *count, int *tstp_first,
                                int *tstp_last, char *errm, int errm_len);

/* Harmonics on a frame cut into bands (see beom_set_harmonics): GLOBAL ref and sum assembled from every band's OWNED rows
 * through the moments' path, chains and rings; the bits are a single handle's.  Every band accumulates over its whole window
 * and is sampled with beom_sample_harmonics(h, tres + dtd8*(double)t) exactly where the bands' moments are sampled (in front
 * of step t + 1, and once more behind the last step of a beom_multi_step call), so cut steps stay cut and beom_multi_stats
 * is what it is without harmonics.  gram, omega, count and the step numbers come from band 0 (every band holds the same).
 * A ring's row mm+1 comes from the companion frame, which samples behind its own steps.  Refused with -6: handles that
 * hold one band's window (beom_multi_create_local*). */
int beom_multi_set_harmonics(beom_multi_handle m, int nfreq, const double *omega, int level, int stride, char *errm, int errm_len);
int beom_multi_reset_harmonics(beom_multi_handle m, char *errm, int errm_len);
int beom_multi_download_harmonics(beom_multi_handle m, double *ref, double *sum, double *gram, double *omega, long long *count,
                                  int *tstp_first, int *tstp_last, char *errm, int errm_len);

/* Forcing in time on a frame cut into bands (see beom_set_forcing): GLOBAL frames, handles created from the global arrays
 * (beom_multi_create[_ex]), chains with and without land, and rings.  Every frame is cut into the bands' windows exactly as
 * beom_multi_create cuts taus and hdot; a ring's companion frame gets its rows the same way.  Each band interpolates its own
 * window, ghost rows included, at the top of its step (phase 1 of a cut step), so cut steps stay cut, beom_multi_stats is
 * what it is for a steady handle, and the bits are a single handle's.  The arguments are checked on the global arrays
 * before any band is touched (-3).  beom_multi_download_forcing assembles the bands' OWNED rows.  Refused with -6: handles
 * that hold one band's window (beom_multi_create_local*). */
int beom_multi_set_forcing(beom_multi_handle m, int field, int nfr, const double *times, double period, const double *frames,
                           char *errm, int errm_len);
int beom_multi_download_forcing(beom_multi_handle m, double *taus, double *hdot, char *errm, int errm_len);

/* Tracer moments on a frame cut into bands (see beom_set_tracer_moments): GLOBAL arrays assembled from every band's OWNED
 * rows; the bits are a single handle's.  Every band samples over its whole window where the bands' field moments are sampled:
 * behind the wait for the landed ghost rows, so the S row of a band's first owned row holds the neighbour's owned values.
 * Refused with -6, as tracers themselves are: bands of a frame periodic in y (a ring) and handles that hold one band's
 * window (beom_multi_create_local*). */
int beom_multi_set_tracer_moments(beom_multi_handle m, int level, int stride, char *errm, int errm_len);
int beom_multi_reset_tracer_moments(beom_multi_handle m, char *errm, int errm_len);
int beom_multi_download_tracer_moments(beom_multi_handle m, double *ref, double *sum, double *sq, long long *count, int *tstp_first,
                                       int *tstp_last, char *errm, int errm_len);

/* ---- Floats on bands (see beom_set_floats): Lagrangian floats on a frame cut into bands, every handle of
 * beom_multi_create[_ex] (all bands in one process, any transport): chains with and without land, rings, a ring of one band.
 * The positions are bit for bit a single handle's.
 *   Replicated slots: every band holds the arrays of ALL n floats — x, y in GLOBAL grid units, layer, rejected, k1x, k1y,
 *   xs, ys; slot t is float t on every band.  Owner test: in a float launch a band's thread t acts only if the home row
 *   floor(y[t]) + 1 is one of the band's owned rows; every other lane reads y[t] and leaves.  a, b, the wraps and every sum
 *   are formed from the global x, y as on a single handle; only the integer row of a lookup is translated into the window
 *   (modulo mm on a ring; a row the window holds twice is taken where it is owned).  No row offset is ever subtracted from y.
 *   Hand-over: K steps still cost K + 1 launches per band.  The launch behind step n finishes stage 2 for the band's floats
 *   and runs stage 1 of step n + 1 on the new position even when that lies outside the band's rows: with cdt |u|, cdt |v| < 1
 *   every lookup stays within 2 rows of the owned rows, and the 4 ghost rows hold the neighbour's owned values bit for bit.
 *   For such a float the band appends one RECORD to its south or north OUTBOX (atomicAdd on a count in front of the records):
 *     64 bytes = 8 words of 8 bytes: id, x, y, k1x, k1y, xs, ys (FP64 bits), rejected (int32 in the low half);
 *     an outbox = the count at byte 0, record r at byte 64 (r + 1), `capacity` records.
 *   The neighbour copies the outbox (hipMemcpyPeerAsync, count and capacity records) into an inbox and one k_floats_ingest
 *   launch (capacity threads per inbox; thread i < count writes record i into slot id) takes them in; the order of records is
 *   not deterministic, the result is (slot = id, no float depends on another).  Bands are coupled by stream events only: a
 *   copy waits for the sender's float launch; the ingest, which also empties the band's own outboxes, waits for the
 *   neighbours' copies of them.  The launch of step n sits on each band's main stream where it has joined the exchange of
 *   step n (in front of everything of step n + 1 that writes u, v; once more, as stage 2 alone, behind the last step of a
 *   beom_multi_step call; stage 1 alone in front of the first).  A handle without floats launches what it launched before.
 *   Two conditions are COUNTED on the device and refuse beom_multi_download_floats:
 *     BEOM_ERR_FLOAT_REACH     "out of reach": a lookup's row lies in the frame but outside the band's window (cdt |v| >= 1).
 *                              The lane reads nothing outside the window: the cell counts as 0.
 *     BEOM_ERR_FLOAT_OVERFLOW  an outbox was full and a record was dropped (more than `capacity` floats left a band
 *                              through one side in one step).
 *   and BEOM_ERR_FLOAT_CLAIM if a float is claimed (owner test on each band's own y) by other than exactly one band; stale
 *   copies point outside their band, so exactly one band claims.
 * beom_multi_set_floats: n floats (0 frees them), capacity records per outbox (0 = the default max(4096, n / 8)).  Refused
 * with -6: handles that hold one band's window (beom_multi_create_local*): a float would have to travel between processes.
 * There is no track recorder on bands.  One band that is the whole frame forwards to beom_set_floats etc.
 * beom_multi_upload_floats: all or nothing as beom_upload_floats; every band checks the floats of its rows; the error (-3)
 * names the smallest offending index over all bands: a layer outside 1..nlay, a dry start, or a float in no band's rows.
 * beom_multi_download_floats takes every slot from its claimant.  beom_multi_update_floats: the per-sweep entry (stage 1 | 2
 * on the state as it stands; the hand-over behind stage 2).  beom_info on a band's handle: "floats", "float_launches",
 * "float_handovers" (records the band has ingested, as of the latest download).
 * The beom_band_floats_* calls are the band-side pieces beom_multi_* is built from (a band = a dense slab handle): allocate
 * for the rows own0..own0+nown-1 behind ghost_s ghost rows; check candidates / commit them; one float launch (mode 1, 2 or
 * 3 = 2 then 1) or one ingest on the handle's stream; the four boxes' device addresses; the band's copy and its counts
 * (stats3 = out of reach, dropped, ingested). */
#define BEOM_ERR_FLOAT_REACH    (-41)
#define BEOM_ERR_FLOAT_OVERFLOW (-42)
#define BEOM_ERR_FLOAT_CLAIM    (-43)
int beom_multi_set_floats(beom_multi_handle m, int64_t n, int capacity, char *errm, int errm_len);
int beom_multi_upload_floats(beom_multi_handle m, const double *x, const double *y, const int32_t *layer, char *errm, int errm_len);
int beom_multi_download_floats(beom_multi_handle m, double *x, double *y, int32_t *layer, int32_t *rejected, char *errm, int errm_len);
int beom_multi_update_floats(beom_multi_handle m, int stage);
int beom_band_floats_set(beom_handle h, int64_t n, int capacity, int own0, int nown, int ghost_s, int has_south, int has_north,
                         int frame_mm, int xper, int ring, char *errm, int errm_len);
int beom_band_floats_check(beom_handle h, const double *x, const double *y, unsigned long long *first_dry, char *errm, int errm_len);
int beom_band_floats_commit(beom_handle h, const int32_t *layer, char *errm, int errm_len);
int beom_band_floats_launch(beom_handle h, int mode);
int beom_band_floats_ingest(beom_handle h);
int beom_band_floats_boxes(beom_handle h, void **out_s, void **out_n, void **in_s, void **in_n, size_t *bytes);
int beom_band_floats_download(beom_handle h, double *x, double *y, int32_t *layer, int32_t *rejected, unsigned long long *stats3,
                              char *errm, int errm_len);

/* Conservation integrals (see beom_integrals).  Global-array handles: every band forms the row sums of its OWNED rows; a
 * ring's row mm+1 duplicates row 1 and is all +0, so the companion frame is not asked; combined in global row order. */
int beom_multi_integrals(beom_multi_handle m, double *out, char *errm, int errm_len);
/* one band per process: the row sums of this band's owned rows own0..own1 (rows[(j-own0)*count + k]); the caller gathers the
 * bands' rows in global row order (row mm+1 of a frame periodic in y: zeros) and combines with beom_integral_combine */
int beom_multi_integral_rows_local(beom_multi_handle m, int *own0, int *own1, double *rows, char *errm, int errm_len);

/* Series (see beom_set_series).  Global-array handles: every band records its OWNED rows; the record is taken on the band's
 * main stream behind the wait for that step's ghost rows, where the tracer-moment sample sits, so the S neighbours of a
 * band's first owned row are landed ghosts; cut steps stay cut.  beom_multi_step refuses with -3, before launching anything,
 * a call whose steps would overflow the recorder.  beom_multi_download_series places the bands' rows at their global rows:
 * rows[n][mm+1][cnt]; row mm+1 of a frame periodic in y is the duplicated row, all +0.0 (the companion frame is not asked).
 * Chains with and without land, and rings.  -6 for handles that hold one band's window (beom_multi_create_local*): their
 * rows are nowhere assembled.  One band that is the whole frame forwards to beom_set_series etc. */
int beom_multi_set_series(beom_multi_handle m, int level, int stride, int nrec, char *errm, int errm_len);
int beom_multi_download_series(beom_multi_handle m, double *rows, int *tstp, int *count, char *errm, int errm_len);

/* Column series (see beom_set_column_series): both refuse with -6 and say why; a column's tree crosses the bands. */
int beom_multi_set_column_series(beom_multi_handle m, int level, int stride, int nrec, int jlo, int jhi, char *errm, int errm_len);
int beom_multi_download_column_series(beom_multi_handle m, double *cols, int *tstp, int *count, char *errm, int errm_len);

/* Maps (see beom_set_maps): both refuse with -6 and say why; a block's tree must not cross a seam between bands. */
int beom_multi_set_maps(beom_multi_handle m, int level, int block, int stride, int nrec, char *errm, int errm_len);
int beom_multi_download_maps(beom_multi_handle m, double *maps, int *tstp, int *count, char *errm, int errm_len);

/* Tracer column series (see beom_set_tracer_column_series): both refuse with -6 and say why; a column's tree crosses the bands. */
int beom_multi_set_tracer_column_series(beom_multi_handle m, int level, int stride, int nrec, int jlo, int jhi, char *errm, int errm_len);
int beom_multi_download_tracer_column_series(beom_multi_handle m, double *cols, int *tstp, int *count, char *errm, int errm_len);

/* Tracer series (see beom_set_tracer_series), placed like the series: every band records its OWNED rows on its main stream
 * behind the wait for that step's ghost rows, so q(S) and hlay(S) of a band's first owned row are landed ghosts; cut steps
 * stay cut and beom_multi_stats is the same with and without it.  beom_multi_step refuses an overflowing call with -3 before
 * launching anything.  The download places the bands' rows at their global rows: rows[n][mm+1][cnt].  -6 where the bands
 * carry no tracers (rings, handles that hold one band's window), -3 without tracers.  One band that is the whole frame
 * forwards to beom_set_tracer_series etc. */
int beom_multi_set_tracer_series(beom_multi_handle m, int level, int stride, int nrec, char *errm, int errm_len);
int beom_multi_download_tracer_series(beom_multi_handle m, double *rows, int *tstp, int *count, char *errm, int errm_len);

#ifdef __cplusplus
}
#endif
#endif /* BEOM_HIP_H */
