/*
 * lbl_amd.h -- C ABI of the MI355X (gfx950) molecular-lines engine.
 *
 * This is the drop-in boundary for the lines backend of GRIPS-code/pyLBL: the one
 * native entry point the reference binds over ctypes is
 *
 *     int absorption(double pressure, double temperature, double volume_mixing_ratio,
 *                    int v0, int vn, int n_per_v, double *k, char *database,
 *                    char *formula, int cut_off, int remove_pedestal);
 *                                        (pyLBL/c_lib/absorption.c:19-30, bound at
 *                                         pyLBL/c_lib/gas_optics.py:68-91)
 *
 * That call re-opens the SQLite file, re-reads every transition of the molecule and
 * computes ONE (level, molecule) spectrum on one CPU thread.  The replacement splits it
 * into (1) a one-time upload of a molecule's line table to HBM and (2) a batched compute
 * call over many atmospheric levels, and keeps a same-signature compatibility entry.
 *
 * Conventions: plain C types only; every function returns LBL_OK (0) or a non-zero
 * status and never throws; the message for the last failure on a handle is available
 * from lbl_last_error().  All arrays are caller-owned; "host" pointers are ordinary
 * process memory, "device" pointers are HIP device allocations on the engine's GPU.
 *
 * Threads: every entry point may be called from any number of threads on the SAME handle at
 * once, as the reference's absorption() may (no globals or statics, absorption.c:19-99; ctypes
 * releases the GIL around it, gas_optics.py:79-91).  A handle serialises the host side of its
 * calls -- queueing work is microseconds -- with a mutex of its own; a blocking call waits for
 * its result after it has released that mutex, so other threads' calls queue up behind it on
 * the GPU meanwhile, and each call returns exactly what it would have returned alone.
 * lbl_last_error() returns the calling thread's own last message.  What stays with the caller:
 * output blocks that several asynchronous calls share (LBL_ACCUMULATE) see those calls in the
 * order they were made, so threads that add into ONE block without ordering themselves get the
 * sum in a nondeterministic order of additions; and there is one deferred call per handle
 * (LBL_DEFER_FINISH) -- a pipeline that defers should not share its handle with other threads
 * while it does (pylbl_amd.Spectroscopy holds a lock per engine for that).  Distinct handles
 * are independent.
 */
#ifndef LBL_AMD_H_
#define LBL_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBL_OK              0
#define LBL_ERROR           1   /* generic failure (message in lbl_last_error)            */
#define LBL_BAD_ARGUMENT    2
#define LBL_NO_DEVICE       3   /* no usable gfx950 device / HIP runtime failure           */
#define LBL_OUT_OF_RANGE    4   /* temperature outside the TIPS table, iso id without data  */
/* lbl_table_read / lbl_molecule_load_sqlite: the first thing the file lacks for the molecule, in
 * the order the reference looks things up (absorption.c:50-73) */
#define LBL_TABLE_OPEN_FAILED       10  /* not an SQLite file this process can open            */
#define LBL_TABLE_NO_ALIAS          11  /* spectral_database.c:152-156: the reference's rc 1    */
#define LBL_TABLE_NO_TIPS           12  /* absorption.c:53-59: the reference returns zeros      */
#define LBL_TABLE_NOT_RECTANGULAR   13  /* spectral_database.c:85-90                            */
#define LBL_TABLE_NO_ISOTOPOLOGUES  14
#define LBL_TABLE_NO_TRANSITIONS    15

/* Which rows of the table take part (reference: pyLBL/c_lib/absorption.c:80-83). */
#define LBL_RANGE_REFERENCE 0   /* stop at the first row outside [v0-(cut+1), vn+cut+1]    */
#define LBL_RANGE_SKIP      1   /* ignore out-of-range rows, keep going                     */

/* Where the per-line scalars (shifted centre, widths, strength) are evaluated. */
#define LBL_PREP_DEVICE     0   /* HIP kernel (default)                                     */
#define LBL_PREP_HOST       1   /* host libm, same operation order as spectra.c:17-45       */

/* lbl_compute flags */
#define LBL_OUT_DEVICE      1   /* k is a device pointer                                    */
#define LBL_ASYNC           2   /* return after enqueueing; pair with lbl_synchronize       */
#define LBL_SCALE_DENSITY   4   /* multiply by number density P x /(kb T): the lines slot of
                                   Spectroscopy.compute_absorption (spectroscopy.py:181-191) */
#define LBL_ACCUMULATE      8   /* add into k instead of overwriting it                     */
#define LBL_FARFIELD       16   /* this call: lines at least 4 tile half-widths away (and beyond
                                   every line core) enter through one power series per tile
                                   instead of point by point -- truncation <= ~1.5e-11 relative,
                                   3-4x faster at 0.001 cm-1 (same as option "farfield" = 1);
                                   on grids so coarse that a tile is as wide as a line's window
                                   (0.1 cm-1 and up) nothing is far and the call runs without  */
#define LBL_DEFER_FINISH   32   /* with LBL_ASYNC | LBL_OUT_DEVICE and remove_pedestal: everything
                                 * is queued except the last kernels, which apply the pedestal
                                 * to k (and the copies of lbl_compute_streamed): those wait for
                                 * lbl_finish_deferred (or lbl_synchronize).  A long call can
                                 * then be queued FIRST and still be the LAST to add into a block
                                 * other calls write meanwhile -- the reference's loop has no
                                 * such order to keep, its calls are serial (spectroscopy.py:166).
                                 * One deferred call at a time; ignored where it cannot apply
                                 * (no pedestal, several level passes, host output). */

/* The largest cut_off a call with remove_pedestal accepts (others fail with LBL_BAD_ARGUMENT
 * before any GPU work): the pedestal pre-pass stages 2 x 16 runs of 2 cut_off + 3 slot sums in
 * one workgroup's LDS, 256 (2 cut_off + 3) + 2048 bytes plus 4608 of its own, and a CU has
 * 160 KiB.  Without the pedestal any cut_off >= 0 is accepted. */
#define LBL_MAX_PEDESTAL_CUT_OFF 305

typedef struct lbl_engine lbl_engine;

/* Creates an engine bound to HIP device `device`.  Fails with LBL_NO_DEVICE when the HIP
 * runtime reports no such GPU: there is no CPU fallback. */
int lbl_engine_create(int device, lbl_engine **engine);
int lbl_engine_destroy(lbl_engine *engine);

/* Message of the calling thread's last failure on this handle (of the handle's last failure
 * if this thread has had none; "" if none); engine may be NULL to read the message of a failed
 * lbl_engine_create on the calling thread.  The pointer stays valid until the calling thread's
 * next failure or next call of this function. */
const char *lbl_last_error(const lbl_engine *engine);

/* Uploads one molecule: replaces the per-call SQLite row loop of absorption.c:44-86
 * (tips_data, mass_data, line_parameters of spectral_database.c:49-180).
 *   rows in reference row order; local_iso_id raw (0 means isotopologue 10);
 *   mass[32] indexed isoid-1 (isoid 0 at slot 9);
 *   tips_temperature[num_t]; tips_data[num_iso*num_t] isotopologue-major.
 * On success *molecule receives a small non-negative handle. */
int lbl_molecule_load(lbl_engine *engine, int64_t n_lines,
                      const double *nu, const double *sw, const double *gamma_air,
                      const double *gamma_self, const double *n_air, const double *elower,
                      const double *delta_air, const int32_t *local_iso_id,
                      const double *mass, int32_t num_iso, int32_t num_t,
                      const double *tips_temperature, const double *tips_data,
                      int32_t *molecule);
int lbl_molecule_free(lbl_engine *engine, int32_t molecule);

/* Absorption cross-section spectra [m2 molecule-1] of one molecule at n_levels levels:
 * the batched form of absorption() (absorption.c:19-99).
 *   k: n_levels rows of (vn-v0)*n_per_v doubles, row stride level_stride doubles
 *      (0 means dense); host memory unless LBL_OUT_DEVICE.
 *   evals (optional): sum over accepted lines and levels of last-first+1, the
 *      reference's inner-loop iteration count (spectra.c:48-62), computed in closed form. */
int lbl_compute(lbl_engine *engine, int32_t molecule, int32_t n_levels,
                const double *temperature, const double *pressure, const double *vmr,
                int32_t v0, int32_t vn, int32_t n_per_v, int32_t cut_off,
                int32_t remove_pedestal, int32_t range_policy, int32_t flags,
                double *k, int64_t level_stride, int64_t *evals);

/* lbl_compute into device memory (LBL_OUT_DEVICE required) with the result ALSO delivered to
 * host memory while the call still computes: the grid is worked through in `pieces` runs of
 * tiles (1..8), and the first `columns` points of every level of a finished run are copied to
 * `host` (row l at host + l*host_pitch bytes; page-locked memory from lbl_host_alloc for the
 * copies to overlap) beside the kernels of the next run.  What the reference's callers get --
 * a host array per call (gas_optics.py:65,91) -- without a copy behind the last kernel.  The
 * values are those of lbl_compute (same kernels, same order of additions).  With LBL_ASYNC the
 * copies are complete after lbl_synchronize -- and until then the copied part of `k` must not be
 * written again: the engine orders calls by the memory they WRITE (two calls into one block run
 * in the order they were made), not by what a copy still reads; the same holds for
 * lbl_copy_rows_to_host with LBL_ASYNC.  (An event behind every copy, for later writers to wait
 * for, was measured: it takes the copies' back-to-back rate away, 3.3 -> 3.6 ms for the call that
 * delivers four blocks.) */
int lbl_compute_streamed(lbl_engine *engine, int32_t molecule, int32_t n_levels,
                         const double *temperature, const double *pressure, const double *vmr,
                         int32_t v0, int32_t vn, int32_t n_per_v, int32_t cut_off,
                         int32_t remove_pedestal, int32_t range_policy, int32_t flags,
                         double *k, int64_t level_stride, void *host, int64_t host_pitch,
                         int64_t columns, int32_t pieces);

/* Queues the part of a call that LBL_DEFER_FINISH kept back (no-op without one).  lbl_deferred:
 * 1 while a call is kept back, 0 otherwise -- in particular right after a call whose
 * LBL_DEFER_FINISH could not be honoured and which therefore finished at once. */
int lbl_finish_deferred(lbl_engine *engine);
int lbl_deferred(const lbl_engine *engine);
/* Drops what a call kept back instead of queueing it: the call's target block and host range
 * are then never written by it (what it queued before works in buffers of the engine).  For
 * hosts that fail between a deferred call and its lbl_finish_deferred and are about to release
 * the block.  lbl_copy_to_host, lbl_copy_rows_to_host and lbl_order_stream_after_engine finish a
 * deferred call first (like lbl_synchronize); lbl_device_free and lbl_host_free do so only when
 * the memory they release is memory that call still has to write (its output block, the host
 * range of its delivery) -- a free of anything else, from whichever thread, leaves the deferral
 * and with it the order of a pipeline's additions alone. */
int lbl_cancel_deferred(lbl_engine *engine);

/* Waits for everything enqueued on the engine (all of its streams); a deferred call is finished
 * first. */
int lbl_synchronize(lbl_engine *engine);

/* Zeroes n_levels rows of n doubles (row stride level_stride, 0 = dense) of host memory, or of
 * device memory with LBL_OUT_DEVICE (LBL_ASYNC: queued like a compute call).  What the reference
 * returns for a molecule without partition-function rows or transitions (absorption.c:41,
 * :53-59): hosts use it to give a caller-supplied output buffer those semantics. */
int lbl_fill_zero(lbl_engine *engine, double *k, int32_t n_levels, int64_t n,
                  int64_t level_stride, int32_t flags);

/* Optical depth and transmittance along paths (Spectroscopy.compute_path).  beta is a device
 * block of absorption coefficients [m-1] whose row r (stride row_stride values) is flat level
 * level_begin + r; the levels are n_paths paths of levels_per_path consecutive levels each, and
 * this call covers the run [level_begin, level_begin + level_count) of them.  path_length (host,
 * level_count values [m], finite and >= 0) is each level's length along its path.
 *   tau_p = sum_l s_{p,l} beta_{p,l}, added level by level as tau = tau + s*beta from tau = 0:
 *   upward from the path's first level, or with LBL_PATH_FROM_LAST downward from its last.
 * A path's running tau lives in its row of carry (device, [n_paths][row_stride]) between runs:
 * a run that starts inside a path in sweep order must carry LBL_PATH_CONTINUE, one that starts a
 * path must not.  (The run alone decides this; the flag is there so that a caller who loses
 * track of its runs gets LBL_BAD_ARGUMENT instead of a sum that silently restarts or goes on.)
 * Runs of one sweep are queued in sweep order.  Only the first `columns` values of
 * a row count.
 * Outputs (device; LBL_PATH_OPTICAL_DEPTH -> optical_depth, LBL_PATH_TRANSMITTANCE ->
 * transmittance = exp(-tau), not clamped):
 *   n_bands == 0, per path:         row p of [n_paths][row_stride], written by the run that
 *                                   finishes path p;
 *   n_bands == 0, LBL_PATH_CUMULATIVE: row r of [level_count][row_stride]: tau after level
 *                                   level_begin + r;
 *   n_bands > 0: band b is columns [band_start[b], band_start[b+1]) (host, n_bands + 1
 *                non-decreasing values in [0, columns]); the output is the arithmetic mean over
 *                the band of tau or of exp(-tau), NaN for an empty band, in row p of
 *                [n_paths][n_bands] (per path) or row r of [level_count][n_bands] (cumulative).
 *                With LBL_PATH_CUMULATIVE the run's rows of beta are overwritten by the
 *                cumulative tau, which the means then read.
 * The means are reduced in a fixed order without atomics: repeated calls give the same bits.
 * Ordered like lbl_fill_zero: behind everything queued on the engine; LBL_ASYNC returns after
 * queueing.  LBL_BAD_ARGUMENT (message in lbl_last_error) for NULL pointers, columns > row_stride,
 * bad band starts, negative or non-finite lengths, a run outside the levels or one whose
 * LBL_PATH_CONTINUE does not match it, LBL_PATH_FROM_LAST without LBL_PATH_CUMULATIVE, or no
 * quantity requested; the engine stays usable. */
#define LBL_PATH_OPTICAL_DEPTH  0x100
#define LBL_PATH_TRANSMITTANCE  0x200
#define LBL_PATH_CUMULATIVE     0x400   /* one result per level instead of per path          */
#define LBL_PATH_FROM_LAST      0x800   /* tau over levels l .. L-1, summed from L-1 down     */
#define LBL_PATH_CONTINUE      0x1000   /* the run's first path goes on from its carry row    */
int lbl_path_compute(lbl_engine *engine, double *beta, int64_t row_stride, int64_t columns,
                     int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                     int32_t level_count, const double *path_length, int32_t n_bands,
                     const int64_t *band_start, double *carry, double *optical_depth,
                     double *transmittance, int32_t flags);

/* Thermal emission along paths (Spectroscopy.compute_radiance): the radiance that leaves each
 * path, with the levels as isothermal layers.  beta, row_stride, columns, n_paths,
 * levels_per_path, level_begin, level_count, path_length, carry, band_start / n_bands,
 * LBL_PATH_CUMULATIVE, LBL_PATH_CONTINUE and LBL_ASYNC as for lbl_path_compute; a path's
 * running radiance lives in its carry row between runs.
 *   grid: a handle of lbl_grid_load with at least `columns` points; nu_j is its value j [cm-1].
 *   temperature (host, level_count values [K], finite and > 0): each level's temperature.
 *   boundary_temperature / boundary_emissivity (host, n_paths values each, or NULL for all 0 /
 *   all 1): what enters path p before its first level in sweep order; a boundary temperature of
 *   0 means no source behind the path, emissivities lie in [0, 1].
 * With C1 = LBL_PLANCK_C1 and C2 = LBL_PLANCK_C2 (CODATA 2018 h, c, k, exactly):
 *   B(nu, T) = (((C1*nu)*nu)*nu) / expm1((C2*nu)/T), 0 for nu <= 0  [W m-2 sr-1 (cm-1)-1]
 *   level l, x = s_l*beta_l: t = exp(-x), a = -expm1(-x), source B(nu, T_l) (isothermal layer)
 *   I = eps*B(nu, T_boundary) (0 without a boundary), then I = I*t + B_l*a for every level in
 *   sweep order: upward from the path's first level, or with LBL_PATH_FROM_LAST (allowed here
 *   without LBL_PATH_CUMULATIVE) downward from its last.  Each product and sum rounded as written.
 *   brightness temperature = (C2*nu) / log1p((((C1*nu)*nu)*nu) / I), 0 where I <= 0 or nu <= 0.
 * Outputs (device; LBL_PATH_RADIANCE -> radiance, LBL_PATH_BRIGHTNESS -> brightness_temperature):
 *   n_bands == 0: row p of [n_paths][row_stride], written by the run that finishes path p, or
 *                 with LBL_PATH_CUMULATIVE row r of [level_count][row_stride]: I just after level
 *                 level_begin + r;
 *   n_bands > 0:  the arithmetic mean of I over each band, NaN for an empty band, as
 *                 lbl_path_compute forms it (radiance only: LBL_PATH_BRIGHTNESS with bands is
 *                 LBL_BAD_ARGUMENT).  With LBL_PATH_CUMULATIVE the run's rows of beta are
 *                 overwritten by the cumulative radiance, which the means then read.
 * LBL_BAD_ARGUMENT (message in lbl_last_error) as for lbl_path_compute, and for an unknown or
 * short grid, temperatures that are not finite and > 0, boundary temperatures that are negative
 * or not finite, emissivities outside [0, 1]; the engine stays usable. */
#define LBL_PLANCK_C1  1.1910429723971885e-08  /* 2 h c^2 1e8 [W m-2 sr-1 (cm-1)-4]          */
#define LBL_PLANCK_C2  1.4387768775039338      /* h c / k 1e2 [cm K]                          */
#define LBL_PATH_RADIANCE      0x2000
#define LBL_PATH_BRIGHTNESS    0x4000   /* brightness temperature [K]                        */
int lbl_path_radiance(lbl_engine *engine, double *beta, int64_t row_stride, int64_t columns,
                      int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                      int32_t level_count, const double *path_length, const double *temperature,
                      const double *boundary_temperature, const double *boundary_emissivity,
                      int32_t n_bands, const int64_t *band_start, double *carry, double *radiance,
                      double *brightness_temperature, int32_t flags);

/* Longwave fluxes (Spectroscopy.compute_flux): one sweep of n_angles radiances (1..8) through a
 * run of levels, down from space or, with LBL_PATH_FLUX_UP, up from a Lambertian surface.  beta,
 * row_stride, columns, grid, n_paths, levels_per_path, level_begin, level_count, temperature,
 * band_start / n_bands, LBL_PATH_FROM_LAST, LBL_PATH_CONTINUE and LBL_ASYNC as for
 * lbl_path_radiance (the sweep order sets LBL_PATH_FROM_LAST: the down sweep of a path whose
 * surface is its first level runs from its last).
 *   path_length (host, [level_count][n_angles], finite and >= 0): s_l/mu_k, each level's
 *   length along angle k [m]; weight (host, n_angles values, finite and >= 0): w_k.
 *   surface_temperature / surface_emissivity (host, n_paths values each; read by the up sweep
 *   alone, may be NULL on the down sweep): T_s finite and > 0, eps in [0, 1].
 * With B as in lbl_path_radiance, each product and sum rounded as written, sums from k = 0:
 *   x = s_{l,k}*beta_l, I_k = I_k*exp(-x) + B(nu, T_l)*(-expm1(-x)) for every level in sweep order;
 *   down: I_k = 0 at the path's start; the run that finishes a path writes R = sum_k w_k*I_k to
 *   its row of reflection (device, [n_paths][row_stride]);
 *   up: I_k = eps*B(nu, T_s) + (1 - eps)*R at the path's start, and the run that starts a path
 *   replaces R in its row of reflection by the flux at the surface interface;
 *   F = pi*(sum_k w_k*I_k), pi = 3.141592653589793.
 * The K radiances of a path live in carry (device, [n_paths][n_angles][row_stride]) between runs.
 * Outputs (device): level_flux [level_count][row_stride] (not beta): row r is F just after level
 * level_begin + r.  With n_bands > 0 also the band means of lbl_path_compute: of the level rows
 * in flux [level_count][n_bands], and on the up sweep of the surface rows of the paths the run
 * starts in surface_flux [n_paths][n_bands].
 * LBL_BAD_ARGUMENT (message in lbl_last_error) as for lbl_path_radiance, and for n_angles outside
 * 1..8, lengths or weights that are negative or not finite, surface temperatures that are not
 * finite and > 0 or emissivities outside [0, 1] on the up sweep, level_flux == beta, or a band
 * output that is NULL; the engine stays usable. */
#define LBL_PATH_FLUX_UP      0x8000    /* the up sweep: from the surface toward space        */
int lbl_path_flux(lbl_engine *engine, double *beta, int64_t row_stride, int64_t columns,
                  int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                  int32_t level_count, int32_t n_angles, const double *path_length,
                  const double *weight, const double *temperature,
                  const double *surface_temperature, const double *surface_emissivity,
                  int32_t n_bands, const int64_t *band_start, double *carry, double *reflection,
                  double *level_flux, double *flux, double *surface_flux, int32_t flags);

/* lbl_path_radiance and lbl_path_flux with a source that is linear in optical depth inside each
 * level (Spectroscopy.compute_radiance / compute_flux with source="linear_in_tau").  Every argument
 * as for lbl_path_radiance / lbl_path_flux, and
 *   edge_temperature (host, [level_count][2] values [K], finite and > 0, or NULL): [r][0] is the
 *   temperature of the interface of level level_begin + r on the side of its path's first level,
 *   [r][1] of the interface on the side of its path's last level.  Inside a path of the run the
 *   table must be continuous, [r][1] == [r + 1][0]: the kernels evaluate Planck once per level, at
 *   the interface the sweep leaves it through, and keep it as the next level's entry value.
 * NULL: the isothermal source, exactly lbl_path_radiance / lbl_path_flux (which are these calls
 * with NULL).  Otherwise `temperature` is still checked but not used for the source, and for a
 * level in sweep order, with B_in = B(nu, T_edge) at the interface the sweep enters it through
 * ([r][0] upward, [r][1] with LBL_PATH_FROM_LAST) and B_out at the one it leaves through:
 *   x = s*beta, t = exp(-x), a = -expm1(-x)
 *   w = 1 - a/x  (x/2 - x^2/6 + x^3/24 - ...; 0 at x = 0),  u_in = a - w
 *   I = I*t + (B_in*u_in + B_out*w)
 * each product and sum rounded as written, with w formed as
 *   |x| <  1/16:  x*(1./2. - x*(1./6. - x*(1./24. - x*(1./120. - x*(1./720. - x*(1./5040.
 *                 - x*(1./40320. - x*(1./362880.))))))))   (8 terms, Horner)
 *   otherwise:    1. - a/x
 * (1 - a/x alone is 0/0 at x = 0 and wrong by 4e-4 relative at x = 1e-12; this form is within
 * 6.2e-15 relative of long double for x from -3 to 1e3).  x = 0 leaves I unchanged bit for bit;
 * negative x gives finite results.  In lbl_path_flux_source B_in and B_out are shared by the
 * angles.  The boundary and surface terms, carry and reflection rows, band means, cumulative rows
 * and LBL_PATH_CONTINUE are those of lbl_path_radiance / lbl_path_flux: a run that continues a
 * path takes B_in of its first level from its own table.
 * LBL_BAD_ARGUMENT as for lbl_path_radiance / lbl_path_flux, and for an edge temperature that is
 * not finite and > 0 or a table that is not continuous within a path; the engine stays usable. */
int lbl_path_radiance_source(lbl_engine *engine, double *beta, int64_t row_stride, int64_t columns,
                             int32_t grid, int32_t n_paths, int32_t levels_per_path,
                             int32_t level_begin, int32_t level_count, const double *path_length,
                             const double *temperature, const double *edge_temperature,
                             const double *boundary_temperature,
                             const double *boundary_emissivity, int32_t n_bands,
                             const int64_t *band_start, double *carry, double *radiance,
                             double *brightness_temperature, int32_t flags);
int lbl_path_flux_source(lbl_engine *engine, double *beta, int64_t row_stride, int64_t columns,
                         int32_t grid, int32_t n_paths, int32_t levels_per_path,
                         int32_t level_begin, int32_t level_count, int32_t n_angles,
                         const double *path_length, const double *weight,
                         const double *temperature, const double *edge_temperature,
                         const double *surface_temperature, const double *surface_emissivity,
                         int32_t n_bands, const int64_t *band_start, double *carry,
                         double *reflection, double *level_flux, double *flux,
                         double *surface_flux, int32_t flags);

/* The lower boundary of Spectroscopy.compute_radiance: a surface with a spectral emissivity that
 * may also reflect the radiance the atmosphere sends down to it.
 *
 * lbl_surface_emissivity fills rows[p][j] = E_p(nu_j) for the paths p in [path_begin, path_begin +
 * path_count) of n_paths, nu_j the points of `grid` (a handle of lbl_grid_load, ascending or not):
 *   knot_wavenumber (host, n_knots values k_0 < ... < k_{M-1} [cm-1], finite, 2 <= M <= 1024);
 *   knot_emissivity (host, [path_count][n_knots], every value in [0, 1]): e_0 .. e_{M-1} of each
 *   path of the call;
 *   for k_j <= nu < k_{j+1}:  E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)),
 *   E = e_0 for nu <= k_0,  E = e_{M-1} for nu >= k_{M-1}
 * -- numpy.interp: constant outside the knots, linear inside; each operation rounded as written,
 * so a flat table e_j = c gives E = c exactly.
 *   rows (device, [n_paths][row_stride], row_stride >= the grid's points): row p receives the
 *   grid's points, the padding is left alone.  flags: LBL_ASYNC or 0.
 * LBL_BAD_ARGUMENT (message in lbl_last_error) for knots that are not finite and strictly
 * ascending, emissivities outside [0, 1], n_knots outside 2..1024, an unknown grid, a row_stride
 * below the grid's points or paths outside n_paths; nothing is launched and the engine stays usable.
 *
 * lbl_path_radiance_surface is lbl_path_radiance_source with two more device pointers, read where
 * a path starts in the run (a run under LBL_PATH_CONTINUE takes its carry row as always):
 *   emissivity_rows ([n_paths][row_stride], e.g. lbl_surface_emissivity's rows, or NULL: E is the
 *   path's scalar boundary_emissivity);
 *   reflection ([n_paths][row_stride]: D, the radiance that arrives at the boundary of each path,
 *   or NULL: nothing is reflected).
 * A path behind a boundary (boundary temperature T_b > 0) starts from
 *   I = E*B(nu, T_b) + (1. - E)*D        (I = E*B(nu, T_b) with reflection == NULL)
 * each product and sum rounded as written, and goes on level by level as in
 * lbl_path_radiance_source; a path without a boundary starts from 0.  With both pointers NULL the
 * call is lbl_path_radiance_source bit for bit (the same kernels).  D is what a sweep against the
 * direction leaves at the boundary: lbl_path_radiance_source with boundary_temperature NULL, the
 * opposite LBL_PATH_FROM_LAST, the lengths of the reflected path (the same lengths: specular
 * reflection in a plane-parallel atmosphere; 1.66 times the layer thickness: the diffusivity
 * approximation of a Lambertian surface) and `reflection` as its per-path radiance output.
 * LBL_BAD_ARGUMENT as for lbl_path_radiance_source, and when reflection is given and a path of the
 * run has boundary temperature 0 (or boundary_temperature is NULL); the engine stays usable. */
int lbl_surface_emissivity(lbl_engine *engine, int32_t grid, int32_t n_paths, int32_t path_begin,
                           int32_t path_count, int32_t n_knots, const double *knot_wavenumber,
                           const double *knot_emissivity, double *rows, int64_t row_stride,
                           int32_t flags);
int lbl_path_radiance_surface(lbl_engine *engine, double *beta, int64_t row_stride,
                              int64_t columns, int32_t grid, int32_t n_paths,
                              int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                              const double *path_length, const double *temperature,
                              const double *edge_temperature,
                              const double *boundary_temperature,
                              const double *boundary_emissivity, int32_t n_bands,
                              const int64_t *band_start, double *carry, double *radiance,
                              double *brightness_temperature, int32_t flags,
                              const double *emissivity_rows, const double *reflection);

/* Analytic radiance Jacobians (Spectroscopy.compute_jacobian): the derivatives of
 * lbl_path_radiance's radiance with respect to the state of every level and of the boundary, for
 * a run of whole paths.  beta (read only), row_stride, columns, grid, n_paths, levels_per_path,
 * level_begin, level_count, path_length, temperature, boundary_temperature, boundary_emissivity,
 * band_start / n_bands, LBL_PATH_FROM_LAST and LBL_ASYNC as for lbl_path_radiance.  The run must
 * consist of whole paths (level_begin and level_count multiples of levels_per_path): there is no
 * carry, and LBL_PATH_CONTINUE and LBL_PATH_CUMULATIVE must not be set.
 * For one path and one grid point nu, with the levels numbered k = 0 .. L-1 in sweep order (k = 0
 * is the path's first level, or with LBL_PATH_FROM_LAST its last), each product and sum rounded
 * as written:
 *   x_k = s_k*beta_k, t_k = exp(-x_k), a_k = -expm1(-x_k), B_k = B(nu, T_k);
 *   forward, exactly lbl_path_radiance's: I_-1 = eps*B(nu, T_b) (0 without a boundary),
 *     I_k = I_{k-1}*t_k + B_k*a_k; the radiance is I_{L-1};
 *   trailing optical depth, summed from the observer backwards: tau'_{L-1} = 0, then
 *     tau'_{k-1} = tau'_k + s_k*beta_k for k = L-1 .. 0; trail_k = exp(-tau'_k),
 *     trail_b = exp(-tau'_{-1});
 *   dB(nu, T): with u = (C2*nu)/T and B = B(nu, T), dB = (B*(u/T))*(1. + B/(((C1*nu)*nu)*nu)),
 *     0 for nu <= 0 (B/(C1 nu^3) is 1/expm1(u): dB/dT without a second expm1).
 * Outputs (device), each chosen by its flag:
 *   LBL_PATH_RADIANCE              radiance                      I_{L-1}, bit for bit
 *                                                                lbl_path_radiance's
 *   LBL_PATH_JACOBIAN_DEPTH        optical_depth_jacobian        dI/dx_k = (B_k - I_k)*trail_k
 *   LBL_PATH_JACOBIAN_LOG_DEPTH    log_optical_depth_jacobian    dI/dln x_k
 *                                                                = x_k*((B_k - I_k)*trail_k)
 *   LBL_PATH_JACOBIAN_TEMPERATURE  temperature_jacobian          dI/dT_k at fixed beta
 *                                                                = (a_k*dB(nu, T_k))*trail_k
 *   LBL_PATH_JACOBIAN_BOUNDARY_T   boundary_temperature_jacobian (eps*dB(nu, T_b))*trail_b
 *   LBL_PATH_JACOBIAN_BOUNDARY_E   boundary_emissivity_jacobian  B(nu, T_b)*trail_b
 * The three per-level ones fill row r of [level_count][row_stride] (flat level level_begin + r),
 * the radiance and the boundary Jacobians row p of [n_paths][row_stride], for the paths of the
 * run.  The dependence of beta on the state is the caller's to chain: s_k*dbeta_k/dq times
 * optical_depth_jacobian.
 *   work (device): n_bands == 0: [level_count][row_stride], the trail_k between the kernel's two
 *     loops; optical_depth_jacobian or log_optical_depth_jacobian (one of them) may be `work`
 *     itself.  n_bands > 0: [max(P, 1)*level_count + Q*paths][row_stride] with P the per-level
 *     and Q the per-path quantities requested and `paths` those of the run: the fine rows of
 *     every quantity, whose band means (as lbl_path_compute forms them, NaN for an empty band)
 *     go to row r of [level_count][n_bands] or row p of [n_paths][n_bands] of the outputs.
 * LBL_BAD_ARGUMENT (message in lbl_last_error) as for lbl_path_radiance, and for a run that does
 * not consist of whole paths, LBL_PATH_CONTINUE or LBL_PATH_CUMULATIVE, a boundary Jacobian
 * requested for a path of the run whose boundary temperature is 0, a requested output that is
 * NULL, an output other than those two that is `work`, or no quantity requested; nothing is
 * launched and the engine stays usable. */
#define LBL_PATH_JACOBIAN_DEPTH        0x10000
#define LBL_PATH_JACOBIAN_LOG_DEPTH    0x20000
#define LBL_PATH_JACOBIAN_TEMPERATURE  0x40000
#define LBL_PATH_JACOBIAN_BOUNDARY_T   0x80000
#define LBL_PATH_JACOBIAN_BOUNDARY_E  0x100000
int lbl_path_jacobian(lbl_engine *engine, const double *beta, int64_t row_stride, int64_t columns,
                      int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                      int32_t level_count, const double *path_length, const double *temperature,
                      const double *boundary_temperature, const double *boundary_emissivity,
                      int32_t n_bands, const int64_t *band_start, double *work, double *radiance,
                      double *optical_depth_jacobian, double *log_optical_depth_jacobian,
                      double *temperature_jacobian, double *boundary_temperature_jacobian,
                      double *boundary_emissivity_jacobian, int32_t flags);

/* Instrument line shapes (Spectroscopy.compute_path / compute_radiance with `instrument`): N
 * channels, each a weighted mean of a row of fine-grid values under its line shape.
 * lbl_instrument_create binds an instrument to a grid (a handle of lbl_grid_load, ascending):
 * it checks the arguments, computes every channel's window columns on the host in fp64 and
 * uploads its tables with a copy of the grid in one staged copy.  The handle holds no reference
 * to the grid afterwards.  With Delta = nu_j - nu_c (host arrays of n_channels values, the
 * per-channel `parameter` and `half_width` finite and > 0):
 *   LBL_INSTRUMENT_BOXCAR     w = 1,                          window nu_c -/+ parameter/2
 *   LBL_INSTRUMENT_TRIANGLE   w = 1 - |Delta|/parameter,      window nu_c -/+ parameter
 *   LBL_INSTRUMENT_GAUSSIAN   w = exp(-G*((Delta/parameter)*(Delta/parameter))), G = 4 ln 2,
 *                                                             window nu_c -/+ half_width
 *   LBL_INSTRUMENT_FTS        w = S(Delta) = sinc(2 L Delta), L = parameter (max path
 *                             difference [cm]), sinc(x) = sin(pi x)/(pi x), sinc(0) = 1,
 *                                                             window nu_c -/+ half_width
 *   LBL_INSTRUMENT_FTS_HAMMING w = 0.54 S(Delta) + 0.23 (S(Delta - 1/(2L)) + S(Delta + 1/(2L)))
 *   LBL_INSTRUMENT_TABULATED  w = linear interpolation of response at Delta on offsets (n_table
 *                             >= 2 finite, strictly increasing values; response [response_rows]
 *                             [n_table], response_rows 1 (shared) or n_channels), window
 *                             [nu_c + offsets[0], nu_c + offsets[n_table - 1]]; parameter and
 *                             half_width may be NULL.
 * Channel c covers the columns searchsorted(grid, lo, "left") <= j < searchsorted(grid, hi,
 * "right") of its window [lo, hi].
 * lbl_instrument_apply writes out[r][c] (device, [rows][n_channels], in the order of the centers)
 *   R_c = (sum_j w_j v_j) / (sum_j w_j) over the window, v_j = values[r*row_stride + j] (device,
 *   row_stride >= the grid's points), or exp(-v_j) with LBL_PATH_TRANSMITTANCE;
 * NaN where the window holds no points, lies not wholly inside [grid[0], grid[n - 1]], or its
 * weights do not sum to > 0.  The sums are formed in a fixed order without atomics: the same
 * bits for every call and however the rows are split between calls.  Queued on the engine
 * stream like lbl_path_compute, behind whatever wrote `values`, and recorded as a write of `out`;
 * LBL_ASYNC returns after queueing.  LBL_BAD_ARGUMENT (message in lbl_last_error) for an unknown
 * grid or instrument handle, a descending grid, bad shapes, centers, widths or tables, NULL
 * pointers, rows < 1, a short row_stride or unknown flags; the engine stays usable.
 * lbl_instrument_free releases the handle. */
#define LBL_INSTRUMENT_BOXCAR        0
#define LBL_INSTRUMENT_TRIANGLE      1
#define LBL_INSTRUMENT_GAUSSIAN      2
#define LBL_INSTRUMENT_FTS           3
#define LBL_INSTRUMENT_FTS_HAMMING   4
#define LBL_INSTRUMENT_TABULATED     5
int lbl_instrument_create(lbl_engine *engine, int32_t grid, int32_t shape, int32_t n_channels,
                          const double *centers, const double *parameter,
                          const double *half_width, int32_t n_table, const double *offsets,
                          const double *response, int32_t response_rows, int32_t *handle);
int lbl_instrument_free(lbl_engine *engine, int32_t handle);
int lbl_instrument_apply(lbl_engine *engine, const double *values, int64_t row_stride,
                         int32_t rows, int32_t handle, int32_t flags, double *out);

/* Options (fourteen; anything else is LBL_BAD_ARGUMENT):
 *   "prep"                LBL_PREP_DEVICE (default) / LBL_PREP_HOST: where the per-line scalars are formed
 *   "points_per_lane"     0 = by the grid (default), 1/2/4/8 grid points per lane of the accumulate kernel
 *   "timing"              0/1/2: HIP events around every kernel; 2 = only around the accumulate and
 *                         far-field series launches, so that the others keep running back to back
 *   "workspace_bytes"     per-lane workspace that bounds the levels of one pass (default 4 GiB)
 *   "farfield"            0/1: distant lines by their power series (farfield.h); default 0
 *   "aligned_tiles"       0/1: cell-aligned tiles also without the far-field series; default 0
 *   "wing_batches"        1, 2, 4, 8: most batches of eight far-wing lines per reciprocal in the
 *                         four-points-per-lane kernel (each level may get fewer); default 8
 *   "overlap_pedestal"    0/1: pedestal pre-pass on a side stream beside the accumulate launch; default 1
 *   "scan_chain"          0/1: the pedestal recurrence by relaxation where it applies, the serial
 *                         chain behind it; 0 = the serial chain alone; default 1
 *   "relax_launches"      0, 2..7: relaxation sweeps before the serial chain takes what has not
 *                         settled; 0 = three, or five for tables with more than two runs per window
 *   "lanes"               0, 2..8: streams that asynchronous calls rotate over; 0 = by kind of call
 *   "overlap_plain"       0/1: plain asynchronous calls on grids larger than small_points take turns
 *                         on two lanes, so that one call's last workgroups run beside the next
 *                         call's first; default 1; 0 = back to back on the first stream
 *   "small_points"        grids of up to so many points x levels count as short calls (default 2^20)
 *   "skip_delivery_lanes" 0/1: lbl_compute_streamed avoids the internal streams that share a
 *                         hardware queue with the copy stream; default 1
 *   "poison_workspace"    0/1: a test hook; 1 = every call's pedestal pre-pass first fills its
 *                         floating-point buffers (the relaxation's pedestals, the runs' slot sums,
 *                         the serial chain's slots, the bins' totals) with 0xFF bytes, a NaN, so that
 *                         a value read before the call wrote it cannot pass for a right one; the
 *                         results do not change by a bit; default 0
 * A library built with -DLBL_ABLATE (scripts/ablate_*.sh; never the shipped one) also takes "ablate":
 * parts of the accumulate kernel switched off for timing, results wrong. */
int lbl_set_option(lbl_engine *engine, const char *name, int64_t value);

/* With option timing=1 (or 2): accumulated kernel milliseconds and launch counts since the last
 * reset; index 0 line-scalar prep (+ tile schedule: one prologue launch), 1 the far-field
 * series kernels (and the tile schedule when it is launched alone, LBL_PREP_HOST), 2 Voigt
 * accumulate (+ combine), 3 pedestal,
 * 4 continuum band spectra, 5 continuum interpolation, 6 cross-section fit, 7 cross-section
 * interpolation.  Synchronizes the streams. */
int lbl_timing(lbl_engine *engine, double ms[8], int64_t launches[8], int32_t reset);

/* Same indices: the milliseconds during which AT LEAST ONE timed launch of the kind was running
 * since the last reset (the union of the launches' intervals on the device's clock).  Queued calls
 * take turns on several streams and their launches overlap: the sum lbl_timing returns then counts
 * such a stretch twice, this counts it once -- evals / busy time is the rate of the kernel while any
 * of it runs.  Call it BEFORE the lbl_timing(..., reset = 1) that clears both. */
int lbl_timing_busy(lbl_engine *engine, double busy_ms[8]);

/* The engine's first HIP stream (a hipStream_t), for callers that time with their own events.
 * Blocking calls run on it back to back; asynchronous calls into device memory rotate over
 * several streams, so events on this one do not bracket them (use lbl_synchronize / lbl_timing,
 * or lbl_order_stream_after_engine in front of the caller's own event). */
void *lbl_stream(lbl_engine *engine);

/* Sharing HBM blocks with another HIP user of the same device without stopping the host (the
 * reference has no analogue: it is serial and host-only; this is what lets the collection of a
 * multi-GPU call, pylbl_amd/distributed.py, start behind the kernels instead of behind a
 * lbl_synchronize).  `stream` is a hipStream_t of the caller, NULL for the null stream.
 *   lbl_order_stream_after_engine: work the caller queues on `stream` from now on runs after
 *     everything queued on the engine so far (it may read what the engine wrote);
 *   lbl_order_engine_after_stream: everything the engine queues from now on runs after what
 *     `stream` holds now (the engine may overwrite what that work read). */
int lbl_order_stream_after_engine(lbl_engine *engine, void *stream);
int lbl_order_engine_after_stream(lbl_engine *engine, void *stream);

/* Device memory helpers so that hosts without a HIP binding can keep spectra in HBM. */
int lbl_device_alloc(lbl_engine *engine, int64_t bytes, void **pointer);
int lbl_device_free(lbl_engine *engine, void *pointer);
int lbl_copy_to_host(lbl_engine *engine, void *host, const void *device, int64_t bytes);
/* `rows` rows of `row_bytes` bytes from device memory (row pitch device_pitch bytes) into host
 * memory (row pitch host_pitch bytes): lets a host place the first grid.size columns of every
 * level straight into its final array, e.g. beta[level, mechanism, :]
 * (pyLBL/spectroscopy.py:188-191), without an intermediate copy.  Without LBL_ASYNC it returns
 * when the rows have arrived. */
int lbl_copy_rows_to_host(lbl_engine *engine, void *host, int64_t host_pitch,
                          const void *device, int64_t device_pitch, int64_t row_bytes,
                          int64_t rows, int32_t flags);
/* Page-locked host memory for results: copies into it run at the full rate of the host link and,
 * with LBL_ASYNC in lbl_copy_rows_to_host, beside the kernels queued after them (the copy waits
 * for everything queued before it on any lane; lbl_synchronize waits for the copy). */
int lbl_host_alloc(lbl_engine *engine, int64_t bytes, void **pointer);
int lbl_host_free(lbl_engine *engine, void *pointer);

/* Debug/inspection: per-line scalars for one level as the engine computed them, in
 * reference row order: n_lines x 8 doubles {centre, doppler hwhm, lorentz hwhm, strength,
 * first index, last index, status (1 evaluated, 0 skipped, -1 not accepted), pedestal}. */
int lbl_line_scalars(lbl_engine *engine, int32_t molecule, double temperature,
                     double pressure, double vmr, int32_t v0, int32_t vn, int32_t n_per_v,
                     int32_t cut_off, int32_t remove_pedestal, int32_t range_policy,
                     double *derived);

/* ---------------------------------------------------------------------------------------
 * MT-CKD continua: mechanism slot 1 of Spectroscopy.compute_absorption
 * (pyLBL/spectroscopy.py:193-197).  Replaces BandedContinuum.spectra
 * (pyLBL/mt_ckd/utils.py:157-174) and the Continuum.spectra method of the 16 band classes
 * (water_vapor.py, carbon_dioxide.py, nitrogen.py, oxygen.py, ozone.py).
 * ------------------------------------------------------------------------------------- */

/* Band formulas (the class each one replaces). */
#define LBL_BAND_H2O_SELF        0  /* WaterVaporARMSelfContinuum      columns bs296, bs260          */
#define LBL_BAND_H2O_FOREIGN     1  /* WaterVaporIASIForeignContinuum  columns bfh2o, scale          */
#define LBL_BAND_CO2             2  /* CarbonDioxideHartmannContinuum  columns bfco2, chi, exponent  */
#define LBL_BAND_N2_ROTATION     3  /* NitrogenCIAPureRotationContinuum ct_296, ct_220, sf_296, sf_220 */
#define LBL_BAND_N2_FUNDAMENTAL  4  /* NitrogenCIAFundamentalContinuum xn2_272, xn2_228, a_h2o       */
#define LBL_BAND_N2_OVERTONE     5  /* NitrogenCIAFirstOvertoneContinuum xn2                         */
#define LBL_BAND_O2_FUNDAMENTAL  6  /* OxygenCIAFundamentalContinuum   o2_f, o2_t                    */
#define LBL_BAND_O2_NIR          7  /* OxygenCIANIRContinuum           o2_inf1                       */
#define LBL_BAND_O2_NIR2         8  /* OxygenCIANIR2Continuum          analytic shape / wavenumber   */
#define LBL_BAND_O2_NIR3         9  /* OxygenCIANIR3Continuum          o2_inf3                       */
#define LBL_BAND_O2_VISIBLE     10  /* OxygenVisibleContinuum          o2_invis                      */
#define LBL_BAND_O2_HERZBERG    11  /* OxygenHerzbergContinuum         analytic shape                */
#define LBL_BAND_O2_UV          12  /* OxygenUVContinuum               o2_infuv                      */
#define LBL_BAND_O3_CHAPPUIS    13  /* OzoneChappuisWulfContinuum      x_o3, y_o3, z_o3              */
#define LBL_BAND_O3_HARTLEY     14  /* OzoneHartleyHugginsContinuum    o3_hh0, o3_hh1, o3_hh2        */
#define LBL_BAND_O3_UV          15  /* OzoneUVContinuum                o3_huv                        */
#define LBL_MAX_BANDS            8

/* One band: `size` coefficients per column on the grid lower_bound + j*resolution
 * (utils.py:136-143); column[c] is the offset (in doubles) of column c in `table`, -1 if the
 * formula has fewer columns. */
typedef struct lbl_band
{
    int32_t kind;
    int32_t size;
    double lower_bound;
    double resolution;
    int64_t column[4];
} lbl_band;

/* Mole fractions a level supplies, in this order (the reference passes a dictionary of all
 * gases, spectroscopy.py:173): the gas the continuum belongs to, H2O, O2, N2, and the sum
 * over every gas of the atmosphere (air_number_density, utils.py:16-28). */
#define LBL_VMR_SELF   0
#define LBL_VMR_H2O    1
#define LBL_VMR_O2     2
#define LBL_VMR_N2     3
#define LBL_VMR_TOTAL  4
#define LBL_VMR_COUNT  5

/* Uploads the bands of one continuum (<= LBL_MAX_BANDS) and their coefficient table. */
int lbl_continuum_load(lbl_engine *engine, int32_t n_bands, const lbl_band *bands,
                       const double *table, int64_t table_size, int32_t *continuum);
int lbl_continuum_free(lbl_engine *engine, int32_t continuum);

/* Uploads a spectral grid [cm-1] (any ascending array; the reference interpolates onto the
 * caller's own array, utils.py:171-173) and keeps it in HBM.  A grid whose every element equals
 * first + i*(second - first) in double precision -- what numpy.arange fills -- is recognised
 * (checked element by element), and the interpolation kernels then form the wavenumber in
 * registers, the same bits, instead of reading it. */
int lbl_grid_load(lbl_engine *engine, int64_t n, const double *wavenumber, int32_t *grid);
int lbl_grid_free(lbl_engine *engine, int32_t grid);

/* Continuum extinction [m-1] at n_levels levels on a loaded grid: BandedContinuum.spectra.
 *   pressure in Pa; vmr: n_levels rows of LBL_VMR_COUNT doubles;
 *   extinction: n_levels rows of n doubles, row stride level_stride (0 = dense); host memory
 *   unless LBL_OUT_DEVICE; LBL_ASYNC and LBL_ACCUMULATE as for lbl_compute. */
int lbl_continuum_compute(lbl_engine *engine, int32_t continuum, int32_t grid,
                          int32_t n_levels, const double *temperature, const double *pressure,
                          const double *vmr, int32_t flags, double *extinction,
                          int64_t level_stride);

/* Several continua in ONE pass over the grid: what compute_absorption does with the continua of
 * a gas (spectroscopy.py:193-197 adds each of them into mechanism slot 1; water vapour has two,
 * :58-61) and, in its "gas" / "total" formats, with the slots of all gases (:225-234).
 *   continua: n_continua handles, evaluated and added in this order -- every continuum's bands
 *   summed from zero, then continuum after continuum onto the block: the same values, bit for
 *   bit, as n_continua calls of lbl_continuum_compute (the first writing, the others with
 *   LBL_ACCUMULATE), at 8 (+ 8 with LBL_ACCUMULATE) bytes of HBM traffic per point and level
 *   instead of 16 + 24 (n_continua - 1);
 *   vmr: [n_continua][n_levels][LBL_VMR_COUNT] (LBL_VMR_SELF differs between the continua);
 *   extinction: device memory only (LBL_OUT_DEVICE required); LBL_ASYNC, LBL_ACCUMULATE and
 *   level_stride as for lbl_continuum_compute.  At most 64 bands in all. */
int lbl_continuum_compute_many(lbl_engine *engine, int32_t n_continua, const int32_t *continua,
                               int32_t grid, int32_t n_levels, const double *temperature,
                               const double *pressure, const double *vmr, int32_t flags,
                               double *extinction, int64_t level_stride);

/* Coarse spectra [cm-1] of every band for one level, concatenated in band order:
 * Continuum.spectra(temperature, pressure [mb], vmr) (utils.py:98-108). */
int lbl_continuum_bands(lbl_engine *engine, int32_t continuum, double temperature,
                        double pressure_mb, const double *vmr, double *spectra);

/* ---------------------------------------------------------------------------------------
 * ARTS-crossfit absorption cross-sections: mechanism slot 2 of compute_absorption
 * (pyLBL/spectroscopy.py:199-203).  Replaces CrossSection.absorption_coefficient
 * (pyLBL/arts_crossfit/cross_section.py:19-48) and calculate_xsec_fullmodel
 * (pyLBL/arts_crossfit/xsec_aux_functions.py:14-121).
 * ------------------------------------------------------------------------------------- */
#define LBL_MAX_XSEC_BANDS 16

/* Uploads the bands of one molecule: sizes[n_bands] frequencies per band; `frequency` [Hz]
 * concatenated over the bands, strictly ascending within a band; `coefficients` per band the
 * [4][size] matrix p00, p10, p01, p20 of the fit z = p00 + p10 T + p01 P + p20 T^2,
 * concatenated in band order. */
int lbl_xsec_load(lbl_engine *engine, int32_t n_bands, const int32_t *sizes,
                  const double *frequency, const double *coefficients, int32_t *xsec);
int lbl_xsec_free(lbl_engine *engine, int32_t xsec);

/* Cross sections [m2] at n_levels levels on a loaded grid (lbl_grid_load); with
 * LBL_SCALE_DENSITY multiplied by P vmr /(kb T), i.e. slot 2 itself [m-1] (vmr may be NULL
 * otherwise).  out / level_stride / LBL_OUT_DEVICE / LBL_ASYNC / LBL_ACCUMULATE as for
 * lbl_continuum_compute. */
int lbl_xsec_compute(lbl_engine *engine, int32_t xsec, int32_t grid, int32_t n_levels,
                     const double *temperature, const double *pressure, const double *vmr,
                     int32_t flags, double *out, int64_t level_stride);

/* The fit with negative values removed on the bands' own frequency grids, concatenated in
 * band order: calculate_xsec_fullmodel(temperature, pressure [Pa], coeffs) per band. */
int lbl_xsec_bands(lbl_engine *engine, int32_t xsec, double temperature, double pressure,
                   double *values);

/* Same signature and semantics as the reference's absorption() (absorption.c:19-30):
 * opens the SQLite file, uploads the molecule, computes one level.  Returns 0 on success, 1 on
 * error (message on stderr), 0 with zeros when the molecule has no TIPS rows
 * (absorption.c:53-59).
 *   Device: LBL_DEVICE if set, else LOCAL_RANK / OMPI_COMM_WORLD_LOCAL_RANK / SLURM_LOCALID
 *   modulo the visible devices, else 0 (indices relative to HIP_VISIBLE_DEVICES), fixed at the
 *   first call of the process.
 *   Residency: the uploaded line table is kept per (path, formula) and re-read when the file's
 *   mtime, size or inode changed; at most LBL_COMPAT_CACHE (default 16) molecules stay in HBM,
 *   least recently used evicted first. */
int lbl_absorption(double pressure, double temperature, double volume_mixing_ratio,
                   int v0, int vn, int n_per_v, double *k, char *database, char *formula,
                   int cut_off, int remove_pedestal);

/* The reference's own symbol (pyLBL/c_lib/absorption.c:19-30, bound by
 * pyLBL/c_lib/gas_optics.py:11-12,68-91): an alias of lbl_absorption, exported so that this
 * library, installed as libabsorption*.so beside gas_optics.py, serves an unmodified pyLBL.
 * Define LBL_NO_REFERENCE_SYMBOL before including this header when the reference's own
 * absorption.h is in the same translation unit. */
#ifndef LBL_NO_REFERENCE_SYMBOL
int absorption(double pressure, double temperature, double volume_mixing_ratio,
               int v0, int vn, int n_per_v, double *k, char *database, char *formula,
               int cut_off, int remove_pedestal);
#endif

/* The reader of lbl_absorption by itself -- no GPU involved: one molecule's rows out of an SQLite
 * file in pyLBL's schema (database.py:418-486) through the reference C reader's own SELECTs
 * (absorption.c:69-70; spectral_database.c:55, :113, :143), as host arrays.  Replaces, for hosts,
 * the ORM route of pyLBL/database.py:350-395 (Database.gas / Database.tips) at the speed of the C
 * row loop.  `name` is any alias of the molecule.  Status LBL_OK or LBL_TABLE_* (message:
 * lbl_last_error(NULL)); *table is then NULL.
 *   lbl_table_shape: row counts (transitions; isotopologue rows; TIPS isotopologues x temperatures),
 *     the molecule's id and ordinary formula.
 *   lbl_table_copy: copies out (any pointer may be NULL) the seven fp64 columns nu, sw, gamma_air,
 *     gamma_self, n_air, elower, delta_air as columns[7][n_lines]; local_iso_id[n_lines] raw;
 *     isoid / mass of the isotopologue rows in row order; tips_temperature[num_t];
 *     tips_data[num_iso][num_t]. */
typedef struct lbl_table lbl_table;
int lbl_table_read(const char *path, const char *name, lbl_table **table);
int lbl_table_shape(const lbl_table *table, int64_t *n_lines, int32_t *molecule_id,
                    int32_t *n_isotopologues, int32_t *num_iso, int32_t *num_t,
                    char *formula, int32_t formula_bytes);
int lbl_table_copy(const lbl_table *table, double *columns, int32_t *local_iso_id,
                   int64_t *isoid, double *mass, double *tips_temperature, double *tips_data);
int lbl_table_free(lbl_table *table);

/* File -> HBM in one call (read as above, masses filed under isoid with 0 -> 10, then
 * lbl_molecule_load): what lbl_absorption does at its first call on a (path, formula). */
int lbl_molecule_load_sqlite(lbl_engine *engine, const char *path, const char *name,
                             int32_t *molecule);

/* State of the compatibility entry: the device it computes on (-1 before its first call) and
 * the number of molecules it keeps in HBM. */
int lbl_compat_state(int32_t *device, int32_t *resident);

/* Library version string. */
const char *lbl_version(void);

/* Batches of eight far-wing lines that share one reciprocal (1, 2, 4 or 8), as the accumulate
 * kernel chooses them per level from four binary-exponent bounds of its far-wing terms:
 * bounds = {t_low, -t_high, b_low, -b_high} with 2^t_low <= t < 2^t_high for t = d^2 + gamma^2
 * and 2^b_low <= |b| < 2^b_high for the non-zero Lorentz amplitudes; 0x7f7f7f7f marks a bound
 * no line contributed to.  Exposed for tests. */
int lbl_wing_batches(const int32_t *bounds);

/* Sunlight without scattering (Spectroscopy.compute_solar): the direct beam at every interface
 * of the paths and the sunlight a Lambertian surface reflects to a viewer, both pure absorption
 * along slant paths through the block of absorption coefficients in HBM.
 *
 * lbl_solar_spectrum fills row[j] = S(nu_j) [W m-2 (cm-1)-1] for the first `columns` points nu_j
 * of `grid` (a handle of lbl_grid_load, ascending or not):
 *   n_knots == 0: the blackbody  S = scale*B(nu, temperature), B as in lbl_path_radiance (0 for
 *   nu <= 0); for the Sun scale = LBL_SOLAR_SOLID_ANGLE times the distance factor and temperature =
 *   LBL_SOLAR_TEMPERATURE;
 *   knot_wavenumber == NULL and n_knots == columns: S = scale*knot_irradiance[j], the values on
 *   the grid as they are (host, finite and >= 0);
 *   otherwise a table: knot_wavenumber (host, k_0 < ... < k_{M-1} [cm-1], finite, 2 <= M <= 2^22)
 *   and knot_irradiance (host, e_0 .. e_{M-1}, finite and >= 0), interpolated exactly as
 *   lbl_surface_emissivity interpolates:
 *   for k_j <= nu < k_{j+1}:  E = e_j + (nu - k_j)*((e_{j+1} - e_j)/(k_{j+1} - k_j)),
 *   E = e_0 for nu <= k_0,  E = e_{M-1} for nu >= k_{M-1},  S = scale*E;
 *   scale finite and > 0 (1.: the table's own bits); row (device, >= columns values).
 *   flags: LBL_ASYNC or 0.
 * LBL_BAD_ARGUMENT (message in lbl_last_error) for an unknown grid, columns outside the grid, a
 * scale or temperature that is not finite and > 0, knots that are not finite and strictly
 * ascending, irradiances that are negative or not finite, or n_knots outside what its mode allows;
 * nothing is launched and the engine stays usable.
 *
 * lbl_path_solar sweeps the levels of a run from space to the surface.  beta (read only),
 * row_stride, columns, n_paths, levels_per_path, level_begin, level_count, n_bands, band_start and
 * the flags LBL_PATH_FROM_LAST, LBL_PATH_CONTINUE and LBL_ASYNC as for lbl_path_flux: the Sun
 * shines in from the end of each path the sweep starts at (its last level with
 * LBL_PATH_FROM_LAST, else its first), and the surface lies behind the other end.
 *   solar_length (host, [level_count], finite and >= 0): a_l, the solar slant length of level
 *   level_begin + l [m];
 *   view_length (host, [level_count], finite and >= 0, or NULL: no viewer): v_l, the length of the
 *   path from the surface to the viewer in that level [m];
 *   solar_zenith_cosine (host, [n_paths]): mu0 of each path, in (0, 1];
 *   solar_row (device, >= columns values): S, e.g. lbl_solar_spectrum's row;
 *   albedo_rows (device, [n_paths][row_stride], e.g. lbl_surface_emissivity's rows) or albedo
 *   (host, [n_paths], in [0, 1]): the Lambertian albedo A; exactly one of them with view_length,
 *   neither without;
 *   carry (device, [n_paths][2][row_stride]): tau and tv of each path, left there by every call
 *   and read under LBL_PATH_CONTINUE.
 * Per path and column, each product and sum rounded as written (no fused multiply-add):
 *   F0 = mu0*S;  tau = 0, tv = 0;  F at the interface that faces space = F0
 *   for each level in order from space to the surface:
 *     tau = tau + a_l*beta_l;  tv = tv + v_l*beta_l
 *     F at the interface below the level = F0*exp(-tau)
 *   reflected radiance = ((A*F0)/pi)*exp(-(tau + tv)),  pi = 3.141592653589793, tau and tv at the
 *   surface.
 * Both optical depths are added in the Sun's order, space to surface.  Outputs (device, NULL: not
 * wanted; at least one is), all on the grid:
 *   interface_rows ([level_count][row_stride], not beta): F at the interface below each level;
 *   space_rows ([n_paths][row_stride]): F0, written for the paths the run starts;
 *   surface_rows ([n_paths][row_stride]): F at the surface, written for the paths the run finishes
 *   (the same bits as the last interface row of the path);
 *   reflected_rows ([n_paths][row_stride]): the reflected radiance [W m-2 sr-1 (cm-1)-1] of the paths
 *   the run finishes; given if and only if view_length is.
 * With n_bands > 0, interface_mean ([level_count][n_bands]), space_mean, surface_mean and
 * reflected_mean ([n_paths][n_bands]) receive lbl_path_compute's ordered band means of the rows
 * of the same name, which must be given too (NULL: not wanted); NaN for a band without points.
 * LBL_BAD_ARGUMENT for bad shapes, a run whose LBL_PATH_CONTINUE does not match, lengths that are
 * negative or not finite, a cosine outside (0, 1], an albedo outside [0, 1], a view without an
 * albedo or an albedo without a view, reflected_rows without a view, interface_rows == beta, no
 * output at all, or a band mean without its rows or without bands; nothing is launched and the
 * engine stays usable. */
#define LBL_SOLAR_TEMPERATURE  5772.                    /* effective temperature of the Sun [K]   */
#define LBL_SOLAR_SOLID_ANGLE  6.794273971369406e-05    /* pi (6.957e8/1.495978707e11)^2 [sr]     */
int lbl_solar_spectrum(lbl_engine *engine, int32_t grid, int64_t columns, int32_t n_knots,
                       const double *knot_wavenumber, const double *knot_irradiance,
                       double temperature, double scale, double *row, int32_t flags);
int lbl_path_solar(lbl_engine *engine, double *beta, int64_t row_stride, int64_t columns,
                   int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                   int32_t level_count, const double *solar_length, const double *view_length,
                   const double *solar_zenith_cosine, const double *solar_row,
                   const double *albedo_rows, const double *albedo, int32_t n_bands,
                   const int64_t *band_start, double *carry, double *interface_rows,
                   double *space_rows, double *surface_rows, double *reflected_rows,
                   double *interface_mean, double *space_mean, double *surface_mean,
                   double *reflected_mean, int32_t flags);

/* Band k-distributions: every (row, band) segment of a block sorted in place, and what a
 * correlated-k table stores of it (kernels: pylbl_amd/csrc/band_sort.h).
 *
 * values (device, [n_rows][row_stride], the first `columns` of each row used; rows of any stride
 * and alignment): band b is the columns band_start[b] <= j < band_start[b + 1] (host,
 * [n_bands + 1], n_bands >= 1, not decreasing, inside [0, columns]; a band may be empty).  On return each band
 * of each row holds its own values sorted ascending in this total order: with u the 64 bits of a
 * value, key = u ^ 0x8000000000000000 for a clear sign bit and ~u for a set one, keys compared as
 * unsigned integers: -inf < negatives < -0 < +0 < positives < +inf < NaN with the sign clear.
 * The sorted values are the input's bits, permuted; columns in no band and the padding of the
 * rows are not touched.  The result does not depend on how the work is cut: repeated calls, any
 * layout and any split of the rows over calls give the same bits.
 *   scratch (device, a block shaped like `values`, not overlapping it): work space, needed when a
 *   band is longer than 4096 columns (else it may be NULL); its contents are undefined afterwards.
 *   interval_start (host, [n_intervals + 1], not decreasing, inside [0, columns]) and means
 *   (device, [n_rows][n_intervals]), or both NULL / 0: means[r][q] = the arithmetic mean of the
 *   sorted row r over the columns interval_start[q] <= j < interval_start[q + 1], formed as
 *   lbl_path_compute forms its band means (fixed order, no atomics); NaN for an interval without
 *   columns.  The intervals are columns of the row, so sub-ranges of the sorted bands.
 *   point_index (host, int64 [n_bands][n_points]), point_fraction (host, [n_bands][n_points]) and
 *   quantiles (device, [n_rows][n_bands][n_points]), or all NULL / 0: with k the sorted band of N
 *   values, i = point_index[b][p] and f = point_fraction[b][p],
 *     quantiles[r][b][p] = k_i + f*(k_j - k_i),  j = min(i + 1, N - 1),
 *   each operation rounded as written (no fused multiply-add); NaN where i < 0 or i >= N.
 *   flags: LBL_ASYNC or 0.
 * The call runs on the engine's stream like lbl_path_compute, behind whatever wrote `values`, and
 * is recorded as a write of values, scratch, means and quantiles.
 * LBL_BAD_ARGUMENT (message in lbl_last_error) for bad shapes, band or interval starts that
 * decrease or leave [0, columns], a band longer than 4096 columns without scratch, scratch ==
 * values, means without intervals or quantiles without their tables, or other flags; nothing is
 * launched and the engine stays usable. */
int lbl_band_distribution(lbl_engine *engine, double *values, int64_t row_stride, int64_t columns,
                          int32_t n_rows, const int64_t *band_start, int32_t n_bands,
                          double *scratch, const int64_t *interval_start, int32_t n_intervals,
                          double *means, const int64_t *point_index, const double *point_fraction,
                          int32_t n_points, double *quantiles, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
