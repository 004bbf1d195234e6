/* lbl_amd_scatterer.h: the two-stream entries of liblbl_amd.so with spectral cloud and aerosol
 * optics, beside lbl_amd.h, lbl_amd_twostream.h, lbl_amd_thermal.h and lbl_amd_thermal_source.h. */
#ifndef LBL_AMD_SCATTERER_H_
#define LBL_AMD_SCATTERER_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two-stream fluxes through scatterers whose optics vary with wavenumber
 * (Spectroscopy.compute_solar_flux_spectral and compute_thermal_flux_spectral): the grey
 * scatterer of lbl_path_two_stream (lbl_amd_twostream.h),
 * lbl_path_thermal_two_stream (lbl_amd_thermal.h) and lbl_path_thermal_two_stream_source
 * (lbl_amd_thermal_source.h) -- one tau_c, omega_c and g_c per level, the same at every grid
 * point -- becomes a table per level over M knots, interpolated like lbl_surface_emissivity's
 * (kernels: pylbl_amd/csrc/scatterer.h, twostream.h, twostream_thermal.h).  These two entries
 * extend the C ABI of lbl_amd.h, which this header includes and leaves as it is; they are exported
 * by the same library and take the same engine, grid handles, flags and status codes.
 *
 * The knot arguments of both entries:
 *   grid: a handle of lbl_grid_load with at least `columns` points nu_j [cm-1], ascending or not;
 *   n_knots: M, 2 <= M <= 1024;
 *   knot_wavenumber (host, [n_knots]): k_0 < ... < k_{M-1} [cm-1], finite and strictly ascending;
 *   knot_optics (host, [level_count][n_knots][3]): tau_c (finite, >= 0), omega_c (in [0, 1]) and
 *   g_c (in [0, 1)) of flat level level_begin + r at every knot.
 * The spectral scatterer at grid point nu of a level, each product, sum and quotient rounded as
 * written (no fused multiply-add):
 *   j = the largest index with k_j <= nu, limited to 0 .. M-2
 *   u = (nu - k_j)/(k_{j+1} - k_j), limited to [0, 1]
 *     (nu <= k_0 gives u = 0 and nu >= k_{M-1} gives u = 1: the optics are constant outside the
 *     knots; j and u belong to the column, not to the level)
 *   for each of e in {tau_c, omega_c, g_c} of the level:
 *     v = e_j + u*(e_{j+1} - e_j), then v is limited to [min(e_j, e_{j+1}), max(e_j, e_{j+1})]
 *     (whatever the rounding does, tau_c >= 0, 0 <= omega_c <= 1 and 0 <= g_c < 1 per element)
 *   w_c = omega_c*tau_c and, for the shortwave layer, h_c = w_c*g_c
 * From there on the layer and the adding recurrences are, line by line, those of the grey entry:
 * lbl_path_two_stream's layer takes (tau_c, w_c, h_c) per element, the longwave layer (tau_c, w_c,
 * g_c) per element, with f = g_c*g_c and gp = g_c/(1 + g_c) formed per element.
 * Two properties follow.
 *   1. A table that is flat in nu (e_j = c at every knot) gives the grey entry's result for the
 *      level values c bit for bit: the difference is 0, the limit is [c, c], and the products are
 *      those the caller forms for the grey level table.
 *   2. A level whose knots all have omega_c*tau_c == 0 (no scatterer, or one that only absorbs)
 *      is a clear level of the longwave entry for the whole wavefront: one exp, one expm1 and the
 *      Planck function, with tau = s_l*beta + tau_c(nu).  The entry derives that from the knot
 *      table.  (Knots that scatter only where there is no optical depth, omega_c > 0 beside
 *      tau_c == 0 and the other way round at the next knot, make such a level too: the longwave
 *      entry then leaves out the scattering that the interpolation gives between them.)
 *      In a level that is not clear every element takes the cloudy branches, also one whose w_c
 *      is 0, with g_c as it comes; only where tau = s_l*beta + tau_c is 0, which the grey entry's
 *      cloudy level cannot have and where omega = w_c/tau would be 0/0, the element takes the
 *      clear branch: x = 0, the identity.
 *
 * lbl_path_two_stream_spectral takes lbl_path_two_stream's arguments, with the same meaning,
 * shapes and checks, and behind level_table grid, n_knots, knot_wavenumber and knot_optics.
 * lbl_path_thermal_two_stream_spectral takes lbl_path_thermal_two_stream_source's arguments,
 * likewise, and behind edge_temperature n_knots, knot_wavenumber and knot_optics; edge_temperature
 * may be NULL: the source is then lbl_path_thermal_two_stream's, the Planck function of T_l.
 * In both, the scatterer words of level_table must be 0: tau_c, w_c and h_c of the shortwave
 * table, tau_c, w_c and g_c of the longwave table.
 * Outputs, band means and work as for the grey entries.
 * LBL_BAD_ARGUMENT (message in lbl_last_error) for everything the grey entry refuses and for an
 * unknown grid or one with fewer than `columns` points, n_knots outside 2 .. 1024, knot arguments
 * that are NULL, knots that are not finite and strictly ascending, optics that are not finite or
 * outside their ranges, and scatterer words of the level table that are not 0; nothing is launched
 * and the engine stays usable. */
int lbl_path_two_stream_spectral(lbl_engine *engine, double *beta, int64_t row_stride,
                                 int64_t columns, int32_t n_paths, int32_t levels_per_path,
                                 int32_t level_begin, int32_t level_count,
                                 const double *level_table, int32_t grid, int32_t n_knots,
                                 const double *knot_wavenumber, const double *knot_optics,
                                 const double *solar_zenith_cosine, const double *solar_row,
                                 const double *rayleigh_row, const double *albedo_rows,
                                 const double *albedo, int32_t n_bands, const int64_t *band_start,
                                 double *work, double *up_rows, double *down_rows,
                                 double *direct_rows, double *diffuse_rows, double *top_up_rows,
                                 double *top_down_rows, double *top_direct_rows,
                                 double *top_diffuse_rows, double *up_mean, double *down_mean,
                                 double *direct_mean, double *diffuse_mean, double *top_up_mean,
                                 double *top_down_mean, double *top_direct_mean,
                                 double *top_diffuse_mean, int32_t flags);
int lbl_path_thermal_two_stream_spectral(lbl_engine *engine, double *beta, int64_t row_stride,
                                         int64_t columns, int32_t grid, int32_t n_paths,
                                         int32_t levels_per_path, int32_t level_begin,
                                         int32_t level_count, const double *level_table,
                                         const double *edge_temperature, int32_t n_knots,
                                         const double *knot_wavenumber, const double *knot_optics,
                                         double diffusivity, const double *surface_temperature,
                                         const double *emissivity_rows, const double *emissivity,
                                         int32_t n_bands, const int64_t *band_start, double *work,
                                         double *up_rows, double *down_rows, double *top_up_rows,
                                         double *top_down_rows, double *up_mean, double *down_mean,
                                         double *top_up_mean, double *top_down_mean,
                                         int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
