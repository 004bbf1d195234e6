/* lbl_amd_scatterer_radiance.h: the two radiance entries of liblbl_amd.so with spectral cloud and
 * aerosol optics, beside lbl_amd.h, lbl_amd_scatterer.h, lbl_amd_thermal_radiance.h and
 * lbl_amd_solar_radiance.h. */
#ifndef LBL_AMD_SCATTERER_RADIANCE_H_
#define LBL_AMD_SCATTERER_RADIANCE_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The radiance a viewer above the atmosphere sees through scatterers whose optics vary with
 * wavenumber (Spectroscopy.compute_thermal_radiance_spectral and
 * compute_solar_radiance_spectral): the grey scatterer of lbl_path_thermal_radiance
 * (lbl_amd_thermal_radiance.h) and lbl_path_solar_radiance (lbl_amd_solar_radiance.h) -- one
 * tau_c, omega_c and g_c per level, the same at every grid point -- becomes the table per level
 * over M knots of lbl_amd_scatterer.h, whose definition these entries take unchanged: the knot
 * arguments grid, n_knots, knot_wavenumber and knot_optics, where a grid point lies among the
 * knots (j, u), the interpolation of tau_c, omega_c and g_c and its limit, and w_c = omega_c*tau_c,
 * h_c = w_c*g_c, each product, sum and quotient rounded as written (kernels:
 * pylbl_amd/csrc/thermal_radiance.h, solar_radiance.h, scatterer.h).  These two entries extend
 * the C ABI of lbl_amd.h, which this header includes and leaves as it is; they are exported by the
 * same library and take the same engine, grid handles, flags and status codes.
 *
 * The flux rows they read are those of lbl_path_thermal_two_stream_spectral (without
 * edge_temperature: the source of the view is the Planck function of T_l) and of
 * lbl_path_two_stream_spectral for the same run, tables, knots and surface.
 *
 * What the view adds to lbl_amd_scatterer.h.  Per element (level, path and grid point) the level
 * arithmetic is the grey entry's, line by line, with the element's own scatterer.
 * Longwave (lbl_path_thermal_radiance_spectral):
 *   A level whose knots all have omega_c*tau_c == 0 is a clear level for the whole wavefront:
 *     tau = s_l*beta + tau_c(nu) ; x = tau/mu ; I_top = I_bot*exp(-x) + B*(-expm1(-x))
 *   and reads no flux row.  In a level that scatters every element takes the cloudy lines of
 *   lbl_path_thermal_radiance with its own tau_c, w_c = omega_c*tau_c, f = g_c*g_c,
 *   gp = g_c/(1 + g_c) and a = (3*(gp*mu))/2: the view's a is per element.  An element with
 *   tau == 0 takes the clear line (x = 0: the identity), as in the flux entry.
 * Shortwave (lbl_path_solar_radiance_spectral):
 *   Per element tau_c, w_c and h_c go into the level of lbl_path_solar_radiance, and the
 *   Henyey-Greenstein factor PH is per element too, from gc = h_c/w_c (0 where w_c == 0): from the
 *   products, as the grey entry forms it, not from the interpolated g_c.  gc < 1: with g_c <=
 *   1 - 2^-53 and w_c a normal number, w_c*g_c lies at least half an ulp of w_c below w_c and rounds
 *   to a double below it, and the quotient of two doubles h_c < w_c rounds to at most 1 - 2^-53.  A
 *   subnormal w_c can give h_c == w_c, so the kernel limits gc to 1 - 2^-53, which changes no value
 *   below it: the grey entry's refusal of h_c >= w_c has no counterpart per element.
 *   Without a Rayleigh row, a level none of whose knots scatters reads no flux row:
 *     tau = s_l*beta + tau_c(nu) ; I_top = I_bot*exp(-tau/mu)
 * Four properties follow.
 *   1. A table that is flat in nu (e_j = c at every knot) gives the grey view entry's result for
 *      the level values c bit for bit, in every branch, general and conservative: the interpolation
 *      returns c, the products are those the caller forms for the grey level table, and the level
 *      is the grey entry's.
 *   2. A longwave level that scatters at no knot is a clear level with tau_c(nu).  With no
 *      scatterer anywhere, eps = 1 and mu = 1 the result is lbl_path_radiance's bit for bit, as for
 *      the grey entry.
 *   3. Shortwave, with no Rayleigh row and a table that scatters nowhere, the result is
 *      lbl_path_solar's reflected radiance under view lengths s_l/mu to the few roundings per level
 *      that lbl_path_solar_radiance documents; a table that only absorbs (omega_c = 0, tau_c(nu) >
 *      0) attenuates by exp(-tau_c(nu)/mu) on top in every level, along both slant paths, as the
 *      flux rows have it.
 *   4. j and u belong to the column: the view sweep and the flux sweeps before it place every
 *      column among the knots by the same lines (scatterer.h's scatterer_lane), so that the view
 *      and the flux rows it reads hold the same scatterer in every element.
 *
 * lbl_path_thermal_radiance_spectral takes lbl_path_thermal_radiance's arguments, with the same
 * meaning, shapes and checks, and behind level_table n_knots, knot_wavenumber and knot_optics.
 * lbl_path_solar_radiance_spectral takes lbl_path_solar_radiance's arguments, likewise, and behind
 * level_table grid, n_knots, knot_wavenumber and knot_optics.  In both, the scatterer words of
 * level_table must be 0: tau_c, w_c and g_c of the longwave table, tau_c, w_c and h_c of the
 * shortwave table.  Outputs and band means as for the grey entries.
 * LBL_BAD_ARGUMENT (message in lbl_last_error) for everything the grey entry refuses and for an
 * unknown grid or one with fewer than `columns` points, n_knots outside 2 .. 1024, knot arguments
 * that are NULL, knots that are not finite and strictly ascending, optics that are not finite or
 * outside their ranges, and scatterer words of the level table that are not 0; nothing is launched
 * and the engine stays usable. */
int lbl_path_thermal_radiance_spectral(lbl_engine *engine, double *beta, int64_t row_stride,
                                       int64_t columns, int32_t grid, int32_t n_paths,
                                       int32_t levels_per_path, int32_t level_begin,
                                       int32_t level_count, const double *level_table,
                                       int32_t n_knots, const double *knot_wavenumber,
                                       const double *knot_optics, double diffusivity,
                                       const double *view_cosine,
                                       const double *surface_temperature,
                                       const double *emissivity_rows, const double *emissivity,
                                       const double *up_rows, const double *down_rows,
                                       int32_t n_bands, const int64_t *band_start,
                                       double *radiance_rows, double *brightness_rows,
                                       double *radiance_mean, int32_t flags);
int lbl_path_solar_radiance_spectral(lbl_engine *engine, double *beta, int64_t row_stride,
                                     int64_t columns, int32_t n_paths, int32_t levels_per_path,
                                     int32_t level_begin, int32_t level_count,
                                     const double *level_table, int32_t grid, int32_t n_knots,
                                     const double *knot_wavenumber, const double *knot_optics,
                                     const double *solar_zenith_cosine, const double *view_cosine,
                                     const double *scattering_cosine, const double *solar_row,
                                     const double *rayleigh_row, const double *albedo_rows,
                                     const double *albedo, const double *up_rows,
                                     const double *direct_rows, const double *diffuse_rows,
                                     int32_t n_bands, const int64_t *band_start,
                                     double *radiance_rows, double *radiance_mean, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
