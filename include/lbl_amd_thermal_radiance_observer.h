/* lbl_amd_thermal_radiance_observer.h: the all-sky radiance entry of liblbl_amd.so for an observer
 * at any interface, looking down or up, beside lbl_amd.h, lbl_amd_thermal_radiance.h and
 * lbl_amd_thermal_radiance_source.h. */
#ifndef LBL_AMD_THERMAL_RADIANCE_OBSERVER_H_
#define LBL_AMD_THERMAL_RADIANCE_OBSERVER_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Radiances through clouds at an observer inside, above or below the atmosphere
 * (Spectroscopy.compute_thermal_radiance_at): the view sweep of lbl_path_thermal_radiance
 * (lbl_amd_thermal_radiance.h) and of lbl_path_thermal_radiance_source
 * (lbl_amd_thermal_radiance_source.h), run in either direction and stopped after the levels the ray
 * passes (kernel: pylbl_amd/csrc/thermal_radiance_observer.h).  This entry extends the C ABI of
 * lbl_amd.h, which this header includes and leaves as it is; it is exported by the same library and
 * takes the same engine, grid handles, flags and status codes.
 *
 * lbl_path_thermal_radiance_observer takes lbl_path_thermal_radiance_source's arguments, with the
 * same meaning, shapes and checks, with three differences:
 *   edge_temperature may be NULL: isothermal levels, with up_rows and down_rows the fluxes of
 *   lbl_path_thermal_two_stream; otherwise they are those of lbl_path_thermal_two_stream_source.
 *   observer_levels (host, [n_paths], behind view_cosine): n_p, the levels the ray of path p
 *   passes, 0 <= n_p <= levels_per_path.
 *   view_up (behind observer_levels): 0 looking down, 1 looking up.
 * The flags and LBL_PATH_FROM_LAST (the surface is level 0 of each path) are as in those entries.
 * With L = levels_per_path, interface 0 facing space, level i between interfaces i and i + 1, and
 * up[i], down[i] the fluxes at interface i (down[0] = 0 is a constant, not read): per level call
 * the face by which the ray enters E and the face by which it leaves X, and
 *   F_with: the flux travelling with the ray at E ; F_against: the flux travelling against it at X
 *   B_E, B_X: B at the temperatures of the two faces (with edge_temperature)
 * The level maps I_E to I_X by the lines of lbl_path_thermal_radiance (edge_temperature NULL) or of
 * lbl_path_thermal_radiance_source, each product, sum and quotient rounded as written (no fused
 * multiply-add), with their arguments read as
 *   up[i+1] := F_with ; down[i] := F_against ; Bb := B_E ; Bt := B_X ; a = (3*(gp*mu))/2
 * (a ray that travels downward through a level is the ray that travels upward through the mirrored
 * level, and the layer's two-stream solution is symmetric under that mirror).
 * looking down (view_up == 0):
 *   E is the surface-side face ; F_with = up[i+1] ; F_against = down[i]
 *   start: I = eps*B(T_s) + (1 - eps)*(down[L]/pi), the surface line of lbl_path_thermal_radiance
 *   levels: the n_p levels nearest the surface, in order ; result: I at interface L - n_p
 * looking up (view_up == 1):
 *   E is the space-side face ; F_with = down[i] ; F_against = up[i+1]
 *   start: I = 0 at interface 0
 *   levels: 0 ... n_p - 1 counted from space, in order ; result: I at interface n_p
 *   with edge_temperature:
 *     c = (pi*(B_space - B_surface))/(su*t)
 *     u1 = (down[i] - pi*B_space) - c ; d0 = (up[i+1] - pi*B_surface) + c
 *   clear level with edge_temperature: I_X = I_E*exp(-x) + (B_E*(A - lw) + B_X*lw)
 * down[0] = 0 is used only where level 0 itself is passed; an observer inside the atmosphere has a
 * down row at its interface, and that row is read.
 * With n_p == L and view_up == 0 the rows are lbl_path_thermal_radiance's (edge_temperature NULL) or
 * lbl_path_thermal_radiance_source's bit for bit.  A path with n_p == 0 writes its start value; the
 * brightness temperature of a radiance <= 0 is 0, as in lbl_path_radiance.
 * Outputs, band means and write records as for lbl_path_thermal_radiance.
 * LBL_BAD_ARGUMENT for everything lbl_path_thermal_radiance_source refuses (but a NULL
 * edge_temperature), for a NULL observer_levels, an entry of it outside [0, levels_per_path] and a
 * view_up other than 0 or 1; the surface arguments are checked with view_up == 1 too, although that
 * sweep does not read them; nothing is launched, no output is written and the engine stays
 * usable. */
int lbl_path_thermal_radiance_observer(lbl_engine *engine, double *beta, int64_t row_stride,
                                       int64_t columns, int32_t grid, int32_t n_paths,
                                       int32_t levels_per_path, int32_t level_begin,
                                       int32_t level_count, const double *level_table,
                                       const double *edge_temperature, double diffusivity,
                                       const double *view_cosine, const int32_t *observer_levels,
                                       int32_t view_up, const double *surface_temperature,
                                       const double *emissivity_rows, const double *emissivity,
                                       const double *up_rows, const double *down_rows,
                                       int32_t n_bands, const int64_t *band_start,
                                       double *radiance_rows, double *brightness_rows,
                                       double *radiance_mean, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
