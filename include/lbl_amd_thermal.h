/* lbl_amd_thermal.h: the two-stream longwave entry of liblbl_amd.so, beside lbl_amd.h. */
#ifndef LBL_AMD_THERMAL_H_
#define LBL_AMD_THERMAL_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two-stream longwave fluxes through clouds (Spectroscopy.compute_thermal_flux): upward and
 * downward fluxes at every interface of whole paths, plane-parallel, in an atmosphere that absorbs,
 * emits and holds one grey scatterer per level, from a delta-scaled two-stream layer solution with
 * a thermal source and the adding recurrences (kernels: pylbl_amd/csrc/twostream_thermal.h).  This
 * entry extends the C ABI of lbl_amd.h, which this header includes and leaves as it is; it is
 * exported by the same library and takes the same engine, grid handles, flags and status codes.
 *
 * lbl_path_thermal_two_stream takes a run of whole paths.  beta (read only), row_stride, columns,
 * n_paths, levels_per_path, level_begin, level_count, n_bands and band_start as for
 * lbl_path_two_stream: level_begin and level_count are multiples of levels_per_path, nothing is
 * carried between calls.  grid: a handle of lbl_grid_load with at least `columns` points, as for
 * lbl_path_flux.  Flags: LBL_PATH_FROM_LAST (the surface lies behind level 0 of each path and space
 * behind its last level; without it the other way round) and LBL_ASYNC.
 *   level_table (host, [level_count][5], finite and >= 0): per level s_l [m], tau_c (the extinction
 *   optical depth of a grey scatterer), w_c = omega_c*tau_c <= tau_c, g_c in [0, 1) (the
 *   scatterer's asymmetry) and T_l > 0 [K];
 *   diffusivity: D in [1, 2] (1.66; 2 is the hemispheric mean of Toon et al. 1989);
 *   surface_temperature (host, [n_paths]): T_s > 0;
 *   emissivity_rows (device, [n_paths][row_stride]) or emissivity (host, [n_paths], in [0, 1]):
 *   the surface emissivity eps; exactly one of them;
 *   work (device, [level_count][2][row_stride]): U and Rs at the interface above each level.
 * With piB(T) = pi*B(nu, T), pi = numpy.pi and B as in lbl_path_radiance (0 for nu <= 0), per path
 * and column, each product, sum and quotient rounded as written (no fused multiply-add):
 *   tau_a = s_l*beta ; tau = tau_a + tau_c
 *   clear level (w_c == 0, the same for the whole wavefront):
 *     x = D*tau ; R = 0 ; T = exp(-x) ; em = -expm1(-x)
 *   cloudy level (w_c > 0; f = g_c*g_c and gp = g_c/(1 + g_c) are level scalars):
 *     omega = w_c/tau ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc
 *     g2 = (D*(w*(1 - gp)))/2 ; dif = D*(1 - w) ; g1 = g2 + dif ; su = g1 + g2 ; k2 = dif*su
 *     conservative, where k2*(1 + t*t) <= 1e-10:
 *       x = g1*t ; R = x/(1 + x) ; T = 1/(1 + x) ; em = (dif*t)/(1 + x)
 *     general:
 *       k = sqrt(k2) ; E = exp(-(k*t)) ; E2 = E*E ; o1 = -expm1(-(2*(k*t)))
 *       den = k*(1 + E2) + g1*o1 ; R = (g2*o1)/den ; T = (2*(k*E))/den
 *       em = (k*((1 - E)*(1 - E)) + dif*o1)/den        (= 1 - R - T, without the cancellation)
 *   S = piB(T_l)*em        the layer's own emission, the same upward and downward
 *   Adding, interface 0 facing space, level i between interfaces i and i + 1 in the order space ->
 *   surface:
 *   up, from the surface:  Rs[L] = 1 - eps ; U[L] = eps*piB(T_s) ;  for i = L-1 .. 0:
 *     m1 = 1/(1 - R_i*Rs[i+1])
 *     U[i] = S_i + T_i*((U[i+1] + Rs[i+1]*S_i)*m1)
 *     Rs[i] = R_i + T_i*((T_i*Rs[i+1])*m1)
 *   down, from space:  Dn = 0, Rd = 0 ;  at every interface i = 0 .. L:
 *     m2 = 1/(1 - Rd*Rs[i])
 *     down[i] = (Dn + Rd*U[i])*m2 ; up[i] = (U[i] + Rs[i]*Dn)*m2
 *     then through level i:  m3 = 1/(1 - Rd*R_i)
 *     Dn = S_i + T_i*((Dn + Rd*S_i)*m3) ; Rd = R_i + T_i*((T_i*Rd)*m3)
 * Outputs (device, NULL: not wanted; at least one is; none of them beta or work), on the grid
 * [W m-2 (cm-1)-1]: up_rows and down_rows ([level_count][row_stride]): the two fluxes at the
 * interface below each level (nearer the surface); top_up_rows and top_down_rows
 * ([n_paths][row_stride]): the same at interface 0 of the run's paths (top_down_rows is 0 and
 * top_up_rows is U[0] bit for bit).  With n_bands > 0 the four *_mean outputs
 * ([level_count][n_bands] and [n_paths][n_bands]) receive lbl_path_compute's ordered band means of
 * the rows of the same name, which must be given too; NaN for a band without points.
 * LBL_BAD_ARGUMENT for bad shapes, an unknown grid, a run that cuts a path, other flags, a level
 * table that is negative or not finite or has w_c > tau_c, g_c outside [0, 1) or T_l <= 0, a
 * diffusivity outside [1, 2], a surface temperature <= 0, an emissivity outside [0, 1], both or
 * neither emissivity, an output that is beta or work, no output at all, or a band mean without its
 * rows or without bands; nothing is launched and the engine stays usable. */
int lbl_path_thermal_two_stream(lbl_engine *engine, double *beta, int64_t row_stride,
                                int64_t columns, int32_t grid, int32_t n_paths,
                                int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                                const double *level_table, double diffusivity,
                                const double *surface_temperature, const double *emissivity_rows,
                                const double *emissivity, int32_t n_bands,
                                const int64_t *band_start, double *work, double *up_rows,
                                double *down_rows, double *top_up_rows, double *top_down_rows,
                                double *up_mean, double *down_mean, double *top_up_mean,
                                double *top_down_mean, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
