/* lbl_amd_thermal_source.h: the two-stream longwave entry of liblbl_amd.so with a source that is
 * linear in optical depth, beside lbl_amd.h and lbl_amd_thermal.h. */
#ifndef LBL_AMD_THERMAL_SOURCE_H_
#define LBL_AMD_THERMAL_SOURCE_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two-stream longwave fluxes through clouds with a linear-in-tau source
 * (Spectroscopy.compute_thermal_flux_linear): lbl_path_thermal_two_stream (lbl_amd_thermal.h) with
 * the Planck function varying linearly in every layer's optical depth between the values at its
 * two interfaces, as lbl_path_flux_source does for the clear sky (kernels:
 * pylbl_amd/csrc/twostream_thermal_source.h).  This entry extends the C ABI of lbl_amd.h, which
 * this header includes and leaves as it is; it is exported by the same library and takes the same
 * engine, grid handles, flags and status codes.
 *
 * lbl_path_thermal_two_stream_source takes lbl_path_thermal_two_stream's arguments, with the same
 * meaning, shapes and checks, and behind level_table
 *   edge_temperature (host, [level_count][2], finite and > 0): the interface temperatures [K] of
 *   flat level level_begin + r, [r][0] on its first-level side and [r][1] on its last-level side,
 *   as for lbl_path_flux_source; inside a path [r][1] == [r + 1][0].
 * T_l of the level table is checked (> 0) and not used; surface_temperature T_s stays apart from
 * the interface temperature at the surface.
 * With piB(T) = pi*B(nu, T), pi = numpy.pi and B as in lbl_path_radiance (0 for nu <= 0), per path
 * and column, each product, sum and quotient rounded as written (no fused multiply-add):
 *   tau_a = s_l*beta ; tau = tau_a + tau_c
 *   clear level (w_c == 0, the same for the whole wavefront):
 *     x = D*tau ; R = 0 ; T = exp(-x) ; em = -expm1(-x)
 *     q = a - linear_weight(x, a)
 *       (a = em; linear_weight(x, a) is lbl_path_radiance_source's w: 1 - a/x for |x| >= 1/16, its
 *       8-term series below)
 *   cloudy level (w_c > 0; f = g_c*g_c and gp = g_c/(1 + g_c) are level scalars):
 *     omega = w_c/tau ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc
 *     g2 = (D*(w*(1 - gp)))/2 ; dif = D*(1 - w) ; g1 = g2 + dif ; su = g1 + g2 ; k2 = dif*su
 *     conservative, where k2*(1 + t*t) <= 1e-10:
 *       x = g1*t ; R = x/(1 + x) ; T = 1/(1 + x) ; em = (dif*t)/(1 + x)
 *       q = ((dif*t)*(1 + (su*t)/3))/(2*(1 + x))
 *     general:
 *       k = sqrt(k2) ; E = exp(-(k*t)) ; E2 = E*E ; o1 = -expm1(-(2*(k*t)))
 *       den = k*(1 + E2) + g1*o1 ; R = (g2*o1)/den ; T = (2*(k*E))/den
 *       em = (k*((1 - E)*(1 - E)) + dif*o1)/den        (= 1 - R - T, without the cancellation)
 *       y = k*t ; z = y*y
 *       p = o1 - 2*(y*E)        for y >= 1/2, and for y < 1/2
 *       p = E*(((y*z)/3)*(1 + z*(1/20 + z*(1/840 + z*(1/60480 + z*(1/6652800 + z*(1/1037836800
 *           + z*(1/217945728000 + z*(1/59281238016000)))))))))
 *       q = ((k*(o1*o1))/(su*((1 + E)*(1 + E))) + p)/(den*t)
 *         (o1/(1 + E) is 1 - E without its cancellation)
 *   Bt = piB(T at the level's space-side interface) ; Bb = piB(T at its surface-side interface)
 *   dB = Bb - Bt
 *   S_up = Bt*em + dB*q        what the layer sends out of its space-side face
 *   S_dn = Bb*em - dB*q        what it sends out of its surface-side face
 *   (q = (1 - T + R)/(su*t) - T, from the particular solution F+- = pi*(B(tau) +- B'/su), formed
 *   without the difference; with dB = 0 both are Bt*em and the call has
 *   lbl_path_thermal_two_stream's bits)
 *   Adding, interface 0 facing space, level i between interfaces i and i + 1 in the order space ->
 *   surface:
 *   up, from the surface:  Rs[L] = 1 - eps ; U[L] = eps*piB(T_s) ;  for i = L-1 .. 0:
 *     m1 = 1/(1 - R_i*Rs[i+1])
 *     U[i] = S_up_i + T_i*((U[i+1] + Rs[i+1]*S_dn_i)*m1)
 *     Rs[i] = R_i + T_i*((T_i*Rs[i+1])*m1)
 *   down, from space:  Dn = 0, Rd = 0 ;  at every interface i = 0 .. L:
 *     m2 = 1/(1 - Rd*Rs[i])
 *     down[i] = (Dn + Rd*U[i])*m2 ; up[i] = (U[i] + Rs[i]*Dn)*m2
 *     then through level i:  m3 = 1/(1 - Rd*R_i)
 *     Dn = S_dn_i + T_i*((Dn + Rd*S_up_i)*m3) ; Rd = R_i + T_i*((T_i*Rd)*m3)
 * Outputs, band means and work as for lbl_path_thermal_two_stream (top_down_rows is 0 and
 * top_up_rows is U[0] bit for bit).
 * LBL_BAD_ARGUMENT for everything lbl_path_thermal_two_stream refuses and for edge temperatures
 * that are NULL, not finite, <= 0 or not continuous within a path; nothing is launched and the
 * engine stays usable. */
int lbl_path_thermal_two_stream_source(lbl_engine *engine, double *beta, int64_t row_stride,
                                       int64_t columns, int32_t grid, int32_t n_paths,
                                       int32_t levels_per_path, int32_t level_begin,
                                       int32_t level_count, const double *level_table,
                                       const double *edge_temperature, double diffusivity,
                                       const double *surface_temperature,
                                       const double *emissivity_rows, const double *emissivity,
                                       int32_t n_bands, const int64_t *band_start, double *work,
                                       double *up_rows, double *down_rows, double *top_up_rows,
                                       double *top_down_rows, double *up_mean, double *down_mean,
                                       double *top_up_mean, double *top_down_mean, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
