/* lbl_amd_thermal_radiance.h: the all-sky radiance entry of liblbl_amd.so, beside lbl_amd.h. */
#ifndef LBL_AMD_THERMAL_RADIANCE_H_
#define LBL_AMD_THERMAL_RADIANCE_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sounder radiances through clouds (Spectroscopy.compute_thermal_radiance): the radiance a viewer
 * above the atmosphere sees along one zenith cosine per path, by the two-stream source-function
 * technique (Toon et al. 1989): the fluxes of lbl_path_thermal_two_stream (lbl_amd_thermal.h) are
 * the scattering source, and the transfer equation is integrated exactly along the viewing
 * direction (kernel: pylbl_amd/csrc/thermal_radiance.h).  This entry extends the C ABI of
 * lbl_amd.h, which this header includes and leaves as it is; it is exported by the same library
 * and takes the same engine, grid handles, flags and status codes.
 *
 * lbl_path_thermal_radiance takes a run of whole paths.  beta (read only), row_stride, columns,
 * grid, n_paths, levels_per_path, level_begin, level_count, level_table, diffusivity,
 * surface_temperature, emissivity_rows, emissivity, n_bands and band_start as for
 * lbl_path_thermal_two_stream, and the same flags: LBL_PATH_FROM_LAST (the surface lies behind
 * level 0 of each path and space behind its last level; without it the other way round) and
 * LBL_ASYNC.
 *   view_cosine (host, [n_paths]): mu in (0, 1], the viewing zenith cosine of each path;
 *   up_rows, down_rows (device, [level_count][row_stride], read only): the two-stream fluxes at
 *   the interface below each level (nearer the surface), as lbl_path_thermal_two_stream writes
 *   them for the same run, table, D and surface.
 * Inputs.  Per level l the table row is (s_l, tau_c, w_c, g_c, T_l) and D the diffusivity factor:
 * lbl_path_thermal_two_stream's, bit for bit, with its tau, the clear/cloudy branch and
 *   omega = w_c/tau ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc
 *   g2 = (D*(w*(1 - gp)))/2 ; dif = D*(1 - w) ; g1 = g2 + dif ; su = g1 + g2 ; k2 = dif*su
 *   conservative, where k2*(1 + t*t) <= 1e-10 ; general: k = sqrt(k2) ; E = exp(-(k*t))
 * up[i], down[i]: the fluxes at interface i; level i lies between interfaces i and i + 1,
 * interface 0 faces space and down[0] = 0 is a constant, not read.  B = B(nu, T_l) as in
 * lbl_path_radiance (0 for nu <= 0) and piB = pi*B, pi = numpy.pi.
 *   gp = g_c/(1 + g_c) ; a = (3*(gp*mu))/2
 * Model.  Within a level the source is J(tau) = B + (w/(2 pi))*[f+(tau)(1 + a) + f-(tau)(1 - a)]
 * with f+- = F+- - piB: the two-stream phase function 1 + 3 g' mu mu' with hemispherically
 * isotropic I+- = F+-/pi.  Per path and column, each product, sum and quotient rounded as written
 * (no fused multiply-add), with
 *   u1 = up[i+1] - piB ; d0 = down[i] - piB ; Dm = exp(-t/mu) ; Em = -expm1(-t/mu)
 * the level maps the radiance entering its surface-side face, I_bot, to
 *   I_top = I_bot*Dm + B*Em + (w/(2 pi))*C
 * clear level (w_c == 0):  x = tau/mu and C = 0:
 *   I_top = I_bot*exp(-x) + B*(-expm1(-x))
 *   (lbl_path_radiance's lines: mu = 1 without tau_c gives its bits)
 * cloudy, general:
 *   Gamma = g2/(g1 + k) ; n = 1 - (Gamma*E)*(Gamma*E)
 *   P = (u1 - (Gamma*E)*d0)/n ; Q = (d0 - (Gamma*E)*u1)/n
 *   C = P*((1 + a) + Gamma*(1 - a))*h + Q*(Gamma*(1 + a) + (1 - a))*((1 - E*Dm)/(1 + k*mu))
 *   h = (E - Dm)/(1 - k mu), formed without its pole and without overflow:
 *     y = ((1 - k*mu)*t)/mu ; phi(z) = -expm1(-z)/z for z > 0, phi(0) = 1
 *     h = E*((t/mu)*phi(y)) for y >= 0 ; h = Dm*((t/mu)*phi(-y)) for y < 0
 * cloudy, conservative:
 *   x = g1*t ; N = (u1 - d0)/(1 + x)
 *   C = ((u1 + d0) - x*N + a*N)*Em + (2*(g1*N))*(mu*W)
 *   W = Em - (t/mu)*Dm, formed without its cancellation as
 *     W = (t/mu)*(Em - linear_weight(t/mu, Em))
 *     (linear_weight: lbl_path_radiance_source's w = 1 - Em/(t/mu) in its two-branch form)
 * Surface and result.  I_L = eps*B(T_s) + (1 - eps)*(down[L]/pi): a Lambertian surface.  The
 * result is I at interface 0.
 * Outputs (device, NULL: not wanted; at least one is; none of them beta or a flux row), on the
 * grid, [n_paths][row_stride], the rows of the run's paths: radiance_rows [W m-2 sr-1 (cm-1)-1]
 * and brightness_rows [K], inverted as lbl_path_radiance inverts.  With n_bands > 0
 * radiance_mean ([n_paths][n_bands]) receives lbl_path_compute's ordered band means of
 * radiance_rows, which must be given too; NaN for a band without points.
 * LBL_BAD_ARGUMENT for any of lbl_path_thermal_two_stream's shape, grid, run, flag, table,
 * diffusivity and surface errors, a view cosine outside (0, 1] or not finite, a flux row that is
 * NULL, an output that is beta or a flux row, no output at all, or a band mean without its rows or
 * without bands; nothing is launched and the engine stays usable. */
int lbl_path_thermal_radiance(lbl_engine *engine, double *beta, int64_t row_stride,
                              int64_t columns, int32_t grid, int32_t n_paths,
                              int32_t levels_per_path, int32_t level_begin, int32_t level_count,
                              const double *level_table, double diffusivity,
                              const double *view_cosine, const double *surface_temperature,
                              const double *emissivity_rows, const double *emissivity,
                              const double *up_rows, const double *down_rows, int32_t n_bands,
                              const int64_t *band_start, double *radiance_rows,
                              double *brightness_rows, double *radiance_mean, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
