/* lbl_amd_solar_radiance.h: the scattered-sunlight radiance entry of liblbl_amd.so, beside
 * lbl_amd.h. */
#ifndef LBL_AMD_SOLAR_RADIANCE_H_
#define LBL_AMD_SOLAR_RADIANCE_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sunlight scattered to a sensor (Spectroscopy.compute_solar_radiance): the radiance a viewer
 * above the atmosphere sees along one zenith cosine and one azimuth per path, by the two-stream
 * source-function technique (Toon et al. 1989): the fluxes of lbl_path_two_stream
 * (lbl_amd_twostream.h) are the source of multiply scattered light, the singly scattered direct
 * beam is treated with the true phase functions (the TMS correction of Nakajima & Tanaka 1988),
 * and the transfer equation is integrated exactly along the viewing direction (kernel:
 * pylbl_amd/csrc/solar_radiance.h).  This entry extends the C ABI of lbl_amd.h, which this header
 * includes and leaves as it is; it is exported by the same library and takes the same engine,
 * flags and status codes.
 *
 * lbl_path_solar_radiance takes a run of whole paths.  beta (read only), row_stride, columns,
 * n_paths, levels_per_path, level_begin, level_count, level_table, solar_zenith_cosine,
 * solar_row, rayleigh_row, albedo_rows, albedo, n_bands and band_start as for
 * lbl_path_two_stream, and the same flags: LBL_PATH_FROM_LAST (the surface lies behind level 0 of
 * each path and space behind its last level; without it the other way round) and LBL_ASYNC.  Where
 * a level holds a scatterer (w_c > 0) the table needs h_c < w_c.
 *   view_cosine (host, [n_paths]): mu in (0, 1], the viewing zenith cosine of each path;
 *   scattering_cosine (host, [n_paths]): cosT in [-1, 1], the cosine of the angle between the
 *   directions of propagation of the sunlight and of the viewed light;
 *   up_rows, direct_rows, diffuse_rows (device, [level_count][row_stride], read only): the
 *   two-stream fluxes at the interface below each level (nearer the surface), as
 *   lbl_path_two_stream writes them for the same run, table, Sun and surface.
 * Inputs.  The level row (s_l, c_l, tau_c, w_c, h_c), sigma(nu), A, F0 = mu0*S and every layer
 * scalar are lbl_path_two_stream's, bit for bit:
 *   tau_a = s_l*beta ; tau_R = c_l*sigma ; tau = (tau_a + tau_R) + tau_c ; tau_s = tau_R + w_c
 *   omega = tau_s/tau ; g = h_c/tau_s ; f = g*g ; sc = 1 - omega*f ; t = sc*tau
 *   w = ((1 - f)*omega)/sc ; gp = g/(1 + g) ; g2 = (3*(w*(1 - gp)))/4 ; dif = 2*(1 - w)
 *   g1 = g2 + dif ; su = g1 + g2 ; g3 = (2 - 3*(mu0*gp))/4 ; g4 = 1 - g3 ; k2 = dif*su
 *   a1 = g1*g4 + g2*g3 ; a2 = g1*g3 + g2*g4
 *   conservative, where k2*(1 + t*t) <= 1e-10: m = mu0
 *   general: k = sqrt(k2) ; m = mu0 ; x = k*m
 *     if |1 - x| < 1e-4: m = (x >= 1 ? (1 + 1e-4) : (1 - 1e-4))/k ; x = k*m
 *     E = exp(-(k*t))
 *   Dm = exp(-t/m)
 * Inside the guard around k*mu0 = 1 the level uses the moved cosine m for the beam, in its
 * particular solution and in its single scattering, as the flux rows do.
 * up[i], diffuse[i], direct[i]: the fluxes at interface i; level i lies between interfaces i
 * (space side) and i + 1, interface 0 faces space, and direct[0] = F0 and diffuse[0] = 0 are
 * constants, not read.  pi = numpy.pi.
 * Model.  tau' in [0, t] is measured from the level's space-side face and S_i = direct[i]:
 *   Dv = exp(-t/mu) ; a = (3*(gp*mu))/2
 *   beam       B(tau') = S_i*exp(-tau'/m)
 *   diffuse    F+(tau'), F-(tau'): the two-stream solution in the level (below)
 *   source     J(tau') = (w/(2 pi))*[F+(tau')(1 + a) + F-(tau')(1 - a)]
 *                      + ((omega/sc)*Pmix/(4 pi))*(S_i/m)*exp(-tau'/m)
 *   Pmix = (tau_R*PR + w_c*PH)/tau_s ;  PR = (3/4)(1 + cosT^2)
 *   PH = (1 - gc^2)/(1 + gc^2 - 2 gc cosT)^(3/2),  gc = h_c/w_c  (0 where w_c == 0)
 *   transfer   I_top = I_bot*Dv + Integral_0^t J(tau') exp(-tau'/mu) dtau'/mu
 * F+- solve the Meador-Weaver equations
 *   dF+/dtau' = g1 F+ - g2 F- - w g3 (B/m) ;  dF-/dtau' = g2 F+ - g1 F- + w g4 (B/m)
 * whose particular solution Z+- exp(-tau'/m) has, with X = (1 - x)*(1 + x) (X = 1, conservative),
 * per path and column, each product, sum and quotient rounded as written (no fused multiply-add):
 *   ws = w*S_i ; Z+ = (ws*(g3 - a2*m))/X ; Z- = -((ws*(g4 + a1*m))/X)
 *   u1 = up[i+1] - Z+*Dm ; d0 = diffuse[i] - Z-
 *   bm = (m/(m + mu))*(-expm1(-(t/m + t/mu)))
 *   I_top = I_bot*Dv + (w/(2 pi))*C + (((omega/sc)*Pmix)/(4 pi))*((S_i/m)*bm)
 * general:
 *   Gamma = g2/(g1 + k) ; n = 1 - (Gamma*E)*(Gamma*E)
 *   P = (u1 - (Gamma*E)*d0)/n ; Q = (d0 - (Gamma*E)*u1)/n
 *   C = P*((1 + a) + Gamma*(1 - a))*h + Q*(Gamma*(1 + a) + (1 - a))*((1 - E*Dv)/(1 + k*mu))
 *       + (Z+*(1 + a) + Z-*(1 - a))*bm
 *   h = (E - Dv)/(1 - k mu), formed without its pole and without overflow:
 *     y = ((1 - k*mu)*t)/mu ; phi(z) = -expm1(-z)/z for z > 0, phi(0) = 1
 *     h = E*((t/mu)*phi(y)) for y >= 0 ; h = Dv*((t/mu)*phi(-y)) for y < 0
 * conservative:
 *   x = g1*t ; N = (u1 - d0)/(1 + x) ; Ev = -expm1(-t/mu)
 *   C = ((u1 + d0) - x*N + a*N)*Ev + (2*(g1*N))*(mu*W) + (Z+*(1 + a) + Z-*(1 - a))*bm
 *   W = Ev - (t/mu)*Dv, formed without its cancellation as
 *     W = (t/mu)*(Ev - linear_weight(t/mu, Ev))
 *     (linear_weight: lbl_path_radiance_source's w = 1 - Ev/(t/mu) in its two-branch form)
 * Special levels.  tau == 0: the identity.  tau_s == 0: I_top = I_bot*exp(-tau/mu).  Without a
 * Rayleigh row a level with w_c == 0 reads no flux row.
 * Surface and result.  I_L = A*((direct[L] + diffuse[L])/pi): a Lambertian surface.  The result is
 * I at interface 0.  The diffuse field is two-stream: against a multi-stream code radiances are
 * good to several per cent; the single scattering is exact.
 * Outputs (device; neither beta nor a flux row), on the grid, [n_paths][row_stride], the rows of
 * the run's paths: radiance_rows [W m-2 sr-1 (cm-1)-1].  With n_bands > 0 radiance_mean
 * ([n_paths][n_bands]) receives lbl_path_compute's ordered band means of radiance_rows; NaN for a
 * band without points.
 * LBL_BAD_ARGUMENT for any of lbl_path_two_stream's shape, run, flag, table, cosine and albedo
 * errors, a scatterer with h_c >= w_c, a view cosine outside (0, 1], a scattering cosine outside
 * [-1, 1] or not finite, a flux row that is NULL, an output that is beta or a flux row, no output
 * at all, or a band mean without its rows or without bands; nothing is launched and the engine
 * stays usable. */
int lbl_path_solar_radiance(lbl_engine *engine, double *beta, int64_t row_stride, int64_t columns,
                            int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                            int32_t level_count, const double *level_table,
                            const double *solar_zenith_cosine, const double *view_cosine,
                            const double *scattering_cosine, const double *solar_row,
                            const double *rayleigh_row, const double *albedo_rows,
                            const double *albedo, const double *up_rows,
                            const double *direct_rows, const double *diffuse_rows,
                            int32_t n_bands, const int64_t *band_start, double *radiance_rows,
                            double *radiance_mean, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
