/* lbl_amd_twostream.h: the two-stream shortwave entries of liblbl_amd.so, beside lbl_amd.h. */
#ifndef LBL_AMD_TWOSTREAM_H_
#define LBL_AMD_TWOSTREAM_H_

#include "lbl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two-stream shortwave fluxes with scattering (Spectroscopy.compute_solar_flux): upward, downward,
 * direct and diffuse fluxes at every interface of whole paths, plane-parallel, from a delta-scaled
 * PIFM layer solution and the adding recurrences (kernels: pylbl_amd/csrc/twostream.h).  These two
 * entries extend the C ABI of lbl_amd.h, which this header includes and leaves as it is; they are
 * exported by the same library and take the same engine, grid handles, flags and status codes.
 *
 * lbl_rayleigh_row fills row[j] = sigma(nu_j) [m2], the Rayleigh scattering cross-section per
 * molecule of air, for the first `columns` points nu_j of `grid` (a handle of lbl_grid_load):
 *   cross_section == NULL: Bucholtz (1995) with lambda = 1e4/nu in um,
 *   sigma = 1e-4*A*lambda^-(B + C*lambda + D/lambda), formed as (1e-4*A)*exp(-(e*log(lambda))) with
 *   e = (B + C*lambda) + D/lambda; lambda <= 0.5: A = 3.01577e-28, B = 3.55212, C = 1.35579,
 *   D = 0.11563; lambda > 0.5: A = 4.01061e-28, B = 3.99668, C = 1.10298e-3, D = 2.71393e-2; the
 *   fits are used as they are outside 0.2 .. 4 um; sigma = 0 for nu <= 0;
 *   cross_section (host, [columns], finite and >= 0): the values on the grid as they are.
 *   row (device, >= columns values).  flags: LBL_ASYNC or 0.
 * LBL_BAD_ARGUMENT (message in lbl_last_error) for an unknown grid, columns outside the grid, or
 * cross-sections that are negative or not finite; nothing is launched and the engine stays usable.
 *
 * lbl_path_two_stream takes a run of whole paths.  beta (read only), row_stride, columns, n_paths,
 * levels_per_path, level_begin, level_count, n_bands and band_start as for lbl_path_jacobian:
 * level_begin and level_count are multiples of levels_per_path, nothing is carried between calls.
 * Flags: LBL_PATH_FROM_LAST (the surface lies behind level 0 of each path and the Sun shines in at
 * its last level; without it the other way round) and LBL_ASYNC.
 *   level_table (host, [level_count][5], finite and >= 0, h_c <= w_c <= tau_c): per level
 *   s_l [m], c_l [m-2] (the air column (p_l/(K_B*T_l))*s_l, 0: no Rayleigh scattering), tau_c (the
 *   extinction optical depth of a grey scatterer), w_c = omega_c*tau_c and h_c = (omega_c*tau_c)*g_c;
 *   solar_zenith_cosine (host, [n_paths]): mu0 of each path, in (0, 1];
 *   solar_row (device, >= columns values): S, e.g. lbl_solar_spectrum's row;
 *   rayleigh_row (device, >= columns values, or NULL: sigma = 0): e.g. lbl_rayleigh_row's row;
 *   albedo_rows (device, [n_paths][row_stride]) or albedo (host, [n_paths], in [0, 1]): the
 *   Lambertian albedo A; exactly one of them;
 *   work (device, [level_count][2][row_stride]): Rup and Rupd at the interface above each level.
 * Per path and column, each product, sum and quotient rounded as written (no fused multiply-add):
 *   tau_a = s_l*beta ;  tau_R = c_l*sigma(nu) ;  tau = (tau_a + tau_R) + tau_c
 *   tau_s = tau_R + w_c ;  omega = tau_s/tau ;  g = h_c/tau_s  (g = 0 where tau_s == 0)
 *   tau == 0: the layer is the identity (Rdif = Rdir = Tdp = 0, Tdif = D = 1)
 *   f = g*g ; sc = 1 - omega*f ; t = sc*tau ; w = ((1 - f)*omega)/sc ; gp = g/(1 + g)
 *   g2 = (3*(w*(1 - gp)))/4 ; dif = 2*(1 - w) ; g1 = g2 + dif ; su = g1 + g2
 *   g3 = (2 - 3*(mu0*gp))/4 ; g4 = 1 - g3 ; k2 = dif*su ; D = exp(-t/mu0)
 *   where k2*(1 + t*t) <= 1e-10 (the conservative branch):
 *     x = g1*t ; Rdif = x/(1 + x) ; Tdif = 1/(1 + x)
 *     Rdir = (x + (g3 - g1*mu0)*(-expm1(-t/mu0)))/(1 + x) ; Tdp = (1 - Rdir) - D
 *   else (Meador and Weaver 1980, scaled by exp(-k t)):
 *     k = sqrt(k2) ; m = mu0 ; x = k*m
 *     if |1 - x| < 1e-4: m = (x >= 1 ? (1 + 1e-4) : (1 - 1e-4))/k ; x = k*m
 *     Dm = exp(-t/m) ; E = exp(-(k*t)) ; E2 = E*E ; o1 = -expm1(-(2*(k*t)))
 *     den = k*(1 + E2) + g1*o1 ; q = ((1 - x)*(1 + x))*den
 *     Rdif = (g2*o1)/den ; Tdif = (2*(k*E))/den
 *     a1 = g1*g4 + g2*g3 ; a2 = g1*g3 + g2*g4
 *     Rdir = w*((1 - x)*(a2 + k*g3) - ((1 + x)*(a2 - k*g3))*E2 - (2*(k*(g3 - a2*m)))*(E*Dm))/q
 *     Ttot = Dm*(1 - w*((1 + x)*(a1 + k*g4) - ((1 - x)*(a1 - k*g4))*E2)/q) + w*((2*(k*(g4 + a1*m)))*E)/q
 *     Tdp = Ttot - Dm
 *   Adding, interface 0 facing space, level i between interfaces i and i + 1 in the Sun's order,
 *   F0 = mu0*S:
 *   up, from the surface:  Rup[L] = Rupd[L] = A ;  for i = L-1 .. 0:
 *     m1 = 1/(1 - Rdif_i*Rupd[i+1])
 *     Rup[i] = Rdir_i + Tdif_i*((Tdp_i*Rupd[i+1] + D_i*Rup[i+1])*m1)
 *     Rupd[i] = Rdif_i + Tdif_i*((Tdif_i*Rupd[i+1])*m1)
 *   down, from space:  Tb = 1, Td = 0, Rd = 0 ;  at every interface i = 0 .. L:
 *     m2 = 1/(1 - Rd*Rupd[i])
 *     direct[i] = F0*Tb ; diffuse_down[i] = F0*((Td + (Tb*Rup[i])*Rd)*m2)
 *     up[i] = F0*((Tb*Rup[i] + Td*Rupd[i])*m2) ; down[i] = direct[i] + diffuse_down[i]
 *     then through level i:  m3 = 1/(1 - Rd*Rdif_i)
 *     Td = Tb*Tdp_i + Tdif_i*((Td + (Tb*Rd)*Rdir_i)*m3) ; Rd = Rdif_i + Tdif_i*((Tdif_i*Rd)*m3)
 *     Tb = Tb*D_i
 * Against the two-stream equations themselves (tests/two_stream_ode_cases.py solves them without
 * these closed forms) the layer is exact to rounding, except: the conservative branch neglects
 * up to its criterion, 1e-10 (measured 4.8e-11 of F0 per layer); and inside the guard
 * |1 - k*mu0| < 1e-4 the layer is solved at the moved mu0, which puts Rdir and Tdp off by up to
 * 0.12*(1e-4 - |1 - k*mu0|) of F0 (measured, g_c <= 0.9): 1.2e-5 of F0 at k*mu0 = 1 under
 * mu0 = 1, falling linearly to 0 at the guard's edges.
 * Outputs (device, NULL: not wanted; at least one is; none of them beta or work), on the grid
 * [W m-2 (cm-1)-1]: up_rows, down_rows, direct_rows and diffuse_rows ([level_count][row_stride]):
 * the four fluxes at the interface below each level (nearer the surface); top_up_rows,
 * top_down_rows, top_direct_rows and top_diffuse_rows ([n_paths][row_stride]): the same at
 * interface 0 of the run's paths (top_direct_rows is F0 bit for bit).  With n_bands > 0 the eight
 * *_mean outputs ([level_count][n_bands] and [n_paths][n_bands]) receive lbl_path_compute's ordered
 * band means of the rows of the same name, which must be given too; NaN for a band without points.
 * LBL_BAD_ARGUMENT for bad shapes, a run that cuts a path, other flags, a level table that is
 * negative, not finite or not ordered, a cosine outside (0, 1], an albedo outside [0, 1], both or
 * neither albedo, an output that is beta or work, no output at all, or a band mean without its
 * rows or without bands; nothing is launched and the engine stays usable. */
int lbl_rayleigh_row(lbl_engine *engine, int32_t grid, int64_t columns,
                     const double *cross_section, double *row, int32_t flags);
int lbl_path_two_stream(lbl_engine *engine, double *beta, int64_t row_stride, int64_t columns,
                        int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                        int32_t level_count, const double *level_table,
                        const double *solar_zenith_cosine, const double *solar_row,
                        const double *rayleigh_row, const double *albedo_rows,
                        const double *albedo, int32_t n_bands, const int64_t *band_start,
                        double *work, double *up_rows, double *down_rows, double *direct_rows,
                        double *diffuse_rows, double *top_up_rows, double *top_down_rows,
                        double *top_direct_rows, double *top_diffuse_rows, double *up_mean,
                        double *down_mean, double *direct_mean, double *diffuse_mean,
                        double *top_up_mean, double *top_down_mean, double *top_direct_mean,
                        double *top_diffuse_mean, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
