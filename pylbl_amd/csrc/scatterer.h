// Spectral cloud and aerosol optics of the two-stream kernels (lbl_path_two_stream_spectral,
// lbl_path_thermal_two_stream_spectral; include/lbl_amd_scatterer.h states the definition): the
// scatterer of a level is a table of (tau_c, omega_c, g_c) at M knots k_0 < ... < k_{M-1} [cm-1],
// interpolated linearly in wavenumber and constant outside the knots.  The TU builds with
// -ffp-contract=off: every product, sum and quotient below is rounded as written.
//
// Per column (grid point nu), once per lane and sweep (scatterer_lane):
//   j = the largest index with k_j <= nu, limited to 0 .. M-2
//   u = (nu - k_j)/(k_{j+1} - k_j), limited to [0, 1]
// Per level, column and e in {tau_c, omega_c, g_c} (scatterer_value):
//   v = e_j + u*(e_{j+1} - e_j), then limited to [min(e_j, e_{j+1}), max(e_j, e_{j+1})]
// The limit makes what the grey layer needs hold per element whatever the rounding does: tau_c >=
// 0, 0 <= omega_c <= 1, 0 <= g_c < 1; a table that is flat in nu gives its value bit for bit (the
// difference is 0 and the limit is [c, c]).
//
// Where the rows live: the device copy is [level][3][M], read with per-lane loads.  j differs from
// lane to lane, so the scalar unit cannot fetch the values; neighbouring lanes read the same or
// the adjacent 16 bytes of a row of at most 8 KB, which the vector cache serves, and a level's
// six values per column are loaded together ahead of the layer's arithmetic.  The knots are read
// in the binary search only (at most 10 steps, before the sweep; the first steps are the same
// address for the whole wavefront).
#pragma once

#include <hip/hip_runtime.h>

#include "path.h"

namespace lbl {

constexpr int kScattererMaxKnots = 1024;    // as lbl_surface_emissivity's
constexpr int kScattererWords = 3;          // tau_c, omega_c, g_c per level and knot

struct ScattererKnots
{
    const double * nu;          // [columns]: the grid [cm-1]
    const double * knot;        // [n_knots]: k_0 < ... < k_{M-1}
    const double * optics;      // [count][3][n_knots]: tau_c, omega_c, g_c of flat level first + i
    int n_knots;
};

// Where a lane's columns lie among the knots: the same for every level of its sweep.
struct ScattererLane
{
    int j[kPathWidth];
    double u[kPathWidth];
};

// nu: the lane's columns of the grid (a column beyond the lane's width may hold anything: its j
// stays inside 0 .. M-2).
__device__ __forceinline__ ScattererLane scatterer_lane(const ScattererKnots & s,
                                                        const double (&nu)[kPathWidth])
{
    ScattererLane lane;
#pragma unroll
    for (int i = 0; i < kPathWidth; ++i)
    {
        int lo = 0, hi = s.n_knots - 1;
        while (hi - lo > 1)
        {
            const int mid = (lo + hi) >> 1;
            if (s.knot[mid] <= nu[i]) lo = mid; else hi = mid;
        }
        const double k0 = s.knot[lo], k1 = s.knot[lo + 1];
        const double u = (nu[i] - k0)/(k1 - k0);
        lane.j[i] = lo;
        lane.u[i] = fmin(fmax(u, 0.), 1.);
    }
    return lane;
}

// The three rows [3][n_knots] of the level at index `index` of the per-level tables.
__device__ __forceinline__ const double * scatterer_rows(const ScattererKnots & s, int index)
{
    return s.optics + (long long)index*(kScattererWords*s.n_knots);
}

// One row of a level at a column: row[j] and row[j + 1] interpolated and limited.
__device__ __forceinline__ double scatterer_value(const double * row, int j, double u)
{
    const double e0 = row[j], e1 = row[j + 1];
    const double v = e0 + u*(e1 - e0);
    return fmin(fmax(v, fmin(e0, e1)), fmax(e0, e1));
}

}  // namespace lbl
