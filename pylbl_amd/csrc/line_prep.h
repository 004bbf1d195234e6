// Per-line physics ("K1"): turns one HITRAN transition and one atmospheric level into
// the handful of scalars the accumulate kernel needs.
//
// Reference statement: pyLBL/c_lib/spectra.c:12-62 (pressure shift, Lorentz and Doppler
// widths, line-strength temperature scaling, window indices) and the first lines of
// pyLBL/c_lib/voigt.c:7-15,33-34 (repwid, y, far-wing limit).  Operation order of every
// expression follows the reference; the translation unit is compiled with
// -ffp-contract=off so no multiply-add is fused here.
//
// What is hoisted out of the per-line work (it depends on the level and isotopologue
// only) and done once on the host: p, p*x, 296/T, sqrt(2 ln2 R T / M_iso) and the TIPS
// ratio Q_iso(296)/Q_iso(T) (spectral_database.c:97-104) -- see LevelScalars.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace lbl {

constexpr int kMassSlots = 32;          // absorption.c:62 (double mass[32])
constexpr double kPi = 3.14159265358979323846;

// Scalars of one atmospheric level, prepared on the host.
struct LevelScalars
{
    double temperature;     // T [K]
    double p_atm;           // P*9.86923e-6                      spectra.c:17
    double p_partial;       // p*x                               spectra.c:18
    double tfact;           // 296/T                             spectra.c:19
    double t_minus_ref;     // T - 296                           spectra.c:33
    double t_times_ref;     // T*296                             spectra.c:33
    double shift_max;       // bound on |p*delta_air| over the table (+ margin)
    double core_reach;      // bound on (far-wing limit / repwid) / nu over the table
    double density;         // P x /(kb T)                       spectroscopy.py:18-29
    double inner_possible;  // 0: y >= 8.425 for every line of this call at this level, i.e. no line
                            // has points in the inner regions (voigt.c:35-43); else 1
    double doppler[kMassSlots];   // sqrt(2 ln2 * 8314.472 * T / mass[iso])   spectra.c:29
    double q_ratio[kMassSlots];   // Q(296)/Q(T) per isotopologue             spectra.c:41-42
};

struct GridSpec
{
    int v0, vn, n_per_v, cut_off;
    int n;                  // (vn - v0)*n_per_v                 absorption.c:34
    double dv;              // 1./n_per_v                        absorption.c:33
};

// What the accumulate kernel reads per line and level.  Two 32-byte halves so that the
// far-wing loop (the >99 % case) touches only the first.
struct alignas(32) LineWing
{
    double centre;          // nu + p*delta_air                  spectra.c:22
    double g2;              // gamma^2
    double bl;              // S*gamma/pi: Lorentz amplitude (voigt.c:24 / :82 rewritten in cm-1)
    int first, last;        // window [first, last] inclusive    spectra.c:48-62; empty if first > last
};

// 128 bytes, read by scalar loads a part at a time: the first 24 bytes by every row of the core
// range that has no selection to make, the next 24 as well by a row that takes the reference's
// chain, y and amp by the inner pass alone, the index ranges lane = line.
//
// A, B, A2: w4 region 1 (voigt.c:91-96) times the amplitude of voigt.c:188 as one quotient in
// D = (v - centre)^2 -- numerator and denominator of (a0 + xq)/(d0 + xq(d2 + xq)), xq = D repwid^2,
// divided by repwid^4, and amp rsqrpi y/repwid^2 = bl:
//   bl (A + D)/(A2 + D (B + D)),  A = g2 + 1/(2 repwid^2),  B = 2 g2 - 1/repwid^2,  A2 = A A.
// B + D never cancels where region 1 is evaluated (y < 8.425: D >= 164/repwid^2; else B > 0) and
// the denominator is at least D^2 or g2^2.
struct alignas(128) LineCore
{
    double A, B, A2;        // region 1 as a quotient (above)
    double repwid;          // sqrt(ln2)/alpha                   voigt.c:13
    double xlim0;           // far-wing limit                    voigt.c:34
    double xlim1;           // w4 region-1 limit                 voigt.c:35-43, :48-53
    double y;               // repwid*gamma                      voigt.c:14
    double amp;             // S/sqrt(pi)*repwid                 voigt.c:188
    int core_first, core_last;  // grid indices that may fall inside |x| < xlim0 (conservative)
    // Grid indices that CERTAINLY lie inside the window and inside |x| < xlim0 (one index and
    // 1e-9 of the reach inside the limit), and the indices that may lie inside |x| < xlim1 (the
    // range of inner_index_range(); empty when the line has no inner regions).  A 64-point row
    // inside the first range and clear of the second is w4 region 1 on every lane
    // (voigt.c:95-96): accumulate.h evaluates it without the per-lane region chain.
    int mid_first, mid_last;
    int hole_first, hole_last;
    int pad[10];
};
static_assert(sizeof(LineCore) == 128, "LineCore is read by scalar loads: 128 bytes");

// An empty index range that intersects no row, tile or grid (including index 0).
constexpr int kEmptyFirst = 0x3fffffff;
constexpr int kEmptyLast = -0x3fffffff;

__host__ __device__ inline void mark_empty(LineWing & w, LineCore & c)
{
    w.centre = 0.; w.g2 = 1.; w.bl = 0.; w.first = kEmptyFirst; w.last = kEmptyLast;
    c.A = 1.; c.B = 0.; c.A2 = 1.;      // with bl = 0: 0 over 1 + D^2
    c.repwid = 1.; c.y = 100.; c.amp = 0.; c.xlim0 = 0.; c.xlim1 = 0.;
    c.core_first = kEmptyFirst; c.core_last = kEmptyLast;
    c.mid_first = kEmptyFirst; c.mid_last = kEmptyLast;
    c.hole_first = kEmptyFirst; c.hole_last = kEmptyLast;
    for (int i = 0; i < 10; ++i) c.pad[i] = 0;
}

// The index ranges of a line's core and inner regions are kept inside [kIndexFloor, kIndexCeiling]:
// up to 2^30, one past the last point of the largest grid the entry takes (2^30 - 1 points), and
// down to -1e9, so that `index - i0` (rows_meeting, accumulate_lines.h) fits an int for every
// first point i0 of a tile.  (The ceiling was 1e9 once: on a grid of more than 1e9 points the
// ranges of the lines beyond that index ended there, and their rows were summed as far wing.)
constexpr double kIndexFloor = -1.e9;
constexpr double kIndexCeiling = 1073741824.;

// Grid indices that may fall inside |x| < xlim1, the inner regions of a line (w4 regions 2-3,
// CPF12; voigt.c:98-186): conservative, with the margins of core_first / core_last above.
__host__ __device__ inline void inner_index_range(double centre, double repwid, double xlim1,
                                                  int v0, int n_per_v, int & first, int & last)
{
    const double near = (xlim1/repwid)*(1. + 1.e-9);
    double lo = floor((centre - near - (double)v0)*n_per_v) - 1.;
    double hi = floor((centre + near - (double)v0)*n_per_v) + 2.;
    if (lo < kIndexFloor) lo = kIndexFloor;
    if (hi > kIndexCeiling) hi = kIndexCeiling;
    if (hi < kIndexFloor) hi = kIndexFloor;
    if (lo > kIndexCeiling) lo = kIndexCeiling;
    first = (int)lo;
    last = (int)hi;
}

// Range of the far-wing terms of one level, as binary exponents (ilogb): what decides how many
// batches of eight lines the far-wing loop may merge before one reciprocal (accumulate_lines.h,
// fast_ranges).  Reduced over the lines by atomicMin from the fill value kWingBoundsFill (the
// maxima are kept negated, so one operation and one fill value serve all four).
enum WingBound
{
    kWingTLow,          // t = d^2 + g2 >= 2^kWingTLow for every far-wing (line, point) pair
    kWingTHighNeg,      // -(e) with t < 2^e
    kWingBLow,          // |bl| >= 2^kWingBLow for every line with bl != 0
    kWingBHighNeg,      // -(e) with |bl| < 2^e
    kWingBounds
};
constexpr int kWingBoundsFill = 0x7f7f7f7f;     // hipMemset byte 0x7f
#ifndef LBL_WING_BATCHES
#define LBL_WING_BATCHES 8      // most batches of eight far-wing lines per reciprocal: 1, 2, 4 or 8
#endif
constexpr int kWingBatchesMax = LBL_WING_BATCHES;

// floor(log2 x) and floor(log2 x) + 1 for x > 0 and finite; anything else is made to look as
// far out of range as an exponent can be (wing_batches() then answers 1).
__host__ __device__ inline int wing_exponent_low(double x)
{
    return (x > 0. && x < 1.e300) ? ilogb(x) : -4096;
}

__host__ __device__ inline int wing_exponent_high(double x)
{
    return (x > 0. && x < 1.e300) ? ilogb(x) + 1 : 4096;
}

// The contribution of one line record to the four bounds (`bound` holds the line's values, to be
// min-reduced).  Lines in a tile's far-wing ranges cover the whole tile (|d| <= cut_off + 1) and
// lie beyond their own far-wing limit, |d| >= xlim0/repwid (schedule_tile: the core range of a
// tile reaches core_reach*nu, core_reach bounds (xlim0/repwid)/nu over the table).  Accepted lines
// there always have a real record; a line the range rule refused carries mark_empty's (centre 0,
// g2 1, bl 0), so t = v^2 + 1 up to the end of the grid when its nu lies where the ranges look
// (schedule_tile: a line that covers a tile has nu in [v0 - cut_off - 1, vn + cut_off)).
__host__ __device__ inline void wing_line_bounds(const GridSpec & g, double nu, int status,
                                                 const LineWing & w, const LineCore & c,
                                                 int (&bound)[kWingBounds])
{
    bound[kWingTLow] = bound[kWingTHighNeg] = kWingBoundsFill;
    bound[kWingBLow] = bound[kWingBHighNeg] = kWingBoundsFill;
    if (status == 1 && w.last >= w.first)
    {
        const double reach = c.xlim0 > 0. ? (c.xlim0/c.repwid)*(1. - 1.e-6) : 0.;
        const double far = (double)g.cut_off + 1.;
        bound[kWingTLow] = wing_exponent_low(reach*reach + w.g2);
        bound[kWingTHighNeg] = -wing_exponent_high(far*far + w.g2);
        const double b = fabs(w.bl);
        if (b != 0.)
        {
            bound[kWingBLow] = wing_exponent_low(b);
            bound[kWingBHighNeg] = -wing_exponent_high(b);
        }
    }
    else if (status == -1 && nu >= (double)(g.v0 - g.cut_off - 1) &&
             nu < (double)(g.vn + g.cut_off))
    {
        const double v = fmax(fabs((double)g.v0), fabs((double)g.vn));
        bound[kWingTHighNeg] = -wing_exponent_high(v*v + 1.);
    }
}

// Batches of eight far-wing lines per reciprocal, from the reduced bounds: the largest
// K in {1, 2, 4, 8} for which the running products of fast_ranges stay normal --
// T = prod of 8K values of t and N = sum b_i prod_{j != i} t_j (at most 8K terms) within
// 2^-1000 .. 2^1000.  K = 1 is the eight-line group that needs no bound (today's range).
// The merge is N = fma(n, T, N t): the product N t is rounded on its own, n T inside the FMA.
// With amplitudes of one sign every term of N has that sign, so |N t| is one part of the new |N|
// and never above it: the upper guard on N covers it.  Downwards N t holds at least one term
// b_i prod t_j over the lines merged so far and the new eight, i.e. it lies above
// 2^(n t_lo + b_lo), which the lower guard keeps at or above 2^-1000: N t is a normal number and
// its rounding a relative 2^-53, like that of n T in the other order.  The table loader refuses no
// sign, and the bounds are those of |bl|.  With amplitudes of both signs the upper guard still
// holds term by term (|N| <= sum |b_i| prod t_j), while N may cancel below any lower bound.  A
// product N t that falls under 2^-1022 then is rounded as a denormal, an absolute error below
// 2^-1074 against terms n T of at least 2^-1000 each: it changes nothing that the cancellation
// itself has not already taken from the sum's relative accuracy.
__host__ __device__ inline int wing_batches(const int (&bound)[kWingBounds])
{
    const long long t_lo = bound[kWingTLow], t_hi = -(long long)bound[kWingTHighNeg];
    long long b_lo = bound[kWingBLow], b_hi = -(long long)bound[kWingBHighNeg];
    if (t_lo == kWingBoundsFill || -t_hi == kWingBoundsFill)
    {
        return 1;           // no far-wing line at this level
    }
    if (b_lo == kWingBoundsFill)
    {
        b_lo = b_hi = 0;    // every bl is 0: N is 0
    }
    if (t_lo < -2000 || t_hi > 2000 || b_lo < -2000 || b_hi > 2000)
    {
        return 1;
    }
    for (int k = kWingBatchesMax; k > 1; k >>= 1)
    {
        const long long n = 8*k;
        // (T >= 2^(n t_lo), N >= 2^((n-1) t_lo + b_lo) with the exponents floored; T < 2^(n t_hi),
        // N < n 2^((n-1) t_hi + b_hi), n <= 2^6.)
        const long long lowest = (t_lo < 0 ? n*t_lo : (n - 1)*t_lo) + (b_lo < 0 ? b_lo : 0);
        const long long highest = (t_hi > 0 ? n*t_hi : (n - 1)*t_hi) + (b_hi > 0 ? b_hi : 0) + 6;
        if (lowest >= -1000 && highest <= 1000 && n*t_lo >= -1000 && n*t_hi <= 1000)
        {
            return k;
        }
    }
    return 1;
}

// The eights of a level (lines base + 8 g .. base + 8 g + 7 of the sorted table, base the first line
// the call's range rule can accept: what lies below a call's windows moves no group) as the far-wing
// loop of accumulate_kernel<4> takes them where a tile is eligible (accumulate_lines.h,
// scaled_ranges): the eight amplitudes folded into the denominators, so that the eight fractions
// sum as a chain of unit numerators.
//   m     = rint(centre of the first line): v - m and centre - m are exact (Sterbenz) for tiles
//           at or above max(64, 2 (cut_off + 2)) cm-1 and lines within kWingGroupReach of m;
//   beta  = geometric mean of the eight bl (wing_group_beta);
//   s     = sqrt(beta/bl), nas = -((centre - m) s), gs = g2 (s s) per line, so that
//           t' = fma(d', d', gs), d' = fma(v - m, s, nas), is t beta/bl up to rounding and
//           sum bl/t = beta sum 1/t'.
// A group is PLAIN (beta = 0, m = 0 and s = nas = 0, gs = 1 on every line, so that the chain
// gives t' = 1 and the group adds 0/1 to the loop's running sums; the loop then sums it from its
// LineWing records, as before) when it has fewer than eight lines of the table, when any bl is not a
// positive normal number (mark_empty's records, amplitudes of the other sign), when any centre is
// farther than kWingGroupReach from m, when the binary exponents of its amplitudes span more than
// kWingGroupSpread (the partial products of the chain then leave the range its whole product
// keeps: they differ from the products of t by at most 2^(2 spread)), or when any field comes out
// not finite (s and gs: not normal).  The rule reads the line scalars alone: host and device make
// the same records, bit for bit (divisions, square roots, frexp and ldexp are exact or correctly
// rounded on both).
struct WingScaled
{
    double s, nas, gs;
};

struct alignas(16) WingGroup
{
    double s[8];
    double gs[8];
    double nas[8];
    double beta;            // 0: a plain group
    double m;
};
static_assert(sizeof(WingGroup) == 208, "WingGroup is read by wide loads: 26 doubles");

__host__ __device__ inline void wing_group_set(WingGroup & g, int i, const WingScaled & l)
{
    g.s[i] = l.s;
    g.nas[i] = l.nas;
    g.gs[i] = l.gs;
}

// A line of a plain group: d' = 0 v + 0 and t' = 0 + 1 at every point.
constexpr WingScaled kWingPlainLine = {0., 0., 1.};
constexpr double kWingGroupReach = 1.5;
constexpr int kWingGroupSpread = 128;

__host__ __device__ inline bool wing_is_normal(double x)
{
    const double a = fabs(x);
    return a >= 2.2250738585072014e-308 && a <= 1.7976931348623157e308;
}

// The geometric mean of eight positive normal numbers: mantissas multiplied in index order (a
// product in [2^-8, 1)), exponents added, the sum split into 8 q + r, three square roots of the
// mantissa product times 2^r and a last ldexp by q.  Within a few 2^-53 of the exact root.
__host__ __device__ inline double wing_group_beta(const double (&bl)[8])
{
    double mantissa = 1.;
    int exponent = 0;
    for (int i = 0; i < 8; ++i)
    {
        int e;
        mantissa *= frexp(bl[i], &e);
        exponent += e;
    }
    const int q = exponent >> 3, r = exponent & 7;      // floor and remainder, also below zero
    return ldexp(sqrt(sqrt(sqrt(ldexp(mantissa, r)))), q);
}

// What the eight amplitudes and the first centre decide: false = plain.
__host__ __device__ inline bool wing_group_header(double first_centre, const double (&bl)[8],
                                                  int lines, double & beta, double & m)
{
    beta = 0.;
    m = 0.;
    if (lines < 8 || !(fabs(first_centre) < 4.e15))
    {
        return false;
    }
    int low = 4096, high = -4096;
    for (int i = 0; i < 8; ++i)
    {
        if (!(bl[i] > 0.) || !wing_is_normal(bl[i]))
        {
            return false;
        }
        const int e = ilogb(bl[i]);
        low = e < low ? e : low;
        high = e > high ? e : high;
    }
    if (high - low > kWingGroupSpread)
    {
        return false;
    }
    beta = wing_group_beta(bl);
    m = rint(first_centre);
    return wing_is_normal(beta);
}

// One line of a group whose header passed: false = the group is plain after all.
__host__ __device__ inline bool wing_group_line(double centre, double g2, double bl, double beta,
                                                double m, WingScaled & out)
{
    const double a = centre - m;
    const double s = sqrt(beta/bl);
    out.s = s;
    out.nas = -(a*s);
    out.gs = g2*(s*s);
    return fabs(a) <= kWingGroupReach && wing_is_normal(s) && wing_is_normal(out.gs) &&
           fabs(out.nas) <= 1.7976931348623157e308;
}

// The record of one group from its eight line records (`lines` of them belong to the table).
__host__ __device__ inline void wing_group_of(const double (&centre)[8], const double (&g2)[8],
                                              const double (&bl)[8], int lines, WingGroup & out)
{
    double beta, m;
    bool scaled = wing_group_header(centre[0], bl, lines, beta, m);
    for (int i = 0; i < 8; ++i)
    {
        WingScaled l;
        scaled = wing_group_line(centre[i], g2[i], bl[i], beta, m, l) && scaled;
        wing_group_set(out, i, l);
    }
    out.beta = beta;
    out.m = m;
    if (!scaled)
    {
        for (int i = 0; i < 8; ++i) wing_group_set(out, i, kWingPlainLine);
        out.beta = 0.;
        out.m = 0.;
    }
}

// status: 1 evaluated, 0 window right of the grid / empty, -1 not accepted by the range rule.
// derived (optional, 8 doubles): centre, alpha, gamma, strength, first, last, status, 0.
__host__ __device__ inline int prepare_line(const LevelScalars & lv, const GridSpec & g,
                                            double nu, double sw, double gamma_air,
                                            double gamma_self, double n_air, double elower,
                                            double delta_air, int iso_slot, bool accepted,
                                            LineWing & w, LineCore & c, double * derived)
{
    const double vlight = 2.99792458e8;
    const double c2 = 1.4387752;
    const double rsqrpi = 1./sqrt(kPi);
    const double sqrln2 = sqrt(log(2.));
    mark_empty(w, c);
    if (derived != nullptr)
    {
        for (int i = 0; i < 8; ++i) derived[i] = 0.;
        derived[6] = -1.;
    }
    if (!accepted)
    {
        return -1;
    }
    // spectra.c:22-45
    const double centre = nu + lv.p_atm*delta_air;
    const double gamma = (gamma_air*(lv.p_atm - lv.p_partial) + gamma_self*lv.p_partial)*
                         pow(lv.tfact, n_air);
    const double alpha = (nu/vlight)*lv.doppler[iso_slot];
    const double sb = exp(elower*c2*lv.t_minus_ref/lv.t_times_ref);
    const double gg = exp((-c2*nu)/lv.temperature);
    const double gref = exp((-c2*nu)/296.);
    const double se = (1. - gg)/(1. - gref);
    const double strength = sw*sb*se*lv.q_ratio[iso_slot]*0.01*0.01;

    // spectra.c:48-62 (v[0] == v0 exactly: absorption.c:39 with i = 0)
    const double fl = floor(centre);
    int first = (int)((fl - g.cut_off - (double)g.v0)*g.n_per_v);
    int last = 0;
    int status = 1;
    if (first >= g.n)
    {
        status = 0;
    }
    else
    {
        if (first < 0) first = 0;
        last = (int)((fl + g.cut_off + 1 - (double)g.v0)*g.n_per_v);
        if (last >= g.n) last = g.n - 1;
    }
    if (derived != nullptr)
    {
        derived[0] = centre; derived[1] = alpha; derived[2] = gamma; derived[3] = strength;
        derived[4] = first; derived[5] = last; derived[6] = status;
    }
    if (status == 0 || last < first)
    {
        // Nothing to add (a window wholly left of the grid gives last < 0).
        return status;
    }
    // voigt.c:13-15
    const double repwid = sqrln2/alpha;
    const double y = repwid*gamma;
    w.centre = centre;
    w.g2 = gamma*gamma;
    w.bl = strength*gamma/kPi;
    w.first = first;
    w.last = last;
    c.repwid = repwid;
    c.y = y;
    c.amp = strength*rsqrpi*repwid;
    const double inverse_r2 = 1./(repwid*repwid);
    c.A = w.g2 + 0.5*inverse_r2;
    c.B = (w.g2 + w.g2) - inverse_r2;
    c.A2 = c.A*c.A;
    if (y < 70.55)
    {
        // voigt.c:34: beyond xlim0 Doppler half-widths the profile is the Lorentz wing.
        const double xlim0 = sqrt(15100. + y*(40. - y*3.6));
        double xlim1 = (y >= 8.425) ? 0. : sqrt(164. - y*(4.3 + y*1.8));
        if (y <= 0.000001) xlim1 = xlim0;               // voigt.c:48-53
        c.xlim0 = xlim0;
        c.xlim1 = xlim1;
        const double reach = (xlim0/repwid)*(1. + 1.e-9);
        double lo = floor((centre - reach - (double)g.v0)*g.n_per_v) - 1.;
        double hi = floor((centre + reach - (double)g.v0)*g.n_per_v) + 2.;
        if (lo < kIndexFloor) lo = kIndexFloor;
        if (hi > kIndexCeiling) hi = kIndexCeiling;
        if (hi < kIndexFloor) hi = kIndexFloor;
        if (lo > kIndexCeiling) lo = kIndexCeiling;
        c.core_first = (int)lo;
        c.core_last = (int)hi;
        const double sure = (xlim0/repwid)*(1. - 1.e-9);
        double mid_lo = ceil((centre - sure - (double)g.v0)*g.n_per_v) + 1.;
        double mid_hi = floor((centre + sure - (double)g.v0)*g.n_per_v) - 1.;
        if (mid_lo < (double)first) mid_lo = (double)first;
        if (mid_hi > (double)last) mid_hi = (double)last;
        if (mid_hi >= mid_lo)
        {
            c.mid_first = (int)mid_lo;
            c.mid_last = (int)mid_hi;
        }
        if (xlim1 > 0.)
        {
            inner_index_range(centre, repwid, xlim1, g.v0, g.n_per_v, c.hole_first, c.hole_last);
        }
    }
    return status;
}

}  // namespace lbl
