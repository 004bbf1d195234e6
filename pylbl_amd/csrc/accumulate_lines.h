// The hot kernel's line loops: what a wavefront does with each of the cut-point ranges of its
// tile (accumulate.h states the ranges) -- fast_ranges (far wing, eight lines per reciprocal),
// scaled_ranges (the table-aligned eights of the far wing as chains of unit numerators, <4>),
// clipped_ranges / general_line (windows that end inside the tile), core_lines / core_pair (tiles
// that may hold a line's core: voigt.c:74-189 row by row, two lines per reciprocal) and inner_ranges / inner_batch (the
// points nearer than xlim1, packed by class through LDS).  Included by accumulate.h after its
// argument structs.
#pragma once

namespace lbl {

// Far-wing loop over two index ranges [a0,a1) and [b0,b1) whose lines all cover the whole
// tile with the tile in their Lorentz wing.  Eight (or four) lines share one reciprocal;
// only whole groups of four are taken here, the caller sends the 0-3 left-over lines of each
// range down the general path.  The records arrive by scalar loads whose latency is covered
// by the other resident wavefronts of the SIMD.
//
// P = 4 (the form that carries the default workload; its SIMDs are full of fp64 FMA-class work
// here, so only fewer operations per evaluation make it faster): every batch of eight lines
// becomes one fraction n/t per row (wing_eight), merged into a running N/T -- N = n T + (N t),
// T = T t, three operations -- and `batches` of them (wave-uniform, per level: wing_batches(),
// which keeps the products in range) share one reciprocal and one FMA into acc.  At most 8 line
// records are held at a time, as before; the running sums take 2 P VGPRs.  The order of the
// operations is fixed: results are bitwise the same from run to run.  batches = 1 is the plain
// eight-line group.
// The product rounded on its own is N t, the one that lives in N's register: the FMA accumulates
// into it and N never leaves its place.  Written the other way round (N t + (n T)) the compiler
// formed n T in a fresh register, accumulated there and copied N back once per row and batch --
// four v_mov_b64 in the loop block of a trip, 2.2e7 per launch of the default workload
// (profiles/wing_trip_ab.txt).  A trip now compiles to its arithmetic alone: 148 fp64
// operations in the first batch, 160 in every later one, 12 and the four reciprocals at the end.
template <int P>
__device__ __forceinline__ void fast_ranges(const LineWing * __restrict__ wing,
                                            int a0, int a1, int b0, int b1, int batches,
                                            const double (&v)[P], double (&acc)[P])
{
    const int qa = (a1 - a0) >> 2;
    const int quads = qa + ((b1 - b0) >> 2);
    int q = 0;
#if LBL_WING_GROUP == 8
    auto eight = [&](int at, WingTerm (&l)[8]) {
        const int ja = at < qa ? a0 + 4*at : b0 + 4*(at - qa);
        const int jb = (at + 1) < qa ? a0 + 4*(at + 1) : b0 + 4*(at + 1 - qa);
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            const LineWing wa = wing[ja + i], wb = wing[jb + i];
            l[i] = WingTerm{wa.centre, wa.g2, wa.bl};
            l[4 + i] = WingTerm{wb.centre, wb.g2, wb.bl};
        }
    };
    if (P == 4 && batches > 1)
    {
        const int eights = quads >> 1;
        for (int o = 0; o < eights; )
        {
            const int stop = min(o + batches, eights);
            double num[P], den[P];
            {
                WingTerm l[8];
                eight(2*o, l);
#pragma unroll
                for (int p = 0; p < P; ++p)
                {
                    wing_eight(v[p], l, num[p], den[p]);
                }
            }
            for (++o; o < stop; ++o)
            {
                WingTerm l[8];
                eight(2*o, l);
#pragma unroll
                for (int p = 0; p < P; ++p)
                {
                    double n, t;
                    wing_eight(v[p], l, n, t);
                    num[p] = __builtin_fma(n, den[p], num[p]*t);
                    den[p] = den[p]*t;
                }
            }
#pragma unroll
            for (int p = 0; p < P; ++p)
            {
                acc[p] = __builtin_fma(num[p], rcp_newton(den[p]), acc[p]);
            }
        }
        q = 2*eights;
    }
    // Two groups of four per step: eight lines share one reciprocal.
    for (; q + 2 <= quads; q += 2)
    {
        WingTerm l[8];
        eight(q, l);
#pragma unroll
        for (int p = 0; p < P; ++p)
        {
            acc[p] = lorentz_eight(v[p], l, acc[p]);
        }
    }
#endif
    for (; q < quads; ++q)
    {
        const int j = q < qa ? a0 + 4*q : b0 + 4*(q - qa);
        const LineWing l1 = wing[j], l2 = wing[j + 1], l3 = wing[j + 2], l4 = wing[j + 3];
#pragma unroll
        for (int p = 0; p < P; ++p)
        {
            acc[p] = lorentz_four(v[p], l1.centre, l1.g2, l1.bl, l2.centre, l2.g2, l2.bl,
                                  l3.centre, l3.g2, l3.bl, l4.centre, l4.g2, l4.bl, acc[p]);
        }
    }
}

// The far-wing loop of accumulate_kernel<4> over a wavefront's table-aligned eights, [a0,a1) and
// [b0,b1) (line indices, `group_base` plus multiples of 8), on tiles that begin at or above max(64, 2 (cut_off + 2))
// cm-1.  A group is summed from its scaled record (line_prep.h, WingGroup) as a chain of unit
// numerators on pre-scaled offsets (scaled_eight): per row u = v - m, which is exact, the chain,
// n = beta N -- 32 operations where wing_eight has 37 -- and the fraction n/t joins the running
// N/T as in fast_ranges: N = fma(n, T, N t), T = T t, `batches` groups per reciprocal.  t is the
// product of the eight t_i up to rounding (beta is the geometric mean of the amplitudes), so the
// running products have the magnitudes wing_batches() bounds.  The record arrives by scalar
// loads, 26 doubles per group where the eight LineWing records are 32.  A vector instruction of
// gfx950 reads one scalar operand, so d' = fma(u, s, nas) takes nas from a vector register: one
// v_mov_b64 per line and batch, shared by the four rows -- 148 vector instructions per batch
// where fast_ranges has 160.  (Fetched by vector loads of one address instead, the same value on
// every lane, the copies go and the step is slower: profiles/wing_scaled_ab.txt.)
// A plain group (beta = 0: an amplitude that is not positive, a centre beyond 1.5 cm-1 of m, ...)
// passes through that loop without a branch and without a trace: its record gives t' = 1 on every
// line, so n = 0 N = 0 and t = 1 -- N = fma(0, T, N 1), T = T 1.  (With a branch the loop had two
// bodies that left the running sums in different registers, and eight v_mov_b64 at their join.)
// Its lines are added afterwards from their LineWing records, eight per reciprocal
// (lorentz_eight).  An eight never spans the two ranges; a trip may.  The order of the operations
// is fixed.
template <bool First>
__device__ __forceinline__ void scaled_batch(const WingGroup * __restrict__ g,
                                             const double (&v)[4], double (&num)[4],
                                             double (&den)[4])
{
    const double beta = g->beta, m = g->m;
    double s[8], gs[8], nas[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
    {
        nas[i] = g->nas[i];
        s[i] = g->s[i];
        gs[i] = g->gs[i];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
    {
        double n, t;
        scaled_eight(v[p] - m, s, nas, gs, n, t);
        n = beta*n;
        if (First)
        {
            num[p] = n;
            den[p] = t;
        }
        else
        {
            num[p] = __builtin_fma(n, den[p], num[p]*t);
            den[p] = den[p]*t;
        }
    }
}

__device__ __forceinline__ void scaled_ranges(const LineWing * __restrict__ wing,
                                              const WingGroup * __restrict__ groups, int group_base,
                                              int a0, int a1, int b0, int b1, int batches,
                                              int lane, const double (&v)[4], double (&acc)[4])
{
    // (the cuts come out of share_of's float arithmetic: said to be wave-uniform here, the loop
    // counts and the record addresses stay in scalar registers)
    a0 = __builtin_amdgcn_readfirstlane(a0);
    b0 = __builtin_amdgcn_readfirstlane(b0);
    const int ea = __builtin_amdgcn_readfirstlane((a1 - a0) >> 3);
    const int eights = ea + __builtin_amdgcn_readfirstlane((b1 - b0) >> 3);
    auto line_of = [&](int at) { return at < ea ? a0 + 8*at : b0 + 8*(at - ea); };
    auto group_of = [&](int at) { return groups + ((line_of(at) - group_base) >> 3); };
    for (int o = 0; o < eights; )
    {
        const int stop = min(o + batches, eights);
        double num[4], den[4];
        scaled_batch<true>(group_of(o), v, num, den);
        for (++o; o < stop; ++o)
        {
            scaled_batch<false>(group_of(o), v, num, den);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
        {
            acc[p] = __builtin_fma(num[p], rcp_newton(den[p]), acc[p]);
        }
    }
    // The plain groups, 64 at a time: lane = group looks at beta, the wavefront walks the bits.
    for (int base = 0; base < eights; base += 64)
    {
        const int at = min(base + lane, eights - 1);
        const bool plain = base + lane < eights && !(group_of(at)->beta != 0.);
        unsigned long long left = __ballot(plain);
        while (left != 0)
        {
            const int j = line_of(base + __builtin_ctzll(left));
            WingTerm l[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
            {
                const LineWing w = wing[j + i];
                l[i] = WingTerm{w.centre, w.g2, w.bl};
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
            {
                acc[p] = lorentz_eight(v[p], l, acc[p]);
            }
            left &= left - 1;
        }
    }
}

// One line that may clip the tile or have its core in it, row by row (64 points each).
// Per row the decisions are wave-uniform: skip (outside the window), Lorentz (whole row in
// the far wing), or core.  In a core row every lane applies the reference's chain on
// xi = (v-nu')*repwid (voigt.c:76-84): region 0 and w4 region 1 (voigt.c:95-96) are
// evaluated inline.  Lanes closer to the centre than xlim1 add nothing here: the inner points of
// all the lines walked here are summed afterwards, in a pass of their own (inner_ranges), into
// the wavefront's LDS sums.
// Which of a tile's rows (row p = grid indices [i0 + 64 p, i0 + 64 p + 63], p < rows <= 8) meet
// the index range [a, b], and which lie wholly inside it: one bit per row.  The row-by-row
// decisions below are wave-uniform and were, written as comparisons per row, ~19 scalar
// instructions per row and line -- the scalar unit, one per CU, was the busiest unit of the kernel
// wherever the general path carries the work (the far-field option: 183 M scalar against 139 M
// vector instructions per launch).  As masks they cost ~10 scalar instructions per range and line
// and a bit test per row.
__device__ __forceinline__ unsigned row_bits(int lo, int hi, int rows)
{
    lo = max(lo, 0);
    hi = min(hi, rows - 1);
    return lo > hi ? 0u : ((2u << hi) - 1u) & ~((1u << lo) - 1u);
}

__device__ __forceinline__ unsigned rows_meeting(int a, int b, int i0, int rows)
{
    return b < a ? 0u : row_bits((a - i0) >> 6, (b - i0) >> 6, rows);
}

__device__ __forceinline__ unsigned rows_inside(int a, int b, int i0, int rows)
{
    return b < a ? 0u : row_bits((a - i0 + 63) >> 6, (b - 63 - i0) >> 6, rows);
}

// One row of one line as a quotient N/T in D = (v - centre)^2, for rows on which no lane has a
// selection to make (line_prep.h, LineCore): the far wing bl/(D + g2), or w4 region 1
// (voigt.c:95-96 times the amplitude of voigt.c:188) bl (A + D)/(A2 + D (B + D)).  `d` = v - centre.
struct RegionOne
{
    double A, B, A2;        // LineCore's, fetched once per line
};

__device__ __forceinline__ RegionOne region_one_of(const LineCore * __restrict__ c)
{
    return RegionOne{c->A, c->B, c->A2};
}

__device__ __forceinline__ void far_quotient(const LineWing & l, double d, double & num,
                                             double & den)
{
    num = l.bl;
    den = __builtin_fma(d, d, l.g2);
}

__device__ __forceinline__ void region_one_quotient(const LineWing & l, const RegionOne & q,
                                                    double d, double & num, double & den)
{
    const double D = d*d;
    const double n = q.A + D;
    const double u = q.B + D;
    den = __builtin_fma(D, u, q.A2);
    num = l.bl*n;
}

// Bit 0 of `kind`: region 1, else the far wing (rows that take the chain do not come here).
__device__ __forceinline__ void row_quotient(const LineWing & l, const RegionOne & q,
                                             unsigned kind, double d, double & num, double & den)
{
    if (kind & 1u)
    {
        region_one_quotient(l, q, d, num, den);
    }
    else
    {
        far_quotient(l, d, num, den);
    }
}

// A row that may hold a point of the line's core: the reference's chain on xi = (v-nu')*repwid
// (voigt.c:76-84), comparison for comparison; region 0 and w4 region 1 are evaluated here, lanes
// nearer than xlim1 add nothing (inner_ranges).  repwid and the limits are fetched only here.
__device__ __forceinline__ double chain_row(const LineWing & l,
                                            const LineCore * __restrict__ c, double d)
{
    const double xi = d*c->repwid;                  // voigt.c:76
    const double abx = fabs(xi);
    const bool far = abx >= c->xlim0;
    const bool mid = !far && abx >= c->xlim1;
    double value = 0.;
    if (__any(far))
    {
        // voigt.c:82 / :24 in wavenumber units.
        const double wing = l.bl*rcp_newton(__builtin_fma(d, d, l.g2));
        value = far ? wing : value;
    }
    if (__any(mid))
    {
        double num, den;
        region_one_quotient(l, region_one_of(c), d, num, den);
        const double w4 = num*rcp_newton(den);
        value = mid ? w4 : value;
    }
    return value;
}

template <int P>
__device__ __forceinline__ void general_line(const LineWing & l,
                                             const LineCore * __restrict__ c,
                                             int i0, int i1, int lane,
                                             const double (&v)[P], double (&acc)[P])
{
    const unsigned in_window = rows_meeting(l.first, l.last, i0, P);
    if (in_window == 0)
    {
        return;     // also skips empty windows
    }
    // Rows wholly inside the window and in w4 region 1 on every lane (line_prep.h), and rows
    // that may hold a point of the core.
    const unsigned all_region_one = rows_inside(c->mid_first, c->mid_last, i0, P) &
                                    ~rows_meeting(c->hole_first, c->hole_last, i0, P);
    const unsigned near_core = rows_meeting(c->core_first, c->core_last, i0, P);
#pragma unroll
    for (int p = 0; p < P; ++p)
    {
        if (!(in_window & (1u << p)))
        {
            continue;
        }
        const int r0 = i0 + p*64;
        const double d = v[p] - l.centre;
        if (all_region_one & (1u << p))
        {
            // voigt.c:95-96 with no selection left to make.
            double num, den;
            region_one_quotient(l, region_one_of(c), d, num, den);
            acc[p] = __builtin_fma(num, rcp_newton(den), acc[p]);
            continue;
        }
        const int i = r0 + lane;
        const bool inside = (i >= l.first) && (i <= l.last);
        double value;
        if (!(near_core & (1u << p)))
        {
            // voigt.c:82 / :24 in wavenumber units: the whole row is in the far wing.
            value = l.bl*rcp_newton(__builtin_fma(d, d, l.g2));
        }
        else
        {
            value = chain_row(l, c, d);
        }
        acc[p] += inside ? value : 0.;
    }
}

// Up to five index ranges of lines in general position, walked as one list.
struct GeneralList
{
    int begin[5];
    int count[5];
};

__device__ __forceinline__ int general_index(const GeneralList & g, int k)
{
    if (k < g.count[0]) return g.begin[0] + k;
    k -= g.count[0];
    if (k < g.count[1]) return g.begin[1] + k;
    k -= g.count[1];
    if (k < g.count[2]) return g.begin[2] + k;
    k -= g.count[2];
    if (k < g.count[3]) return g.begin[3] + k;
    k -= g.count[3];
    return g.begin[4] + k;
}

// The inner points (|x| < xlim1: w4 regions 2-3, CPF12) of a batch of lines, packed twice.
// Row by row they would leave most of a wavefront idle in the most expensive branches of the
// profile: a line's inner points are a few dozen consecutive grid points (27 for a CO2 line at
// 1000 cm-1 and 0.001 cm-1 spacing, a few hundred at 5000 cm-1 and 0.0005 cm-1), and within them
// the three classes of voigt_profile.h -- costing roughly 35, 120 and 190 instruction slots per
// point -- each hold a part of the lanes while the wavefront pays for all three.
//   step 1, lane = line:  fetch the line's scalars, clip its inner index range to tile and
//                         window, inclusive scan of the segment lengths (the segments of all
//                         queued lines laid end to end);
//   step 2, lane = point: for every 64 positions of that sequence, find the line and grid point
//                         of each lane, form x, classify with the reference's comparisons, and
//                         append (line, point) to the class's list (ballot + prefix count);
//   step 3, lane = entry of ONE class list, whenever a list holds 64 entries (and at the end):
//                         evaluate that class's formula, and add to `slab` (LDS sums of the
//                         wavefront, index = point - tile_first) one line at a time: two lines of
//                         a list may cover the same grid point, and the order of additions is
//                         fixed -- results do not depend on scheduling.
constexpr int kInnerQueue = 32;         // lines per batch (lane = line in step 1)
constexpr int kInnerList = 128;         // entries a class list can hold (64 left + 64 new)

struct InnerStage
{
    int first[kInnerQueue];             // first inner point in tile and window
    int begin[kInnerQueue], end[kInnerQueue];   // the line's segment in the packed sequence
    double centre[kInnerQueue], repwid[kInnerQueue], y[kInnerQueue], amp[kInnerQueue];
    double xlim1[kInnerQueue];
    unsigned short list[kInnerClasses][kInnerList];     // (queue slot << 9) | (point - tile_first)
};

template <int C>
__device__ __forceinline__ void inner_evaluate(InnerStage & stage, int count, int i0, int v0,
                                               double dv, int lane, double * slab)
{
    const bool active = lane < count;
    const unsigned record = stage.list[C][active ? lane : 0];
    const int q = record >> 9;
    const int offset = record & 511;
    // absorption.c:39: v[i] = v0 + i*dv (product rounded, then the sum); voigt.c:76-78.
    const double v = (double)v0 + (double)(i0 + offset)*dv;
    const double xi = (v - stage.centre[q])*stage.repwid[q];
    double value = 0.;
    if (active)
    {
        const double y = stage.y[q];
        const double k = C == 0 ? inner_class_a(xi, y)
                       : (C == 1 ? inner_class_b(xi, y) : inner_class_c(xi, y));
        value = stage.amp[q]*k;
    }
    unsigned long long left = __ballot(active);
    while (left != 0)
    {
        const int q0 = __builtin_amdgcn_readlane(q, __builtin_ctzll(left));
        const bool now = active && q == q0;
        if (now)
        {
            slab[offset] += value;
        }
        left &= ~__ballot(now);
    }
}

// `j` is this lane's line of the batch (lanes >= kInnerQueue and lanes beyond the batch: has =
// false).  Returns without touching LDS when no line of the batch has an inner point in the tile:
// the common case at tropospheric pressure, where y >= 8.425 switches the inner regions off for
// most lines, and for the lines of a batch whose cores lie in other tiles.
__device__ __forceinline__ bool inner_batch(const LineWing * __restrict__ wing,
                                            const LineCore * __restrict__ core,
                                            InnerStage & stage, int j, bool has, int i0, int i1,
                                            int v0, int n_per_v, double dv, int lane,
                                            double * slab, bool slab_in_use, int slab_rows)
{
    // Step 1.
    unsigned long long todo;
    int total;
    {
        // Two fields decide for most lines (xlim1 == 0: no inner regions at all; core range
        // elsewhere): the rest of the record is fetched only if some line of the batch passes.
        const double xlim1 = core[j].xlim1;
        const bool candidate = has && xlim1 > 0. && core[j].core_last >= i0 &&
                               core[j].core_first <= i1;
        if (__ballot(candidate) == 0)
        {
            return false;
        }
        const LineWing l = wing[j];
        const LineCore c = core[j];
        int first = 0, last = -1;
        if (candidate)
        {
            inner_index_range(l.centre, c.repwid, c.xlim1, v0, n_per_v, first, last);
            first = max(max(first, l.first), i0);
            last = min(min(last, l.last), i1);
        }
        const int length = last >= first ? last - first + 1 : 0;
        todo = __ballot(length > 0);
        if (todo == 0)
        {
            return false;
        }
        if (!slab_in_use)
        {
            // The wavefront's LDS sums are cleared by the first batch that has something to add
            // (most tiles at tropospheric pressure never get here).
            for (int p = 0; p < slab_rows; ++p) slab[p*64 + lane] = 0.;
        }
        int inclusive = length;
#pragma unroll
        for (int offset = 1; offset < kInnerQueue; offset <<= 1)
        {
            const int below = __shfl_up(inclusive, offset, 64);
            inclusive += (lane >= offset) ? below : 0;
        }
        if (lane < kInnerQueue)
        {
            stage.first[lane] = first;
            stage.begin[lane] = inclusive - length;
            stage.end[lane] = inclusive;
            stage.centre[lane] = l.centre;
            stage.repwid[lane] = c.repwid;
            stage.y[lane] = c.y;
            stage.amp[lane] = c.amp;
            stage.xlim1[lane] = c.xlim1;
        }
        total = __builtin_amdgcn_readlane(inclusive, kInnerQueue - 1);
    }

    int count[kInnerClasses] = {0, 0, 0};
    for (int base = 0; ; base += 64)
    {
        const bool drain = base >= total;
        if (!drain)
        {
            // Step 2.
            const int u = base + lane;
            double m_centre = 0., m_repwid = 1., m_y = 100., m_xlim1 = 0.;
            int m_point = i0, m_line = -1;
            unsigned long long scan = todo;
            while (scan != 0)
            {
                const int q = __builtin_ctzll(scan);
                const int begin = __builtin_amdgcn_readfirstlane(stage.begin[q]);
                if (begin >= base + 64)
                {
                    break;
                }
                const int end = __builtin_amdgcn_readfirstlane(stage.end[q]);
                const bool mine = u >= begin && u < end;
                m_centre = mine ? stage.centre[q] : m_centre;
                m_repwid = mine ? stage.repwid[q] : m_repwid;
                m_y = mine ? stage.y[q] : m_y;
                m_xlim1 = mine ? stage.xlim1[q] : m_xlim1;
                m_point = mine ? stage.first[q] + (u - begin) : m_point;
                m_line = mine ? q : m_line;
                if (end <= base + 64)
                {
                    todo &= ~(1ull << q);       // this line's segment ends here
                }
                scan &= scan - 1;
            }
            const double v = (double)v0 + (double)m_point*dv;
            const double abx = fabs((v - m_centre)*m_repwid);
            const bool take = m_line >= 0 && abx < m_xlim1;
            const int cls = inner_class(abx, inner_limits(m_y));
            const unsigned short record = (unsigned short)((m_line << 9) | (m_point - i0));
#pragma unroll
            for (int c = 0; c < kInnerClasses; ++c)
            {
                const bool member = take && cls == c;
                const unsigned long long mask = __ballot(member);
                if (member)
                {
                    const int rank = __builtin_amdgcn_mbcnt_hi(
                        (unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                    stage.list[c][count[c] + rank] = record;
                }
                count[c] += __builtin_popcountll(mask);
            }
        }
        // Step 3.
#pragma unroll
        for (int c = 0; c < kInnerClasses; ++c)
        {
            if (count[c] >= 64 || (drain && count[c] > 0))
            {
                const int now = min(count[c], 64);
                if (c == 0) inner_evaluate<0>(stage, now, i0, v0, dv, lane, slab);
                if (c == 1) inner_evaluate<1>(stage, now, i0, v0, dv, lane, slab);
                if (c == 2) inner_evaluate<2>(stage, now, i0, v0, dv, lane, slab);
                count[c] -= now;
                // What is left (fewer than 64 entries) moves to the front of the list.
                const unsigned short rest = stage.list[c][64 + lane];
                if (lane < count[c])
                {
                    stage.list[c][lane] = rest;
                }
            }
        }
        if (drain)
        {
            break;
        }
    }
    return true;
}

// Two lines of the core range [c1, c2): their windows cover the whole tile (the range lies inside
// [a1, a2)), so what is left to decide per row and line is `rows`, prepared by core_lines():
//   bit p       row p lies wholly in w4 region 1 (and inside the window): no selection at all;
//   bit 8 + p   row p may hold a point of the core and is not of the first kind: the reference's
//               chain lane by lane;
//   neither     the whole row is in the far wing.
// A row of the first or the last kind is a quotient N/T in (v - centre)^2 (far_quotient,
// region_one_quotient).  Where both lines have one, the two are merged -- N = Na Tb + Nb Ta,
// T = Ta Tb, the far-wing loop's three operations -- and share one reciprocal and one FMA into
// acc, whatever the kinds.  Where a line takes the chain on a row, each line goes alone there
// (single_row): the chain for the one, its own reciprocal for the other.  The order of the
// operations is fixed: results are bitwise the same from run to run.
__device__ __forceinline__ double single_row(const LineWing & l, const RegionOne & q,
                                             const LineCore * __restrict__ c, unsigned kind,
                                             double d, double sum)
{
    if (kind & 0x100u)
    {
        return sum + chain_row(l, c, d);
    }
    double num, den;
    row_quotient(l, q, kind, d, num, den);
    return __builtin_fma(num, rcp_newton(den), sum);
}

template <int P>
__device__ __forceinline__ void core_pair(const LineWing & la, const LineWing & lb,
                                          const LineCore * __restrict__ pair,
                                          unsigned rows_a, unsigned rows_b,
                                          const double (&v)[P], double (&acc)[P])
{
    const RegionOne qa = region_one_of(pair), qb = region_one_of(pair + 1);
#pragma unroll
    for (int p = 0; p < P; ++p)
    {
        const double da = v[p] - la.centre, db = v[p] - lb.centre;
        if (__builtin_expect(((rows_a | rows_b) & (0x100u << p)) == 0, 1))
        {
            double na, ta, nb, tb;
            row_quotient(la, qa, rows_a >> p, da, na, ta);
            row_quotient(lb, qb, rows_b >> p, db, nb, tb);
            acc[p] = __builtin_fma(__builtin_fma(na, tb, nb*ta), rcp_newton(ta*tb), acc[p]);
        }
        else
        {
            acc[p] = single_row(la, qa, pair, rows_a >> p, da, acc[p]);
            acc[p] = single_row(lb, qb, pair + 1, rows_b >> p, db, acc[p]);
        }
    }
}

// The core range, two lines at a time.  The row masks of 64 lines are formed at once, lane =
// line, by vector integer arithmetic (half an instruction per line where the scalar unit spent
// ~35), and handed to the walk through v_readlane.
template <int P>
__device__ __forceinline__ void core_lines(const LineWing * __restrict__ wing,
                                           const LineCore * __restrict__ core,
                                           int begin, int count, int i0, int lane,
                                           const double (&v)[P], double (&acc)[P])
{
    for (int base = 0; base < count; base += 64)
    {
        const int n = min(64, count - base);        // even: the caller keeps an odd line back
        const LineCore * __restrict__ mine = core + begin + base + min(lane, n - 1);
        const unsigned all_region_one = rows_inside(mine->mid_first, mine->mid_last, i0, P) &
                                        ~rows_meeting(mine->hole_first, mine->hole_last, i0, P);
        const unsigned near_core = rows_meeting(mine->core_first, mine->core_last, i0, P);
        const unsigned packed = all_region_one | ((near_core & ~all_region_one) << 8);
        for (int k = 0; k < n; k += 2)
        {
            const int j = begin + base + k;
            const LineWing la = wing[j], lb = wing[j + 1];
            core_pair<P>(la, lb, core + j,
                         (unsigned)__builtin_amdgcn_readlane((int)packed, k),
                         (unsigned)__builtin_amdgcn_readlane((int)packed, k + 1), v, acc);
        }
    }
}

template <int P>
__device__ __forceinline__ void general_ranges(const LineWing * __restrict__ wing,
                                               const LineCore * __restrict__ core,
                                               const GeneralList & g, int i0, int i1, int lane,
                                               const double (&v)[P], double (&acc)[P])
{
    // The core range (the bulk) ...
    core_lines<P>(wing, core, g.begin[1], g.count[1] & ~1, i0, lane, v, acc);
    // ... and its odd line with the few lines of the other ranges, one at a time.
    GeneralList rest = g;
    rest.begin[1] = g.begin[1] + (g.count[1] & ~1);
    rest.count[1] = g.count[1] & 1;
    const int total = rest.count[0] + rest.count[1] + rest.count[2] + rest.count[3] + rest.count[4];
    for (int k = 0; k < total; ++k)
    {
        const int j = general_index(rest, k);
        const LineWing l = wing[j];
        const LineCore c = core[j];
        general_line<P>(l, &c, i0, i1, lane, v, acc);
    }
}

// The lines whose windows END inside the tile (ranges [lo,a1) and [a2,hi)), when the cut-off is
// wide enough that the tile lies in the Lorentz wing of every one of them (the host's test,
// AccumulateArgs::inner_everywhere == 0).  Windows begin and end on integer wavenumbers
// (spectra.c:48-62), so neighbours in the sorted table mostly share theirs: eight lines with the
// same [first, last] are summed like a far-wing group -- one reciprocal, rows outside the window
// skipped, the row the window ends in masked -- instead of line by line, row by row.  On grids
// whose tiles are aligned to the 1 cm-1 cells this is the closing point of ~80 windows on the
// first tile of every cell; on coarse grids (100 points per cm-1) a tenth of all (line, tile)
// pairs.  Groups that straddle a change of window, and what is left over, go line by line.
template <int P>
__device__ __forceinline__ void clipped_ranges(const LineWing * __restrict__ wing,
                                               const LineCore * __restrict__ core,
                                               int begin0, int count0, int begin1, int count1,
                                               int i0, int i1, int lane,
                                               const double (&v)[P], double (&acc)[P])
{
    const int total = count0 + count1;
    int k = 0;
    while (k < total)
    {
        const int j = k < count0 ? begin0 + k : begin1 + (k - count0);
        const bool room = k < count0 ? k + 8 <= count0 : k + 8 <= total;
        if (room)
        {
            // Lanes 0-7 (and their copies) look at the eight windows; the records are asked for
            // at the same time (one round trip, not two: they are rarely not wanted).
            const LineWing * __restrict__ mine = wing + j + (lane & 7);
            const int my_first = mine->first, my_last = mine->last;
            WingTerm l[8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
            {
                const LineWing w = wing[j + i];
                l[i] = WingTerm{w.centre, w.g2, w.bl};
            }
            const int first = __builtin_amdgcn_readfirstlane(my_first);
            const int last = __builtin_amdgcn_readfirstlane(my_last);
            if (__ballot(my_first != first || my_last != last) == 0)
            {
#pragma unroll
                for (int p = 0; p < P; ++p)
                {
                    const int r0 = i0 + p*64;
                    if (last < r0 || first > r0 + 63)
                    {
                        continue;
                    }
                    const int i = r0 + lane;
                    // Lanes outside the window add 0/den (den is a finite product of eight t):
                    // selected on the numerator, the sum stays in its own register.
                    double num, den;
                    wing_eight(v[p], l, num, den);
                    acc[p] = __builtin_fma((i >= first && i <= last) ? num : 0., rcp_newton(den),
                                           acc[p]);
                }
                k += 8;
                continue;
            }
        }
        const LineWing w = wing[j];
        const LineCore c = core[j];
        general_line<P>(w, &c, i0, i1, lane, v, acc);
        k += 1;
    }
}

// The second pass over the lines of the general list, kInnerQueue at a time with lane = line
// (their records arrive by one coalesced gather): the inner points the rows left out.  Kept
// apart from the walk above on purpose -- the two need different registers, and as one loop each
// paid for the other's (53 spilled SGPRs against 26, 1-6 % on workloads that have no inner point
// to evaluate).
__device__ __forceinline__ bool inner_ranges(const LineWing * __restrict__ wing,
                                             const LineCore * __restrict__ core,
                                             const GeneralList & g, InnerStage & stage,
                                             int i0, int i1, int v0, int n_per_v, double dv,
                                             int lane, double * slab, int slab_rows)
{
    bool used = false;
    const int total = g.count[0] + g.count[1] + g.count[2] + g.count[3] + g.count[4];
    for (int base = 0; base < total; base += kInnerQueue)
    {
        const int k = base + lane;
        const bool has = lane < kInnerQueue && k < total;
        // general_index() lane by lane.
        int j = g.begin[0], rest = has ? k : 0;
#pragma unroll
        for (int r = 0; r < 5; ++r)
        {
            const bool here = rest >= 0 && rest < g.count[r];
            j = here ? g.begin[r] + rest : j;
            rest = here ? -1 : rest - g.count[r];
        }
        used |= inner_batch(wing, core, stage, j, has, i0, i1, v0, n_per_v, dv, lane, slab, used,
                            slab_rows);
    }
    return used;
}

}  // namespace lbl
