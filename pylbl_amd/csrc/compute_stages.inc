// The stages of one batched lines call, in the order compute() (compute_call.inc) strings them
// together: the request put into the engine's terms, the lane the call takes and what it waits for
// there, the level scalars of a pass, the prologue (on the host under LBL_PREP_HOST), the pedestal
// pre-pass, the launches of a piece, the part that finishes a pass, the ways results go back to
// host memory, and the end of the call.  Included by engine.hip after lanes_plans.inc.
namespace {

// A request checked and put into the engine's terms.
struct CallShape
{
    Molecule * m = nullptr;
    GridSpec g;
    long long n_long = 0;       // grid points
    long long stride = 0;       // doubles between the levels of the output
    RangeRule rule;
    Tiling tiling;
    int farfield = 0;           // far lines by power series
    int points = 0;             // grid points per lane of a tile
};

// Arguments as the ABI promises to check them (include/lbl_amd.h), the range rule of
// absorption.c:80-83, the tiling.  Returns LBL_OK or the status fail() recorded.
int shape_of(lbl_engine * engine, const ComputeRequest & rq, CallShape & s)
{
    s.m = find_molecule(engine, rq.molecule);
    if (s.m == nullptr) return fail(engine, LBL_BAD_ARGUMENT, "unknown molecule handle.");
    if (rq.n_levels < 1 || rq.temperature == nullptr || rq.pressure == nullptr ||
        rq.vmr == nullptr)
    {
        return fail(engine, LBL_BAD_ARGUMENT, "need at least one level with T, P and x.");
    }
    if (rq.n_per_v < 1 || rq.vn <= rq.v0 || rq.cut_off < 0)
    {
        return fail(engine, LBL_BAD_ARGUMENT,
                    "need vn > v0, n_per_v >= 1 and cut_off >= 0 (grid must start on an "
                    "integer wavenumber with spacing 1/integer).");
    }
    static_assert(LBL_MAX_PEDESTAL_CUT_OFF == pedestal_cut_off_limit(),
                  "LBL_MAX_PEDESTAL_CUT_OFF follows the pre-pass's LDS (pedestal.h)");
    if (rq.remove_pedestal && rq.cut_off > LBL_MAX_PEDESTAL_CUT_OFF)
    {
        return fail(engine, LBL_BAD_ARGUMENT,
                    "cut_off " + std::to_string(rq.cut_off) + " with remove_pedestal: the largest "
                    "supported is LBL_MAX_PEDESTAL_CUT_OFF = " +
                    std::to_string(LBL_MAX_PEDESTAL_CUT_OFF) +
                    " (the pedestal pre-pass's LDS); call without remove_pedestal for wider windows.");
    }
    s.n_long = (long long)(rq.vn - rq.v0)*rq.n_per_v;
    if (s.n_long > 0x3fffffff)
    {
        return fail(engine, LBL_BAD_ARGUMENT, "grid has more than 2^30 points.");
    }
    if (rq.k == nullptr && rq.derived == nullptr)
    {
        return fail(engine, LBL_BAD_ARGUMENT, "k is NULL.");
    }
    s.g.v0 = rq.v0; s.g.vn = rq.vn; s.g.n_per_v = rq.n_per_v; s.g.cut_off = rq.cut_off;
    s.g.n = (int)s.n_long;
    s.g.dv = 1./rq.n_per_v;
    s.stride = rq.level_stride > 0 ? rq.level_stride : s.n_long;
    if (s.stride < s.n_long)
    {
        return fail(engine, LBL_BAD_ARGUMENT, "level_stride < grid points.");
    }

    s.rule.policy = rq.range_policy == LBL_RANGE_SKIP ? 1 : 0;
    s.rule.nu_min = rq.v0 - (rq.cut_off + 1);
    s.rule.nu_max = rq.vn + rq.cut_off + 1;
    s.rule.row_limit = first_row_out_of_range(*s.m, s.rule.nu_min, s.rule.nu_max);
    for (const auto & bad : s.m->bad_rows)
    {
        if (line_accepted(s.rule, bad.nu, bad.row))
        {
            return fail(engine, LBL_OUT_OF_RANGE,
                        "row " + std::to_string(bad.row) + ": local_iso_id " +
                        std::to_string(bad.local_iso_id) +
                        " has no mass or no partition-function row.");
        }
    }

    // The far-field series: an engine-wide option, or this call's choice (LBL_FARFIELD).
    s.farfield = (engine->farfield || (rq.flags & LBL_FARFIELD)) ? 1 : 0;
    s.points = pick_tiling(engine, s.farfield, rq.n_per_v, s.n_long, s.tiling);
    if (s.farfield && kFarRatio*0.5*(double)s.tiling.length >= (double)rq.cut_off*rq.n_per_v)
    {
        // A tile so wide (coarse grids: 0.1 cm-1 and up) that no line of a window is kFarRatio
        // half-widths away: the series would sum nothing and its two kernels only cost their
        // launches (configs[0]: 0.033 -> 0.041 ms per step, profiles/r04_farfield_small_grids.txt).
        s.farfield = 0;
        s.points = pick_tiling(engine, s.farfield, rq.n_per_v, s.n_long, s.tiling);
    }
    return LBL_OK;
}

// What decides where a call runs and what it may overlap with.
struct CallTraits
{
    bool out_device, want_k;
    bool small;             // a launch does not fill the chip, latency rules
    bool add_into_block;    // LBL_ACCUMULATE
    bool pedestal_pass;     // remove_pedestal and lines to remove it from
    bool alternate;         // takes turns over the lanes instead of running on lane 0
};

CallTraits traits_of(const lbl_engine * engine, const ComputeRequest & rq, const CallShape & s)
{
    CallTraits t;
    t.out_device = (rq.flags & LBL_OUT_DEVICE) != 0;
    t.want_k = rq.k != nullptr;
    // Asynchronous calls that leave their spectra in device memory rotate over the lanes, because
    // sharing the GPU pays: for calls with a pedestal (their serial chain leaves it almost idle),
    // for calls on small grids (a launch does not fill the chip, latency rules: up to 2^20 points x
    // levels, BASELINE configs[1], 500 k points: 0.625 -> 0.597 ms per step with four calls in
    // flight), and -- round 5 -- for plain calls on large grids too: the next call's prologue and
    // the head of its accumulate grid run beside the tail of this one's, where the chip is no
    // longer full (5 M points, H2O + CO2: 4.30 -> 4.11 ms per step, configs[2] 12.15 -> 11.92;
    // profiles/r05_ab_plain_lanes.txt; option overlap_plain = 0 queues them back to back on lane
    // 0 again).  Anything the caller waits for runs on lane 0, behind all the other lanes hold.
    t.small = s.n_long*rq.n_levels <= engine->small_points;
    // With the far-field series a call is five short kernels whatever the grid: the next call's
    // prologue and series kernels fit beside this one's accumulate kernel (0.83 -> 0.77 ms per
    // step at 5 M points).
    const bool short_kernels = s.farfield != 0 && engine->small_points > 0;
    const bool large_plain = engine->overlap_plain != 0;
    // A call that adds into its output can share the GPU too when it removes the pedestal:
    // only its last kernel (pedestal_apply_kernel) touches the output, everything before
    // works in the lane's own buffers.
    t.add_into_block = (rq.flags & LBL_ACCUMULATE) != 0;
    // (A molecule without lines has no pedestal pass: its accumulate kernel itself adds
    // into the block, so such a call must not leave lane 0's ordering.)
    t.pedestal_pass = rq.remove_pedestal && s.m->n_lines > 0;
    t.alternate = (rq.flags & LBL_ASYNC) && t.want_k && rq.derived == nullptr &&
                  ((t.pedestal_pass && (!t.add_into_block || t.out_device)) ||
                   ((t.small || short_kernels || large_plain) && t.out_device &&
                    !t.add_into_block));
    return t;
}

// The lane of a call that takes turns (CallTraits::alternate).
int next_lane_for(lbl_engine * engine, const ComputeRequest & rq, const CallShape & s,
                  const CallTraits & t)
{
    // How many lanes: the runtime maps streams onto four hardware queues, and calls on more
    // lanes than that only stretch one another's kernels.  Measured (profiles/
    // r03_ab_lanes.txt): calls with a pedestal pass (two streams each) 4 lanes against 8:
    // -1 % on the default workload, -8...-12 % with the far-field series; calls on tiny
    // grids (three short dependent kernels, nothing to overlap but launch gaps) 2 lanes:
    // 23.6 us per call against 33-35 us on 4 or 8.
    // (Round 5: with the far-field series a call with a pedestal pass does best on two
    // lanes too -- its accumulate grid is short, and four calls' light kernels in flight
    // only keep each other's from being placed: 0.85 -> 0.82 ms per step.)
    // (Round 5: plain calls on grids between 2^15 and 2^20 points x levels -- BASELINE
    // configs[1] -- do best on THREE lanes, 0.583 -> 0.562 ms per step with four calls in
    // flight (4.45e12 -> 4.62e12), where the 3 010-point grid of configs[0] takes twice as
    // long per call on three as on two: profiles/r05_ab_small_lanes.txt.)
    const bool middle = t.small && !s.farfield && !t.pedestal_pass &&
                        s.n_long*rq.n_levels > (1ll << 15);
    const int rotate = engine->lanes_in_use > 0 ? engine->lanes_in_use
                       : (t.pedestal_pass && !s.farfield) ? 4 : middle ? 3 : 2;
    int lane_index = (int)(engine->next_lane++ % rotate);
    if (&engine->lanes[lane_index] == engine->deferred ||
        (lane_index == 0 && (rq.flags & LBL_DEFER_FINISH)))
    {
        lane_index = (int)(engine->next_lane++ % rotate);
    }
    // A call that delivers its result while it computes: not on a lane whose accumulate
    // launches would hold up its copies (see delivers_badly).
    for (int tries = 1; tries < rotate && rq.host != nullptr && t.out_device &&
                        engine->skip_delivery_lanes && engine->delivers_badly[lane_index];
         ++tries)
    {
        const int next = (int)(engine->next_lane % rotate);
        if (&engine->lanes[next] == engine->deferred) break;
        lane_index = next;
        engine->next_lane += 1;
    }
    return lane_index;
}

// The lane a call runs on, ordered against the calls on the other lanes and a call kept back.
Lane & take_lane(lbl_engine * engine, const ComputeRequest & rq, const CallShape & s,
                 const CallTraits & t, long long out_bytes)
{
    if ((rq.flags & LBL_DEFER_FINISH) || (!t.alternate && engine->deferred == &engine->lanes[0]))
    {
        // There is one deferral at a time; and a call about to reuse lane 0's buffers must not
        // find a kept-back call still needing them.  (Kept-back calls stay off lane 0,
        // next_lane_for, so a plain call -- another thread's, say -- leaves a deferral alone: the
        // order in which a pipeline's calls add into their block does not depend on who else uses
        // the engine.  The kept-back kernels order themselves behind every write of their block
        // when they are queued, run_finish.)
        engine->finish_deferred();
    }
    Lane & lane = engine->lanes[t.alternate ? next_lane_for(engine, rq, s, t) : 0];
    if (!t.alternate)
    {
        if ((rq.flags & LBL_ASYNC) && t.out_device)
        {
            engine->join_lanes(lane.main);      // the host keeps queueing
        }
        else
        {
            for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
        }
    }
    else
    {
        lane.used = true;
        if (t.out_device && !t.add_into_block)
        {
            // Calls on different lanes run side by side; two that write the same memory must
            // not: the later one waits for the earlier one's last kernel.  (A call that adds
            // into the block waits later, in front of the one kernel that does the adding.)
            engine->order_after_writers(lane.main, rq.k, out_bytes, &lane);
        }
    }
    return lane;
}

// Levels per pass, bounded by the workspace budget.
long long levels_per_pass(const lbl_engine * engine, const ComputeRequest & rq,
                          const CallShape & s, const CallTraits & t, const Molecule::Plan & plan)
{
    const long long n_lines = s.m->n_lines;
    const long long per_level = plan.partial_slots*64*s.points*8 + n_lines*(long long)(sizeof(LineWing) + sizeof(LineCore)) +
                                (long long)s.tiling.n_tiles*sizeof(TileSchedule) +
                                (t.out_device ? 0 : s.n_long*8) +
                                (rq.remove_pedestal ? pedestal_bytes_per_level(n_lines, rq.vn - rq.v0, rq.cut_off) : 0);
    const long long chunk = std::max(1ll, engine->workspace_bytes/std::max(per_level, 1ll));
    return std::min<long long>(std::min<long long>(chunk, rq.n_levels), 65535);
}

// One lines call on its lane: what the stages below share.
struct LinesCall
{
    lbl_engine * engine;
    const ComputeRequest & rq;
    const CallShape & shape;
    const CallTraits & traits;
    Lane & lane;
    hipStream_t stream;             // lane.main
    const Molecule::Plan & plan;
    bool streamed;                  // lbl_compute_streamed: columns go to host memory piece by piece
    int pieces;                     // runs of tiles launched one after the other; 1 unless streamed
    bool with_pedestal;
    long long out_bytes;            // the caller's block, first byte to last
    long long chunk;                // levels per pass
};

// The lane's buffers for passes of `chunk` levels.  (Waits for the copy of the previous call's
// level scalars out of the pinned block this call is about to fill.)
void reserve_for_call(const LinesCall & c)
{
    const ComputeRequest & rq = c.rq;
    const CallShape & s = c.shape;
    const CallTraits & t = c.traits;
    Lane & lane = c.lane;
    const long long n_lines = s.m->n_lines, n_tiles = s.tiling.n_tiles, chunk = c.chunk;
    lane.level_feed.refill((size_t)chunk);
    lane.levels.reserve((size_t)chunk);
    lane.wing.reserve((size_t)(chunk*std::max(n_lines, 1ll)));
    lane.core.reserve((size_t)(chunk*std::max(n_lines, 1ll)));
    lane.groups.reserve((size_t)(chunk*std::max((n_lines + 7) >> 3, 1ll)));
    lane.schedule.reserve((size_t)(chunk*n_tiles));
    if (t.want_k && !t.out_device) lane.staging.reserve((size_t)(chunk*s.n_long));
    if (c.with_pedestal && t.out_device && t.add_into_block)
    {
        lane.raw.reserve((size_t)(chunk*s.n_long));
    }
    if (t.want_k && s.farfield)
    {
        lane.far_series.reserve((size_t)(chunk*n_tiles*kFarTerms));
    }
    if (t.want_k)
    {
        lane.partial.reserve((size_t)std::max(1ll, chunk*c.plan.partial_slots*64*s.points));
    }
    lane.wing_bounds.reserve((size_t)(chunk*kWingBounds));
    if (rq.evals != nullptr)
    {
        lane.evals.reserve(1);
        HIP_TRY(hipMemsetAsync(lane.evals.data, 0, sizeof(unsigned long long), c.stream));
    }
    if (rq.derived != nullptr) lane.derived.reserve((size_t)(std::max(n_lines, 1ll)*8));
}

// The far-field series of `count` levels (farfield.h): the sums of distant lines per group of
// kFarGroup tiles, then per tile what only the tile can take, re-centred on it.
void launch_far_series(lbl_engine * engine, Lane & lane, const CallShape & s, int count,
                       hipStream_t stream)
{
    const GridSpec & g = s.g;
    const int n_tiles = s.tiling.n_tiles;
    const int n_groups = (n_tiles + kFarGroup - 1)/kFarGroup;
    const long long n_lines = s.m->n_lines;
    engine->timed(kTimeSchedule, stream, [&] {
        dim3 far_grid((unsigned)(((n_groups + 7)/8)*8), (unsigned)count);
        hipLaunchKernelGGL(farfield_series_kernel, far_grid, dim3(256), 0, stream, lane.wing.data,
                           lane.schedule.data, s.m->d_column[0].data, lane.levels.data, n_lines,
                           s.tiling, n_groups, g.v0, g.n_per_v, g.n, g.dv, lane.far_series.data);
        HIP_TRY(hipGetLastError());
    }, 1);
}

// Can any accepted line have y < 8.425 at this level (voigt.c:35-43: below that the inner
// regions exist)?  y = sqrt(ln2) gamma/alpha with gamma >= the smallest half-widths of the table
// at this pressure (spectra.c:25-26) and alpha <= the widest Doppler width at the largest accepted
// wavenumber (spectra.c:29, absorption.c:80-83).  The accumulate kernel skips its look for inner
// points at levels where the answer is no: all of a CO2 table at 1 atm, for instance.
void bound_inner_regions(const Molecule & m, const RangeRule & rule, LevelScalars & lv)
{
    lv.inner_possible = 1.;
    const double foreign = lv.p_atm - lv.p_partial;
    if (foreign >= 0. && lv.p_partial >= 0. && m.min_gamma_air >= 0. &&
        m.min_gamma_self >= 0. && m.n_lines > 0)
    {
        double widest = 0.;
        for (int slot = 0; slot < kMassSlots; ++slot)
        {
            widest = std::max(widest, lv.doppler[slot]);
        }
        const double power = std::min(pow(lv.tfact, m.min_n_air), pow(lv.tfact, m.max_n_air));
        const double gamma = (m.min_gamma_air*foreign + m.min_gamma_self*lv.p_partial)*power;
        const double alpha = (rule.nu_max/2.99792458e8)*widest;
        const double y_lower = sqrt(log(2.))*gamma/alpha*(1. - 1.e-9);
        if (alpha > 0. && y_lower >= 8.425)
        {
            lv.inner_possible = 0.;
        }
    }
}

// A few levels travel as kernel arguments of the prologue kernel (no copy in front of it); more
// go through the pinned block.
bool levels_inline(const lbl_engine * engine, int count)
{
    return engine->prep != LBL_PREP_HOST && count <= kInlineLevels;
}

// The level scalars of a pass into the lane's pinned block and, unless they travel inline, on
// their way to the device.  Returns LBL_OK or the status fail() recorded.
int stage_levels(const LinesCall & c, long long base, int count)
{
    const ComputeRequest & rq = c.rq;
    Lane & lane = c.lane;
    // The previous pass may still be reading the pinned block.
    if (base > 0) HIP_TRY(hipStreamSynchronize(c.stream));
    for (int l = 0; l < count; ++l)
    {
        std::string why;
        LevelScalars & lv = lane.level_feed.block[l];
        if (!fill_level(*c.shape.m, rq.temperature[base + l], rq.pressure[base + l],
                        rq.vmr[base + l], lv, why))
        {
            return fail(c.engine, LBL_OUT_OF_RANGE,
                        "level " + std::to_string(base + l) + ": " + why);
        }
        bound_inner_regions(*c.shape.m, c.shape.rule, lv);
    }
    if (!levels_inline(c.engine, count))
    {
        lane.level_feed.upload(lane.levels.data, (size_t)count, c.stream);
    }
    return LBL_OK;
}

// Can a line outside a tile's core range have its core in the tile?  Only if the window
// (cut_off + 1 on either side) is not much wider than a core can reach (schedule_tile:
// core_reach x wavenumber, + the widest pressure shift) plus a tile.
int inner_points_everywhere(const LevelScalars * levels, int count, const ComputeRequest & rq,
                            const CallShape & s)
{
    double reach = 0.;
    for (int l = 0; l < count; ++l)
    {
        const LevelScalars & lv = levels[l];
        const double kk = lv.core_reach;
        reach = std::max(reach, kk < 0.5 ? kk*(rq.vn + 1.)/(1. - kk) + 2.*lv.shift_max : 1.e9);
    }
    const double tile_width = (double)s.tiling.length*s.g.dv;
    return (rq.cut_off - 1. <= reach + tile_width + 1.) ? 1 : 0;
}

// The line from which the eights of the scaled far-wing records are counted (line_prep.h,
// WingGroup): the first line of the sorted table that the range rule can accept, nu >= v0 -
// (cut_off + 1) under either policy.  What lies below it in the table moves no group.
long long wing_group_base(const CallShape & s)
{
    const std::vector<double> & nu = s.m->column[0];
    return (long long)(std::lower_bound(nu.begin(), nu.begin() + s.m->n_lines, s.rule.nu_min) -
                       nu.begin());
}

// LBL_PREP_HOST: the per-line scalars of `count` levels made by the host's own prepare_line
// (line_prep.h, the code the prologue kernel runs) and copied over; the tile cut points by
// schedule_kernel.  Adds the closed-form eval count to *rq.evals.
struct HostPrep
{
    std::vector<LineWing> wing;
    std::vector<LineCore> core;
    std::vector<WingGroup> groups;
    std::vector<double> derived;
    std::vector<int> wing_bounds;
};

void prepare_on_host(lbl_engine * engine, Lane & lane, const ComputeRequest & rq,
                     const CallShape & s, int count, hipStream_t stream, HostPrep & hp)
{
    const Molecule & m = *s.m;
    const long long n_lines = m.n_lines;
    if (n_lines > 0)
    {
        hp.wing.resize((size_t)(count*n_lines));
        hp.core.resize((size_t)(count*n_lines));
        if (rq.derived != nullptr) hp.derived.assign((size_t)(n_lines*8), 0.);
        hp.wing_bounds.assign((size_t)(count*kWingBounds), kWingBoundsFill);
        unsigned long long total = 0;
        for (int l = 0; l < count; ++l)
        {
            for (long long j = 0; j < n_lines; ++j)
            {
                const bool ok = m.iso_slot[j] >= 0 &&
                                line_accepted(s.rule, m.column[0][j], m.order[j]);
                double * d = (rq.derived != nullptr && l == 0) ? hp.derived.data() + j*8
                                                               : nullptr;
                LineWing & w = hp.wing[(size_t)(l*n_lines + j)];
                const int status = prepare_line(
                    lane.level_feed.block[l], s.g, m.column[0][j], m.column[1][j], m.column[2][j],
                    m.column[3][j], m.column[4][j], m.column[5][j], m.column[6][j],
                    std::max(m.iso_slot[j], 0), ok, w, hp.core[(size_t)(l*n_lines + j)], d);
                if (status == 1 && w.last >= w.first) total += w.last - w.first + 1;
                int bound[kWingBounds];
                wing_line_bounds(s.g, m.column[0][j], status, w,
                                 hp.core[(size_t)(l*n_lines + j)], bound);
                for (int b = 0; b < kWingBounds; ++b)
                {
                    int & least = hp.wing_bounds[(size_t)(l*kWingBounds + b)];
                    least = std::min(least, bound[b]);
                }
            }
        }
        // The scaled records of the eights counted from the first line the range rule can accept
        // (line_prep.h): what prepare_block makes.  Only accumulate_kernel<4> reads them.
        const long long base = wing_group_base(s);
        const long long n_groups = s.points == 4 ? (n_lines - base + 7) >> 3 : 0;
        const long long group_stride = (n_lines + 7) >> 3;
        hp.groups.assign((size_t)(count*group_stride), WingGroup());
        for (int l = 0; l < count; ++l)
        {
            for (long long group = 0; group < n_groups; ++group)
            {
                double centre[8], g2[8], bl[8];
                const long long first = base + 8*group;
                const int lines = (int)std::min(8ll, n_lines - first);
                for (int i = 0; i < 8; ++i)
                {
                    const bool real = i < lines;
                    const LineWing * w = real ? &hp.wing[(size_t)(l*n_lines + first + i)]
                                              : nullptr;
                    centre[i] = real ? w->centre : 0.;
                    g2[i] = real ? w->g2 : 1.;
                    bl[i] = real ? w->bl : 0.;
                }
                wing_group_of(centre, g2, bl, lines, hp.groups[(size_t)(l*group_stride + group)]);
            }
        }
        engine->timed(kTimePrepare, stream, [&] {
            HIP_TRY(hipMemcpyAsync(lane.wing.data, hp.wing.data(),
                                   hp.wing.size()*sizeof(LineWing), hipMemcpyHostToDevice,
                                   stream));
            HIP_TRY(hipMemcpyAsync(lane.core.data, hp.core.data(),
                                   hp.core.size()*sizeof(LineCore), hipMemcpyHostToDevice,
                                   stream));
            HIP_TRY(hipMemcpyAsync(lane.groups.data, hp.groups.data(),
                                   hp.groups.size()*sizeof(WingGroup), hipMemcpyHostToDevice,
                                   stream));
            HIP_TRY(hipMemcpyAsync(lane.wing_bounds.data, hp.wing_bounds.data(),
                                   hp.wing_bounds.size()*sizeof(int), hipMemcpyHostToDevice,
                                   stream));
        });
        HIP_TRY(hipStreamSynchronize(stream));
        if (rq.evals != nullptr) *rq.evals += (int64_t)total;
    }
    if (rq.k != nullptr)
    {
        engine->timed(kTimeSchedule, stream, [&] {
            dim3 grid((unsigned)((8ll*s.tiling.n_tiles + 255)/256), (unsigned)count);
            hipLaunchKernelGGL(schedule_kernel, grid, dim3(256), 0, stream, m.view(),
                               lane.levels.data, s.g, s.tiling, s.farfield, lane.schedule.data);
            HIP_TRY(hipGetLastError());
        });
    }
}

// K1: per-line scalars (+ the tile cut points, in the same launch) of a pass.
void launch_prologue(const LinesCall & c, int count, HostPrep & hp)
{
    lbl_engine * engine = c.engine;
    const ComputeRequest & rq = c.rq;
    const CallShape & s = c.shape;
    Lane & lane = c.lane;
    hipStream_t stream = c.stream;
    if (engine->prep == LBL_PREP_HOST)
    {
        prepare_on_host(engine, lane, rq, s, count, stream, hp);
        return;
    }
    const bool inline_levels = levels_inline(engine, count);
    InlineLevels packed;
    if (inline_levels)
    {
        std::memcpy(packed.level, lane.level_feed.block, count*sizeof(LevelScalars));
    }
    // (the threads begin up to eight lines in front of the table: prepare_block)
    const int prepare_blocks = (int)((s.m->n_lines + 8 + 255)/256);
    const int schedule_blocks = c.traits.want_k ? (int)((8ll*s.tiling.n_tiles + 255)/256) : 0;
    // (every bound starts at kWingBoundsFill: byte 0x7f)
    HIP_TRY(hipMemsetAsync(lane.wing_bounds.data, 0x7f, (size_t)count*kWingBounds*sizeof(int),
                           stream));
    engine->timed(kTimePrepare, stream, [&] {
        dim3 grid((unsigned)std::max(prepare_blocks + schedule_blocks, 1), (unsigned)count);
        hipLaunchKernelGGL(prologue_kernel, grid, dim3(256), 0, stream, s.m->view(),
                           lane.levels.data, packed, inline_levels ? 1 : 0, s.g, s.rule, s.tiling,
                           s.farfield, prepare_blocks, lane.wing.data, lane.core.data,
                           lane.schedule.data,
                           rq.derived != nullptr ? lane.derived.data : nullptr,
                           rq.evals != nullptr ? lane.evals.data : nullptr,
                           lane.wing_bounds.data,
                           s.points == 4 ? lane.groups.data : nullptr, (int)wing_group_base(s));
        HIP_TRY(hipGetLastError());
    });
}

// Where the spectra of a pass end up, where the accumulate kernel writes, and the streams of the
// pedestal pre-pass and of the part that finishes the pieces.
Lane::Pass pass_of(const LinesCall & c, long long base, int count)
{
    const CallTraits & t = c.traits;
    Lane::Pass p;
    p.base = base;
    p.count = count;
    p.target = t.out_device ? c.rq.k + base*c.shape.stride : c.lane.staging.data;
    p.target_stride = t.out_device ? c.shape.stride : c.shape.n_long;
    p.sums = p.target;
    p.sums_stride = p.target_stride;
    if (c.with_pedestal && t.out_device && t.add_into_block)
    {
        p.sums = c.lane.raw.data;
        p.sums_stride = c.shape.n_long;
    }
    p.ped_stream = c.engine->overlap_pedestal ? c.lane.side : c.stream;
    // With a pedestal the pieces are finished on the stream the chain runs on (the apply kernels
    // follow it there, while the main stream goes on with the accumulate launches of the later
    // pieces), else on the main stream.
    p.finish_stream = c.with_pedestal ? p.ped_stream : c.stream;
    return p;
}

// The pedestal pre-pass only needs the per-line scalars: it runs on the side stream next to the
// accumulate kernel (its serial chain keeps one CU busy).  Its run-finding kernels go first: once
// the accumulate grid owns the chip their wide workgroups would wait for it to drain.
void start_pedestal_search(const LinesCall & c, const Lane::Pass & p)
{
    lbl_engine * engine = c.engine;
    Lane & lane = c.lane;
    if (engine->overlap_pedestal)
    {
        lane.prepared.record(c.stream);
        HIP_TRY(hipStreamWaitEvent(lane.side, lane.prepared, 0));
    }
    engine->timed(kTimePedestal, p.ped_stream, [&] {
        pedestal_find_runs(lane.pedestal, p.ped_stream, c.shape.m->view(), lane.wing.data,
                           c.shape.g, p.count, c.rq.vn - c.rq.v0, engine->scan_chain != 0,
                           engine->poison_workspace != 0);
    }, 0);
    if (engine->overlap_pedestal)
    {
        lane.runs_found.record(lane.side);
    }
}

AccumulateArgs accumulate_args(const LinesCall & c, const Lane::Pass & p)
{
    const ComputeRequest & rq = c.rq;
    const CallShape & s = c.shape;
    const GridSpec & g = s.g;
    const Lane & lane = c.lane;
    const bool add_into = c.traits.out_device && c.traits.add_into_block;
    AccumulateArgs args;
    args.wing = lane.wing.data;
    args.core = lane.core.data;
    args.schedule = lane.schedule.data;
    args.levels = lane.levels.data;
    args.items = c.plan.items.data;
    args.far_series = s.farfield ? lane.far_series.data : nullptr;
    args.wing_bounds = lane.wing_bounds.data;
    args.wing_batches = c.engine->wing_batches;
    args.groups = lane.groups.data;
    args.group_base = (int)wing_group_base(s);
    {
        // Tiles that begin at or above max(64, 2 (cut_off + 2)) cm-1 take the scaled eights: as a
        // grid index, v = v0 + i/n_per_v (accumulate_lines.h, scaled_ranges).
        const long long gate = std::max(64ll, 2ll*((long long)g.cut_off + 2));
        const long long from = std::max(0ll, gate - (long long)g.v0)*(long long)g.n_per_v;
        args.scaled_from = (int)std::min(from, 0x7fffffffll);
    }
    args.partial = lane.partial.data;
    args.partial_slots = c.plan.partial_slots;
    args.level_stride = p.sums_stride;
    args.k = p.sums;
    args.n_lines = s.m->n_lines;
    args.tiling = s.tiling;
    args.n_tiles = s.tiling.n_tiles;
    args.n = g.n;
    args.v0 = g.v0;
    args.n_per_v = g.n_per_v;
    args.dv = g.dv;
    args.v0_real = (double)g.v0;
    // With a pedestal the kernel stores plain sums; pedestal_apply_kernel finishes.
    args.scale_density = (!c.with_pedestal && (rq.flags & LBL_SCALE_DENSITY)) ? 1 : 0;
    args.accumulate = (!c.with_pedestal && add_into) ? 1 : 0;
    args.inner_everywhere = inner_points_everywhere(lane.level_feed.block, p.count, rq, s);
#ifdef LBL_ABLATE
    args.ablate = c.engine->ablate;
#endif
    return args;
}

// The accumulate launch of a piece's work items and the sums of its split tiles.
void launch_piece(const LinesCall & c, const Lane::Pass & p, const AccumulateArgs & args,
                  int piece)
{
    const Molecule::Plan & plan = c.plan;
    hipStream_t stream = c.stream;
    const int points = c.shape.points, count = p.count;
    const int item0 = plan.item_begin[piece], item1 = plan.item_begin[piece + 1];
    const int split0 = plan.split_begin[piece], split1 = plan.split_begin[piece + 1];
    c.engine->timed(kTimeAccumulate, stream, [&] {
        if (item1 > item0)
        {
            // One workgroup per work item, heaviest items first.
            AccumulateArgs mine = args;
            mine.items = plan.items.data + item0;
            dim3 grid((unsigned)(item1 - item0), (unsigned)count);
            launch_accumulate(points, grid, stream, mine);
        }
        if (split1 > split0)
        {
            const int units = (split1 - split0)*points;     // (split tile, 64-point row)
            hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((units + 3)/4), (unsigned)count),
                               dim3(256), 0, stream, args, plan.split.data + split0,
                               split1 - split0, 64*points);
            HIP_TRY(hipGetLastError());
        }
    });
}

// Lane::Finish of a pass: what copy_piece_home and run_finish go by.
void describe_finish(const LinesCall & c, const Lane::Pass & p)
{
    const ComputeRequest & rq = c.rq;
    const CallTraits & t = c.traits;
    Lane::Finish & f = c.lane.finish;
    f.pass = p;
    f.g = c.shape.g;
    f.pieces = c.pieces;
    f.flags = rq.flags;
    // (a run of tiles may be empty -- few tiles, uneven weights -- and must not move its
    // neighbours' bounds: entry i is both the end of run i-1 and the start of run i)
    long long reached = 0;
    for (int piece = 0; piece < c.pieces; ++piece)
    {
        long long q0, q1;
        c.plan.point_range(piece, c.shape.tiling, c.shape.g, q0, q1);
        if (q1 <= q0)
        {
            q0 = q1 = reached;
        }
        f.point_begin[piece] = q0;
        f.point_begin[piece + 1] = q1;
        reached = q1;
    }
    f.streamed = c.streamed;
    f.add_into = t.out_device && t.add_into_block;
    f.order_writers = t.alternate && f.add_into;
    f.host = rq.host;
    f.host_pitch = rq.host_pitch;
    f.columns = rq.columns;
    // The block's write record: only once, behind the call's last pass.
    const bool last_pass = p.base + p.count >= rq.n_levels;
    f.k = (t.out_device && last_pass) ? rq.k : nullptr;
    f.block = rq.k;
    f.out_bytes = c.out_bytes;
}

// Behind the accumulate launches of a pass with a pedestal: the pedestal chain (the host waits for
// the run counts inside), then what finishes the pieces -- now, or kept back.  (Queueing the chain
// in front of the accumulate launches of a far-field call: +-0, profiles/r05_ab_chain_first.txt.)
void finish_with_pedestal(const LinesCall & c, const Lane::Pass & p)
{
    lbl_engine * engine = c.engine;
    const ComputeRequest & rq = c.rq;
    Lane & lane = c.lane;
    engine->timed(kTimePedestal, p.ped_stream, [&] {
        pedestal_finish(lane.pedestal, p.ped_stream, c.shape.m->view(), lane.wing.data,
                        lane.core.data, c.shape.g, p.count, rq.vn - rq.v0,
                        engine->scan_chain != 0, engine->relax_launches,
                        engine->poison_workspace != 0);
    });
    lane.finish.pending = true;
    // Kept back for lbl_finish_deferred only if nothing of this call comes after it: one pass,
    // spectra in device memory, the host not waiting.
    if ((rq.flags & LBL_DEFER_FINISH) && (rq.flags & LBL_ASYNC) && c.traits.out_device &&
        c.traits.alternate && c.chunk >= rq.n_levels && rq.evals == nullptr)
    {
        engine->deferred = &lane;
    }
    else
    {
        engine->run_finish(lane);
    }
}

// Spectra of one pass from the lane's staging block into the caller's host memory (a call
// without LBL_OUT_DEVICE): one copy where the rows are dense and nothing is added, through a
// temporary otherwise.  Waits, except for the last pass of a blocking call (the end of the call
// waits for that one).
void spectra_to_host(Lane & lane, const ComputeRequest & rq, const CallShape & s,
                     long long base, int count, hipStream_t stream)
{
    const long long n_long = s.n_long;
    if (s.stride == n_long && !(rq.flags & LBL_ACCUMULATE))
    {
        HIP_TRY(hipMemcpyAsync(rq.k + base*s.stride, lane.staging.data, (size_t)count*n_long*8,
                               hipMemcpyDeviceToHost, stream));
        if (base + count < rq.n_levels || (rq.flags & LBL_ASYNC))
        {
            HIP_TRY(hipStreamSynchronize(stream));
        }
        return;
    }
    std::vector<double> tmp((size_t)count*n_long);
    HIP_TRY(hipMemcpyAsync(tmp.data(), lane.staging.data, tmp.size()*8, hipMemcpyDeviceToHost,
                           stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int l = 0; l < count; ++l)
    {
        double * dst = rq.k + (base + l)*s.stride;
        const double * src = tmp.data() + (size_t)l*n_long;
        if (rq.flags & LBL_ACCUMULATE)
        {
            for (long long i = 0; i < n_long; ++i) dst[i] += src[i];
        }
        else
        {
            std::memcpy(dst, src, (size_t)n_long*8);
        }
    }
}

// The per-line derived scalars (lbl_derived: spectra.c:17-62 per line) back in the reference's
// row order.
void derived_to_host(lbl_engine * engine, Lane & lane, const ComputeRequest & rq,
                     const CallShape & s, const HostPrep & hp, hipStream_t stream)
{
    const long long n_lines = s.m->n_lines;
    std::vector<double> sorted((size_t)(n_lines*8));
    if (engine->prep == LBL_PREP_HOST)
    {
        sorted = hp.derived;
    }
    else if (n_lines > 0)
    {
        HIP_TRY(hipMemcpyAsync(sorted.data(), lane.derived.data, sorted.size()*8,
                               hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    for (long long j = 0; j < n_lines; ++j)
    {
        std::memcpy(rq.derived + (size_t)s.m->order[j]*8, sorted.data() + (size_t)j*8, 64);
    }
}

// The end of a call: the block's write record, what goes back by value, and the wait of a call
// without LBL_ASYNC -- here, or left to the caller as an event (compute()'s wait_for).
int end_call(const LinesCall & c, const HostPrep & hp, Event * wait_for)
{
    lbl_engine * engine = c.engine;
    const ComputeRequest & rq = c.rq;
    Lane & lane = c.lane;
    hipStream_t stream = c.stream;
    if (c.traits.out_device && c.traits.want_k && !c.with_pedestal)
    {
        lane.note_write(rq.k, c.out_bytes, stream);     // (with a pedestal: run_finish does)
    }
    if (rq.evals != nullptr && !(engine->prep == LBL_PREP_HOST))
    {
        unsigned long long total = 0;
        HIP_TRY(hipMemcpyAsync(&total, lane.evals.data, sizeof(total), hipMemcpyDeviceToHost,
                               stream));
        HIP_TRY(hipStreamSynchronize(stream));
        *rq.evals = (int64_t)total;
    }
    if (rq.derived != nullptr)
    {
        derived_to_host(engine, lane, rq, c.shape, hp, stream);
    }
    if (!(rq.flags & LBL_ASYNC))
    {
        if (wait_for != nullptr)
        {
            *wait_for = engine->take_event();
            wait_for->record(stream);
        }
        else
        {
            HIP_TRY(hipStreamSynchronize(stream));
        }
    }
    return LBL_OK;
}

}  // namespace
