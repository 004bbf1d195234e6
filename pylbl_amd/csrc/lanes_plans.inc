// Host-side helpers between the C ABI and the kernels: error reporting, the per-level scalars
// (spectra.c:17-19,29,41-42 hoisted out of the line loop), the range rule of
// absorption.c:80-83, the choice of tiling, the work-item plans of a (molecule, grid) and the
// launches of the accumulate kernel (plain, and as a replayed HIP graph for tiny grids).
// Included by engine.hip after engine_core.h.
namespace {

int fail(lbl_engine * engine, int code, const std::string & message)
{
    if (engine != nullptr)
    {
        std::lock_guard<std::recursive_mutex> guard(engine->mutex);
        engine->error = message;
        g_thread_error = message;
        g_thread_error_engine = engine;
    }
    else
    {
        g_create_error = message;
    }
    return code;
}

typedef std::lock_guard<std::recursive_mutex> EngineLock;

// The frame of an entry point: a null engine, the engine's lock, and HIP failures, failed host
// allocations and whatever else the standard library throws as LBL_ERROR: nothing leaves through
// the C ABI.  body() returns the entry's status.
template <typename Body>
int entry(lbl_engine * engine, Body body)
{
    if (engine == nullptr) return LBL_BAD_ARGUMENT;
    EngineLock lock(engine->mutex);
    try
    {
        return body();
    }
    catch (const HipFailure & f)
    {
        return fail(engine, LBL_ERROR, f.message);
    }
    catch (const std::bad_alloc &)
    {
        return fail(engine, LBL_ERROR, "host allocation failed.");
    }
    catch (const std::exception & e)
    {
        return fail(engine, LBL_ERROR, e.what());
    }
}

Molecule * find_molecule(lbl_engine * engine, int32_t handle)
{
    if (handle < 0 || (size_t)handle >= engine->molecules.size()) return nullptr;
    return engine->molecules[handle].get();
}

// spectral_database.c:97-104 with bounds checks the reference lacks.
bool tips_value(const Molecule & m, double temperature, int slot, double * value)
{
    const double * t = m.tips_t.data() + (size_t)slot*m.num_t;
    const double * q = m.tips_q.data() + (size_t)slot*m.num_t;
    const int i = (int)(floor(temperature)) - (int)(t[0]);
    if (i < 0 || i + 1 >= m.num_t) return false;
    *value = q[i] + (q[i+1] - q[i])*(temperature - t[i])/(t[i+1] - t[i]);
    return true;
}

bool fill_level(const Molecule & m, double temperature, double pressure, double vmr,
                LevelScalars & lv, std::string & why)
{
    const double pa_to_atm = 9.86923e-6;            // spectra.c:13
    const double r2 = 2*log(2)*8314.472;            // spectra.c:14
    const double kb = 1.38064852e-23;               // spectroscopy.py:15
    const double vlight = 2.99792458e8;
    const double sqrln2 = sqrt(log(2.));
    if (!(temperature > 0.) || !std::isfinite(temperature) || !std::isfinite(pressure) ||
        !std::isfinite(vmr))
    {
        why = "temperature, pressure and mixing ratio must be finite (temperature > 0).";
        return false;
    }
    std::memset(&lv, 0, sizeof(lv));
    lv.temperature = temperature;
    lv.p_atm = pressure*pa_to_atm;
    lv.p_partial = lv.p_atm*vmr;
    lv.tfact = 296./temperature;
    lv.t_minus_ref = temperature - 296.;
    lv.t_times_ref = temperature*296.;
    lv.density = pressure*vmr/(kb*temperature);
    double widest = 0.;
    for (int slot = 0; slot < kMassSlots; ++slot)
    {
        lv.doppler[slot] = 0.;
        lv.q_ratio[slot] = 0.;
        if (!(m.used_slots & (1u << slot))) continue;
        lv.doppler[slot] = sqrt(r2*temperature/m.mass[slot]);
        widest = std::max(widest, lv.doppler[slot]);
        double q_ref, q_t;
        if (!tips_value(m, 296., slot, &q_ref) || !tips_value(m, temperature, slot, &q_t))
        {
            why = "temperature " + std::to_string(temperature) +
                  " K (or 296 K) lies outside the partition-function table.";
            return false;
        }
        lv.q_ratio[slot] = q_ref/q_t;
    }
    lv.shift_max = fabs(lv.p_atm)*m.max_abs_delta*(1. + 1.e-12) + 1.e-12;
    // voigt.c:34: xlim0 = sqrt(15100 + y(40 - 3.6y)) <= 123.34 for every y.
    lv.core_reach = 123.4/sqrln2/vlight*widest*(1. + 1.e-9);
    return true;
}

int first_row_out_of_range(const Molecule & m, double nu_min, double nu_max)
{
    const auto & nu = m.nu_row;
    if (m.ascending)
    {
        if (nu.empty() || nu.front() < nu_min) return 0;
        return (int)(std::upper_bound(nu.begin(), nu.end(), nu_max) - nu.begin());
    }
    for (size_t i = 0; i < nu.size(); ++i)
    {
        if (nu[i] > nu_max || nu[i] < nu_min) return (int)i;   // absorption.c:80-83
    }
    return (int)nu.size();
}

// Points per lane P (tile = 64*P points) and the tiling.  Cell-aligned tiles are used when
// they waste at most 6 % of the lanes on padding.
int pick_tiling(const lbl_engine * engine, int farfield, int n_per_v, long long n, Tiling & tiling)
{
    const int forced = engine->points_per_lane;
    const bool is_forced = forced == 1 || forced == 2 || forced == 4 || forced == 8;
    const int candidates[4] = {8, 4, 2, 1};
    for (int c = 0; c < 4; ++c)
    {
        const int p = is_forced ? forced : candidates[c];
        const int width = 64*p;
        const int per_cell = (n_per_v + width - 1)/width;
        const double waste = (double)per_cell*width/n_per_v - 1.;
        // (With the far-field series the tiles are cell-aligned wherever that wastes few lanes: no
        // window ends inside a tile then -- bar the closing point -- and the lines left to the
        // direct kernel are few enough for that to show: 0.94 -> 0.86 ms per step on the 5 M-point
        // workload.  The direct kernel alone gains nothing, profiles/r03_ab_tiling.txt.)
        if ((engine->aligned_tiles || farfield) && waste <= 0.06)
        {
            tiling.aligned = 1;
            tiling.per_cell = per_cell;
            tiling.length = (n_per_v + per_cell - 1)/per_cell;
            tiling.n_tiles = (int)(n/n_per_v)*per_cell;
            return p;
        }
        if (is_forced) break;
    }
    int p = forced;
    if (!is_forced)
    {
        // Measured on the 0.001 cm-1 workload: 4 is ~2 % ahead of 8 for the direct kernel,
        // 8 is ahead when the far-field series carries most lines.  With the series a tile does
        // best at 0.5-1.3 cm-1 (the lines within four half-widths stay with the direct kernel):
        // at 0.01 cm-1 two points per lane, 0.467 -> 0.423 ms per step
        // (profiles/r04_farfield_small_grids.txt).
        p = (n_per_v >= 400 && farfield) ? 8 : (n_per_v >= 100 && farfield) ? 2
            : n_per_v >= 100 ? 4 : n_per_v >= 10 ? 2 : 1;
    }
    tiling.aligned = 0;
    tiling.per_cell = 0;
    tiling.length = 64*p;
    tiling.n_tiles = (int)((n + tiling.length - 1)/tiling.length);
    return p;
}

// Splits the tiles into work items of bounded size and orders them heaviest first.  Line
// counts per tile come from the sorted wavenumbers alone (pressure shifts move them by a line
// or two, which does not matter for balance); the exact per-level cut points are still the
// schedule kernel's.
Molecule::Plan & plan_for(lbl_engine * engine, int farfield, Molecule & m, const GridSpec & g,
                          const Tiling & tiling, int points, hipStream_t stream, int pieces = 1)
{
    for (size_t i = 0; i < m.plans.size(); ++i)
    {
        Molecule::Plan * p = m.plans[i].get();
        if (p->v0 == g.v0 && p->vn == g.vn && p->n_per_v == g.n_per_v &&
            p->cut_off == g.cut_off && p->points == points && p->aligned == tiling.aligned &&
            p->farfield == farfield && p->pieces == pieces)
        {
            // Most recently used last.
            std::rotate(m.plans.begin() + i, m.plans.begin() + i + 1, m.plans.end());
            return *m.plans.back();
        }
    }
    // A long-lived process may see many grids: keep the 16 most recent plans per molecule.
    if (m.plans.size() >= 16)
    {
        engine->drain_lanes();      // a queued kernel may still read the oldest plan's items
        m.plans.erase(m.plans.begin());
    }
    std::unique_ptr<Molecule::Plan> plan(new Molecule::Plan());
    plan->v0 = g.v0; plan->vn = g.vn; plan->n_per_v = g.n_per_v; plan->cut_off = g.cut_off;
    plan->points = points; plan->aligned = tiling.aligned; plan->farfield = farfield;
    plan->pieces = pieces;
    const int n_tiles = tiling.n_tiles;
    const std::vector<double> & nu = m.column[0];
    std::vector<long long> weight((size_t)n_tiles);
    std::vector<long long> clipped((size_t)n_tiles, 0);
    long long total = 0;
    for (int t = 0; t < n_tiles; ++t)
    {
        long long i0, i1;
        tile_bounds(tiling, t, g.n_per_v, g.n, i0, i1);
        double lo = (double)((i0 + g.n_per_v - 1)/g.n_per_v + g.v0 - g.cut_off - 1) - 0.05;
        double hi = (double)(i1/g.n_per_v + g.v0 + g.cut_off) + 1.05;
        if (farfield)
        {
            // Only the lines near the tile are evaluated point by point -- and those whose windows
            // end inside it (the ranges [lo,a1) and [a2,hi) of schedule_tile), which the series
            // cannot take: a few dozen on an even table, thousands where a dense cm-1 of lines
            // closes on the tile (counted apart, see below).
            const double full_lo = (double)((i1 + g.n_per_v - 1)/g.n_per_v + g.v0 - g.cut_off - 1);
            const double full_hi = (double)(i0/g.n_per_v + g.v0 + g.cut_off) + 1.;
            clipped[t] = std::max<long long>(0, std::lower_bound(nu.begin(), nu.end(), full_lo + 0.05) -
                                                std::lower_bound(nu.begin(), nu.end(), lo)) +
                         std::max<long long>(0, std::lower_bound(nu.begin(), nu.end(), hi) -
                                                std::lower_bound(nu.begin(), nu.end(), full_hi - 0.05));
            const double u0 = tile_centre(g.v0, g.dv, i0, i1);
            const double radius = kFarRatio*0.5*(double)(i1 - i0)*g.dv + 0.6;
            lo = std::max(lo, u0 - radius);
            hi = std::min(hi, u0 + radius);
        }
        weight[t] = std::lower_bound(nu.begin(), nu.end(), hi) -
                    std::lower_bound(nu.begin(), nu.end(), lo);
        total += weight[t];
    }
    // Aim for ~8 items per workgroup slot of the chip (256 CUs x 6 resident workgroups): enough
    // rounds that the last one costs little, few enough that uniform tables leave their tiles
    // whole -- every extra item pays the kernel's prologue again and every split tile a pass
    // of combine_kernel (A/B on the 5 M-point workloads: 2-3 % against items half that size).
    // Dense bands still get their heavy tiles cut.  On small grids (a launch does not fill the
    // chip; every scalar load is a miss) short chains of lines per wavefront matter more than the
    // per-item overhead: items down to 128 lines.  (Grids in between -- 0.01 cm-1 over 5000 cm-1,
    // ~2000 tiles -- do best with at least 2048 lines per item now that their calls take turns on
    // two lanes: 0.590 -> 0.579 ms per step against 1024, which had been 2 % ahead of 512.)
    // (Round 5: far-field plans on large grids take the same floor as direct ones.  With 128 the
    // 400 k-line table's 10 000 tiles of ~1 300 near lines were each cut in two -- twice the
    // workgroups, each paying the kernel's fixed part, 80 MB of partial sums and a combine pass:
    // far-field step with the pedestal 0.98 -> 0.85 ms, profiles/r05_ab_farped.txt.)
    const long long floor_lines = n_tiles < 1024 ? 128 : 2048;
    const long long target = std::max<long long>(floor_lines, total/(8*1536) + 1);
    // Streamed calls (lbl_compute_streamed) launch the tiles in `pieces` runs, each followed by
    // the copy of its columns: runs of about equal weight, every tile counted with a floor that
    // stands for its fixed cost.
    plan->tile_begin.assign((size_t)pieces + 1, n_tiles);
    plan->tile_begin[0] = 0;
    {
        const long long unit = std::max<long long>(total/std::max(n_tiles, 1), 1);
        const long long all = total + unit*n_tiles;
        long long running = 0;
        int piece = 1;
        for (int t = 0; t < n_tiles && piece < pieces; ++t)
        {
            running += weight[t] + unit;
            // (Runs of doubling weight -- 1/8, 1/8, 1/4, 1/2, so that the first copy of a
            // delivering call starts earlier -- were measured in round 5: +-0 on the user-facing
            // call, profiles/r05_perf_api_pieces.txt.)
            if (running*pieces >= all*piece)
            {
                plan->tile_begin[piece++] = t + 1;
            }
        }
    }
    std::vector<int> piece_of_tile((size_t)n_tiles, 0);
    for (int piece = 0; piece < pieces; ++piece)
    {
        for (int t = plan->tile_begin[piece]; t < plan->tile_begin[piece + 1]; ++t)
        {
            piece_of_tile[t] = piece;
        }
    }
    std::vector<WorkItem> items;
    std::vector<SplitTile> split;
    std::vector<long long> item_weight;
    long long slots = 0;
    plan->split_begin.assign((size_t)pieces + 1, 0);
    for (int t = 0; t < n_tiles; ++t)
    {
        int parts = (int)std::min<long long>(64, (weight[t] + target - 1)/target);
        if (parts < 1) parts = 1;
        // Far-field plans: a tile on which many windows end (each such line costs about three
        // evaluated ones, row by row) is cut by that load too; the plans of even tables stay as
        // they are.  (A 150 000-line table with 7 330 lines below 1 cm-1: four tiles at 25-27 cm-1
        // held the whole launch, 1.70 -> 0.7 ms per spectrum; profiles/r04_hitran_shaped.txt.)
        long long load = weight[t];
        if (3*clipped[t] > 4*target)
        {
            load += 3*clipped[t];
            parts = (int)std::min<long long>(64, (load + target - 1)/target);
        }
        const int slot = parts > 1 ? (int)slots : -1;
        if (parts > 1)
        {
            split.push_back(SplitTile{t, parts, slot, 0});      // ascending tiles: piece-major
            plan->split_begin[piece_of_tile[t] + 1] += 1;
            slots += parts;
        }
        for (int k = 0; k < parts; ++k)
        {
            items.push_back(WorkItem{t, k, parts, slot});
            item_weight.push_back(load/parts);
        }
    }
    for (int piece = 0; piece < pieces; ++piece)
    {
        plan->split_begin[piece + 1] += plan->split_begin[piece];
    }
    std::vector<int> order(items.size());
    std::iota(order.begin(), order.end(), 0);
    // Heaviest first -- by CLASS of weight (classes a quarter octave wide),
    // tiles in grid order within a class: on a table without bands every tile weighs the same to a
    // few per cent, and sorting those by their exact weight shuffles them, so that workgroups
    // running side by side read the line records of windows thousands of tiles apart.
    auto weight_class = [&](long long w) {
        return w > 0 ? std::floor(4.*std::log2((double)w)) : -1.;
    };
    std::vector<double> item_class(items.size());
    for (size_t i = 0; i < items.size(); ++i) item_class[i] = weight_class(item_weight[i]);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        const int pa = piece_of_tile[items[a].tile], pb = piece_of_tile[items[b].tile];
        return pa != pb ? pa < pb : item_class[a] > item_class[b];
    });
    plan->item_begin.assign((size_t)pieces + 1, 0);
    for (const auto & item : items)
    {
        plan->item_begin[piece_of_tile[item.tile] + 1] += 1;
    }
    for (int piece = 0; piece < pieces; ++piece)
    {
        plan->item_begin[piece + 1] += plan->item_begin[piece];
    }
    std::vector<WorkItem> sorted(items.size());
    for (size_t i = 0; i < items.size(); ++i) sorted[i] = items[order[i]];
    {
        // Workgroups go to the eight XCDs in turn (workgroup b of a launch to XCD b mod 8), each
        // with an L2 of its own.  Inside a run of items of one class (grid order) XCD x takes two
        // contiguous stretches of the run -- number x of sixteen, then number 15 - x -- instead of
        // every eighth item: the line records of a region of the grid are fetched into one L2, not
        // into all eight (FETCH_SIZE of the default launch 154 -> 32 MB).  An XCD cannot take work
        // from another; the pairing keeps their loads equal where the weight of a tile drifts along
        // the grid (core-range lines cost more towards high wavenumbers) -- one stretch each, and
        // the far-field step took 8 % longer (profiles/r05_ab_xcd_stretches.txt).
        std::vector<WorkItem> dealt(sorted.size());
        for (int piece = 0; piece < pieces; ++piece)
        {
            const size_t first = (size_t)plan->item_begin[piece];
            const size_t last = (size_t)plan->item_begin[piece + 1];
            size_t s = first;
            while (s < last)
            {
                size_t e = s + 1;
                while (e < last && item_class[order[e]] == item_class[order[s]]) ++e;
                const size_t length = e - s;
                std::vector<size_t> slots[8], mine[8], spill;
                for (size_t q = s; q < e; ++q) slots[(q - first) & 7].push_back(q);
                auto cut = [&](size_t j) { return s + length*j/16; };
                for (size_t x = 0; x < 8; ++x)
                {
                    for (size_t q = cut(x); q < cut(x + 1); ++q) mine[x].push_back(q);
                    for (size_t q = cut(15 - x); q < cut(16 - x); ++q) mine[x].push_back(q);
                }
                // (XCDs in the order they first appear in the run.)  Slot counts and stretch
                // lengths each differ by at most one, not in step: what does not fit an XCD's
                // slots goes to the XCDs with a slot to spare.
                auto xcd_of = [&](size_t x) { return (s - first + x) & 7; };
                for (size_t x = 0; x < 8; ++x)
                {
                    while (mine[x].size() > slots[xcd_of(x)].size())
                    {
                        spill.push_back(mine[x].back());
                        mine[x].pop_back();
                    }
                }
                for (size_t x = 0; x < 8; ++x)
                {
                    const auto & place = slots[xcd_of(x)];
                    while (mine[x].size() < place.size())
                    {
                        mine[x].push_back(spill.back());
                        spill.pop_back();
                    }
                    for (size_t i = 0; i < place.size(); ++i) dealt[place[i]] = sorted[mine[x][i]];
                }
                s = e;
            }
        }
        sorted.swap(dealt);
    }
    plan->n_items = (int)sorted.size();
    plan->n_split = (int)split.size();
    plan->partial_slots = slots;
    plan->items.upload(sorted.data(), sorted.size(), stream);
    plan->split.upload(split.data(), split.size(), stream);
    HIP_TRY(hipStreamSynchronize(stream));      // the host vectors go out of scope
    m.plans.push_back(std::move(plan));
    return *m.plans.back();
}

void launch_accumulate(int points, dim3 grid, hipStream_t stream, const AccumulateArgs & args)
{
    switch (points)
    {
    case 1: hipLaunchKernelGGL(accumulate_kernel<1>, grid, dim3(256), 0, stream, args); break;
    case 2: hipLaunchKernelGGL(accumulate_kernel<2>, grid, dim3(256), 0, stream, args); break;
    case 4: hipLaunchKernelGGL(accumulate_kernel<4>, grid, dim3(256), 0, stream, args); break;
    default: hipLaunchKernelGGL(accumulate_kernel<8>, grid, dim3(256), 0, stream, args); break;
    }
    HIP_TRY(hipGetLastError());
}

}  // namespace
