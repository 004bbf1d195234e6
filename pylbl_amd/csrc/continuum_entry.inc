// Host side of the continuum entry points of include/lbl_amd.h (kernels: continuum.h).
// Included at the end of engine.hip after slot_entry.inc.  Like the lines path there is no CPU
// compute here.

namespace {

const int kBandColumns[kBandKinds] = {2, 2, 3, 4, 3, 1, 2, 1, 1, 1, 1, 1, 1, 3, 3, 1};

// utils.py:16-42: dry air from the ideal-gas law at the Loschmidt reference, air = dry air
// times the sum of all mole fractions.
ContinuumLevel continuum_level(double temperature, double pressure_mb, const double * vmr)
{
    ContinuumLevel s;
    s.t = temperature;
    s.p = pressure_mb;
    s.dry = mtckd::kLoschmidt*(pressure_mb/mtckd::kP0)*(mtckd::kT273/temperature)*
            (1. - vmr[LBL_VMR_H2O]);
    s.air = s.dry*vmr[LBL_VMR_TOTAL];
    s.self = vmr[LBL_VMR_SELF];
    s.h2o = vmr[LBL_VMR_H2O];
    s.o2 = vmr[LBL_VMR_O2];
    s.n2 = vmr[LBL_VMR_N2];
    return s;
}

void launch_band_spectra(ContinuumSet & c, int n_levels, hipStream_t stream)
{
    dim3 grid((unsigned)((c.widest + 255)/256), (unsigned)c.set.n_bands, (unsigned)n_levels);
    hipLaunchKernelGGL(band_spectra_kernel, grid, dim3(256), 0, stream, c.set, c.table.data,
                       c.levels.data, c.coarse.data, c.slopes.data);
    HIP_TRY(hipGetLastError());
}

}  // namespace

extern "C" {

int lbl_continuum_load(lbl_engine * engine, int32_t n_bands, const lbl_band * bands,
                       const double * table, int64_t table_size, int32_t * continuum)
{
    return entry(engine, [&] {
        if (continuum == nullptr || bands == nullptr || table == nullptr || n_bands < 1 ||
            n_bands > kMaxBands || table_size < 1)
        {
            return fail(engine, LBL_BAD_ARGUMENT, "lbl_continuum_load: bad argument.");
        }
        HIP_TRY(hipSetDevice(engine->device));
        std::unique_ptr<ContinuumSet> c(new ContinuumSet());
        c->set.n_bands = n_bands;
        long long points = 0;
        for (int k = 0; k < n_bands; ++k)
        {
            const lbl_band & in = bands[k];
            if (in.kind < 0 || in.kind >= kBandKinds || in.size < 2 || !(in.resolution > 0.) ||
                !std::isfinite(in.lower_bound))
            {
                return fail(engine, LBL_BAD_ARGUMENT,
                            "band " + std::to_string(k) + ": bad kind, size or grid.");
            }
            Band & b = c->set.band[k];
            b.kind = in.kind;
            b.size = in.size;
            b.lower = in.lower_bound;
            b.resolution = in.resolution;
            b.per_step = 1./in.resolution;
            for (int col = 0; col < 4; ++col)
            {
                const bool needed = col < kBandColumns[in.kind];
                const long long at = in.column[col];
                if (needed && (at < 0 || at + in.size > table_size))
                {
                    return fail(engine, LBL_BAD_ARGUMENT,
                                "band " + std::to_string(k) + ": column " +
                                std::to_string(col) + " lies outside the table.");
                }
                b.column[col] = needed ? at : -1;
            }
            b.spectrum = points;
            points += in.size;
            c->widest = std::max(c->widest, (int)in.size);
        }
        c->set.coarse_points = (int)points;
        c->table.upload(table, (size_t)table_size, engine->stream);
        HIP_TRY(hipStreamSynchronize(engine->stream));
        *continuum = store_slot(engine->continua, std::move(c));
        return LBL_OK;
    });
}

int lbl_continuum_free(lbl_engine * engine, int32_t continuum)
{
    return free_slot(engine, &lbl_engine::continua, continuum, "unknown continuum handle.", [&] {
        // (groups that hold the continuum's table go with it)
        for (auto & group : engine->groups)
        {
            if (group && std::find(group->members.begin(), group->members.end(), continuum) !=
                             group->members.end())
            {
                group.reset();
            }
        }
    });
}

int lbl_grid_load(lbl_engine * engine, int64_t n, const double * wavenumber, int32_t * grid)
{
    return entry(engine, [&] {
        if (grid == nullptr || wavenumber == nullptr || n < 1 || n > 0x7fffffff)
        {
            return fail(engine, LBL_BAD_ARGUMENT,
                        "lbl_grid_load: bad argument (1 ... 2^31 - 1 points).");
        }
        HIP_TRY(hipSetDevice(engine->device));
        std::unique_ptr<SpectralGrid> g(new SpectralGrid());
        g->n = n;
        g->ascending = std::is_sorted(wavenumber, wavenumber + n);
        // numpy.arange fills first + i*(second - first) (compiled with -ffp-contract=off here, as
        // the kernels are: product rounded, then the sum).
        if (n >= 2)
        {
            const double start = wavenumber[0], step = wavenumber[1] - wavenumber[0];
            bool same = std::isfinite(start) && std::isfinite(step);
            for (int64_t i = 0; i < n && same; ++i)
            {
                const double offset = (double)i*step;
                same = (start + offset) == wavenumber[i];
            }
            g->arithmetic = same;
            g->start = start;
            g->step = step;
        }
        g->wavenumber.upload(wavenumber, (size_t)n, engine->stream);
        HIP_TRY(hipStreamSynchronize(engine->stream));
        *grid = store_slot(engine->grids, std::move(g));
        return LBL_OK;
    });
}

int lbl_grid_free(lbl_engine * engine, int32_t grid)
{
    return free_slot(engine, &lbl_engine::grids, grid, "unknown grid handle.");
}

int lbl_continuum_compute(lbl_engine * engine, int32_t continuum, int32_t grid,
                          int32_t n_levels, const double * temperature, const double * pressure,
                          const double * vmr, int32_t flags, double * extinction,
                          int64_t level_stride)
{
    return entry(engine, [&] {
        ContinuumSet * c = find_slot(engine->continua, continuum);
        if (c == nullptr) return fail(engine, LBL_BAD_ARGUMENT, "unknown continuum handle.");
        SlotCall call{engine, n_levels, flags, extinction};
        const int status = call.check(
            grid, level_stride,
            n_levels < 0 || extinction == nullptr ||
            (n_levels > 0 && (temperature == nullptr || pressure == nullptr || vmr == nullptr)),
            "lbl_continuum_compute: bad argument.");
        if (status != LBL_OK || n_levels == 0) return status;
        const SpectralGrid * g = call.g;
        const long long n = call.n;
        return call.run(*c, c->coarse, c->set.coarse_points, kTimeContinuum,
            [&](long long l) {      // utils.py:13,172
                return continuum_level(temperature[l], pressure[l]*0.01, vmr + l*LBL_VMR_COUNT);
            },
            [&](int count) {
                engine->timed(kTimeBandSpectra, call.stream, [&] {
                    launch_band_spectra(*c, count, call.stream);
                });
            },
            [&](int count, double * target, long long target_stride, int add) {
                // Measured on 5 M points (scripts/perf_continuum.py): 4 points x 1 level for a
                // single level, 2 points x 4 levels for a batch.
                const int pt = count == 1 ? 4 : 2, lv = count == 1 ? 1 : 4;
                const long long per_block = 256*pt;
                dim3 blocks((unsigned)((n + per_block - 1)/per_block),
                            (unsigned)((count + lv - 1)/lv));
#define LBL_INTERP(PT, LV)                                                                 \
                hipLaunchKernelGGL((continuum_interp_kernel<PT, LV>), blocks, dim3(256), 0, \
                                   call.stream, c->set, c->coarse.data, c->slopes.data,     \
                                   g->form(), n, count, target, target_stride, add)
                if (count == 1) LBL_INTERP(4, 1); else LBL_INTERP(2, 4);
#undef LBL_INTERP
            });
    });
}

int lbl_continuum_compute_many(lbl_engine * engine, int32_t n_continua,
                               const int32_t * continua, int32_t grid, int32_t n_levels,
                               const double * temperature, const double * pressure,
                               const double * vmr, int32_t flags, double * extinction,
                               int64_t level_stride)
{
    return entry(engine, [&] {
        if (n_continua < 1 || continua == nullptr)
        {
            return fail(engine, LBL_BAD_ARGUMENT, "lbl_continuum_compute_many: no continua.");
        }
        SlotCall call{engine, n_levels, flags, extinction};
        const int status = call.check(
            grid, level_stride,
            n_levels < 0 || extinction == nullptr || !(flags & LBL_OUT_DEVICE) ||
            (n_levels > 0 && (temperature == nullptr || pressure == nullptr || vmr == nullptr)),
            "lbl_continuum_compute_many: bad argument (the output is a device block: "
            "LBL_OUT_DEVICE).");
        if (status != LBL_OK || n_levels == 0) return status;
        std::vector<ContinuumSet *> sets;
        int total_bands = 0;
        for (int m = 0; m < n_continua; ++m)
        {
            ContinuumSet * c = find_slot(engine->continua, continua[m]);
            if (c == nullptr) return fail(engine, LBL_BAD_ARGUMENT, "unknown continuum handle.");
            sets.push_back(c);
            total_bands += c->set.n_bands;
        }
        if (total_bands > kMaxGroupBands)
        {
            return fail(engine, LBL_BAD_ARGUMENT, "more than 64 bands in one group of continua.");
        }
        call.open();
        hipStream_t stream = call.stream;
        // The group of exactly these continua in this order (built at first use).
        ContinuumGroup * group = nullptr;
        const std::vector<int32_t> wanted(continua, continua + n_continua);
        for (auto & candidate : engine->groups)
        {
            if (candidate && candidate->members == wanted) group = candidate.get();
        }
        if (group == nullptr)
        {
            std::unique_ptr<ContinuumGroup> fresh(new ContinuumGroup());
            fresh->members = wanted;
            std::vector<GroupBand> list;
            long long points = 0;
            for (int m = 0; m < n_continua; ++m)
            {
                for (int k = 0; k < sets[m]->set.n_bands; ++k)
                {
                    GroupBand gb;
                    gb.band = sets[m]->set.band[k];
                    gb.band.spectrum = points;
                    gb.table = sets[m]->table.data;
                    gb.owner = m;
                    gb.first_of_owner = k == 0 ? 1 : 0;
                    points += gb.band.size;
                    fresh->widest = std::max(fresh->widest, gb.band.size);
                    list.push_back(gb);
                }
            }
            fresh->n_bands = (int)list.size();
            fresh->level_points = (int)points;
            fresh->bands.upload(list.data(), list.size(), stream);
            HIP_TRY(hipStreamSynchronize(stream));      // the host list goes out of scope
            if (engine->groups.size() >= 32)
            {
                engine->drain_lanes();
                engine->groups.erase(engine->groups.begin());
            }
            engine->groups.push_back(std::move(fresh));
            group = engine->groups.back().get();
        }
        // Up to 65535 levels at a time, like the one-slot calls (SlotCall::run): the levels are a
        // launch dimension of both kernels.  Chunk after chunk on one stream, through the same
        // level block and coarse spectra.
        // (waits first: the previous call's copy may still read the pinned level block)
        const long long chunk = std::min<long long>(n_levels, 65535);
        ContinuumLevel * staged = group->pinned.refill((size_t)(n_continua*chunk));
        group->levels.reserve((size_t)(n_continua*chunk));
        group->coarse.reserve((size_t)(chunk*group->level_points));
        group->slopes.reserve((size_t)(chunk*group->level_points));
        for (long long base = 0; base < n_levels; base += chunk)
        {
            const int count = (int)std::min<long long>(chunk, n_levels - base);
            for (int m = 0; m < n_continua; ++m)
            {
                for (int l = 0; l < count; ++l)
                {
                    // vmr: [continuum][level][LBL_VMR_COUNT] -- LBL_VMR_SELF differs between them
                    staged[(size_t)m*count + l] = continuum_level(
                        temperature[base + l], pressure[base + l]*0.01,
                        vmr + ((size_t)m*n_levels + base + l)*LBL_VMR_COUNT);   // utils.py:13,172
                }
            }
            group->pinned.upload(group->levels.data, (size_t)n_continua*count, stream);
            engine->timed(kTimeBandSpectra, stream, [&] {
                dim3 blocks((unsigned)((group->widest + 255)/256), (unsigned)group->n_bands,
                            (unsigned)count);
                hipLaunchKernelGGL(group_band_spectra_kernel, blocks, dim3(256), 0, stream,
                                   group->bands.data, group->level_points, group->levels.data,
                                   count, group->coarse.data, group->slopes.data);
                HIP_TRY(hipGetLastError());
            });
            double * target = extinction + base*call.stride;
            engine->timed(kTimeContinuum, stream, [&] {
                // PT points x LV levels per thread.  Measured (round 5,
                // profiles/r05_perf_continuum_group.txt): 4 x 1 for one level (23 us for three
                // continua at 5 M points; 2 x 1: 29, 8 x 1: 28), 4 x 2 for batches; taking the
                // bands two to four at a time (table values requested together) only cost
                // registers.
                const int pt = 4, lv = count == 1 ? 1 : 2;
                const long long per_block = 256*pt;
                dim3 blocks((unsigned)((call.n + per_block - 1)/per_block),
                            (unsigned)((count + lv - 1)/lv));
#define LBL_GROUP_INTERP(PT, LV)                                                             \
                hipLaunchKernelGGL((group_interp_kernel<PT, LV>), blocks, dim3(256), 0,      \
                                   stream, group->bands.data, group->n_bands,                \
                                   group->level_points, group->coarse.data,                  \
                                   group->slopes.data, call.g->form(), call.n, count,        \
                                   target, call.stride, call.add_into ? 1 : 0)
                if (count == 1) LBL_GROUP_INTERP(4, 1); else LBL_GROUP_INTERP(4, 2);
#undef LBL_GROUP_INTERP
                HIP_TRY(hipGetLastError());
            });
            if (base + count < n_levels) group->pinned.wait();
        }
        group->mark(stream);
        return call.close();
    });
}

int lbl_continuum_bands(lbl_engine * engine, int32_t continuum, double temperature,
                        double pressure_mb, const double * vmr, double * spectra)
{
    return entry(engine, [&] {
        ContinuumSet * c = find_slot(engine->continua, continuum);
        if (c == nullptr) return fail(engine, LBL_BAD_ARGUMENT, "unknown continuum handle.");
        if (vmr == nullptr || spectra == nullptr)
        {
            return fail(engine, LBL_BAD_ARGUMENT, "lbl_continuum_bands: bad argument.");
        }
        HIP_TRY(hipSetDevice(engine->device));
        for (int i = 1; i < kAllLanes; ++i) engine->lanes[i].drain();
        hipStream_t stream = engine->stream;
        c->pinned.wait();
        const ContinuumLevel level = continuum_level(temperature, pressure_mb, vmr);
        c->levels.reserve(1);
        c->coarse.reserve((size_t)c->set.coarse_points);
        c->slopes.reserve((size_t)c->set.coarse_points);
        HIP_TRY(hipMemcpyAsync(c->levels.data, &level, sizeof(level), hipMemcpyHostToDevice,
                               stream));
        launch_band_spectra(*c, 1, stream);
        HIP_TRY(hipMemcpyAsync(spectra, c->coarse.data, (size_t)c->set.coarse_points*8,
                               hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return LBL_OK;
    });
}

}  // extern "C"
