// lbl_path_flux_source: one sweep (down from space or up from the surface) of K angles through a
// block of absorption coefficients in HBM (kernel: flux.h; band means: path.h), and
// lbl_path_flux, the same call without edge temperatures.  Included by engine.hip
// after radiance_entry.inc; shares path_entry.inc's PathCall, PathTables and PathBands.
namespace {

template <bool kVector, int K>
void launch_flux(const PathFlux & a, const dim3 & grid, hipStream_t stream)
{
    if (a.edge != nullptr)
    {
        hipLaunchKernelGGL((path_flux_kernel<kVector, K, true>), grid, dim3(kPathThreads), 0,
                           stream, a);
    }
    else
    {
        hipLaunchKernelGGL((path_flux_kernel<kVector, K>), grid, dim3(kPathThreads), 0, stream, a);
    }
}

template <bool kVector>
void launch_flux(int angles, const PathFlux & a, const dim3 & grid, hipStream_t stream)
{
    switch (angles)
    {
    case 1: launch_flux<kVector, 1>(a, grid, stream); break;
    case 2: launch_flux<kVector, 2>(a, grid, stream); break;
    case 3: launch_flux<kVector, 3>(a, grid, stream); break;
    case 4: launch_flux<kVector, 4>(a, grid, stream); break;
    case 5: launch_flux<kVector, 5>(a, grid, stream); break;
    case 6: launch_flux<kVector, 6>(a, grid, stream); break;
    case 7: launch_flux<kVector, 7>(a, grid, stream); break;
    default: launch_flux<kVector, 8>(a, grid, stream); break;
    }
}

}  // namespace

extern "C" {

int lbl_path_flux_source(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                         int32_t grid, int32_t n_paths, int32_t levels_per_path,
                         int32_t level_begin, int32_t level_count, int32_t n_angles,
                         const double * path_length, const double * weight,
                         const double * temperature, const double * edge_temperature,
                         const double * surface_temperature, const double * surface_emissivity,
                         int32_t n_bands, const int64_t * band_start, double * carry,
                         double * reflection, double * level_flux, double * flux,
                         double * surface_flux, int32_t flags)
{
    return path_entry(engine, flags, [&] {
        PathCall call{engine, "lbl_path_flux_source", row_stride, columns, n_paths, levels_per_path,
                      level_begin, level_count, flags};
        const bool up = (flags & LBL_PATH_FLUX_UP) != 0;
        if (beta == nullptr || path_length == nullptr || weight == nullptr ||
            temperature == nullptr || carry == nullptr || reflection == nullptr ||
            level_flux == nullptr)
        {
            return call.bad("beta, path_length, weight, temperature, carry, reflection and "
                            "level_flux must not be NULL.");
        }
        if (level_flux == beta)
        {
            return call.bad("level_flux must not be beta: the up sweep reads it.");
        }
        if (up && (surface_temperature == nullptr || surface_emissivity == nullptr))
        {
            return call.bad("the up sweep needs surface_temperature and surface_emissivity.");
        }
        if (n_angles < 1 || n_angles > kFluxMaxAngles) return call.bad("need 1 <= n_angles <= 8.");
        if (const char * problem = call.find_grid(grid)) return call.bad(problem);
        if (const char * problem = call.check(path_length, n_angles)) return call.bad(problem);
        if (!finite_at_least_zero(weight, n_angles, false))
        {
            return call.bad("weights must be finite and >= 0.");
        }
        if (!finite_at_least_zero(temperature, level_count, true))
        {
            return call.bad("temperatures must be finite and > 0.");
        }
        if (edge_temperature != nullptr)
        {
            if (const char * problem = check_edge_temperatures(edge_temperature, level_begin,
                                                               level_count, levels_per_path))
            {
                return call.bad(problem);
            }
        }
        if (up)
        {
            for (int p = 0; p < n_paths; ++p)
            {
                if (!(surface_temperature[p] > 0.) || !std::isfinite(surface_temperature[p]))
                {
                    return call.bad("surface temperatures must be finite and > 0.");
                }
                if (!(surface_emissivity[p] >= 0. && surface_emissivity[p] <= 1.))
                {
                    return call.bad("surface emissivities must lie in [0, 1].");
                }
            }
        }
        PathBands bands;
        if (const char * problem = bands.check(n_bands, band_start, columns))
        {
            return call.bad(problem);
        }
        if (n_bands > 0 && (flux == nullptr || (up && surface_flux == nullptr)))
        {
            return call.bad("band means need flux (and surface_flux on the up sweep).");
        }

        // The surface temperatures and emissivities of the run's paths (0 on the down sweep).
        const PathRun & run = call.run;
        PathTables tables;
        const size_t length_at = tables.add((size_t)level_count*n_angles, path_length);
        const size_t weight_at = tables.add(n_angles, weight);
        const size_t temperature_at = tables.add(level_count, temperature);
        const size_t surface_at = tables.add(2*(size_t)run.paths);
        double * surface = tables.words.data() + surface_at;
        for (int i = 0; i < run.paths && up; ++i)
        {
            surface[i] = surface_temperature[run.first_path + i];
            surface[run.paths + i] = surface_emissivity[run.first_path + i];
        }
        const size_t band_at = tables.add(bands, band_start);
        // After the tables every call has, so that theirs lie where they always lay.
        const bool linear = edge_temperature != nullptr;
        const size_t edge_at = linear ? tables.add(2*(size_t)level_count, edge_temperature) : 0;
        const double * d_tables = call.begin(tables);

        PathFlux a;
        a.beta = beta;
        a.stride = row_stride;
        a.columns = columns;
        a.nu = call.grid->wavenumber.data;
        a.length = d_tables + length_at;
        a.weight = d_tables + weight_at;
        a.temperature = d_tables + temperature_at;
        a.surface_t = d_tables + surface_at;
        a.surface_e = a.surface_t + run.paths;
        a.edge = linear ? d_tables + edge_at : nullptr;
        a.first = level_begin;
        a.count = level_count;
        a.row_base = level_begin;
        a.levels_per_path = levels_per_path;
        a.table_path = run.first_path;
        a.from_last = call.from_last() ? 1 : 0;
        a.up = up ? 1 : 0;
        a.carry = carry;
        a.reflection = reflection;
        a.level_flux = level_flux;
        const bool vector = path_vector(row_stride, {beta, carry, a.nu, reflection, level_flux});
        call.launch([&](const dim3 & launch, int first_path) {
            a.first_path = first_path;
            if (vector)
            {
                launch_flux<true>(n_angles, a, launch, engine->stream);
            }
            else
            {
                launch_flux<false>(n_angles, a, launch, engine->stream);
            }
        });
        call.note_rows(beta, level_count);
        call.note_rows(level_flux, level_count);
        call.note_rows(carry, (long long)n_paths*n_angles);
        call.note_rows(reflection, n_paths);

        if (n_bands > 0)
        {
            const long long * d_bands = reinterpret_cast<const long long *>(d_tables + band_at);
            bands.means(engine, d_bands, level_flux, (long long)row_stride, level_count, false,
                        flux);
            if (up)
            {
                // The surface-interface rows of the paths this run starts in sweep order: upward
                // those whose first level is in the run, downward those whose last level is.
                const PathRows rows = path_rows(level_begin, call.level_end(), levels_per_path,
                                                call.from_last());
                bands.means(engine, d_bands, reflection + (long long)rows.first*row_stride,
                            (long long)row_stride, rows.count, false,
                            surface_flux + (long long)rows.first*n_bands);
            }
        }
        return LBL_OK;
    });
}

int lbl_path_flux(lbl_engine * engine, double * beta, int64_t row_stride, int64_t columns,
                  int32_t grid, int32_t n_paths, int32_t levels_per_path, int32_t level_begin,
                  int32_t level_count, int32_t n_angles, const double * path_length,
                  const double * weight, const double * temperature,
                  const double * surface_temperature, const double * surface_emissivity,
                  int32_t n_bands, const int64_t * band_start, double * carry,
                  double * reflection, double * level_flux, double * flux, double * surface_flux,
                  int32_t flags)
{
    return lbl_path_flux_source(engine, beta, row_stride, columns, grid, n_paths, levels_per_path,
                                level_begin, level_count, n_angles, path_length, weight,
                                temperature, nullptr, surface_temperature, surface_emissivity,
                                n_bands, band_start, carry, reflection, level_flux, flux,
                                surface_flux, flags);
}

}  // extern "C"
